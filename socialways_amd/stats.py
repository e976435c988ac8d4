"""Toy-set mode-coverage statistics of calc_statistics.py: the leave-one-out 1-NN
two-sample test and the per-pedestrian assignment cost ("EMD") between real and generated futures.
The O(K^2 T) distance matrices are computed on the GPU (`sw_traj_dist`), the nearest-neighbour votes
with device reductions; the K x K assignment problems go to scipy's Hungarian solver on the host, as in
the reference (calc_statistics.py:62).

Beyond the reference: `scene_clearance`, the closest approach between the agents of a scene along K joint futures - the
quantity behind the collision rates of `SocialWaysTrainer.evaluate_scenes()`, for trajectories from anywhere - and
`sample_modes`, the greedy score-ordered suppression behind `SocialWaysTrainer.sample_diverse()`, likewise, and
`compose_scenes`, the collision-free choice of one draw per agent behind `SocialWaysTrainer.sample_composed()`, and
`clearance_penalty`, the pairwise clearance penalty and its gradient behind `SocialWaysTrainer.set_clearance_loss()`, and
`plan_risk`, the collision risk of candidate ego paths against the K draws behind `SocialWaysTrainer.plan_risk()`, and
`refine_plans`, the descent that moves such paths away from the draws behind `SocialWaysTrainer.refine_plans()`, and
`path_walls` / `wall_penalty`, the clearance of paths to a static map and the penalty behind `SocialWaysTrainer.set_wall_loss()`."""
import os

import numpy as np
import torch

from . import _lib as L
from . import ops
from .data import WallGrid, check_pred_len


def _dev(x, device):
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x, dtype=torch.float32)
    return t.to(device).contiguous()


def traj_dist(a, b, obsv_len=2, device="cuda"):
    """D[k,i,j] = mean_t ||a[i,k,t] - b[j,k,t]|| over t >= obsv_len; a (Na,nPed,T,2), b (Nb,nPed,T,2)."""
    a, b = _dev(a, device), _dev(b, device)
    L.require_gpu(a)
    Na, nPed, T = a.shape[0], a.shape[1], a.shape[2]
    if b.shape[1:] != a.shape[1:] or a.shape[3] != 2:
        raise ValueError("sample sets must be (N, nPed, T, 2) with equal nPed and T: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    D = torch.empty(nPed, Na, b.shape[0], device=a.device)
    L.call("sw_traj_dist", L.ptr(a), L.ptr(b), Na, b.shape[0], nPed, T, int(obsv_len), L.ptr(D), L.stream())
    return D


def compute_1nn(reals, fakes, obsv_len=2, device="cuda"):
    """calc_statistics.py:7-44 -> np.array([accuracy, real recall, fake recall])."""
    reals, fakes = _dev(reals, device), _dev(fakes, device)
    n_r, n_f, n_ped = reals.shape[0], fakes.shape[0], reals.shape[1]
    D = traj_dist(torch.cat([reals, fakes]), torch.cat([reals, fakes]), obsv_len, device)
    D.diagonal(dim1=1, dim2=2).fill_(1000.0)                     # self-distance = the matrix' initial value
    nn_ind = torch.argmin(D, dim=2)                              # first minimum, like np.argmin
    is_real = torch.arange(n_r + n_f, device=D.device) < n_r
    same = is_real[nn_ind] == is_real[None, :]
    real_pos = int((same & is_real[None, :]).sum())
    fake_pos = int((same & ~is_real[None, :]).sum())
    return np.array([(real_pos + fake_pos) / ((n_r + n_f) * n_ped), real_pos / (n_r * n_ped), fake_pos / (n_f * n_ped)])


def compute_wasserstein(reals, fakes, obsv_len=2, device="cuda"):
    """calc_statistics.py:47-66.  The reference's loop writes every distance to D[ii,jj] AND D[jj,ii]
    of the real x fake matrix, so what reaches the solver is the lower triangle mirrored upwards; kept
    for drop-in parity (requires as many fakes as reals, like the reference's use)."""
    import scipy.optimize as sopt
    reals, fakes = _dev(reals, device), _dev(fakes, device)
    if reals.shape[0] != fakes.shape[0]:
        raise ValueError("compute_wasserstein needs as many generated as real samples (calc_statistics.py:57-60)")
    D = traj_dist(reals, fakes, obsv_len, device)
    C = (torch.tril(D) + torch.tril(D, -1).transpose(1, 2)).double().cpu().numpy()
    cost = 0.0
    for k in range(C.shape[0]):
        r, c = sopt.linear_sum_assignment(C[k])
        cost += C[k][r, c].sum()
    return cost / (reals.shape[0] * reals.shape[1])


def calc_and_store_stats(main_dir, real_samples, n_past=2, n_next=2, stats_file=None, device="cuda", min_ped=6):
    """calc_statistics.py:70-125 without the plotting: for every `<main_dir>/<epoch>/*.npz` written by
    `SocialWaysTrainer.test(write_to_file=...)` (keys obsvs, preds_our) compare the K real samples with
    the first K generated ones; returns ({epoch: 1nn accuracy}, {epoch: EMD}) and writes the reference's
    `stats_1nn` / `stats_wst` arrays (epoch order) to `stats_file` if given.
    real_samples: (K, nPed, n_past+n_next, 2)."""
    real_samples = np.asarray(real_samples, dtype=np.float32)
    K = real_samples.shape[0]
    stats_1nn, stats_wst = {}, {}
    for dirpath, _, filenames in sorted(os.walk(main_dir)):
        cur = os.path.basename(dirpath)
        if not cur.isdigit():
            continue
        s1 = sw = 0.0
        n_files = 0
        for f in sorted(filenames):
            if "npz" not in f:
                continue
            fake = np.load(os.path.join(dirpath, f))
            obsvs, preds = fake["obsvs"], fake["preds_our"]
            n_ped = obsvs.shape[0]
            if n_ped < min_ped:
                continue
            fo = np.broadcast_to(obsvs[None], (K,) + obsvs.shape)
            fake_samples = np.concatenate((fo, preds[:K]), axis=2).astype(np.float32)
            real = real_samples.reshape(K, n_ped, n_past + n_next, 2)
            s1 += compute_1nn(real, fake_samples, n_past, device)[0]
            sw += compute_wasserstein(real, fake_samples, n_past, device)
            n_files += 1
        if n_files:
            stats_1nn[int(cur)], stats_wst[int(cur)] = s1 / n_files, sw / n_files
    if stats_file is not None:
        np.savez(stats_file, stats_1nn=[stats_1nn[k] for k in sorted(stats_1nn)],
                 stats_wst=[stats_wst[k] for k in sorted(stats_wst)])
    return stats_1nn, stats_wst


# ---- the argument front of the public forms below: host data or tensors from anywhere -> device tensors, every check written
# once.  What only this layer knows: what is read on the host (lens, the queries), the default scene of a query, the division by
# scale.  The scalar checks are ops' own (ops.check_*).  The shape checks that ops makes again behind a form stay, because they
# stand in front of the form's require_gpu: on a CPU tensor their ValueError is what the caller gets, and
# tests/test_geometry_args_host.py holds every form to that. -------------------------------------------------------------------
def _trajs_arg(trajs, device, ranks=(4,), empty=False):
    """trajs (K >= 1, B, T, 2 | 4) or - with 3 among `ranks` - (B, T, 2 | 4), x and y first -> (the 4-d tensor on the device, the
    leading axes of what was given); empty: a 3-d input may hold no rows (the scene index refuses it behind this)."""
    t = _dev(trajs, device)
    if t.dim() not in ranks or t.shape[-1] not in (2, 4) or t.shape[-2] < 1 or (t.shape[0] < 1 and not (empty and t.dim() == 3)):
        raise ValueError("trajs must be %s, got %s" % (" or ".join({4: "(K >= 1, B, T, 2 or 4)", 3: "(B, T, 2 or 4)"}[r] for r in ranks),
                                                      tuple(t.shape)))
    return (t if t.dim() == 4 else t.unsqueeze(0)), tuple(t.shape[:-2])


def _start_arg(start, B, device):
    """start (B, 2) or None: a point in front of every path."""
    if start is None:
        return None
    start = _dev(start, device)
    if tuple(start.shape) != (B, 2):
        raise ValueError("start must be (B, 2) = (%d, 2), got %s" % (B, tuple(start.shape)))
    return start


def _lens_arg(lens, B, T, device):
    """lens (B,) or None - list, numpy array or tensor of integers 1 .. T - checked on the host -> int32 on the device."""
    if lens is None:
        return None
    host = lens.cpu().numpy() if isinstance(lens, torch.Tensor) else lens
    return torch.from_numpy(check_pred_len(host, B, T)).to(device)


def _scored_arg(trajs, score, device):
    """trajs (K >= 1, B, T, 2 | 4) and score (K, B) -> both on the device."""
    t, s = _trajs_arg(trajs, device)[0], _dev(score, device)
    if tuple(s.shape) != tuple(t.shape[:2]):
        raise ValueError("score must be (K, B) = (%d, %d), got %s" % (t.shape[0], t.shape[1], tuple(s.shape)))
    return t, s


def _dist_over_scale(dist, scale):
    """dist and scale, both finite and > 0 -> (dist / scale, scale): |scale c| < dist  <=>  |c| < dist / scale."""
    dist, scale = ops.check_penalty_distance(dist, "dist", fp32=False), ops.check_penalty_distance(scale, "scale", fp32=False)
    return dist / scale, scale


def _query_arg(x, Q, name, device):
    """A per-query integer argument (Q,) - list, numpy array or tensor - checked on the host -> int32 on the device."""
    host = np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    if host.shape != (Q,) or host.dtype.kind not in "iu":
        raise ValueError("%s must hold Q = %d integers, got shape %s dtype %s" % (name, Q, host.shape, host.dtype))
    return torch.from_numpy(host.astype(np.int32)).to(device)


def _query_front(trajs, sub_batches, plans, plan_start, start, scene, ego, lens, device):
    """What plan_risk() and refine_plans() share: the draws, the scene index, the plans (Q, P >= 1, T, 2) or (P, T, 2) with their
    start points, and the queries - scene None: query q belongs to scene q, Q = S -> (trajs, start, scenes, K, plans, plan_start,
    scene, ego, lens) as ops.plan_risk() takes them."""
    t = _trajs_arg(trajs, device)[0]
    K, B, T = t.shape[0], t.shape[1], t.shape[2]
    p = _dev(plans, device)
    if p.dim() == 3:
        p = p.unsqueeze(0)
    if p.dim() != 4 or p.shape[1] < 1 or tuple(p.shape[2:]) != (T, 2):
        raise ValueError("plans must be (Q, P >= 1, T, 2) or (P, T, 2) with T = %d, got %s" % (T, tuple(p.shape)))
    Q = p.shape[0]
    start = _start_arg(start, B, device)
    if plan_start is not None:
        plan_start = _dev(plan_start, device)
        if tuple(plan_start.shape) != (Q, 2):
            raise ValueError("plan_start must be (Q, 2) = (%d, 2), got %s" % (Q, tuple(plan_start.shape)))
    scenes = ops.SceneIndex.get(sub_batches, B, t.device)
    if scene is None:
        if Q != scenes.S:
            raise ValueError("without `scene` query q belongs to scene q: plans hold Q = %d queries, there are %d scenes" % (Q, scenes.S))
        scene = np.arange(Q)
    scene = _query_arg(scene, Q, "scene", t.device)
    ego = _query_arg(ego, Q, "ego", t.device) if ego is not None else None
    return t, start, scenes, K, p, plan_start, scene, ego, _lens_arg(lens, B, T, t.device)


def scene_clearance(trajs, sub_batches, start=None, scale=1.0, device="cuda"):
    """Closest approach of every agent to the other agents of its scene, per joint draw (`sw_scene_clearance`).
    trajs (K, B, T, 2 | 4) or (B, T, 2 | 4): K joint futures of B agents, x and y first (prediction files, `collect`
    records, ground truth); sub_batches (S, 2) [start, end) rows tiling [0, B), [] = one scene; start (B, 2) or None: a
    point in front of every path (the last observed position), giving T segments instead of T - 1.  Within a segment
    both agents move linearly, so two agents that swap places between two frames have clearance 0.  The distance is
    multiplied by `scale`.  Returns a device tensor (K, B), or (B,) for a 3-d input; +inf in single-agent scenes."""
    return scene_clearance_len(trajs, sub_batches, None, start, scale, device)


def scene_clearance_len(trajs, sub_batches, lens, start=None, scale=1.0, device="cuda"):
    """scene_clearance() for futures of different lengths (`sw_scene_clearance_len`): lens (B,) - list, numpy array or
    tensor of integers 1 .. T - gives the frames agent a is present for, left-aligned in trajs (what lies behind them is
    padding and reaches no output).  A collision needs both agents present: the segment of a pair that ends at frame t counts
    only if t < min(lens[a], lens[b]).  An agent for which no segment counts has clearance +inf.  Everything else as
    scene_clearance(), which is this call with lens None."""
    t, lead = _trajs_arg(trajs, device, (4, 3), empty=True)
    K, B, T = t.shape[0], t.shape[1], t.shape[2]
    lens = _lens_arg(lens, B, T, t.device)
    start = _start_arg(start, B, device)
    L.require_gpu(t)
    return ops.scene_clearance(t, start, ops.SceneIndex.get(sub_batches, B, t.device), K, float(scale), lens=lens).reshape(lead)


def clearance_penalty(trajs, sub_batches, dist, start=None, scale=1.0, device="cuda"):
    """The scene-clearance penalty SocialWaysTrainer.set_clearance_loss() trains against, for trajectories from anywhere
    (`sw_clearance_grad`): per pair of agents of a scene and per segment, max(0, 1 - (scale |c|)^2 / dist^2)^2 with c the
    closest approach of scene_clearance() - both agents moving linearly within the segment.  trajs (B, T, 2 | 4), x and y
    first; sub_batches (S, 2) [start, end) rows tiling [0, B), [] = one scene; start (B, 2) or None: a point in front of
    every path (the last observed position; it takes no gradient), giving T segments instead of T - 1.  `scale` converts
    trajs to the units of `dist`, as in scene_clearance().  Returns device tensors (loss (B,), grad (B, T, 2), count (B,)
    int32): the agent's share of the penalty (loss.sum() = the sum over pairs and segments), its gradient with respect to
    trajs[..., :2] in the units of trajs, and the agent's number of (partner, segment)s closer than dist."""
    t = _trajs_arg(trajs, device, (3,), empty=True)[0].squeeze(0)
    B, T = t.shape[0], t.shape[1]
    d0, _ = _dist_over_scale(dist, scale)
    start = _start_arg(start, B, device)
    L.require_gpu(t)
    grad = torch.zeros(B, T, 2, device=t.device)
    loss = torch.zeros(B, device=t.device)
    count = torch.zeros(B, dtype=torch.int32, device=t.device)
    scenes = ops.SceneIndex.get(sub_batches, B, t.device)
    ops.clearance_grad(t, start, scenes, d0, 1.0, grad, loss, count)
    return loss, grad, count


def sample_modes(trajs, score, radius, top_m, metric="fde", sub_batches=None, scale=1.0, device="cuda"):
    """The modes among K scored futures (`sw_sample_nms`), for trajectories and scores from anywhere: the highest-scored
    draw is kept, every draw within `radius` of it is counted to its mode, then the highest-scored of the rest, top_m times
    at most.  trajs (K, B, T, 2 | 4), x and y first; score (K, B), higher = better; the distance between two draws is `scale`
    times the Euclidean distance at the last step (metric "fde") or its mean over the T steps ("ade").  sub_batches None:
    every agent on its own; (S, 2) [start, end) rows tiling [0, B), [] = one scene: per scene, draw k of a scene being
    draw k of each of its agents - one mode only if every agent is within the radius, scored as the lowest-scored agent.
    Returns device tensors over the G = B or S groups: order (G, top_m) int32 (the kept draws, best first, -1 past count),
    count (G,) int32, weight (G, top_m) (the share of the K draws in each mode, rows sum to 1), assign (G, K) int32 (the
    mode of every draw)."""
    t, s = _scored_arg(trajs, score, device)
    K, B = s.shape
    L.require_gpu(t)
    scenes = ops.SceneIndex.get(sub_batches, B, t.device) if sub_batches is not None else None
    return ops.sample_nms(t, s, K, int(top_m), radius, metric, scenes, inv_ss=float(scale))[:4]


def compose_scenes(trajs, score, sub_batches, coll_dist, start=None, scale=1.0, sweeps=8, lens=None, device="cuda"):
    """One draw per agent, per scene, so that no two chosen paths come closer than coll_dist (`sw_scene_compose`), for
    trajectories and scores from anywhere.  trajs (K, B, T, 2 | 4), x and y first: K futures per agent, drawn independently
    per agent given what was observed - then every tuple of per-agent draws is a joint future; score (K, B), higher = better;
    sub_batches (S, 2) [start, end) rows tiling [0, B), [] = one scene; start (B, 2) or None: a point in front of every path, as
    scene_clearance(); distances are multiplied by `scale`; lens (B,) or None: the frames every agent is present for, as
    scene_clearance_len().  Every agent starts on its highest-scored draw; in up to `sweeps` sweeps over a scene's agents one
    that conflicts with another's chosen path moves to the draw with the fewest conflicts (the highest score among equals) if
    that is fewer than it has.  Returns device tensors: sel (B,) int32 the chosen draws, sel0 (B,) int32 the highest-scored
    ones, clear (B,) the closest approach of each chosen path to the others of its scene (+inf alone), per_scene (S, 4) int32 =
    conflicting pairs before | after | agents moved | sweeps that changed something."""
    t, s = _scored_arg(trajs, score, device)
    K, B = s.shape
    start = _start_arg(start, B, device)
    lens = _lens_arg(lens, B, t.shape[2], t.device)
    L.require_gpu(t)
    scenes = ops.SceneIndex.get(sub_batches, B, t.device)
    return ops.scene_compose(t, start, s, scenes, K, coll_dist, float(scale), int(sweeps), lens=lens)[:4]


def plan_risk(trajs, sub_batches, plans, coll_dist, plan_start=None, start=None, scene=None, ego=None, scale=1.0, lens=None,
              plan_lens=None, device="cuda"):
    """How likely is a candidate ego path to run into somebody (`sw_plan_risk`), for trajectories from anywhere.  trajs
    (K, B, T, 2 | 4), x and y first: K futures per agent, drawn independently per agent given what was observed; sub_batches
    (S, 2) [start, end) rows tiling [0, B), [] = one scene.  plans (Q, P, T, 2), or (P, T, 2) for one query: P candidate paths
    per query - paths that are not among the draws.  Query q looks at scene scene[q] (None: query q belongs to scene q, Q = S)
    and leaves out row ego[q] (None or -1: nobody; an absolute row of trajs - the ego's own draws, when the ego is an agent of
    the scene so that the social block saw its observed track).  start (B, 2) and plan_start (Q, 2), both or neither: a point
    in front of every path and every plan (the last observed positions), giving T segments instead of T - 1.  Distances are
    multiplied by `scale`; a conflict is a closest approach below coll_dist, both moving linearly within a segment.  lens (B,)
    / plan_lens (Q,) or None: the frames an agent / the plans of a query are present for, as scene_clearance_len().
    The draws are OPEN-LOOP: the pedestrians do not react to the plan.
    Returns device tensors (risk (Q, P): 1 - the product over the other agents of the share of their draws that stay clear;
    clear_min (Q, P): the closest approach to any draw; counts (Q, P, 4) int32: draws k with a conflict of some agent's draw k |
    frame of the earliest conflict, -1 | the row with the most conflicting draws, -1 | its number of them)."""
    ops.check_distance("coll_dist", coll_dist)
    ops.check_positive("scale", scale)
    if (start is None) != (plan_start is None):
        raise ValueError("start and plan_start go together: a point in front of the paths and of the plans, or of neither")
    t, start, scenes, K, p, plan_start, scene, ego, lens = _query_front(trajs, sub_batches, plans, plan_start, start, scene, ego, lens,
                                                                        device)
    plan_lens = _lens_arg(plan_lens, p.shape[0], t.shape[2], t.device)
    L.require_gpu(t)
    return ops.plan_risk(t, start, scenes, K, p, plan_start, scene, ego, coll_dist, float(scale), lens=lens, plan_lens=plan_lens)


def path_walls(trajs, walls, dist, start=None, scale=1.0, lens=None, device="cuda"):
    """How close do paths come to the static map (`sw_path_walls`), for trajectories from anywhere: trajs (K, B, T, 2 | 4) or
    (B, T, 2 | 4), x and y first - draws, true futures or plans; walls (M, 2, 2): line segments [w0, w1] in the units of trajs, a
    zero-length one being a post, M = 0 .. 1024 - or a WallGrid of any size (then `sw_path_walls_grid`, and clear is +inf beyond
    the grid's reach); start (B, 2) or None: a point in front of every path, giving T segments
    instead of T - 1; distances are multiplied by `scale`; lens (B,) or None: the frames every agent is present for, as
    scene_clearance_len().  Within a segment the path point moves linearly and the wall stands still.
    Returns device tensors shaped like the leading axes of trajs: clear - the smallest distance to any wall, +inf without
    walls; first int32 - the frame at which the first segment closer than dist ends, -1 without; nseg int32 - the (segment,
    wall) pairs closer than dist."""
    ops.check_distance("dist", dist)
    ops.check_positive("scale", scale)
    t, lead = _trajs_arg(trajs, device, (4, 3))
    K, B, T = t.shape[0], t.shape[1], t.shape[2]
    w = ops.walls_arg(walls, device)
    if isinstance(w, WallGrid):
        ops.check_wall_grid_arg(w, t.device, float(np.float32(dist)) / float(np.float32(scale)), "dist / scale")
    start = _start_arg(start, B, device)
    lens = _lens_arg(lens, B, T, t.device)
    L.require_gpu(t)
    return tuple(o.reshape(lead) for o in ops.path_walls(t, start, K, w, dist, float(scale), lens=lens))


def wall_penalty(trajs, walls, dist, start=None, scale=1.0, lens=None, device="cuda"):
    """The wall penalty SocialWaysTrainer.set_wall_loss() trains against, for trajectories from anywhere (`sw_wall_grad`): per
    segment of a path and per wall, max(0, 1 - (scale |c|)^2 / dist^2)^2 with c the closest approach of path_walls() - the
    path point moving linearly within the segment, the wall standing still.  trajs (K, B, T, 2 | 4) or (B, T, 2 | 4), x and y
    first - the K draws, true futures or plans; walls (M, 2, 2) as path_walls(), M = 0 .. 1024, or a WallGrid; start (B, 2) or None: a point in
    front of every path (the last observed position; it takes no gradient), giving T segments instead of T - 1; `scale`
    converts trajs to the units of `dist`, as in clearance_penalty(); lens (B,) or None: the frames every agent is present
    for, as path_walls().  Returns device tensors (loss, grad, count): loss and count (int32) shaped like the leading axes of
    trajs - the path's penalty (no 1/2: a path owns its pairs alone) and its number of (segment, wall)s closer than dist - and
    grad (.., T, 2): the gradient of loss.sum() with respect to trajs[..., :2] in the units of trajs, exactly 0 where a path
    crosses a wall."""
    dw, _ = _dist_over_scale(dist, scale)
    t, lead = _trajs_arg(trajs, device, (4, 3))
    K, B, T = t.shape[0], t.shape[1], t.shape[2]
    w = ops.walls_arg(walls, device)
    if isinstance(w, WallGrid):
        ops.check_wall_grid_arg(w, t.device, float(np.float32(dw)), "dist / scale")
    start = _start_arg(start, B, device)
    lens = _lens_arg(lens, B, T, t.device)
    L.require_gpu(t)
    grad = torch.zeros(K, B, T, 2, device=t.device)
    loss = torch.zeros(K, B, device=t.device)
    count = torch.zeros(K, B, dtype=torch.int32, device=t.device)
    ops.wall_grad(t, start, K, w, dw, 1.0, grad, loss, count, lens=lens)
    return loss.reshape(lead), grad.reshape(lead + (T, 2)), count.reshape(lead)


def refine_plans(trajs, sub_batches, plans, dist, plan_start, start, scene=None, ego=None, scale=1.0, lens=None, device="cuda",
                 walls=None, wall_dist=None, w_wall=1.0, **descent):
    """The nearest paths that stay clear of the sampled futures (`sw_plan_refine`), for trajectories from anywhere: every plan
    is moved by n_iter steps of gradient descent, in one launch, on the expected clearance penalty against the K draws - the
    penalty of clearance_penalty() at distance `dist`, averaged over each agent's draws - plus a term that keeps it near the
    original and one that keeps it smooth.  trajs, sub_batches, plans, scene, ego, scale, lens as plan_risk(); start (B, 2)
    and plan_start (Q, 2) are REQUIRED: the point in front of every path and of every plan, which does not move.  `dist` is in
    the units of scale * trajs, like the coll_dist of plan_risk().  descent: n_iter=32, lr=0.1, w_track=0.05, w_smooth=0.5,
    max_move=0.5 (dimensionless; no waypoint moves further than max_move * dist per iteration; lr (2 w_track + 32 w_smooth) < 2).
    The draws are OPEN-LOOP: the pedestrians do not react to the plan.
    Returns device tensors (refined (Q, P, T, 2) in the units of trajs; cost (Q, P, 2, 3): before | after x expected penalty |
    sum |x - x0|^2 / dist^2 | sum |x_{t+1} - 2 x_t + x_{t-1}|^2 / dist^2, unweighted; moved (Q, P): the largest displacement of a
    waypoint, times scale).
    walls (M, 2, 2) as path_walls(): the same launch also descends w_wall * the penalty of the plan's own segments against the
    walls at the distance wall_dist (default dist; in the units of scale * trajs) - `sw_plan_refine_walls` - and cost is
    (Q, P, 2, 4), the unweighted wall penalty last.  Where a plan CROSSES a wall the gradient is exactly 0: descent cannot undo a
    crossing; path_walls() reports it."""
    d0, scale = _dist_over_scale(dist, scale)
    ops.refuse_wall_grid(walls, "refine_plans")
    wall = {}
    if walls is not None:
        wall = dict(walls=ops.walls_arg(walls, device), wall_d0=d0 if wall_dist is None else float(wall_dist) / scale, w_wall=w_wall)
    ops.check_descent(d0, **{k: v for k, v in wall.items() if k != "walls"}, **descent)
    if start is None or plan_start is None:
        raise ValueError("refine_plans needs start (B, 2) and plan_start (Q, 2): the points in front of the paths and of the plans")
    t, start, scenes, K, p, plan_start, scene, ego, lens = _query_front(trajs, sub_batches, plans, plan_start, start, scene, ego, lens,
                                                                        device)
    L.require_gpu(t)
    return ops.plan_refine(t, start, scenes, K, p, plan_start, scene, ego, d0, scale, lens=lens, **wall, **descent)
