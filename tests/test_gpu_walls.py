"""Walls on the device: sw_path_walls and sw_plan_refine_walls on constructed cases against the numpy reference written from
the header comment (tests/_walls_ref.py), bit-for-bit properties, the parallel corridor where candidates tie, the corridor
scenario, and the layers above - stats.path_walls, stats.refine_plans(walls=), trainer.refine_plans(walls=).
Bounds.  sw_path_walls: first and nseg EXACTLY the reference's (tests/test_walls_host.py asserts that no distance of a case
lies within a relative 1e-4 of dist); clear within max(4 d32, c 2^-24 M) inv_ss, d32 = the largest difference between the
float32 and the float64 run of the REFERENCE on that case (computed here on the CPU, never from the kernel), M the largest
coordinate, c = 40: a distance takes 17 roundings - the two differences a = p - w0 and f, the dot product a.f and |f|^2 (three
each), the reciprocal, u, u f, the subtraction, |c|^2 (three), the square root and the product with inv_ss - on quantities of
magnitude up to 2 M (differences of coordinates), each of which moves the distance by at most 2 2^-24 M: 34, rounded up.
One refinement iteration (n_iter = 1, no cap): the gradient (X0 - out) / (lr d0^2) and all four cost columns within GRAD_REL
(2e-5) of the largest float64 entry.  32 iterations: max(4 d32, 2 N 2^-24 M) as tests/test_gpu_refine.py.
Observed on an MI355X (pytest -s): clear max|err| up to 1.9e-6 (r257_tp12_m1; d32 2.2e-6, bound 8.2e-5);
one iteration, gradient max|err| / max|ref| up to 1.6e-6 (sizes_k20_ps4_p5_m130_long), costs up to 3.6e-7, the wall column within
2.8e-5 of 28.1; 32 iterations, out max|err| at most 8.6e-6 (sizes_k20_ps4_p5_m130; d32 8.6e-6) against bounds of 2e-5 .. 3e-4,
the smallest margin k260_n3_m1: 2.2e-6 against 2.0e-5 (d32 1.1e-6); the parallel corridor: the sum of the step (-8.3e-7, -4.5)
against (0, -4.5)."""
import functools

import numpy as np
import pytest
import torch

import _refine_ref as R
import _walls_ref as W
from _ref64 import GRAD_REL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATHS = dict(W.path_cases())
REFINE = dict(W.refine_cases())
ONE = dict(n_iter=1, lr=1.0, w_track=0.05, w_smooth=0.02, max_move=1e6)      # tests/test_gpu_refine.py's
C_ROUNDINGS = 40


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def scene_list(sizes):
    o = np.concatenate([[0], np.cumsum(sizes)])
    return np.stack([o[:-1], o[1:]], axis=1).astype(np.int64)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def run_paths(case, **kw):
    from socialways_amd import ops
    c = dict(case, **kw)
    out = ops.path_walls(dev(c["pos"]), dev(c["start"]), c["K"], dev(c["walls"]), c["dist"], c["inv_ss"], lens=dev(c["lens"]))
    torch.cuda.synchronize()
    return out


def run_refine(case, walls="case", **descent):
    from socialways_amd import ops
    pos = dev(case["pos"])
    scenes = ops.SceneIndex.get(scene_list(case["sizes"]), pos.shape[1], pos.device)
    wall = {} if walls is None else dict(walls=dev(case["walls"] if isinstance(walls, str) else walls), wall_d0=case["wall_d0"],
                                         w_wall=case["w_wall"])
    out = ops.plan_refine(pos, dev(case["start"]), scenes, case["K"], dev(case["plans"]), dev(case["plan_start"]), dev(case["q_scene"]),
                          dev(case["q_ego"]), case["d0"], case["inv_ss"], lens=dev(case["lens"]), **wall, **descent)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def path_reference(name, dtype):
    return W.run_path_reference(PATHS[name], dtype)


@functools.lru_cache(maxsize=None)
def refine_reference(name, dtype, one):
    return W.run_refine_reference(REFINE[name], dtype=dtype, **(ONE if one else {}))


def largest(case):
    return float(max(np.nanmax(np.abs(case["pos"][..., :2])), np.abs(case["plans"]).max(), np.abs(case["start"]).max(),
                     np.abs(case["plan_start"]).max(), np.abs(case["walls"]).max(initial=0.0)))


# ---- sw_path_walls against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PATHS))
def test_path_walls(name):
    case, w64, w32 = PATHS[name], path_reference(name, np.float64), path_reference(name, np.float32)
    clear, first, nseg = (t.cpu().numpy() for t in run_paths(case))
    K, B = case["K"], case["B"]
    assert clear.shape == first.shape == nseg.shape == (K, B) and first.dtype == nseg.dtype == np.int32
    assert np.array_equal(first, w64["first"]) and np.array_equal(nseg, w64["nseg"])
    fin = np.isfinite(w64["clear"])
    assert np.array_equal(np.isfinite(clear), fin) and (clear[~fin] == np.inf).all()
    M = float(max(np.nanmax(np.abs(case["pos"][..., :2])), np.abs(case["walls"]).max(initial=0.0),
                  0.0 if case["start"] is None else np.abs(case["start"]).max()))
    d32 = float(np.abs(w32["clear"][fin].astype(np.float64) - w64["clear"][fin]).max(initial=0.0))
    bound = max(4 * d32, C_ROUNDINGS * 2.0 ** -24 * M * case["inv_ss"])
    err = float(np.abs(clear[fin].astype(np.float64) - w64["clear"][fin]).max(initial=0.0))
    print("%s: clear max|fp32 kernel - float64| %.3g, reference fp32 - float64 %.3g, M %.3g, bound %.3g; %d pairs closer than dist, "
          "%d paths at distance 0" % (name, err, d32, M, bound, nseg.sum(), (w64["clear"] == 0).sum()))
    assert err <= bound
    assert same(run_paths(case), [dev(clear), dev(first), dev(nseg)]), "two calls give the same bits"


def test_path_walls_shapes_and_limits():
    from socialways_amd import ops, _lib as L
    case = PATHS["r64_tp17_m33_start"]
    K, B = case["K"], case["B"]
    flat = ops.path_walls(dev(case["pos"]).reshape(K * B, case["Tp"], -1), dev(case["start"]), K, dev(case["walls"]), case["dist"], case["inv_ss"])
    assert same(flat, run_paths(case))
    wide_start = torch.zeros(B, 5, device=DEV)                   # a strided start, read in place
    wide_start[:, :2] = dev(case["start"])
    assert same(ops.path_walls(dev(case["pos"]), wide_start[:, :3], K, dev(case["walls"]), case["dist"], case["inv_ss"]), flat)
    clear, first, nseg = run_paths(case, walls=np.zeros((0, 2, 2), np.float32))
    assert bool(torch.isinf(clear).all()) and bool((first == -1).all()) and not bool(nseg.any())
    assert W.WALLS_MAX == L.WALLS_MAX
    with pytest.raises(ValueError):
        run_paths(case, walls=np.zeros((L.WALLS_MAX + 1, 2, 2), np.float32))
    none = ops.path_walls(torch.zeros(3, 0, 4, 2, device=DEV), None, 3, dev(case["walls"]), 0.5)
    assert none[0].shape == (3, 0)
    # dist = 0 admits no conflict; a huge one counts every counted pair
    clear0, first0, nseg0 = run_paths(case, dist=0.0)
    assert same([clear0], [flat[0]]), "the clearance does not depend on dist"
    assert bool((first0 == -1).all()) and not bool(nseg0.any())
    _, first1, nseg1 = run_paths(case, dist=1e9)
    assert bool((first1 == 0).all()) and bool((nseg1 == case["Tp"] * case["M"]).all())


def test_path_walls_padding_reaches_nothing():
    case = PATHS["r65_tp33_m33_ragged"]
    a = run_paths(case)
    pos = case["pos"].copy()
    pos[np.isnan(pos)] = 1e30                                    # other garbage behind the lengths changes nothing
    assert same(a, run_paths(case, pos=pos)) and not bool(torch.isnan(a[0]).any())      # +inf: an agent seen for one frame, no start point
    walls = case["walls"].copy()
    walls[5] = walls[5, ::-1].copy()                             # a wall turned round is the same wall: the same distances
    b = run_paths(case, walls=walls)
    inf = torch.isinf(a[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(inf, torch.isinf(b[0]))
    assert float((a[0] - b[0])[~inf].abs().max()) <= 1e-5


# ---- sw_plan_refine_walls against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(REFINE))
def test_one_iteration_is_the_gradient(name):
    case, want = REFINE[name], refine_reference(name, np.float64, True)
    out, cost, moved = (t.cpu().numpy().astype(np.float64) for t in run_refine(case, **ONE))
    Q, P = case["plans"].shape[:2]
    assert out.shape == (Q, P, case["Tp"], 2) and cost.shape == (Q, P, 2, 4) and moved.shape == (Q, P)
    d02 = float(case["d0"]) ** 2
    grad = (case["plans"].astype(np.float64) - out) / (ONE["lr"] * d02)
    ref = want["step0"] / d02
    eg, ec = np.abs(grad - ref).max(), np.abs(cost - want["cost"]).max()
    print("%s: gradient max|err| %.3g of max|ref| %.3g (%.3g), cost max|err| %.3g of %.3g (%.3g), wall column %.3g of %.3g; bound %.1g; tie gap %.3g"
          % (name, eg, np.abs(ref).max(), eg / np.abs(ref).max(), ec, np.abs(want["cost"]).max(), ec / np.abs(want["cost"]).max(),
             np.abs(cost[..., 3] - want["cost"][..., 3]).max(), np.abs(want["cost"][..., 3]).max(), GRAD_REL, want["gap"]))
    assert np.isfinite(out).all() and np.isfinite(cost).all() and (want["cost"][..., 0, 3] > 0).any()
    assert eg <= GRAD_REL * np.abs(ref).max()
    assert ec <= GRAD_REL * np.abs(want["cost"]).max()
    assert np.abs(moved - want["moved"]).max() <= GRAD_REL * max(want["moved"].max(), 1e-30) + 2.0 ** -23 * largest(case) * case["inv_ss"]


@pytest.mark.parametrize("name", list(REFINE))
def test_32_iterations(name):
    case, w64, w32 = REFINE[name], refine_reference(name, np.float64, False), refine_reference(name, np.float32, False)
    N, M = 32, largest(case)
    d32 = float(np.abs(w32["out"].astype(np.float64) - w64["out"]).max())
    bound = max(4 * d32, 2 * N * 2.0 ** -24 * M)
    out, cost, moved = (t.cpu().numpy().astype(np.float64) for t in run_refine(case))
    err = np.abs(out - w64["out"]).max()
    print("%s: out max|fp32 kernel - float64| %.3g, reference fp32 - float64 %.3g, M %.3g, bound %.3g; cost max|err| %.3g of %.3g"
          % (name, err, d32, M, bound, np.abs(cost - w64["cost"]).max(), np.abs(w64["cost"]).max()))
    assert np.isfinite(out).all() and err <= bound
    assert np.array_equal(cost[..., 0, 1], np.zeros_like(cost[..., 0, 1])), "the original plan has not moved"


# ---- bit for bit -----------------------------------------------------------------------------------------------------------
def test_without_walls_and_with_none_of_them():
    from socialways_amd import ops
    for name in ("sizes_k20_ps4_p5", "k65_tp33_ragged_half", "queries", "tp1"):
        case = dict(dict(R.constructed_cases())[name], wall_d0=0.3, w_wall=2.0)
        pos = dev(case["pos"])
        scenes = ops.SceneIndex.get(scene_list(case["sizes"]), pos.shape[1], pos.device)
        plain = ops.plan_refine(pos, dev(case["start"]), scenes, case["K"], dev(case["plans"]), dev(case["plan_start"]), dev(case["q_scene"]),
                                dev(case["q_ego"]), case["d0"], case["inv_ss"], lens=dev(case["lens"]))
        none = run_refine(case, walls=None)
        assert none[1].shape[-1] == 3 and same(plain, none), "walls=None is ops.plan_refine"
        empty = run_refine(case, walls=np.zeros((0, 2, 2), np.float32))
        assert empty[1].shape[-1] == 4 and not bool(empty[1][..., 3].any())
        assert same((plain[0], plain[2], plain[1]), (empty[0], empty[2], empty[1][..., :3]))
        far = run_refine(case, walls=np.full((5, 2, 2), 1e4, np.float32))      # walls nobody comes near: the same bits again
        assert same(empty, far)


def test_two_calls_a_plan_alone_and_no_iteration():
    case = REFINE["sizes_k20_ps4_p5_m130"]
    full = run_refine(case)
    assert same(full, run_refine(case))
    for p in (0, 3):
        alone = run_refine(dict(case, plans=np.ascontiguousarray(case["plans"][:, p:p + 1])))
        assert same([t[:, p:p + 1] for t in full], alone)
    out, cost, moved = run_refine(case, n_iter=0)
    assert torch.equal(bits(out), bits(dev(case["plans"]))) and not bool(moved.any())
    assert torch.equal(bits(cost[:, :, 0]), bits(cost[:, :, 1])) and bool((cost[..., 0, 3] > 0).any())
    assert torch.equal(bits(full[1][:, :, 0]), bits(cost[:, :, 0])), "the costs of the original do not depend on n_iter"


def test_the_egos_draws_and_the_padding_reach_nothing():
    case = REFINE["queries_m130"]
    base = run_refine(case)
    off = np.concatenate([[0], np.cumsum(case["sizes"])])
    seen = 0
    for i, (sc, e) in enumerate(zip(case["q_scene"], case["q_ego"])):      # one query at a time: its ego's draws are NaN
        if not (0 <= sc < len(case["sizes"]) and off[sc] <= e < off[sc + 1]):
            continue
        pos = case["pos"].copy()
        pos[:, e] = np.nan
        got = run_refine(dict(case, pos=pos))
        assert same([t[i:i + 1] for t in base], [t[i:i + 1] for t in got]) and bool(torch.isfinite(got[0][i]).all())
        seen += 1
    assert seen >= 3
    ragged = REFINE["k65_tp17_ragged_x2_m130"]
    a = run_refine(ragged)
    pos = ragged["pos"].copy()
    pos[np.isnan(pos)] = 1e30
    assert same(a, run_refine(dict(ragged, pos=pos))) and all(bool(torch.isfinite(t).all()) for t in a)


# ---- ties ----------------------------------------------------------------------------------------------------------------------
def test_the_parallel_corridor():
    """Every segment but the first ties between its two ends: which end takes the gradient is the order's business, the
    penalties, the clearance and the sum of each segment's two shares are not."""
    case = W.parallel_case()
    par = dict(n_iter=1, lr=1.0, w_track=0.0, w_smooth=0.0, max_move=1e6)
    want = W.run_refine_reference(case, **par)
    out, cost, _ = (t.cpu().numpy().astype(np.float64) for t in run_refine(case, **par))
    step = case["plans"].astype(np.float64) - out                # lr = 1: the step itself
    print("parallel corridor: sum of the step %s against %s, wall penalty %.6g against %.6g"
          % (step[0, 0].sum(0), want["step0"][0, 0].sum(0), cost[0, 0, 0, 3], want["cost"][0, 0, 0, 3]))
    assert want["cost"][0, 0, 0, 3] > 1 and np.abs(want["step0"][0, 0].sum(0)).max() > 1
    assert np.abs(step[0, 0].sum(0) - want["step0"][0, 0].sum(0)).max() <= GRAD_REL * np.abs(want["step0"]).max()
    assert np.abs(cost[0, 0, 0] - want["cost"][0, 0, 0]).max() <= GRAD_REL * np.abs(want["cost"]).max()
    plan = np.ascontiguousarray(case["plans"][0])
    clear, first, nseg = run_paths(dict(K=1, pos=plan, start=case["plan_start"], walls=case["walls"], dist=0.3, inv_ss=1.0, lens=None))
    assert float(clear[0, 0]) == 0.25 and int(first[0, 0]) == 0 and int(nseg[0, 0]) == case["Tp"]


# ---- behaviour, and the public forms ---------------------------------------------------------------------------------------------
def test_the_corridor_through_stats():
    from socialways_amd import stats
    case, C = W.corridor_case(), W.CORRIDOR
    args = (case["pos"], scene_list(case["sizes"]), case["plans"], C["dist"], case["plan_start"], case["start"])
    plain = stats.refine_plans(*args)
    walled = stats.refine_plans(*args, walls=case["walls"], w_wall=C["w_wall"])
    assert plain[1].shape == (1, 1, 2, 3) and walled[1].shape == (1, 1, 2, 4)
    both = torch.cat([plain[0][0], walled[0][0]], 0)             # (2, Tp, 2): the two refined plans as two paths
    clear, first, nseg = stats.path_walls(both, case["walls"].reshape(-1, 4), C["coll_dist"], start=np.repeat(case["plan_start"], 2, 0))
    print("corridor: plan-to-wall clearance %.3f without walls, %.3f with; pedestrian penalty %.3f -> %.3f"
          % (float(clear[0]), float(clear[1]), float(walled[1][0, 0, 0, 0]), float(walled[1][0, 0, 1, 0])))
    assert clear.shape == (2,) and float(clear[0]) < C["coll_dist"] < float(clear[1])
    assert int(first[0]) >= 0 and int(nseg[0]) > 0 and int(first[1]) == -1 and int(nseg[1]) == 0
    assert float(walled[1][0, 0, 1, 0]) < float(walled[1][0, 0, 0, 0])


def test_stats_are_the_public_forms():
    from socialways_amd import stats
    name = "k65_tp17_ragged_x2_m130"
    case = REFINE[name]
    want = run_refine(case, n_iter=5)
    got = stats.refine_plans(case["pos"], scene_list(case["sizes"]), case["plans"], R.D0_WORLD, case["plan_start"], case["start"],
                             ego=case["q_ego"], scale=case["inv_ss"], lens=case["lens"], n_iter=5, walls=case["walls"],
                             wall_dist=W.DW_WORLD, w_wall=case["w_wall"])
    assert len(got) == 3 and same(got, want)
    pc = PATHS["r65_tp33_m33_ragged"]
    assert same(stats.path_walls(pc["pos"], pc["walls"], pc["dist"], scale=pc["inv_ss"], lens=pc["lens"]), run_paths(pc))
    one = stats.path_walls(pc["pos"][0], pc["walls"].reshape(-1, 4), pc["dist"], scale=pc["inv_ss"], lens=pc["lens"])
    assert one[0].shape == (pc["B"],) and same(one, [t[0] for t in run_paths(pc)])


# ---- the trainer -----------------------------------------------------------------------------------------------------------
def test_trainer_refine_plans_is_sample_refine_risk_and_walls():
    import socialways_amd as sw
    from socialways_amd import ops
    from test_gpu_sample import crowd, SIZES
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    obsv, _, sb = crowd(SIZES)
    K, B = 20, obsv.shape[0]
    noise = torch.rand(K, B, 32, device=DEV)
    draws = tr.G.sample(obsv, K, 12, sb, noise)
    egos = np.array([int(a) + int(b - a) // 2 for a, b in np.asarray(sb)])
    plans = sw.predict_cv(obsv, 12)[egos][:, None, :, :2].repeat(1, 2, 1, 1)
    plans[:, 1] += 0.01
    rng = np.random.RandomState(5)
    at = plans[:, 0, 6].cpu().numpy()                            # walls beside the plans' middles, in the coordinates of obsv
    walls = np.stack([at + rng.uniform(-0.03, 0.03, at.shape), at + rng.uniform(-0.03, 0.03, at.shape)], 1).astype(np.float32)
    kw = dict(coll_dist=0.05, sub_batches=sb, ego=egos, noise=noise, scale=2.0, n_iter=8)
    refined, risk, cost, moved, trajs = tr.refine_plans(obsv, plans, K, 0.1, walls=walls, wall_dist=0.08, w_wall=2.0, **kw)
    assert torch.equal(trajs, draws) and refined.shape == plans.shape and risk.shape == (len(egos), 2, 2) and cost.shape == (len(egos), 2, 2, 4)
    scenes = ops.SceneIndex.get(np.asarray(sb, dtype=np.int64), B, obsv.device)
    q_scene = torch.arange(len(egos), dtype=torch.int32, device=DEV)
    q_ego = torch.from_numpy(egos.astype(np.int32)).to(DEV)
    pstart = obsv[q_ego.long(), -1]
    want = ops.plan_refine(draws, obsv[:, -1], scenes, K, plans, pstart, q_scene, q_ego, 0.05, 2.0, n_iter=8, walls=dev(walls),
                           wall_d0=0.04, w_wall=2.0)
    assert same((refined, cost, moved), want) and bool((cost[..., 0, 3] > 0).any())
    after = ops.plan_risk(draws, obsv[:, -1], scenes, K, refined, pstart, q_scene, q_ego, 0.05, 2.0)[0]
    assert torch.equal(bits(risk[..., 1]), bits(after))
    clear, first = tr.last_walls
    assert clear.shape == first.shape == (len(egos), 2, 2) and first.dtype == torch.int32
    for col, pl in ((0, plans), (1, refined)):                  # a second call on the plans themselves gives the same bits
        c2, f2, _ = ops.path_walls(pl.reshape(-1, 12, 2), pstart[:, :2].repeat_interleave(2, 0), 1, dev(walls), 0.05, 2.0)
        assert torch.equal(bits(clear[..., col]), bits(c2.view(-1, 2))) and torch.equal(first[..., col], f2.view(-1, 2))
    print("wall clearance before %.4f after %.4f, wall penalty before %.4f after %.4f"
          % (float(clear[..., 0].mean()), float(clear[..., 1].mean()), float(cost[..., 0, 3].mean()), float(cost[..., 1, 3].mean())))
    plain = tr.refine_plans(obsv, plans, K, 0.1, **kw)
    assert tr.last_walls is None and plain[2].shape[-1] == 3
    empty = tr.refine_plans(obsv, plans, K, 0.1, walls=np.zeros((0, 4), np.float32), **kw)
    assert same((plain[0], plain[1], plain[2], plain[3]), (empty[0], empty[1], empty[2][..., :3], empty[3]))
    assert bool(torch.isinf(tr.last_walls[0]).all())
    with pytest.raises(ValueError):
        tr.refine_plans(obsv, plans, K, 0.1, walls=np.zeros((W.WALLS_MAX + 1, 4), np.float32), **kw)
    torch.manual_seed(1)
    wide = sw.SocialWaysTrainer(12, hidden_size=96, device=DEV)  # any hidden size: it needs only Generator.sample()
    out = wide.refine_plans(obsv[:5], plans[1], 6, 0.1, ego=[2], walls=walls)
    assert out[2].shape == (1, 2, 2, 4) and wide.last_walls[0].shape == (1, 2, 2)


def test_the_corridor_through_the_trainer():
    """trainer.refine_plans() with the corridor's draws in place of the generator's: last_walls says what the wall term is for."""
    import socialways_amd as sw
    case, C = W.corridor_case(), W.CORRIDOR
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(case["Tp"], use_social=True, device=DEV)
    n, K = case["sizes"][0], case["K"]
    obsv = torch.zeros(n, 8, 2, device=DEV)
    obsv[:, -1] = dev(case["start"])                             # every pedestrian path starts at its last observed position
    ph = torch.zeros(K, n, case["Tp"], 4, device=DEV)
    ph[..., :2] = dev(case["pos"])
    tr.G.sample = lambda *a, **k: ph                             # the constructed draws, not the untrained generator's
    kw = dict(coll_dist=C["coll_dist"], plan_start=case["plan_start"])
    tr.refine_plans(obsv, case["plans"], K, C["dist"], walls=case["walls"], w_wall=C["w_wall"], **kw)
    with_w = tr.last_walls[0][..., 1].clone()
    from socialways_amd import stats
    out = tr.refine_plans(obsv, case["plans"], K, C["dist"], **kw)      # the launch without walls
    assert tr.last_walls is None and out[2].shape[-1] == 3
    without, first, _ = stats.path_walls(out[0][0], case["walls"], C["coll_dist"], start=case["plan_start"])
    print("corridor through the trainer: plan-to-wall clearance %.3f with the wall term, %.3f without" % (float(with_w), float(without)))
    assert bool((with_w > C["coll_dist"]).all()) and bool((without < C["coll_dist"]).all()) and int(first[0]) >= 0
    zero = tr.refine_plans(obsv, case["plans"], K, C["dist"], walls=case["walls"], w_wall=0.0, **kw)      # a wall term of weight 0
    assert same((zero[0], zero[3], zero[2][..., :3]), (out[0], out[3], out[2])) and torch.equal(bits(tr.last_walls[0][..., 1]), bits(without[None]))


def biwi():
    import socialways_amd as sw
    from _util import golden
    g = golden("biwi_synth")
    data = sw.SceneDataset(g["obsvs"], g["preds"], g["batches"], g["times"], device=DEV)
    torch.manual_seed(2)
    return g, data, sw.SocialWaysTrainer(data.pred.shape[1], use_social=True, device=DEV)


def world_walls(g, seed=3, n=24, inside=True):
    """Segments in world coordinates: inside the recording's bounding box, or in a frame two units outside it."""
    xy = np.concatenate([g["obsvs"].reshape(-1, 2), g["preds"].reshape(-1, 2)], 0)
    lo, hi = xy.min(0), xy.max(0)
    rng = np.random.RandomState(seed)
    if inside:
        a = lo + rng.rand(n, 2) * (hi - lo)
        return np.concatenate([a, a + rng.uniform(-1.5, 1.5, (n, 2))], 1).astype(np.float32)
    lo, hi = lo - 2.0, hi + 2.0
    return np.array([[lo[0], lo[1], hi[0], lo[1]], [hi[0], lo[1], hi[0], hi[1]], [hi[0], hi[1], lo[0], hi[1]], [lo[0], hi[1], lo[0], lo[1]]],
                    np.float32)


def test_walls_from_world_and_load_walls(tmp_path):
    import socialways_amd as sw
    g, data, _ = biwi()
    seg = world_walls(g)
    path = tmp_path / "map.txt"
    path.write_text("# a map\n" + "\n".join("%r %r %r %r  # wall %d" % (*map(float, r), i) for i, r in enumerate(seg)) + "\n\n")
    assert np.array_equal(sw.load_walls(str(path)), seg)
    (tmp_path / "none.txt").write_text("# nothing\n")
    assert sw.load_walls(str(tmp_path / "none.txt")).shape == (0, 4)
    (tmp_path / "bad.txt").write_text("1 2 3\n")
    with pytest.raises(ValueError):
        sw.load_walls(str(tmp_path / "bad.txt"))
    w = data.walls_from_world(seg)
    assert w.shape == (24, 2, 2) and w.dtype == torch.float32 and w.device == data.obsv.device
    assert torch.equal(w, data.walls_from_world(seg.reshape(-1, 2, 2)))
    back = data.scale.denormalize(w.cpu().numpy())
    assert np.abs(back.reshape(-1, 4) - seg).max() <= 1e-5 * np.abs(seg).max()
    want = data.scale.normalize(seg.reshape(-1, 2, 2).copy())
    assert np.array_equal(w.cpu().numpy(), want) and np.array_equal(seg, world_walls(g)), "the caller's array is not touched"
    assert data.walls_from_world(np.zeros((0, 4))).shape == (0, 2, 2)
    with pytest.raises(ValueError):
        data.walls_from_world(np.zeros((3, 5)))


def test_evaluate_walls():
    g, data, tr = biwi()
    walls = data.walls_from_world(world_walls(g))
    torch.manual_seed(31)
    records = []
    res = tr.evaluate_walls(data, walls, n_gen_samples=20, wall_dist=0.2, collect=records)
    torch.manual_seed(31)
    plain = tuple(tr.evaluate(data, n_gen_samples=20))
    assert (res["ade_avg"], res["fde_avg"], res["ade_min"], res["fde_min"]) == plain
    torch.manual_seed(31)
    assert tr.evaluate_walls(data, walls, n_gen_samples=20, wall_dist=0.2) == res      # without collect: the same numbers
    print({k: res[k] for k in tr.WALL_KEYS + ("n_agents", "n_free")})
    K, N = 20, data.n_test_samples
    assert res["n_agents"] == N == sum(r["obsvs"].shape[0] for r in records) and res["K"] == K and res["wall_dist"] == 0.2
    assert 0 < res["wall_draws"] <= res["wall_agents"] <= 1 and res["wall_blocked"] <= res["wall_draws"]
    # the numbers, rebuilt on the host from the records: integers exactly, means to 1e-6
    ww = world_walls(g).reshape(-1, 2, 2)
    hit_n = agents = blocked = gt = n_free = t_sum = 0
    ade = fde = 0.0
    for r in records:
        first, clear = r["wall_first"], r["wall_clear"]
        n = r["obsvs"].shape[0]
        assert first.shape == clear.shape == (K, n) and np.array_equal(first >= 0, clear < np.float32(0.2))
        ref = W.path_walls_reference(r["preds_our"], r["obsvs"][:, -1], ww, 0.2)      # world coordinates, float64
        decided = np.abs(ref["clear"] - 0.2) > 1e-4
        assert np.array_equal((first >= 0)[decided], (ref["first"] >= 0)[decided])
        fin = np.isfinite(ref["clear"])
        assert np.abs(clear[fin] - ref["clear"][fin]).max() <= 1e-4
        hit = first >= 0
        hit_n += int(hit.sum())
        agents += int(hit.any(0).sum())
        blocked += int(hit.all(0).sum())
        t_sum += int(first[hit].sum())
        gt += int((W.path_walls_reference(r["preds_gtt"][None], r["obsvs"][:, -1], ww, 0.2)["first"] >= 0).sum())
        e = np.sqrt(((r["preds_our"].astype(np.float64) - r["preds_gtt"][None]) ** 2).sum(-1))      # (K, n, T)
        assert r["err"].shape == (K, n, 2) and r["err"].dtype == np.float32
        assert np.abs(r["err"][..., 0] - e.mean(2)).max() <= 1e-4 and np.abs(r["err"][..., 1] - e[:, :, -1]).max() <= 1e-4      # float32 records
        a, f = np.where(hit, np.inf, r["err"][..., 0].astype(np.float64)), np.where(hit, np.inf, r["err"][..., 1].astype(np.float64))
        free = ~hit.all(0)
        n_free += int(free.sum())
        ade, fde = ade + a.min(0)[free].sum(), fde + f.min(0)[free].sum()
    assert res["n_free"] == n_free and res["wall_draws"] == hit_n / (K * N) and res["wall_agents"] == agents / N
    assert res["wall_blocked"] == blocked / N and res["wall_gt"] == gt / N and abs(res["t_first"] - t_sum / max(hit_n, 1)) <= 1e-12
    assert n_free > 0 and abs(res["ade_min_free"] - ade / n_free) <= 1e-6 * ade / n_free      # from the records' per-draw errors
    assert abs(res["fde_min_free"] - fde / n_free) <= 1e-6 * fde / n_free
    # a map outside the recording's bounding box: nobody, drawn or true, touches it ... unless a draw leaves the box
    outside = data.walls_from_world(world_walls(g, inside=False))
    torch.manual_seed(31)
    out = tr.evaluate_walls(data, outside, n_gen_samples=20, wall_dist=0.2)
    assert out["wall_gt"] == 0 and (out["ade_avg"], out["fde_avg"], out["ade_min"], out["fde_min"]) == plain
    torch.manual_seed(31)
    none = tr.evaluate_walls(data, np.zeros((0, 4)), n_gen_samples=20)
    assert none["wall_draws"] == none["wall_gt"] == none["t_first"] == 0 and none["n_free"] == N and none["ade_min_free"] > 0
    assert abs(none["ade_min_free"] - plain[2]) <= 1e-6 * plain[2]


def test_evaluate_refine_with_walls():
    g, data, tr = biwi()
    walls = data.walls_from_world(world_walls(g))
    torch.manual_seed(31)
    records = []
    res = tr.evaluate_refine(data, n_gen_samples=20, dist=0.5, coll_dist=0.1, walls=walls, wall_dist=0.4, w_wall=2.0, collect=records)
    torch.manual_seed(31)
    plain = tr.evaluate_refine(data, n_gen_samples=20, dist=0.5, coll_dist=0.1)
    assert not set(tr.REFINE_WALL_KEYS) & set(plain) and set(tr.REFINE_WALL_KEYS) <= set(res)
    for k in ("ade_avg", "fde_avg", "ade_min", "fde_min", "risk_cv", "col_cv", "pen_cv", "n_ego"):
        assert res[k] == plain[k], k                             # the naive plans and the draws are the same
    print({k: res[k] for k in tr.REFINE_KEYS + tr.REFINE_WALL_KEYS})
    assert 0 <= res["wall_ref"] <= 1 and 0 <= res["wall_cv"] <= 1 and 0 <= res["penw_ref"] and res["penw_cv"] > 0
    multi = [r for r in records if r["obsvs"].shape[0] > 1]
    n = sum(r["obsvs"].shape[0] for r in multi)
    assert n == res["n_ego"]
    ww = world_walls(g).reshape(-1, 2, 2)
    for key, col, name in (("wall_cv", 0, "preds_lnr"), ("wall_ref", 1, "plan_ref")):
        hits = 0
        for r in multi:
            clear = r["wall_plan"][:, col]
            ref = W.path_walls_reference(r[name][None], r["obsvs"][:, -1], ww, 0.1)["clear"][0]
            fin = np.isfinite(ref)
            assert np.abs(clear[fin] - ref[fin]).max() <= 1e-4
            decided = np.abs(ref - 0.1) > 1e-4
            assert np.array_equal((clear < np.float32(0.1))[decided], (ref < 0.1)[decided])
            hits += int((clear < np.float32(0.1)).sum())
        assert abs(res[key] - hits / n) <= 1e-12
    # the mean wall penalties: from the records' per-ego penalties to 1e-6, and those against the float64 reference of the
    # penalty on the records' plans (float32, denormalised: the penalty is a difference of squares, so 1e-3 of the sum there)
    ss = float(data.ss)
    for key, col, name in (("penw_cv", 0, "preds_lnr"), ("penw_ref", 1, "plan_ref")):
        total = sum(float(r["penw_plan"][:, col].astype(np.float64).sum()) for r in multi)
        assert total > 0 and abs(res[key] - total / n) <= 1e-6 * total / n
        ref = 0.0
        for r in multi:
            for i in range(r["obsvs"].shape[0]):
                PX = np.concatenate([r["obsvs"][i, -1:, :2], r[name][i]], 0).astype(np.float64)
                ref += float(W.wall_penalty(PX, ww.astype(np.float64), 0.4, np.float64)[0])
        print("%s: %.6g from the records, %.6g from the float64 penalty of the recorded plans" % (key, total / n, ref / n))
        assert abs(total - ref) <= 1e-3 * ref


def test_evaluate_walls_at_a_wide_hidden_size():
    """The wide and generic trainers take evaluate_walls() through the sampling hook of the evaluate_*() family: the draws are
    Generator.sample()'s, so the four numbers agree with evaluate() as evaluate_scenes()'s do there (1e-5 relative, not bit for
    bit: tests/test_gpu_scene.py), and the wall numbers are those of the records."""
    import socialways_amd as sw
    from socialways_amd import generic
    g, data, _ = biwi()
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(data.pred.shape[1], hidden_size=96, use_social=True, device=DEV)
    assert isinstance(tr, generic.GenericTrainer)
    walls = data.walls_from_world(world_walls(g))
    torch.manual_seed(31)
    four = tr.evaluate(data, n_gen_samples=5)
    torch.manual_seed(31)
    records = []
    res = tr.evaluate_walls(data, walls, n_gen_samples=5, wall_dist=0.2, collect=records)
    got = np.asarray([res[k] for k in ("ade_avg", "fde_avg", "ade_min", "fde_min")])
    assert np.abs(got - np.asarray(four)).max() <= 1e-5 * np.abs(np.asarray(four)).max()
    hits = sum(int((r["wall_first"] >= 0).sum()) for r in records)
    assert res["n_agents"] == data.n_test_samples and res["wall_draws"] == hits / (5 * res["n_agents"]) and hits > 0
