"""train() / test() / checkpoint of the reference (train.py:439-668) over the HIP hot path.

`SocialWaysTrainer.step()` is the body of train.py:458-554 for one packed batch:
two discriminator updates (`n_unrolling_steps`+1), one generator update, the Linear-only restore of
the unrolled-GAN surrogate (train.py:498-499, 541-543) and the ADE/FDE partial sums.
Differences to the reference's *formulation*, none to its results:
  * the three `predict()` calls of a step use the same noise and the same generator weights
    (train.py:473,480,507), so the rollout is computed ONCE and its saved
    activations serve the generator backward;
  * the fake and the real branch of a D update share one observation-LSTM pass;
  * gradients are written by the kernels straight into packed buffers that are the `.grad`s of
    the parameters; Adam stays torch.optim.Adam (same parameter order as train.py:379-385, so the
    optimizer state_dicts interchange with the reference's checkpoint).
Data parallelism (one process per GPU): every rank runs `step()` on a scene-aligned shard of the
packed batch with the GLOBAL batch size in the loss normalisation and the packed gradient buffers
are all-reduced (sum) before each optimizer step - 3 RCCL all-reduces per training step.
"""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.optim as opt

from . import _lib as L
from . import ops
from .data import WallGrid, shard_scenes
from .model import Discriminator, Generator, get_traj_4d, predict_cv, refuse_obs_len
from .noise import EVAL, TRAIN, DeviceNoise


class PackedAdam:
    """Adam (train.py:379-385: lr, betas (0.9, 0.999), eps 1e-8, no weight decay) over ONE packed parameter
    buffer, executed by torch's own fused multi-tensor Adam kernel (`torch._fused_adam_`, the op behind
    `torch.optim.Adam(fused=True)`) on chunk views of the buffer: one kernel launch per update.  The step
    counter is a device scalar the CALLER may supply (`step(step_tensor)`): a hipGraph-replayed training step
    gets its counters from the staging kernel instead of spending a graph node per update on incrementing
    them.  Reads and writes the reference's per-parameter optimizer state_dict (train.py:659,662 / 631,634):
    `slices` = [(offset, numel, shape)] in the reference's parameter order.  Padding floats have zero
    gradients and stay zero."""

    # torch's multi-tensor kernel gives one workgroup per (tensor, 64K chunk): feed it many small views - but at
    # most MAX_CHUNKS of them, beyond which the update is split into a second kernel launch (~5 us per graph node)
    MIN_CHUNK, MAX_CHUNKS = 2048, 30      # swept 8..36 / 512..4096 on one box: flat within noise

    def __init__(self, flat, gflat, slices, lr, betas=(0.9, 0.999), eps=1e-8, capturable=False, disc_tp=0):
        self.slices = slices
        self.flat = flat
        self.gflat = gflat
        # On the GPU the update is the library's own kernel (sw_adam_packed: torch's fused Adam restated operation by
        # operation, the arithmetic the gradient-finishing kernels apply in a single process) - one launch, and the
        # Discriminator's weight images (disc_tp = its horizon) follow the update.  torch's kernel remains for CPU
        # buffers and for a checkpoint that carries weight decay (the reference never sets it, train.py:379-385).
        self.native = flat.is_cuda
        self.disc_tp = int(disc_tp)
        n = flat.numel()
        c = self.CHUNK = max(self.MIN_CHUNK, (-(-n // self.MAX_CHUNKS) + 255) // 256 * 256)
        self.m, self.v = torch.zeros_like(flat), torch.zeros_like(flat)
        cut = lambda t: [t[o:min(o + c, n)] for o in range(0, n, c)]
        self.ps, self.gs, self.ms, self.vs = cut(flat), cut(gflat), cut(self.m), cut(self.v)
        self.t = 0                                              # updates applied so far
        self.step_t = torch.zeros((), device=flat.device)       # device copy of `t` for self-counted updates
        self.group = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                          foreach=None, capturable=capturable, differentiable=False, fused=True)

    @torch.no_grad()
    def step(self, step_tensor=None):
        """One update.  `step_tensor` = device scalar holding the 1-based index of this update (the caller
        then also advances `self.t`); without it the optimizer counts itself."""
        if step_tensor is None:
            self.t += 1
            self.step_t.fill_(float(self.t))      # eager only: a captured update always gets its index from the caller
            step_tensor = self.step_t
        g = self.group
        if self.native and not g["weight_decay"]:
            L.call("sw_adam_packed", L.ptr(self.flat), L.ptr(self.gflat), L.ptr(self.m), L.ptr(self.v), self.flat.numel(),
                   L.ptr(step_tensor), float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                   self.disc_tp, L.stream())
            return
        torch._fused_adam_(self.ps, self.gs, self.ms, self.vs, [], [step_tensor] * len(self.ps), amsgrad=False,
                           lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1], weight_decay=g["weight_decay"],
                           eps=g["eps"], maximize=False, grad_scale=None, found_inf=None)

    @property
    def keeps_images(self):
        """Does step() keep registered Discriminator images current (sw_adam_packed does, torch's kernel cannot)?"""
        return bool(self.native and not self.group["weight_decay"] and self.disc_tp > 0)

    @property
    def fusable(self):
        """May a gradient-finishing kernel apply this update itself (sw_disc_bwd_gan_adam / sw_gen_wgrad_adam)?  Their
        arithmetic is Adam without weight decay."""
        return not self.group["weight_decay"]

    def fused_args(self, step_tensor=None):
        """(m, v, step scalar, lr, beta1, beta2, eps) for a kernel that applies this update itself
        (sw_disc_bwd_gan_adam) - the bookkeeping of `step()` without the launch."""
        if step_tensor is None:
            self.t += 1
            self.step_t.fill_(float(self.t))
            step_tensor = self.step_t
        g = self.group
        return (self.m, self.v, step_tensor, g["lr"], g["betas"][0], g["betas"][1], g["eps"])

    def zero_grad(self, set_to_none=False):
        for t in self.gs:
            t.zero_()

    @property
    def param_groups(self):
        return [self.group]

    def state_dict(self):
        g = dict(self.group)
        g["params"] = list(range(len(self.slices)))
        state = {}
        if self.t > 0:
            for i, sl in enumerate(self.slices):
                off, n, shape = sl[:3]
                pick = lambda buf: self._true(buf[off:off + n], sl).clone()
                state[i] = {"step": torch.tensor(float(self.t)), "exp_avg": pick(self.m), "exp_avg_sq": pick(self.v)}
        return {"state": state, "param_groups": [g]}

    @staticmethod
    def _true(flat_slice, sl):
        """A parameter's slice of a packed buffer in the reference's shape: (offset, numel, kernel shape) alone, or
        followed by (true shape, index of the true entries) for zero-padded hidden sizes (model._Packed._true)."""
        if len(sl) == 3:
            return flat_slice.view(sl[2])
        return flat_slice[sl[4].to(flat_slice.device)].view(sl[3])

    def load_state_dict(self, sd):
        grp = sd["param_groups"][0]
        for k in ("lr", "betas", "eps", "weight_decay"):
            if k in grp:
                self.group[k] = tuple(grp[k]) if k == "betas" else grp[k]
        state = sd.get("state", {})
        self.m.zero_()
        self.v.zero_()
        self.t = 0
        for i, sl in enumerate(self.slices):
            off, n = sl[0], sl[1]
            # torch Adam keeps state only for parameters that ever received a gradient: the unmodified reference
            # runs with use_social=False (train.py:83), so its checkpoints hold no entries for the attention /
            # feature-embedder parameters (optimizer indices 0..7).  Their moments stay zero here.
            e = state.get(i, state.get(str(i)))
            if e is None:
                continue
            for buf, key in ((self.m, "exp_avg"), (self.v, "exp_avg_sq")):
                val = e[key].to(self.flat.device).reshape(-1)
                if len(sl) == 3:
                    buf[off:off + n] = val
                else:                              # zero-padded hidden size: the true entries into their padded places
                    buf[off:off + n].index_copy_(0, sl[4].to(self.flat.device), val)
            self.t = max(self.t, int(float(e["step"])))       # one shared counter: every present entry was stepped together
        self.step_t.fill_(float(self.t))


class _EvalSums:
    """What test() and every evaluate_*() return first: the per-agent sums ade_avg | fde_avg | ade_min | fde_min, float64 on the
    device, added chunk by chunk and divided by data.n_test_samples at the end; and `scenes`, the row ranges evaluated."""
    KEYS = ("ade_avg", "fde_avg", "ade_min", "fde_min")

    def __init__(self, device):
        self.sums, self.scenes = torch.zeros(4, dtype=torch.float64, device=device), []

    def add(self, c):
        self.scenes += c.ab
        self.sums += c.per_agent.double().sum(0)      # per agent: mean_k ADE | mean_k FDE | min_k ADE | min_k FDE

    def result(self, data):
        return dict(zip(self.KEYS, (self.sums / data.n_test_samples).tolist()))


@torch.no_grad()
def _scored_draws(tr, obsv_p, n_samples, top_m, sub_batches, noise, row0, obs_len=None):
    """What sample_ranked() and sample_diverse() start with: (K, M, the K draws (K, B, n_next, 4), their scores (K, B)); top_m
    is checked before anything of the trainer is touched.  obs_len (ragged histories, Generator.sample()) is checked and
    moved to the device once and goes to both the sampling and the scoring call."""
    K, M = int(n_samples), int(top_m)
    if not 1 <= M <= K:
        raise ValueError("top_m must lie in 1 .. n_samples = %d, got %d" % (K, M))
    if obs_len is not None:
        if not isinstance(tr.G, Generator):      # the generic-width and wide paths: no ragged kernels
            refuse_obs_len(obs_len, type(tr).__name__)
        obs_len = ops.obs_len_arg(obs_len, obsv_p.shape[0], obsv_p.shape[1], 2, obsv_p.device)
    ph = tr.G.sample(obsv_p, K, tr.n_next, sub_batches, noise, row0=row0, obs_len=obs_len)
    return K, M, ph, tr.D.score_samples(obsv_p, ph, obs_len=obs_len)[0]


def _plan_queries(n_next, obsv_p, plans, n_samples, sub_batches, scene, ego, plan_start, scale):
    """The arguments plan_risk() and refine_plans() share, checked on the host before anything is sampled -> (K, B, plans
    (Q, P, n_next, 2), sb, scene (Q,) int32, ego (Q,) int32 or None, plan_start (Q, 2) or None with ego)."""
    K = int(n_samples)
    if K < 1:
        raise ValueError("n_samples must be at least 1, got %r" % (n_samples,))
    if not float(scale) > 0.0:
        raise ValueError("scale must be > 0, got %r" % (scale,))
    if obsv_p.dim() != 3 or obsv_p.shape[1] < 1 or obsv_p.shape[2] < 2:
        raise ValueError("obsv_p must be (B, To, >= 2), got %s" % (tuple(obsv_p.shape),))
    B = obsv_p.shape[0]
    plans = torch.as_tensor(plans, dtype=torch.float32)
    if plans.dim() == 3:
        plans = plans.unsqueeze(0)
    if plans.dim() != 4 or plans.shape[1] < 1 or tuple(plans.shape[2:]) != (n_next, 2):
        raise ValueError("plans must be (Q, P >= 1, n_next, 2) or (P, n_next, 2) with n_next = %d, got %s"
                         % (n_next, tuple(plans.shape)))
    Q = plans.shape[0]
    sb = np.asarray(sub_batches, dtype=np.int64).reshape(-1, 2)
    S = max(len(sb), 1)

    def rows(x, name, hi):
        host = np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
        if host.shape != (Q,) or host.dtype.kind not in "iu" or (host < 0).any() or (host >= hi).any():
            raise ValueError("%s must hold Q = %d integers in 0 .. %d, got %r" % (name, Q, hi - 1, x))
        return host.astype(np.int32)

    if scene is None:
        if Q != S:
            raise ValueError("without `scene` query q belongs to scene q: plans hold Q = %d queries, there are %d scenes" % (Q, S))
        scene = np.arange(Q)
    scene = rows(scene, "scene", S)
    if ego is not None:
        if plan_start is not None:
            raise ValueError("plan_start and ego exclude each other: with ego the plans start at obsv_p[ego[q], -1]")
        ego = rows(ego, "ego", B)
    elif plan_start is None:
        raise ValueError("without ego the plans need plan_start (Q, 2)")
    else:
        plan_start = torch.as_tensor(plan_start, dtype=torch.float32)
        if tuple(plan_start.shape) != (Q, 2):
            raise ValueError("plan_start must be (Q, 2) = (%d, 2), got %s" % (Q, tuple(plan_start.shape)))
    return K, B, plans, sb, scene, ego, plan_start


def _plan_walls(both, plan_start, walls, dist, inv_ss, lens=None):
    """ONE sw_path_walls launch on plans laid side by side: both (Q, N, T, 2) with their start points plan_start (Q, 2) and
    lens (Q,) or None -> (clear (Q, N), first (Q, N) int32, nseg (Q, N) int32)."""
    Q, N = both.shape[0], both.shape[1]
    clear, first, nseg = ops.path_walls(both.reshape(Q * N, both.shape[2], 2), plan_start.repeat_interleave(N, 0), 1, walls, dist,
                                        inv_ss, lens=None if lens is None else lens.repeat_interleave(N))
    return clear.view(Q, N), first.view(Q, N), nseg.view(Q, N)


def _refuse_ragged(data, what, why):
    """Calls without ragged kernels behind them refuse a dataset that carries obs_len, loudly, before any launch."""
    if getattr(data, "obs_len", None) is not None:
        raise L.SocialWaysHipError("%s does not take a dataset with obs_len (ragged observation histories): %s" % (what, why))


def _refuse_pred_len(data, what, why):
    """Ragged futures are an evaluation feature: every call whose losses or errors would read the padding of a short future
    as truth refuses a dataset that carries pred_len, loudly, before any launch."""
    if getattr(data, "pred_len", None) is not None:
        raise L.SocialWaysHipError("%s does not take a dataset with pred_len (ragged futures): %s" % (what, why))


_PRED_LEN_TRAIN = ("a truncated future has no discriminator input (D encodes the flattened n_next frames) and the losses would "
                   "read the padding as truth - train on full windows (create_dataset / create_dataset_ragged without "
                   "min_next) and evaluate the short futures with evaluate*() / evaluate_horizon()")


def _wall_key(wall):
    """The wall term's entry of the graph key: None, or (the address of the walls, M, dist, weight) - with a WallGrid, its key()
    in place of the first two."""
    if wall is None:
        return None
    if isinstance(wall[0], WallGrid):
        return wall[0].key() + (wall[1], wall[2])
    return (wall[0].data_ptr(), int(wall[0].shape[0]), wall[1], wall[2])


def _wall_reach(wall, ss):
    """A step with a WallGrid behind the wall term asks about dw = dist * ss: refused on the host, before any launch, unless
    the grid's reach covers it."""
    if wall is not None and isinstance(wall[0], WallGrid):
        ops.check_wall_grid_arg(wall[0], wall[0].device, float(np.float32(wall[1] * float(ss))), "set_wall_loss: dist * ss =")


class SocialWaysTrainer:
    STEPS_PER_LAUNCH = 4    # train_epoch: consecutive packed batches of one scene layout per graph launch (step_many)
    Z_COLS = 32             # noise columns of the kernels (hidden size 64: train.py:81); smaller models are zero-padded
    _direct = None          # the direct gradient exchange (SW_ALLREDUCE=direct / auto; the fused trainer only) and what the
    exchange_probe = None   # auto mode's probe measured - class-level defaults: the wider trainers have their own __init__
    noise = None            # a DeviceNoise: z of train_epoch() / evaluate*() from the device stream; None = the reference's host streams
    ragged_fused = False    # step(obs_len=...): D updates in one launch (sw_disc_update_ragged) and, with use_graph, captured steps
    clearance_loss = None   # (dist, weight): the scene-clearance term of the generator loss (set_clearance_loss()); None = off
    last_clearance = None   # with the term on: (loss (B,), count (B,) int32) of the last step (sw_clearance_grad's outputs)
    wall_loss = None        # (walls (M, 2, 2) on the device or a WallGrid, dist, weight): the wall term of the generator loss (set_wall_loss()); None = off
    last_wall_loss = None   # with the term on: (loss (B,), count (B,) int32) of the last step (sw_wall_grad's outputs)
    last_walls = None       # refine_plans(walls=...): (clear (Q, P, 2), first (Q, P, 2) int32) before | after; None without walls

    def __new__(cls, n_next=None, hidden_size=64, *args, **kw):
        """Widths above the fused kernels' 64 units and latent-code counts other than 2 (train.py:42-44, 65) train on
        the generic-width path (generic.py: the same model layer by layer, same public surface)."""
        nl = kw.get("n_latent_codes", args[6] if len(args) > 6 else 2)      # positional slot 9 of __init__'s signature
        if cls is SocialWaysTrainer and (int(hidden_size) > 64 or int(nl) != 2):
            from .generic import GenericTrainer
            from .wide import WideTrainer
            # widths that are multiples of 32: the wide path (time-step-level kernels, explicit backward, one hipGraph per
            # step); anything else the reference accepts: the layer-by-layer generic path under torch's tape
            if os.environ.get("SW_WIDE", "1") != "0" and WideTrainer.supports(hidden_size, nl, kw.get("use_variety_loss", False)):
                return object.__new__(WideTrainer)
            return object.__new__(GenericTrainer)
        return object.__new__(cls)

    def _device_noise(self, noise):
        """The DeviceNoise a call works with: its `noise` argument, else self.noise; None = the host stream."""
        dn = self.noise if noise is None else noise
        if dn is not None and not isinstance(dn, DeviceNoise):
            raise TypeError("noise must be a DeviceNoise or None, got %s" % type(dn).__name__)
        return dn

    def set_clearance_loss(self, dist, weight=1.0):
        """Train against collisions: the generator loss gains L_col = weight / (Bg * Tp) * the sum over the scenes of the
        packed batch, the pairs a < b of a scene and the Tp segments of max(0, 1 - |c|^2 / d0^2)^2 - c the closest approach of
        the two predicted futures within the segment, each path starting at the agent's last observed position, both agents
        moving linearly (the quantity behind col_* of evaluate_scenes(), sw_clearance_grad) - with d0 = dist * ss: `dist` is
        in world units like evaluate_scenes()'s coll_dist, Bg the agents of the global packed batch (the L2 term's
        normalisation).  The penalty is C1 where a pair reaches d0, its gradient continuous across the ends of a segment,
        finite everywhere and exactly 0 for coincident agents.  One extra launch per step between the other terms on
        d/d(pred_hat) and the generator's backward pass (which then runs un-fused from the D pass, as with use_l2_loss); dense
        and ragged steps, eager and captured, single process and data parallel (scenes are sharded whole: every pair is
        rank-local).  `last_clearance` = (loss (B,), count (B,) int32) then holds the last step's per-agent shares of the
        unscaled sum and numbers of (partner, segment)s closer than d0 - views of buffers the next step overwrites;
        L_col = weight / (Bg * Tp) * loss.sum().  weight 0 measures without training on it.  set_clearance_loss(None)
        switches the term off: the step then makes exactly the launches it made before.  Assigning the tuple
        (dist, weight) or None to `clearance_loss` does the same without the checks."""
        if dist is None:
            self.clearance_loss = None
            self.last_clearance = None
            return
        dist, weight = float(dist), float(weight)
        if not (np.isfinite(dist) and dist > 0.0):
            raise ValueError("set_clearance_loss: dist must be finite and > 0, got %r" % dist)
        if not (np.isfinite(weight) and weight >= 0.0):
            raise ValueError("set_clearance_loss: weight must be finite and >= 0, got %r" % weight)
        self.clearance_loss = (dist, weight)

    def set_wall_loss(self, walls, dist=None, weight=1.0):
        """Train against the map: the generator loss gains L_wall = weight / (Bg * Tp) * the sum over the agents of the packed
        batch, the Tp segments of an agent's predicted future - the path starting at its last observed position, the agent
        moving linearly between frames - and the M walls of max(0, 1 - |c|^2 / dw^2)^2, c the closest approach of the segment
        to the wall (the quantity behind wall_* of evaluate_walls(), sw_wall_grad), with dw = dist * ss: `dist` is in world
        units like evaluate_walls()'s wall_dist, Bg the agents of the global packed batch (the normalisation of the L2 and
        clearance terms).  walls: the static map in the dataset's coordinates (data.walls_from_world(...)), a tensor or host
        data, (M, 2, 2) or (M, 4), M = 0 .. 1024 (an empty map is accepted), or a WallGrid of any size on the trainer's device
        (data.wall_grid_from_world(...); the step then launches sw_wall_grad_grid, and dist * ss must stay below the grid's
        reach: ValueError from step() before any launch); a tensor is copied to the trainer's device unless it is a
        float32 (M, 2, 2) tensor there already, and the trainer holds it.  A captured step bakes in the tensor's address: writing
        into that tensor in place is seen by the replays; a new map is a new set_wall_loss() call.
        The penalty is C1 where a segment reaches dw, its gradient finite everywhere and exactly 0 where a path CROSSES a wall:
        descent keeps paths off the walls, it cannot undo a crossing.  One extra launch per step behind the other terms on
        d/d(pred_hat) (the clearance term, when both are on, comes first), the generator's backward pass then running un-fused
        from the D pass as with use_l2_loss; dense and ragged steps, eager and captured, single process and data parallel
        (the map is the same on every rank, rows are rank-local).  `last_wall_loss` = (loss (B,), count (B,) int32) then holds
        the last step's per-agent unscaled sums and numbers of (segment, wall)s closer than dw - views of buffers the next step
        overwrites; L_wall = weight / (Bg * Tp) * loss.sum().  weight 0 measures without training on it.  set_wall_loss(None)
        switches the term off: the step then makes exactly the launches it made before.  The loss rows step() returns do not
        show the term."""
        if walls is None:
            self.wall_loss = None
            self.last_wall_loss = None
            return
        if dist is None:
            raise ValueError("set_wall_loss: a map needs its dist")
        dist, weight = float(dist), float(weight)
        if not (np.isfinite(dist) and dist > 0.0):
            raise ValueError("set_wall_loss: dist must be finite and > 0, got %r" % dist)
        if not (np.isfinite(weight) and weight >= 0.0):
            raise ValueError("set_wall_loss: weight must be finite and >= 0, got %r" % weight)
        walls = ops.walls_arg(walls, self.device)                               # shape and M <= 1024: ValueError
        self.wall_loss = (walls, dist, weight)

    def _pad_z(self, z):
        return z if z.shape[-1] == self.Z_COLS else torch.nn.functional.pad(z, (0, self.Z_COLS - z.shape[-1]))

    def __init__(self, n_next, hidden_size=64, lr_g=1e-4, lr_d=1e-3, n_unrolling_steps=1, use_social=True,
                 use_info_loss=True, loss_info_w=0.5, n_latent_codes=2, device="cuda", process_group=None,
                 fused_adam=True, use_graph=None, use_l2_loss=False, use_variety_loss=False, loss_l2_w=0.5, variety_k=20,
                 ragged_fused=False):
        self.device = L.indexed_device(device)
        # Ragged steps (step(obs_len=...), train_epoch_ragged()) on the fused route: each D update one launch
        # (ops.disc_update(obs_len=...)) and, with use_graph, the step captured per layout like the dense one, obs_len staged
        # through the pinned slot.  Off (the default): every ragged step makes the eager launches it always made.
        self.ragged_fused = bool(ragged_fused)
        self.n_next = n_next
        self.noise_len = hidden_size // 2
        self.n_unrolling_steps = n_unrolling_steps
        self.use_info_loss = use_info_loss
        self.loss_info_w = loss_info_w
        # train.py:67-69.  `use_variety_loss` reproduces train.py:527-536 AS WRITTEN: its 20 predict()
        # calls reuse the same noise (identical values) and only the k = 19 term - the L2 of AGENT 19 of
        # the packed batch - enters the loss; the 20 redundant rollouts are not executed.
        # `use_variety_loss="fixed"` is the term the reference evidently MEANT (Social-GAN's best-of-K L2):
        # `variety_k` rollouts with independent z (the step's own z is sample 0), per agent the minimum over the samples
        # of the mean squared error, averaged over the batch; the gradient reaches the arg-min sample only.  The K
        # rollouts run as ONE folded batch of K*B agents (like test()), so the generator's work grows K-fold.
        if use_variety_loss not in (False, True, "fixed"):
            raise ValueError("use_variety_loss: False, True (train.py:527-536 as written) or 'fixed'")
        self.use_l2_loss, self.use_variety_loss, self.loss_l2_w = use_l2_loss, use_variety_loss, loss_l2_w
        self.variety_k = int(variety_k)
        self.last_variety = None             # fixed mode: (per-agent minimum (B,), arg-min sample (B,) int32) of the last step
        # construction order = train.py:370-385 (RNG -> init mapping, optimizer parameter order)
        self.G = Generator(hidden_size, 1, use_social=use_social, device=self.device)
        self.G.unify()
        self.world = 1 if process_group is None else torch.distributed.get_world_size(process_group)
        if use_graph is None:          # hipGraph replay of the step (segmented around the all-reduces when world > 1)
            use_graph = self.device.type == "cuda" and fused_adam
        self.use_graph = bool(use_graph)
        self.max_graphs = int(os.environ.get("SW_MAX_GRAPHS", "8"))    # captured packed-batch layouts (the rest of the steps run eagerly)
        self._graphs = {}
        self._force_dist = os.environ.get("SW_FORCE_DIST", "") == "1"   # 1-rank group still runs the collectives (tests)
        self._fuse_d_adam = True      # D's Adam inside the gradient reduction (single process; tests switch it off to compare)
        self._fuse_g_adam = True      # ... and the generator's (needs the weight images)
        # Data parallel: are the RCCL all-reduces recorded INSIDE the step graph (one launch for K steps) or run
        # eagerly between graph segments (3 segment boundaries per step)?  SW_GRAPH_COLLECTIVES=1 / 0 decides;
        # unset = probe once (a small captured all-reduce replayed twice and checked on every rank) and use the
        # in-graph form only if the whole group agrees that it works.
        gc_env = os.environ.get("SW_GRAPH_COLLECTIVES", "")
        self._graph_collectives = True if gc_env == "1" else False if gc_env == "0" else None
        packed = fused_adam and self.device.type == "cuda"
        if packed:
            self.predictor_optimizer = PackedAdam(self.G._flat_all, self.G._gflat_all, self.G.packed_slices(), lr_g)
        else:       # per-parameter torch Adam (CPU tests, literal autograd formulation)
            self.predictor_optimizer = opt.Adam(self.G.predictor_params(), lr=lr_g, betas=(0.9, 0.999))
        self.D = Discriminator(n_next, hidden_size, n_latent_codes, device=self.device)
        if packed:
            self.D_optimizer = PackedAdam(self.D._flat, self.D._gflat,
                                          [(off, k, tuple(p.shape)) + (self.D._true[i] if self.D._true is not None else ())
                                           for i, ((off, k), p) in enumerate(zip(self.D._slices, self.D.parameters()))], lr_d,
                                          disc_tp=n_next)
        else:
            self.D_optimizer = opt.Adam(self.D.parameters(), lr=lr_d, betas=(0.9, 0.999))
        self.pg = process_group
        self.rank = 0 if process_group is None else torch.distributed.get_rank(process_group)
        self.epoch = 0
        if self.pg is not None and self.world > 1:
            self.sync_replicas()
        # SW_ALLREDUCE=direct: the three gradient buckets of a step go through the library's own two-hop all-reduce over
        # hipIpc-mapped exchange buffers (csrc/sw_comm.hip) instead of RCCL's ring; everything else (epoch sums, broadcasts)
        # stays on the process group.  The kernel is an ordinary graph node: the step is captured as ONE graph.
        # SW_ALLREDUCE=auto: build it, check it against the group's all-reduce and time both on this node's links; use it if
        # every rank agrees that it is correct and faster (comm.probe; the verdict is kept in self.exchange_probe).
        self._direct, self.exchange_probe = None, None
        mode = os.environ.get("SW_ALLREDUCE", "")
        if (self.pg is not None and (self.world > 1 or self._force_dist) and self.device.type == "cuda"
                and mode in ("direct", "auto")):
            from . import comm
            buckets = [self.D._gflat.numel(), self.G._gflat_all.numel()]
            if mode == "direct":
                self._direct = comm.DirectAllReduce(self.pg, self.device, max(buckets))
                # no timing, but never unchecked: the exchange must reproduce the group's all-reduce on this node's links
                # before a weight depends on it (collective; SW_ALLREDUCE_CHECK=0 skips it)
                if os.environ.get("SW_ALLREDUCE_CHECK", "1") != "0" and not self._direct.check(buckets):
                    self._direct.close()
                    self._direct = None
                    raise L.SocialWaysHipError("SW_ALLREDUCE=direct: the exchange disagrees with the process group's all-reduce "
                                               "on this node (or a wait timed out); use SW_ALLREDUCE=auto or unset it")
            else:
                self._direct, self.exchange_probe = comm.probe(self.pg, self.device, buckets)
            if self._direct is not None and self._graph_collectives is None:
                self._graph_collectives = bool(self.use_graph)
        self.ws = ops.Workspaces(self.device)
        self._ws_version = 0
        # derived images of the generator's weights (composed input matrix, fc4 . fc3, transposed decoder matrices):
        # computed once per step by the staging launch instead of by every workgroup of four launches (sw_gen_images)
        self._gimg = torch.empty(L.load().sw_gen_image_floats(), device=self.device) if self.device.type == "cuda" else None
        # ... and of the discriminator's (A-operand images of weight_hh / its transpose, the transposed head matrices in the
        # backward kernels' LDS layout): scattered by the staging launch, kept current by the kernels that apply D's Adam
        # update (sw_disc_images; include/socialways_hip.h)
        self._dimg = self._dtab = None
        if self.device.type == "cuda":
            lib = L.load()
            tab = np.empty((self.D._flat.numel(), 2), dtype=np.int32)
            if lib.sw_disc_image_table(n_next, tab.ctypes.data) != 0:
                raise L.SocialWaysHipError("sw_disc_image_table(%d)" % n_next)
            self._dtab = torch.from_numpy(tab).to(self.device)
            self._dimg = torch.zeros(lib.sw_disc_image_floats(n_next), device=self.device)    # padding stays zero for good
        self._lin_mask = None
        self._lin_maskf = None
        self._noise_src = None

    # ------------------------------------------------------------------------------------------
    @property
    def use_social(self):
        return self.G.use_social

    def sync_replicas(self):
        """Data-parallel replicas must start from identical weights and optimizer state: rank 0's are broadcast (at
        construction and after load_checkpoint).  The reference has one process; here a user who does not seed every
        rank identically would otherwise train diverging replicas on all-reduced gradients."""
        dist = torch.distributed
        src = dist.get_global_rank(self.pg, 0)
        bufs = [self.G._flat_all, self.D._flat]
        for o in (self.predictor_optimizer, self.D_optimizer):
            if isinstance(o, PackedAdam):
                bufs += [o.m, o.v]
            else:
                for st in o.state.values():
                    bufs += [st["exp_avg"], st["exp_avg_sq"]]
        for b in bufs:
            dist.broadcast(b, src, group=self.pg)
        ts = torch.tensor([float(getattr(o, "t", 0)) for o in (self.predictor_optimizer, self.D_optimizer)] + [float(self.epoch)],
                          device=self.device if dist.get_backend(self.pg) == "nccl" else "cpu")
        dist.broadcast(ts, src, group=self.pg)
        for o, t in zip((self.predictor_optimizer, self.D_optimizer), ts.tolist()):
            if isinstance(o, PackedAdam):
                o.t = int(t)
                o.step_t.fill_(float(o.t))
        self.epoch = int(ts[2].item())

    def sync_rng(self):
        """train.py:471-473 draws the label-noise scalars and z from the process-global numpy / torch generators.
        Every rank must draw the SAME values for a packed batch (z is sliced per shard): rank 0's generator states
        are broadcast once per epoch, so the job as a whole follows rank 0's stream - the stream a single process
        seeded like rank 0 would follow."""
        dist = torch.distributed
        obj = [(np.random.get_state(), torch.get_rng_state())] if self.rank == 0 else [None]
        dist.broadcast_object_list(obj, src=dist.get_global_rank(self.pg, 0), group=self.pg,
                                   device=self.device if dist.get_backend(self.pg) == "nccl" else None)
        if self.rank != 0:
            np.random.set_state(obj[0][0])
            torch.set_rng_state(obj[0][1])

    def _allreduce(self, flat):
        if self.pg is not None and (self.world > 1 or self._force_dist):
            d = self._direct
            if (d is not None and flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous()
                    and 1024 <= flat.numel() <= d.max_floats):
                d(flat)        # SW_ALLREDUCE=direct: the two-hop exchange over peer-mapped buffers (comm.py), a plain kernel
            else:
                torch.distributed.all_reduce(flat, op=torch.distributed.ReduceOp.SUM, group=self.pg)

    def _exchange_adam(self, opt, flat):
        """Does the direct exchange also apply this optimizer's update (sw_allreduce_direct_adam)?  A data-parallel step on
        SW_ALLREDUCE=direct with a packed, decay-free Adam."""
        return (self._direct is not None and (self.world > 1 or self._force_dist) and isinstance(opt, PackedAdam) and opt.native
                and opt.fusable and flat.numel() >= 1024)

    def _probe_graph_collectives(self):
        """Can this process group's all-reduce be recorded in a hipGraph and replayed?  Only RCCL ("nccl") is
        tried: a 4 KB SUM all-reduce is captured, replayed twice and compared with the known answer; every rank
        reports and the group takes the minimum, so all ranks choose the same step structure."""
        import ctypes
        import threading
        dev, W = self.device, self.world
        if torch.distributed.get_backend(self.pg) != "nccl":      # gloo & co. synchronise the stream: not capturable
            return False
        ok = 0.0
        # a collective that never completes would otherwise block forever in synchronize()
        guard = threading.Timer(180.0, lambda: (sys.stderr.write("socialways_amd: captured all-reduce probe hung; "
                                                                 "set SW_GRAPH_COLLECTIVES=0\n"), os._exit(3)))
        guard.daemon = True
        guard.start()
        x = torch.full((1024,), float(self.rank + 1), device=dev)
        y = torch.zeros_like(x)
        self._allreduce(y)          # eager first: connections / buffers of the communicator are set up outside capture
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                g.capture_begin(capture_error_mode="thread_local")
                try:
                    y.copy_(x)
                    self._allreduce(y)
                except Exception:
                    try:
                        g.capture_end()
                    except Exception:      # noqa: BLE001 - the capture is already invalid; make sure the stream left it
                        pass
                    hip, junk = ctypes.CDLL("libamdhip64.so"), ctypes.c_void_p()
                    hip.hipStreamEndCapture(ctypes.c_void_p(side.cuda_stream), ctypes.byref(junk))
                    hip.hipGetLastError()
                    raise
                g.capture_end()
                for _ in range(2):
                    g.replay()
            torch.cuda.synchronize()
            ok = float(bool((y == W * (W + 1) / 2.0).all()))
            del g
        except Exception as e:      # noqa: BLE001 - any failure means "do not record collectives"
            sys.stderr.write("socialways_amd: all-reduce not capturable here (%s: %s); using graph segments\n"
                             % (type(e).__name__, str(e).splitlines()[0] if str(e) else ""))
        finally:
            guard.cancel()
        torch.cuda.synchronize()
        flag = torch.tensor([ok], device=dev)
        torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN, group=self.pg)
        return bool(flag.item() > 0.5)

    def _resolve_collectives(self):
        """Every rank passes here at the start of every packed batch (step / step_many / _empty_step), so the
        probe's own collectives line up across the group even when some ranks have no scenes in a batch."""
        if self._graph_collectives is None and self.pg is not None and (self.world > 1 or self._force_dist):
            self._graph_collectives = bool(self.use_graph) and self._probe_graph_collectives()

    def release_graphs(self):
        """Drop every captured step graph (they hold the communicator's recorded collectives: release them before
        the process group is destroyed)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        self._graphs.clear()
        self.ws.release_retired()
        self._ws_version = self.ws.version

    def close(self):
        """End of this trainer's life: captured graphs dropped, the direct exchange's buffers freed and its peer mappings
        closed (collective when a direct exchange exists: every rank calls it).  Idempotent."""
        self.release_graphs()
        d, self._direct = self._direct, None
        if d is not None:
            d.close()

    def _z_resident(self, batches):
        """Is the z of every step of this launch a contiguous fp32 device tensor of the kernels' width?  Then the
        staging kernel reads it from HBM through its pointer (sw_stage_step_zdev) instead of pulling its values over PCIe."""
        return all(nz.is_cuda and nz.dtype == torch.float32 and nz.is_contiguous() and nz.device == self.device
                   and tuple(nz.shape) == (b[0].shape[0], self.Z_COLS) for b in batches for nz in (b[4],))

    def _graph_key(self, scenes, To, ss, Bg, K, zdev=False, ragged=False):
        """Everything a captured step bakes in besides the buffer addresses: the scene layout, the loss switches and
        weights, the unrolling depth and the optimizer hyper-parameters (host-side scalars of the recorded launches)."""
        og, od = self.predictor_optimizer.param_groups[0], self.D_optimizer.param_groups[0]
        return (scenes.key, To, float(ss), float(Bg), self._row0, K, self.n_unrolling_steps, self.use_info_loss,
                self.loss_info_w, self.use_l2_loss, self.use_variety_loss, self.loss_l2_w, self.variety_k,
                og["lr"], tuple(og["betas"]), og["eps"], og.get("weight_decay", 0), od["lr"], tuple(od["betas"]), od["eps"],
                od.get("weight_decay", 0), _wall_key(getattr(self, "wall_loss", None)), getattr(self, "clearance_loss", None),
                ops.scene_wg(scenes, self.use_social, ragged), bool(ragged), bool(zdev))

    def _graphs_current(self):
        """A workspace outgrown since the last capture means captured graphs hold retired addresses: they stay valid
        (the retired tensors are alive) but pin memory, so all graphs are dropped and re-captured on the new buffers."""
        if self._ws_version != self.ws.version:
            self.release_graphs()

    def step(self, obsv, pred, sub_batches, zeros_val, ones_val, noise, ss=1.0, global_B=None, out=None, global_row0=0,
             variety_noise=None, obs_len=None):
        """One packed batch (train.py:458-554) on this rank's rows.  obsv (B,To,2), pred (B,Tp,2) and
        noise (B,32) are tensors (noise normally lives on the host, like train.py:473); `global_B` = agents
        of the whole packed batch over all ranks.
        Returns a (U+3, 3) float64 device tensor: rows = the U+1 D updates, the G phase, ADE/FDE; loss rows
        hold SUMS of squared errors over the local rows [label_a, code, label_b], the last row
        [sum err / Tp, sum err[:, -1], sum err^2].  The kernels leave one partial triple per 16-agent tile
        (no reduction kernels on the critical path); they are summed here in float64.  `out=False` returns
        the raw (U+3, tiles, 3) partials without that extra reduction (bench loop).
        With `use_graph` the whole step - ~35 kernels incl. the input staging and the Adam updates - is
        captured once per batch layout into a hipGraph and replayed: per step the host only fills a pinned
        slot (pointers of the track slices, z, the two label-noise scalars) and launches the graph.
        obs_len (B,) - tensor, numpy array or list: ragged histories.  Row a holds obs_len[a] valid frames, 2 .. To,
        right-aligned in obsv and trains exactly as if its two observation LSTMs (encoder, discriminator) ran on those
        frames alone from the zero state; the padding is never read.  By default such a step runs eagerly, never through a
        captured graph, on the unfused route: no precomputed D observation pass, D updates as disc_forward + disc_backward_gan
        (with the fused Adam), the generator phase as disc_dpred (or, where Tp > 24, disc_forward + disc_backward_gan),
        never inside the decode BPTT launch; the backward launches, losses and all-reduce points are the dense step's.
        With `ragged_fused` every D update is one launch wherever the dense step's is (ops.disc_update(obs_len=...): the same
        bits) and, with `use_graph` (not the "fixed" variety step), the step is captured per layout like the dense one - a
        graph of its own beside the layout's dense graph, obs_len travelling by address through the pinned slot
        (sw_stage_step_ragged), an obs_len given as a device tensor never read by the host.  Still out: the D observation
        pass inside the decode forward launch and the generator-phase D pass inside the decode BPTT launch."""
        _wall_reach(self.wall_loss, ss)
        self._resolve_collectives()
        B = obsv.shape[0]
        self._obs_len = None        # read by _step_body of this step only
        if obs_len is not None:
            if obsv.shape[2] != 2:
                raise ValueError("step(obs_len=...) takes positions (B, To, 2)")
            obs_len = ops.obs_len_arg(obs_len, B, obsv.shape[1], 2, self.device)
        Bg = float(global_B if global_B is not None else B)
        dev = self.device
        self._row0 = int(global_row0)       # first row of this rank's shard in the packed batch (variety term only)
        if self.use_variety_loss is True and Bg < 20:
            raise ValueError("use_variety_loss indexes agent 19 of the packed batch (train.py:531): batch of %d" % Bg)
        self._vnoise = None
        if self.use_variety_loss == "fixed":          # z of the samples 1..K-1: ((K-1)*B, 32), drawn like train.py:473 if not given
            vn = variety_noise if variety_noise is not None else torch.rand((self.variety_k - 1) * B, self.noise_len)
            if vn.dim() != 2 or vn.shape[0] != (self.variety_k - 1) * B or vn.shape[1] not in (self.noise_len, self.Z_COLS):
                raise ValueError("variety_noise must be ((variety_k - 1) * B, %d)" % self.noise_len)
            self._vnoise = self._pad_z(vn.to(dev, non_blocking=True)).contiguous()
        part = None
        if not self._graphs and self.ws.retired:      # eager-only runs: nothing captured can reference an outgrown workspace
            self.ws.release_retired()                 # (stream-ordered allocator: kernels already queued on it stay valid)
        # the folded K-sample step runs eagerly, and so does the ragged step without `ragged_fused`
        if self.use_graph and self.use_variety_loss != "fixed" and (obs_len is None or self.ragged_fused):
            # one graph set per packed-batch layout; datasets with ragged scenes produce many layouts, so the
            # number of captured layouts is capped and the rest of the steps run eagerly
            scenes = ops.SceneIndex.get(sub_batches, B, dev)
            self._graphs_current()
            zdev = self._z_resident([(obsv, pred, zeros_val, ones_val, noise)])
            key = self._graph_key(scenes, obsv.shape[1], ss, Bg, 1, zdev, obs_len is not None)
            if key in self._graphs or len(self._graphs) < self.max_graphs:
                part = self._step_graph([(obsv, pred, zeros_val, ones_val, noise)], sub_batches, float(ss), Bg,
                                        None if obs_len is None else [obs_len])[0]
        if part is None:
            part = torch.zeros(self.n_unrolling_steps + 3, (B + 15) // 16, 3, device=dev)     # one triple per 16-agent tile
            scenes = ops.SceneIndex.get(sub_batches, B, dev)
            noise = self._pad_z(noise.to(dev, non_blocking=True)).contiguous()
            # label-noise scalars of train.py:471-472 live in device memory: [zeros_val, ones_val]
            targets = torch.tensor([float(zeros_val), float(ones_val)], dtype=torch.float32).to(dev, non_blocking=True)
            self._obs_len = obs_len
            try:
                self._step_impl(obsv.contiguous(), pred.contiguous(), None, scenes, targets, noise, float(ss), Bg, part)
            finally:
                self._obs_len = None
        if out is False:           # caller reads the static partials before the next step overwrites them
            return part
        return part.sum(1, dtype=torch.float64)

    def step_many(self, batches, sub_batches, ss=1.0, global_B=None, out=None, global_row0=0, **ragged):
        """K consecutive training steps on K packed batches of the SAME scene layout in ONE graph launch:
        `batches` = [(obsv, pred, zeros_val, ones_val, noise), ...].  Exactly the K `step()` calls in order (same
        kernels, same results); what it saves is the gap between two graph launches (~13 us, the system-scope
        fence at the end of a hipGraph) on K-1 of the K steps.  Returns the list of the K step results.
        obs_len: a list of the K batches' obs_len (ragged histories, see step()) or None.  With `ragged_fused` and
        `use_graph` the K ragged steps are one graph launch; otherwise they are K step(obs_len=...) calls.  It is the one
        keyword `**ragged` takes: the named parameters are the dense call's, as tests/test_ragged_train_host.py pins them."""
        obs_len = ragged.pop("obs_len", None)
        if ragged:
            raise TypeError("step_many() got an unexpected keyword argument %r" % sorted(ragged)[0])
        if obs_len is not None:       # checked before anything of the trainer is touched
            obs_len = list(obs_len)
            if len(obs_len) != len(batches):
                raise ValueError("step_many(obs_len=...) takes one obs_len per batch: %d for %d batches" % (len(obs_len), len(batches)))
            n_none = sum(ol is None for ol in obs_len)
            if 0 < n_none < len(obs_len):
                raise ValueError("step_many(obs_len=...) takes an obs_len for every batch or None, not a mix of both")
            if n_none:
                obs_len = None
        _wall_reach(self.wall_loss, ss)
        self._resolve_collectives()
        ols = obs_len if obs_len is not None else [None] * len(batches)

        def steps():
            return [self.step(o, p, sub_batches, zv, ov, nz, ss, global_B, out, global_row0, obs_len=ol)
                    for (o, p, zv, ov, nz), ol in zip(batches, ols)]
        if not self.use_graph or len(batches) == 1 or self.use_variety_loss or (obs_len is not None and not self.ragged_fused):
            return steps()
        B, To = batches[0][0].shape[0], batches[0][0].shape[1]
        if obs_len is not None:
            if any(b[0].shape[2] != 2 for b in batches):
                raise ValueError("step_many(obs_len=...) takes positions (B, To, 2)")
            obs_len = [ops.obs_len_arg(ol, B, To, 2, self.device) for ol in obs_len]
        Bg = float(global_B if global_B is not None else B)
        self._row0 = int(global_row0)
        scenes = ops.SceneIndex.get(sub_batches, B, self.device)
        self._graphs_current()
        key = self._graph_key(scenes, To, ss, Bg, len(batches), self._z_resident(batches), obs_len is not None)
        if key not in self._graphs and len(self._graphs) >= self.max_graphs:
            return steps()
        self._obs_len = None
        parts = self._step_graph(batches, sub_batches, float(ss), Bg, obs_len)
        return parts if out is False else [q.sum(1, dtype=torch.float64) for q in parts]

    def _step_graph(self, batches, sub_batches, ss, Bg, obs_lens=None):
        """obs_lens: the K batches' obs_len as int32 device tensors (the captured ragged step, `ragged_fused`) or None."""
        K = len(batches)
        B, To, Tp = batches[0][0].shape[0], batches[0][0].shape[1], self.n_next
        dev = self.device
        scenes = ops.SceneIndex.get(sub_batches, B, dev)
        zdev = self._z_resident(batches)
        ragged = obs_lens is not None
        key = self._graph_key(scenes, To, ss, Bg, K, zdev, ragged)
        st = self._graphs.get(key)
        HDR = 12 if ragged else 8                                 # SW_STAGE_HEADER[_RAGGED] words in front of z
        if st is None:
            st = self._graphs[key] = dict(
                n=0, graph=None, flip=0, scenes=scenes, obsv=torch.empty(B, To, 2, device=dev),
                pred=torch.empty(B, Tp, 2, device=dev), pred4=torch.empty(B, Tp, 4, device=dev),
                targets=torch.empty(4, device=dev), noise=torch.zeros(B, self.Z_COLS, device=dev),
                steps=torch.zeros(self.n_unrolling_steps + 2, device=dev),   # Adam step indices of the U+1 D updates, the G update
                outs=[torch.zeros(self.n_unrolling_steps + 3, (B + 15) // 16, 3, device=dev) for _ in range(K)],
                slots=[[torch.zeros(HDR + B * self.Z_COLS, dtype=torch.float32).pin_memory() for _ in range(K)]
                       for _ in range(2)],
                done=[torch.cuda.Event(), torch.cuda.Event()], keep=[None, None],
                # the ragged graph's static obs_len (clamped by the staging launch), read by its ragged kernels
                obs_len=torch.full((B,), To, dtype=torch.int32, device=dev) if ragged else None)
        # Inputs of a step travel through a pinned host slot that the step's first graph node (sw_stage_step)
        # reads itself: the device pointers of this batch's track slices, the two label-noise scalars, the Adam
        # counters and z.  A hipMemcpyAsync enqueued behind graph launches would block the host until the stream
        # drains; a kernel reading device-mapped host memory does not.  One slot per (graph executable, sub-step).
        k = (st["flip"] ^ 1) if st["graph"] is not None else 0
        st["done"][k].synchronize()                            # the replay that last read these slots has finished
        packed = isinstance(self.D_optimizer, PackedAdam)
        keep = []
        for j, (obsv, pred, zeros_val, ones_val, noise) in enumerate(batches):
            obsv, pred = obsv.contiguous(), pred.contiguous()
            keep.append((obsv, pred))                          # alive until the slot is rewritten
            hn = st["slots"][k][j].numpy()
            hn[:4].view(np.uint64)[:] = (obsv.data_ptr(), pred.data_ptr())
            hn[4], hn[5] = float(zeros_val), float(ones_val)
            if ragged:        # this step's obs_len travels by address, like the tracks
                hn[10:12].view(np.uint64)[:] = obs_lens[j].data_ptr()
                keep.append(obs_lens[j])
            if packed:        # updates applied so far: the staging kernel turns them into this step's Adam step indices
                hn[6], hn[7] = float(self.D_optimizer.t), float(self.predictor_optimizer.t)
                self.D_optimizer.t += self.n_unrolling_steps + 1
                self.predictor_optimizer.t += 1
            if zdev:          # z already in HBM: only its address travels
                hn[8:10].view(np.uint64)[:] = noise.data_ptr()    # words [8, 9] in both slot layouts
                keep.append(noise)
                continue
            # (a hidden size below 64 draws fewer z columns: the kernels' remaining columns stay zero, like their weights)
            np.copyto(hn[HDR:].reshape(B, self.Z_COLS)[:, :self.noise_len], (noise.cpu() if noise.is_cuda else noise).numpy())
        st["keep"][k] = keep

        def stage(kk, j):
            slot = st["slots"][kk][j]
            if ragged:        # the ragged encoder launch pulls no z: the staging launch fills it in both z modes
                L.call("sw_stage_step_ragged", slot.data_ptr(), B, To, Tp, L.ptr(st["obsv"]), L.ptr(st["pred"]),
                       L.ptr(st["pred4"]), L.ptr(st["targets"]), L.ptr(st["noise"]), L.ptr(st["steps"]),
                       self.n_unrolling_steps + 1,
                       L.ptr(self.G.encoder._flat), L.ptr(self.G.decoder._flat), L.ptr(self.G.feature_embedder._flat),
                       L.ptr(self.G.attention._flat), L.ptr(self._gimg),
                       L.ptr(self.D._flat) if self._dimg is not None else None, L.ptr(self._dimg), L.ptr(self._dtab), int(zdev),
                       L.ptr(st["obs_len"]), L.stream())
                self._noise_src = None
                return
            L.call("sw_stage_step_zdev", slot.data_ptr(), B, To, Tp, L.ptr(st["obsv"]), L.ptr(st["pred"]),
                   L.ptr(st["pred4"]), L.ptr(st["targets"]), L.ptr(st["noise"]) if zdev else None, L.ptr(st["steps"]),
                   self.n_unrolling_steps + 1,
                   L.ptr(self.G.encoder._flat), L.ptr(self.G.decoder._flat), L.ptr(self.G.feature_embedder._flat),
                   L.ptr(self.G.attention._flat), L.ptr(self._gimg),
                   L.ptr(self.D._flat) if self._dimg is not None else None, L.ptr(self._dimg), L.ptr(self._dtab), int(zdev),
                   L.stream())
            # z in host memory: pulled by idle workgroups of the encoder launch; z in HBM: copied by this staging launch
            self._noise_src = None if zdev else slot.data_ptr() + 4 * HDR

        def args(j):
            return (st["obsv"], st["pred"], st["pred4"], scenes, st["targets"], st["noise"], ss, Bg, st["outs"][j],
                    st["steps"] if packed else None)

        def one_step(j, pre=None):   # its segments; a ragged graph's kernels read its static obs_len (_step_body)
            self._obs_len = st["obs_len"]
            try:
                yield from self._step_gen(*args(j), pre=pre)
            finally:
                self._obs_len = None

        def body(kk):          # the K steps of one executable, back to back
            for j in range(K):
                yield from one_step(j, pre=lambda j=j: stage(kk, j))
        replayed = st["graph"] is not None
        if replayed:
            st["flip"] = k
            for g, buf in st["graph"][k]:
                g.replay()
                if buf is not None:
                    self._allreduce(buf)
            self.last_clearance = st["clearance"]              # the replayed launches wrote the buffers the capture saw
            self.last_wall_loss = st["wall_loss"]
        elif st["n"] < 2:          # first steps of a layout run eagerly (lazy inits, workspace growth)
            st["n"] += 1
            for j in range(K):
                stage(0, j)
                for buf in one_step(j):
                    self._allreduce(buf)
        else:
            # Capture.  Single GPU: one graph for the K steps.  Data parallel: the same with the RCCL
            # all-reduces recorded in it when the group can do that (see __init__), else one graph per
            # segment between the all-reduce points with the collectives run eagerly in between, all
            # segments sharing one memory pool so intermediates stay alive.
            # Everything is captured TWICE and the two executables alternate: launching an executable
            # that is still running makes hipGraphLaunch wait for it, which would put the host-side
            # launch cost (~150 us for ~40 nodes) on the critical path of every step.
            torch.cuda.synchronize()
            pool, sets = None, []
            for kk in range(2):
                gen = body(kk)
                graphs, fin = [], False
                while not fin:
                    g = torch.cuda.CUDAGraph()
                    # thread_local: other threads (the RCCL watchdog) may touch the runtime during capture
                    with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                        while True:
                            try:
                                buf = next(gen)
                            except StopIteration:
                                buf, fin = None, True
                            if fin:
                                break
                            if self.world > 1 or self._force_dist:
                                if not self._graph_collectives:
                                    break                      # segment boundary: the all-reduce runs eagerly
                                self._allreduce(buf)           # opt-in: RCCL all-reduce recorded inside the graph
                    graphs.append((g, buf))
                    pool = g.pool()
                sets.append(graphs)
            st["graph"], st["flip"] = sets, 0
            for g, buf in sets[0]:     # capture only records: this replay IS the step
                g.replay()
                if buf is not None:
                    self._allreduce(buf)
        if not replayed:
            st["clearance"] = self.last_clearance              # set by _step_body (eager warm-up steps and the capture)
            st["wall_loss"] = self.last_wall_loss
        st["done"][k].record()
        return st["outs"]

    def _step_impl(self, obsv, pred, pred4, scenes, targets, noise, ss, Bg, out, steps=None):
        """Eager step: run the segments, all-reducing the packed gradient buffer each one hands back."""
        for buf in self._step_gen(obsv, pred, pred4, scenes, targets, noise, ss, Bg, out, steps):
            self._allreduce(buf)
        return out

    def _step_gen(self, obsv, pred, pred4, scenes, targets, noise, ss, Bg, out, steps=None, pre=None):
        """Device-only body of the step (no host syncs, no host-dependent values: capturable) as a
        generator: it yields the packed gradient buffer at each of the 3 points where data-parallel
        ranks must all-reduce before the optimizer step (D, D, G).  `out` (U+3, tiles, 3) receives the
        per-tile loss / ADE partial sums; `steps` (U+2 device scalars) = the Adam step indices of this
        step's updates when the staging kernel provides them; `pre` = the input staging of a captured step."""
        G, D = self.G, self.D
        B, Tp = obsv.shape[0], self.n_next
        dev = self.device
        ws = self.ws
        U = self.n_unrolling_steps
        g_label = 1.0 / Bg
        g_code = (self.loss_info_w if self.use_info_loss else 0.0) / (2.0 * Bg)
        # One stream: inside a hipGraph every cross-stream edge costs 5-10 us of queue synchronisation on
        # this runtime - more than any of the small kernels that could be overlapped (measured).
        if pre is not None:
            pre()
        else:                            # eager step without a staging launch: derive the weight images here
            if self._gimg is not None:
                L.call("sw_gen_images", L.ptr(G.encoder._flat), L.ptr(G.decoder._flat), L.ptr(G.feature_embedder._flat),
                       L.ptr(G.attention._flat), L.ptr(self._gimg), L.stream())
            self._disc_images()
        try:
            yield from self._step_body(obsv, pred, pred4, scenes, targets, noise, ss, Bg, out, steps)
        finally:
            if self._gimg is not None:   # the generator's Adam step follows / has run: the images are stale
                L.call("sw_gen_images", None, None, None, None, None, None)
            if self._dimg is not None:   # D.load(backup) has run (train.py:541-542) / the weights are the caller's again
                L.call("sw_disc_images", None, None, None, 0, None)

    def _disc_images(self):
        """(Re-)scatter the packed D weights into their images and register them (sw_disc_images)."""
        if self._dimg is not None:
            L.call("sw_disc_images", L.ptr(self.D._flat), L.ptr(self._dimg), L.ptr(self._dtab), self.n_next, L.stream())

    def _step_body(self, obsv, pred, pred4, scenes, targets, noise, ss, Bg, out, steps):
        G, D = self.G, self.D
        B, Tp = obsv.shape[0], self.n_next
        dev = self.device
        ws = self.ws
        U = self.n_unrolling_steps
        g_label = 1.0 / Bg
        g_code = (self.loss_info_w if self.use_info_loss else 0.0) / (2.0 * Bg)
        noise_src, self._noise_src = self._noise_src, None      # set by the staging of this step (graph / warm-up path)
        ol = getattr(self, "_obs_len", None)                    # ragged histories (step(obs_len=...))
        if pred4 is None:          # real future as 4-d (train.py:470); the observation stays 2-d: kernels form (p, v) on the fly
            pred4 = torch.empty(B, Tp, 4, device=dev)
            o4_scratch = ws.get("o4", B * obsv.shape[1] * 4)
            L.call("sw_traj_4d", L.ptr(obsv), L.ptr(pred), B, obsv.shape[1], Tp, L.ptr(o4_scratch), L.ptr(pred4), L.stream())
        # ---- generator rollout, once (train.py:480/507 are identical) ---------------
        enc, emb, att, dec = G.encoder, G.feature_embedder, G.attention, G.decoder
        KV = self.variety_k if self.use_variety_loss == "fixed" else 1
        if KV > 1:
            # best-of-K variety term: the K rollouts are K copies of the scenes in one batch; copy 0 (the step's own z)
            # is the prediction every other loss term and the ADE/FDE sums see
            # (the encoder over the observed steps and the social pooling do not depend on z: once for all K copies)
            pred_hat_k, gctx = ops.gen_forward_k(enc._flat, emb._flat, att._flat, dec._flat, obsv,
                                                 torch.cat([noise, self._vnoise]), scenes, Tp, G.use_social, KV, ws=ws, obs_len=ol)
            pred_hat = pred_hat_k[:B]
            out[U + 2].zero_()
            L.call("sw_ade_fde", L.ptr(pred_hat), L.ptr(pred), B, Tp, 1.0 / float(ss), L.ptr(out[U + 2]),
                   L.ptr(ws.get("ade_scratch", 3 * L.RED_BLOCKS)), L.stream())
            d_pre = None
        else:
            # the decode kernel also leaves the ADE/FDE partial sums of the prediction (train.py:546-551)
            # ... and, while it leaves CUs idle, the observation LSTM of the first D pass (independent of the generator)
            d_pre = ops.d_obs_buffer(ws, B, obsv.shape[1], Tp) if obsv.shape[2] == 2 and ol is None else None
            pred_hat, gctx = ops.gen_forward(enc._flat, emb._flat, att._flat, dec._flat, obsv, noise, scenes, Tp,
                                             G.use_social, save=True, ws=ws, ade=(pred, 1.0 / float(ss), out[U + 2]),
                                             noise_src=noise_src, d_obs=(D._flat, d_pre) if d_pre is not None else None,
                                             obs_len=ol)
        d_gflat = D.grad_views()
        backup = None
        # ---- discriminator updates (train.py:476-499) ------------------------------------------------
        for u in range(self.n_unrolling_steps + 1):
            if u == 1:     # deepcopy(D) after the first update (train.py:498-499) = the weights of this forward pass
                backup = ws.get("d_backup", D._flat.numel())
            # the loss gradients AND the reported loss sums (per-tile partials) are formed inside the backward kernel;
            # in a single process (no all-reduce between gradient and update) D's Adam step rides in the kernel that
            # finishes the gradients
            fuse = (self._fuse_d_adam and isinstance(self.D_optimizer, PackedAdam) and self.D_optimizer.fusable
                    and not (self.world > 1 or self._force_dist))
            adam = self.D_optimizer.fused_args(None if steps is None else steps[u]) if fuse else None
            if ((ol is None or self.ragged_fused) and obsv.shape[2] == 2
                    and ops.disc_update_supported(D._flat, B, obsv.shape[1], Tp)):
                # shapes that leave CUs idle: forward + loss gradients + backward of the pass in ONE launch (sw_disc_update;
                # ragged histories with `ragged_fused`: sw_disc_update_ragged)
                ops.disc_update(D._flat, obsv, [pred_hat, pred4], targets, (0, 1), noise, g_label, g_code, d_gflat, ws,
                                obs_pre=(u == 0 and d_pre is not None), w_snapshot=backup if u == 1 else None,
                                loss_part=out[u], adam=adam, obs_len=ol)
            else:
                labels, codes, dctx = ops.disc_forward(D._flat, obsv, [pred_hat, pred4], save=True, ws=ws,
                                                       save_lstm=2 if (u == 0 and d_pre is not None) else 1,
                                                       w_snapshot=backup if u == 1 else None, obs_len=ol)
                ops.disc_backward_gan(D._flat, dctx, labels, codes, targets, (0, 1), noise, g_label, g_code, d_gflat, (), ws=ws,
                                      loss_part=out[u], adam=adam)
            if self._exchange_adam(self.D_optimizer, d_gflat):
                # SW_ALLREDUCE=direct: gradient exchange + D's Adam update in ONE launch (no all-reduce point to hand back)
                self._direct.adam(d_gflat, self.D_optimizer, None if steps is None else steps[u])
                continue
            yield d_gflat
            if not fuse:
                self.D_optimizer.step() if steps is None else self.D_optimizer.step(steps[u])
                if not getattr(self.D_optimizer, "keeps_images", False):
                    self._disc_images()        # an update the image table did not see (torch's Adam): scatter again
        # ---- generator update (train.py:503-539) ----------------------------------------------------
        # D forward on the prediction + backward of its heads down to d(g_loss)/d(pred_hat), one launch, nothing saved
        # ... which is tile-local and feeds only the decode BPTT of the same tile: in the plain step (no extra terms on
        # d/d(pred_hat)) it runs inside that launch (ops.gen_backward(dfuse=...): one graph node less)
        # ... when its LDS fits one workgroup (Tp <= 24); longer horizons run the forward with saves and the backward of
        # the heads as two launches (same d/d(pred_hat), same loss sums)
        dfuse = None
        one_pass = ops.disc_dpred_supported(Tp)
        clr = self.clearance_loss                               # an extra term on d/d(pred_hat), like use_l2_loss
        wall = self.wall_loss                                   # ... and another (set_wall_loss())
        if (ops.DFUSE and one_pass and KV == 1 and not self.use_l2_loss and self.use_variety_loss is False
                and obsv.shape[2] == 2 and ol is None and clr is None and wall is None):
            dfuse = (D._flat, pred_hat, targets, 1, noise, g_label, g_code, out[U + 1])
        dpred = None
        if dfuse is None and one_pass:
            dpred = ops.disc_dpred(D._flat, obsv, pred_hat, targets, 1, noise, g_label, g_code, loss_part=out[U + 1], obs_len=ol)
        elif dfuse is None:
            labels, codes, dctx = ops.disc_forward(D._flat, obsv, [pred_hat], save=True, ws=ws, save_lstm=0, obs_len=ol)
            dpred = ops.disc_backward_gan(D._flat, dctx, labels, codes, targets, (1,), noise, g_label, g_code, None, (True,),
                                          ws=ws, loss_part=out[U + 1])[0]
        if self.use_l2_loss:                                                 # train.py:525-526
            L.call("sw_l2_grad", L.ptr(pred_hat), L.ptr(pred), B, Tp, 0, B, self.loss_l2_w / (Bg * Tp), L.ptr(dpred), L.stream())
        if self.use_variety_loss is True:                                    # train.py:527-536 as written
            r = 19 - self._row0
            if 0 <= r < B:
                L.call("sw_l2_grad", L.ptr(pred_hat), L.ptr(pred), B, Tp, r, r + 1, self.loss_l2_w / Tp, L.ptr(dpred), L.stream())
        if KV > 1:                                                           # ... and with its intended semantics
            dk = torch.zeros(KV * B, Tp, 4, device=dev)
            dk[:B].copy_(dpred)
            l2min, kmin = torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
            L.call("sw_variety_grad", L.ptr(pred_hat_k), L.ptr(pred), KV, B, Tp, self.loss_l2_w / (Bg * Tp), L.ptr(dk),
                   L.ptr(kmin), L.ptr(l2min), L.stream())
            self.last_variety = (l2min, kmin)
            dpred = dk
        self.last_clearance = None
        if clr is not None:
            # the scene-clearance term (set_clearance_loss()) on the prediction every other term sees (copy 0 of the K-sample
            # step): rows [0, B).  Its outputs live in the workspace so that a replayed graph finds them where it was captured.
            closs, ccount = ws.get("clr_loss", B)[:B], ws.get("clr_count", B)[:B].view(torch.int32)
            ops.clearance_grad(pred_hat, obsv[:, -1], scenes, clr[0] * float(ss), clr[1] / (Bg * Tp), dpred[:B], closs, ccount)
            self.last_clearance = (closs, ccount)
        self.last_wall_loss = None
        if wall is not None:
            # the wall term (set_wall_loss()), on the same prediction and rows; its outputs live in the workspace likewise
            wloss, wcount = ws.get("wall_loss", B)[:B], ws.get("wall_count", B)[:B].view(torch.int32)
            ops.wall_grad(pred_hat, obsv[:, -1], 1, wall[0], wall[1] * float(ss), wall[2] / (Bg * Tp), dpred[:B], wloss, wcount)
            self.last_wall_loss = (wloss, wcount)
        restore = None
        if self.n_unrolling_steps > 0:     # D.load(backup) restores the Linear layers only (train.py:311-316, 541-542); D is
            if self._lin_maskf is None:    # not read again in this step: done by idle workgroups of the decode BPTT launch
                self._lin_maskf = D.linear_mask().float().contiguous()
            restore = (backup[:D._flat.numel()], D._flat, self._lin_maskf)
        G.grad_views()
        # Single process: the generator's Adam step rides in the two kernels that finish its gradients (the reduction of
        # the grouped GEMM and the composition back-propagation; the latter reads the step-start weight snapshot of the
        # image buffer).  Without social problems in the launch the attention / embedder weights would miss their
        # (zero-gradient) update: torch's kernel then.
        fuse = (KV == 1 and self._fuse_g_adam and self._gimg is not None and isinstance(self.predictor_optimizer, PackedAdam)
                and self.predictor_optimizer.fusable and not (self.world > 1 or self._force_dist)
                and (not G.use_social or gctx.scenes.P > 0 or gctx.scenes.NB > 0))
        adam = None
        if fuse:
            opt = self.predictor_optimizer
            adam = (G._flat_all, G._gflat_all) + opt.fused_args(None if steps is None else steps[U + 1])
        if KV > 1:
            ops.gen_backward_k(enc._flat, emb._flat, att._flat, dec._flat, gctx, dpred, enc._gflat, emb._gflat, att._gflat,
                               dec._gflat, ws=ws, aux=restore)
        else:
            ops.gen_backward(enc._flat, emb._flat, att._flat, dec._flat, gctx, dpred, enc._gflat, emb._gflat, att._gflat,
                             dec._gflat, ws=ws, aux=restore, tag="g", adam=adam, dfuse=dfuse)
        if self._exchange_adam(self.predictor_optimizer, G._gflat_all):
            self._direct.adam(G._gflat_all, self.predictor_optimizer, None if steps is None else steps[U + 1])
        else:
            yield G._gflat_all
            if not fuse:
                self.predictor_optimizer.step() if steps is None else self.predictor_optimizer.step(steps[U + 1])
        self.last_pred_hat = pred_hat
        self.last_pred_hat_k = pred_hat_k if KV > 1 else None

    # ------------------------------------------------------------------------------------------
    def losses_from(self, out, B_global, Tp=None, ss=1.0):
        """(n_steps, U+3, 3) sums -> the reference's MSE terms in its order
        [d_fake, d_info, d_real] x (U+1), [g_l2, g_fool, g_info] per step (train.py:484-488,512-516)."""
        o = out.detach().double().cpu().numpy()
        if o.ndim == 2:
            o = o[None]
        Bg = np.asarray(B_global, dtype=np.float64).reshape(-1, 1)
        U = self.n_unrolling_steps + 1
        Tp = Tp or self.n_next
        cols = []
        for u in range(U):
            cols += [o[:, u, 0:1] / Bg, o[:, u, 1:2] / (2 * Bg), o[:, u, 2:3] / Bg]
        cols += [o[:, U + 1, 2:3] * (ss * ss) / (2 * Tp * Bg), o[:, U, 0:1] / Bg, o[:, U, 1:2] / (2 * Bg)]
        return np.concatenate(cols, axis=1)

    def train_epoch(self, data, batch_size, draw=None):
        """train() (train.py:439-557).  `draw(bs)` -> (zeros_val, ones_val, noise_cpu) overrides the
        RNG draws of train.py:471-473 (tests feed the reference's recorded values).
        With `self.noise` (a DeviceNoise) and no `draw`, z comes from the device stream's training domain: step =
        noise.step, counted once per packed batch on every rank; draw 0 = the step's z, draws 1 .. variety_k-1 the extra
        samples of use_variety_loss="fixed"; row = the row in the GLOBAL packed batch, so a rank fills only its shard and
        the union over ranks is the single-process z.  The z of the batches that share a step_many launch is one fill
        launch in front of the graph launch on the same stream, read by the steps through their z-resident path (no
        pinned-slot copy).  The label-noise scalars stay the reference's two host draws.
        A dataset with obs_len (ragged histories) is refused: its steps run eagerly through train_epoch_ragged()."""
        _refuse_pred_len(data, "train_epoch()", _PRED_LEN_TRAIN)
        _refuse_ragged(data, "train_epoch()", "its graph-captured steps have no ragged form - train on the ragged windows with "
                       "train_epoch_ragged(), or on full windows (create_dataset) and evaluate the ragged ones with "
                       "evaluate*() / evaluate_history()")
        return self._train_epoch(data, batch_size, draw, None)

    def train_epoch_ragged(self, data, batch_size, draw=None):
        """train_epoch() for a dataset that carries obs_len (create_dataset_ragged / SceneDataset(obs_len=...)): the same
        packed batches, RNG draws (host stream or `self.noise`), scene sharding, return value and epoch counter, one eager
        step(..., obs_len=data.obs_len[rows]) per packed batch (see step(): the unfused route, no graph capture).
        With `ragged_fused` and `use_graph` (not the "fixed" variety step) the loop is train_epoch()'s: consecutive packed
        batches of one local layout share a step_many(obs_len=[...]) launch of up to STEPS_PER_LAUNCH captured ragged steps,
        with `self.noise` one fill launch in front of it - the same weights and return values bit for bit.
        A dataset without obs_len is refused: train_epoch() is its call; so is one with pred_len (ragged futures)."""
        _refuse_pred_len(data, "train_epoch_ragged()", _PRED_LEN_TRAIN)
        ol = getattr(data, "obs_len", None)
        if ol is None:
            raise L.SocialWaysHipError("train_epoch_ragged() needs a dataset with obs_len (create_dataset_ragged, "
                                       "SceneDataset(obs_len=...)): train a dataset of full windows with train_epoch()")
        return self._train_epoch(data, batch_size, draw, ol)

    def _train_epoch(self, data, batch_size, draw, obs_len):
        """The epoch loop of train_epoch() (obs_len None) and train_epoch_ragged() (obs_len = data.obs_len)."""
        outs, sizes = [], []
        pend, pend_key = [], None        # consecutive packed batches of one layout share a graph launch
        dn = self._device_noise(None) if draw is None else None
        if self.world > 1 and draw is None:
            self.sync_rng()
        if self._direct is not None and self.world > 1:
            # the exchange kernels WAIT for their peers on the device (bounded: SW_COMM_TIMEOUT_S): ranks enter an epoch
            # together, whatever one of them did alone in between (test(), save(), a capture)
            torch.distributed.barrier(group=self.pg)

        def flush():
            nonlocal pend, pend_key
            if pend:
                items = [p[0] for p in pend]
                if dn is not None:      # the z of these consecutive steps: one fill launch in front of their graph launch
                    r0 = pend[0][3]
                    z = dn.fill(items[0][0].shape[0], self.noise_len, domain=TRAIN, step=pend[0][4], n_steps=len(pend), row0=r0,
                                ld=self.Z_COLS, device=self.device)
                    items = [it[:4] + (z[j, 0],) for j, it in enumerate(items)]
                kw = dict(obs_len=[p[5] for p in pend]) if obs_len is not None else {}     # (the wider trainers' step_many has none)
                outs.extend(self.step_many(items, pend[0][1], data.ss, global_B=pend[0][2], global_row0=pend[0][3], **kw))
                pend, pend_key = [], None
        for a, b, sb in data.packed_steps(batch_size):
            bs = b - a
            vn = step_i = None
            if draw is None:
                zv = np.random.uniform(0, 0.1)                               # train.py:471
                ov = np.random.uniform(0.9, 1.0)                             # train.py:472
                if dn is None:
                    noise = torch.rand(bs, self.noise_len)                   # train.py:473 (CPU generator)
                else:                   # every rank counts every packed batch, with or without a scene of it
                    noise, step_i = None, dn.step
                    dn.step += 1
            else:
                zv, ov, noise, *extra = draw(bs)
                vn = extra[0] if extra else None      # optional 4th value: the (variety_k - 1, bs, noise_len) z of "fixed"
            fixed = self.use_variety_loss == "fixed"
            if fixed and vn is None and dn is None:   # z of the extra samples, drawn for the whole packed batch
                vn = torch.rand(self.variety_k - 1, bs, self.noise_len)
            sizes.append((bs, len(sb)))
            r0, r1, sbl = 0, bs, sb
            if self.world > 1:      # this rank's scene-aligned shard of the packed batch (z / label noise: global draws, sliced)
                lo, hi = shard_scenes(sb, self.world)[self.rank]
                if hi <= lo:        # no scene for this rank: it still takes part in the step's three all-reduces
                    flush()
                    outs.append(self._empty_step())
                    continue
                r0, r1 = int(sb[lo, 0]), int(sb[hi - 1, 1])
                sbl = sb[lo:hi] - r0
            item = (data.obsv[a + r0:a + r1], data.pred[a + r0:a + r1], zv, ov, noise[r0:r1] if noise is not None else None)
            # the folded K-sample step and, without `ragged_fused` + `use_graph`, the ragged step are not graph-captured:
            if fixed or (obs_len is not None and not (self.ragged_fused and self.use_graph)):
                flush()                          # one step() per packed batch
                z0, vnl = item[4], None
                if dn is not None:    # draws 0 .. variety_k-1 of this rank's rows in one launch, padded to the kernels' width
                    z = dn.fill(r1 - r0, self.noise_len, domain=TRAIN, step=step_i, n_draws=self.variety_k if fixed else 1,
                                row0=r0, ld=self.Z_COLS, device=self.device)[0]
                    z0, vnl = z[0], z[1:].reshape(-1, self.Z_COLS) if fixed else None
                elif fixed:
                    vnl = vn[:, r0:r1].reshape(-1, self.noise_len)
                outs.append(self.step(*item[:2], sbl, zv, ov, z0, data.ss, global_B=bs, global_row0=r0, variety_noise=vnl,
                                      obs_len=obs_len[a + r0:a + r1] if obs_len is not None else None))
                continue
            # consecutive packed batches with the same local layout share one graph launch (step_many)
            key = (bs, r0, np.asarray(sbl).tobytes())
            if key != pend_key or len(pend) == self.STEPS_PER_LAUNCH:
                flush()
                pend_key = key
            pend.append((item, sbl, bs, r0, step_i, obs_len[a + r0:a + r1] if obs_len is not None else None))
        flush()
        allo = torch.stack(outs)
        self._allreduce(allo)
        if self._direct is not None and self._direct.status_all() != 0:      # collective: every rank raises, none hangs
            raise L.SocialWaysHipError("the direct gradient exchange timed out waiting for a peer during this epoch on at "
                                       "least one rank (sw_comm_status): a rank whose wait times out publishes nothing and "
                                       "applies no update from it, so the replicas are no longer identical - restart from "
                                       "the last checkpoint (SW_COMM_TIMEOUT_S sets the wait, default 30 s)")
        o = allo.double().cpu().numpy()
        ade = float(o[:, -1, 0].sum() / data.n_train_samples)
        fde = float(o[:, -1, 1].sum() / data.n_train_samples)
        losses = self.losses_from(allo, [s[0] for s in sizes], data.n_next, data.ss)
        self.epoch += 1
        return ade, fde, losses, sizes

    def _empty_step(self):
        """A rank without scenes in this packed batch still takes part in the 3 all-reduces."""
        self._resolve_collectives()
        d_g = self.D.grad_views()
        self.G.grad_views()
        for u in range(self.n_unrolling_steps + 1):
            d_g.zero_()
            self._allreduce(d_g)
            self.D_optimizer.step()
            if u == 0 and self.n_unrolling_steps > 0:
                backup = self.D._flat.clone()
        self.G._gflat_all.zero_()
        self._allreduce(self.G._gflat_all)
        self.predictor_optimizer.step()
        if self.n_unrolling_steps > 0:
            if self._lin_mask is None:
                self._lin_mask = self.D.linear_mask() > 0
            self.D._flat.copy_(torch.where(self._lin_mask, backup, self.D._flat))
        return torch.zeros(self.n_unrolling_steps + 3, 3, device=self.device, dtype=torch.float64)

    # ------------------------------------------------------------------------------------------
    TEST_CHUNK = 16384      # agent copies (K x agents) per rollout launch of test(): scenes are folded up to this many

    def test(self, data, n_gen_samples=20, linear=False, write_to_file=None, just_one=False, collect=None):
        """test() (train.py:563-616): K sampled futures per held-out scene, avg / min-over-K ADE & FDE,
        optional prediction npz ('<epoch>-<t>.npz': timestamp, obsvs, preds_our, preds_gtt, preds_lnr,
        all denormalised - the schema visualize.py / calc_statistics.py read).  The K rollouts of a
        scene are independent given the noise, so they run as ONE batch of K*n agents with K copies
        of the scene, and consecutive held-out scenes are folded into the same launch (block-diagonal social
        block: a scene's rollout does not depend on its neighbours in the batch) up to TEST_CHUNK agent copies:
        identical rollouts, one launch sequence and one host sync per chunk instead of per scene.  The noise is
        drawn scene by scene, K draws of (n, noise_len) each, in the reference's order (train.py:584).
        A dataset with obs_len (ragged histories) is refused: this call replicates the dense forward pass."""
        _refuse_pred_len(data, "test()", "its errors run over all n_next frames of the dense forward pass - use evaluate() / "
                         "evaluate_horizon(), whose sampling launch scores each agent on its valid frames")
        _refuse_ragged(data, "test()", "it runs the dense forward pass on K copies of every scene - use evaluate() / "
                       "evaluate_history(), whose sampling path encodes each agent over its valid frames")
        ss, dev, K = data.ss, self.device, n_gen_samples
        base = _EvalSums(dev)
        for first, scenes in self._eval_fold(data, K, just_one):
            lo, hi = scenes[0][0], scenes[-1][1]
            c = SimpleNamespace(first=first, ab=scenes, lo=lo, n=hi - lo, obsv=data.obsv[lo:hi], pred=data.pred[lo:hi])
            with torch.no_grad():
                if linear and not write_to_file:
                    preds_k = predict_cv(c.obsv, self.n_next).unsqueeze(0)
                else:
                    # copy k of scene s sits at rows k * n + (scene rows): K copies of the chunk, each copy its scenes
                    noise = self.eval_noise(scenes, K, self.noise_len)
                    sb1 = np.asarray([[a - lo, b - lo] for a, b in scenes], dtype=np.int64)
                    sb = np.concatenate([sb1 + k * c.n for k in range(K)])
                    preds_k = self.G(c.obsv.repeat(K, 1, 1), noise.view(K * c.n, -1).to(dev), self.n_next, sb
                                     ).view(K, c.n, self.n_next, 4)
                errs = torch.pow((preds_k[:, :, :, :2] - c.pred.unsqueeze(0)) / ss, 2).sum(dim=3, keepdim=True).sqrt()
                if write_to_file or collect is not None:
                    for rec in self._eval_records(data, c, preds_k):
                        self._eval_emit(rec, collect, write_to_file)
                e = errs.double()
                base.sums += torch.stack([e.mean(2).mean(0).sum(), e[:, :, -1].mean(0).sum(),
                                          e.mean(2).min(0)[0].sum(), e[:, :, -1].min(0)[0].sum()])
        return tuple(base.result(data).values())

    @staticmethod
    def eval_chunks(batches, K, chunk):
        """The folding of test(): runs [i, j) of consecutive held-out scenes whose K copies fit `chunk` rows."""
        i = 0
        while i < len(batches):
            j, tot = i + 1, batches[i][1] - batches[i][0]
            while (j < len(batches) and batches[j][0] == batches[j - 1][1]
                   and (tot + batches[j][1] - batches[j][0]) * K <= chunk):
                tot += batches[j][1] - batches[j][0]
                j += 1
            yield i, j
            i = j

    @staticmethod
    def eval_noise(batches, K, noise_len):
        """The host noise of one chunk of test(): scene by scene, K draws of (n, noise_len) each from the torch CPU generator
        (train.py:584) -> (K, rows of the chunk, noise_len).  Needs no device."""
        lo, hi = batches[0][0], batches[-1][1]
        noise = torch.empty(K, hi - lo, noise_len)
        for a, b in batches:
            for k in range(K):
                noise[k, a - lo:b - lo] = torch.rand(b - a, noise_len)
        return noise

    # ---- the loop test() and every evaluate_*() share ---------------------------------------------------------------------
    def _eval_fold(self, data, K, just_one):
        """(index of its first scene, [(a, b) row range per scene]) of every chunk: the held-out scenes, the first one only
        with just_one, folded by eval_chunks up to TEST_CHUNK agent copies."""
        batches = [(int(b[0]), int(b[1])) for b in data.test_batches]
        if just_one:
            batches = batches[:1]
        for i, j in self.eval_chunks(batches, K, self.TEST_CHUNK):
            yield i, batches[i:j]

    def _eval_draws(self, data, K, just_one, dn, base, want_pred=True):
        """The K draws of the held-out scenes, chunk by chunk: what evaluate() and every evaluate_*() do before their own
        work.  Yields a namespace per chunk: first (index of its first scene), ab (its scenes' row ranges), lo, n (its rows
        are lo .. lo + n-1 of the held-out tracks), obsv, pred, sb and scenes (the chunk-local scene ranges and their
        SceneIndex), obs_len (the chunk's slice of data.obs_len - ragged histories - or None), pred_len (the slice of
        data.pred_len - ragged futures: per_agent and err are then over each row's valid frames - or None), z (K, n, Z_COLS) on the device,
        and from the sampling hook ph (K, n, n_next, 4; None without want_pred),
        per_agent (n, 4), err (K, n, 2), best (n,) int32.  z comes from `dn` (a DeviceNoise: evaluation domain, row = the
        ABSOLUTE held-out row, so a scene's draws do not depend on the chunking; one launch that also writes the padding),
        else from the reference's host stream (eval_noise), padded and copied once.  The chunk's scenes and per-agent sums
        are added to `base` (an _EvalSums) before it is handed out.  The loop body of the caller runs under this generator's
        torch.no_grad(), which ends with the generator (if the body raises: when the generator is collected)."""
        ol = getattr(data, "obs_len", None)
        if ol is not None and not isinstance(self.G, Generator):      # the generic-width and wide paths: refused before any chunk is built
            refuse_obs_len(ol, type(self).__name__)
        pl = getattr(data, "pred_len", None)
        if not isinstance(self.G, Generator):
            _refuse_pred_len(data, "%s.evaluate*()" % type(self).__name__, "ragged futures are implemented for the fused 64-unit "
                             "path only (hidden_size <= 64, n_latent_codes = 2)")
        dev = self.device
        with torch.no_grad():
            for first, scenes in self._eval_fold(data, K, just_one):
                lo, hi = scenes[0][0], scenes[-1][1]
                c = SimpleNamespace(first=first, ab=scenes, lo=lo, n=hi - lo, obsv=data.obsv[lo:hi], pred=data.pred[lo:hi])
                c.obs_len = ol[lo:hi] if ol is not None else None
                c.pred_len = pl[lo:hi] if pl is not None else None
                if dn is not None:
                    c.z = dn.fill(c.n, self.noise_len, domain=EVAL, n_draws=K, row0=lo, ld=self.Z_COLS, device=dev)[0]
                else:
                    c.z = self._pad_z(self.eval_noise(scenes, K, self.noise_len)).to(dev)
                c.sb = np.asarray([[a - lo, b - lo] for a, b in scenes], dtype=np.int64)
                c.scenes = ops.SceneIndex.get(c.sb, c.n, c.obsv.device)
                c.ph, c.per_agent, c.err, c.best = self._sample_draws(c, K, data.ss, want_pred)
                base.add(c)
                yield c

    def _sample_draws(self, c, K, ss, want_pred):
        """The sampling hook of _eval_draws(): K draws of chunk c from c.z -> (ph (K, n, n_next, 4) kept on the device, or None
        without want_pred; per_agent (n, 4) = mean_k ADE | mean_k FDE | min_k ADE | min_k FDE; err (K, n, 2); best (n,) int32 =
        the min-ADE draw).  Here: the observations are encoded and pooled ONCE, one launch rolls out the K copies and forms
        their errors (ops.gen_sample), the mean / min over K is reduced on the device."""
        G = self.G
        ph, red = ops.gen_sample(G.encoder.packed(), G.feature_embedder.packed(), G.attention.packed(), G.decoder.packed(),
                                 c.obsv, c.z.view(K * c.n, -1), c.scenes, self.n_next, G.use_social, K, gt=c.pred,
                                 inv_ss=1.0 / float(ss), want_pred=want_pred, pred_len=c.pred_len, obs_len=c.obs_len)
        return ph.view(K, c.n, self.n_next, 4) if ph is not None else None, red[0], red[2], red[1]

    def _eval_records(self, data, c, preds_k, extra={}):
        """The prediction records of chunk c, one per held-out scene: the dict test() writes - timestamp, obsvs, preds_our
        (K, n, n_next, 2) from preds_k, preds_gtt, preds_lnr, all denormalised - plus the scene's part of every entry of
        `extra` = {key: (device tensor, axis)}: axis = the one that runs over the chunk's rows, None = one entry per scene.
        A ragged chunk (c.obs_len): every record also has obs_len (n,), and preds_lnr is predict_cv of each row's VALID
        frames - a row of two frames gets the two-frame rule, not a velocity through its padding.
        A chunk with ragged futures (c.pred_len): every record also has pred_len (n,); preds_gtt keeps its padding."""
        linear_preds = predict_cv(c.obsv, self.n_next)
        if getattr(c, "pred_len", None) is not None:
            extra = dict(extra, pred_len=(c.pred_len, 0))
        obs_len = getattr(c, "obs_len", None)
        if obs_len is not None:
            extra = dict(extra, obs_len=(obs_len, 0))
            if c.obsv.shape[1] > 2:
                linear_preds = torch.where((obs_len <= 2)[:, None, None], predict_cv(c.obsv[:, -2:], self.n_next), linear_preds)
        sc = data.scale
        host = {k: (v.cpu().numpy(), ax) for k, (v, ax) in extra.items()}
        for si, (a, b) in enumerate(c.ab):
            t = data.times[a] if data.times is not None else c.first + si
            r = slice(a - c.lo, b - c.lo)
            rec = dict(timestamp=t, obsvs=sc.denormalize(c.obsv[r, :, :2].cpu().numpy()),
                       preds_our=sc.denormalize(preds_k[:, r, :, :2].cpu().numpy()),
                       preds_gtt=sc.denormalize(c.pred[r, :, :2].cpu().numpy()),
                       preds_lnr=sc.denormalize(linear_preds[r, :, :2].cpu().numpy()))
            for k, (v, ax) in host.items():
                rec[k] = v[si if ax is None else (slice(None),) * ax + (r,)].copy()
            yield rec

    def _eval_emit(self, rec, collect, write_to_file=None):
        """One record into `collect` and / or the file '<epoch>-<timestamp>.npz' under `write_to_file`."""
        if collect is not None:
            collect.append(rec)
        if write_to_file:
            os.makedirs(write_to_file, exist_ok=True)
            np.savez(os.path.join(write_to_file, str(self.epoch) + '-' + str(rec["timestamp"]) + '.npz'), **rec)

    def evaluate(self, data, n_gen_samples=20, write_to_file=None, just_one=False, collect=None, noise=None):
        """The contract of test() (train.py:563-616; without its `linear` branch) on the sampling path: the same four
        return values, prediction files, host noise stream and folding of scenes.  `noise` (default self.noise): a
        DeviceNoise replaces the host stream by the device stream's evaluation domain - draw k of held-out row r is a
        function of (seed, k, r) alone, so two calls agree and TEST_CHUNK / just_one do not change a scene's draws.
        The chunks and their draws are _eval_draws()'s; the K x n trajectories leave the kernel only when a file or
        `collect` wants them."""
        dn = self._device_noise(noise)
        base = _EvalSums(self.device)
        want_pred = bool(write_to_file) or collect is not None
        for c in self._eval_draws(data, n_gen_samples, just_one, dn, base, want_pred):
            if want_pred:
                for rec in self._eval_records(data, c, c.ph):
                    self._eval_emit(rec, collect, write_to_file)
        return tuple(base.result(data).values())

    def _evaluate_by_length(self, data, K, just_one, noise, attr, top, key):
        """evaluate() split by a per-agent length: chunk attribute `attr` (obs_len / pred_len; None: every agent in bucket
        `top`), buckets 0 .. top, the buckets that hold agents under result key `key`.  The sums are float64 on the device,
        one host sync at the end.  A select per bucket, not a product with a 0 / 1 mask: a row whose error is not finite
        stays in its own bucket."""
        dn = self._device_noise(noise)
        dev = self.device
        base = _EvalSums(dev)
        acc = torch.zeros(top + 1, 5, dtype=torch.float64, device=dev)      # per length: count | the four sums
        lens = torch.arange(top + 1, device=dev)[:, None]
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        for c in self._eval_draws(data, K, just_one, dn, base, want_pred=False):
            n = getattr(c, attr)
            if n is None:
                n = torch.full((c.n,), top, dtype=torch.int32, device=dev)
            rows = torch.cat([torch.ones(c.n, 1, dtype=torch.float64, device=dev), c.per_agent.double()], dim=1)
            acc += torch.where((n[None, :] == lens)[:, :, None], rows[None], zero).sum(1)      # (top + 1, n, 5) -> (top + 1, 5)
        vals = torch.cat([base.sums / data.n_test_samples, acc.flatten()]).tolist()
        out = dict(zip(_EvalSums.KEYS, vals[:4]))
        by = {}
        for n in range(top + 1):
            cnt, *sums = vals[4 + 5 * n:9 + 5 * n]
            if cnt > 0:
                by[n] = dict(count=int(cnt), **{k: v / cnt for k, v in zip(_EvalSums.KEYS, sums)})
        out.update({key: by}, n_agents=sum(b - a for a, b in base.scenes))
        return out

    def evaluate_history(self, data, n_gen_samples=20, just_one=False, noise=None):
        """evaluate() split by history length: what an agent seen for n frames is predicted with.  Returns a dict:
          ade_avg, fde_avg, ade_min, fde_min  the numbers of evaluate() from the same RNG state, bit for bit;
          by_len   {n: {count, ade_avg, fde_avg, ade_min, fde_min}} for every history length n present among the agents
                   evaluated (data.obs_len; a dataset without it: the single bucket n_past), the means over that length's
                   agents: sum_n count_n * by_len[n][key] / data.n_test_samples is the overall key;
          n_agents.
        Chunking, noise and sampling launches are evaluate()'s; the sums are float64 on the device, one host sync at the end.
        A row whose error is not finite stays in its own bucket (a select per bucket, as in evaluate_horizon())."""
        return self._evaluate_by_length(data, n_gen_samples, just_one, noise, "obs_len", data.n_past, "by_len")

    def evaluate_horizon(self, data, n_gen_samples=20, just_one=False, noise=None):
        """evaluate() split by FUTURE length, the twin of evaluate_history(): what an agent that stays for m more frames is
        predicted with.  Returns a dict:
          ade_avg, fde_avg, ade_min, fde_min  the numbers of evaluate() from the same RNG state, bit for bit;
          by_next  {m: {count, ade_avg, fde_avg, ade_min, fde_min}} for every future length m present among the agents
                   evaluated (data.pred_len; a dataset without it: the single bucket n_next), the means over that length's
                   agents: sum_m count_m * by_next[m][key] / data.n_test_samples is the overall key;
          n_agents.
        Chunking, noise and sampling launches are evaluate()'s; the sums are float64 on the device, one host sync at the end."""
        return self._evaluate_by_length(data, n_gen_samples, just_one, noise, "pred_len", data.n_next, "by_next")

    def evaluate_scenes(self, data, n_gen_samples=20, coll_dist=0.1, just_one=False, collect=None):
        """evaluate() plus what its K joint draws say about the scene as a whole.  Draw k of a scene is draw k of each of
        its agents - the joint future that copy k of the scene rolls out.  Returns a dict:
          ade_avg, fde_avg, ade_min, fde_min  the numbers of evaluate() from the same RNG state, bit for bit;
          jade_min, jfde_min   joint min ADE / FDE: per scene the minimum over k of the scene's MEAN error (one k for the
                               whole scene, where ade_min picks a k per agent), summed with the scene's agent count and
                               divided by data.n_test_samples like the four above: ade_min <= jade_min <= ade_avg;
          col_joint            mean over the scenes of two or more agents of the share of draws in which two agents come
                               closer than coll_dist (world units, the units of the errors) at any moment of the future,
                               moving linearly between frames and starting at the last observed position;
          col_best             share of those scenes whose jade_min draw collides;
          col_agent            share of colliding (draw, agent) over those scenes, agent-weighted;
          col_gt               share of those scenes whose ground-truth future collides (the same kernel, K = 1);
          n_scenes, n_multi    scenes evaluated, and those of two or more agents (0: the col_* are 0).
        Chunking, host noise and sampling launches are evaluate()'s; per chunk two more launches (ops.scene_metrics) work on
        the draws where they are and the same two on the ground truth; sums are float64 on the device, one host sync at the end.  With `collect` every
        record of evaluate() also has `clear` (K, n), `per_scene` (6,) and `kbest` (columns: ops.scene_reduce).
        With self.noise set (a DeviceNoise) the draws are evaluate()'s from that stream.  This call's argument list is pinned
        (tests/test_scene_host.py), so the stream reaches it through the attribute only, not through a keyword.
        A dataset with pred_len (ragged futures): the errors are over each agent's valid frames and a collision needs both
        agents present - the segment of a pair that ends at frame t counts only while t < both lengths, for the K draws
        and for col_gt alike (ops.scene_clearance(lens=...)): a draw is not charged for crossing a place nobody was seen at."""
        dn = self._device_noise(None)
        dev, K = self.device, n_gen_samples
        inv_ss = 1.0 / float(data.ss)
        base = _EvalSums(dev)
        # sum n * jade | sum n * jfde | then over multi-agent scenes: colliding share | kbest flag | n * agent share | gt flag
        acc = torch.zeros(6, dtype=torch.float64, device=dev)
        for c in self._eval_draws(data, K, just_one, dn, base):
            per_scene, kbest, clear = ops.scene_metrics_len(c.err, c.ph, c.obsv, c.scenes, K, self.n_next, inv_ss, coll_dist,
                                                            lens=c.pred_len)      # no lengths: scene_metrics()'s launches
            gt_scene, _ = ops.scene_reduce(torch.zeros(1, c.n, 2, device=dev),
                                           ops.scene_clearance(c.pred, c.obsv[:, -1], c.scenes, 1, inv_ss, lens=c.pred_len),
                                           c.scenes, 1, coll_dist)
            cnt = (c.scenes.scene_off[1:] - c.scenes.scene_off[:-1]).double()
            multi = (cnt > 1).double()
            ps = per_scene.double()
            acc += torch.stack([(cnt * ps[:, 0]).sum(), (cnt * ps[:, 1]).sum(), (multi * ps[:, 2]).sum(),
                                (multi * ps[:, 3]).sum(), (multi * cnt * ps[:, 5]).sum(),
                                (multi * gt_scene[:, 2].double()).sum()])
            if collect is not None:
                for rec in self._eval_records(data, c, c.ph, dict(clear=(clear, 1), per_scene=(per_scene, None), kbest=(kbest, None))):
                    rec["kbest"] = int(rec["kbest"])
                    collect.append(rec)
        n_multi = sum(1 for a, b in base.scenes if b - a > 1)
        agents_multi = sum(b - a for a, b in base.scenes if b - a > 1)
        out = base.result(data)
        jade, jfde, joint, best, agent, gt = acc.tolist()
        out.update(jade_min=jade / data.n_test_samples, jfde_min=jfde / data.n_test_samples,
                   col_joint=joint / n_multi if n_multi else 0.0, col_best=best / n_multi if n_multi else 0.0,
                   col_agent=agent / agents_multi if n_multi else 0.0, col_gt=gt / n_multi if n_multi else 0.0,
                   n_scenes=len(base.scenes), n_multi=n_multi)
        return out

    def sample_ranked(self, obsv_p, n_samples, top_m, sub_batches=[], noise=None, row0=0, obs_len=None):
        """The deployment call - K draws, no ground truth, pick a few: the top_m of n_samples futures per agent that the
        discriminator scores highest, best first.  obsv_p (B, To, 2), noise (K, B, noise_len), None or a DeviceNoise (rows from
        `row0`) as Generator.sample().  obs_len (B,) - tensor, numpy array or list: ragged histories, as Generator.sample() -
        an agent seen for fewer than To frames (at least 2, right-aligned in obsv_p) is sampled and scored on those frames
        alone and stays in its scene's social block.
        Returns (trajs (M, B, n_next, 4), score (M, B) raw LSGAN score, non-increasing along M, order (B, M) int32: trajs[m, a]
        is draw order[a, m]).  A sampling launch (Generator.sample), a scoring launch (Discriminator.score_samples), a
        ranking launch (ops.sample_rank) and a gather."""
        K, M, ph, score = _scored_draws(self, obsv_p, n_samples, top_m, sub_batches, noise, row0, obs_len)
        with torch.no_grad():
            order, _ = ops.sample_rank(score, K, M)
            idx = order.t().long()
            trajs = ph.gather(0, idx[:, :, None, None].expand(M, ph.shape[1], self.n_next, 4))
            return trajs, score.gather(0, idx), order

    RANKED_KEYS = ("ade_top1", "fde_top1", "ade_topm", "fde_topm", "best_rank", "score_draws", "score_gt", "code_mse")

    def evaluate_ranked(self, data, n_gen_samples=20, top_m=5, just_one=False, collect=None, noise=None):
        """evaluate() plus what the discriminator makes of its K draws WITHOUT the ground truth: it scores every draw
        (Discriminator.score_samples: one launch, the observation encoded once), ranks them per agent (ops.sample_rank) and
        the errors of the draws it prefers are read off.  Returns a dict:
          ade_avg, fde_avg, ade_min, fde_min  the numbers of evaluate() from the same RNG state, bit for bit;
          ade_top1, fde_top1   the error of each agent's top-scored draw - what shipping D's choice costs;
          ade_topm, fde_topm   per agent the minimum over its top_m highest-scored draws: ade_min <= ade_topm <= ade_top1;
          best_rank            mean over agents of the rank D gives the min-ADE draw: 0 = always first, (K - 1) / 2 = a ranker
                               without information;
          score_draws, score_gt   mean raw LSGAN score over (draw, agent), and over the agents' ground-truth futures;
          code_mse             mean over (draw, agent) of the mean squared difference between D's code_hat and the first
                               columns of that draw's z: the InfoGAN term of the training losses, unweighted;
          n_agents, K, top_m.
        Per-agent sums are divided by data.n_test_samples like evaluate()'s, per-(draw, agent) sums by K times that; float64
        sums on the device, one host sync at the end.  Chunking, host noise and sampling launches are evaluate()'s.  With
        `collect` every record of evaluate() also has `score` (K, n), `order` (n, top_m) and `code_hat` (K, n, codes).
        `noise`: as evaluate() - a DeviceNoise (default self.noise) gives evaluate(noise=...)'s draws.
        A dataset with pred_len (ragged futures): the errors are over each agent's valid frames; D scores the draws, which are
        full length, as ever; a truncated future is no D input, so score_gt is the mean over the agents with a FULL future,
        divided by their count n_full (0.0 when there is none), and the dict gains n_full."""
        dn = self._device_noise(noise)
        dev, K, M = self.device, int(n_gen_samples), int(top_m)
        if not 1 <= M <= K:
            raise ValueError("top_m must lie in 1 .. n_gen_samples = %d, got %d" % (K, M))
        base = _EvalSums(dev)
        acc = torch.zeros(len(self.RANKED_KEYS), dtype=torch.float64, device=dev)
        ragged_next = getattr(data, "pred_len", None) is not None
        n_full = torch.zeros(1, dtype=torch.float64, device=dev)      # rows with a full future (ragged futures only)
        for c in self._eval_draws(data, K, just_one, dn, base):
            score, code = self.D.score_samples(c.obsv, c.ph, obs_len=c.obs_len)
            order, ranked = ops.sample_rank(score, K, M, err=c.err, best=c.best)
            gt_score, _ = self.D.score_samples(c.obsv, get_traj_4d(c.obsv, c.pred)[1].unsqueeze(0), obs_len=c.obs_len)
            if c.pred_len is not None:      # a select: what D made of a padded future is dropped, whatever it is
                full = (c.pred_len == self.n_next).view(1, -1)
                gt_score = torch.where(full, gt_score, torch.zeros_like(gt_score))
                n_full += full.sum()
            csq = (code.double() - c.z[:, :, :code.shape[-1]].double()).pow(2).mean(dim=2)
            acc += torch.cat([ranked.double().sum(0), torch.stack([score.double().sum(), gt_score.double().sum(), csq.sum()])])
            if collect is not None:
                collect.extend(self._eval_records(data, c, c.ph, dict(score=(score, 1), order=(order, 0), code_hat=(code, 1))))
        nt = data.n_test_samples
        out = base.result(data)
        div = torch.tensor([nt] * 5 + [K * nt, nt, K * nt], dtype=torch.float64, device=dev)
        if ragged_next:      # score_gt over the full rows, divided on the device (no full row: 0 / 1); n_full rides along
            div[6:7] = n_full.clamp(min=1.0)
        vals = torch.cat([acc / div, n_full]).tolist()
        out.update(zip(self.RANKED_KEYS, vals))
        out.update(n_agents=sum(b - a for a, b in base.scenes), K=K, top_m=M)
        if ragged_next:
            out.update(n_full=int(vals[-1]))
        return out

    @staticmethod
    def _gather_picks(values, idx, fill):
        """values (K, B, ...) at idx (M, B) along K; `fill` where idx is -1 (a slot past the group's count)."""
        tail = (1,) * (values.dim() - 2)
        valid = (idx >= 0).view(idx.shape + tail)
        at = idx.clamp(min=0).view(idx.shape + tail).expand(idx.shape + tuple(values.shape[2:]))
        return torch.where(valid, values.gather(0, at), torch.full((), fill, dtype=values.dtype, device=values.device))

    def sample_diverse(self, obsv_p, n_samples, top_m, radius, metric="fde", joint=False, sub_batches=[], noise=None, row0=0,
                       scale=1.0, obs_len=None):
        """sample_ranked() without the near-duplicates: of n_samples futures the highest-scored one is kept, every draw within
        `radius` of it (metric "fde": distance at the last step, "ade": mean distance over the steps, both times `scale` -
        the `scale` of stats.scene_clearance) counts as the same mode, then the highest-scored of the rest, top_m times at
        most (ops.sample_nms).  joint=False: per agent.  joint=True: per scene of sub_batches - draw k of a scene is draw k of
        each of its agents; two joint draws are one mode only if every agent is within the radius, and a joint draw scores
        as its lowest-scored agent.  obsv_p, noise, row0, obs_len as sample_ranked().
        Returns (trajs (M, B, n_next, 4), weight, score (M, B), order, count): order (B, M) int32, weight (B, M) = the share of
        the n_samples draws that fell to each kept mode (rows sum to 1) and count (B,) int32 = the modes found - per scene
        with joint=True: (S, M), (S, M), (S,), and trajs[m, a] is draw order[scene of a, m] of agent a, score[m, a] that draw's
        own score.  Per agent the scores do not increase along M.  Slots from count on: zeros in trajs, -inf in score, 0 in
        weight, -1 in order.  Sampling, scoring, one suppression launch and a gather."""
        K, M, ph, score = _scored_draws(self, obsv_p, n_samples, top_m, sub_batches, noise, row0, obs_len)
        with torch.no_grad():
            B = ph.shape[1]
            scenes = ops.SceneIndex.get(sub_batches, B, ph.device) if joint else None
            order, count, weight, _, _ = ops.sample_nms(ph, score, K, M, radius, metric, scenes, inv_ss=scale)
            rows = order
            if joint:      # the scene of every row: the number of scene ends at or below it
                rows = order[torch.bucketize(torch.arange(B, device=ph.device), scenes.scene_off[1:].long(), right=True)]
            idx = rows.t().long()
            return self._gather_picks(ph, idx, 0.0), weight, self._gather_picks(score, idx, float("-inf")), order, count

    DIVERSE_KEYS = ("ade_div1", "fde_div1", "ade_divm", "fde_divm", "rank_hit", "w_hit", "n_modes", "w_first")

    def evaluate_diverse(self, data, n_gen_samples=20, top_m=5, radius=0.5, metric="fde", joint=False, just_one=False,
                         collect=None, noise=None):
        """evaluate() plus what a diverse selection of its K draws is worth: the draws are scored as in evaluate_ranked() and
        reduced to at most top_m modes per group by greedy suppression in score order (ops.sample_nms; `radius` in world
        units through data.ss like the coll_dist of evaluate_scenes(), metric "fde" or "ade").  A group is an agent, or with
        joint=True a held-out scene (draw k of a scene is draw k of each of its agents).  Returns a dict:
          ade_avg, fde_avg, ade_min, fde_min  the numbers of evaluate() from the same RNG state, bit for bit;
          ade_div1, fde_div1   the error of each agent's draw in the first pick of its group;
          ade_divm, fde_divm   per agent the minimum over the kept modes: ade_min <= ade_divm <= ade_div1;
          n_modes              mean over the groups of the modes found (<= top_m);
          w_first              mean over the groups of the weight of the first pick (its share of the K draws);
          w_hit                mean over the agents of the weight of the mode that holds the agent's min-ADE draw: the
                               probability the selection gives the right mode;
          rank_hit             mean over the agents of the index of that mode (0 = the first pick);
          jade_divm, jfde_divm (joint=True only) per scene the minimum over the picks of the scene's MEAN error, summed with
                               the scene's agent count like jade_min of evaluate_scenes(): jade_min <= jade_divm;
          n_agents, n_groups, K, top_m, radius, metric.
        Per-agent sums are divided by data.n_test_samples like evaluate_ranked()'s (at radius 0 ade_div1 / ade_divm are its
        ade_top1 / ade_topm bit for bit; like them, ade_divm at top_m = K and radius 0 is ade_min up to the last bit of that
        division and to the bit where 1 / n_test_samples is exact), per-group sums by n_groups; float64 sums on the
        device, one host sync at the end.  Chunking, noise streams and sampling launches are evaluate_ranked()'s.  With
        `collect` every record of evaluate() also has `order`, `count`, `weight` and `assign` of its scene: (n, top_m), (n,),
        (n, top_m), (n, K) per agent, or (top_m,), a number, (top_m,), (K,) with joint=True."""
        dn = self._device_noise(noise)
        ss, dev, K, M = data.ss, self.device, int(n_gen_samples), int(top_m)
        if not 1 <= M <= K:
            raise ValueError("top_m must lie in 1 .. n_gen_samples = %d, got %d" % (K, M))
        if metric not in ops.NMS_METRICS:
            raise ValueError("metric must be one of %s, got %r" % (sorted(ops.NMS_METRICS), metric))
        inv_ss = 1.0 / float(ss)
        base = _EvalSums(dev)
        acc = torch.zeros(len(self.DIVERSE_KEYS) + 2, dtype=torch.float64, device=dev)      # ... | sum n * jade | sum n * jfde
        for c in self._eval_draws(data, K, just_one, dn, base):
            score, _ = self.D.score_samples(c.obsv, c.ph, obs_len=c.obs_len)
            order, count, weight, assign, per_row = ops.sample_nms(c.ph, score, K, M, radius, metric, c.scenes if joint else None,
                                                                   inv_ss=inv_ss, err=c.err, best=c.best)
            # the first five columns summed in the shape evaluate_ranked() sums its own: the same bits at radius 0
            part = [torch.cat([per_row[:, :4], per_row[:, 5:6]], dim=1).double().sum(0),
                    torch.stack([per_row[:, 4].double().sum(), count.double().sum(), weight[:, 0].double().sum()])]
            if joint:
                off = c.scenes.scene_off.long()
                cnt = (off[1:] - off[:-1]).double()
                run = torch.cat([torch.zeros(K, 1, 2, dtype=torch.float64, device=dev), c.err.double().cumsum(1)], dim=1)
                mean = ((run[:, off[1:]] - run[:, off[:-1]]) / cnt[None, :, None]).permute(1, 0, 2)      # (S, K, 2)
                at = order.long().clamp(min=0)[:, :, None].expand(-1, -1, 2)
                picked = torch.where((order >= 0)[:, :, None], mean.gather(1, at), torch.full_like(mean[:, :1], float("inf")))
                part.append((cnt[:, None] * picked.min(dim=1)[0]).sum(0))
            else:
                part.append(torch.zeros(2, dtype=torch.float64, device=dev))
            acc += torch.cat(part)
            if collect is not None:
                ax = None if joint else 0      # per scene, or the rows of the scene's agents
                collect.extend(self._eval_records(data, c, c.ph, dict(order=(order, ax), count=(count, ax), weight=(weight, ax),
                                                                      assign=(assign, ax))))
        nt, n_agents = data.n_test_samples, sum(b - a for a, b in base.scenes)
        n_groups = len(base.scenes) if joint else n_agents
        out = base.result(data)
        div = torch.tensor([nt] * 6 + [n_groups] * 2 + [nt] * 2, dtype=torch.float64, device=dev)
        vals = (acc / div).tolist()
        out.update(zip(self.DIVERSE_KEYS, vals))
        if joint:
            out.update(jade_divm=vals[-2], jfde_divm=vals[-1])
        out.update(n_agents=n_agents, n_groups=n_groups, K=K, top_m=M, radius=float(radius), metric=metric)
        return out

    @staticmethod
    def _check_compose(coll_dist, sweeps):
        """The arguments sample_composed() and evaluate_composed() share, checked before anything is sampled."""
        if not float(coll_dist) >= 0.0:
            raise ValueError("coll_dist must be >= 0, got %r" % (coll_dist,))
        if int(sweeps) < 1:
            raise ValueError("sweeps must be at least 1, got %r" % (sweeps,))

    def sample_composed(self, obsv_p, n_samples, coll_dist, sub_batches=[], noise=None, row0=0, scale=1.0, sweeps=8,
                        obs_len=None):
        """sample_ranked(top_m=1) with the picks checked against each other: ONE future per agent, chosen per scene of
        sub_batches so that no two chosen paths come closer than coll_dist (times `scale`, the `scale` of
        stats.scene_clearance) at any moment - agents moving linearly between frames, every path starting at the last observed
        position.  Given the observations the generator's K draws of different agents are independent: the social block
        sees the observed steps only and a draw's rollout reads its own noise and its own agent's encoding.  So a tuple
        with a different draw per agent is as much a sample of the scene's joint future as "draw k of everybody" - this
        call chooses among the K^n tuples that one sampling launch has paid for, it does not patch a joint draw.  Every
        agent starts on the draw D scores highest; in up to `sweeps` sweeps over the scene's agents one in conflict moves to
        the draw with the fewest conflicts against the others' current picks, the highest score among equals, if that is
        fewer than it has (ops.scene_compose).  obsv_p, noise, row0, obs_len as sample_ranked().
        Returns (trajs (B, n_next, 4), score (B,) the chosen draws' own scores, sel (B,) int32: trajs[a] is draw sel[a],
        clear (B,): the closest approach of every chosen path to the others of its scene, +inf alone - an agent with
        clear < coll_dist could not be freed -, per_scene (S, 4) int32: conflicting pairs among the top-scored picks | among
        the chosen | agents that left their top-scored draw | sweeps that changed something).  Sampling, scoring, one
        composing launch and a gather."""
        self._check_compose(coll_dist, sweeps)
        K, _, ph, score = _scored_draws(self, obsv_p, n_samples, 1, sub_batches, noise, row0, obs_len)
        with torch.no_grad():
            B = ph.shape[1]
            scenes = ops.SceneIndex.get(sub_batches, B, ph.device)
            sel, _, clear, per_scene, _ = ops.scene_compose(ph, obsv_p[:, -1], score, scenes, K, coll_dist, inv_ss=scale,
                                                            sweeps=sweeps)
            idx = sel.long()[None]
            trajs = ph.gather(0, idx[:, :, None, None].expand(1, B, self.n_next, 4))[0]
            return trajs, score.gather(0, idx)[0], sel, clear, per_scene

    COMPOSED_KEYS = ("ade_top1", "fde_top1", "ade_comp", "fde_comp", "score_top1", "score_comp", "moved", "col_top1", "col_comp",
                     "pairs_top1", "pairs_comp")

    def evaluate_composed(self, data, n_gen_samples=20, coll_dist=0.1, sweeps=8, just_one=False, collect=None, noise=None):
        """evaluate() plus what composing a scene's future from the per-agent draws buys (sample_composed(): given the
        observations the agents' draws are independent, so one draw per agent, whichever, is a joint sample).  The draws are
        scored as in evaluate_ranked(); per held-out scene every agent starts on its top-scored draw and agents in conflict -
        closer than coll_dist to another's pick, in world units through data.ss like evaluate_scenes() - move to other draws
        (ops.scene_compose, `sweeps` sweeps at most).  Returns a dict:
          ade_avg, fde_avg, ade_min, fde_min  the numbers of evaluate() from the same RNG state, bit for bit;
          ade_top1, fde_top1     the error of each agent's top-scored draw (evaluate_ranked()'s);
          ade_comp, fde_comp     the error of each agent's composed draw: what avoiding the collisions costs;
          score_top1, score_comp the mean raw LSGAN score of the two picks (score_comp <= score_top1);
          moved                  share of agents whose draw changed;
          col_top1, col_comp     share of the scenes of two or more agents with at least one conflicting pair, before and after;
          pairs_top1, pairs_comp mean conflicting pairs per such scene, before and after (pairs_comp <= pairs_top1);
          n_scenes, n_multi, K, coll_dist, sweeps.
        Per-agent sums are divided by data.n_test_samples like evaluate_ranked()'s, per-scene sums by n_multi (0: they are
        0); float64 sums on the device, one host sync at the end.  Chunking, noise streams and sampling launches are
        evaluate_ranked()'s.  With `collect` every record of evaluate() also has `sel`, `sel0`, `clear` (n,) and `per_scene`
        (4,) (columns: ops.scene_compose).  A dataset with pred_len (ragged futures): the errors are over each agent's valid
        frames and a pair's segment counts only while both agents are present, as in evaluate_scenes()."""
        self._check_compose(coll_dist, sweeps)
        dn = self._device_noise(noise)
        dev, K = self.device, int(n_gen_samples)
        inv_ss = 1.0 / float(data.ss)
        base = _EvalSums(dev)
        acc = torch.zeros(len(self.COMPOSED_KEYS), dtype=torch.float64, device=dev)
        for c in self._eval_draws(data, K, just_one, dn, base):
            score, _ = self.D.score_samples(c.obsv, c.ph, obs_len=c.obs_len)
            sel, sel0, clear, per_scene, per_row = ops.scene_compose(c.ph, c.obsv[:, -1], score, c.scenes, K, coll_dist, inv_ss,
                                                                     sweeps, lens=c.pred_len, err=c.err)
            picks = score.gather(0, torch.stack([sel0, sel]).long()).double().sum(1)      # single-agent scenes: no pairs
            ps = per_scene.double()
            acc += torch.cat([per_row.double().sum(0), picks, ps[:, 2].sum()[None], (ps[:, :2] > 0).double().sum(0),
                              ps[:, :2].sum(0)])
            if collect is not None:
                collect.extend(self._eval_records(data, c, c.ph, dict(sel=(sel, 0), sel0=(sel0, 0), clear=(clear, 0),
                                                                      per_scene=(per_scene, None))))
        nt = data.n_test_samples
        n_multi = sum(1 for a, b in base.scenes if b - a > 1)
        out = base.result(data)
        div = torch.tensor([nt] * 7 + [max(n_multi, 1)] * 4, dtype=torch.float64, device=dev)
        out.update(zip(self.COMPOSED_KEYS, (acc / div).tolist()))
        out.update(n_scenes=len(base.scenes), n_multi=n_multi, K=K, coll_dist=float(coll_dist), sweeps=int(sweeps))
        return out

    def plan_risk(self, obsv_p, plans, n_samples, coll_dist, sub_batches=[], scene=None, ego=None, plan_start=None, noise=None,
                  row0=0, scale=1.0, obs_len=None):
        """"If the ego takes this path, how likely is it to run into somebody?" - candidate paths that are NOT among the draws,
        scored against the K sampled futures of the scene's pedestrians.  obsv_p (B, To, 2), sub_batches, noise (K, B,
        noise_len), None or a DeviceNoise (rows from `row0`) and obs_len as sample_ranked(): ONE sampling launch, the draws
        Generator.sample() returns, then ONE risk launch (ops.plan_risk).  plans (Q, P, n_next, 2), or (P, n_next, 2) for one
        query: P candidate futures per query, in the coordinates of obsv_p.  Query q looks at scene scene[q] of sub_batches
        (None: query q belongs to scene q, Q = the number of scenes).  ego (Q,) rows of obsv_p or None: the ego's OBSERVED track is
        an agent of the scene, so the social block sees it; its own draws are left out of the risk and its plans start at
        obsv_p[ego[q], -1].  Without ego the plans start at plan_start[q] (Q, 2), which is then required.  Every pedestrian
        path starts at its last observed position; all move linearly between frames; a conflict is a closest approach times
        `scale` below coll_dist.  The draws are OPEN-LOOP: the pedestrians do not react to the plan.
        Given the observations the generator's draws of different agents are independent (sample_composed()), so the chance
        that a plan stays clear of everybody is the product over the agents of each agent's share of clear draws - all K^n
        tuples that one sampling launch has paid for, where the index-paired draws give a multiple of 1 / K.
        Returns (risk (Q, P), clear_min (Q, P), counts (Q, P, 4) int32 - the columns of ops.plan_risk -, trajs (K, B, n_next, 4)).
        Works at any hidden size: it needs only Generator.sample()."""
        if not float(coll_dist) >= 0.0:
            raise ValueError("coll_dist must be >= 0, got %r" % (coll_dist,))
        K, B, plans, sb, scene, ego, plan_start = _plan_queries(self.n_next, obsv_p, plans, n_samples, sub_batches, scene, ego,
                                                                plan_start, scale)
        dev = obsv_p.device
        L.require_gpu(obsv_p)
        if obs_len is not None:
            if not isinstance(self.G, Generator):      # the generic-width and wide paths: no ragged kernels
                refuse_obs_len(obs_len, type(self).__name__)
            obs_len = ops.obs_len_arg(obs_len, B, obsv_p.shape[1], 2, dev)
        with torch.no_grad():
            scenes = ops.SceneIndex.get(sb, B, dev)
            q_scene = torch.from_numpy(scene).to(dev)
            q_ego = None
            if ego is not None:
                q_ego = torch.from_numpy(ego).to(dev)
                plan_start = obsv_p[q_ego.long(), -1, :2]
            ph = self.G.sample(obsv_p, K, self.n_next, sub_batches, noise, row0=row0, obs_len=obs_len)
            risk, clear_min, counts = ops.plan_risk(ph, obsv_p[:, -1], scenes, K, plans.to(dev), plan_start.to(dev), q_scene, q_ego,
                                                    coll_dist, inv_ss=float(scale))
            return risk, clear_min, counts, ph

    RISK_KEYS = ("risk_mean", "col_gt_agent", "brier", "brier_diag", "risk_hit", "risk_miss", "t_first_err")

    def evaluate_risk(self, data, n_gen_samples=20, coll_dist=0.1, just_one=False, collect=None, noise=None):
        """evaluate() plus a score of the generator as a COLLISION PREDICTOR, leave-one-out: every held-out agent of a scene of
        two or more agents is the ego once.  Its plan is its ground-truth future (its pred_len frames when the dataset carries
        one), the others are the K draws of the scene's other agents (plan_risk(): open-loop, the draws do not react to the
        plan), and coll_dist is in world units through data.ss like evaluate_scenes().  With r_a the product risk, d_a =
        counts[.., 0] / K the index-paired estimate and y_a = [the clearance of agent a among the ground-truth futures <
        coll_dist] (the K = 1 launch behind col_gt), over those agents - returns a dict:
          ade_avg, fde_avg, ade_min, fde_min  the numbers of evaluate() from the same RNG state, bit for bit;
          risk_mean              the mean of r;      col_gt_agent   the mean of y;
          brier, brier_diag      the mean of (r - y)^2 and of (d - y)^2: does a predicted 0.3 come true 30 % of the time;
          brier_base             the Brier score of the constant col_gt_agent, which a useful predictor beats;
          risk_hit, risk_miss    the mean of r over the agents with y = 1 / y = 0 (0 without such agents);
          t_first_err            over the agents with y = 1 and r > 0, the mean |frame of the predicted first conflict - frame of
                                 the true one| (0 without such agents);
          n_ego, K, coll_dist.
        Chunking, noise streams and sampling launches are evaluate()'s; per chunk one risk launch on the draws where they are, the
        ground-truth clearance launch and one K = 1 risk launch on the ground truth for the true first frame.  Sums are float64
        on the device, one host sync at the end.  With `collect` every record of evaluate() also has `risk`, `risk_diag`, `hit_gt`
        (n,) and `risk_counts` (n, 4) (columns: ops.plan_risk; agents alone in their scene: risk 0, no hit)."""
        if not float(coll_dist) >= 0.0:
            raise ValueError("coll_dist must be >= 0, got %r" % (coll_dist,))
        dn = self._device_noise(noise)
        dev, K = self.device, int(n_gen_samples)
        inv_ss = 1.0 / float(data.ss)
        base = _EvalSums(dev)
        # over the egos: sum r | sum y | sum (r - y)^2 | sum (d - y)^2 | sum r y | sum r (1 - y) | sum |dt| | agents in that sum
        acc = torch.zeros(8, dtype=torch.float64, device=dev)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        for c in self._eval_draws(data, K, just_one, dn, base):
            q_scene, multi = c.scenes.row_scene()
            q_ego = torch.arange(c.n, dtype=torch.int32, device=dev)
            start = c.obsv[:, -1]
            plans, pstart = c.pred[:, None, :, :2].contiguous(), start[:, :2].contiguous()
            risk, _, counts = ops.plan_risk(c.ph, start, c.scenes, K, plans, pstart, q_scene, q_ego, coll_dist, inv_ss,
                                            lens=c.pred_len, plan_lens=c.pred_len)
            gt_clear = ops.scene_clearance(c.pred, start, c.scenes, 1, inv_ss, lens=c.pred_len)[0]
            _, _, gt_counts = ops.plan_risk(c.pred, start, c.scenes, 1, plans, pstart, q_scene, q_ego, coll_dist, inv_ss,
                                            lens=c.pred_len, plan_lens=c.pred_len)
            hit = (gt_clear < coll_dist) & multi
            r, y = risk[:, 0].double(), hit.double()
            d = counts[:, 0, 0].double() / K
            timed = hit & (risk[:, 0] > 0)
            dt = (counts[:, 0, 1] - gt_counts[:, 0, 1]).abs().double()
            rows = torch.stack([r, y, (r - y) ** 2, (d - y) ** 2, r * y, r * (1 - y), torch.where(timed, dt, zero), timed.double()])
            acc += torch.where(multi[None], rows, zero).sum(1)
            if collect is not None:
                collect.extend(self._eval_records(data, c, c.ph, dict(risk=(risk[:, 0], 0), risk_diag=(d.float(), 0), hit_gt=(hit, 0),
                                                                      risk_counts=(counts[:, 0], 0))))
        n_ego = sum(b - a for a, b in base.scenes if b - a > 1)
        out = base.result(data)
        sr, sy, sb2, sd2, shit, smiss, sdt, ndt = acc.tolist()
        ne = max(n_ego, 1)
        ybar = sy / ne
        out.update(risk_mean=sr / ne, col_gt_agent=ybar, brier=sb2 / ne, brier_diag=sd2 / ne,
                   brier_base=ybar * (1.0 - ybar) if n_ego else 0.0,
                   risk_hit=shit / sy if sy else 0.0, risk_miss=smiss / (n_ego - sy) if n_ego - sy else 0.0,
                   t_first_err=sdt / ndt if ndt else 0.0, n_ego=n_ego, K=K, coll_dist=float(coll_dist))
        return out

    def refine_plans(self, obsv_p, plans, n_samples, dist, coll_dist=None, sub_batches=[], scene=None, ego=None, plan_start=None,
                     noise=None, row0=0, scale=1.0, obs_len=None, walls=None, wall_dist=None, w_wall=1.0, **descent):
        """"What is the nearest path that does NOT run into somebody?" - plan_risk() turned round: every candidate path is moved
        away from the K sampled futures of the scene's pedestrians by gradient descent on the expected clearance penalty (the
        penalty of set_clearance_loss() at distance `dist`, averaged over each agent's K draws - given the observations the
        agents' draws are independent, so this is the mean over all K^n joint futures), held near the original by a tracking
        and a smoothness term.  obsv_p, plans, n_samples, sub_batches, scene, ego, plan_start, noise, row0, scale, obs_len as
        plan_risk(): `ego` xor `plan_start`; with ego the plans start at obsv_p[ego[q], -1], the ego's own draws are left out and
        its observed track stays in the social block.  dist and coll_dist (default dist) are in the units of scale * obsv_p.
        descent: n_iter=32, lr=0.1, w_track=0.05, w_smooth=0.5, max_move=0.5 (ops.plan_refine).  ONE sampling launch, the draws
        Generator.sample() returns, ONE refine launch for all iterations (ops.plan_refine) and ONE risk launch on the original
        and the refined plans side by side (ops.plan_risk at coll_dist).  The draws are OPEN-LOOP: the pedestrians do not
        react to the plan, neither to the original nor to the refined one.
        Returns (refined (Q, P, n_next, 2), risk (Q, P, 2) before | after, cost (Q, P, 2, 3) and moved (Q, P) - the columns of
        ops.plan_refine -, trajs (K, B, n_next, 4)).  Works at any hidden size: it needs only Generator.sample().
        walls (M, 2, 2) or (M, 4), a tensor (SceneDataset.walls_from_world) or host data in the coordinates of obsv_p: the static
        map.  The refine launch then also descends w_wall * the penalty of the plan's own segments against the walls at the
        distance wall_dist (default dist; the units of scale * obsv_p) - ops.plan_refine(walls=...), cost (Q, P, 2, 4) with the
        unweighted wall penalty last - and ONE more launch (ops.path_walls at coll_dist) measures the original and the refined
        plans side by side: self.last_walls = (clear (Q, P, 2), first (Q, P, 2) int32), before | after; None after a call
        without walls.  Where a plan CROSSES a wall the wall gradient is exactly 0: descent cannot undo a crossing, last_walls
        reports it.  The tuple returned keeps its arity."""
        ops.refuse_wall_grid(walls, "refine_plans")
        dist = float(dist)
        coll_dist = dist if coll_dist is None else coll_dist
        if not float(coll_dist) >= 0.0:
            raise ValueError("coll_dist must be >= 0, got %r" % (coll_dist,))
        K, B, plans, sb, scene, ego, plan_start = _plan_queries(self.n_next, obsv_p, plans, n_samples, sub_batches, scene, ego,
                                                                plan_start, scale)
        wall = {}
        if walls is not None:
            wall = dict(walls=ops.walls_arg(walls, obsv_p.device), wall_d0=(dist if wall_dist is None else float(wall_dist)) / float(scale),
                        w_wall=w_wall)
        ops.check_descent(dist / float(scale), **{k: v for k, v in wall.items() if k != "walls"}, **descent)
        dev = obsv_p.device
        L.require_gpu(obsv_p)
        if obs_len is not None:
            if not isinstance(self.G, Generator):      # the generic-width and wide paths: no ragged kernels
                refuse_obs_len(obs_len, type(self).__name__)
            obs_len = ops.obs_len_arg(obs_len, B, obsv_p.shape[1], 2, dev)
        with torch.no_grad():
            scenes = ops.SceneIndex.get(sb, B, dev)
            q_scene = torch.from_numpy(scene).to(dev)
            q_ego = None
            if ego is not None:
                q_ego = torch.from_numpy(ego).to(dev)
                plan_start = obsv_p[q_ego.long(), -1, :2]
            plans, plan_start = plans.to(dev), plan_start.to(dev)
            P = plans.shape[1]
            ph = self.G.sample(obsv_p, K, self.n_next, sub_batches, noise, row0=row0, obs_len=obs_len)
            refined, cost, moved = ops.plan_refine(ph, obsv_p[:, -1], scenes, K, plans, plan_start, q_scene, q_ego,
                                                   dist / float(scale), inv_ss=float(scale), **wall, **descent)
            both = torch.cat([plans, refined], 1)
            risk = ops.plan_risk(ph, obsv_p[:, -1], scenes, K, both, plan_start, q_scene, q_ego, coll_dist, inv_ss=float(scale))[0]
            self.last_walls = None
            if walls is not None:
                clear, first, _ = _plan_walls(both, plan_start.float(), wall["walls"], coll_dist, float(scale))
                self.last_walls = (torch.stack([clear[:, :P], clear[:, P:]], dim=2), torch.stack([first[:, :P], first[:, P:]], dim=2))
            return refined, torch.stack([risk[:, :P], risk[:, P:]], dim=2), cost, moved, ph

    REFINE_KEYS = ("risk_cv", "risk_ref", "col_cv", "col_ref", "pen_cv", "pen_ref", "moved")

    def evaluate_refine(self, data, n_gen_samples=20, dist=0.5, coll_dist=0.1, just_one=False, collect=None, noise=None, walls=None,
                        wall_dist=None, w_wall=1.0, **descent):
        """evaluate() plus an answer to: does refining a naive plan against the PREDICTED futures make it collide less with the
        TRUE ones?  Leave-one-out like evaluate_risk(): every held-out agent of a scene of two or more agents is the ego once.
        Its naive plan is the constant-velocity extrapolation of its observations (predict_cv: the preds_lnr of the records; on
        ragged histories of its valid frames); refine_plans() moves it away from the K draws of the scene's other agents (dist,
        coll_dist in world units through data.ss like evaluate_scenes(); descent: ops.plan_refine).  Over the egos - returns a
        dict:
          ade_avg, fde_avg, ade_min, fde_min  the numbers of evaluate() from the same RNG state, bit for bit;
          risk_cv, risk_ref    the mean predicted risk (plan_risk() at coll_dist) of the naive and of the refined plan;
          col_cv, col_ref      the share of egos whose naive / refined plan comes closer than coll_dist to the TRUE future of
                               another agent of its scene (the K = 1 risk launch on the ground truth);
          pen_cv, pen_ref      the mean expected penalty of the two (pen_ref <= pen_cv is what the descent is for);
          moved                the mean largest displacement of a waypoint, in world units;
          n_ego, K, dist, coll_dist.
        The draws are open-loop and so is the ground truth: nobody reacts to the refined plan.  Chunking, noise streams and
        sampling launches are evaluate()'s; per chunk one refine launch and two risk launches.  A dataset with pred_len (ragged
        futures): a pedestrian counts while it is present, in the refinement and in both risks, and both risks count the ego's
        frames as evaluate_risk() does.  Sums are float64 on the device,
        one host sync at the end.  With `collect` every record of evaluate() also has `plan_ref` (n, n_next, 2; denormalised),
        `risk_plan`, `hit_plan` (n, 2: naive | refined) and `moved` (n,).
        walls (the static map in the coordinates of the dataset: data.walls_from_world()): the refinement carries the wall term
        (refine_plans(walls=...): wall_dist, default dist, in world units; w_wall), one more launch per chunk (ops.path_walls)
        measures both plans, and the dict gains
          wall_cv, wall_ref    the share of egos whose naive / refined plan comes within coll_dist of a wall;
          penw_cv, penw_ref    the mean wall penalty of the two;
        the records `wall_plan` (n, 2): the clearance of the two plans to the walls, in world units, and `penw_plan` (n, 2):
        their wall penalties."""
        if not float(coll_dist) >= 0.0:
            raise ValueError("coll_dist must be >= 0, got %r" % (coll_dist,))
        ss = float(data.ss)
        ops.refuse_wall_grid(walls, "evaluate_refine")
        wall = {}
        if walls is not None:
            wall = dict(walls=ops.walls_arg(walls, self.device), wall_d0=(float(dist) if wall_dist is None else float(wall_dist)) * ss,
                        w_wall=w_wall)
        d0 = ops.check_descent(float(dist) * ss, **{k: v for k, v in wall.items() if k != "walls"}, **descent)[0]      # world units -> the dataset's
        dn = self._device_noise(noise)
        dev, K = self.device, int(n_gen_samples)
        inv_ss = 1.0 / ss
        base = _EvalSums(dev)
        keys = self.REFINE_KEYS + (self.REFINE_WALL_KEYS if walls is not None else ())
        acc = torch.zeros(len(keys), dtype=torch.float64, device=dev)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        for c in self._eval_draws(data, K, just_one, dn, base):
            q_scene, multi = c.scenes.row_scene()
            q_ego = torch.arange(c.n, dtype=torch.int32, device=dev)
            start = c.obsv[:, -1]
            naive = predict_cv(c.obsv, self.n_next)
            if c.obs_len is not None and c.obsv.shape[1] > 2:      # the rule of the records' preds_lnr
                naive = torch.where((c.obs_len <= 2)[:, None, None], predict_cv(c.obsv[:, -2:], self.n_next), naive)
            naive, pstart = naive[:, None, :, :2].contiguous(), start[:, :2].contiguous()
            refined, cost, moved = ops.plan_refine(c.ph, start, c.scenes, K, naive, pstart, q_scene, q_ego, d0, inv_ss,
                                                   lens=c.pred_len, **wall, **descent)
            both = torch.cat([naive, refined], 1)
            risk = ops.plan_risk(c.ph, start, c.scenes, K, both, pstart, q_scene, q_ego, coll_dist, inv_ss, lens=c.pred_len,
                                 plan_lens=c.pred_len)[0]
            hit = ops.plan_risk(c.pred, start, c.scenes, 1, both, pstart, q_scene, q_ego, coll_dist, inv_ss, lens=c.pred_len,
                                plan_lens=c.pred_len)[2][:, :, 0] > 0
            rows = torch.cat([risk.double(), hit.double(), cost[:, 0, :, 0].double(), moved.double()], dim=1)      # (n, 7)
            extra = {}
            if walls is not None:
                wclear, wfirst, _ = _plan_walls(both, pstart, wall["walls"], coll_dist, inv_ss, c.pred_len)
                rows = torch.cat([rows, (wfirst >= 0).double(), cost[:, 0, :, 3].double()], dim=1)      # (n, 11)
                extra = dict(wall_plan=(wclear, 0), penw_plan=(cost[:, 0, :, 3], 0))
            acc += torch.where(multi[:, None], rows, zero).sum(0)
            if collect is not None:
                for rec in self._eval_records(data, c, c.ph, dict(plan_ref=(refined[:, 0], 0), risk_plan=(risk, 0), hit_plan=(hit, 0),
                                                                  moved=(moved[:, 0], 0), **extra)):
                    rec["plan_ref"] = data.scale.denormalize(rec["plan_ref"])
                    collect.append(rec)
        n_ego = sum(b - a for a, b in base.scenes if b - a > 1)
        out = base.result(data)
        out.update(zip(keys, (acc / max(n_ego, 1)).tolist()))
        out.update(n_ego=n_ego, K=K, dist=float(dist), coll_dist=float(coll_dist))
        return out

    REFINE_WALL_KEYS = ("wall_cv", "wall_ref", "penw_cv", "penw_ref")
    WALL_KEYS = ("wall_draws", "wall_agents", "wall_blocked", "wall_gt", "ade_min_free", "fde_min_free", "t_first")

    def evaluate_walls(self, data, walls, n_gen_samples=20, wall_dist=0.1, just_one=False, collect=None, noise=None):
        """evaluate() plus the ENVIRONMENT collision rate of the K draws: how many of them walk through the static map of the
        recording?  walls: the map in the coordinates of the dataset (data.walls_from_world(load_walls(file))); wall_dist in
        world units through data.ss like the coll_dist of evaluate_scenes().  A draw CONFLICTS when a segment of it - from
        the last observed position on, the agent moving linearly between frames - comes closer than wall_dist to a wall.
        Returns a dict:
          ade_avg, fde_avg, ade_min, fde_min  the numbers of evaluate() from the same RNG state, bit for bit;
          wall_draws      the share of (draw, agent) that conflict;
          wall_agents     the share of agents with at least one conflicting draw;
          wall_blocked    the share of agents with NO clear draw;
          wall_gt         the same share for the true futures - 0 when the map fits the data;
          ade_min_free, fde_min_free   the best of the CLEAR draws, over the agents that have one (0 without such agents);
          t_first         the mean frame at which the first conflicting segment ends, over the conflicting draws (0 without);
          n_agents, n_free, K, wall_dist.
        Chunking, noise streams and sampling launches are evaluate()'s; per chunk ONE path-walls launch on the draws where
        they are (ops.path_walls) and one on the ground truth; the small reductions are torch ops on the device, float64 sums,
        one host sync at the end; the trajectories go to the host only when `collect` asks.  A dataset with pred_len (ragged
        futures): a segment counts while the agent is present, for the draws and the truth alike.  With `collect` every
        record of evaluate() also has `wall_clear` (K, n): the clearance of every draw to the walls, in world units,
        `wall_first` (K, n) and `err` (K, n, 2): the ADE | FDE of every draw as the sampling launch formed them.  Excluding the conflicting draws from sample_ranked() / sample_composed() / sample_modes() is score
        masking by the caller (score.masked_fill(clear < d, -inf)), not part of this call.  The wide and generic trainers take
        it through their sampling hook, like evaluate_scenes(): there the four numbers agree with evaluate() to rounding."""
        if not float(wall_dist) >= 0.0:
            raise ValueError("wall_dist must be >= 0, got %r" % (wall_dist,))
        walls = ops.walls_arg(walls, self.device)
        inv_ss = 1.0 / float(data.ss)
        if isinstance(walls, WallGrid):          # a map of any size (data.wall_grid_from_world): the reach, before any launch
            ops.check_wall_grid_arg(walls, walls.device, float(np.float32(wall_dist)) / float(np.float32(inv_ss)), "wall_dist * ss =")
        dn = self._device_noise(noise)
        dev, K = self.device, int(n_gen_samples)
        base = _EvalSums(dev)
        # conflicting draws | agents with one | agents with no clear draw | conflicting truths | sum min ADE, FDE of the clear
        # draws | agents with a clear draw | sum of the first frames
        acc = torch.zeros(8, dtype=torch.float64, device=dev)
        inf = torch.full((), float("inf"), device=dev)
        for c in self._eval_draws(data, K, just_one, dn, base):
            start = c.obsv[:, -1]
            clear, first, _ = ops.path_walls(c.ph, start, K, walls, wall_dist, inv_ss, lens=c.pred_len)
            gt_first = ops.path_walls(c.pred, start, 1, walls, wall_dist, inv_ss, lens=c.pred_len)[1][0]
            hit = first >= 0                                                       # (K, n)
            nhit = hit.sum(0)
            free = nhit < K
            best = torch.where(hit[:, :, None], inf, c.err).min(0)[0].double()     # (n, 2): the best of the clear draws
            best = torch.where(free[:, None], best, torch.zeros((), dtype=torch.float64, device=dev))
            acc += torch.stack([nhit.sum().double(), (nhit > 0).sum().double(), (~free).sum().double(), (gt_first >= 0).sum().double(),
                                best[:, 0].sum(), best[:, 1].sum(), free.sum().double(),
                                torch.where(hit, first, torch.zeros_like(first)).sum().double()])
            if collect is not None:
                collect.extend(self._eval_records(data, c, c.ph, dict(wall_clear=(clear, 1), wall_first=(first, 1), err=(c.err, 1))))
        n_agents = sum(b - a for a, b in base.scenes)
        out = base.result(data)
        draws, agents, blocked, gt, ade, fde, n_free, tsum = acc.tolist()
        na = max(n_agents, 1)
        out.update(wall_draws=draws / (K * na), wall_agents=agents / na, wall_blocked=blocked / na, wall_gt=gt / na,
                   ade_min_free=ade / n_free if n_free else 0.0, fde_min_free=fde / n_free if n_free else 0.0,
                   t_first=tsum / draws if draws else 0.0, n_agents=n_agents, n_free=int(n_free), K=K, wall_dist=float(wall_dist))
        return out

    # ------------------------------------------------------------------------------------------
    def checkpoint(self, epoch=None):
        """The reference's checkpoint dict (train.py:653-663), plus a 'noise' entry ({seed, step}) when self.noise is set."""
        G = self.G
        ck = {'epoch': self.epoch if epoch is None else epoch,
              'attentioner_dict': G.attention.state_dict(),
              'feature_embedder_dict': G.feature_embedder.state_dict(),
              'encoder_dict': G.encoder.state_dict(),
              'decoder_dict': G.decoder.state_dict(),
              'pred_optimizer': self.predictor_optimizer.state_dict(),
              'D_dict': self.D.state_dict(),
              'D_optimizer': self.D_optimizer.state_dict()}
        if self.noise is not None:       # the device stream continues where it stood; without one the dict is the reference's
            ck['noise'] = self.noise.state_dict()
        return ck

    def save(self, path, epoch=None):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(self.checkpoint(epoch), path)

    def load_checkpoint(self, ck):
        """Resume (train.py:622-634); optimizer entries are optional (weights-only dicts load too)."""
        if isinstance(ck, (str, os.PathLike)):
            ck = torch.load(ck, map_location=self.device)
        G = self.G
        G.attention.load_state_dict(ck['attentioner_dict'])
        G.feature_embedder.load_state_dict(ck['feature_embedder_dict'])
        G.encoder.load_state_dict(ck['encoder_dict'])
        G.decoder.load_state_dict(ck['decoder_dict'])
        self.D.load_state_dict(ck['D_dict'])
        for key, optim in (('pred_optimizer', self.predictor_optimizer), ('D_optimizer', self.D_optimizer)):
            if key in ck:
                if isinstance(optim, PackedAdam):
                    optim.load_state_dict(ck[key])
                    continue
                keep = {k: optim.param_groups[0].get(k) for k in ('fused', 'foreach', 'capturable')}
                optim.load_state_dict(copy.deepcopy(ck[key]))
                for k, v in keep.items():
                    optim.param_groups[0][k] = v
        self.epoch = int(ck.get('epoch', 0))
        if 'noise' in ck:                # written by a trainer with a DeviceNoise: the same stream goes on
            if self.noise is None:
                self.noise = DeviceNoise(0)
            self.noise.load_state_dict(ck['noise'])
        if self.pg is not None and self.world > 1:
            self.sync_replicas()
        return self.epoch + 1
