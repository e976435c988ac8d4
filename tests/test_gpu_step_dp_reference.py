"""_train_epoch() under real process groups against the float64 step of tests/_step_ref.py: what every rank's shard adds up
to, all-reduced bucket by bucket, with lr_g = lr_d = 0.0 so that every step of every epoch differentiates at the weights the
trainer was built with (see test_gpu_step_reference.py for the premise).

One test per world size, 2 and 3 (gloo, all ranks on cuda:0 - at most 4 processes with the GPU open, the parent included); a
world is spawned once and each worker runs all variants in turn.  The worker wraps tr._allreduce to clone every bucket to the
host right after the exchange (gloo's exchanges are never inside a graph, so every one passes the wrapper): at U = 1 two D
buckets and one G bucket per packed batch, and the epoch's sums, told apart by their dtype.  The parent holds every D bucket
and every G bucket of every packed batch of every epoch to the full-batch float64 gradient (GRAD_REL per tensor through the
packed slices, close_grads_branch_consistent), the epoch's loss rows and ADE / FDE to its losses (_close_out), the weights to
the initial ones bit for bit, and buckets, weights and Adam moments to be bit-identical across ranks.

Data: synth_tracks(18, SCENES, 8, 12, seed=21), batch_size 43: the 14 training scenes pack into batches of 43 / 26 / 37 agents
(all >= 20: the as-written variety term is legal) whose shards are asserted in `_shard_facts` before anything relies on
them - rank 0 is idle in batch 2 at world 3 (_empty_step); global row 19 falls to rank 0 (world 2) / rank 1 (world 3: r = 13
and, behind the idle rank, r = 19) in batches 1 and 2, and in batch 3 to rank 1 (r = 1) at world 2 and rank 2 (r = 0) at world 3.

Variants (U = 1): 1 dense, host z through draw=, 4 epochs (graph segments from the third); 2 train_epoch_ragged, default
route, obs_len[i] = 2 + (5 i) % 7 over the dataset's rows, NaN padding; 3 the same with ragged_fused + use_graph, 4 epochs;
4 dense with DeviceNoise, draw=None, 3 epochs - every rank seeds numpy differently, sync_rng() makes rank 0's label scalars
everyone's, the parent reproduces them from rank 0's seed and the z of packed batch i of epoch e from
DeviceNoise(seed).fill(B, 32, domain=TRAIN, step=3 e + i), noise.step == 9 on every rank; 5 variant 4 on the ragged dataset
with ragged_fused; 6 "fixed" (k = 3) + L2 with host z and with DeviceNoise (draws 1 .. 2 of the step); 7 the variety term as
written, host z.  Seed rule of tests/_ref64.py: the draw seed (host z) or the stream's seed (DeviceNoise) is the first of
SEEDS without an ambiguous unit over all steps of the variant, else the one with the fewest.
One run at the real learning rates (variant 5, 3 epochs) asserts only what holds exactly: replicas, both optimizers' t and
noise.step equal across ranks.  No closeness to a single process: two fp32 sums in different orders feed lr * sign(g).

Observed on an MI355X, largest max|err| / max|ref| (outputs; gradients), the same at both world sizes to the digits shown:
1.dense 3.8e-7; 1.11e-5 and the one tensor at 2.20e-5.  2.ragged 8.0e-8; 5.4e-6.  3.ragged_fused 1.1e-7; 1.12e-5.  4.dense_dn 7.7e-8;
6.9e-6.  5.ragged_fused_dn 2.2e-7; 9.4e-6 (one ambiguous unit, not flipped).  6.fixed 8.1e-8; 4.2e-6.  6.fixed_dn 4.5e-8; 7.7e-6.
7.variety 9.3e-8; 1.59e-5 and the two tensors at 2.82e-5 and 2.12e-5.  The three tensors past GRAD_REL carry bounds of their own, derived at
REL_OF below.  """
import hashlib
import os
import socket

import numpy as np
import pytest
import torch

import _step_ref as S
from _ref64 import (GRAD_REL, MAX_AMBIGUOUS, _close_grad, _close_out, _report, close_grads_branch_consistent, count_ambiguous,  # noqa: F401
                    pick_fewest)

pytestmark = pytest.mark.gpu

SCENES = [5, 1, 17, 8, 3, 9, 20, 2, 4, 18, 1, 6, 6, 6, 7, 3, 2, 1]
To, Tp, BATCH = 8, 12, 43
WSEED, NPSEED = 500, 1000          # torch seed of rank 0's weights (+ 1000 rank elsewhere), numpy seed of rank 0 (+ 17 rank)
# name -> (flags, ragged dataset, trainer keywords, z from "host" | "device", epochs)
VARIANTS = {
    "1.dense": (S.flags(), False, {}, "host", 4),
    "2.ragged": (S.flags(), True, {}, "host", 1),
    "3.ragged_fused": (S.flags(), True, dict(ragged_fused=True, use_graph=True), "host", 4),
    "4.dense_dn": (S.flags(), False, {}, "device", 3),
    "5.ragged_fused_dn": (S.flags(), True, dict(ragged_fused=True), "device", 3),
    "6.fixed": (S.flags(variety="fixed", variety_k=3, l2=True), False, {}, "host", 1),
    "6.fixed_dn": (S.flags(variety="fixed", variety_k=3, l2=True), False, {}, "device", 1),
    "7.variety": (S.flags(variety=True), False, {}, "host", 1),
}
REAL_LR = "5.ragged_fused_dn"


def _dataset(ragged, device="cuda:0"):
    import socialways_amd as sw
    t = sw.synth_tracks(18, SCENES, To, Tp, seed=21)
    if not ragged:
        return sw.SceneDataset(t["obsvs"], t["preds"], t["batches"], device=device)
    n = t["obsvs"].shape[0]
    ln = (2 + (5 * np.arange(n)) % 7).astype(np.int32)
    data = sw.SceneDataset(t["obsvs"], t["preds"], t["batches"], device=device, obs_len=ln)
    pad = torch.arange(To)[None, :] < (To - torch.from_numpy(ln).long())[:, None]
    data.obsv[pad.to(data.obsv.device)] = float("nan")      # nothing in front of a row's valid frames is ever read
    return data


class HostDraws:
    """draw(bs) of train_epoch(): the label scalars, z and - "fixed" - the extra samples' z of the whole packed batch."""

    def __init__(self, seed, f):
        self.rs, self.gen, self.f = np.random.RandomState(seed), torch.Generator().manual_seed(seed), f

    def __call__(self, bs):
        d = (float(self.rs.uniform(0, 0.1)), float(self.rs.uniform(0.9, 1.0)), torch.rand(bs, 32, generator=self.gen))
        if self.f.variety == "fixed":
            d += (torch.rand(self.f.variety_k - 1, bs, 32, generator=self.gen),)
        return d


def _sha(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _trainer(name, seed_offset=0, pg=None, device="cuda:0", **lr):
    import socialways_amd as sw
    f, _, kw, _, _ = VARIANTS[name]
    torch.manual_seed(WSEED + sorted(VARIANTS).index(name) + seed_offset)
    return sw.SocialWaysTrainer(Tp, use_social=True, device=device, process_group=pg, **S.trainer_kw(f), **kw, **lr)


def _run_variant(name, rank, pg, seed, real_lr=False):
    """One variant on one rank -> what the parent compares (arrays from rank 0 only, hashes from everyone)."""
    import socialways_amd as sw
    f, ragged, _, zsrc, epochs = VARIANTS[name]
    data = _dataset(ragged)
    tr = _trainer(name, 1000 * rank, pg, **({} if real_lr else dict(lr_g=0.0, lr_d=0.0)))
    w0 = (tr.D._flat.clone(), tr.G._flat_all.clone())
    buckets, real = [], tr._allreduce

    def tap(flat):
        real(flat)
        if flat.dtype == torch.float32:          # a gradient bucket; the epoch's sums are float64
            buckets.append(flat.detach().cpu().clone())
    tr._allreduce = tap
    np.random.seed(NPSEED + 17 * rank)           # differs per rank on purpose: sync_rng() makes rank 0's stream everyone's
    draw = None
    if zsrc == "device":
        tr.noise = sw.DeviceNoise(seed)
    else:
        draw = HostDraws(seed, f)
    res = []
    for _ in range(3 if real_lr else epochs):
        ade, fde, losses, sizes = (tr.train_epoch_ragged if ragged else tr.train_epoch)(data, BATCH, draw=draw)
        res.append((ade, fde, np.asarray(losses), sizes))
    torch.cuda.synchronize()
    opts = (tr.D_optimizer, tr.predictor_optimizer)
    out = dict(sha_buckets=[_sha(b) for b in buckets], n_buckets=[b.numel() for b in buckets],
               sha_state=[_sha(t) for t in (tr.D._flat, tr.G._flat_all) + tuple(x for o in opts for x in (o.m, o.v))],
               t=[o.t for o in opts], noise_step=None if tr.noise is None else tr.noise.step, epoch=tr.epoch,
               untouched=bool(torch.equal(tr.D._flat, w0[0]) and torch.equal(tr.G._flat_all, w0[1])),
               graphs=[(k[5], k[-2], k[-1], st["graph"] is not None) for k, st in tr._graphs.items()],
               sizes=[r[3] for r in res], epochs=[(r[0], r[1], r[2]) for r in res])
    if rank == 0:
        out.update(buckets=[b.numpy() for b in buckets], wD=tr.D._flat.cpu().numpy(), wG=tr.G._flat_all.cpu().numpy())
    tr.release_graphs()
    return out


def _worker(rank, world, port, ret, seeds):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.pop("SW_GRAPH_COLLECTIVES", None)
    os.environ.pop("SW_ALLREDUCE", None)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {name: _run_variant(name, rank, dist.group.WORLD, seeds[name]) for name in sorted(VARIANTS)}
    out["real_lr"] = _run_variant(REAL_LR, rank, dist.group.WORLD, seeds[REAL_LR], real_lr=True)
    ret[rank] = out
    dist.destroy_process_group()


# ---- the parent's side: the float64 reference of every packed batch of every epoch, once for both world sizes ---------------------
_cache = {}


def _labels(n):
    """Rank 0's label scalars of n packed batches with draw=None: its numpy stream, two uniforms per batch (train.py:471-472)."""
    rs = np.random.RandomState(NPSEED)
    return [(float(rs.uniform(0, 0.1)), float(rs.uniform(0.9, 1.0))) for _ in range(n)]


def _device_z(seed, B, step, f):
    """(z, the extra samples' z or None) of the packed batch `step` of a DeviceNoise(seed) stream, for the whole batch."""
    import socialways_amd as sw
    from socialways_amd.noise import TRAIN
    K = f.variety_k if f.variety == "fixed" else 1
    z = sw.DeviceNoise(seed).fill(B, 32, domain=TRAIN, step=step, n_draws=K)[0].cpu()
    return z[0], (z[1:].reshape(-1, 32) if K > 1 else None)


def _reference(name, device="cuda:0"):
    """-> dict(seed, trainer (the slices' owner, rank 0's weights), refs [epoch][batch] = step64 result, steps, ...).  The weights
    are drawn on the CPU generator and the host draws need no device: device="cpu" gives the same reference of a host-z
    variant without a GPU (test_step_ref_host.py re-derives the per-case bounds below from it)."""
    if (name, device) in _cache:
        return _cache[name, device]
    f, ragged, _, zsrc, epochs = VARIANTS[name]
    data = _dataset(ragged, device)
    tr = _trainer(name, device=device, lr_g=0.0, lr_d=0.0)
    orc = S.oracle_of(tr.G, tr.D, Tp)
    steps = list(data.packed_steps(BATCH))
    assert [(b - a, len(sb)) for a, b, sb in steps] == [(43, 6), (26, 3), (37, 5)]
    ol = None if not ragged else data.obs_len.cpu().numpy()
    labels = _labels(epochs * len(steps))

    def make(seed):
        """The draws of every packed batch of every epoch: (zeros_val, ones_val, z, extra z)."""
        host, out = HostDraws(seed, f), []
        for e in range(epochs):
            for i, (a, b, sb) in enumerate(steps):
                if zsrc == "host":
                    d = host(b - a)
                    out.append((d[0], d[1], d[2], d[3].reshape(-1, 32) if len(d) > 3 else None))
                else:
                    out.append(labels[len(steps) * e + i] + _device_z(seed, b - a, len(steps) * e + i, f))
        return out

    def inputs(i):
        a, b, sb = steps[i % len(steps)]
        return data.obsv[a:b].cpu(), data.pred[a:b].cpu(), sb, (None if ol is None else ol[a:b])

    def ambiguous_of(draws):
        n = 0
        for i, (zv, ov, z, vn) in enumerate(draws):
            o, p, sb, ln = inputs(i)
            n += S.step_ambiguous(orc, orc.D, o, p, sb, z, obs_len=ln, variety_noise=vn, flags=f)
        return n
    seed, draws, n_amb = pick_fewest(make, ambiguous_of)
    assert n_amb <= MAX_AMBIGUOUS, (name, seed, n_amb)
    refs = []
    for i, (zv, ov, z, vn) in enumerate(draws):
        o, p, sb, ln = inputs(i)
        refs.append(S.step64(orc, orc.D, o, p, sb, zv, ov, z, ss=data.ss, obs_len=ln, variety_noise=vn, flags=f, seed=seed))
    _cache[name, device] = dict(seed=seed, tr=tr, refs=refs, steps=steps, ss=data.ss, n_train=data.n_train_samples, draws=draws,
                                inputs=inputs, tag="%s: seed %d, %d kink inputs near 0" % (name, seed, n_amb))
    return _cache[name, device]


def _shard_facts(world):
    """The shards the module's docstring promises, from shard_scenes() itself."""
    from socialways_amd.data import shard_scenes
    want = {2: [[(0, 23), (23, 43)], [(0, 20), (20, 26)], [(0, 18), (18, 37)]],
            3: [[(0, 6), (6, 23), (23, 43)], [None, (0, 20), (20, 26)], [(0, 18), (18, 19), (19, 37)]]}[world]
    steps = _reference("1.dense")["steps"]
    for (a, b, sb), rows in zip(steps, want):
        got = [None if hi <= lo else (int(sb[lo, 0]), int(sb[hi - 1, 1])) for lo, hi in shard_scenes(sb, world)]
        assert got == rows, (world, got, rows)
    owner = [[r for r, s in enumerate(rows) if s is not None and s[0] <= 19 < s[1]] for rows in want]
    assert owner == {2: [[0], [0], [1]], 3: [[1], [1], [2]]}[world]
    return want


# ---- the two buckets with bounds of their own ---------------------------------------------------------------------------------
# Of the 162 buckets a world compares (54 of them the generator's), three tensors of the social block in two generator buckets
# miss GRAD_REL, by 6 to 41 %.  All three are sums over a packed batch's pairs of dsigma_ij times a factor, where dsigma_ij = a_ij
# (q_ij - sum_k a_ik q_ik) is itself a difference and every row of dsigma sums to zero:
#   variant 1, epoch 3, batch 3 (37 agents), d/d attention.W.bias = sum over 432 pairs of dsigma_ij f_ij.  Its largest entry is
#     6.7e-8 in this step, 3 to 9 times smaller than in the variant's eleven other steps, from terms of the same size: their
#     absolute values add up to 42 .. 64 times the result (5 .. 16 times elsewhere).  The all-reduced bucket misses float64 by
#     2.20e-5 of that entry, at both world sizes (1.47e-12 absolute, as in the other steps);
#   variant 7, epoch 1, batch 2 (26 agents: scenes of 20, 2 and 4), where the as-written variety term puts the L2 of one agent,
#     row 19, undivided by the batch size onto d/d(pred_hat), so one row of dsigma carries the social block's gradient:
#     d/d attention.W.bias misses by 2.82e-5, and d/d feature_embedder.fc.4.bias = sum over 420 pairs of dsigma_ij Wh_j, the tensor
#     of REL_200_3 (tests/test_gpu_gen_reference.py; absolute sum 13 .. 25 times the result), by 2.12e-5.
# The bound is REL_200_3's: 4 x the fp32 CPU oracle's own error against float64 on that very case (two fp32 evaluations in
# different orders); the kernels' error does not enter it.  The oracle has two fp32 formulations of the social block, the
# reference's own op sequence ("faithful") and the block-diagonal one: the same sums in two orders.  They miss float64 by
# (faithful / block-diagonal) 1.46e-5 / 4.31e-6, 1.39e-5 / 9.46e-6 and 9.60e-6 / 6.47e-6 on the three tensors in the order above
# (and on batch 1 of variant 7 the faithful one misses fc.4.bias by 2.95e-5, past GRAD_REL itself).  The larger of the two is
# what an honest fp32 evaluation of that sum is off by, and it is the figure taken; with the block-diagonal one alone the first
# tensor would stay 28 % past its bound, the other two would pass.  test_step_ref_host.py recomputes the six figures on the
# CPU.  Every other tensor of the two buckets stays at GRAD_REL.
OWN_ERROR = {("1.dense", 3, 3, "attention.W.bias"): 1.46e-5,           # (variant, epoch, batch, tensor) -> the fp32 oracle's own error
             ("7.variety", 1, 2, "attention.W.bias"): 1.39e-5,
             ("7.variety", 1, 2, "feature_embedder.fc.4.bias"): 9.60e-6}
REL_DENSE_E3B3_ATT_BIAS = 4 * 1.46e-5
REL_VARIETY_E1B2_ATT_BIAS = 4 * 1.39e-5
REL_VARIETY_E1B2_FC4_BIAS = 4 * 9.60e-6
REL_OF = {("1.dense", 3, 3, "G bucket"): {"attention.W.bias": REL_DENSE_E3B3_ATT_BIAS},        # (variant, epoch, batch, bucket)
          ("7.variety", 1, 2, "G bucket"): {"attention.W.bias": REL_VARIETY_E1B2_ATT_BIAS,
                                            "feature_embedder.fc.4.bias": REL_VARIETY_E1B2_FC4_BIAS}}


def fp32_oracle_own_error(name, epoch, batch, tensor, device="cpu"):
    """{formulation: max|err| / max|ref|} of the fp32 CPU oracle's generator gradient `tensor` against float64 on packed batch
    `batch` of epoch `epoch` (1-based) of a host-z variant, at the seed the seed rule picks -> (seed, errors)."""
    f = VARIANTS[name][0]
    R = _reference(name, device)
    i = len(R["steps"]) * (epoch - 1) + batch - 1
    (zv, ov, z, vn), (o, p, sb, ln) = R["draws"][i], R["inputs"](i)
    want = R["refs"][i].g_run.grads()[tensor]
    out = {}
    for social in ("faithful", "blockdiag"):
        o32 = S.oracle_of(R["tr"].G, R["tr"].D, Tp, dtype=torch.float32)
        o32.social = social
        got = S.step64(o32, o32.D, o, p, sb, zv, ov, z, ss=R["ss"], obs_len=ln, variety_noise=vn, flags=f,
                       dtype=torch.float32).g_run.grads()[tensor]
        out[social] = float((got.double() - want).abs().max() / want.abs().max())
    return R["seed"], out


def _close_bucket(got, run, group, tag, rel_of):
    """close_grads_branch_consistent at GRAD_REL; a bucket with a bound of its own for some tensor (REL_OF) has no ambiguous
    unit, so it is _close_grad tensor by tensor, every other tensor still at GRAD_REL, all misses in one message."""
    if not rel_of:
        return close_grads_branch_consistent(got, run, group, tag)
    assert count_ambiguous(run.rec) == 0 and set(rel_of) <= set(got), tag
    ref, missed = run.grads(), []
    for k in got:
        try:
            _close_grad(got[k], ref[k], "d/d%s" % k, group, tag, rel_of.get(k, GRAD_REL))
        except AssertionError as err:
            missed.append(str(err))
    assert not missed, "; ".join(missed)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _check_variant(world, name, R, got, rows, misses):
    """One variant of one world: the replicas' state (asserted), then every bucket, loss row and epoch sum against float64 -
    those are all compared and every miss is appended to `misses`, so one run reports all of them."""
    f, ragged, tkw, zsrc, epochs = VARIANTS[name]
    g0 = got[0][name]
    tr, group = R["tr"], "dp%d.%s" % (world, name.split(".")[1])
    nD, nG, nb = tr.D._gflat.numel(), tr.G._gflat_all.numel(), len(R["steps"])

    def soft(fn, *args):
        try:
            fn(*args)
        except AssertionError as err:
            misses.append(str(err).splitlines()[0])
    # replicas: buckets, weights and moments bit-identical across ranks; weights untouched; the stream counted by everyone
    for r in range(world):
        g = got[r][name]
        assert g["sha_buckets"] == g0["sha_buckets"] and g["sha_state"] == g0["sha_state"], (name, r)
        assert g["untouched"] and g["t"] == g0["t"] == [2 * nb * epochs, nb * epochs], (name, r, g["untouched"], g["t"])
        assert g["noise_step"] == (nb * epochs if zsrc == "device" else None) and g["epoch"] == epochs, (name, r)
        assert g["n_buckets"] == [nD, nD, nG] * (nb * epochs), (name, r)
        if f.variety != "fixed" and (not ragged or tkw.get("ragged_fused")):
            # the graph route: one layout per packed batch this rank has rows of, ragged / z by address as the variant says;
            # four epochs capture every layout (two eager steps, and a workspace that grows on the way drops the counters once)
            idle = sum(row[r] is None for row in rows)
            assert 1 <= len(g["graphs"]) <= nb - idle, (name, r, g["graphs"])
            assert all(c[0] == 1 and c[1] == ragged and c[2] == (zsrc == "device") for c in g["graphs"]), (name, r, g["graphs"])
            assert epochs < 4 or (len(g["graphs"]) == nb - idle and all(c[3] for c in g["graphs"])), (name, r, g["graphs"])
        else:                 # the default ragged route and the folded K-sample step run eagerly
            assert not g["graphs"], (name, r, g["graphs"])
    assert np.array_equal(g0["wD"], tr.D._flat.cpu().numpy()) and np.array_equal(g0["wG"], tr.G._flat_all.cpu().numpy()), name
    # every bucket of every packed batch against the full-batch float64 gradient
    for e in range(epochs):
        ade, fde, losses = g0["epochs"][e]
        for i in range(nb):
            ref = R["refs"][nb * e + i]
            tag = "%s, epoch %d batch %d, %d ranks" % (R["tag"], e + 1, i + 1, world)
            b3 = g0["buckets"][3 * (nb * e + i):3 * (nb * e + i) + 3]
            for what, bkw, run in (("D bucket 1", dict(d_bucket=b3[0]), ref.d_run), ("D bucket 2", dict(d_bucket=b3[1]), ref.d_run),
                                   ("G bucket", dict(g_bucket=b3[2]), ref.g_run)):
                soft(_close_bucket, S.bucket_grads(tr, **bkw), run, group, "%s, %s" % (tag, what),
                     REL_OF.get((name, e + 1, i + 1, what), {}))
            soft(_close_out, torch.from_numpy(losses[i]), torch.from_numpy(ref.losses), "MSE terms", group, tag)
        want = R["refs"][nb * e:nb * e + nb]
        soft(_close_out, torch.tensor([ade, fde]), torch.tensor([sum(r.ade for r in want), sum(r.fde for r in want)]) / R["n_train"],
             "epoch ADE / FDE", group, "%s, epoch %d, %d ranks" % (R["tag"], e + 1, world))
        assert g0["sizes"][e] == [(b - a, len(sb)) for a, b, sb in R["steps"]]


def _check_world(world):
    import torch.multiprocessing as mp
    rows = _shard_facts(world)
    assert rows[1][0] is None if world == 3 else all(r is not None for b in rows for r in b)
    refs = {name: _reference(name) for name in sorted(VARIANTS)}
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _port(), ret, {k: v["seed"] for k, v in refs.items()}), nprocs=world, join=True)
    got = [ret[r] for r in range(world)]
    misses = []
    for name in sorted(VARIANTS):
        try:
            _check_variant(world, name, refs[name], got, rows, misses)
        except AssertionError as err:
            misses.append("%s, %d ranks, the replicas' state: %s" % (name, world, str(err).splitlines()[0]))
    assert not misses, "%d checks failed:\n%s" % (len(misses), "\n".join(misses))
    # the real learning rates: only what holds exactly
    r0 = got[0]["real_lr"]
    assert not r0["untouched"] and r0["t"] == [18, 9] and r0["noise_step"] == 9
    for r in range(1, world):
        g = got[r]["real_lr"]
        assert g["sha_state"] == r0["sha_state"], "rank %d: replicas diverged at the real learning rates" % r
        assert g["t"] == r0["t"] and g["noise_step"] == r0["noise_step"] and g["sha_buckets"] == r0["sha_buckets"]


@pytest.mark.timeout(600)
def test_two_ranks_every_bucket_of_every_epoch_against_float64():
    """Observed wall time on an MI355X box: 12 s, of which the float64 references both tests share take about 7."""
    _check_world(2)


@pytest.mark.timeout(600)
def test_three_ranks_with_an_idle_rank_every_bucket_of_every_epoch_against_float64():
    """Observed wall time on an MI355X box: 5 s with the references already computed."""
    _check_world(3)
