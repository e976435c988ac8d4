"""The wall term of the generator loss on the GPU: sw_wall_grad / ops.wall_grad / stats.wall_penalty against the float64
reference of tests/_wall_loss_ref.py, its exactness properties bit for bit, and SocialWaysTrainer.step() with set_wall_loss()
against the float64 step of tests/_step_ref.py plus the float64 gradient of L_wall alone.

a. kernel   the rows of _wall_loss_ref.GPU_CASES: R = K B of 1, 63, 64, 65, 129 (3 x 43) and 130; Tp 1 / 12 / 17 / 25 (no segment
            without start at Tp 1; one and two time chunks and the point they share); M 0, 1, 3, 5, 33, 130 and 1024; with and
            without start; pstride and dstride 2 and 4; ragged lens with NaN padding, one beyond Tp and one below 1; dpos zero
            and pre-filled.  Bound: max|err| <= 2e-5 max|ref| (GRAD_REL of tests/_ref64.py) for dpos and for loss; count equal
            off the near mask; a split-ambiguous path (at most 5 % of a case, near at most 1 %, by the choice of the seed) is
            compared on loss, count and the sum of g over its points.
b. exact    rows with count 0 and every row at M = 0 untouched, two calls, a path alone / in its batch / with the others
            permuted, a crossing, a post, a motionless segment, the parallel corridor, a wall exactly dw away (not counted, its
            rows not read: profiles/seeded_faults_r2.txt), count = nseg of ops.path_walls.
c. stats    stats.wall_penalty = the ops call, bit for bit, for (B, .) and (K, B, .) inputs.
d. step     trainers with lr_g = lr_d = 0 on [8, 3, 1, 17] (29 agents), To 8, Tp 12, dist 2 (dw = dist * ss = 0.5), weight 1.5,
            5 walls beside the agents' last observed positions: every generator gradient against step64(...).g_run + the
            float64 gradient of L_wall through orc.predict, at close_grads_branch_consistent's bound; D's gradients and the
            loss rows bit-identical to the same step without the term; last_wall_loss against the reference.  Routes: eager,
            graph (2 eager, capture, 2 replays), step_many of 3, + L2, "fixed" variety (K = 3), ragged, ragged_fused captured,
            two scene shards, both terms on.
e. effect   tests/golden/biwi_synth.npz, its training scenes as one packed batch, the four sides of the bounding box of the
            true futures as walls, 300 steps at lr_g 1e-3: the run with the term on (dist 2 m, weight 20) ends with a lower
            last_wall_loss[0].sum() than the same run with weight 0.

Observed on an MI355X (pytest -s), largest max|err| / max|ref|: a. dpos 2.13e-6 (R 130, Tp 25, M 33), loss 1.10e-7, every count
equal; no near path, 1 of 65 (M 130) and 2 of 130 (Tp 25, M 33) split-ambiguous paths at seed 1, none in the other cases.  b. parallel
corridor 1.3e-7, the rest exact.  d. generator gradients: eager 3.86e-6, graph 1.96e-5, step_many 4.23e-6, + L2 7.04e-6, "fixed"
4.21e-6, ragged 5.18e-6, ragged_fused 3.59e-6, two shards 3.81e-6, both terms 3.79e-6; outputs 3.4e-7; no ambiguous unit.
e. penalty sum 259.30 at step 1, 138.20 (weight 20) against 489.59 (weight 0) at step 300.  The 29 cases take 8.5 s together.
"""
import numpy as np
import pytest
import torch

import _step_ref as S
import _wall_loss_ref as WR
import _walls_ref as W
from _ref64 import SEEDS, RefRun, _close_grad, _f64, _note, _report, gen_mods, gen_params  # noqa: F401
from _util import golden
from test_gpu_clearance_loss import DIST as CDIST, WEIGHT as CWEIGHT, _col_ref, _with_col
from test_gpu_ragged_train import dev_len
from test_gpu_step_reference import SS, Case, _names, _step, calls, rule_a  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DW = WR.DW


def _bits(t):
    return t.contiguous().view(torch.int32)


def _widen(x, stride, fill):
    """(.., 2) numpy or tensor -> float32 tensor (.., stride) with `fill` in the columns behind x and y."""
    x = torch.as_tensor(x, dtype=torch.float32)
    if stride == 2:
        return x.clone()
    out = torch.full(x.shape[:-1] + (stride,), fill, dtype=torch.float32)
    out[..., :2] = x
    return out


def _call(pos, start, K, walls, dw, scale, dpos, lens=None, with_outputs=True):
    """ops.wall_grad on device copies -> (loss, count), NaN / -1 where the kernel did not write."""
    from socialways_amd import ops
    R = pos.shape[0] * (pos.shape[1] if pos.dim() == 4 else 1)
    loss = torch.full((R,), float("nan"), device=DEV) if with_outputs else None
    count = torch.full((R,), -1, dtype=torch.int32, device=DEV) if with_outputs else None
    ops.wall_grad(pos, None if start is None else torch.as_tensor(start).to(DEV), K, torch.as_tensor(walls).to(DEV), dw, scale, dpos,
                  loss, count, None if lens is None else torch.as_tensor(lens).to(DEV))
    torch.cuda.synchronize()
    return loss, count


# ---- a. the kernel against the float64 reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("row", WR.GPU_CASES, ids=lambda r: "k%d_b%d_tp%d_m%d_%s%s_p%dd%d" % (
    r[0], r[1], r[2], r[3], "start" if r[4] else "nostart", "_ragged" if r[5] else "", r[6], r[7]))
def test_kernel_against_float64(row):
    K, B, Tp, M, with_start, ragged, pstride, dstride = row
    case, pos, start, lens, ref = WR.gpu_case(*row)
    R, tag = K * B, "%s, seed %d" % (row, case["seed"])
    assert ref["split"].sum() <= WR.CAP_SPLIT * R and ref["near"].sum() <= WR.CAP_NEAR * R
    p = _widen(pos, pstride, 7.0)
    if ragged:
        for a in range(B):
            p[:, a, int(np.clip(lens[a], 1, Tp)):] = float("nan")
    p = p.to(DEV)
    gmax = float(np.abs(ref["grad"]).max())
    scale = 2.0 / gmax if gmax > 0 else 1.0                   # scale * g comparable to the unit-variance pre-fill
    gen = torch.Generator().manual_seed(case["seed"])
    for what, pre in (("dpos from zero", torch.zeros(R, Tp, 2)), ("dpos accumulated", torch.randn(R, Tp, 2, generator=gen))):
        before = _widen(pre, dstride, 3.0).reshape(K, B, Tp, dstride)
        dpos = before.to(DEV)
        loss, count = _call(p, start, K, case["walls"], DW, scale, dpos, lens)
        got = dpos.cpu()
        err, lerr = WR.compare(got[..., :2].numpy(), loss.cpu().numpy(), count.cpu().numpy(), ref, scale, pre.numpy())
        print("wall kernel  %-58s %-16s dpos %.2e  loss %.2e  (split %d, near %d, active %d of %d)"
              % (tag, what, err, lerr, ref["split"].sum(), ref["near"].sum(), ref["active"].sum(), R))
        _note("a.kernel", "grad", err)
        _note("a.kernel", "out", lerr)
        if dstride == 4:
            assert bool((got[..., 2:] == 3.0).all()), "columns 2 and 3 of dpos (%s)" % tag
        if ragged:
            for a in range(B):
                ln = int(np.clip(lens[a], 1, Tp))
                assert torch.equal(_bits(got[:, a, ln:]), _bits(before[:, a, ln:])), "rows behind a length are not written (%s)" % tag


# ---- b. exactness ---------------------------------------------------------------------------------------------------------------
def test_rows_with_nothing_counted_and_an_empty_map_are_not_touched():
    row = (1, 130, 12, 5, False, False)
    case, pos, start, lens, ref = WR.gpu_case(*row)
    idle = (ref["count"] == 0) & ~ref["near"]
    assert 20 <= idle.sum() <= 110
    pre = torch.randn(130, 12, 4, generator=torch.Generator().manual_seed(4))
    pre[:, 0, 0], pre[:, 3, 1], pre[:, :, 3] = -0.0, float("nan"), float("nan")
    dpos = pre.to(DEV)
    loss, count = _call(torch.as_tensor(pos[0]).to(DEV), None, 1, case["walls"], DW, 1.0, dpos)
    idle_t = torch.as_tensor(idle).to(DEV)
    assert torch.equal(_bits(dpos[idle_t]), _bits(pre.to(DEV)[idle_t])), "rows of paths with every |c| >= dw"
    assert not bool(loss[idle_t].any()) and not bool(count[idle_t].any()) and bool((count[~idle_t] > 0).any())
    assert not torch.equal(_bits(dpos[~idle_t][..., :2]), _bits(pre.to(DEV)[~idle_t][..., :2]))
    assert torch.equal(_bits(dpos[..., 2:]), _bits(pre[..., 2:].to(DEV))), "columns 2 and 3, NaN included"
    dpos = pre.to(DEV)                                        # M = 0: every row
    loss, count = _call(torch.as_tensor(pos[0]).to(DEV), None, 1, np.zeros((0, 2, 2), np.float32), DW, 1.0, dpos)
    assert torch.equal(_bits(dpos), _bits(pre.to(DEV))) and not bool(loss.any()) and not bool(count.any())


def test_two_calls_give_the_same_bits_and_a_path_does_not_see_the_batch():
    row = (1, 130, 25, 33, True, False)
    case, pos, start, lens, ref = WR.gpu_case(*row)
    pos, walls = pos[0], case["walls"]

    def run(rows):
        dpos = torch.zeros(len(rows), 25, 4, device=DEV)
        loss, count = _call(_widen(pos[rows], 4, 7.0).to(DEV), start[rows], 1, walls, DW, 0.5, dpos)
        return dpos, loss, count
    every = np.arange(130)
    d1, l1, c1 = run(every)
    d2, l2, c2 = run(every)
    assert bool(d1.any()) and torch.equal(_bits(d1), _bits(d2)) and torch.equal(_bits(l1), _bits(l2)) and torch.equal(c1, c2)
    d4 = torch.zeros(130, 25, 4, device=DEV)                  # loss and count are optional
    _call(_widen(pos, 4, 7.0).to(DEV), start, 1, walls, DW, 0.5, d4, with_outputs=False)
    assert torch.equal(_bits(d4), _bits(d1))
    perm = np.random.RandomState(3).permutation(130)
    d3, l3, c3 = run(perm)
    pt = torch.as_tensor(perm).to(DEV)
    assert torch.equal(_bits(d3), _bits(d1[pt])) and torch.equal(_bits(l3), _bits(l1[pt])) and torch.equal(c3, c1[pt])
    r = int(np.nonzero(ref["active"])[0][-1])                 # an active path, alone: another lane, another workgroup
    assert r >= 64
    d5, l5, c5 = run(np.array([r]))
    assert bool(d5.any()) and torch.equal(_bits(d5[0]), _bits(d1[r])) and torch.equal(_bits(l5[0]), _bits(l1[r])) and c5[0] == c1[r]
    # K = 2: the second draw of agent a is row B + a and reads start[a]
    dk = torch.zeros(2, 130, 25, 4, device=DEV)
    lk, ck = _call(_widen(np.stack([pos, pos]), 4, 7.0).to(DEV), start, 2, walls, DW, 0.5, dk)
    assert torch.equal(_bits(dk[0]), _bits(d1)) and torch.equal(_bits(dk[1]), _bits(d1)) and torch.equal(ck[130:], c1)


def _tiny(points, walls, start=None):
    P = torch.tensor([points], dtype=torch.float32)
    dpos = torch.zeros(1, P.shape[1], 2, device=DEV)
    loss, count = _call(P.to(DEV), None if start is None else np.array([start], np.float32), 1, np.array(walls, np.float32).reshape(-1, 2, 2),
                        0.5, 1.0, dpos)
    return dpos[0].cpu(), float(loss[0]), int(count[0])


def test_a_crossing_a_post_and_a_motionless_segment():
    g, loss, count = _tiny([[0.5, 0.25]], [[0.0, -1.0, 0.0, 1.0]], start=[-0.5, 0.25])
    assert not bool(g.any()) and loss == 1.0 and count == 1, "a crossing: phi = 1, gradient 0"
    # a post 0.25 beside the path at s = 1/4: u = 3/4, k = -12, w = k c = (0, 3)
    g, loss, count = _tiny([[0.0, 0.25], [1.0, 0.25]], [[0.25, 0.5, 0.25, 0.5]])
    assert g.tolist() == [[0.0, 2.25], [0.0, 0.75]] and loss == 0.5625 and count == 1
    # a motionless segment 0.25 above a wall: the first candidate wins, s = 0, everything lands on the segment's first point
    g, loss, count = _tiny([[0.0, 0.25], [0.0, 0.25]], [[-1.0, 0.0, 1.0, 0.0]])
    assert g.tolist() == [[0.0, -3.0], [0.0, 0.0]] and loss == 0.5625 and count == 1
    # ... and with a start point that first point is data
    g, loss, count = _tiny([[0.0, 0.25]], [[-1.0, 0.0, 1.0, 0.0]], start=[0.0, 0.25])
    assert not bool(g.any()) and loss == 0.5625 and count == 1


def test_the_parallel_corridor_ties_go_to_the_first_candidate():
    case = W.parallel_case()
    pos, start, walls = case["plans"][0], case["plan_start"], case["walls"]
    ref = WR.reference(pos, start, walls, 0.5)
    assert ref["count"][0] == pos.shape[1] and np.abs(ref["grad"]).max() > 0
    dpos = torch.zeros(1, pos.shape[1], 2, device=DEV)
    loss, count = _call(torch.as_tensor(pos).to(DEV), start, 1, walls, 0.5, 1.0, dpos)
    assert int(count[0]) == ref["count"][0] and not bool(dpos[0, -1].any()), "s = 0 wins every tie: the last point takes nothing"
    _close_grad(dpos.sum(1), torch.as_tensor(ref["grad"]).sum(1), "sum over the points", "b.exact", "parallel corridor")
    _close_grad(loss, torch.as_tensor(ref["loss"]), "loss", "b.exact", "parallel corridor")


NEG0 = np.float32(-0.0).view(np.int32)      # the bits of a pre-filled -0.0: a row that took `+= 0` holds +0.0 instead


def _written(dpos):
    """(.., Tp, >= 2) pre-filled with -0.0 -> bool (.., Tp): the kernel made its read-modify-write of the row"""
    return (_bits(dpos[..., :2].cpu()) != int(NEG0)).any(-1).numpy()


def test_a_wall_exactly_dw_away_is_not_counted_and_its_rows_keep_their_bits():
    """One segment (0, 0.5) -> (1, 0.5) above a wall on the x axis: |c|^2 = 0.25 = dw^2 exactly at dw = 0.5 (the reference's
    margin is 0, asserted), so the pair is not counted and the pre-filled -0.0 of the dpos rows is not even read; at dw = 0.75
    it is counted, u = 5 / 9: against the float64 reference, both rows rewritten."""
    pos, walls = np.array([[[0.0, 0.5], [1.0, 0.5]]], np.float32), np.array([[[-1.0, 0.0], [2.0, 0.0]]], np.float32)
    cc = W.closest(pos[0, 0].astype(np.float64), pos[0, 1].astype(np.float64), walls[0, 0], walls[0, 1])[2]
    assert float(cc) == 0.25 == float(np.float32(0.5) * np.float32(0.5))
    ref = WR.reference(pos, None, walls, 0.5)
    assert ref["count"][0] == 0 and not ref["grad"].any()
    dpos = torch.full((1, 2, 2), -0.0, device=DEV)
    loss, count = _call(torch.as_tensor(pos).to(DEV), None, 1, walls, 0.5, 1.0, dpos)
    assert int(count[0]) == 0 and float(loss[0]) == 0.0
    assert not _written(dpos).any(), "a pair that is not counted makes no read-modify-write"
    ref = WR.reference(pos, None, walls, 0.75)
    assert ref["count"][0] == 1 and abs(ref["grad"][0, 0, 1]) > 1.0
    dpos = torch.full((1, 2, 2), -0.0, device=DEV)
    loss, count = _call(torch.as_tensor(pos).to(DEV), None, 1, walls, 0.75, 1.0, dpos)
    WR.compare(dpos.cpu().numpy(), loss.cpu().numpy(), count.cpu().numpy(), ref)
    assert _written(dpos).all()


def test_count_is_nseg_of_path_walls():
    from socialways_amd import ops
    for seed in SEEDS:
        case = WR.walls_case(130, 12, 5, seed)
        pos, start = WR.split_case(case, True)
        margin = W.path_walls_reference(pos, start, case["walls"], DW)["margin"]
        if margin > 1e-4:
            break
    assert margin > 1e-4
    p, st, walls = torch.as_tensor(pos).to(DEV), torch.as_tensor(start).to(DEV), torch.as_tensor(case["walls"]).to(DEV)
    _, count = _call(p, start, 1, case["walls"], DW, 1.0, torch.zeros(1, 130, 12, 2, device=DEV))
    nseg = ops.path_walls(p, st, 1, walls, DW, 1.0)[2]
    assert int(nseg.sum()) > 0 and torch.equal(count, nseg.reshape(-1))


# ---- c. stats --------------------------------------------------------------------------------------------------------------------
def test_stats_wall_penalty_is_the_ops_call():
    from socialways_amd import stats
    case = WR.walls_case(3 * 43, 12, 33, 1, K=3)
    pos, start = WR.split_case(case, True)
    scale, dist = 4.0, 2.0                                       # trajs in quarter units: dw = dist / scale in theirs
    lens = np.random.RandomState(2).randint(1, 13, 43)
    loss, grad, count = stats.wall_penalty(pos, case["walls"].reshape(-1, 4), dist, start=start, scale=scale, lens=lens, device=DEV)
    dpos = torch.zeros(3, 43, 12, 4, device=DEV)
    l2, c2 = _call(_widen(pos, 4, 7.0).to(DEV), start, 3, case["walls"], dist / scale, 1.0, dpos, lens.astype(np.int32))
    assert grad.shape == (3, 43, 12, 2) and loss.shape == count.shape == (3, 43) and count.dtype == torch.int32 and bool(grad.any())
    assert torch.equal(_bits(grad), _bits(dpos[..., :2])) and torch.equal(_bits(loss.reshape(-1)), _bits(l2))
    assert torch.equal(count.reshape(-1), c2)
    l3, g3, c3 = stats.wall_penalty(torch.as_tensor(pos[1]), case["walls"], dist, scale=scale, device=DEV)      # (B, .), no start
    d3 = torch.zeros(43, 12, 2, device=DEV)
    l4, c4 = _call(torch.as_tensor(pos[1]).to(DEV), None, 1, case["walls"], dist / scale, 1.0, d3)
    assert l3.shape == (43,) and g3.shape == (43, 12, 2) and int(c3.sum()) > 0
    assert torch.equal(_bits(g3), _bits(d3)) and torch.equal(_bits(l3), _bits(l4)) and torch.equal(c3, c4)


# ---- d. the step ---------------------------------------------------------------------------------------------------------------
SIZES29 = [8, 3, 1, 17]
DIST, WEIGHT = 2.0, 1.5          # dw = DIST * SS = 0.5


def _predict(c, i):
    o, p, _, _, z, _ = c.draws[i]
    o64, z64 = o.double(), z.double()
    ln = None if c.lens is None else c.lens[i]
    return S._forms(c.orc, c.orc.D, o64, p.double(), c.sb, S._len(ln), c.Tp)[0], o64, z64


def _step_walls(c, steps):
    """5 walls, each with one end beside a random agent's last observed position: the first seed for which the float64 reference
    of every step in `steps` has a counted pair and no split-ambiguous one."""
    preds = []
    for i in steps:
        predict, o64, z64 = _predict(c, i)
        with torch.no_grad(), _f64():
            preds.append((predict(z64).numpy(), o64[:, -1].numpy()))
    for seed in SEEDS:
        rng = np.random.RandomState(seed)
        w0 = preds[0][1][rng.randint(0, c.B, 5)] + rng.normal(0, 0.3, (5, 2))
        walls = np.stack([w0, w0 + rng.normal(0, 1.0, (5, 2))], 1).astype(np.float32)
        refs = [WR.reference(ph, st, walls, DIST * SS, want_masks=True) for ph, st in preds]
        if all(r["count"].sum() > 0 and not r["split"].any() for r in refs):
            return walls
    raise AssertionError("no seed of %s gives walls with a counted pair and no split-ambiguous one" % (SEEDS,))


def _wall_ref(c, i, walls):
    """Float64: the gradient of L_wall alone with respect to every generator parameter (a RefRun), and the per-agent reference
    (loss, count, near) of the reference's prediction."""
    predict, o64, z64 = _predict(c, i)
    box = {}

    def fn():
        ph = predict(z64)
        box["ph"] = ph.detach()
        return WR.l_wall(ph, o64[:, -1], walls, DIST * SS, WEIGHT, c.B), None
    run, _ = S._run(gen_params(c.orc), gen_mods(c.orc), fn, c.seed, torch.float64)
    return run, WR.reference(box["ph"].numpy(), o64[:, -1].numpy(), walls, DIST * SS, want_masks=True)


def _group(tag):
    return "d." + tag.split(",")[0]          # one line per route in the module's report (pytest -s)


def _check_last(last, ref, tag):
    loss, count = last
    assert tuple(loss.shape) == ref["loss"].shape and count.dtype == torch.int32
    _close_grad(loss, torch.as_tensor(ref["loss"]), "last_wall_loss loss", _group(tag), tag)
    assert not bool(((count.cpu().long().numpy() != ref["count"]) & ~ref["near"]).any()), "last_wall_loss count (%s)" % tag
    assert int(ref["count"].sum()) > 0


def _check_on(c, out, i, tag, also=None):
    c.premise()
    d_got, g_got = S.trainer_grads(c.tr)
    run, ref = _wall_ref(c, i, c.walls)
    full = _with_col(c.ref(i), run)
    if also is not None:
        full = _with_col(full, also)
    c.compare(out, d_got, g_got, full, _group(tag), "step %d (%s)" % (i + 1, tag))
    _check_last(c.tr.last_wall_loss, ref, tag)


def _case(f=None, n_steps=1, on=True, **kw):
    c = Case(SIZES29, 8, 12, f or S.flags(), n_steps=n_steps, **kw)
    c.walls = _step_walls(c, range(n_steps))
    if on:
        c.tr.set_wall_loss(c.walls, DIST, WEIGHT)
    return c


def test_step_eager_and_the_term_switched_off_and_on(calls):
    c = _case(on=False, use_graph=False)
    _step(c, 0)                                # lazy initialisations make their launches here
    del calls[:]
    out0 = _step(c, 0).clone()
    d0, g0 = S.trainer_grads(c.tr)
    names0 = _names(calls)
    assert "sw_wall_grad" not in names0 and c.tr.last_wall_loss is None and "sw_dec_rollout_bwd_dfuse" in names0
    del calls[:]
    c.tr.set_wall_loss(c.walls, DIST, WEIGHT)
    out1 = _step(c, 0).clone()
    d1, g1 = S.trainer_grads(c.tr)
    assert _names(calls).count("sw_wall_grad") == 1 and "sw_dec_rollout_bwd_dfuse" not in _names(calls)
    assert _names(calls).index("sw_disc_dpred") < _names(calls).index("sw_wall_grad")
    _check_on(c, out1, 0, "eager")
    assert torch.equal(out0, out1), "the loss rows do not see the term"
    assert all(torch.equal(d0[k], d1[k]) for k in d0), "D's gradients do not see the term"
    assert any(not torch.equal(g0[k], g1[k]) for k in g0)
    del calls[:]
    c.tr.set_wall_loss(None)
    out2 = _step(c, 0)
    d2, g2 = S.trainer_grads(c.tr)
    assert _names(calls) == names0 and c.tr.last_wall_loss is None, "switched off: the launches of before"
    assert torch.equal(out0, out2) and all(torch.equal(g0[k], g2[k]) for k in g0) and all(torch.equal(d0[k], d2[k]) for k in d0)


def test_step_through_the_graph(calls):
    c = _case(n_steps=5)
    assert c.tr.use_graph
    held = c.tr.wall_loss[0]
    for i in range(5):
        del calls[:]
        out = _step(c, i)
        assert len(c.tr._graphs) == 1 and [k[-5] for k in c.tr._graphs] == [(held.data_ptr(), 5, DIST, WEIGHT)]
        assert [k[-4] for k in c.tr._graphs] == [None]
        st = next(iter(c.tr._graphs.values()))
        assert (st["graph"] is not None) == (i >= 2)
        if i >= 3:
            assert not calls, "a replayed step makes no launch of its own"
        elif i < 2:
            assert _names(calls).count("sw_wall_grad") == 1
        _check_on(c, out, i, "graph")
    c.tr.set_wall_loss(None)                 # another key: the captured graph with the term is not replayed
    _step(c, 0)
    assert len(c.tr._graphs) == 2 and c.tr.last_wall_loss is None


def test_step_many_of_three():
    c = _case(n_steps=9)
    for r in range(3):
        outs = c.tr.step_many([c.device_draw(i) for i in range(3 * r, 3 * r + 3)], c.sb, SS)
        torch.cuda.synchronize()
        assert [k[5] for k in c.tr._graphs] == [3]
        assert (next(iter(c.tr._graphs.values()))["graph"] is not None) == (r >= 2)
        _check_on(c, outs[2], 3 * r + 2, "step_many, launch %d" % (r + 1))      # p.grad and last_wall_loss are the last step's


def test_step_with_l2():
    c = _case(S.flags(l2=True))
    _check_on(c, _step(c, 0), 0, "+ L2")


def test_step_with_fixed_variety(calls):
    c = _case(S.flags(variety="fixed", variety_k=3))
    out = _step(c, 0)
    assert "sw_variety_grad" in _names(calls) and "sw_wall_grad" in _names(calls)
    _check_on(c, out, 0, "fixed variety, K = 3")


def test_step_ragged(calls):
    c = _case(lens=[rule_a(29)])
    out = _step(c, 0, obs_len=c.lens[0])
    assert not c.tr._graphs and "sw_disc_fwd_ragged" in _names(calls)
    _check_on(c, out, 0, "ragged")


def test_step_ragged_fused_captured():
    c = _case(n_steps=4, lens=[rule_a(29)] * 4, ragged_fused=True)
    for i in range(4):
        out = _step(c, i, obs_len=dev_len(c.lens[i]))
        st = next(iter(c.tr._graphs.values()))
        assert [k[-2] for k in c.tr._graphs] == [True] and (st["graph"] is not None) == (i >= 2)
        if i >= 2:
            _check_on(c, out, i, "ragged_fused, %s" % ("captured" if i == 2 else "replayed"))


def test_two_scene_shards_add_up():
    c = _case()
    o, p, zv, ov, z = c.device_draw(0)
    run, wref = _wall_ref(c, 0, c.walls)
    ref = _with_col(c.ref(0), run)
    out_sum, d_sum, g_sum, loss, count = 0.0, None, None, [], []
    for lo, hi in ((0, 2), (2, 4)):
        r0, r1 = int(c.sb[lo, 0]), int(c.sb[hi - 1, 1])
        out = c.tr.step(o[r0:r1], p[r0:r1], c.sb[lo:hi] - r0, zv, ov, z[r0:r1], SS, global_B=c.B, global_row0=r0)
        c.premise()
        d_got, g_got = S.trainer_grads(c.tr)
        out_sum = out_sum + out.double()
        d_sum = d_got if d_sum is None else {k: d_sum[k] + v for k, v in d_got.items()}
        g_sum = g_got if g_sum is None else {k: g_sum[k] + v for k, v in g_got.items()}
        loss.append(c.tr.last_wall_loss[0].clone())
        count.append(c.tr.last_wall_loss[1].clone())
    c.compare(out_sum, d_sum, g_sum, ref, _group("two shards"), "two shards")
    _check_last((torch.cat(loss), torch.cat(count)), wref, "two shards")


def test_both_terms_on(calls):
    c = _case(on=False, use_graph=False)
    c.tr.set_clearance_loss(CDIST, CWEIGHT)
    _step(c, 0)
    torch.cuda.synchronize()
    closs, ccount = (t.clone() for t in c.tr.last_clearance)
    del calls[:]
    c.tr.set_wall_loss(c.walls, DIST, WEIGHT)
    out = _step(c, 0)
    names = _names(calls)
    assert names.index("sw_disc_dpred") < names.index("sw_clearance_grad") < names.index("sw_wall_grad")
    _check_on(c, out, 0, "both terms", also=_col_ref(c, 0)[0])
    assert torch.equal(_bits(c.tr.last_clearance[0]), _bits(closs)) and torch.equal(c.tr.last_clearance[1], ccount), \
        "last_clearance does not see the wall term"
    assert int(ccount.sum()) > 0


# ---- e. the effect ---------------------------------------------------------------------------------------------------------------
def test_training_with_the_term_lowers_the_penalty():
    import socialways_amd as sw
    g = golden("biwi_synth")
    data = sw.SceneDataset(g["obsvs"], g["preds"], g["batches"], g["times"], device=DEV)
    sb = np.asarray(data.train_batches)
    B = int(sb[-1, 1])
    o, p = data.obsv[:B], data.pred[:B]
    lo, hi = p[..., :2].reshape(-1, 2).min(0).values.cpu().numpy(), p[..., :2].reshape(-1, 2).max(0).values.cpu().numpy()
    walls = np.array([[lo[0], lo[1], hi[0], lo[1]], [hi[0], lo[1], hi[0], hi[1]], [hi[0], hi[1], lo[0], hi[1]],
                      [lo[0], hi[1], lo[0], lo[1]]], np.float32)          # the four sides of the box of the true futures
    final = {}
    for weight in (20.0, 0.0):
        torch.manual_seed(11)
        tr = sw.SocialWaysTrainer(12, lr_g=1e-3, use_social=True, device=DEV)
        tr.set_wall_loss(walls, 2.0, weight)
        gen = torch.Generator().manual_seed(12)
        first = None
        for _ in range(300):
            tr.step(o, p, sb, 0.02, 0.97, torch.rand(B, 32, generator=gen), data.ss)
            if first is None:
                first = float(tr.last_wall_loss[0].sum())
        final[weight] = float(tr.last_wall_loss[0].sum())
        print("wall effect  weight %4.1f: penalty sum %.4f at step 1, %.4f at step 300 (%d agents, %d scenes)"
              % (weight, first, final[weight], B, len(sb)))
        assert first > 0, "the training batch has predicted segments closer than 2 m to the box"
    assert final[20.0] < final[0.0]
