"""The scene-clearance term on the GPU: sw_clearance_grad / ops.clearance_grad / stats.clearance_penalty against the float64
reference of tests/_clear_ref.py, its exactness properties bit for bit, and SocialWaysTrainer.step() with
set_clearance_loss() against the float64 step of tests/_step_ref.py plus the float64 gradient of L_col alone.

a. kernel   scene sizes [1, 2, 8, 9, 33, 64, 65, 130] in one batch (312 agents: single agent, pair, below / at / above one
            64-agent tile, three tiles), Tp 1 / 12 / 17 / 25 (no segment without start at Tp 1; one, two time chunks), with and
            without start, pstride and dstride 2 and 4, dpos zero and pre-filled.  Inputs: the random walks of
            _step_ref.make_draws, d0 = 0.5: between 30 % and 63 % of the reference's (pair, segment)s are closer than d0 (both
            shares asserted >= 10 % wherever the path has a segment).  Bound: max|err| <= 2e-5 max|ref| (GRAD_REL of
            tests/_ref64.py) for dpos and for loss; count equal except for agents whose float64 reference has a (b, s) with
            | |c|^2 / d0^2 - 1 | < 1e-5 - at most 1 % of the agents, by the choice of the seed (first of SEEDS that keeps it).
            And one scene of 520 agents (Tp 3): nine tiles where the grid gives a scene eight, so a wave owns two of them.
b. exact    antisymmetry of a two-agent scene, rows that are not touched, two calls, permuted scenes, columns 2 and 3 of a
            4-wide dpos, parallel equal motion (dv = 0).
c. stats    stats.clearance_penalty = the ops call, bit for bit.
d. step     trainers with lr_g = lr_d = 0 on [8, 3, 1, 17] (29 agents), To 8, Tp 12, dist 2 (d0 = dist * ss = 0.5): every
            generator gradient against step64(...).g_run + the float64 gradient of L_col through orc.predict (the loss is a
            sum, so the gradients add), at close_grads_branch_consistent's bound; D's gradients and the loss rows bit-identical
            to the same step without the term; last_clearance against the reference.  Routes: eager, graph (2 eager, capture,
            2 replays), step_many of 3, + L2, "fixed" variety (K = 3), ragged, ragged_fused captured, two scene shards.
e. effect   tests/golden/biwi_synth.npz, its training scenes as one packed batch, 300 steps at lr_g 1e-3: the run with the
            term on (dist 2 m, weight 20) ends with a lower last_clearance[0].sum() than the same run with weight 0.

Observed on an MI355X (pytest -s), largest max|err| / max|ref|: a. dpos 6.6e-6 (Tp 25), loss 5.5e-7, every count away from the threshold equal.
d. generator gradients: eager 5.6e-6, graph 1.66e-5, step_many 1.10e-5, + L2 1.8e-6, "fixed" 2.4e-6, ragged 3.2e-6, ragged_fused
7.4e-6, two shards 7.2e-6; outputs 3.4e-7; no ambiguous unit at the picked seeds.  e. penalty sum 56.39 at step 1, 4.75 (weight 20)
against 412.3 (weight 0) at step 300.  The 47 cases take 7 s together.  """
import numpy as np
import pytest
import torch

import _clear_ref as CR
import _step_ref as S
from _ref64 import SEEDS, RefRun, _close_grad, _report, gen_mods, gen_params, scene_rows  # noqa: F401
from _util import golden
from test_gpu_ragged_train import dev_len
from test_gpu_step_reference import SS, Case, _names, _step, calls, rule_a  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 8, 9, 33, 64, 65, 130]
D0 = 0.5
NEAR = 1e-5
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _scenes(sizes):
    from socialways_amd import ops
    return ops.SceneIndex.get(scene_rows(sizes), int(np.sum(sizes)), torch.device(DEV))


def _widen(x, stride, fill=0.0):
    """(B, T, 2) -> (B, T, stride) with `fill` in the columns behind x and y."""
    if stride == 2:
        return x.clone()
    out = torch.full(x.shape[:2] + (stride,), fill, dtype=x.dtype)
    out[..., :2] = x
    return out


_picked = {}


def _inputs(Tp, with_start, sizes=SIZES):
    """(seed, obsv fp32, pred fp32, reference (loss, count, grad, share, near)): the first seed of SEEDS whose float64
    reference keeps the agents with a (b, s) near the threshold at 1 % or fewer; computed once per shape."""
    key = (Tp, with_start, tuple(sizes))
    if key not in _picked:
        sb, B = scene_rows(sizes), sum(sizes)
        for seed in SEEDS:
            o, p = S.make_draws(sizes, 8, Tp)(seed)[0][:2]
            start = o[:, -1].double() if with_start else None
            share, near = CR.shares(p.double(), start, sb, D0, NEAR)
            if int(near.sum()) <= B // 100:
                break
        else:
            raise AssertionError("no seed of %s keeps the near-threshold agents at 1 %%" % (SEEDS,))
        loss, count = CR.penalty(p.double(), start, sb, D0)
        _picked[key] = (seed, o, p, (loss, count, CR.closed_form_grad(p.double(), start, sb, D0), share, near))
    return _picked[key]


def _call(pos, start, sizes, d0, scale, dpos, with_outputs=True):
    from socialways_amd import ops
    B = pos.shape[0]
    loss = torch.full((B,), float("nan"), device=DEV) if with_outputs else None
    count = torch.full((B,), -1, dtype=torch.int32, device=DEV) if with_outputs else None
    ops.clearance_grad(pos, start, _scenes(sizes), d0, scale, dpos, loss, count)
    torch.cuda.synchronize()
    return loss, count


# ---- a. the kernel against the float64 reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("pstride,dstride", [(2, 2), (2, 4), (4, 2), (4, 4)])
@pytest.mark.parametrize("with_start", [True, False])
@pytest.mark.parametrize("Tp", [1, 12, 17, 25])
def test_kernel_against_float64(Tp, with_start, pstride, dstride):
    seed, o, p, (loss64, count64, g64, share, near) = _inputs(Tp, with_start)
    B, tag = sum(SIZES), "Tp %d, %s start, strides %d / %d, seed %d" % (Tp, "with" if with_start else "no", pstride, dstride, seed)
    if Tp > 1 or with_start:             # a path of one point has no segment: nothing to have a share of
        assert 0.10 <= share <= 0.90, "active share %.3f (%s)" % (share, tag)
    assert int(near.sum()) <= B // 100
    pos = _widen(p, pstride, 7.0).to(DEV)
    start = o.to(DEV)[:, -1] if with_start else None          # a strided view, read in place
    gmax = float(g64.abs().max())
    scale = 2.0 / gmax if gmax > 0 else 1.0                    # scale * g comparable to the unit-variance pre-fill
    gen = torch.Generator().manual_seed(seed)
    for what, pre in (("dpos from zero", torch.zeros(B, Tp, 2)), ("dpos accumulated", torch.randn(B, Tp, 2, generator=gen))):
        dpos = _widen(pre, dstride, 3.0).to(DEV)
        loss, count = _call(pos, start, SIZES, D0, scale, dpos)
        want = pre.double() + scale * g64
        err = float((dpos[..., :2].cpu().double() - want).abs().max()) / max(float(want.abs().max()), 1e-30)
        lerr = float((loss.cpu().double() - loss64).abs().max()) / max(float(loss64.abs().max()), 1e-30)
        print("clearance kernel  %-46s %-16s dpos %.2e  loss %.2e" % (tag, what, err, lerr))
        _close_grad(dpos[..., :2], want, what, "a.kernel", tag)
        _close_grad(loss, loss64, "loss", "a.kernel", tag)
        differs = count.cpu().long() != count64
        assert not bool((differs & ~near).any()), "count differs away from the threshold (%s)" % tag
        if dstride == 4:
            assert bool((dpos[..., 2:] == 3.0).all()), "columns 2 and 3 of dpos (%s)" % tag


def test_scene_above_eight_tiles():
    """520 agents in one scene: nine 64-agent tiles on a grid of eight per scene, so one wave owns tiles 0 and 8."""
    sizes = [520, 3]
    seed, o, p, (loss64, count64, g64, share, near) = _inputs(3, True, sizes)
    B, tag = sum(sizes), "520-agent scene, seed %d" % seed
    assert int(near.sum()) <= B // 100
    dpos = torch.zeros(B, 3, 2, device=DEV)
    loss, count = _call(p.to(DEV), o.to(DEV)[:, -1], sizes, D0, 1.0, dpos)
    _close_grad(dpos, g64, "dpos", "a.kernel", tag)
    _close_grad(loss, loss64, "loss", "a.kernel", tag)
    assert not bool(((count.cpu().long() != count64) & ~near).any()) and bool(dpos[512:520].any()), tag


# ---- b. exactness ---------------------------------------------------------------------------------------------------------------
def test_two_agent_scene_is_antisymmetric_bit_for_bit():
    o, p = S.make_draws([2], 8, 17)(1)[0][:2]
    dpos = torch.zeros(2, 17, 2, device=DEV)
    loss, count = _call(p.to(DEV), o.to(DEV)[:, -1], [2], D0, 0.37, dpos)
    assert int(count[0]) > 0 and bool(dpos.any())
    assert torch.equal(dpos[0], -dpos[1])        # every value the exact negative (-0.0 == 0.0: an untouched point)
    assert torch.equal(_bits(loss[:1]), _bits(loss[1:])) and count[0] == count[1]


def test_rows_with_nothing_closer_than_d0_are_not_touched():
    """A single-agent scene, a scene whose agents are all farther apart than d0, and a scene that does collide: the rows of
    the first two keep their bits - -0.0 and NaN included."""
    sizes = [1, 5, 4]
    o, p = S.make_draws(sizes, 8, 17)(2)[0][:2]
    far = torch.zeros(10, 1, 2)
    far[1:6, 0, 0] = 100.0 * torch.arange(5)
    o, p = o + far, p + far
    pre = torch.randn(10, 17, 4, generator=torch.Generator().manual_seed(4))
    pre[0, 0, 0], pre[2, 3, 1], pre[:, :, 3] = -0.0, float("nan"), float("nan")
    dpos = pre.to(DEV)
    loss, count = _call(p.to(DEV), o.to(DEV)[:, -1], sizes, D0, 1.0, dpos)
    assert torch.equal(_bits(dpos[:6]), _bits(pre[:6].to(DEV))), "rows of agents with every |c| >= d0"
    assert not bool(loss[:6].any()) and not bool(count[:6].any()) and bool((count[6:] > 0).all())
    assert not torch.equal(_bits(dpos[6:, :, :2]), _bits(pre[6:, :, :2].to(DEV)))
    assert torch.equal(_bits(dpos[..., 2:]), _bits(pre[..., 2:].to(DEV))), "columns 2 and 3, NaN included"


def test_two_calls_give_the_same_bits_and_scenes_do_not_see_each_other():
    sizes = [3, 9, 65, 2, 1, 70]
    o, p = S.make_draws(sizes, 8, 17)(3)[0][:2]
    B, sb = sum(sizes), scene_rows(sizes)

    def run(order):
        rows = torch.cat([torch.arange(int(sb[s, 0]), int(sb[s, 1])) for s in order])
        dpos = torch.zeros(B, 17, 4, device=DEV)
        loss, count = _call(_widen(p[rows], 4).to(DEV), o[rows].to(DEV)[:, -1], [sizes[s] for s in order], D0, 0.5, dpos)
        return rows, dpos, loss, count
    rows, d1, l1, c1 = run(range(6))
    _, d2, l2, c2 = run(range(6))
    assert bool(d1.any()) and torch.equal(_bits(d1), _bits(d2)) and torch.equal(_bits(l1), _bits(l2)) and torch.equal(c1, c2)
    d4 = torch.zeros(B, 17, 4, device=DEV)           # loss and count are optional
    _call(_widen(p, 4).to(DEV), o.to(DEV)[:, -1], sizes, D0, 0.5, d4, with_outputs=False)
    assert torch.equal(_bits(d4), _bits(d1))
    rows, d3, l3, c3 = run([4, 2, 0, 5, 3, 1])
    rows = rows.to(DEV)
    assert torch.equal(_bits(d3), _bits(d1[rows])) and torch.equal(_bits(l3), _bits(l1[rows])) and torch.equal(c3, c1[rows])


def test_parallel_equal_motion_takes_tau_zero():
    a = torch.tensor([[0.0, 0.0], [0.5, 0.25], [1.0, 0.5], [1.5, 0.75]])
    P = torch.stack([a, a + torch.tensor([0.25, 0.0]), a + torch.tensor([0.0, 0.375])])
    g64 = CR.closed_form_grad(P.double(), None, [], 0.5)
    loss64, count64 = CR.penalty(P.double(), None, [], 0.5)
    dpos = torch.zeros(3, 4, 2, device=DEV)
    loss, count = _call(P.to(DEV), None, [3], 0.5, 1.0, dpos)
    assert bool(g64[:, 0].any()) and not bool(g64[:, -1].any())
    _close_grad(dpos, g64, "dpos", "b.exact", "dv = 0")
    _close_grad(loss, loss64, "loss", "b.exact", "dv = 0")
    assert torch.equal(count.cpu().long(), count64) and not bool(dpos[:, -1].any())


def test_a_closest_approach_exactly_d0_is_not_an_active_pair():
    """Two agents in step 0.5 apart: |c|^2 = 0.25 = d0^2 exactly at d0 = 0.5, `<` is strict, so count is 0 and the pre-filled
    -0.0 of the dpos rows keeps its bits (a `+= 0` would leave +0.0); at d0 = 0.75 the same pair is active, against float64."""
    a = torch.tensor([[0.0, 0.0], [1.0, 0.0]])
    P = torch.stack([a, a + torch.tensor([0.0, 0.5])])
    loss64, count64 = CR.penalty(P.double(), None, [], 0.5)
    assert not bool(count64.any()) and not bool(loss64.any()) and not bool(CR.closed_form_grad(P.double(), None, [], 0.5).any())
    dpos = torch.full((2, 2, 2), -0.0, device=DEV)
    loss, count = _call(P.to(DEV), None, [2], 0.5, 1.0, dpos)
    assert not bool(count.any()) and not bool(loss.any())
    assert torch.equal(_bits(dpos), _bits(torch.full((2, 2, 2), -0.0, device=DEV))), "a pair that is not active makes no read-modify-write"
    g64 = CR.closed_form_grad(P.double(), None, [], 0.75)
    loss64, count64 = CR.penalty(P.double(), None, [], 0.75)
    assert count64.tolist() == [1, 1] and float(g64.abs().max()) > 1.0
    dpos = torch.zeros(2, 2, 2, device=DEV)
    loss, count = _call(P.to(DEV), None, [2], 0.75, 1.0, dpos)
    _close_grad(dpos, g64, "dpos", "b.exact", "d0 = 0.75")
    _close_grad(loss, loss64, "loss", "b.exact", "d0 = 0.75")
    assert torch.equal(count.cpu().long(), count64)


# ---- c. stats --------------------------------------------------------------------------------------------------------------------
def test_stats_clearance_penalty_is_the_ops_call():
    from socialways_amd import stats
    sizes = [1, 2, 8, 9, 33]
    o, p = S.make_draws(sizes, 8, 12)(1)[0][:2]
    scale, dist = 4.0, 2.0                                       # trajs in quarter units: d0 = dist / scale in theirs
    loss, grad, count = stats.clearance_penalty(p.numpy(), scene_rows(sizes), dist, start=o[:, -1].numpy(), scale=scale, device=DEV)
    dpos = torch.zeros(sum(sizes), 12, 4, device=DEV)
    l2, c2 = _call(_widen(p, 4).to(DEV), o.to(DEV)[:, -1], sizes, dist / scale, 1.0, dpos)
    assert grad.shape == (53, 12, 2) and count.dtype == torch.int32 and bool(grad.any())
    assert torch.equal(_bits(grad), _bits(dpos[..., :2])) and torch.equal(_bits(loss), _bits(l2)) and torch.equal(count, c2)
    l3, g3, c3 = stats.clearance_penalty(p, [], dist, scale=scale, device=DEV)      # one scene, no start
    assert l3.shape == (53,) and g3.shape == (53, 12, 2) and int(c3.sum()) > int(count.sum())


# ---- d. the step ---------------------------------------------------------------------------------------------------------------
SIZES29 = [8, 3, 1, 17]
DIST, WEIGHT = 2.0, 1.5          # d0 = DIST * SS = 0.5


def _col_ref(c, i):
    """Float64: the gradient of L_col alone with respect to every generator parameter (a RefRun), and the per-agent loss,
    count and near-threshold mask of the reference's prediction."""
    o, p, _, _, z, _ = c.draws[i]
    o64, z64 = o.double(), z.double()
    ln = None if c.lens is None else c.lens[i]
    predict = S._forms(c.orc, c.orc.D, o64, p.double(), c.sb, S._len(ln), c.Tp)[0]
    box = {}

    def fn():
        ph = predict(z64)
        box["ph"] = ph.detach()
        return CR.l_col(ph, o64[:, -1], c.sb, DIST * SS, WEIGHT), None
    run, _ = S._run(gen_params(c.orc), gen_mods(c.orc), fn, c.seed, torch.float64)
    loss, count = CR.penalty(box["ph"], o64[:, -1], c.sb, DIST * SS)
    return run, loss, count, CR.shares(box["ph"], o64[:, -1], c.sb, DIST * SS, NEAR)[1]


def _with_col(ref, col):
    """step64's result with g_run = its generator gradient + the gradient of L_col."""
    a, b = ref.g_run.grads(), col.grads()
    assert any(bool(v.any()) for v in b.values()), "the clearance term has a gradient in this case"
    run = RefRun(ref.g_run.params, list(ref.g_run.rec) + list(col.rec), ref.g_run.seed)
    run.grads = lambda: {k: a[k] + b[k] for k in a}
    ref.g_run = run
    return ref


def _group(tag):
    return "d." + tag.split(",")[0]          # one line per route in the module's report (pytest -s)


def _check_last(last, col, tag):
    _, loss64, count64, near = col
    loss, count = last
    assert loss.shape == loss64.shape and count.dtype == torch.int32
    _close_grad(loss, loss64, "last_clearance loss", _group(tag), tag)
    assert not bool(((count.cpu().long() != count64) & ~near).any()), "last_clearance count (%s)" % tag
    assert int(count64.sum()) > 0


def _check_on(c, out, i, tag):
    c.premise()
    d_got, g_got = S.trainer_grads(c.tr)
    col = _col_ref(c, i)
    c.compare(out, d_got, g_got, _with_col(c.ref(i), col[0]), _group(tag), "step %d (%s)" % (i + 1, tag))
    _check_last(c.tr.last_clearance, col, tag)


def _case(f=None, **kw):
    c = Case(SIZES29, 8, 12, f or S.flags(), **kw)
    c.tr.set_clearance_loss(DIST, WEIGHT)
    return c


def test_step_eager_and_the_term_switched_off_and_on(calls):
    c = Case(SIZES29, 8, 12, S.flags(), use_graph=False)
    out0 = _step(c, 0).clone()
    d0, g0 = S.trainer_grads(c.tr)
    assert "sw_clearance_grad" not in _names(calls) and c.tr.last_clearance is None
    assert "sw_dec_rollout_bwd_dfuse" in _names(calls)
    del calls[:]
    c.tr.set_clearance_loss(DIST, WEIGHT)
    out1 = _step(c, 0).clone()
    d1, g1 = S.trainer_grads(c.tr)
    assert _names(calls).count("sw_clearance_grad") == 1 and "sw_dec_rollout_bwd_dfuse" not in _names(calls)
    assert _names(calls).index("sw_disc_dpred") < _names(calls).index("sw_clearance_grad")
    _check_on(c, out1, 0, "eager")
    assert torch.equal(out0, out1), "the loss rows do not see the term"
    assert all(torch.equal(d0[k], d1[k]) for k in d0), "D's gradients do not see the term"
    assert any(not torch.equal(g0[k], g1[k]) for k in g0)
    del calls[:]
    c.tr.set_clearance_loss(None)
    out2 = _step(c, 0)
    d2, g2 = S.trainer_grads(c.tr)
    assert "sw_clearance_grad" not in _names(calls) and c.tr.last_clearance is None
    assert torch.equal(out0, out2) and all(torch.equal(g0[k], g2[k]) for k in g0) and all(torch.equal(d0[k], d2[k]) for k in d0)


def test_step_through_the_graph(calls):
    c = _case(n_steps=5)
    assert c.tr.use_graph
    for i in range(5):
        del calls[:]
        out = _step(c, i)
        assert len(c.tr._graphs) == 1 and [k[-4] for k in c.tr._graphs] == [(DIST, WEIGHT)]
        st = next(iter(c.tr._graphs.values()))
        assert (st["graph"] is not None) == (i >= 2)
        if i >= 3:
            assert not calls, "a replayed step makes no launch of its own"
        elif i < 2:
            assert _names(calls).count("sw_clearance_grad") == 1
        _check_on(c, out, i, "graph")
    c.tr.set_clearance_loss(None)            # another key: the captured graph with the term is not replayed
    _step(c, 0)
    assert len(c.tr._graphs) == 2 and c.tr.last_clearance is None


def test_step_many_of_three():
    c = _case(n_steps=9)
    for r in range(3):
        outs = c.tr.step_many([c.device_draw(i) for i in range(3 * r, 3 * r + 3)], c.sb, SS)
        torch.cuda.synchronize()
        assert [k[5] for k in c.tr._graphs] == [3]
        assert (next(iter(c.tr._graphs.values()))["graph"] is not None) == (r >= 2)
        _check_on(c, outs[2], 3 * r + 2, "step_many, launch %d" % (r + 1))      # p.grad and last_clearance are the last step's


def test_step_with_l2():
    c = _case(S.flags(l2=True))
    _check_on(c, _step(c, 0), 0, "+ L2")


def test_step_with_fixed_variety(calls):
    c = _case(S.flags(variety="fixed", variety_k=3))
    out = _step(c, 0)
    assert "sw_variety_grad" in _names(calls) and "sw_clearance_grad" in _names(calls)
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
    col = _col_ref(c, 0)
    ref = _with_col(c.ref(0), col[0])
    out_sum, d_sum, g_sum, loss, count = 0.0, None, None, [], []
    for lo, hi in ((0, 2), (2, 4)):
        r0, r1 = int(c.sb[lo, 0]), int(c.sb[hi - 1, 1])
        out = c.tr.step(o[r0:r1], p[r0:r1], c.sb[lo:hi] - r0, zv, ov, z[r0:r1], SS, global_B=c.B, global_row0=r0)
        c.premise()
        d_got, g_got = S.trainer_grads(c.tr)
        out_sum = out_sum + out.double()
        d_sum = d_got if d_sum is None else {k: d_sum[k] + v for k, v in d_got.items()}
        g_sum = g_got if g_sum is None else {k: g_sum[k] + v for k, v in g_got.items()}
        loss.append(c.tr.last_clearance[0].clone())
        count.append(c.tr.last_clearance[1].clone())
    c.compare(out_sum, d_sum, g_sum, ref, _group("two shards"), "two shards")
    _check_last((torch.cat(loss), torch.cat(count)), col, "two shards")


# ---- e. the effect ---------------------------------------------------------------------------------------------------------------
def test_training_with_the_term_lowers_the_penalty():
    import socialways_amd as sw
    g = golden("biwi_synth")
    data = sw.SceneDataset(g["obsvs"], g["preds"], g["batches"], g["times"], device=DEV)
    sb = np.asarray(data.train_batches)
    B = int(sb[-1, 1])
    o, p = data.obsv[:B], data.pred[:B]
    final = {}
    for weight in (20.0, 0.0):
        torch.manual_seed(11)
        tr = sw.SocialWaysTrainer(12, lr_g=1e-3, use_social=True, device=DEV)
        tr.set_clearance_loss(2.0, weight)
        gen = torch.Generator().manual_seed(12)
        first = None
        for _ in range(300):
            tr.step(o, p, sb, 0.02, 0.97, torch.rand(B, 32, generator=gen), data.ss)
            if first is None:
                first = float(tr.last_clearance[0].sum())
        final[weight] = float(tr.last_clearance[0].sum())
        print("clearance effect  weight %4.1f: penalty sum %.4f at step 1, %.4f at step 300 (%d agents, %d scenes)"
              % (weight, first, final[weight], B, len(sb)))
        assert first > 0, "the training batch has pairs closer than 2 m"
    assert final[20.0] < final[0.0]
