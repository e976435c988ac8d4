"""Plan risk without a GPU: the float64 reference (tests/_risk_ref.py) on cases worked out by hand, the empty gap around
coll_dist of every constructed case the GPU tests use, sw_plan_risk's argument checks through the C ABI (they return before
the device is touched), and the argument errors of the Python layers."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _risk_ref as R
from _compose_ref import swap_case


def ref(pos, plans, sizes, coll=0.5, start=None, plan_start=None, q_scene=None, q_ego=None, **kw):
    plans = np.asarray(plans, np.float32)
    q_scene = np.arange(plans.shape[0]) if q_scene is None else q_scene
    return R.risk_reference(np.asarray(pos, np.float32), start, sizes, plans, plan_start, q_scene, q_ego, coll, **kw)


# ---- the reference on cases worked out by hand -----------------------------------------------------------------------------
def test_a_plan_that_swaps_places_inside_a_segment_has_clearance_zero():
    case = swap_case()                                           # agent 0: (0,0) -> (2,0); agent 1 draw 0 the reverse, draw 1 3 away
    plan = case["pos"][0, 0][None, None]                         # the plan walks agent 0's path: (1, 1, 2, 2)
    r = ref(case["pos"][:, 1:2], plan, [1])
    assert r["clear_min"].tolist() == [[0.0]] and r["counts"].tolist() == [[[1, 1, 0, 1]]]      # draw 0 conflicts, in the segment ending at frame 1
    assert r["risk"].tolist() == [[0.5]]
    # three frames, the swap in the second segment: the first conflict ends at frame 2
    pos = np.zeros((1, 1, 3, 2), np.float32)
    pos[0, 0] = [[9, 9], [2, 0], [0, 0]]
    r = ref(pos, [[[[0, 0], [0, 0], [2, 0]]]], [1])
    assert r["clear_min"].tolist() == [[0.0]] and r["counts"].tolist() == [[[1, 2, 0, 1]]] and r["risk"].tolist() == [[1.0]]
    # with a start point the first segment ends at frame 0
    r = ref(pos, [[[[0, 0], [0, 0], [2, 0]]]], [1], start=np.array([[1, 0]], np.float32), plan_start=np.array([[9, 9]], np.float32))
    assert r["counts"][0, 0, 1] == 0


def test_the_ego_row_is_left_out_and_rows_outside_the_scene_leave_nobody_out():
    pos = np.zeros((2, 3, 2, 2), np.float32)
    pos[:, 0, :, 1] = 0.0                                        # row 0 on the plan's line in both draws
    pos[:, 1, :, 1] = 5.0
    pos[0, 2, :, 1] = 0.1                                        # row 2 close in draw 0 only
    pos[1, 2, :, 1] = 7.0
    plan = np.zeros((1, 1, 2, 2), np.float32)
    plans = np.repeat(plan, 4, 0)
    r = ref(pos, plans, [3], q_scene=[0, 0, 0, 0], q_ego=[-1, 0, 2, 17])
    assert r["risk"][:, 0].tolist() == [1.0, 0.5, 1.0, 1.0]
    assert r["counts"][:, 0].tolist() == [[2, 1, 0, 2], [1, 1, 2, 1], [2, 1, 0, 2], [2, 1, 0, 2]]
    assert r["n_other"].tolist() == [3, 2, 2, 3]
    # a scene index outside 0 .. S-1: nothing is read
    r = ref(pos, plan, [3], q_scene=[4])
    assert r["risk"].tolist() == [[0.0]] and np.isinf(r["clear_min"]).all() and r["counts"].tolist() == [[[0, -1, -1, 0]]]
    # the only agent is the ego: no other agent
    r = ref(pos[:, :1], plan, [1], q_ego=[0])
    assert r["risk"].tolist() == [[0.0]] and np.isinf(r["clear_min"]).all() and r["counts"].tolist() == [[[0, -1, -1, 0]]]


def test_lengths_gate_segments_and_nan_padding_reaches_nothing():
    pos = np.zeros((1, 2, 4, 2), np.float32)
    pos[0, 0, :, 0] = [0, 1, 2, 3]
    pos[0, 0, :, 1] = [3, 3, 0, 0]                               # agent 0 reaches the plan's line at frame 2
    pos[0, 1] = np.nan
    pos[0, 1, 0] = [50, 50]                                      # agent 1: one frame, then padding
    plan = np.zeros((1, 1, 4, 2), np.float32)
    plan[0, 0, :, 0] = [0, 1, 2, 3]
    full = ref(pos, plan, [2], lens=[4, 1])
    assert full["counts"].tolist() == [[[1, 2, 0, 1]]] and full["clear_min"].tolist() == [[0.0]] and full["risk"].tolist() == [[1.0]]
    cut = ref(pos, plan, [2], lens=[2, 1])                       # agent 0 gone before it comes close: the segment ending at frame 2 does not count
    assert cut["counts"].tolist() == [[[0, -1, -1, 0]]] and cut["clear_min"].tolist() == [[3.0]] and cut["risk"].tolist() == [[0.0]]
    pcut = ref(pos, plan, [2], lens=[4, 1], plan_lens=[2])       # the same through the plan's length
    assert pcut["counts"].tolist() == [[[0, -1, -1, 0]]] and pcut["clear_min"].tolist() == [[3.0]]
    plan_nan = plan.copy()
    plan_nan[0, 0, 2:] = np.nan
    again = ref(pos, plan_nan, [2], lens=[4, 1], plan_lens=[2])
    assert again["counts"].tolist() == [[[0, -1, -1, 0]]] and again["clear_min"].tolist() == [[3.0]] and again["risk"].tolist() == [[0.0]]
    clamp = ref(pos, plan, [2], lens=[99, -5], plan_lens=[0])    # clamped into 1 .. Tp: the plan has one frame, no segment without a start
    assert np.isinf(clamp["clear_min"]).all() and clamp["risk"].tolist() == [[0.0]]


def test_the_product_formula_exact_zero_and_one_and_the_tie_rule():
    K = 4
    pos = np.zeros((K, 3, 2, 2), np.float32)
    pos[..., 1] = 9.0                                            # everybody far from the plan's line y = 0 ...
    pos[:1, 0, :, 1] = 0.0                                       # ... but draw 0 of row 0,
    pos[1:3, 1, :, 1] = 0.0                                      # draws 1, 2 of row 1
    pos[2:4, 2, :, 1] = 0.0                                      # and draws 2, 3 of row 2
    plan = np.zeros((1, 1, 2, 2), np.float32)
    r = ref(pos, plan, [3])
    assert r["risk"][0, 0] == 1.0 - 0.75 * 0.5 * 0.5             # all 4^3 tuples, where the diagonal sees 4 / 4
    assert r["counts"].tolist() == [[[4, 1, 1, 2]]]              # rows 1 and 2 tie at h = 2: the lowest row
    far = np.full((1, 1, 2, 2), 100.0, np.float32)
    r = ref(pos, far, [3])
    assert r["risk"].tolist() == [[0.0]] and r["counts"].tolist() == [[[0, -1, -1, 0]]]
    pos[:, 2, :, 1] = 0.0                                        # every draw of row 2 conflicts
    r = ref(pos, plan, [3])
    assert r["risk"].tolist() == [[1.0]] and r["counts"].tolist() == [[[4, 1, 2, 4]]]
    assert R.risk_bound(3) == 8 * 2.0 ** -24


# ---- the constructed cases: nothing within 0.1 of coll_dist, every regime present ------------------------------------------
def test_constructed_cases_stay_clear_of_the_threshold_and_reach_every_regime():
    seen = set()
    for name, case in R.constructed_cases():
        r = R.run_reference(case)
        c = r["c"]
        assert ((c < 0.4) | (c > 0.6)).all(), (name, c[(c >= 0.4) & (c <= 0.6)][:5])          # over every tuple, none left out
        if case["Tp"] == 1 and case["start"] is None:
            assert len(c) == 0 and not r["risk"].any() and (r["counts"][..., 1] == -1).all(), name
            seen.add("no_segment")
            continue
        assert len(c) > 0, name
        some = r["n_other"][:, None] > 0
        inner = (r["hsum"] > 0) & (r["hmax"] < case["K"])
        assert ((r["risk"] > 0) & (r["risk"] < 1))[inner].all() and (r["risk"][r["hmax"] == case["K"]] == 1).all()
        assert (r["risk"][r["hsum"] == 0] == 0).all()
        seen |= {"inner"} if inner.any() else set()
        seen |= {"one"} if (some & (r["hmax"] == case["K"])).any() else set()
        seen |= {"zero"} if (some & (r["hsum"] == 0)).any() else set()
        if name == "all_hit":
            assert (r["risk"] == 1).all()
        if name == "all_clear":
            assert (r["risk"] == 0).all() and np.isfinite(r["clear_min"]).all()
        if name.startswith("sizes"):
            assert inner.mean() >= 0.5, (name, inner.mean())
    assert seen == {"no_segment", "inner", "one", "zero"}, seen


# ---- sw_plan_risk refuses bad arguments before the device is touched -------------------------------------------------------
def test_argument_validation_without_gpu():
    from socialways_amd import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15                       # host memory, 16-byte aligned: never dereferenced
    good = dict(pos=p, pstride=2, start=p, sstride=2, scene_off=p, len=None, S=1, B=2, K=4, Tp=3, plans=p, plan_start=p,
                plan_len=None, q_scene=p, q_ego=None, Q=1, P=2, inv_ss=1.0, coll=0.5, risk=p, clear_min=p, counts=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sw_plan_risk(*[a[k] for k in good])

    assert call(Q=0) == 0                                        # SW_OK without a launch
    assert call(Q=0, start=None, plan_start=None) == 0
    for name in ("pos", "scene_off", "plans", "q_scene", "risk", "clear_min", "counts"):
        assert call(**{name: None}) == -1, name
    assert call(plan_start=None) == -1 and call(start=None) == -1
    for kw in (dict(S=-1), dict(B=-1), dict(Q=-1), dict(K=0), dict(Tp=0), dict(P=0), dict(pstride=3), dict(pstride=1),
               dict(pos=p + 4), dict(plans=p + 4), dict(sstride=1), dict(inv_ss=0.0), dict(inv_ss=-1.0), dict(inv_ss=float("nan")),
               dict(coll=-0.5), dict(coll=float("nan"))):
        assert call(**kw) == -1, kw
        assert "Q" in kw or call(**dict(kw, Q=0)) == -1, kw      # the checks come before the early return
    assert call(K=4097) == -2 and call(K=4097, Q=0) == -2        # SW_ESHAPE
    assert call(sstride=1, start=None, plan_start=None, Q=0) == 0      # sstride is read only with a start


# ---- the Python layers: errors before any launch, no CPU fallback ----------------------------------------------------------
def test_ops_and_stats_refuse_bad_arguments_and_cpu_tensors():
    import socialways_amd as sw
    from socialways_amd import ops
    K, B, Tp, Q, P = 3, 4, 5, 2, 2
    scenes = ops.SceneIndex.get([[0, 2], [2, 4]], B, "cpu")
    pos, plans = torch.zeros(K, B, Tp, 2), torch.zeros(Q, P, Tp, 2)
    start, pstart = torch.zeros(B, 2), torch.zeros(Q, 2)
    qs = torch.tensor([0, 1], dtype=torch.int32)
    a = dict(pos=pos, start=start, scenes=scenes, K=K, plans=plans, plan_start=pstart, q_scene=qs, q_ego=None, coll_dist=0.5)
    for kw in (dict(coll_dist=-1.0), dict(coll_dist=float("nan")), dict(inv_ss=0.0), dict(plans=torch.zeros(Q, P, Tp + 1, 2)),
               dict(plans=torch.zeros(Q, P, Tp, 3)), dict(plans=torch.zeros(Q, 0, Tp, 2)), dict(plans=plans.double()),
               dict(plan_start=None), dict(start=None), dict(plan_start=torch.zeros(Q + 1, 2)), dict(q_scene=qs.long()),
               dict(q_scene=qs[:1]), dict(q_ego=torch.zeros(Q)), dict(lens=torch.zeros(B)), dict(plan_lens=torch.zeros(Q + 1, dtype=torch.int32)),
               dict(pos=torch.zeros(K, B + 1, Tp, 2)), dict(plans=plans[0], q_scene=qs)):
        with pytest.raises(ValueError):
            ops.plan_risk(**dict(a, **kw))
    with pytest.raises(sw.SocialWaysHipError):                  # checked arguments on the CPU: refused, never computed on the host
        ops.plan_risk(**a)
    with pytest.raises(sw.SocialWaysHipError):
        ops.plan_risk(**dict(a, plans=plans[0], plan_start=pstart[:1], q_scene=qs[:1]))      # (P, Tp, 2): Q = 1

    s = dict(trajs=np.zeros((K, B, Tp, 2)), sub_batches=[[0, 2], [2, 4]], plans=np.zeros((Q, P, Tp, 2)), coll_dist=0.5, device="cpu")
    for kw in (dict(coll_dist=-1.0), dict(plans=np.zeros((3, P, Tp, 2))), dict(scene=[0, 1, 1]), dict(scene=[0.5, 1.0]),
               dict(ego=[0]), dict(start=np.zeros((B, 2))), dict(plan_start=np.zeros((Q, 2))), dict(lens=[1, 2, 3, 9]),
               dict(plan_lens=[0, 1]), dict(trajs=np.zeros((B, Tp, 2))), dict(scale=0.0)):
        with pytest.raises(ValueError):
            sw.stats.plan_risk(**dict(s, **kw))
    with pytest.raises(sw.SocialWaysHipError):
        sw.stats.plan_risk(**s)
    with pytest.raises(sw.SocialWaysHipError):
        sw.stats.plan_risk(**dict(s, plans=np.zeros((3, P, Tp, 2)), scene=[0, 1, 1], ego=[-1, 2, 0], start=np.zeros((B, 2)),
                                  plan_start=np.zeros((3, 2)), lens=[1, 2, 3, 5], plan_lens=[5, 1, 2]))


def test_the_trainers_refuse_bad_arguments_before_anything_is_sampled():
    import socialways_amd as sw
    from socialways_amd import generic, wide
    me = types.SimpleNamespace(_device_noise=lambda noise: None, device="cpu", n_next=5)      # no generator: sampling would raise AttributeError
    data = types.SimpleNamespace(ss=1.0)
    obsv, plans = torch.zeros(4, 8, 2), torch.zeros(2, 3, 5, 2)
    sb = [[0, 2], [2, 4]]
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        good = dict(obsv_p=obsv, plans=plans, n_samples=6, coll_dist=0.5, sub_batches=sb, ego=[0, 3])
        for kw in (dict(coll_dist=-1.0), dict(coll_dist=float("nan")), dict(n_samples=0), dict(scale=0.0), dict(plans=torch.zeros(2, 3, 4, 2)),
                   dict(plans=torch.zeros(3, 3, 5, 2)), dict(ego=None), dict(ego=[0, 4]), dict(ego=[0]), dict(plan_start=torch.zeros(2, 2)),
                   dict(ego=None, plan_start=torch.zeros(3, 2)), dict(scene=[0, 2]), dict(scene=[0, 1, 1]), dict(sub_batches=[])):
            with pytest.raises(ValueError):
                cls.plan_risk(me, **dict(good, **kw))
        with pytest.raises(sw.SocialWaysHipError):              # CPU observations: refused before the generator is touched
            cls.plan_risk(me, **good)
        with pytest.raises(sw.SocialWaysHipError):
            cls.plan_risk(me, **dict(good, ego=None, plan_start=torch.zeros(2, 2), scene=[1, 1]))
        for bad in (-1.0, float("nan")):
            with pytest.raises(ValueError):
                cls.evaluate_risk(me, data, n_gen_samples=6, coll_dist=bad)
