"""Host side of the composed scene futures (no GPU): sw_scene_compose is declared and bound, rejects bad arguments before the
device is touched, ops.scene_compose names the shapes it expects, the public calls exist on every trainer and in stats - and
the constructed cases of tests/test_gpu_compose.py are shown, by the float64 reference alone, to stay clear of coll_dist and
to reach every regime of the selection loop."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _compose_ref as R
from test_sample_host import declared_arguments

EARG, ESHAPE = -1, -2


def test_header_and_binding_agree_on_the_compose_entry_point():
    from socialways_amd import _lib as L
    lib = L.load()
    assert "sw_scene_compose" in L.PROTOTYPES
    res, args = L.PROTOTYPES["sw_scene_compose"]
    assert declared_arguments("sw_scene_compose") == len(args) == 21
    assert res is L._i and args[-1] is L._vp               # status int, void* stream last
    assert args[11] is L._f and args[12] is L._f and args[13] is L._i      # inv_ss, coll_dist, sweeps
    assert hasattr(lib, "sw_scene_compose")


def test_argument_validation_without_gpu():
    """Every SW_EARG / SW_ESHAPE condition, with B = 0 and with B > 0; `p` is a non-NULL, 8-byte aligned address nobody
    dereferences: each call returns from its argument checks (B == 0 or S == 0: SW_OK without a launch)."""
    from socialways_amd import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(128)
    p = (ctypes.addressof(buf) + 15) & ~15

    def cmp(pos=p, pstride=4, start=p, sstride=16, score=p, scene_off=p, len=p, S=0, B=0, K=20, Tp=12, inv_ss=1.0, coll=0.5,
            sweeps=8, err=p, sel=p, sel0=p, clear=p, per_scene=p, per_row=p):
        return lib.sw_scene_compose(pos, pstride, start, sstride, score, scene_off, len, S, B, K, Tp, inv_ss, coll, sweeps, err,
                                    sel, sel0, clear, per_scene, per_row, None)
    assert cmp() == 0 and cmp(err=None, per_row=None) == 0 and cmp(per_row=None) == 0 and cmp(sel0=None, len=None) == 0
    assert cmp(start=None, sstride=0) == 0 and cmp(pstride=2, coll=0.0, sweeps=1, K=1, Tp=1) == 0 and cmp(K=4096) == 0
    assert cmp(B=7, S=0) == 0 and cmp(B=0, S=3) == 0 and cmp(sstride=2) == 0
    bad = (dict(pos=None), dict(score=None), dict(scene_off=None), dict(sel=None), dict(clear=None), dict(per_scene=None),
           dict(S=-1), dict(B=-1), dict(K=0), dict(K=-2), dict(Tp=0), dict(sweeps=0), dict(sweeps=-1), dict(pstride=3),
           dict(pstride=1), dict(pstride=0), dict(pos=p + 4), dict(err=p + 4), dict(sstride=1), dict(sstride=0),
           dict(inv_ss=0.0), dict(inv_ss=-1.0), dict(inv_ss=float("nan")), dict(coll=-1e-3), dict(coll=float("nan")),
           dict(err=None))
    for kw in bad:
        assert cmp(**kw) == EARG, kw
        if "B" not in kw and "S" not in kw:
            assert cmp(B=7, S=2, **kw) == EARG, kw
    assert cmp(S=-1, B=7) == EARG and cmp(B=-1, S=2) == EARG
    assert cmp(K=4097) == ESHAPE and cmp(B=7, S=2, K=4097) == ESHAPE
    assert cmp(K=4097, sweeps=0) == EARG                   # the argument checks come first


def test_ops_wrapper_names_the_expected_shape():
    from socialways_amd import ops, SocialWaysHipError
    K, B, Tp = 20, 7, 12
    pos, score, start = torch.zeros(K, B, Tp, 4), torch.zeros(K, B), torch.zeros(B, 2)
    err, lens = torch.zeros(K, B, 2), torch.ones(B, dtype=torch.int32)
    scenes = types.SimpleNamespace(B=B, S=2, scene_off=None)
    for kw in (dict(score=score[0]), dict(K=19), dict(pos=pos[:, :6]), dict(pos=pos[..., :3]),
               dict(pos=pos.view(K * B, Tp, 4)[:-1]), dict(pos=torch.zeros(B, K, Tp, 4)), dict(pos=pos[0]),
               dict(start=start[:6]), dict(start=start[:, :1]), dict(start=start[0]), dict(err=err[:, :6]), dict(err=err[..., :1]),
               dict(lens=lens[:6]), dict(lens=lens.long()), dict(lens=[1] * B), dict(coll_dist=-0.1), dict(coll_dist=float("nan")),
               dict(inv_ss=0.0), dict(sweeps=0), dict(scenes=types.SimpleNamespace(B=6, S=2, scene_off=None)),
               dict(score=torch.zeros(5000, B), K=5000)):
        a = dict(pos=pos, start=start, score=score, scenes=scenes, K=K, coll_dist=0.5, inv_ss=1.0, sweeps=8, lens=lens, err=err)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.scene_compose(**a)
    with pytest.raises(ValueError, match=r"\(K \* B, Tp, 2 or 4\)"):
        ops.scene_compose(pos[:, :6], start, score, scenes, K, 0.5)
    with pytest.raises(ValueError, match=r"\(K, B, 2\) = \(20, 7, 2\)"):
        ops.scene_compose(pos, start, score, scenes, K, 0.5, err=err[:, :6])
    with pytest.raises(ValueError, match=r"start must be \(B, >= 2\) = \(7, >= 2\)"):
        ops.scene_compose(pos, start[:6], score, scenes, K, 0.5)
    with pytest.raises(ValueError, match=r"lens must be an int32 tensor \(B,\) = \(7,\)"):
        ops.scene_compose(pos, start, score, scenes, K, 0.5, lens=lens[:6])
    with pytest.raises(ValueError, match=r"scenes index 6 rows, score has B = 7"):
        ops.scene_compose(pos, start, score, types.SimpleNamespace(B=6, S=2, scene_off=None), K, 0.5)
    for good in (pos, pos.view(K * B, Tp, 4), pos[..., :2].contiguous()):      # well-formed, but not on the GPU: no CPU fallback
        with pytest.raises(SocialWaysHipError):
            ops.scene_compose(good, start, score, scenes, K, 0.5, lens=lens, err=err)


def test_public_surface():
    import socialways_amd as sw
    from socialways_amd import generic, wide
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        assert callable(getattr(cls, "sample_composed")) and callable(getattr(cls, "evaluate_composed"))
    assert callable(sw.stats.compose_scenes)
    with pytest.raises(sw.SocialWaysHipError):             # no CPU fallback
        sw.stats.compose_scenes(np.zeros((4, 3, 2, 2)), np.zeros((4, 3)), [], 0.5, device="cpu")
    with pytest.raises(ValueError):
        sw.stats.compose_scenes(np.zeros((4, 3, 2, 2)), np.zeros((4, 2)), [], 0.5, device="cpu")
    with pytest.raises(ValueError):
        sw.stats.compose_scenes(np.zeros((4, 3, 2, 2)), np.zeros((4, 3)), [], 0.5, start=np.zeros((2, 2)), device="cpu")


@pytest.mark.parametrize("kw", [dict(coll_dist=-1.0), dict(coll_dist=float("nan")), dict(sweeps=0)])
def test_bad_thresholds_are_refused_before_anything_is_sampled(kw):
    import socialways_amd as sw
    from socialways_amd import generic, wide
    me = types.SimpleNamespace(_device_noise=lambda noise: None, device="cpu", _check_compose=sw.SocialWaysTrainer._check_compose)
    data = types.SimpleNamespace(ss=1.0)
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        a = dict(coll_dist=0.5, sweeps=8)
        a.update(kw)
        with pytest.raises(ValueError):
            cls.sample_composed(me, torch.zeros(3, 8, 2), 6, **a)
        with pytest.raises(ValueError):
            cls.evaluate_composed(me, data, n_gen_samples=6, **a)


# ---- the constructed cases, by the reference alone -------------------------------------------------------------------------
COLL = 0.5
HAND = {
    # agents 1, 2, 3 share lane 1; agent 1 can only leave towards agent 0's lane: that move sends agent 0 away a sweep later
    "second_sweep": dict(lanes=[[0, 3], [1, 0], [1, 2], [1, 1]], order=[[0, 1]] * 4),
    "one_sweep": dict(lanes=[[0, 1], [0, 2], [5, 5]], order=[[0, 1]] * 3),
    "free": dict(lanes=[[0, 0], [1, 0], [2, 0]], order=[[0, 1]] * 3),
    "stuck": dict(lanes=[[0, 0, 0], [0, 0, 0], [4, 0, 4]], order=[[0, 1, 2]] * 3),
}


def host_cases():
    """(name, case, sweeps): small enough for the full table of cross clearances."""
    out = [(name, R.hand_case(**kw), 8) for name, kw in HAND.items()]
    out.append(("second_sweep_cut", R.hand_case(**HAND["second_sweep"]), 1))
    out.append(("swap", R.swap_case(), 8))
    out.append(("lanes_cont", R.lane_case([1, 2, 7, 5], 6, 12, seed=1, spread=5), 8))
    out.append(("lanes_quant", R.lane_case([7, 3, 9], 5, 4, seed=2, spread=6, scores="quant", inv_ss=2.0), 8))
    out.append(("lanes_start", R.lane_case([2, 7, 4], 6, 5, seed=3, stride=2, spread=5, with_start=True, pstride=4, scores="quant"), 8))
    out.append(("lanes_ragged", R.lane_case([6, 1, 8], 4, 17, seed=4, spread=5, ragged=True, inv_ss=0.5), 8))
    out.append(("lanes_ragged_start", R.lane_case([5, 7], 5, 12, seed=5, stride=1, spread=4, with_start=True, ragged=True), 8))
    out.append(("dense", R.lane_case([12], 4, 3, seed=6, spread=6), 8))
    out.append(("dense_cut", R.lane_case([12], 4, 3, seed=6, spread=6), 1))
    return out


def run_ref(case, sweeps, coll=COLL):
    return R.compose_reference(case["pos"], case["start"], case["score"], case["sizes"], coll, case["inv_ss"], sweeps,
                               case["lens"], case["err"])


def test_constructed_cases_stay_clear_of_the_threshold():
    for name, case, _ in host_cases():
        c = R.cross_clearances(case["pos"], case["start"], case["sizes"], case["inv_ss"], case["lens"])
        assert len(c) > 0, name
        assert ((c < 0.4) | (c > 0.6)).all(), (name, c[(c >= 0.4) & (c <= 0.6)][:5])
        if name.startswith("lanes"):
            assert (c < 0.4).any() and (c > 0.6).any(), name


def test_the_reference_reaches_every_regime():
    seen = set()
    for name, case, sweeps in host_cases():
        r = run_ref(case, sweeps)
        full = run_ref(case, 64) if sweeps < 64 else r
        o = 0
        for s, n in enumerate(case["sizes"]):
            p0, p1, moved, swept = r["per_scene"][s]
            assert p1 <= p0 and swept <= sweeps and (swept > 0 or moved == 0)
            cut = not np.array_equal(r["sel"][o:o + n], full["sel"][o:o + n])
            if n > 1 and p0 == 0:
                seen.add("free")
            if p0 > 0 and p1 == 0 and swept == 1:
                seen.add("one_sweep")
            if p0 > 0 and p1 == 0 and swept >= 2:
                seen.add("later_sweep")
            if p1 > 0 and not cut and r["stuck"][s]:
                seen.add("stuck")
            if cut and sweeps == 1:
                seen.add("cut_short")
            if r["kept"][s]:
                seen.add("kept")
            o += n
    assert seen == {"free", "one_sweep", "later_sweep", "stuck", "cut_short", "kept"}, seen


def test_hand_built_cases_have_the_outcome_worked_out_by_hand():
    r = run_ref(R.hand_case(**HAND["second_sweep"]), 8)
    assert r["sel0"].tolist() == [0, 0, 0, 0] and r["sel"].tolist() == [1, 1, 1, 0] and r["per_scene"].tolist() == [[3, 0, 3, 2]]
    r = run_ref(R.hand_case(**HAND["second_sweep"]), 1)
    assert r["sel"].tolist() == [0, 1, 1, 0] and r["per_scene"].tolist() == [[3, 1, 2, 1]]
    r = run_ref(R.hand_case(**HAND["stuck"]), 8)
    assert r["sel"].tolist() == [0, 0, 0] and r["per_scene"].tolist() == [[1, 1, 0, 0]] and r["kept"][0] and r["stuck"][0]
    assert np.isinf(r["clear"][2]) or r["clear"][2] > 0.6
    # two agents swap places inside the one segment: distance 2 at both frames, clearance 0 between them; agent 0's other draw
    # is the same path (no fewer conflicts: it stays), agent 1's passes three units away
    case = R.swap_case()
    c = R.cross_clearances(case["pos"], None, [2])
    assert sorted(c.tolist()) == [0.0, 0.0, 3.0, 3.0]
    r = run_ref(case, 8)
    assert r["sel0"].tolist() == [0, 0] and r["sel"].tolist() == [0, 1] and r["per_scene"].tolist() == [[1, 0, 1, 1]]
    assert r["clear"].tolist() == [3.0, 3.0] and r["kept"][0]
    assert run_ref(case, 8, coll=0.0)["sel"].tolist() == [0, 0]        # coll_dist = 0 admits no conflict


def test_single_frame_without_start_has_no_segment():
    case = R.lane_case([3, 2], 4, 1, seed=7, spread=1)
    r = run_ref(case, 8)
    assert np.isinf(r["clear"]).all() and np.array_equal(r["sel"], r["sel0"]) and not r["per_scene"].any()
