"""Host side of the diverse top-M selection (no GPU): sw_sample_nms is declared and bound, rejects bad arguments before the
device is touched, ops.sample_nms names the shape it expects, and the public calls exist on every trainer and in stats."""
import ctypes
import types

import numpy as np
import pytest
import torch

from test_sample_host import declared_arguments

EARG, ESHAPE = -1, -2


def test_header_and_binding_agree_on_the_selection_entry_point():
    from socialways_amd import _lib as L
    lib = L.load()
    assert "sw_sample_nms" in L.PROTOTYPES
    res, args = L.PROTOTYPES["sw_sample_nms"]
    assert declared_arguments("sw_sample_nms") == len(args) == 20
    assert res is L._i and args[-1] is L._vp               # status int, void* stream last
    assert args[10] is L._f and args[11] is L._f           # inv_ss, radius
    assert hasattr(lib, "sw_sample_nms")


def test_argument_validation_without_gpu():
    """Every SW_EARG / SW_ESHAPE condition, with B = 0 and with B > 0; `p` is a non-NULL, 8-byte aligned address nobody
    dereferences: each call returns from its argument checks (B == 0: SW_OK without a launch)."""
    from socialways_amd import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(128)
    p = (ctypes.addressof(buf) + 15) & ~15

    def nms(pos=p, pstride=4, score=p, scene_off=None, S=0, B=0, K=20, Tp=12, M=5, metric=0, inv_ss=1.0, radius=0.5, err=p,
            best=p, order=p, count=p, weight=p, assign=p, per_row=p):
        return lib.sw_sample_nms(pos, pstride, score, scene_off, S, B, K, Tp, M, metric, inv_ss, radius, err, best, order, count,
                                 weight, assign, per_row, None)
    assert nms() == 0 and nms(err=None, best=None, per_row=None) == 0 and nms(best=None) == 0 and nms(per_row=None) == 0
    assert nms(pstride=2, metric=1, M=20, radius=0.0) == 0 and nms(K=1, M=1, Tp=1) == 0 and nms(K=4096, M=4096) == 0
    assert nms(scene_off=p, S=0) == 0 and nms(scene_off=p, S=3) == 0 and nms(S=-1) == 0      # S is unused without scene_off
    bad = (dict(pos=None), dict(score=None), dict(order=None), dict(count=None), dict(weight=None), dict(assign=None),
           dict(B=-1), dict(K=0), dict(K=-2), dict(M=0), dict(M=-1), dict(M=21), dict(Tp=0), dict(pstride=3), dict(pstride=1),
           dict(pstride=0), dict(metric=2), dict(metric=-1), dict(radius=-1e-3), dict(radius=float("nan")), dict(inv_ss=0.0),
           dict(inv_ss=-1.0), dict(inv_ss=float("nan")), dict(err=None), dict(err=None, best=None), dict(scene_off=p, S=-1),
           dict(pos=p + 4), dict(err=p + 4))
    for kw in bad:
        assert nms(**kw) == EARG, kw
        if "B" not in kw:
            assert nms(B=7, **kw) == EARG, kw
            assert nms(B=7, scene_off=kw.get("scene_off", p), S=kw.get("S", 2), **{k: v for k, v in kw.items()
                                                                                  if k not in ("scene_off", "S")}) == EARG, kw
    assert nms(K=4097) == ESHAPE and nms(B=7, K=4097) == ESHAPE and nms(B=7, K=4097, M=4097) == ESHAPE
    assert nms(K=4097, M=4098) == EARG                     # the argument checks come first


def test_ops_wrapper_names_the_expected_shape():
    from socialways_amd import ops, SocialWaysHipError
    K, B, Tp = 20, 7, 12
    pos, score = torch.zeros(K, B, Tp, 4), torch.zeros(K, B)
    err, best = torch.zeros(K, B, 2), torch.zeros(B, dtype=torch.int32)
    scenes = types.SimpleNamespace(B=6, S=2, scene_off=None)
    for kw in (dict(score=score[0]), dict(K=19), dict(M=0), dict(M=21), dict(pos=pos[:, :6]), dict(pos=pos[..., :3]),
               dict(pos=pos.view(K * B, Tp, 4)[:-1]), dict(pos=torch.zeros(B, K, Tp, 4)), dict(pos=pos[0]),
               dict(err=err[:, :6]), dict(err=err[..., :1]), dict(best=best[:6]), dict(best=best.long()),
               dict(err=None), dict(metric="mse"), dict(radius=-0.1), dict(radius=float("nan")), dict(inv_ss=0.0),
               dict(scenes=scenes), dict(score=torch.zeros(5000, 2), K=5000, M=5)):
        a = dict(pos=pos, score=score, K=K, M=5, radius=0.5, metric="fde", scenes=None, inv_ss=1.0, err=err, best=best)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.sample_nms(a["pos"], a["score"], a["K"], a["M"], a["radius"], a["metric"], a["scenes"], a["inv_ss"], a["err"],
                           a["best"])
    with pytest.raises(ValueError, match=r"\(K \* B, Tp, 2 or 4\)"):
        ops.sample_nms(pos[:, :6], score, K, 5, 0.5)
    with pytest.raises(ValueError, match=r"\(K, B, 2\) = \(20, 7, 2\)"):
        ops.sample_nms(pos, score, K, 5, 0.5, err=err[:, :6])
    with pytest.raises(ValueError, match=r"M must lie in 1 \.\. K = 20"):
        ops.sample_nms(pos, score, K, 21, 0.5)
    for good in (pos, pos.view(K * B, Tp, 4), pos[..., :2].contiguous()):      # well-formed, but not on the GPU: no CPU fallback
        with pytest.raises(SocialWaysHipError):
            ops.sample_nms(good, score, K, 5, 0.5, err=err, best=best)


def test_public_surface():
    import socialways_amd as sw
    from socialways_amd import generic, wide
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        assert callable(getattr(cls, "sample_diverse")) and callable(getattr(cls, "evaluate_diverse"))
    assert callable(sw.stats.sample_modes)
    with pytest.raises(sw.SocialWaysHipError):             # no CPU fallback
        sw.stats.sample_modes(np.zeros((4, 3, 2, 2)), np.zeros((4, 3)), 0.5, 2, device="cpu")
    with pytest.raises(ValueError):
        sw.stats.sample_modes(np.zeros((4, 3, 2, 2)), np.zeros((4, 2)), 0.5, 2, device="cpu")


@pytest.mark.parametrize("top_m", [0, -1, 7])
def test_top_m_outside_1_to_k_is_refused(top_m):
    """Both calls check top_m against the number of draws before they sample anything (no trainer, no device needed)."""
    import socialways_amd as sw
    from socialways_amd import generic, wide
    me = types.SimpleNamespace(_device_noise=lambda noise: None, device="cpu")
    data = types.SimpleNamespace(ss=1.0)
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        with pytest.raises(ValueError, match="top_m must lie in 1"):
            cls.sample_diverse(me, torch.zeros(3, 8, 2), 6, top_m, 0.5)
        with pytest.raises(ValueError, match="top_m must lie in 1"):
            cls.evaluate_diverse(me, data, n_gen_samples=6, top_m=top_m)
    with pytest.raises(ValueError, match="metric"):
        sw.SocialWaysTrainer.evaluate_diverse(me, data, n_gen_samples=6, top_m=2, metric="mse")


def test_the_equidistant_leftover_case_is_exact_in_float32():
    """What tests/test_gpu_nms.py's tie case relies on: every distance of its input is the same number in fp32 and float64,
    draw 2 is equally far from both picks and strictly outside the radius, and draw 4 is strictly nearer to pick 1."""
    from test_gpu_nms import equidistant_leftover, nms_reference, pair_dist
    pos, score, M, radius = equidistant_leftover()
    for metric in ("fde", "ade"):
        for c in (0, 1):
            d64 = pair_dist(pos, c, metric)
            x = pos[..., 0, 0]
            d32 = np.abs(x - x[c]).astype(np.float32)                  # one step, y = 0: the distance is |dx|, exact
            assert np.array_equal(d64, d32.astype(np.float64))
        d0, d1 = pair_dist(pos, 0, metric)[:, 0], pair_dist(pos, 1, metric)[:, 0]
        assert d0[2] == d1[2] == 4.0 > radius and d1[4] < d0[4] and d0[3] <= radius
        assert nms_reference(pos, score, [(0, 1)], M, radius, metric)[3].tolist() == [[0, 1, 0, 0, 1]]
