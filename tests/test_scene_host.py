"""Host side of the scene-level K-sample metrics (no GPU): the two C-ABI entry points are declared, bound and reject bad
arguments before the device is touched, and the public surface exists."""
import ctypes
import inspect

from test_sample_host import declared_arguments


def test_header_and_binding_agree_on_the_scene_entry_points():
    from socialways_amd import _lib as L
    lib = L.load()
    for name, n_args in (("sw_scene_clearance", 12), ("sw_scene_reduce", 10)):
        assert name in L.PROTOTYPES, name
        res, args = L.PROTOTYPES[name]
        assert declared_arguments(name) == len(args) == n_args
        assert res is L._i and args[-1] is L._vp           # status int, void* stream last
        assert hasattr(lib, name)


def test_scene_entry_points_reject_bad_arguments_without_a_device():
    from socialways_amd import _lib as L
    lib = L.load()
    EARG = -1
    buf = (ctypes.c_float * 64)()               # host memory with 8-byte alignment: never dereferenced by a rejected call
    off = (ctypes.c_int * 3)(0, 2, 4)
    p, o = ctypes.addressof(buf), ctypes.addressof(off)
    assert p % 8 == 0

    def clearance(pos=p, pstride=2, start=p, sstride=2, scene_off=o, S=2, B=4, K=1, Tp=2, inv_ss=1.0, clear=p):
        return lib.sw_scene_clearance(pos, pstride, start, sstride, scene_off, S, B, K, Tp, inv_ss, clear, None)
    for kw in (dict(pos=None), dict(scene_off=None), dict(clear=None), dict(pstride=3), dict(pstride=0), dict(pos=p + 4),
               dict(sstride=1), dict(S=-1), dict(B=-1), dict(K=0), dict(Tp=0), dict(inv_ss=0.0), dict(inv_ss=-1.0),
               dict(inv_ss=float("nan")), dict(S=1 << 30, K=4)):
        assert clearance(**kw) == EARG, kw
    assert clearance(B=0) == 0 and clearance(S=0) == 0          # a successful no-op, still without a device
    assert clearance(B=0, start=None, sstride=0) == 0 and clearance(S=0, pstride=4) == 0
    for kw in (dict(pos=p + 4), dict(pstride=3), dict(sstride=1), dict(inv_ss=0.0)):
        assert clearance(B=0, **kw) == EARG and clearance(S=0, **kw) == EARG, kw      # the checks come before the early return

    def reduce(err=p, clear=p, scene_off=o, S=2, B=4, K=1, coll=0.1, per_scene=p, best=None):
        return lib.sw_scene_reduce(err, clear, scene_off, S, B, K, coll, per_scene, best, None)
    for kw in (dict(err=None), dict(scene_off=None), dict(per_scene=None), dict(S=-1), dict(B=-1), dict(K=0), dict(err=p + 4)):
        assert reduce(**kw) == EARG, kw
    assert reduce(B=0) == 0 and reduce(S=0) == 0 and reduce(B=0, clear=None) == 0


def test_public_surface():
    import socialways_amd as sw
    from socialways_amd import generic, ops, stats, wide
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        fn = getattr(cls, "evaluate_scenes")
        assert callable(fn)
        assert list(inspect.signature(fn).parameters)[1:] == ["data", "n_gen_samples", "coll_dist", "just_one", "collect"]
        assert inspect.signature(fn).parameters["coll_dist"].default == 0.1
    assert "stats" in sw.__all__ and callable(stats.scene_clearance)
    assert list(inspect.signature(stats.scene_clearance).parameters) == ["trajs", "sub_batches", "start", "scale", "device"]
    assert list(inspect.signature(ops.scene_metrics).parameters) == ["err", "pred4", "obsv", "scenes", "K", "n_next", "inv_ss",
                                                                   "coll_dist"]
    assert inspect.signature(ops.gen_sample).parameters["keep_pred"].default is False


def test_the_threshold_case_separates_strict_from_non_strict():
    """What tests/test_gpu_scene.py's threshold case relies on: its clearances hit coll_dist exactly, and in every scene of
    two or more agents the per-agent collision share with `<` (the definition) and with `<=` differ by far more than the
    relative 1e-5 of check_reduce."""
    import numpy as np
    from test_gpu_scene import SIZES, clearances_on_the_threshold, scene_reference
    err, clear, coll = clearances_on_the_threshold()
    assert clear.dtype == np.float32 and np.float32(coll) == coll and 0.05 < (clear == np.float32(coll)).mean() < 0.2
    want, _ = scene_reference(err, clear, SIZES, coll)
    o = np.concatenate([[0], np.cumsum(SIZES)])
    for s, n in enumerate(SIZES):
        if n > 1:
            loose = (clear[:, o[s]:o[s + 1]] <= np.float32(coll)).mean()
            assert loose - want[s, 5] > 1e-3 * max(want[s, 5], 1e-3), (s, n, loose, want[s, 5])
    assert clear[0].min() == np.float32(coll)
