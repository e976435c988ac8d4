"""Host side of the ragged futures (no GPU): create_dataset_ragged(min_next=) keeps the pedestrians whose track ends inside
the horizon, SceneDataset carries pred_len, the Python layer refuses a bad pred_len, the training calls refuse such a dataset,
and the two new entry points are declared, bound and reject bad arguments before the device is touched."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

from test_sample_host import declared_arguments

EARG, ESHAPE = -1, -2


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """synth_crowd_frames() defaults written and parsed like tests/test_ragged_host.py does."""
    from socialways_amd import data as D
    path = str(tmp_path_factory.mktemp("ragged_next") / "obsmat.txt")
    D.write_biwi_obsmat(path, *D.synth_crowd_frames())
    p_data, t_data, interval = D.parse_biwi(path)
    return types.SimpleNamespace(path=path, p=p_data, t=t_data, range=range(int(t_data[0][0]), int(t_data[-1][-1]), interval))


def test_min_next_none_is_todays_builder(recording):
    from socialways_amd import data as D
    r = recording
    out = D.create_dataset_ragged(r.p, r.t, r.range, min_past=2)
    same = D.create_dataset_ragged(r.p, r.t, r.range, min_past=2, min_next=None)
    assert len(out) == len(same) == 5 and out[0].shape == (340, 8, 2)
    for a, b in zip(out, same):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for bad in (0, 13, -1, 1.5):
        with pytest.raises(ValueError, match="min_next"):
            D.create_dataset_ragged(r.p, r.t, r.range, min_next=bad)


def test_min_next_equal_to_n_next_reproduces_create_dataset(recording):
    from socialways_amd import data as D
    r = recording
    o0, p0, t0, b0 = D.create_dataset(r.p, r.t, r.range)
    out = D.create_dataset_ragged(r.p, r.t, r.range, min_past=8, min_next=12)
    assert len(out) == 6
    o, p, t, b, n, m = out
    assert o.dtype == o0.dtype and np.array_equal(o, o0) and p.dtype == p0.dtype and np.array_equal(p, p0)
    assert list(t) == list(t0) and b.dtype == b0.dtype and np.array_equal(b, b0)
    assert (n == 8).all() and m.dtype == np.int32 and m.shape == (196,) and (m == 12).all()
    # ... and with short histories: the five outputs of min_next=None
    five = D.create_dataset_ragged(r.p, r.t, r.range, min_past=2)
    six = D.create_dataset_ragged(r.p, r.t, r.range, min_past=2, min_next=12)
    for a, e in zip(five, six[:5]):
        assert np.array_equal(np.asarray(a), np.asarray(e))
    assert (six[5] == 12).all()


def test_short_futures_join_the_full_windows(recording):
    from socialways_amd import data as D
    r = recording
    o0, p0, t0, b0 = D.create_dataset(r.p, r.t, r.range)
    o, p, t, b, n, m = D.create_dataset_ragged(r.p, r.t, r.range, min_past=8, min_next=1)
    N = len(o)
    assert N > len(o0) and o.shape == (N, 8, 2) and p.shape == (N, 12, 2) and len(t) == N and m.shape == (N,) and m.dtype == np.int32
    assert (n == 8).all() and m.min() == 1 and m.max() == 12
    counts = np.bincount(m, minlength=13)
    assert (counts[1:] > 0).all(), "every future length 1 .. 12 occurs"
    # the counts of the issue: 450 windows in 45 scenes, 254 of them short, every short length at least 14 times
    assert N == 450 and len(b) == 45 and int((m < 12).sum()) == 254 and counts[1:12].min() == 14
    full = m == 12
    assert np.array_equal(o[full], o0) and np.array_equal(p[full], p0)      # create_dataset's rows, in its order
    # batches: a partition of the rows into runs of equal t
    assert b[0, 0] == 0 and b[-1, 1] == N and (b[1:, 0] == b[:-1, 1]).all() and (b[:, 1] > b[:, 0]).all()
    t = np.asarray(t)
    for a, e in b:
        assert (t[a:e] == t[a]).all()
    assert (t[b[1:, 0]] > t[b[:-1, 0]]).all()
    # every row: its valid part is the track from t on, the padding repeats the last valid sample, and a future is short
    # only because the track ends there
    samples = {}
    for pd, td in zip(r.p, r.t):
        for k, tt in enumerate(td):
            samples.setdefault(int(tt), []).append((pd, k))
    for row in range(N):
        j = int(m[row])
        hits = [(pd, k) for pd, k in samples[int(t[row])]
                if k >= 8 and np.array_equal(pd[k - 8:k].astype(np.float32), o[row]) and len(pd) >= k + j
                and np.array_equal(pd[k:k + j].astype(np.float32), p[row, :j])]
        assert len(hits) == 1, row
        pd, k = hits[0]
        assert (p[row, j:] == p[row, j - 1]).all()
        assert j == 12 or len(pd) == k + j, "a future is short only because the track ends there"
    assert np.isfinite(p).all()
    # min_next in between: the rows of min_next=1 with at least that many frames
    o5, p5, t5, b5, n5, m5 = D.create_dataset_ragged(r.p, r.t, r.range, min_past=8, min_next=5)
    assert np.array_equal(o5, o[m >= 5]) and np.array_equal(p5, p[m >= 5]) and np.array_equal(m5, m[m >= 5])


def test_a_gap_inside_the_future_ends_it():
    """One pedestrian, a sample every 10 frames from 0 to 190 with the one at 130 missing: at t = 80 the future runs
    80 .. 120 (5 samples), not across the gap."""
    from socialways_amd import data as D
    ts = np.array([10 * f for f in range(20) if f != 13], dtype=np.int32)
    pos = np.stack([ts.astype(np.float64), -ts.astype(np.float64)], axis=1)
    o, p, t, b, n, m = D.create_dataset_ragged([pos], [ts], range(0, 200, 10), n_past=4, n_next=8, min_past=4, min_next=1)
    assert len(t) == len(m) == len(p)
    at = list(t).index(80)
    assert m[at] == 5 and np.array_equal(p[at, :5, 0], [80, 90, 100, 110, 120]) and (p[at, 5:, 0] == 120).all()
    assert list(t).count(130) == 0                      # no sample at t = 130: no window
    assert m[list(t).index(120)] == 1 and m[list(t).index(40)] == 8
    # min_next = 8 asks for the whole horizon without a gap
    out = D.create_dataset_ragged([pos], [ts], range(0, 200, 10), n_past=4, n_next=8, min_past=4, min_next=8)
    assert len(out[2]) > 0 and all(tt + 70 < 130 or tt > 130 for tt in out[2]) and (out[5] == 8).all()


def test_python_layer_refuses_a_bad_pred_len(recording, tmp_path):
    import socialways_amd as sw
    from socialways_amd import data as D
    B, Tp = 5, 12
    good = [1, 12, 3, 5, 12]
    assert D.check_pred_len(good, B, Tp).dtype == np.int32 and D.check_pred_len(np.asarray(good, dtype=np.int64), B, Tp).tolist() == good
    obsvs = np.zeros((B, 8, 2)) + np.arange(8)[None, :, None]
    d = sw.SceneDataset(obsvs, np.ones((B, Tp, 2)), [[0, 2], [2, 5]], device="cpu")
    assert d.pred_len is None and sw.SceneDataset.pred_len is None
    for bad in (good[:4], good + [12], [0, 12, 3, 5, 12], [1, 13, 3, 5, 12], [-1, 12, 3, 5, 12], [1.0, 12.0, 3.0, 5.0, 12.0],
                np.asarray(good, dtype=np.float32), np.asarray([good]), torch.tensor(good, dtype=torch.float32)):
        with pytest.raises(ValueError, match="pred_len"):
            D.check_pred_len(bad.numpy() if isinstance(bad, torch.Tensor) else bad, B, Tp)
        with pytest.raises(ValueError, match="pred_len"):
            d.set_pred_len(bad)
        assert d.pred_len is None
    assert d.set_pred_len(good) is d
    assert d.pred_len.dtype == torch.int32 and d.pred_len.tolist() == good
    assert d.set_pred_len(torch.tensor(good)).pred_len.tolist() == good and d.set_pred_len(None).pred_len is None
    # the builder's output through the npz and back, and on a held-out set in another dataset's coordinates
    r = recording
    out = D.biwi_to_npz_ragged(r.path, str(tmp_path / "next.npz"), min_past=8)
    o, p, t, b, n, m = D.create_dataset_ragged(r.p, r.t, r.range, min_past=8, min_next=1)
    assert len(out) == 6 and np.array_equal(out[0], o) and np.array_equal(out[1], p) and np.array_equal(out[5], m)
    back = sw.SceneDataset.from_npz(str(tmp_path / "next.npz"), device="cpu")
    assert back.pred_len.dtype == torch.int32 and np.array_equal(back.pred_len.numpy(), m) and np.array_equal(back.obs_len.numpy(), n)
    plain = sw.SceneDataset(o, p, b, t, device="cpu")
    assert torch.equal(back.pred, plain.pred) and back.ss == plain.ss
    D.biwi_to_npz(r.path, str(tmp_path / "full.npz"))
    assert sw.SceneDataset.from_npz(str(tmp_path / "full.npz"), device="cpu").pred_len is None
    rows = np.arange(b[30, 0], b[-1, 1])
    ev = sw.SceneDataset.held_out(plain, o[rows], p[rows], b[30:] - b[30, 0], np.asarray(t)[rows])
    assert ev.pred_len is None and ev.set_pred_len(m[rows]) is ev and np.array_equal(ev.pred_len.numpy(), m[rows])
    with pytest.raises(ValueError, match="pred_len"):
        ev.set_pred_len(m[rows][:-1])


def test_public_surface_takes_pred_len():
    import socialways_amd as sw
    from socialways_amd import data as D, generic, ops, stats, wide
    params = lambda f: list(inspect.signature(f).parameters.values())
    names = lambda f: [q.name for q in params(f)]
    # the new keywords and functions, with their defaults
    g = params(ops.gen_sample)
    assert [q.name for q in g[-3:]] == ["keep_pred", "pred_len", "obs_len"] and g[-2].default is None and g[-3].default is False
    c = params(ops.scene_clearance)
    assert [q.name for q in c] == ["pos", "start", "scenes", "K", "inv_ss", "lens"] and c[-1].default is None and c[-2].default == 1.0
    assert names(ops.scene_metrics_len)[:8] == names(ops.scene_metrics)
    s = params(stats.scene_clearance_len)
    assert [q.name for q in s] == ["trajs", "sub_batches", "lens", "start", "scale", "device"]
    assert s[3].default is None and s[4].default == 1.0 and s[5].default == "cuda"
    b = params(D.create_dataset_ragged)
    assert [q.name for q in b[-2:]] == ["min_past", "min_next"] and b[-2].default == 2 and b[-1].default is None
    z = params(sw.biwi_to_npz_ragged)
    assert [(q.name, q.default) for q in z[2:]] == [("n_past", 8), ("n_next", 12), ("min_past", 2), ("min_next", 1)]
    assert names(D.check_pred_len) == ["pred_len", "B", "Tp"] and names(sw.SceneDataset.set_pred_len) == ["self", "pred_len"]
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        h = params(cls.evaluate_horizon)
        assert [(q.name, q.default) for q in h[1:]] == [("data", inspect.Parameter.empty), ("n_gen_samples", 20), ("just_one", False),
                                                       ("noise", None)]
    # the pinned signatures are what they were
    last = lambda f: params(f)[-1]
    for f in (ops.gen_sample, sw.SceneDataset.__init__, sw.Generator.sample):
        assert last(f).name == "obs_len" and last(f).default is None
    assert last(sw.biwi_to_npz).name == "min_past" and last(sw.biwi_to_npz).default is None
    assert names(stats.scene_clearance) == ["trajs", "sub_batches", "start", "scale", "device"]
    assert names(ops.scene_metrics) == ["err", "pred4", "obsv", "scenes", "K", "n_next", "inv_ss", "coll_dist"]
    assert names(sw.SocialWaysTrainer.evaluate_scenes)[1:] == ["data", "n_gen_samples", "coll_dist", "just_one", "collect"]
    assert names(sw.SocialWaysTrainer.evaluate)[1:] == ["data", "n_gen_samples", "write_to_file", "just_one", "collect", "noise"]
    assert names(sw.SocialWaysTrainer.evaluate_ranked)[1:] == ["data", "n_gen_samples", "top_m", "just_one", "collect", "noise"]
    assert names(sw.SocialWaysTrainer.evaluate_history)[1:] == ["data", "n_gen_samples", "just_one", "noise"]


def test_training_calls_refuse_a_dataset_with_pred_len():
    """No device: the refusals come before anything of the trainer is touched."""
    import socialways_amd as sw
    from socialways_amd import generic, wide
    short = types.SimpleNamespace(pred_len=torch.tensor([1, 12], dtype=torch.int32), obs_len=None)
    both = types.SimpleNamespace(pred_len=torch.tensor([1, 12], dtype=torch.int32), obs_len=torch.tensor([2, 8], dtype=torch.int32))
    me = types.SimpleNamespace()
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        for data in (short, both):
            with pytest.raises(sw.SocialWaysHipError, match="pred_len"):
                cls.test(me, data)
            with pytest.raises(sw.SocialWaysHipError, match="pred_len"):
                cls.train_epoch(me, data, 64)
            with pytest.raises(sw.SocialWaysHipError, match="pred_len"):
                cls.train_epoch_ragged(me, data, 64)
    # the evaluate*() family of the wide and generic trainers, before a chunk is built (nothing of `me` but G is touched)
    me.G = object()
    for cls in (generic.GenericTrainer, wide.WideTrainer):
        with pytest.raises(sw.SocialWaysHipError, match="pred_len"):
            next(cls._eval_draws(me, short, 3, False, None, None))
    # ops: the lengths describe gt and are an int32 tensor on the device of the tracks
    from socialways_amd import ops
    with pytest.raises(ValueError, match="pred_len"):
        ops._check_pred_len_tensor(torch.tensor([1, 12]), 2, torch.device("cpu"))
    with pytest.raises(ValueError, match="lens"):
        ops._check_pred_len_tensor(torch.tensor([1, 12, 3], dtype=torch.int32), 2, torch.device("cpu"), "lens")
    assert ops._check_pred_len_tensor(torch.tensor([1, 12], dtype=torch.int32), 2, torch.device("cpu")).tolist() == [1, 12]


def test_header_and_binding_agree_on_the_new_entry_points():
    from socialways_amd import _lib as L
    lib = L.load()
    for name, n in (("sw_dec_sample_fwd_plen", 17), ("sw_scene_clearance_len", 13)):
        assert name in L.PROTOTYPES
        res, args = L.PROTOTYPES[name]
        assert declared_arguments(name) == len(args) == n
        assert res is L._i and args[-1] is L._vp
        assert hasattr(lib, name)


def test_argument_validation_without_gpu():
    """Every check of the dense entries, case by case, with and without the lengths; `p` is an address nobody dereferences:
    each call returns from its argument checks (B == 0: SW_OK without a launch)."""
    from socialways_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    off = (ctypes.c_int * 3)(0, 2, 4)
    p, o = ctypes.addressof(buf), ctypes.addressof(off)
    assert p % 8 == 0

    def sample(obsv=p, To=8, z=p, S=p, hT=p, cT=p, enc=p, dec=p, B=0, K=3, Tp=12, pred4=p, gt=p, plen=p, inv_ss=1.0, err=p):
        return lib.sw_dec_sample_fwd_plen(obsv, To, z, S, hT, cT, enc, dec, B, K, Tp, pred4, gt, plen, inv_ss, err, None)

    def dense(obsv=p, To=8, z=p, S=p, hT=p, cT=p, enc=p, dec=p, B=0, K=3, Tp=12, pred4=p, gt=p, plen=None, inv_ss=1.0, err=p):
        return lib.sw_dec_sample_fwd(obsv, To, z, S, hT, cT, enc, dec, B, K, Tp, pred4, gt, inv_ss, err, None)
    for ok in (dict(), dict(plen=None), dict(S=None), dict(pred4=None), dict(err=None, gt=None), dict(Tp=1), dict(K=1), dict(To=2)):
        assert sample(**ok) == 0 == dense(**ok), ok
    bad = (dict(obsv=None), dict(z=None), dict(hT=None), dict(cT=None), dict(enc=None), dict(dec=None), dict(B=-1), dict(K=0),
           dict(To=1), dict(Tp=0), dict(pred4=None, err=None), dict(gt=None))
    for kw in bad:
        assert sample(**kw) == EARG == dense(**kw), kw
        assert sample(plen=None, **kw) == EARG, kw
        if "B" not in kw:
            assert sample(B=7, **kw) == EARG == dense(B=7, **kw), kw
    assert sample(B=1 << 30, K=4) == ESHAPE == dense(B=1 << 30, K=4)

    def clearance(pos=p, pstride=2, start=p, sstride=2, scene_off=o, lens=p, S=2, B=4, K=1, Tp=2, inv_ss=1.0, clear=p):
        return lib.sw_scene_clearance_len(pos, pstride, start, sstride, scene_off, lens, S, B, K, Tp, inv_ss, clear, None)
    for kw in (dict(pos=None), dict(scene_off=None), dict(clear=None), dict(pstride=3), dict(pstride=0), dict(pos=p + 4),
               dict(sstride=1), dict(S=-1), dict(B=-1), dict(K=0), dict(Tp=0), dict(inv_ss=0.0), dict(inv_ss=-1.0),
               dict(inv_ss=float("nan")), dict(S=1 << 30, K=4)):
        assert clearance(**kw) == EARG, kw
        assert clearance(lens=None, **kw) == EARG, kw
    assert clearance(B=0) == 0 and clearance(S=0) == 0 and clearance(B=0, lens=None) == 0 and clearance(S=0, start=None) == 0
