"""Host side of the ragged observation histories (no GPU): the two entry points are declared and bound and reject bad
arguments before the device is touched, the Python layer refuses a bad obs_len, create_dataset_ragged() keeps the
pedestrians with short histories next to create_dataset()'s windows, and SceneDataset carries obs_len."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

from test_sample_host import declared_arguments

EARG, ESHAPE = -1, -2


def test_header_and_binding_agree_on_the_ragged_entry_points():
    from socialways_amd import _lib as L
    lib = L.load()
    for name, n in (("sw_enc_lstm_fwd_ragged", 9), ("sw_disc_score_ragged", 12)):
        assert name in L.PROTOTYPES
        res, args = L.PROTOTYPES[name]
        assert declared_arguments(name) == len(args) == n
        assert res is L._i and args[-1] is L._vp
        assert hasattr(lib, name)


def test_argument_validation_without_gpu():
    """Every SW_EARG / SW_ESHAPE / SW_OK case of both entry points; `p` is a non-NULL address nobody dereferences: each
    call returns from its argument checks (B == 0: SW_OK without a launch)."""
    from socialways_amd import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(128)
    p = (ctypes.addressof(buf) + 15) & ~15

    def enc(x=p, x_mode=0, enc_w=p, obs_len=p, B=0, T=8, hT=p, cT=p):
        return lib.sw_enc_lstm_fwd_ragged(x, x_mode, enc_w, obs_len, B, T, hT, cT, None)
    assert enc() == 0 and enc(obs_len=None) == 0 and enc(x_mode=1) == 0 and enc(T=2) == 0 and enc(x_mode=1, T=1) == 0
    for kw in (dict(x=None), dict(enc_w=None), dict(hT=None), dict(cT=None), dict(B=-1), dict(T=0), dict(T=-3), dict(x_mode=2),
               dict(x_mode=-1), dict(T=1)):
        assert enc(**kw) == EARG, kw
        if "B" not in kw:
            assert enc(B=7, **kw) == EARG, kw
            assert enc(B=7, obs_len=None, **kw) == EARG, kw

    def score(obsv=p, To=8, x_mode=0, obs_len=p, pred4=p, d_w=p, B=0, K=3, Tp=12, score=p, code=p):
        return lib.sw_disc_score_ragged(obsv, To, x_mode, obs_len, pred4, d_w, B, K, Tp, score, code, None)

    def dense(obsv=p, To=8, x_mode=0, obs_len=None, pred4=p, d_w=p, B=0, K=3, Tp=12, score=p, code=p):
        return lib.sw_disc_score(obsv, To, x_mode, pred4, d_w, B, K, Tp, score, code, None)
    assert score() == 0 and score(obs_len=None) == 0 and score(code=None) == 0 and score(x_mode=1, To=1) == 0 and score(To=2) == 0
    assert score(Tp=64) == 0 and score(K=1) == 0
    bad = (dict(obsv=None), dict(pred4=None), dict(d_w=None), dict(score=None), dict(K=0), dict(K=-1), dict(B=-1), dict(To=0),
           dict(Tp=0), dict(x_mode=2), dict(x_mode=-1), dict(To=1))
    for kw in bad:      # the same checks as sw_disc_score, case by case
        assert score(**kw) == EARG == dense(**kw), kw
        if "B" not in kw:
            assert score(B=7, **kw) == EARG == dense(B=7, **kw), kw
    assert score(Tp=65) == ESHAPE == dense(Tp=65) and score(B=7, Tp=65) == ESHAPE
    assert score(Tp=65, K=0) == EARG                       # the argument checks come first


def test_python_layer_refuses_a_bad_obs_len():
    from socialways_amd import ops, data as D
    B, To = 5, 8
    good = [2, 8, 3, 5, 8]
    for lo in (1, 2):
        assert D.check_obs_len(good, B, To, lo).dtype == np.int32
    assert ops.obs_len_arg(None, B, To, 2, "cpu") is None
    t = ops.obs_len_arg(good, B, To, 2, "cpu")
    assert t.dtype == torch.int32 and t.tolist() == good
    assert ops.obs_len_arg(np.asarray(good, dtype=np.int64), B, To, 2, "cpu").dtype == torch.int32
    assert ops.obs_len_arg(torch.tensor(good), B, To, 2, "cpu").tolist() == good
    for bad in (good[:4], good + [8], [1, 8, 3, 5, 8], [2, 9, 3, 5, 8], [2.0, 8.0, 3.0, 5.0, 8.0], np.asarray(good, dtype=np.float32),
                torch.tensor(good, dtype=torch.float32), torch.tensor(good[:4]), torch.tensor([good]), [0, 8, 3, 5, 8],
                [-1, 8, 3, 5, 8]):
        with pytest.raises(ValueError, match="obs_len"):
            ops.obs_len_arg(bad, B, To, 2, "cpu")
    assert ops.obs_len_arg([1, 8, 3, 5, 8], B, To, 1, "cpu").tolist() == [1, 8, 3, 5, 8]      # 4-d input: one state is enough
    with pytest.raises(ValueError, match="obs_len"):
        ops.obs_len_arg([0, 8, 3, 5, 8], B, To, 1, "cpu")
    with pytest.raises(ValueError, match="obs_len"):
        D.SceneDataset(np.zeros((B, To, 2)) + np.arange(To)[None, :, None], np.ones((B, 12, 2)), [[0, 2], [2, 5]], device="cpu",
                       obs_len=[2, 9, 3, 5, 8])


def test_public_surface_takes_obs_len():
    import socialways_amd as sw
    from socialways_amd import generic, ops, wide
    last = lambda f: list(inspect.signature(f).parameters.values())[-1]
    for f in (ops.gen_sample, ops.disc_score, sw.Generator.sample, sw.sample, sw.Discriminator.score_samples,
              sw.SocialWaysTrainer.sample_ranked, sw.SocialWaysTrainer.sample_diverse, sw.SceneDataset.__init__,
              generic.Generator.sample, generic.Discriminator.score_samples):
        assert last(f).name == "obs_len" and last(f).default is None, f      # appended: the positions in front are unchanged
    assert "obs_len" not in inspect.signature(sw.Generator.forward).parameters
    assert "obs_len" not in inspect.signature(sw.predict).parameters
    assert last(sw.biwi_to_npz).name == "min_past" and last(sw.biwi_to_npz).default is None
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        assert callable(cls.evaluate_history)
    # the refusals that need no device: a ragged dataset in test() / train_epoch(), an obs_len on the generic-width modules
    ragged = types.SimpleNamespace(obs_len=torch.tensor([2, 8], dtype=torch.int32))
    me = types.SimpleNamespace()
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
            cls.test(me, ragged)
        with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
            cls.train_epoch(me, ragged, 64)
    # ... and in the evaluate_*() family of those trainers, before a chunk is built (nothing of `me` but G is touched)
    me.G = object()
    for cls in (generic.GenericTrainer, wide.WideTrainer):
        with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
            next(cls._eval_draws(me, ragged, 3, False, None, None))
    with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
        generic.Generator.sample(me, torch.zeros(2, 8, 2), 3, 12, obs_len=[2, 8])
    with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
        generic.Discriminator.score_samples(me, torch.zeros(2, 8, 2), torch.zeros(3, 2, 12, 4), obs_len=[2, 8])


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """synth_crowd_frames() defaults written and parsed like tests/test_data.py does."""
    from socialways_amd import data as D
    path = str(tmp_path_factory.mktemp("ragged") / "obsmat.txt")
    D.write_biwi_obsmat(path, *D.synth_crowd_frames())
    p_data, t_data, interval = D.parse_biwi(path)
    return types.SimpleNamespace(path=path, p=p_data, t=t_data, range=range(int(t_data[0][0]), int(t_data[-1][-1]), interval))


def test_min_past_equal_to_n_past_reproduces_create_dataset(recording):
    from socialways_amd import data as D
    r = recording
    o0, p0, t0, b0 = D.create_dataset(r.p, r.t, r.range)
    o, p, t, b, n = D.create_dataset_ragged(r.p, r.t, r.range, min_past=8)
    assert len(o0) == 196
    assert o.dtype == o0.dtype and np.array_equal(o, o0) and np.array_equal(p, p0) and list(t) == list(t0)
    assert b.dtype == b0.dtype and np.array_equal(b, b0)
    assert n.dtype == np.int32 and n.shape == (196,) and (n == 8).all()
    for bad in (0, 9):
        with pytest.raises(ValueError, match="min_past"):
            D.create_dataset_ragged(r.p, r.t, r.range, min_past=bad)


def test_short_histories_join_the_full_windows(recording):
    from socialways_amd import data as D
    r = recording
    o0, p0, t0, b0 = D.create_dataset(r.p, r.t, r.range)
    o, p, t, b, n = D.create_dataset_ragged(r.p, r.t, r.range, min_past=2)
    assert o.shape == (340, 8, 2) and p.shape == (340, 12, 2) and len(t) == 340 and n.shape == (340,)
    assert np.bincount(n, minlength=9).tolist() == [0, 0, 24, 24, 24, 24, 24, 24, 196]
    full = n == 8
    assert np.array_equal(o[full], o0) and np.array_equal(p[full], p0)      # create_dataset's rows, in its order
    assert [x for x, f in zip(t, full) if f] == list(t0)
    assert len(b) == 41 and len(b0) == 35
    # batches: a partition of the rows into runs of equal t
    assert b[0, 0] == 0 and b[-1, 1] == 340 and (b[1:, 0] == b[:-1, 1]).all() and (b[:, 1] > b[:, 0]).all()
    t = np.asarray(t)
    for a, e in b:
        assert (t[a:e] == t[a]).all()
    assert (t[b[1:, 0]] > t[b[:-1, 0]]).all()
    # every row: its valid part is the pedestrian's samples in front of t, the padding repeats the first of them
    step = r.range.step
    samples = {}
    for pd, td in zip(r.p, r.t):
        for k, tt in enumerate(td):
            samples.setdefault(int(tt), []).append((pd, k))
    for row in range(340):
        hits = [(pd, k) for pd, k in samples[int(t[row])] if np.array_equal(pd[k:k + 12].astype(np.float32), p[row])]
        assert len(hits) == 1, row
        pd, k = hits[0]
        m = int(n[row])
        assert k >= m and np.array_equal(o[row, 8 - m:], pd[k - m:k].astype(np.float32))
        assert (o[row, :8 - m] == o[row, 8 - m]).all()
        assert m == 8 or k == m, "a history is short only because the track begins there"
    assert step == 6


def test_scene_dataset_carries_obs_len(recording, tmp_path):
    import socialways_amd as sw
    from socialways_amd import data as D
    r = recording
    o, p, t, b, n = D.create_dataset_ragged(r.p, r.t, r.range, min_past=2)
    plain = sw.SceneDataset(o, p, b, t, device="cpu")
    d = sw.SceneDataset(o, p, b, t, device="cpu", obs_len=n)
    assert plain.obs_len is None
    assert d.obs_len.dtype == torch.int32 and d.obs_len.shape == (340,) and np.array_equal(d.obs_len.numpy(), n)
    assert d.ss == plain.ss and vars(d.scale) == vars(plain.scale)
    assert torch.equal(d.obsv, plain.obsv) and torch.equal(d.pred, plain.pred)
    # the held-out fifth mixes lengths: what the GPU tests evaluate on
    held = d.obs_len[d.n_train_samples:].numpy()
    assert len(held) == 106 and int((held < 8).sum()) == 26
    assert sum(1 for a, e in d.test_batches if len(set(n[a:e])) > 1) == 5
    out = D.biwi_to_npz(r.path, str(tmp_path / "ragged.npz"), min_past=2)
    assert len(out) == 5 and np.array_equal(out[4], n) and np.array_equal(out[0], o)
    back = sw.SceneDataset.from_npz(str(tmp_path / "ragged.npz"), device="cpu")
    assert torch.equal(back.obs_len, d.obs_len) and torch.equal(back.obsv, d.obsv) and np.array_equal(back.the_batches, d.the_batches)
    # an evaluation set in another dataset's coordinates: every scene held out, that dataset's scale
    rows = np.arange(b[30, 0], b[-1, 1])
    ev = sw.SceneDataset.held_out(plain, o[rows], p[rows], b[30:] - b[30, 0], np.asarray(t)[rows], n[rows])
    assert ev.n_train_samples == 0 and ev.n_test_samples == len(rows) and np.array_equal(ev.test_batches, b[30:] - b[30, 0])
    assert ev.ss == plain.ss and ev.scale is plain.scale and len(ev.train_batches) == 0
    assert torch.equal(ev.obsv, plain.obsv[rows]) and torch.equal(ev.pred, plain.pred[rows])
    assert np.array_equal(ev.obs_len.numpy(), n[rows]) and sw.SceneDataset.held_out(plain, o[rows], p[rows], [[0, len(rows)]]).obs_len is None
    assert len(D.biwi_to_npz(r.path, str(tmp_path / "full.npz"))) == 4
    assert sw.SceneDataset.from_npz(str(tmp_path / "full.npz"), device="cpu").obs_len is None
