"""Ragged observation histories on the GPU: sw_enc_lstm_fwd_ragged / sw_disc_score_ragged against the dense entry points on
the truncated buffers (bit for bit), Generator.sample / score_samples / sample_ranked / sample_diverse with obs_len, the
mixed-length social case against the oracle's modules, and the evaluate_*() family on the ragged synthetic recording."""
import contextlib

import numpy as np
import pytest
import torch

import sw_oracle as O
from _util import assert_close, golden
from test_gpu_sample import SIZES, crowd

pytestmark = pytest.mark.gpu

RT, AT = 2e-5, 2e-6       # tests/test_gpu_kernels.py: pred_hat_4d against the reference
To, Tp, K = 8, 12, 3
B = int(np.sum(SIZES))    # 117 agents: a partial last tile, one scene above 64


def lengths(variant, lo=2, T=To, n=B):
    """cycle: lo .. T row by row, so every 16-row tile mixes all of them; tile2 / tile8: the second tile is all lo / all T."""
    ln = (np.arange(n) % (T - lo + 1)) + lo
    if variant == "tile2":
        ln[16:32] = lo
    elif variant == "tile8":
        ln[16:32] = T
    return ln.astype(np.int32)


def padded(x, ln, fill):
    """x with the columns in front of each row's valid frames overwritten: "repeat" = the first valid frame, else a value."""
    out = x.clone()
    T = x.shape[1]
    for r, n in enumerate(ln):
        out[r, :T - n] = x[r, T - n] if fill == "repeat" else fill
    return out


def groups(ln):
    return [(int(n), torch.from_numpy(np.flatnonzero(ln == n)).cuda()) for n in np.unique(ln)]


@contextlib.contextmanager
def gen_images(G, on):
    from socialways_amd import _lib as L
    if not on:
        yield
        return
    img = torch.empty(L.load().sw_gen_image_floats(), device="cuda")
    L.call("sw_gen_images", L.ptr(G.encoder._flat), L.ptr(G.decoder._flat), L.ptr(G.feature_embedder._flat),
           L.ptr(G.attention._flat), L.ptr(img), L.stream())
    try:
        yield
    finally:
        torch.cuda.synchronize()
        L.call("sw_gen_images", None, None, None, None, None, None)


@contextlib.contextmanager
def disc_images(D, on):
    from socialways_amd import _lib as L
    if not on:
        yield
        return
    lib = L.load()
    tab_h = np.empty((D._flat.numel(), 2), dtype=np.int32)
    assert lib.sw_disc_image_table(D.n_next, tab_h.ctypes.data) == 0
    tab = torch.from_numpy(tab_h).cuda()
    img = torch.zeros(lib.sw_disc_image_floats(D.n_next), device="cuda")
    L.call("sw_disc_images", L.ptr(D._flat), L.ptr(img), L.ptr(tab), D.n_next, L.stream())
    try:
        yield
    finally:
        torch.cuda.synchronize()
        L.call("sw_disc_images", None, None, None, 0, None)


def enc_dense(G, x, x_mode):
    from socialways_amd import _lib as L
    n, T = x.shape[0], x.shape[1]
    hT, cT = torch.empty(n, 64, device="cuda"), torch.empty(n, 64, device="cuda")
    L.call("sw_enc_lstm_fwd", L.ptr(x.contiguous()), x_mode, L.ptr(G.encoder._flat), None, None, n, T, L.ptr(hT), L.ptr(cT), None, None,
           None, 0, L.stream())
    return hT, cT


def enc_ragged(G, x, x_mode, ln):
    from socialways_amd import _lib as L
    n, T = x.shape[0], x.shape[1]
    hT, cT = torch.full((n, 64), 7.0, device="cuda"), torch.full((n, 64), 7.0, device="cuda")
    L.call("sw_enc_lstm_fwd_ragged", L.ptr(x.contiguous()), x_mode, L.ptr(G.encoder._flat), L.ptr(ln), n, T, L.ptr(hT), L.ptr(cT),
           L.stream())
    return hT, cT


def inputs(x_mode, T=To, seed=3):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.rand(B, T, 2, device="cuda", generator=gen) * 0.1 - 0.03).cumsum(1)
    if x_mode == 1:
        x = torch.cat([x, torch.rand(B, T, 2, device="cuda", generator=gen) * 0.1 - 0.05], dim=2)
    return x.contiguous()


@pytest.fixture(scope="module")
def G():
    import socialways_amd as sw
    torch.manual_seed(0)
    return sw.Generator(use_social=True, device="cuda:0")


# ---- 1. the encoder kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["cycle", "tile2", "tile8"])
@pytest.mark.parametrize("x_mode", [0, 1])
@pytest.mark.parametrize("images", [False, True])
def test_encoder_rows_equal_the_dense_kernel_on_the_truncated_buffers(G, images, x_mode, variant):
    lo = 2 if x_mode == 0 else 1
    ln = lengths(variant, lo)
    x = inputs(x_mode)
    with gen_images(G, images):
        hT, cT = enc_ragged(G, padded(x, ln, "repeat"), x_mode, torch.from_numpy(ln).cuda())
        hN, cN = enc_ragged(G, padded(x, ln, float("nan")), x_mode, torch.from_numpy(ln).cuda())
        hI, cI = enc_ragged(G, padded(x, ln, float("inf")), x_mode, torch.from_numpy(ln).cuda())
        assert sorted(n for n, _ in groups(ln)) == list(range(lo, To + 1))
        for n, idx in groups(ln):
            hD, cD = enc_dense(G, x[idx, To - n:], x_mode)
            assert torch.equal(hT[idx], hD) and torch.equal(cT[idx], cD), n
    assert torch.isfinite(hT).all() and float(hT.abs().max()) > 0
    assert torch.equal(hT, hN) and torch.equal(cT, cN) and torch.equal(hT, hI) and torch.equal(cT, cI)      # the padding is never read


@pytest.mark.parametrize("x_mode", [0, 1])
@pytest.mark.parametrize("images", [False, True])
def test_encoder_null_all_full_two_frames_and_device_clamp(G, images, x_mode):
    lo = 2 if x_mode == 0 else 1
    x = inputs(x_mode)
    with gen_images(G, images):
        hD, cD = enc_dense(G, x, x_mode)
        for ln in (None, torch.full((B,), To, dtype=torch.int32, device="cuda")):
            h, c = enc_ragged(G, x, x_mode, ln)
            assert torch.equal(h, hD) and torch.equal(c, cD)
        # out of range on the device: clamped into lo .. To, nothing out of bounds is read
        wild = torch.tensor([-5, 0, 1, To + 1, 100, 2 ** 31 - 1, -2 ** 31, 3], dtype=torch.int32).repeat(B // 8 + 1)[:B].cuda()
        h, c = enc_ragged(G, x, x_mode, wild)
        h2, c2 = enc_ragged(G, x, x_mode, wild.clamp(lo, To))
        assert torch.equal(h, h2) and torch.equal(c, c2) and torch.isfinite(h).all()
        # To = 2: positions have one valid length, 4-d states two
        x2 = inputs(x_mode, T=2, seed=9)
        ln = lengths("cycle", lo, T=2)
        h, c = enc_ragged(G, padded(x2, ln, float("nan")), x_mode, torch.from_numpy(ln).cuda())
        for n, idx in groups(ln):
            hD, cD = enc_dense(G, x2[idx, 2 - n:], x_mode)
            assert torch.equal(h[idx], hD) and torch.equal(c[idx], cD), n


# ---- 2. - 4. Generator.sample ------------------------------------------------------------------------------------------
def test_sample_without_social_equals_sample_on_the_truncated_observations():
    import socialways_amd as sw
    torch.manual_seed(0)
    G = sw.Generator(use_social=False, device="cuda:0")
    obsv, _, sb = crowd(SIZES)
    noise = torch.rand(K, B, 32, device="cuda")
    for variant in ("cycle", "tile2", "tile8"):
        ln = lengths(variant)
        got = G.sample(padded(obsv, ln, float("nan")), K, Tp, sb, noise, obs_len=ln)
        assert got.shape == (K, B, Tp, 4) and torch.isfinite(got).all()
        for n, idx in groups(ln):
            want = G.sample(obsv[idx, To - n:].contiguous(), K, Tp, [], noise[:, idx].contiguous())
            assert torch.equal(got[:, idx], want), (variant, n)
        assert torch.equal(sw.sample(padded(obsv, ln, "repeat"), K, Tp, sb, noise, generator=G, obs_len=list(ln)), got)
    full = G.sample(obsv, K, Tp, sb, noise)
    assert torch.equal(G.sample(obsv, K, Tp, sb, noise, obs_len=np.full(B, To)), full)
    for bad in ([2] * (B - 1), [1] + [8] * (B - 1), [9] + [8] * (B - 1), np.full(B, 8.0), torch.full((B,), 8.0, device="cuda"),
                torch.full((B, 1), 8, device="cuda")):
        with pytest.raises(ValueError, match="obs_len"):
            G.sample(obsv, K, Tp, sb, noise, obs_len=bad)


@pytest.mark.parametrize("n", [2, 5])
def test_social_sample_with_one_short_length_equals_sample_on_the_short_buffers(G, n):
    obsv, _, sb = crowd(SIZES)
    noise = torch.rand(K, B, 32, device="cuda")
    ln = np.full(B, n, dtype=np.int32)
    got = G.sample(padded(obsv, ln, float("nan")), K, Tp, sb, noise, obs_len=torch.from_numpy(ln).cuda())
    want = G.sample(obsv[:, To - n:].contiguous(), K, Tp, sb, noise)
    assert torch.equal(got, want)
    assert not torch.equal(got, G.sample(obsv, K, Tp, sb, noise))


def oracle_ragged(orc, obsv, ln, noise, sb):
    """Per agent the oracle's encoder over its valid frames from zero; then its social block on the last states and
    predict()'s decode loop (train.py:408-430), per draw."""
    n_all = obsv.shape[0]
    enc = orc.encoder
    h, c, last4 = torch.zeros(1, n_all, 64), torch.zeros(1, n_all, 64), torch.zeros(n_all, 4)
    with torch.no_grad():
        for n in np.unique(ln):
            idx = torch.from_numpy(np.flatnonzero(ln == n))
            o4 = O.get_traj_4d(obsv[idx, To - int(n):], [])
            enc.init_lstm(torch.zeros(1, len(idx), 64), torch.zeros(1, len(idx), 64))
            enc(o4)
            h[0, idx], c[0, idx], last4[idx] = enc.lstm_h[0][0], enc.lstm_h[1][0], o4[:, -1]
        S = O.social_pool_blockdiag(last4, h[0], sb, orc.feature_embedder, orc.attention)
        out = []
        for k in range(noise.shape[0]):
            enc.init_lstm(h.clone(), c.clone())
            last, steps = last4, []
            for _ in range(Tp):
                v = orc.decoder(enc.lstm_h[0].view(n_all, -1), S, noise[k]).view(n_all, 2)
                last = torch.cat([v + last[:, :2], v], dim=1)
                steps.append(last)
                enc(last)
            out.append(torch.stack(steps, 1))
    return torch.stack(out)


def test_social_sample_with_mixed_lengths_against_the_oracle():
    import socialways_amd as sw
    torch.manual_seed(4)
    tr = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0")
    orc = O.SocialWaysOracle(Tp, use_social=True)
    orc.load_state({k: {kk: vv.cpu() for kk, vv in v.items()} for k, v in tr.checkpoint().items() if k.endswith("_dict")})
    obsv, _, sb = crowd(SIZES)
    ln = lengths("cycle")
    full_scenes = [3, 6]                      # an 8-agent and a single-agent scene stay at full length
    for s in full_scenes:
        ln[sb[s, 0]:sb[s, 1]] = To
    noise = torch.rand(K, B, 32, device="cuda")
    got = tr.G.sample(padded(obsv, ln, float("nan")), K, Tp, sb, noise, obs_len=ln)
    want = oracle_ragged(orc, obsv.cpu(), ln, noise.cpu(), sb)
    assert_close(got.cpu().numpy(), want.numpy(), RT, AT, "mixed lengths vs the oracle's modules")
    dense = tr.G.sample(obsv, K, Tp, sb, noise)
    differs = (got != dense).flatten(2).any(2).all(0).cpu().numpy()      # per agent: every draw differs somewhere
    n_short = n_neigh = 0
    for s, (a, b) in enumerate(sb):
        if s in full_scenes:
            assert torch.equal(got[:, a:b], dense[:, a:b]), s      # a scene without a short row: the same bits
            continue
        assert (ln[a:b] < To).any()
        for r in range(a, b):
            assert differs[r], (s, r, ln[r])
            n_short += ln[r] < To
            n_neigh += ln[r] == To
    assert n_short > 80 and n_neigh > 8      # full-length rows that share a scene with a short one are among them


# ---- 5. the scoring kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tp,k", [(12, 5), (2, 1), (12, 1), (2, 5)])
@pytest.mark.parametrize("x_mode", [0, 1])
@pytest.mark.parametrize("images", [False, True])
def test_scores_equal_score_samples_on_the_truncated_observations(images, x_mode, tp, k):
    import socialways_amd as sw
    torch.manual_seed(5)
    D = sw.Discriminator(tp, 64, 2, device="cuda:0")
    lo = 2 if x_mode == 0 else 1
    x = inputs(x_mode, seed=11)
    preds = (torch.rand(k, B, tp, 4, device="cuda") * 0.2 - 0.1).contiguous()
    with disc_images(D, images):
        dense, dcode = D.score_samples(x, preds)
        for ln in (None, np.full(B, To), torch.full((B,), To, dtype=torch.int32, device="cuda")):
            s, c = D.score_samples(x, preds, obs_len=ln)
            assert torch.equal(s, dense) and torch.equal(c, dcode)
        for variant in ("cycle", "tile2", "tile8"):
            ln = lengths(variant, lo)
            score, code = D.score_samples(padded(x, ln, float("nan")), preds, obs_len=ln)
            assert score.shape == (k, B) and code.shape == (k, B, 2) and torch.isfinite(score).all()
            assert torch.equal(D.score_samples(padded(x, ln, "repeat"), preds, obs_len=torch.from_numpy(ln).cuda())[0], score)
            for n, idx in groups(ln):
                ws, wc = D.score_samples(x[idx, To - n:].contiguous(), preds[:, idx].contiguous())
                assert torch.equal(score[:, idx], ws) and torch.equal(code[:, idx], wc), (variant, n)
            if variant != "tile8":
                assert not torch.equal(score[:, 16:32], dense[:, 16:32])
    with pytest.raises(ValueError, match="obs_len"):
        D.score_samples(x, preds, obs_len=[lo - 1] + [To] * (B - 1))


# ---- 6. the deployment calls ---------------------------------------------------------------------------------------------
def test_sample_ranked_and_diverse_equal_their_composition_by_hand():
    import socialways_amd as sw
    from socialways_amd import ops
    torch.manual_seed(6)
    tr = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0")
    obsv, _, sb = crowd(SIZES)
    ln = lengths("cycle")
    obsv = padded(obsv, ln, "repeat")
    k, m = 6, 3
    noise = torch.rand(k, B, 32, device="cuda")
    ph = tr.G.sample(obsv, k, Tp, sb, noise, obs_len=ln)
    score = tr.D.score_samples(obsv, ph, obs_len=ln)[0]
    assert not torch.equal(score, tr.D.score_samples(obsv, ph)[0])
    trajs, sc, order = tr.sample_ranked(obsv, k, m, sb, noise, obs_len=ln)
    want_order, _ = ops.sample_rank(score, k, m)
    idx = want_order.t().long()
    assert torch.equal(order, want_order) and torch.equal(sc, score.gather(0, idx))
    assert torch.equal(trajs, ph.gather(0, idx[:, :, None, None].expand(m, B, Tp, 4)))
    for joint in (False, True):
        trajs, weight, sc, order, count = tr.sample_diverse(obsv, k, m, 0.05, "fde", joint, sb, noise, obs_len=torch.from_numpy(ln))
        scenes = ops.SceneIndex.get(sb, B, obsv.device) if joint else None
        o, cnt, w, _, _ = ops.sample_nms(ph, score, k, m, 0.05, "fde", scenes)
        assert torch.equal(order, o) and torch.equal(count, cnt) and torch.equal(weight, w)
        rows = o[torch.bucketize(torch.arange(B, device="cuda"), scenes.scene_off[1:].long(), right=True)] if joint else o
        assert torch.equal(trajs, tr._gather_picks(ph, rows.t().long(), 0.0))
        assert torch.equal(sc, tr._gather_picks(score, rows.t().long(), float("-inf")))
    dn = sw.DeviceNoise(17)
    a = tr.sample_ranked(obsv, k, m, sb, dn, row0=5, obs_len=ln)
    b = tr.sample_ranked(obsv, k, m, sb, dn, row0=5, obs_len=ln)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 7. evaluation on the ragged synthetic recording ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_eval(tmp_path_factory):
    import socialways_amd as sw
    from socialways_amd import data as D
    path = str(tmp_path_factory.mktemp("ragged") / "obsmat.txt")
    D.write_biwi_obsmat(path, *D.synth_crowd_frames())
    p_data, t_data, interval = D.parse_biwi(path)
    o, p, t, b, n = D.create_dataset_ragged(p_data, t_data, range(int(t_data[0][0]), int(t_data[-1][-1]), interval), min_past=2)
    data = sw.SceneDataset(o, p, b, t, device="cuda:0", obs_len=n)
    torch.manual_seed(8)
    tr = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0")
    tr.noise = sw.DeviceNoise(2024)
    data.arrays = (o, p, b, t)
    return data, tr


def test_evaluate_history_on_the_ragged_recording(ragged_eval):
    data, tr = ragged_eval
    held = data.obs_len[data.n_train_samples:].cpu().numpy()
    assert int((held < 8).sum()) >= 20
    assert sum(1 for a, b in data.test_batches if len(set(data.obs_len[a:b].tolist())) > 1) >= 3
    ev = tr.evaluate(data, n_gen_samples=5)
    assert tr.evaluate(data, n_gen_samples=5) == ev and all(np.isfinite(ev)) and min(ev) > 0
    hist = tr.evaluate_history(data, n_gen_samples=5)
    keys = ("ade_avg", "fde_avg", "ade_min", "fde_min")
    assert tuple(hist[k] for k in keys) == ev
    by = hist["by_len"]
    want = {int(n): int(c) for n, c in enumerate(np.bincount(held, minlength=9)) if c}
    assert {n: v["count"] for n, v in by.items()} == want and hist["n_agents"] == len(held) == data.n_test_samples
    for i, k in enumerate(keys):
        total = sum(v["count"] * v[k] for v in by.values()) / data.n_test_samples
        assert abs(total - ev[i]) <= 1e-12 * abs(ev[i]), k
    one = tr.evaluate_history(data, n_gen_samples=5, just_one=True)
    a, b = data.test_batches[0]
    assert sum(v["count"] for v in one["by_len"].values()) == b - a
    # a dataset without obs_len: the single bucket n_past
    import socialways_amd as sw
    plain = sw.SceneDataset(*data.arrays, device="cuda:0")
    assert torch.equal(plain.obsv, data.obsv) and plain.ss == data.ss
    hp = tr.evaluate_history(plain, n_gen_samples=5)
    assert list(hp["by_len"]) == [8] and hp["by_len"][8]["count"] == plain.n_test_samples
    assert tuple(hp[k] for k in keys) == tr.evaluate(plain, n_gen_samples=5)
    assert abs(hp["by_len"][8]["ade_avg"] - hp["ade_avg"]) <= 1e-12 * hp["ade_avg"]
    assert tuple(hp[k] for k in keys) != ev      # the short rows were encoded over their valid frames


def test_evaluate_family_on_the_ragged_recording(ragged_eval):
    data, tr = ragged_eval
    ev = tr.evaluate(data, n_gen_samples=5)
    sc = tr.evaluate_scenes(data, n_gen_samples=5)
    rk = tr.evaluate_ranked(data, n_gen_samples=5, top_m=2)
    dv = tr.evaluate_diverse(data, n_gen_samples=5, top_m=2, radius=0.2)
    for out in (sc, rk, dv):
        assert tuple(out[k] for k in ("ade_avg", "fde_avg", "ade_min", "fde_min")) == ev
    assert sc["ade_min"] <= sc["jade_min"] <= sc["ade_avg"]
    assert rk["ade_min"] <= rk["ade_topm"] <= rk["ade_top1"]
    assert dv["ade_min"] <= dv["ade_divm"] <= dv["ade_div1"]
    coll = []
    assert tr.evaluate(data, n_gen_samples=5, collect=coll) == ev
    assert len(coll) == len(data.test_batches)
    import socialways_amd as sw
    from socialways_amd import predict_cv

    def check_records(records, d):
        """obs_len of every record, and preds_lnr = predict_cv of each row's valid frames (two frames: the two-frame rule)."""
        for rec, (a, b) in zip(records, d.test_batches):
            ln = d.obs_len[a:b].cpu().numpy()
            assert np.array_equal(rec["obs_len"], ln) and rec["obs_len"].dtype == np.int32
            for r in range(b - a):
                want = predict_cv(d.obsv[a + r:a + r + 1, 8 - min(int(ln[r]), 3):], 12)
                assert np.array_equal(rec["preds_lnr"][r], d.scale.denormalize(want[0].cpu().numpy())), (a, r, ln[r])
    check_records(coll, data)
    # the held-out rows have 3 .. 8 frames: the same windows with every history cut to two frames show the two-frame rule
    two = sw.SceneDataset(*data.arrays, device="cuda:0", obs_len=np.full(len(data.arrays[0]), 2))
    coll2 = []
    tr.evaluate(two, n_gen_samples=5, collect=coll2)
    assert len(coll2) == len(coll)
    check_records(coll2, two)
    padded_rule = predict_cv(two.obsv[two.n_train_samples:], 12)      # a velocity through the padding: not what is recorded
    assert not np.array_equal(np.concatenate([r["preds_lnr"] for r in coll2]), two.scale.denormalize(padded_rule.cpu().numpy()))
    rcoll = []
    tr.evaluate_ranked(data, n_gen_samples=5, top_m=2, collect=rcoll)
    assert all("obs_len" in r and "score" in r for r in rcoll)


def test_full_length_obs_len_changes_no_evaluation_number():
    import socialways_amd as sw
    g = golden("biwi_synth")
    torch.manual_seed(9)
    tr = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0")
    tr.noise = sw.DeviceNoise(7)
    plain = sw.SceneDataset(g["obsvs"], g["preds"], g["batches"], g["times"], device="cuda:0")
    full = sw.SceneDataset(g["obsvs"], g["preds"], g["batches"], g["times"], device="cuda:0", obs_len=np.full(len(g["obsvs"]), 8))
    assert plain.obs_len is None and full.obs_len is not None and plain.n_test_samples > 0
    for call in (lambda d: tr.evaluate(d, n_gen_samples=4), lambda d: tr.evaluate_scenes(d, n_gen_samples=4),
                 lambda d: tr.evaluate_ranked(d, n_gen_samples=4, top_m=2),
                 lambda d: tr.evaluate_diverse(d, n_gen_samples=4, top_m=2, radius=0.3),
                 lambda d: {k: v for k, v in tr.evaluate_history(d, n_gen_samples=4).items()}):
        assert call(plain) == call(full)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_paths_without_ragged_kernels_refuse(ragged_eval):
    import socialways_amd as sw
    data, tr = ragged_eval
    w0 = tr.G.encoder._flat.clone()
    with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
        tr.test(data, n_gen_samples=2)
    with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
        tr.train_epoch(data, 64)
    assert torch.equal(tr.G.encoder._flat, w0) and tr.epoch == 0
    obsv, _, sb = crowd([3, 4])
    ln = [2, 8, 5, 8, 8, 3, 8]
    torch.manual_seed(0)
    from socialways_amd import generic
    others = [sw.SocialWaysTrainer(Tp, hidden_size=128, device="cuda:0"),                           # the wide path
              generic.GenericTrainer(Tp, hidden_size=64, n_latent_codes=3, device="cuda:0")]      # the generic path
    assert [type(t).__name__ for t in others] == ["WideTrainer", "GenericTrainer"]
    for wt in others:
        with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
            wt.G.sample(obsv, 2, Tp, sb, obs_len=ln)
        with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
            wt.D.score_samples(obsv, torch.zeros(2, 7, Tp, 4, device="cuda"), obs_len=ln)
        with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
            wt.sample_ranked(obsv, 2, 1, sb, obs_len=ln)
        with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
            wt.sample_diverse(obsv, 2, 1, 0.1, sub_batches=sb, obs_len=ln)
        for call in (wt.test, wt.evaluate, wt.evaluate_scenes, wt.evaluate_history, lambda d, **kw: wt.evaluate_ranked(d, top_m=1, **kw),
                     lambda d, **kw: wt.evaluate_diverse(d, top_m=1, **kw)):
            with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
                call(data, n_gen_samples=2)
        with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
            wt.train_epoch(data, 64)
