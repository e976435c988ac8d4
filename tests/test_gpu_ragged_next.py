"""Ragged futures on the GPU: sw_dec_sample_fwd_plen and sw_scene_clearance_len tied bit for bit to the dense launches on
truncated buffers (which tests/test_gpu_gen_reference.py and tests/test_gpu_scene.py hold to float64), the mixed-length
clearance against a float64 implementation of its definition, and the evaluate*() family on a held-out set whose futures
end inside the horizon.

`evaluate_horizon()`: a row's contribution to its bucket is checked in two ways - the bucket does not change by a bit when
every OTHER row's length and ground truth change (a row is scored against its own valid frames and nothing else), and it
equals the float64 recomputation from the collected records over the rows of that length.  A dataset cut down to the rows
of one length would not see the same draws: the noise streams are indexed by the held-out row."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from _util import assert_close
from test_gpu_sample import crowd as sample_crowd, scene_list
from test_gpu_scene import EPS, clearance_bound, crowd as scene_crowd, dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Tp = 12
KEYS = ("ade_avg", "fde_avg", "ade_min", "fde_min")


# ---- 1. the sampling launch -------------------------------------------------------------------------------------------------
def sizes_of(B):
    return {1: [1], 17: [1, 5, 11], 40: [17, 3, 20], 33: [8, 1, 24]}[B]


def mixed_lengths(B, tp=Tp, seed=0):
    """Lengths 1 .. tp mixed inside every 16-row tile, 1 and tp among them (B >= 2)."""
    ln = np.random.RandomState(seed).randint(1, tp + 1, size=B).astype(np.int32)
    if B >= 2:
        ln[0], ln[1] = 1, tp
    if B >= 17:
        ln[B - 1], ln[16] = tp, 1
    return ln


def sample(G, obsv, noise, sb, gt, n_next, pred_len=None, want_pred=True):
    """ops.gen_sample: (pred4 (K * B, n_next, 4) or None, err (K, B, 2))."""
    from socialways_amd import ops
    K, B = noise.shape[0], obsv.shape[0]
    scenes = ops.SceneIndex.get(sb, B, obsv.device)
    pl = None if pred_len is None else torch.as_tensor(pred_len, dtype=torch.int32).cuda()
    pred4, red = ops.gen_sample(G.encoder.packed(), G.feature_embedder.packed(), G.attention.packed(), G.decoder.packed(), obsv,
                                noise.reshape(K * B, 32), scenes, n_next, G.use_social, K, gt=gt, inv_ss=0.7, want_pred=want_pred,
                                pred_len=pl)
    return pred4, red[2]


def check_rows_against_truncated_dense(G, obsv, noise, sb, gt, ln, err):
    """Every distinct length n: the dense launch with Tp = n on the contiguous truncation of gt, the rows of that length."""
    for n in sorted(set(ln.tolist())):
        _, want = sample(G, obsv, noise, sb, gt[:, :n].contiguous(), n, want_pred=False)
        rows = torch.from_numpy(ln == n).cuda()
        assert torch.equal(err[:, rows], want[:, rows]), "length %d: max |diff| %.3g" % (n, float((err[:, rows] - want[:, rows]).abs().max()))


@pytest.mark.parametrize("social", [False, True])
@pytest.mark.parametrize("B", [1, 17, 40])
def test_sampling_launch_equals_the_dense_launch_on_truncated_futures(B, social):
    import socialways_amd as sw
    torch.manual_seed(3)
    G = sw.Generator(use_social=social, device="cuda:0")
    sizes = sizes_of(B)
    obsv, gt, sb = sample_crowd(sizes, seed=7)
    K = 3
    noise = torch.rand(K, B, 32, device="cuda")
    dense4, dense_err = sample(G, obsv, noise, sb, gt, Tp)
    for ln in ([np.asarray([v], np.int32) for v in (1, 5, 12)] if B == 1 else [mixed_lengths(B)]):
        assert B == 1 or (ln.min() == 1 and ln.max() == Tp and len(set(ln[:16].tolist())) > 2)
        pred4, err = sample(G, obsv, noise, sb, gt, Tp, ln)
        assert err.shape == (K, B, 2) and torch.isfinite(err).all() and float(err.min()) > 0
        assert torch.equal(pred4, dense4), "the rollout is untouched"
        check_rows_against_truncated_dense(G, obsv, noise, sb, gt, ln, err)
        full = torch.from_numpy(ln == Tp).cuda()
        assert torch.equal(err[:, full], dense_err[:, full])
        # metrics only: no trajectory leaves the kernel, the same errors
        none, err2 = sample(G, obsv, noise, sb, gt, Tp, ln, want_pred=False)
        assert none is None and torch.equal(err2, err)
        # NaN in the padding changes nothing
        bad = gt.clone()
        bad[torch.arange(Tp, device="cuda")[None, :] >= torch.from_numpy(ln).cuda()[:, None]] = float("nan")
        assert B == 1 and ln[0] == Tp or torch.isnan(bad).any()
        p3, err3 = sample(G, obsv, noise, sb, bad, Tp, ln)
        assert torch.equal(err3, err) and torch.equal(p3, dense4)
        # a bad length on the device is clamped into 1 .. Tp
        wild = ln.copy()
        wild[ln == 1], wild[ln == Tp] = 0, 99
        if B > 1:
            wild[2] = -7
            ln2 = ln.copy()
            ln2[2] = 1
            _, err4 = sample(G, obsv, noise, sb, gt, Tp, wild, want_pred=False)
            assert torch.equal(err4, sample(G, obsv, noise, sb, gt, Tp, ln2, want_pred=False)[1])
    # no lengths, and all lengths Tp: the dense call
    p5, err5 = sample(G, obsv, noise, sb, gt, Tp, None)
    p6, err6 = sample(G, obsv, noise, sb, gt, Tp, np.full(B, Tp, np.int32))
    assert torch.equal(err5, dense_err) and torch.equal(p5, dense4) and torch.equal(err6, dense_err) and torch.equal(p6, dense4)


def test_sampling_entry_in_all_three_output_combinations_without_images():
    """The C entry itself, no weight images registered (the prologue without them), S_pool = NULL: err and pred4, err alone,
    pred4 alone (nothing for the lengths to say: the dense launch), and pred_len = NULL."""
    import socialways_amd as sw
    from socialways_amd import _lib as L
    torch.manual_seed(4)
    G = sw.Generator(use_social=False, device="cuda:0")
    B, K, To = 17, 3, 8
    obsv, gt, _ = sample_crowd(sizes_of(B), seed=9)
    z = torch.rand(K * B, 32, device="cuda")
    ln = torch.from_numpy(mixed_lengths(B, seed=2)).cuda()
    enc_w, dec_w = G.encoder.packed(), G.decoder.packed()
    hT, cT = torch.empty(B, 64, device="cuda"), torch.empty(B, 64, device="cuda")
    p, st = L.ptr, L.stream()
    L.call("sw_enc_lstm_fwd_aux", p(obsv), 0, p(enc_w), None, None, B, To, p(hT), p(cT), None, None, None, 0, None, None, 0, st)

    def plen(want_pred, want_err, lens=ln, gt=gt):
        pred4 = torch.full((K * B, Tp, 4), 7.0, device="cuda") if want_pred else None
        err = torch.full((K, B, 2), 7.0, device="cuda") if want_err else None
        L.call("sw_dec_sample_fwd_plen", p(obsv), To, p(z), None, p(hT), p(cT), p(enc_w), p(dec_w), B, K, Tp, p(pred4),
               p(gt) if want_err else None, p(lens), 0.7, p(err), st)
        return pred4, err

    def dense(tp, gt):
        pred4, err = torch.empty(K * B, tp, 4, device="cuda"), torch.empty(K, B, 2, device="cuda")
        L.call("sw_dec_sample_fwd", p(obsv), To, p(z), None, p(hT), p(cT), p(enc_w), p(dec_w), B, K, tp, p(pred4), p(gt), 0.7, p(err), st)
        return pred4, err
    d4, derr = dense(Tp, gt)
    both4, both_err = plen(True, True)
    _, only_err = plen(False, True)
    only4, _ = plen(True, False)
    assert torch.equal(both4, d4) and torch.equal(only4, d4) and torch.equal(only_err, both_err)
    for n in sorted(set(ln.tolist())):
        rows = ln == n
        assert torch.equal(both_err[:, rows], dense(n, gt[:, :n].contiguous())[1][:, rows]), n
    null4, null_err = plen(True, True, lens=None)
    assert torch.equal(null4, d4) and torch.equal(null_err, derr)
    assert not torch.equal(both_err, derr)


_TILE_SNIPPET = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from test_gpu_ragged_next import two_tile_case
pred4, err, _ = two_tile_case(torch.load(sys.argv[2]))
torch.save({"pred4": pred4.cpu(), "err": err.cpu()}, sys.argv[3])
'''


def two_tile_case(inp):
    import socialways_amd as sw
    torch.manual_seed(5)
    G = sw.Generator(use_social=True, device="cuda:0")
    obsv, gt, sb = sample_crowd(sizes_of(33), seed=11)
    noise, ln = inp["noise"].cuda(), inp["ln"].numpy()
    pred4, err = sample(G, obsv, noise, sb, gt, Tp, ln)
    return pred4, err, (G, obsv, noise, sb, gt, ln)


def test_sampling_launch_above_256_tiles_in_both_tile_forms(tmp_path):
    """K * B > 256 * 16 rows: the two-tile body (images registered by gen_sample); SW_DEC_FWD2=0 in a child process (the switch
    is read once per process) forces one tile per workgroup.  Same bits, and both tied to the dense launch per length."""
    B, K = 33, 128
    assert K * B > 256 * 16
    inp = {"noise": torch.rand(K, B, 32), "ln": torch.from_numpy(mixed_lengths(B, seed=6))}
    fin, fout = str(tmp_path / "in.pt"), str(tmp_path / "one_tile.pt")
    torch.save(inp, fin)
    pred4, err, (G, obsv, noise, sb, gt, ln) = two_tile_case(inp)
    check_rows_against_truncated_dense(G, obsv, noise, sb, gt, ln, err)
    assert torch.equal(pred4, sample(G, obsv, noise, sb, gt, Tp)[0])
    p = subprocess.run([sys.executable, "-c", _TILE_SNIPPET, ROOT, fin, fout], env=dict(os.environ, SW_DEC_FWD2="0"), capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    one = torch.load(fout)
    assert torch.equal(one["err"], err.cpu()) and torch.equal(one["pred4"], pred4.cpu())


def test_one_step_horizon():
    import socialways_amd as sw
    torch.manual_seed(6)
    G = sw.Generator(use_social=True, device="cuda:0")
    obsv, gt, sb = sample_crowd(sizes_of(17), Tp=1, seed=13)
    noise = torch.rand(3, 17, 32, device="cuda")
    d4, derr = sample(G, obsv, noise, sb, gt, 1)
    p4, err = sample(G, obsv, noise, sb, gt, 1, np.ones(17, np.int32))
    assert torch.equal(p4, d4) and torch.equal(err, derr) and torch.equal(err[..., 0], err[..., 1])


# ---- 2. the clearance -------------------------------------------------------------------------------------------------------
SC_SIZES = [1, 2, 5, 33, 70]      # packed lanes, one full wave, the agent-tile loop


def clearance_len(last, fut, lens, sizes, inv_ss):
    """The definition in float64: the segment of pair (a, b) that ends at frame t counts if t < min(lens[a], lens[b]); segments
    run from t = 0 with a start point, else from t = 1.  fut (K, B, T, 2) -> (K, B), +inf where nothing counts."""
    fut = fut.astype(np.float64)
    K, B, T, _ = fut.shape
    path, first = fut, 1
    if last is not None:
        path, first = np.concatenate([np.broadcast_to(last.astype(np.float64)[None, :, None], (K, B, 1, 2)), fut], 2), 0
    out, o = np.full((K, B), np.inf), 0
    ends = np.arange(first, T)                                  # the frame at which segment j ends
    for n in sizes:
        p, ln = path[:, o:o + n], np.asarray(lens[o:o + n])
        for a in range(n):
            for b in range(n):
                on = ends < min(ln[a], ln[b])
                if a == b or not on.any():
                    continue
                r0 = (p[:, a, :-1] - p[:, b, :-1])[:, on]
                dv = (p[:, a, 1:] - p[:, b, 1:])[:, on] - r0
                dd, rd = (dv * dv).sum(-1), (r0 * dv).sum(-1)
                tau = np.where(dd > 0, np.clip(-rd / np.where(dd > 0, dd, 1), 0, 1), 0)
                c = r0 + tau[..., None] * dv
                out[:, o + a] = np.minimum(out[:, o + a], np.sqrt((c * c).sum(-1)).min(-1) * inv_ss)
        o += n
    return out


def run_clearance_len(obs, fut, lens, inv_ss, with_start, pstride=2):
    from socialways_amd import ops
    K, B = fut.shape[:2]
    pos = fut if pstride == 2 else np.concatenate([fut, np.full_like(fut, 1e3)], axis=-1)
    scenes = ops.SceneIndex.get(scene_list(SC_SIZES), B, torch.device("cuda", 0))
    start = dev(obs)[:, -1] if with_start else None
    ln = None if lens is None else torch.as_tensor(np.asarray(lens), dtype=torch.int32).cuda()
    out = ops.scene_clearance(dev(pos), start, scenes, K, inv_ss, lens=ln)
    assert out.shape == (K, B) and out.dtype == torch.float32
    return out.cpu().numpy()


@pytest.mark.parametrize("with_start", [True, False])
@pytest.mark.parametrize("T", [12, 20])
def test_clearance_with_one_length_equals_the_dense_kernel_on_truncated_paths(T, with_start):
    K, inv_ss = 3, 15.0
    obs, fut = scene_crowd(SC_SIZES, K, Tp=T, seed=4)
    B = fut.shape[1]
    dense = run_clearance_len(obs, fut, None, inv_ss, with_start)
    assert np.isfinite(dense[:, 1:]).all() and np.isinf(dense[:, 0]).all()
    assert np.array_equal(run_clearance_len(obs, fut, np.full(B, T), inv_ss, with_start), dense)
    junk = np.random.RandomState(1).rand(*fut.shape).astype(np.float32) * 100
    for n in range(1, T + 1):
        want = run_clearance_len(obs, np.ascontiguousarray(fut[:, :, :n]), None, inv_ss, with_start)
        assert np.array_equal(run_clearance_len(obs, fut, np.full(B, n), inv_ss, with_start), want), n
        if n in (1, 7, 16, T):      # what lies behind the length - numbers or NaN - changes nothing
            for fill in (junk, np.full_like(fut, np.nan)):
                other = np.where(np.arange(T)[None, None, :, None] < n, fut, fill)
                assert np.array_equal(run_clearance_len(obs, other, np.full(B, n), inv_ss, with_start), want), n
    assert np.isinf(run_clearance_len(obs, fut, np.full(B, 1), inv_ss, False)).all()      # one frame, no start: no segment


@pytest.mark.parametrize("with_start", [True, False])
@pytest.mark.parametrize("T", [12, 20])
def test_clearance_with_mixed_lengths_against_float64(T, with_start):
    from socialways_amd import _lib as L
    from socialways_amd import ops
    K, inv_ss = 3, 15.0
    obs, fut = scene_crowd(SC_SIZES, K, Tp=T, seed=5)
    B = fut.shape[1]
    rng = np.random.RandomState(T)
    lens = rng.randint(1, T + 1, size=B).astype(np.int32)
    lens[1], lens[2] = 1, T                    # the scene of two: one agent seen for a single frame
    lens[3], lens[8], lens[41], lens[B - 1] = 1, T, 1, 1
    want = clearance_len(obs[:, -1] if with_start else None, fut, lens, SC_SIZES, inv_ss)
    M = max(float(np.abs(fut).max()), float(np.abs(obs[:, -1]).max()))
    fin = np.isfinite(want)
    assert np.isinf(want[:, 0]).all() and fin[:, 8].all()
    if not with_start:                         # a single frame and no start point: no segment counts, for either of the pair
        assert np.isinf(want[:, [1, 2, 3, 41, B - 1]]).all()
    for pstride in (2, 4):
        got = run_clearance_len(obs, fut, lens, inv_ss, with_start, pstride)
        assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])      # +inf where no segment counts
        e = float(np.abs(got[fin] - want[fin]).max())
        print("clearance_len T=%d start=%d stride=%d: max |err| %.3g, bound %.3g" % (T, with_start, pstride, e, clearance_bound(M, inv_ss)))
        assert e <= clearance_bound(M, inv_ss)
    # NaN beyond a row's length changes nothing; a length outside 1 .. T is clamped on the device
    bad = np.where(np.arange(T)[None, None, :, None] < lens[None, :, None, None], fut, np.float32(np.nan))
    assert np.isnan(bad).any() and np.array_equal(run_clearance_len(obs, bad, lens, inv_ss, with_start), got)
    wild = lens.copy()
    wild[lens == 1], wild[lens == T] = -3, T + 50
    assert np.array_equal(run_clearance_len(obs, fut, wild, inv_ss, with_start), got)
    # the C entry with len = NULL is the dense launch
    scenes = ops.SceneIndex.get(scene_list(SC_SIZES), B, torch.device("cuda", 0))
    pos, clear = dev(fut), torch.empty(K, B, device="cuda")
    L.call("sw_scene_clearance_len", L.ptr(pos), 2, None, 0, L.ptr(scenes.scene_off), None, scenes.S, B, K, T, inv_ss, L.ptr(clear),
           L.stream())
    assert np.array_equal(clear.cpu().numpy(), run_clearance_len(obs, fut, None, inv_ss, False))


def test_stats_scene_clearance_len_is_the_public_form():
    from socialways_amd import stats
    obs, fut = scene_crowd(SC_SIZES, 3, seed=6)
    B, sb = fut.shape[1], scene_list(SC_SIZES)
    lens = mixed_lengths(B, seed=3)
    want = run_clearance_len(obs, fut, lens, 2.0, True)
    got = stats.scene_clearance_len(fut, sb, lens, start=obs[:, -1], scale=2.0)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(stats.scene_clearance_len(fut, sb, torch.from_numpy(lens), start=obs[:, -1], scale=2.0).cpu().numpy(), want)
    one = stats.scene_clearance_len(fut[1], sb, lens.tolist(), start=obs[:, -1], scale=2.0)
    assert one.shape == (B,) and np.array_equal(one.cpu().numpy(), want[1])
    assert np.array_equal(stats.scene_clearance_len(fut, sb, np.full(B, Tp)).cpu().numpy(), stats.scene_clearance(fut, sb).cpu().numpy())
    for bad in (lens[:-1], lens.astype(np.float32), np.where(lens == 1, 0, lens), np.where(lens == Tp, Tp + 1, lens)):
        with pytest.raises(ValueError, match="pred_len"):
            stats.scene_clearance_len(fut, sb, bad)


# ---- 3. evaluate*() on futures that end inside the horizon --------------------------------------------------------------------
@pytest.fixture(scope="module")
def short_eval(tmp_path_factory):
    """The synthetic recording: the model's coordinates are those of the full windows, the held-out set is EVERY window with a
    future of at least one frame (450 rows in 45 scenes, 254 of them short)."""
    import socialways_amd as sw
    from socialways_amd import data as D
    path = str(tmp_path_factory.mktemp("ragged_next") / "obsmat.txt")
    D.write_biwi_obsmat(path, *D.synth_crowd_frames())
    p_data, t_data, interval = D.parse_biwi(path)
    rng = range(int(t_data[0][0]), int(t_data[-1][-1]), interval)
    o0, p0, t0, b0 = D.create_dataset(p_data, t_data, rng)
    like = sw.SceneDataset(o0, p0, b0, t0, device="cuda:0")
    o, p, t, b, n, m = D.create_dataset_ragged(p_data, t_data, rng, min_past=8, min_next=1)
    data = sw.SceneDataset.held_out(like, o, p, b, t).set_pred_len(m)
    torch.manual_seed(8)
    tr = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0")
    tr.noise = sw.DeviceNoise(2025)
    return types.SimpleNamespace(data=data, tr=tr, like=like, arrays=(o, p, b, t), m=m, full=(o0, p0, b0, t0))


def per_agent_from_records(recs):
    """(N, 4) float64 = mean_k ADE | mean_k FDE | min_k ADE | min_k FDE over each row's valid frames, world units; lengths; M."""
    rows, lens, M = [], [], 0.0
    for r in recs:
        d = np.sqrt(((r["preds_our"].astype(np.float64) - r["preds_gtt"].astype(np.float64)[None]) ** 2).sum(-1))      # (K, n, Tp)
        M = max(M, float(np.abs(r["preds_our"]).max()))
        for a, j in enumerate(r["pred_len"]):
            ade, fde = d[:, a, :j].mean(1), d[:, a, j - 1]
            rows.append([ade.mean(), fde.mean(), ade.min(), fde.min()])
            lens.append(int(j))
    return np.asarray(rows), np.asarray(lens), M


def test_evaluate_and_horizon_on_short_futures(short_eval):
    import socialways_amd as sw
    s = short_eval
    data, tr, K = s.data, s.tr, 4
    assert data.n_test_samples == 450 and int((s.m < Tp).sum()) == 254 and data.n_train_samples == 0
    recs = []
    ev = tr.evaluate(data, n_gen_samples=K, collect=recs)
    assert tr.evaluate(data, n_gen_samples=K) == ev and all(np.isfinite(ev)) and min(ev) > 0
    assert len(recs) == len(data.test_batches)
    for r, (a, b) in zip(recs, data.test_batches):
        assert r["pred_len"].dtype == np.int32 and np.array_equal(r["pred_len"], s.m[a:b])
    rows, lens, M = per_agent_from_records(recs)
    assert np.array_equal(lens, s.m)
    for i, k in enumerate(KEYS):      # recomputed from denormalised positions: tests/test_gpu_scene.py's tolerance
        assert_close(ev[i], rows[:, i].sum() / data.n_test_samples, 1e-5, 32 * EPS * M, k)
    # the padding is not read: the same windows with NaN behind every row's last valid frame
    o, p, b, t = s.arrays
    hole = data.pred.clone()
    hole[torch.arange(Tp, device="cuda")[None, :] >= data.pred_len[:, None]] = float("nan")
    keep, data.pred = data.pred, hole
    try:
        assert tr.evaluate(data, n_gen_samples=K) == ev
    finally:
        data.pred = keep
    # the same rows scored over all 12 frames (no lengths) score the padding as truth: other numbers
    plain = sw.SceneDataset.held_out(s.like, o, p, b, t)
    assert plain.pred_len is None and tr.evaluate(plain, n_gen_samples=K) != ev

    hz = tr.evaluate_horizon(data, n_gen_samples=K)
    assert tuple(hz[k] for k in KEYS) == ev and hz["n_agents"] == 450
    by = hz["by_next"]
    want = {int(j): int(c) for j, c in enumerate(np.bincount(s.m, minlength=Tp + 1)) if c}
    assert {j: v["count"] for j, v in by.items()} == want and sorted(by) == list(range(1, Tp + 1))
    for i, k in enumerate(KEYS):
        total = sum(v["count"] * v[k] for v in by.values()) / data.n_test_samples
        assert abs(total - ev[i]) <= 1e-12 * abs(ev[i]), k
        for j, v in by.items():
            assert_close(v[k], rows[lens == j, i].mean(), 1e-5, 32 * EPS * M, "%s of length %d" % (k, j))
    for j, v in by.items():
        assert abs(v["ade_avg"] - v["fde_avg"]) <= 1e-12 if j == 1 else v["ade_avg"] != v["fde_avg"]
    # a row's share of its bucket depends on nothing but its own valid frames: give every other row another length and
    # another ground truth - bucket j keeps its bits
    for j in (1, 7, 12):
        mine = torch.from_numpy(s.m == j).cuda()
        other_len = torch.where(mine, data.pred_len, torch.full_like(data.pred_len, 3 if j != 3 else 4))
        other_gt = torch.where(mine[:, None, None], data.pred, data.pred.flip(0) + 0.25)
        keep_p, keep_l = data.pred, data.pred_len
        data.pred, data.pred_len = other_gt, other_len
        try:
            assert tr.evaluate_horizon(data, n_gen_samples=K)["by_next"][j] == by[j]
        finally:
            data.pred, data.pred_len = keep_p, keep_l
    one = tr.evaluate_horizon(data, n_gen_samples=K, just_one=True)
    a, b0 = data.test_batches[0]
    assert sum(v["count"] for v in one["by_next"].values()) == b0 - a
    hp = tr.evaluate_horizon(plain, n_gen_samples=K)      # a dataset without pred_len: the single bucket n_next
    assert list(hp["by_next"]) == [Tp] and hp["by_next"][Tp]["count"] == 450
    assert tuple(hp[k] for k in KEYS) == tr.evaluate(plain, n_gen_samples=K)


def test_evaluate_family_on_short_futures(short_eval):
    from socialways_amd import stats
    s = short_eval
    data, tr, K, coll = s.data, s.tr, 4, 0.3
    ev = tr.evaluate(data, n_gen_samples=K)
    recs = []
    sc = tr.evaluate_scenes(data, n_gen_samples=K, coll_dist=coll, collect=recs)
    rk = tr.evaluate_ranked(data, n_gen_samples=K, top_m=2)
    dv = tr.evaluate_diverse(data, n_gen_samples=K, top_m=2, radius=0.2)
    for out in (sc, rk, dv):
        assert tuple(out[k] for k in KEYS) == ev
    one = 1 + 4 * EPS
    assert sc["ade_min"] <= sc["jade_min"] * one and sc["jade_min"] <= sc["ade_avg"] * one
    assert rk["ade_min"] <= rk["ade_topm"] <= rk["ade_top1"]
    assert dv["ade_min"] <= dv["ade_divm"] <= dv["ade_div1"]
    # col_gt: the public length-aware clearance on the ground truth, scene by scene
    inv_ss = 1.0 / float(data.ss)
    gt_clear = stats.scene_clearance_len(data.pred, data.test_batches, data.pred_len, start=data.obsv[:, -1], scale=inv_ss).cpu().numpy()
    flags = [float(gt_clear[a:b].min() < np.float32(coll)) for a, b in data.test_batches if b - a > 1]
    assert sc["n_multi"] == len(flags) > 10 and sc["col_gt"] == float(np.mean(flags))
    dense_clear = stats.scene_clearance(data.pred, data.test_batches, start=data.obsv[:, -1], scale=inv_ss).cpu().numpy()
    assert (gt_clear >= dense_clear).all() and (gt_clear > dense_clear).any()      # fewer segments count, never more
    # the draws: every record's clearance is the length-aware kernel's on the record's own trajectories (world units)
    for r, (a, b) in zip(recs, data.test_batches):
        assert np.array_equal(r["pred_len"], s.m[a:b])
        if b - a > 1:
            M = max(float(np.abs(r["preds_our"]).max()), float(np.abs(r["obsvs"]).max()))
            want = clearance_len(r["obsvs"][:, -1], r["preds_our"], r["pred_len"], [b - a], 1.0)
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(r["clear"]), fin) and fin.all()      # with a start point every agent has a segment
            assert np.abs(r["clear"] - want).max() <= 32 * EPS * M
    # ranked: D scores the ground truth of the rows with a full future only
    full = data.pred_len == Tp
    assert rk["n_full"] == int(full.sum()) == 196 and rk["n_agents"] == 450
    import socialways_amd as sw
    gt4 = sw.get_traj_4d(data.obsv, data.pred)[1]
    score = tr.D.score_samples(data.obsv, gt4.unsqueeze(0))[0]      # one chunk in evaluate_ranked() too: the same launch
    want = float(score[0, full].double().sum()) / 196
    assert abs(rk["score_gt"] - want) <= 1e-12 * abs(want), (rk["score_gt"], want)
    none_full = sw.SceneDataset.held_out(s.like, *s.arrays).set_pred_len(np.minimum(s.m, Tp - 1))
    rk0 = tr.evaluate_ranked(none_full, n_gen_samples=K, top_m=2)
    assert rk0["n_full"] == 0 and rk0["score_gt"] == 0.0
    rcoll = []
    tr.evaluate_ranked(data, n_gen_samples=K, top_m=2, collect=rcoll)
    assert all("pred_len" in r and "score" in r for r in rcoll)


def test_full_length_pred_len_changes_no_evaluation_number(short_eval):
    import socialways_amd as sw
    s = short_eval
    tr = s.tr
    plain = sw.SceneDataset.held_out(s.like, *s.full)
    full = sw.SceneDataset.held_out(s.like, *s.full).set_pred_len(np.full(len(s.full[0]), Tp))
    assert plain.pred_len is None and full.pred_len is not None and plain.n_test_samples == 196

    def ranked(d):
        out = tr.evaluate_ranked(d, n_gen_samples=4, top_m=2)
        assert out.pop("n_full", 196) == 196 and ("n_full" in tr.evaluate_ranked(d, n_gen_samples=4, top_m=2)) == (d is full)
        return out
    for call in (lambda d: tr.evaluate(d, n_gen_samples=4), lambda d: tr.evaluate_scenes(d, n_gen_samples=4), ranked,
                 lambda d: tr.evaluate_diverse(d, n_gen_samples=4, top_m=2, radius=0.3),
                 lambda d: tr.evaluate_history(d, n_gen_samples=4), lambda d: tr.evaluate_horizon(d, n_gen_samples=4)):
        assert call(plain) == call(full)


def test_training_calls_refuse_short_futures_and_touch_nothing(short_eval):
    import socialways_amd as sw
    from socialways_amd import generic
    s = short_eval
    w0 = s.tr.G.encoder._flat.clone()
    for call in (lambda: s.tr.test(s.data, n_gen_samples=2), lambda: s.tr.train_epoch(s.data, 64),
                 lambda: s.tr.train_epoch_ragged(s.data, 64)):
        with pytest.raises(sw.SocialWaysHipError, match="pred_len"):
            call()
    assert torch.equal(s.tr.G.encoder._flat, w0)
    torch.manual_seed(1)
    wide = sw.SocialWaysTrainer(Tp, hidden_size=96, device="cuda:0")
    assert isinstance(wide, generic.GenericTrainer)
    for call in (lambda: wide.evaluate(s.data, n_gen_samples=2), lambda: wide.evaluate_scenes(s.data, n_gen_samples=2),
                 lambda: wide.evaluate_horizon(s.data, n_gen_samples=2)):
        with pytest.raises(sw.SocialWaysHipError, match="pred_len"):
            call()
