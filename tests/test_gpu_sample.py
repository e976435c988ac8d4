"""K-sample inference on the GPU: Generator.sample() / ops.gen_sample (one encoding, one sampling launch for K * B rows,
best-of-K reduction on the device) and SocialWaysTrainer.evaluate() against replication through forward(), the
reference's recorded samples and test()."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _util import golden, state_from, as_checkpoint, dataset_from, assert_close

pytestmark = pytest.mark.gpu

RT, AT = 2e-5, 2e-6       # tests/test_gpu_kernels.py: pred_hat_4d against the reference
SIZES = [1, 5, 17, 8, 3, 70, 1, 12]       # ragged scenes: single agents, above one 16-row tile, above 64 agents; 117 agents
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scene_list(sizes):
    ends = np.cumsum(sizes)
    return np.stack([ends - np.asarray(sizes), ends], axis=1).astype(np.int64)


def crowd(sizes, To=8, Tp=12, seed=3):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    B = int(np.sum(sizes))
    obsv = (torch.rand(B, To, 2, device="cuda", generator=gen) * 0.1 - 0.03).cumsum(1).contiguous()
    gt = (obsv[:, -1:] + (torch.rand(B, Tp, 2, device="cuda", generator=gen) * 0.1 - 0.03).cumsum(1)).contiguous()
    return obsv, gt, scene_list(sizes)


def replicated(G, obsv, noise, Tp, sb):
    """K copies of the batch through forward(), each copy with its own scenes: what test() launches."""
    K, B = noise.shape[0], obsv.shape[0]
    sbk = np.concatenate([sb + k * B for k in range(K)]) if len(sb) else np.asarray([[k * B, (k + 1) * B] for k in range(K)])
    with torch.no_grad():
        return G(obsv.repeat(K, 1, 1), noise.reshape(K * B, -1), Tp, sbk).view(K, B, Tp, 4)


@pytest.mark.parametrize("K", [1, 3, 16, 20])
@pytest.mark.parametrize("social", [False, True])
def test_sample_equals_replicated_forward_bit_for_bit(social, K):
    import socialways_amd as sw
    torch.manual_seed(0)
    G = sw.Generator(use_social=social, device="cuda:0")
    obsv, _, sb = crowd(SIZES)
    B, Tp = obsv.shape[0], 12
    assert B % 16 != 0
    noise = torch.rand(K, B, 32, device="cuda")
    got = G.sample(obsv, K, Tp, sb, noise)
    assert got.shape == (K, B, Tp, 4) and not got.requires_grad
    want = replicated(G, obsv, noise, Tp, sb)
    assert torch.equal(got, want), "max |diff| %.3g" % float((got - want).abs().max())
    assert float(got.abs().max()) > 0.0
    assert torch.equal(sw.sample(obsv, K, Tp, sb, noise, generator=G), got)
    if K == 3:      # the default noise is drawn on the device, and shapes are checked
        a = G.sample(obsv, K, Tp, sb)
        assert a.shape == (K, B, Tp, 4) and a.is_cuda and not torch.equal(a[0], a[1])
        for bad in (noise[:2], noise[:, :5], noise[:, :, :7], noise[0]):
            with pytest.raises(ValueError):
                G.sample(obsv, K, Tp, sb, bad)
        with pytest.raises(ValueError):
            G.sample(obsv, 0, Tp, sb)


_TILE_SNIPPET = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import socialways_amd as sw
from test_gpu_sample import SIZES, crowd, replicated
torch.manual_seed(0)
G = sw.Generator(use_social=True, device="cuda:0")
obsv, _, sb = crowd(SIZES)
K, B = 40, obsv.shape[0]
assert K * B > 256 * 16
noise = torch.rand(K, B, 32, device="cuda")
torch.save({"sample": G.sample(obsv, K, 12, sb, noise).cpu(), "replicated": replicated(G, obsv, noise, 12, sb).cpu()}, sys.argv[2])
'''


def test_sample_above_256_tiles_in_both_tile_forms(tmp_path):
    """K * B > 256 * 16 rows: the sampling launch takes the two-tile body (its images are registered); SW_DEC_FWD2=0
    forces one tile per workgroup.  The switch is read once per process: two child processes."""
    res = {}
    for v in (None, "0"):
        f = str(tmp_path / ("tiles_%s.pt" % v))
        env = {k: x for k, x in os.environ.items() if k != "SW_DEC_FWD2"}
        if v is not None:
            env["SW_DEC_FWD2"] = v
        p = subprocess.run([sys.executable, "-c", _TILE_SNIPPET, ROOT, f], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        res[v] = torch.load(f)
    assert torch.equal(res[None]["sample"], res["0"]["sample"])
    for v in res:
        assert torch.equal(res[v]["sample"], res[v]["replicated"]), v
    assert float(res["0"]["sample"].abs().max()) > 0.0


def eval_golden():
    import socialways_amd as sw
    g = golden("test_eval")
    ds = dataset_from(g)
    data = sw.SceneDataset(ds["obsvs"], ds["preds"], ds["batches"], g["ds.times"], device="cuda:0")
    tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0")
    tr.load_checkpoint(as_checkpoint(state_from(g, "w0.")))
    return g, data, tr


def test_sample_reproduces_the_reference_samples():
    """tests/golden/test_eval.npz: per held-out scene s and draw k the reference's noise and pred_hat (its test() calls
    predict() without sub_batches: one scene)."""
    g, data, tr = eval_golden()
    K = 4
    assert len(data.test_batches) > 0
    for s, (a, b) in enumerate(data.test_batches):
        noise = torch.from_numpy(np.stack([g["noise.%d.%d" % (s, k)] for k in range(K)])).cuda()
        got = tr.G.sample(data.obsv[a:b], K, 12, [], noise).cpu().numpy()
        for k in range(K):
            assert_close(got[k], g["pred_hat.%d.%d" % (s, k)], RT, AT, "scene %d draw %d" % (s, k))


def sample_with_errors(social, K, noise=None, want_pred=True, inv_ss=0.7):
    import socialways_amd as sw
    from socialways_amd import ops
    torch.manual_seed(1)
    G = sw.Generator(use_social=social, device="cuda:0")
    obsv, gt, sb = crowd(SIZES, seed=5)
    B = obsv.shape[0]
    if noise is None:
        noise = torch.rand(K, B, 32, device="cuda")
    scenes = ops.SceneIndex.get(sb, B, obsv.device)
    pred4, red = ops.gen_sample(G.encoder.packed(), G.feature_embedder.packed(), G.attention.packed(), G.decoder.packed(), obsv,
                                noise.reshape(K * B, 32), scenes, 12, social, K, gt=gt, inv_ss=inv_ss, want_pred=want_pred)
    return pred4, red, gt, noise


def reduce_in_torch(err):
    """The kernel's stated order: k ascending, s = s + e_k in fp32, then s / K; strict < keeps the lowest k on ties."""
    K = err.shape[0]
    s, m, best = err[0].clone(), err[0].clone(), torch.zeros(err.shape[1], dtype=torch.int32, device=err.device)
    for k in range(1, K):
        s = s + err[k]
        lower = err[k, :, 0] < m[:, 0]
        best = torch.where(lower, torch.full_like(best, k), best)
        m = torch.minimum(m, err[k])
    return torch.cat([s / K, m], dim=1), best


@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("social", [False, True])
def test_row_errors_and_best_of_k_reduction(social, K):
    pred4, (per_agent, best, err), gt, _ = sample_with_errors(social, K)
    B, Tp = gt.shape[0], gt.shape[1]
    assert err.shape == (K, B, 2) and per_agent.shape == (B, 4) and best.shape == (B,) and best.dtype == torch.int32
    e = (((pred4.view(K, B, Tp, 4)[..., :2] - gt.unsqueeze(0)) * 0.7) ** 2).sum(-1).sqrt()
    assert_close(err[..., 0].cpu(), e.mean(2).cpu(), RT, AT, "per-row ADE")
    assert_close(err[..., 1].cpu(), e[:, :, -1].cpu(), RT, AT, "per-row FDE")
    want, want_best = reduce_in_torch(err)
    assert torch.equal(per_agent[:, 2:], want[:, 2:]) and torch.equal(best, want_best)
    assert_close(per_agent[:, :2].cpu(), want[:, :2].cpu(), 1e-6, 0.0, "mean over k")
    if K > 1:
        assert len(best.unique()) > 1


def test_best_of_k_ties_go_to_the_lowest_k():
    torch.manual_seed(7)
    B = int(np.sum(SIZES))
    row = torch.rand(1, B, 32, device="cuda")
    _, (per_agent, best, err), _, _ = sample_with_errors(True, 3, noise=row.repeat(3, 1, 1))
    assert torch.equal(err[0], err[1]) and torch.equal(err[0], err[2])
    assert int(best.abs().max()) == 0
    assert torch.equal(per_agent[:, 2:], err[0])
    other = torch.rand(1, B, 32, device="cuda")
    _, (_, best, err), _, _ = sample_with_errors(True, 3, noise=torch.cat([other, row, row]))
    assert torch.equal(err[1], err[2]) and int(best.max()) == 1 and int(best.min()) == 0


@pytest.mark.parametrize("social", [False, True])
def test_metrics_only_mode_gives_the_same_errors(social):
    pred4, (pa, best, err), _, noise = sample_with_errors(social, 5)
    none, (pa2, best2, err2), _, _ = sample_with_errors(social, 5, noise=noise, want_pred=False)
    assert none is None and pred4 is not None
    assert torch.equal(err, err2) and torch.equal(pa, pa2) and torch.equal(best, best2)


def test_evaluate_metrics_and_prediction_files_against_the_reference(tmp_path):
    """The assertions of test_gpu_trainer.test_test_eval_and_prediction_npz on evaluate()."""
    g, data, tr = eval_golden()
    tr.epoch = 1
    torch.manual_seed(123)
    coll = []
    metrics = tr.evaluate(data, n_gen_samples=4, write_to_file=str(tmp_path), collect=coll)
    assert_close(np.asarray(metrics), g["metrics"], 2e-5, 2e-6, "evaluate() metrics [ade_avg, fde_avg, ade_min, fde_min]")
    files = sorted(p.name for p in tmp_path.glob("*.npz"))
    assert files == sorted(str(f) for f in g["npz_files"])
    assert len(coll) == len(files)
    for f in files:
        z = np.load(tmp_path / f)
        assert sorted(z.files) == ["obsvs", "preds_gtt", "preds_lnr", "preds_our", "timestamp"]
        for k in ("obsvs", "preds_our", "preds_gtt", "preds_lnr"):
            assert_close(z[k], g["npz.%s.%s" % (f[:-4], k)], 1e-5, 1e-5, f + ":" + k)
    torch.manual_seed(123)      # metrics only: nothing written, same numbers
    assert tr.evaluate(data, n_gen_samples=4) == metrics


@pytest.mark.parametrize("K,just_one,chunk", [(20, False, None), (20, False, 700), (128, True, None)])
def test_evaluate_equals_test(K, just_one, chunk):
    """Same seed, ragged multi-scene held-out set: the metrics of test() and its collected samples (chunk: a smaller
    TEST_CHUNK so that the scenes fold into several launches)."""
    import socialways_amd as sw
    sizes = sw.ragged_scene_sizes(400, 8, seed=11) + [23, 1, 70, 6, 2, 17, 9, 1, 30]
    tracks = sw.synth_tracks(len(sizes), sizes, seed=99)
    data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], tracks["times"], device="cuda:0")
    assert len(data.test_batches) > 8
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0")
    if chunk:
        tr.TEST_CHUNK = chunk
    torch.manual_seed(31)
    ca, cb = [], []
    want = tr.test(data, n_gen_samples=K, just_one=just_one, collect=ca)
    state = torch.get_rng_state()
    torch.manual_seed(31)
    got = tr.evaluate(data, n_gen_samples=K, just_one=just_one, collect=cb)
    assert torch.equal(torch.get_rng_state(), state)
    assert_close(np.asarray(got), np.asarray(want), 2e-5, 2e-6, "evaluate() vs test()")
    assert len(ca) == len(cb) == (1 if just_one else len(data.test_batches))
    for ra, rb in zip(ca, cb):
        assert ra["timestamp"] == rb["timestamp"] and ra["preds_our"].shape[0] == K
        for k in ("obsvs", "preds_our", "preds_gtt", "preds_lnr"):
            assert np.array_equal(ra[k], rb[k]), k
    torch.manual_seed(31)
    assert_close(np.asarray(tr.evaluate(data, n_gen_samples=K, just_one=just_one)), np.asarray(want), 2e-5, 2e-6, "metrics only")


def test_c_abi_argument_checks():
    from socialways_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "sw_dec_sample_fwd") and hasattr(lib, "sw_sample_reduce")
    B, K, To, Tp = 5, 3, 8, 12
    t = lambda *s: torch.full(s, 7.0, device="cuda")
    obsv, z, S, hT, cT, gt = t(B, To, 2), t(K * B, 32), t(B, 64), t(B, 64), t(B, 64), t(B, Tp, 2)
    pred4, err, pa = t(K * B, Tp, 4), t(K, B, 2), t(B, 4)
    enc, dec = t(lib.sw_param_count(L.GRP_ENC, Tp)), t(lib.sw_param_count(L.GRP_DEC, Tp))
    p, st = L.ptr, L.stream()

    def fwd(obsv=obsv, To=To, z=z, hT=hT, cT=cT, enc=enc, dec=dec, B=B, K=K, Tp=Tp, pred4=pred4, gt=gt, err=err):
        return lib.sw_dec_sample_fwd(p(obsv), To, p(z), p(S), p(hT), p(cT), p(enc), p(dec), B, K, Tp, p(pred4), p(gt), 1.0,
                                     p(err), st)
    EARG = -1
    for kw in (dict(obsv=None), dict(z=None), dict(hT=None), dict(cT=None), dict(enc=None), dict(dec=None), dict(B=-1),
               dict(K=0), dict(K=-2), dict(To=1), dict(Tp=0), dict(pred4=None, err=None), dict(gt=None)):
        assert fwd(**kw) == EARG, kw
    assert fwd(B=0) == 0
    assert lib.sw_sample_reduce(None, B, K, p(pa), None, st) == EARG
    assert lib.sw_sample_reduce(p(err), B, K, None, None, st) == EARG
    assert lib.sw_sample_reduce(p(err), -1, K, p(pa), None, st) == EARG
    assert lib.sw_sample_reduce(p(err), B, 0, p(pa), None, st) == EARG
    assert lib.sw_sample_reduce(p(err), 0, K, p(pa), None, st) == 0
    torch.cuda.synchronize()
    for out in (pred4, err, pa):      # nothing was launched
        assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    assert lib.sw_sample_reduce(p(err), B, K, p(pa), None, st) == 0       # best may be NULL
    torch.cuda.synchronize()
    assert torch.equal(pa, t(B, 4))


def test_wide_generator_sample_equals_replicated_forward():
    from socialways_amd import generic
    torch.manual_seed(0)
    G = generic.Generator(128, use_social=True, device="cuda:0")
    sizes = [1, 5, 17, 8]
    obsv, _, sb = crowd(sizes)
    K, B = 3, obsv.shape[0]
    noise = torch.rand(K, B, G.noise_len, device="cuda")
    got = G.sample(obsv, K, 12, sb, noise)
    assert got.shape == (K, B, 12, 4) and not got.requires_grad
    assert torch.equal(got, replicated(G, obsv, noise, 12, sb))
    with pytest.raises(ValueError):
        G.sample(obsv, K, 12, sb, noise[:, :, :5])
