"""Scoring and ranking K sampled futures with the discriminator on the GPU: sw_disc_score against a float64 reference and,
bit for bit, against K calls of Discriminator.forward; sw_sample_rank against torch's stable sort on the same scores;
SocialWaysTrainer.evaluate_ranked() / sample_ranked() against the same quantities put together from public pieces
(eval_chunks, eval_noise, Generator.sample, K x Discriminator.forward, float64 torch ops).

Tolerances: scores against float64 as tests/test_gpu_disc_reference.py (OUT_RT, OUT_AT, the kink-margin seed rule); reduced
metrics against float64 rtol 1e-5 (tests/test_gpu_scene.py); identities between dict values rtol 1e-6 (the K = 1 identities
of evaluate_scenes); everything that is a selection or a count: exact."""
import numpy as np
import pytest
import torch

from test_gpu_disc_reference import _d64, _forward64, _pick, _images, _close_out, _disc, SEEDS, MARGIN, OUT_RT, OUT_AT  # noqa: F401
from test_gpu_sample import crowd, SIZES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- 1. scores against float64 -------------------------------------------------------------------------------------------
def _score_inputs(K, x_mode, To, Tp, B):
    def make(seed):
        g = torch.Generator().manual_seed(seed)
        if x_mode == 0:
            obsv = (torch.randn(B, To, 2, generator=g) * 0.1).cumsum(1)
        else:
            obsv = torch.randn(B, To, 4, generator=g) * 0.2
        return obsv, torch.randn(K, B, Tp, 4, generator=g) * 0.2
    return make


@pytest.mark.parametrize("K,x_mode,To,Tp,B,images", [
    (20, 0, 8, 12, 117, True), (3, 1, 2, 4, 15, False), (128, 0, 8, 12, 8, True), (5, 0, 5, 64, 33, False),
    (40, 0, 8, 12, 200, False), (1, 1, 1, 1, 1, True), (16, 0, 12, 32, 17, True)])
def test_scores_against_float64(K, x_mode, To, Tp, B, images):
    from socialways_amd import ops
    D = _disc(Tp)
    Dref = _d64(D)
    seed, (obsv, preds), margin = _pick(_score_inputs(K, x_mode, To, Tp, B),
                                        lambda inp: _forward64(Dref, inp[0], x_mode, list(inp[1]))[3])
    tag = "seed %d, kink margin %.2e (MARGIN %.1e)" % (seed, margin, MARGIN)
    with _images(D, images):
        score, code = ops.disc_score(D._flat, obsv.to(DEV), preds.to(DEV), K)
        torch.cuda.synchronize()
    assert score.shape == (K, B) and code.shape == (K, B, 2)
    rl, rc, _, _ = _forward64(Dref, obsv, x_mode, list(preds))      # one reference branch per draw
    print("K %d x_mode %d To %d Tp %d B %d: %s" % (K, x_mode, To, Tp, B, tag))
    _close_out(score, torch.stack([l[:, 0] for l in rl]), "score", "score", tag)
    _close_out(code, torch.stack(rc), "code", "score", tag)


# ---- 2. scores against forward(), bit for bit ------------------------------------------------------------------------------
def _forward_k(D, obsv4, preds):
    with torch.no_grad():
        outs = [D(obsv4, preds[k]) for k in range(preds.shape[0])]
    return torch.stack([l[:, 0] for l, _ in outs]), torch.stack([c for _, c in outs])


def _check_bits(D, obsv, preds, images):
    import socialways_amd as sw
    K, B = preds.shape[0], preds.shape[1]
    obsv4 = sw.get_traj_4d(obsv, []) if obsv.shape[2] == 2 else obsv
    with _images(D, images):
        score, code = D.score_samples(obsv, preds)
        want_s, want_c = _forward_k(D, obsv4, preds)
        torch.cuda.synchronize()
    assert score.shape == (K, B) and code.shape == (K, B, 2) and not score.requires_grad and not code.requires_grad
    assert torch.equal(score, want_s), "score: max |diff| %.3g" % float((score - want_s).abs().max())
    assert torch.equal(code, want_c), "code: max |diff| %.3g" % float((code - want_c).abs().max())
    assert float(score.abs().max()) > 0.0 and len(score.unique()) > K * B // 2
    return score, code


def _draws(K, B, Tp, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand(K, B, Tp, 4, device="cuda", generator=gen) - 0.5) * 0.4).contiguous()


@pytest.mark.parametrize("images", [False, True])
@pytest.mark.parametrize("K", [1, 3, 16, 20])
def test_scores_equal_forward_bit_for_bit(K, images):
    D = _disc(12)
    obsv, _, _ = crowd(SIZES)
    B = obsv.shape[0]
    assert B == 117 and B % 16 != 0
    score, code = _check_bits(D, obsv, _draws(K, B, 12, 7 + K), images)
    if K == 3:      # the 4-d observation is accepted as it is, and gives the same bits
        import socialways_amd as sw
        with _images(D, images):
            s4, c4 = D.score_samples(sw.get_traj_4d(obsv, []), _draws(K, B, 12, 7 + K))
        assert torch.equal(s4, score) and torch.equal(c4, code)


# (K, B, To, Tp, images): every k-grouping of the grid rule - groups of one draw pair bounded by K (one tile, K = 128: 64
# groups), tiles x K above the CU count (8 tiles x 100 draws: 32 groups of 3 or 4 draws, pairs with odd tails), more tiles
# than half the CUs (132 tiles: one group that walks all draws), a long horizon whose rows load in place
@pytest.mark.parametrize("K,B,To,Tp,images", [(128, 8, 8, 12, True), (128, 8, 8, 12, False), (100, 117, 8, 12, True),
                                              (3, 2100, 8, 12, False), (5, 2100, 3, 12, True), (7, 33, 5, 64, False),
                                              (4, 40, 8, 16, True)])
def test_scores_equal_forward_in_every_k_grouping(K, B, To, Tp, images):
    D = _disc(Tp)
    gen = torch.Generator(device="cuda").manual_seed(K + B)
    obsv = (torch.rand(B, To, 2, device="cuda", generator=gen) * 0.1 - 0.03).cumsum(1).contiguous()
    _check_bits(D, obsv, _draws(K, B, Tp, 5), images)


def test_scores_equal_forward_at_a_smaller_hidden_size():
    """32 units: the padded packed weights, like every other D kernel."""
    import socialways_amd as sw
    torch.manual_seed(5)
    D = sw.Discriminator(12, 32, 2, device=DEV)
    obsv, _, _ = crowd(SIZES)
    _check_bits(D, obsv, _draws(5, obsv.shape[0], 12, 3), False)


# ---- 3. ranking against torch on the same scores -----------------------------------------------------------------------------
def _rank_reference(score, M, err=None, best=None):
    """Stable descending sort over k, and per_agent from float64 torch ops on err / order."""
    order = torch.sort(score.t().contiguous(), dim=1, descending=True, stable=True)[1]       # (B, K)
    if err is None:
        return order[:, :M], None
    e = err.double().permute(1, 0, 2)                                                        # (B, K, 2)
    top = torch.gather(e, 1, order[:, :M, None].expand(-1, -1, 2))                           # (B, M, 2)
    rank = torch.zeros(score.shape[1], dtype=torch.float64, device=score.device)
    if best is not None:
        rank = (order == best.long()[:, None]).double().argmax(dim=1).double()
    return order[:, :M], torch.cat([top[:, 0], top.min(dim=1)[0], rank[:, None]], dim=1)


@pytest.mark.parametrize("K", [1, 2, 20, 128, 1000])
def test_ranking_against_torch_sort(K):
    from socialways_amd import ops
    B = 37
    gen = torch.Generator(device="cuda").manual_seed(K)
    for ties in (False, True):
        score = torch.randn(K, B, device="cuda", generator=gen)
        if ties:
            score = (score * 2).round() / 2            # a handful of distinct values: most draws tie with others
        err = torch.rand(K, B, 2, device="cuda", generator=gen)
        best = err[..., 0].argmin(dim=0).int()
        for M in sorted({m for m in (1, 5, K) if m <= K}):
            order, per_agent = ops.sample_rank(score, K, M, err=err, best=best)
            want_o, want_p = _rank_reference(score, M, err, best)
            assert order.shape == (B, M) and order.dtype == torch.int32 and per_agent.shape == (B, 5)
            assert torch.equal(order.long(), want_o), (K, M, ties)
            assert torch.equal(per_agent.double(), want_p), (K, M, ties)
            o2, p2 = ops.sample_rank(score, K, M, err=err, best=best)                  # two calls: the same bits
            assert torch.equal(o2, order) and torch.equal(p2, per_agent)
            o3, none = ops.sample_rank(score, K, M)                                    # order alone
            assert none is None and torch.equal(o3, order)
            o4, p4 = ops.sample_rank(score, K, M, err=err)                             # without best: column 4 is 0
            assert torch.equal(o4, order) and torch.equal(p4[:, :4], per_agent[:, :4]) and float(p4[:, 4].abs().max()) == 0.0
    if K > 2:
        assert float(per_agent[:, 4].max()) > 0.0


def test_ranking_ties_go_to_the_lowest_k():
    from socialways_amd import ops
    score = torch.tensor([0.1, 0.7, -0.3, 0.9, 0.2, 0.05, 0.6, 0.9, -1.0, 0.9 - 1e-7], device="cuda").view(10, 1).repeat(1, 3)
    score[:, 2] = 0.5                                   # an agent whose draws all tie: 0, 1, 2, ...
    err = torch.arange(20, dtype=torch.float32, device="cuda").view(10, 1, 2).repeat(1, 3, 1)
    best = torch.tensor([7, 3, 9], dtype=torch.int32, device="cuda")
    order, per_agent = ops.sample_rank(score, 10, 4, err=err, best=best)
    assert order[0].tolist() == [3, 7, 9, 1] and order[1].tolist() == [3, 7, 9, 1] and order[2].tolist() == [0, 1, 2, 3]
    assert per_agent[0].tolist() == [6.0, 7.0, 2.0, 3.0, 1.0]        # top 1 = draw 3; min over {3, 7, 9, 1} = draw 1; 7 is second
    assert per_agent[1].tolist() == [6.0, 7.0, 2.0, 3.0, 0.0]
    assert per_agent[2].tolist() == [0.0, 1.0, 0.0, 1.0, 9.0]


def test_rank_identities_per_agent():
    """ade_min <= ade_topm <= ade_top1 per agent; top_m = K gives the min-over-K columns of the sampling reduction, top_m = 1
    the top-1 columns, K = 1 the mean columns and rank 0: exactly."""
    import socialways_amd as sw
    from socialways_amd import ops
    from test_gpu_sample import sample_with_errors
    torch.manual_seed(4)
    D = sw.Discriminator(12, 64, 2, device=DEV)
    for K in (1, 20):
        pred4, (pa, best, err), gt, _ = sample_with_errors(True, K)
        obsv, _, _ = crowd(SIZES, seed=5)
        score, _ = ops.disc_score(D.packed(), obsv, pred4, K)
        _, full = ops.sample_rank(score, K, K, err=err, best=best)
        _, one = ops.sample_rank(score, K, 1, err=err, best=best)
        assert torch.equal(full[:, 2:4], pa[:, 2:4])
        assert torch.equal(one[:, 2:4], one[:, 0:2]) and torch.equal(one[:, 0:2], full[:, 0:2])
        if K == 1:
            assert torch.equal(full[:, 0:2], pa[:, 0:2]) and float(full[:, 4].abs().max()) == 0.0
        else:
            _, mid = ops.sample_rank(score, K, 5, err=err, best=best)
            assert bool((pa[:, 2] <= mid[:, 2]).all()) and bool((mid[:, 2] <= mid[:, 0]).all())
            assert bool((pa[:, 3] <= mid[:, 3]).all()) and bool((mid[:, 3] <= mid[:, 1]).all())
            assert torch.equal(mid[:, 4], full[:, 4]) and 0.0 < float(full[:, 4].mean()) < K - 1


# ---- 4. evaluate_ranked end to end -------------------------------------------------------------------------------------------
def _held_out():
    import socialways_amd as sw
    sizes = sw.ragged_scene_sizes(400, 8, seed=11) + [23, 1, 70, 6, 2, 17, 9, 1, 30]
    tracks = sw.synth_tracks(len(sizes), sizes, seed=99)
    data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], tracks["times"], device=DEV)
    assert len(data.test_batches) > 8
    return data


def _ranked_from_public_pieces(tr, data, K, M, just_one):
    """The new numbers of evaluate_ranked() without its kernels: float64 torch ops on the draws of Generator.sample and
    the scores of K calls of Discriminator.forward.  Consumes the host RNG exactly like evaluate()."""
    import socialways_amd as sw
    batches = [(int(b[0]), int(b[1])) for b in data.test_batches]
    if just_one:
        batches = batches[:1]
    acc = torch.zeros(8, dtype=torch.float64, device=DEV)
    n_seen, parts = 0, []
    for i, j in tr.eval_chunks(batches, K, tr.TEST_CHUNK):
        lo, hi = batches[i][0], batches[j - 1][1]
        obsv, pred = data.obsv[lo:hi], data.pred[lo:hi]
        n = hi - lo
        noise = tr.eval_noise(batches[i:j], K, tr.noise_len).to(DEV)
        sb = np.asarray([[a - lo, b - lo] for a, b in batches[i:j]], dtype=np.int64)
        ph = tr.G.sample(obsv, K, tr.n_next, sb, noise)
        o4, p4 = sw.get_traj_4d(obsv, pred)
        score, code = _forward_k(tr.D, o4, ph)
        with torch.no_grad():
            gt_score = tr.D(o4, p4)[0]
        e = ((ph[..., :2].double() - pred.double().unsqueeze(0)) / float(data.ss)).pow(2).sum(-1).sqrt()     # (K, n, Tp)
        err = torch.stack([e.mean(2), e[:, :, -1]], dim=2)                                                   # (K, n, 2)
        best = err[..., 0].argmin(dim=0)
        order, per_agent = _rank_reference(score, M, err, best)
        csq = (code.double() - noise[:, :, :2].double()).pow(2).mean(dim=2)
        acc += torch.cat([per_agent.sum(0), torch.stack([score.double().sum(), gt_score.double().sum(), csq.sum()])])
        n_seen += n
        parts.append((score, order, code))
    nt = data.n_test_samples
    div = torch.tensor([nt] * 5 + [K * nt, nt, K * nt], dtype=torch.float64, device=DEV)
    return (acc / div).tolist(), n_seen, parts


def _check_invariants(res):
    assert res["ade_min"] <= res["ade_topm"] <= res["ade_top1"] and res["fde_min"] <= res["fde_topm"] <= res["fde_top1"]
    assert 0.0 <= res["best_rank"] <= res["K"] - 1 and res["code_mse"] >= 0.0


@pytest.mark.parametrize("K,M,just_one,chunk", [(20, 5, False, None), (20, 5, False, 700), (128, 5, True, None)])
def test_evaluate_ranked_end_to_end(K, M, just_one, chunk):
    import socialways_amd as sw
    data = _held_out()
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    if chunk:
        tr.TEST_CHUNK = chunk
        assert len(list(tr.eval_chunks([(int(a), int(b)) for a, b in data.test_batches], K, chunk))) > 2
    torch.manual_seed(31)
    want4 = tr.evaluate(data, n_gen_samples=K, just_one=just_one)
    state = torch.get_rng_state()
    torch.manual_seed(31)
    coll = []
    res = tr.evaluate_ranked(data, n_gen_samples=K, top_m=M, just_one=just_one, collect=coll)
    assert torch.equal(torch.get_rng_state(), state)
    assert sorted(res) == sorted(("ade_avg", "fde_avg", "ade_min", "fde_min") + tr.RANKED_KEYS + ("n_agents", "K", "top_m"))
    assert (res["ade_avg"], res["fde_avg"], res["ade_min"], res["fde_min"]) == tuple(want4)       # Python floats, ==
    assert res["K"] == K and res["top_m"] == M
    torch.manual_seed(31)
    want, n_seen, parts = _ranked_from_public_pieces(tr, data, K, M, just_one)
    assert res["n_agents"] == n_seen
    for key, w in zip(tr.RANKED_KEYS, want):
        print("%-12s evaluate_ranked %.9g   public pieces %.9g" % (key, res[key], w))
    for key, w in zip(tr.RANKED_KEYS, want):
        assert abs(res[key] - w) <= 1e-5 * abs(w), (key, res[key], w)
    _check_invariants(res)
    assert res["score_draws"] != res["score_gt"]
    # collect: evaluate()'s records plus score, order, code_hat; without collect the same numbers
    n_rec = 1 if just_one else len(data.test_batches)
    assert len(coll) == n_rec
    score = torch.cat([p[0] for p in parts], dim=1).cpu().numpy()
    order = torch.cat([p[1] for p in parts], dim=0).cpu().numpy()
    code = torch.cat([p[2] for p in parts], dim=1).cpu().numpy()
    row = 0
    for rec in coll:
        n = rec["obsvs"].shape[0]
        assert rec["preds_our"].shape[:2] == (K, n)
        assert np.array_equal(rec["score"], score[:, row:row + n]) and np.array_equal(rec["order"], order[row:row + n])
        assert np.array_equal(rec["code_hat"], code[:, row:row + n]) and rec["order"].shape == (n, M)
        row += n
    assert row == n_seen
    torch.manual_seed(31)
    assert tr.evaluate_ranked(data, n_gen_samples=K, top_m=M, just_one=just_one) == res
    # top_m = K: the minimum over all draws; top_m = 1: the top-scored draw
    torch.manual_seed(31)
    full = tr.evaluate_ranked(data, n_gen_samples=K, top_m=K, just_one=just_one)
    torch.manual_seed(31)
    one = tr.evaluate_ranked(data, n_gen_samples=K, top_m=1, just_one=just_one)
    for a, b in (("ade_topm", "ade_min"), ("fde_topm", "fde_min")):
        assert abs(full[a] - full[b]) <= 1e-6 * abs(full[b]), (a, full[a], full[b])
    for a, b in (("ade_topm", "ade_top1"), ("fde_topm", "fde_top1")):
        assert abs(one[a] - one[b]) <= 1e-6 * abs(one[b]), (a, one[a], one[b])
    for key in ("ade_top1", "fde_top1", "best_rank", "score_draws", "score_gt", "code_mse"):
        assert full[key] == res[key] == one[key], key
    with pytest.raises(ValueError):
        tr.evaluate_ranked(data, n_gen_samples=K, top_m=K + 1)
    with pytest.raises(ValueError):
        tr.evaluate_ranked(data, n_gen_samples=K, top_m=0)


def test_evaluate_ranked_with_one_draw():
    import socialways_amd as sw
    data = _held_out()
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    torch.manual_seed(31)
    res = tr.evaluate_ranked(data, n_gen_samples=1, top_m=1)
    assert res["best_rank"] == 0.0
    for a, b in (("ade_top1", "ade_avg"), ("fde_top1", "fde_avg"), ("ade_topm", "ade_min"), ("fde_topm", "fde_min")):
        assert abs(res[a] - res[b]) <= 1e-6 * abs(res[b]), (a, res[a], res[b])


@pytest.mark.parametrize("hidden,codes", [(80, 3), (128, 2)])
def test_evaluate_ranked_at_a_generic_width(hidden, codes):
    """80 units, 3 latent codes (the layer-by-layer path) and 128 units (the wide path, which inherits it): scores from their
    own Discriminator.forward, ranking and reduction from the kernels."""
    import socialways_amd as sw
    from socialways_amd import generic
    sizes = sw.ragged_scene_sizes(40, 6, seed=3)
    tracks = sw.synth_tracks(len(sizes), sizes, seed=7)
    data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], tracks["times"], device=DEV)
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, hidden_size=hidden, n_latent_codes=codes, use_social=True, device=DEV)
    assert isinstance(tr, generic.GenericTrainer)
    K, M = 6, 2
    torch.manual_seed(31)
    coll = []
    res = tr.evaluate_ranked(data, n_gen_samples=K, top_m=M, collect=coll)
    assert sorted(res) == sorted(("ade_avg", "fde_avg", "ade_min", "fde_min") + sw.SocialWaysTrainer.RANKED_KEYS
                                 + ("n_agents", "K", "top_m"))
    _check_invariants(res)
    assert all(np.isfinite(v) for v in res.values()) and res["n_agents"] == sum(int(b - a) for a, b in data.test_batches)
    for rec in coll:
        n = rec["obsvs"].shape[0]
        assert rec["score"].shape == (K, n) and rec["order"].shape == (n, M) and rec["code_hat"].shape == (K, n, codes)
        assert (np.diff(np.take_along_axis(rec["score"], rec["order"].T.astype(np.int64), axis=0), axis=0) <= 0).all()
    torch.manual_seed(31)
    full = tr.evaluate_ranked(data, n_gen_samples=K, top_m=K)
    assert abs(full["ade_topm"] - full["ade_min"]) <= 1e-6 * full["ade_min"]
    a, b = (int(x) for x in data.test_batches[0])
    trajs, score, order = tr.sample_ranked(data.obsv[a:b], K, M)
    assert trajs.shape == (M, b - a, 12, 4) and score.shape == (M, b - a) and order.shape == (b - a, M)
    assert bool((score[1:] <= score[:-1]).all())


# ---- 5. sample_ranked ----------------------------------------------------------------------------------------------------------
def test_sample_ranked_returns_the_top_scored_draws():
    import socialways_amd as sw
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    obsv, _, sb = crowd(SIZES)
    K, M, B = 20, 5, obsv.shape[0]
    noise = torch.rand(K, B, 32, device="cuda")
    trajs, score, order = tr.sample_ranked(obsv, K, M, sb, noise)
    assert trajs.shape == (M, B, 12, 4) and score.shape == (M, B) and order.shape == (B, M) and order.dtype == torch.int32
    assert not trajs.requires_grad
    draws = tr.G.sample(obsv, K, 12, sb, noise)
    all_scores, _ = tr.D.score_samples(obsv, draws)
    ar = torch.arange(B, device="cuda")
    for m in range(M):
        assert torch.equal(trajs[m], draws[order[:, m].long(), ar]), m
        assert torch.equal(score[m], all_scores[order[:, m].long(), ar]), m
    assert bool((score[1:] <= score[:-1]).all())
    assert torch.equal(order.long(), torch.sort(all_scores.t().contiguous(), dim=1, descending=True, stable=True)[1][:, :M])
    assert len(order[:, 0].unique()) > 1
    t2, s2, o2 = tr.sample_ranked(obsv, K, K, sb, noise)           # top_m = K: every draw, sorted
    assert torch.equal(o2[:, :M], order) and torch.equal(t2[:M], trajs) and sorted(o2[0].tolist()) == list(range(K))
    assert tr.sample_ranked(obsv, K, 2, sb)[0].shape == (2, B, 12, 4)      # noise drawn on the device
    for bad in (0, K + 1):
        with pytest.raises(ValueError):
            tr.sample_ranked(obsv, K, bad, sb, noise)


# ---- 6. argument checks with a device ----------------------------------------------------------------------------------------
def test_c_abi_edges_on_the_device():
    from socialways_amd import _lib as L, ops
    lib = L.load()
    B, K, To, Tp = 21, 6, 8, 12
    D = _disc(Tp)
    t = lambda *s: torch.full(s, 7.0, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    obsv = torch.rand(B, To, 2, device="cuda", generator=gen).cumsum(1).contiguous()
    pred4 = _draws(K, B, Tp, 2)
    score, code = t(K, B), t(K, B, 2)
    p, st = L.ptr, L.stream()
    # B == 0: SW_OK, nothing launched
    assert lib.sw_disc_score(p(obsv), To, 0, p(pred4), p(D._flat), 0, K, Tp, p(score), p(code), st) == 0
    order, pa = torch.full((B, K), 7, dtype=torch.int32, device="cuda"), t(B, 5)
    assert lib.sw_sample_rank(p(score), None, None, 0, K, K, p(order), None, st) == 0
    torch.cuda.synchronize()
    assert float(score.min()) == 7.0 and float(code.max()) == 7.0 and int(order.min()) == 7
    s0, c0 = ops.disc_score(D._flat, obsv[:0], pred4[:, :0], K)
    assert s0.shape == (K, 0) and c0.shape == (K, 0, 2)
    assert ops.sample_rank(s0, K, 2)[0].shape == (0, 2)
    # code == NULL: the scores alone, the same bits
    want_s, want_c = ops.disc_score(D._flat, obsv, pred4, K)
    assert lib.sw_disc_score(p(obsv), To, 0, p(pred4), p(D._flat), B, K, Tp, p(score), None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(score, want_s) and float(code.min()) == 7.0 and float(code.max()) == 7.0
    only, none = ops.disc_score(D._flat, obsv, pred4, K, want_code=False)
    assert none is None and torch.equal(only, want_s)
    # M == K: a permutation of the draws per agent; M > K is refused
    assert lib.sw_sample_rank(p(score), None, None, B, K, K, p(order), None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(order.long().sort(dim=1)[0], torch.arange(K, device="cuda").expand(B, K))
    assert lib.sw_sample_rank(p(score), None, None, B, K, K + 1, p(order), None, st) == -1
    assert lib.sw_sample_rank(p(score), None, None, B, K, K, p(order), p(pa), st) == -1        # per_agent needs err
    assert lib.sw_disc_score(p(obsv), To, 0, p(pred4), p(D._flat), B, K, 65, p(score), None, st) == -2
    assert lib.sw_disc_score(p(obsv), 1, 0, p(pred4), p(D._flat), B, K, Tp, p(score), None, st) == -1
    torch.cuda.synchronize()
    assert float(pa.min()) == 7.0
