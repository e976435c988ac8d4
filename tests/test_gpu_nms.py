"""The diverse top-M selection on the GPU: sw_sample_nms against a float64 numpy implementation of its definition
(include/socialways_hip.h) that sees nothing of the device but inputs and outputs - on constructed draws whose every
comparison is far from rounding (all outputs exact), on a trainer's real draws with a radius placed in the widest gap of the
pair distances - and SocialWaysTrainer.evaluate_diverse() / sample_diverse() against the same quantities put together from
public pieces.

Tolerances: constructed inputs - everything bit for bit.  Real draws - order, count and the assignment of suppressed draws
exact given the asserted gap around the radius (half the gap >= 1e-5 of the radius; an fp32 distance is off by a few 1e-7
of itself); a leftover draw may take any pick within a factor 1 + 1e-5 of its nearest.  The float64-summed means of
evaluate_diverse against the public pieces: rtol 1e-5, the practice of tests/test_gpu_rank.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- the reference: the definition, float64 numpy --------------------------------------------------------------------------
def pair_dist(pos, c, metric, inv_ss=1.0):
    """d_a(k, c) for every draw k and row a: (K, B) float64.  pos (K, B, Tp, >= 2)."""
    p = np.asarray(pos, dtype=np.float64)[..., :2]
    d = np.sqrt(((p - p[c][None]) ** 2).sum(-1))                       # (K, B, Tp)
    return inv_ss * (d[..., -1] if metric == "fde" else d.mean(-1))


def nms_reference(pos, score, groups, M, radius, metric, inv_ss=1.0, err=None, best=None, slack=None):
    """order (G, M), count (G,), weight (G, M) float64, assign (G, K), per_row (B, 6) or None.  slack: a list that receives,
    for every leftover draw, (group, k, its float64 distances to the picks)."""
    score = np.asarray(score, dtype=np.float64)
    K, B = score.shape
    G = len(groups)
    order, count = -np.ones((G, M), dtype=np.int64), np.zeros(G, dtype=np.int64)
    weight, assign = np.zeros((G, M)), -np.ones((G, K), dtype=np.int64)
    per_row = None if err is None else np.zeros((B, 6))
    for g, (a, b) in enumerate(groups):
        s = score[:, a:b].min(axis=1)
        alive, cols = np.ones(K, dtype=bool), []
        for m in range(M):
            if not alive.any():
                break
            cand = np.nonzero(alive)[0]
            c = int(cand[np.argmax(s[cand])])                          # the first maximum: the lowest k
            D = pair_dist(pos[:, a:b], c, metric, inv_ss).max(axis=1)
            gone = alive & (D <= radius)
            assert gone[c]
            order[g, m], assign[g, gone] = c, m
            alive &= ~gone
            cols.append(D)
        count[g] = len(cols)
        for k in np.nonzero(alive)[0]:
            d = np.array([D[k] for D in cols])
            assign[g, k] = int(np.argmin(d))                           # the first minimum: the lowest m
            if slack is not None:
                slack.append((g, int(k), d))
        weight[g, :count[g]] = np.bincount(assign[g], minlength=M)[:count[g]] / K
        if err is not None:
            e = np.asarray(err, dtype=np.float64)[:, a:b]              # (K, n, 2)
            picks = order[g, :count[g]]
            per_row[a:b, 0:2] = e[picks[0]]
            per_row[a:b, 2:4] = e[picks].min(axis=0)
            if best is not None:
                mb = assign[g, np.asarray(best)[a:b]]
                per_row[a:b, 4], per_row[a:b, 5] = weight[g, mb], mb
    return order, count, weight, assign, per_row


def run_kernel(pos, score, K, M, radius, metric, groups=None, inv_ss=1.0, err=None, best=None):
    from socialways_amd import ops
    B = score.shape[1]
    scenes = ops.SceneIndex.get(np.asarray(groups, dtype=np.int64), B, torch.device(DEV)) if groups is not None else None
    t = lambda x, dt=torch.float32: None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(DEV)
    out = ops.sample_nms(t(pos), t(score), K, M, radius, metric, scenes, inv_ss, t(err), t(best, torch.int32))
    torch.cuda.synchronize()
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.int32 and out[3].dtype == torch.int32
    G = B if groups is None else len(groups)
    assert out[0].shape == (G, M) and out[1].shape == (G,) and out[2].shape == (G, M) and out[3].shape == (G, K)
    return [None if o is None else o.cpu().numpy() for o in out]


def assert_exact(got, want, tag):
    order, count, weight, assign, per_row = got
    w_order, w_count, w_weight, w_assign, w_per_row = want
    assert np.array_equal(count, w_count), (tag, count, w_count)
    assert np.array_equal(order, w_order), (tag, order, w_order)
    assert np.array_equal(assign, w_assign), tag
    assert np.array_equal(weight, w_weight.astype(np.float32)), tag      # an integer over K: one rounding, the same one
    assert np.array_equal(weight.astype(np.float64).sum(axis=1).round(6), np.ones(len(count))), tag
    if w_per_row is not None:
        assert np.array_equal(per_row, w_per_row.astype(np.float32)), (tag, per_row, w_per_row)


# ---- constructed draws: clusters on multiples of 8, jitter in 1/64 steps within +-0.25, radius 1 ----------------------------
CENTRES = 8.0 * np.array([[0, 0], [1, 0], [3, 0], [7, 0], [15, 0]])      # on a line: the ten gaps between two of them are all distinct


def clustered(K, B, Tp, pstride, n_cl, seed, per_group=None):
    """pos (K, B, Tp, pstride) float32, cluster (K, B).  per_group [(a, b)]: the rows of a group share their draw's cluster
    except a fifth of the (draw, row) pairs, which sit in the next one: joint modes are tuples of clusters."""
    rng = np.random.default_rng(seed)
    cl = rng.integers(0, n_cl, size=(K, B))
    cl[:min(K, n_cl), :] = np.arange(min(K, n_cl))[:, None]            # every cluster has a draw where K allows
    cl = cl[rng.permutation(K)]
    if per_group is not None:
        for a, b in per_group:
            cl[:, a:b] = cl[:, a:a + 1]
        cl = np.where(rng.random((K, B)) < 0.2, (cl + 1) % n_cl, cl)
    jit = rng.integers(-16, 17, size=(K, B, Tp, 2)) / 64.0
    drift = np.arange(Tp)[None, None, :, None] * 0.5                   # a common motion: the clusters keep their distance
    pos = np.zeros((K, B, Tp, pstride), dtype=np.float32)
    pos[..., :2] = CENTRES[cl][:, :, None, :] + drift + jit
    if pstride == 4:
        pos[..., 2:] = rng.standard_normal((K, B, Tp, 2))              # velocities: not read
    return pos, cl


def assert_separated(pos, groups, metric):
    """No comparison within reach of rounding: per row, two draws are below 0.75 (one cluster) or above 7 apart."""
    K = pos.shape[0]
    seen = [0, 0]
    for c in range(K):
        d = pair_dist(pos, c, metric)
        assert ((d < 0.75) | (d > 7.0)).all()
        seen[0] += int((d < 0.75).sum()) - d.shape[1]
        seen[1] += int((d > 7.0).sum())
    return seen


def scores_for(K, B, quantised, seed):
    rng = np.random.default_rng(seed + 1000)
    s = rng.standard_normal((K, B)).astype(np.float32)
    return (np.floor(s.clip(-1.0, 0.99) * 2) / 2).astype(np.float32) if quantised else s      # 4 levels: -1, -0.5, 0, 0.5


def _cases():
    """A covering design: every K with every M in {1, 3, K}; B, Tp, pstride, metric, clusters and score pattern rotate."""
    out, i = [], 0
    for K in (1, 20, 64, 65, 130):
        for M in sorted({1, min(3, K), K}):
            for rep in range(2 if K > 1 else 1):
                out.append((K, (1, 5, 7)[i % 3], (1, 12)[(i // 2) % 2], (2, 4)[(i // 3) % 2], M, ("fde", "ade")[i % 2],
                            1 + (i * 2 + rep) % 5, i % 4 != 1))
                i += 1
    return out


CASES = _cases()


def _regime(K, B, Tp, pstride, M, metric, n_cl, quantised):
    seed = K * 7 + B
    pos, _ = clustered(K, B, Tp, pstride, n_cl, seed)
    score = scores_for(K, B, quantised, seed)
    slack = []
    ref = nms_reference(pos, score, [(a, a + 1) for a in range(B)], M, 1.0, metric, slack=slack)
    left = {g for g, _, _ in slack}
    return {("left" if g in left else "full") if ref[1][g] == M else "short" for g in range(B)}


def test_the_cases_cover_the_issue():
    for col, want in ((0, {1, 20, 64, 65, 130}), (1, {1, 5, 7}), (2, {1, 12}), (3, {2, 4}), (5, {"fde", "ade"}),
                      (6, {1, 2, 3, 4, 5}), (7, {False, True})):
        assert {c[col] for c in CASES} == want, col
    for K in (20, 64, 65, 130):
        assert {c[4] for c in CASES if c[0] == K} == {1, 3, K}
    seen = set()
    for c in CASES:
        seen |= _regime(*c)
    assert seen == {"short", "full", "left"}      # count < M | count == M without leftovers | count == M with leftovers


@pytest.mark.parametrize("K,B,Tp,pstride,M,metric,n_cl,quantised", CASES)
def test_kernel_equals_the_definition_on_constructed_draws(K, B, Tp, pstride, M, metric, n_cl, quantised):
    seed = K * 7 + B
    pos, cl = clustered(K, B, Tp, pstride, n_cl, seed)
    near, far = assert_separated(pos, None, metric)
    assert far > 0 or n_cl == 1 or K == 1
    score = scores_for(K, B, quantised, seed)
    if quantised and K >= 20:
        assert len(np.unique(score)) <= 4
    rng = np.random.default_rng(seed + 5)
    err = rng.random((K, B, 2)).astype(np.float32)
    best = err[..., 0].argmin(axis=0).astype(np.int32)
    groups = [(a, a + 1) for a in range(B)]
    slack = []
    want = nms_reference(pos, score, groups, M, 1.0, metric, err=err, best=best, slack=slack)
    for _, _, d in slack:                           # a leftover's nearest pick is nearest by a wide margin, or an exact tie
        ds = np.sort(d)
        assert len(ds) == 1 or ds[1] - ds[0] > 1.0 or ds[1] == ds[0]
    got = run_kernel(pos, score, K, M, 1.0, metric, err=err, best=best)
    assert_exact(got, want, (K, B, Tp, pstride, M, metric, n_cl))
    again = run_kernel(pos, score, K, M, 1.0, metric, err=err, best=best)      # two calls: the same bits
    assert all(np.array_equal(x, y) for x, y in zip(got, again))
    no_rows = run_kernel(pos, score, K, M, 1.0, metric)                      # without err: the selection alone
    assert no_rows[4] is None and all(np.array_equal(x, y) for x, y in zip(got[:4], no_rows[:4]))
    # the clusters are the modes: every draw of a kept mode sits in the cluster of its pick
    for a in range(B):
        for k in range(K):
            m = got[3][a, k]
            if cl[k, a] in cl[got[0][a, :got[1][a]], a]:
                assert cl[got[0][a, m], a] == cl[k, a]


@pytest.mark.parametrize("inv_ss", [1.0, 4.0])
def test_inv_ss_scales_the_distance(inv_ss):
    pos, _ = clustered(20, 5, 12, 4, 3, 3)
    score = scores_for(20, 5, False, 3)
    for metric in ("fde", "ade"):
        want = nms_reference(pos / inv_ss, score, [(a, a + 1) for a in range(5)], 3, 1.0, metric, inv_ss=inv_ss)
        got = run_kernel((pos / inv_ss).astype(np.float32), score, 20, 3, 1.0, metric, inv_ss=inv_ss)
        assert_exact(got, want, (inv_ss, metric))
        assert (want[1] == 3).all()


@pytest.mark.parametrize("metric,Tp,M", [("fde", 1, 40), ("ade", 12, 40), ("fde", 1, 3)])
def test_exact_duplicates_are_suppressed_at_radius_zero(metric, Tp, M):
    """Distance 0 <= radius 0.  M = K: no leftovers, one mode per distinct draw.  M = 3 with one step: the leftovers compare
    square roots of small exact integers (units of 1/4096), which fp32 and float64 order alike."""
    K, B = 40, 5
    rng = np.random.default_rng(11)
    base = (rng.integers(-16, 17, size=(12, B, Tp, 2)) / 64.0).astype(np.float32)
    pos = base[rng.integers(0, 12, size=K)]                            # K draws, 12 distinct ones at most (the same for every row)
    score = scores_for(K, B, True, 11)
    groups = [(a, a + 1) for a in range(B)]
    want = nms_reference(pos, score, groups, M, 0.0, metric)
    distinct = np.array([len({pos[k, a].tobytes() for k in range(K)}) for a in range(B)])
    if M == K:
        assert np.array_equal(want[1], distinct) and distinct.max() < K
    got = run_kernel(pos, score, K, M, 0.0, metric)
    assert_exact(got, want, (metric, Tp, M))
    for a in range(B):                                                 # a mode's draws are copies of its pick
        for k in range(K):
            if M == K:
                assert np.array_equal(pos[k, a], pos[got[0][a, got[3][a, k]], a])


def equidistant_leftover():
    """One row, one step, five draws on the x axis at 0, 8, 4, 0.5, 5 with descending scores, M = 2, radius 1: the picks are
    draws 0 and 1, draw 3 joins pick 0, and of the leftovers draw 2 is exactly 4 from both picks - the lowest m takes it -
    while draw 4 is nearer to pick 1.  Small integers and halves: fp32 and float64 see the same distances
    (tests/test_nms_host.py)."""
    pos = np.zeros((5, 1, 1, 2), dtype=np.float32)
    pos[:, 0, 0, 0] = [0.0, 8.0, 4.0, 0.5, 5.0]
    score = np.array([5.0, 4.0, 3.0, 2.0, 1.0], dtype=np.float32).reshape(5, 1)
    return pos, score, 2, 1.0


@pytest.mark.parametrize("metric", ["fde", "ade"])
def test_a_leftover_between_equally_near_picks_goes_to_the_lowest_m(metric):
    """The tie rule of the leftover loop (`D < bd`, the first minimum): the seeded fault "the later pick takes an
    equidistant leftover" (tools/mutants/nms_leftover_tie.diff) passed every other case of this module, whose leftovers
    never sit at equal distances."""
    pos, score, M, radius = equidistant_leftover()
    want = nms_reference(pos, score, [(0, 1)], M, radius, metric)
    assert want[0].tolist() == [[0, 1]] and want[3].tolist() == [[0, 1, 0, 0, 1]]
    got = run_kernel(pos, score, 5, M, radius, metric)
    assert_exact(got, want, metric)


def test_the_largest_k():
    """K = M = 4096: the whole LDS budget of the launch (131 072 B per workgroup), a partial workgroup."""
    K, B = 4096, 3
    pos, _ = clustered(K, B, 1, 2, 5, 1)
    score = scores_for(K, B, True, 1)
    for c in range(0, K, 512):                                         # separation, on a sample of the columns
        d = pair_dist(pos, c, "fde")
        assert ((d < 0.75) | (d > 7.0)).all()
    want = nms_reference(pos, score, [(a, a + 1) for a in range(B)], K, 1.0, "fde")
    assert (want[1] == 5).all()
    assert_exact(run_kernel(pos, score, K, K, 1.0, "fde"), want, "K 4096")


# ---- scenes ----------------------------------------------------------------------------------------------------------------
RAGGED = [1, 2, 17, 70, 1, 5, 2, 64, 3]


def _groups(sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]


@pytest.mark.parametrize("K,M,metric,pstride", [(20, 3, "fde", 4), (20, 5, "ade", 2), (65, 65, "fde", 2), (20, 1, "ade", 4)])
def test_ragged_scenes_against_the_definition(K, M, metric, pstride):
    groups = _groups(RAGGED)
    B = groups[-1][1]
    assert {1, 2, 17, 70} <= set(RAGGED) and len(groups) % 4 != 0
    pos, cl = clustered(K, B, 12, pstride, 3, K + M, per_group=groups)
    assert_separated(pos, None, metric)
    score = scores_for(K, B, M == 3, K)
    rng = np.random.default_rng(2)
    err = rng.random((K, B, 2)).astype(np.float32)
    best = err[..., 0].argmin(axis=0).astype(np.int32)
    slack = []
    want = nms_reference(pos, score, groups, M, 1.0, metric, err=err, best=best, slack=slack)
    # The maximum over a scene's rows brings a leftover's distances to two picks closer together than they are on one row.
    # An fp32 distance is off by (Tp + 4) * 2^-24 of itself at most (the differences are exact; two roundings under the root,
    # the root, Tp additions, a division, a product): the two must be apart by twice that, here with another factor 2.
    for _, _, d in slack:
        ds = np.sort(d)
        assert len(ds) == 1 or ds[1] - ds[0] > 4 * (12 + 4) * 2.0 ** -24 * ds[0] or ds[1] == ds[0]
    got = run_kernel(pos, score, K, M, 1.0, metric, groups=groups, err=err, best=best)
    assert_exact(got, want, (K, M, metric))
    # a joint mode is a tuple of clusters: the larger scenes have more of them than any single row has clusters
    big = RAGGED.index(70)
    if M == K:
        assert want[1][big] == len({cl[k, groups[big][0]:groups[big][1]].tobytes() for k in range(K)}) > 3
    # the group score is the lowest of its rows: the first pick maximises it
    for g, (a, b) in enumerate(groups):
        assert got[0][g, 0] == int(np.argmax(score[:, a:b].min(axis=1)))


def test_single_agent_scenes_equal_the_per_row_mode():
    K, B, M = 20, 9, 3
    pos, _ = clustered(K, B, 12, 4, 4, 8)
    score = scores_for(K, B, True, 8)
    err = np.random.default_rng(3).random((K, B, 2)).astype(np.float32)
    best = err[..., 0].argmin(axis=0).astype(np.int32)
    for metric in ("fde", "ade"):
        rows = run_kernel(pos, score, K, M, 1.0, metric, err=err, best=best)
        scenes = run_kernel(pos, score, K, M, 1.0, metric, groups=[(a, a + 1) for a in range(B)], err=err, best=best)
        assert all(np.array_equal(x, y) for x, y in zip(rows, scenes))


def test_radius_zero_is_the_ranking_and_a_huge_radius_one_mode():
    from socialways_amd import ops
    K, B = 20, 37
    gen = torch.Generator(device="cuda").manual_seed(5)
    pos = torch.randn(K, B, 12, 4, device="cuda", generator=gen)       # distinct draws
    for ties in (False, True):
        score = torch.randn(K, B, device="cuda", generator=gen)
        if ties:
            score = (score * 2).round() / 2
        for M in (1, 5, K):
            for metric in ("fde", "ade"):
                order, count, weight, assign, _ = ops.sample_nms(pos, score, K, M, 0.0, metric)
                want, _ = ops.sample_rank(score, K, M)
                assert torch.equal(order, want) and bool((count == M).all())
                if M == K:
                    assert torch.equal(weight, torch.full_like(weight, 1.0 / K))
                    assert torch.equal(assign.gather(1, order.long()), torch.arange(K, device="cuda", dtype=torch.int32).expand(B, K))
                scenes = ops.SceneIndex.get(np.asarray(_groups([1] * B)), B, pos.device)
                assert torch.equal(ops.sample_nms(pos, score, K, M, 0.0, metric, scenes)[0], want)
    groups = _groups([5, 1, 20, 11])
    scenes = ops.SceneIndex.get(np.asarray(groups), B, pos.device)
    for sc in (None, scenes):
        order, count, weight, assign, _ = ops.sample_nms(pos, score, K, 5, 1e30, "ade", sc)
        assert bool((count == 1).all()) and bool((weight[:, 0] == 1.0).all()) and bool((weight[:, 1:] == 0.0).all())
        assert bool((order[:, 1:] == -1).all()) and bool((assign == 0).all())
    s_g = torch.stack([score[:, a:b].min(dim=1)[0] for a, b in groups], dim=1)         # (K, S)
    assert torch.equal(order[:, 0].long(), torch.sort(s_g.t().contiguous(), dim=1, descending=True, stable=True)[1][:, 0])


# ---- a trainer's real draws --------------------------------------------------------------------------------------------------
_TRAINED = {}


def trained(kind):
    """A trainer after a handful of steps, its draws, scores, errors for one batch of <= 64 agents: computed once, shared."""
    if kind not in _TRAINED:
        import socialways_amd as sw
        from socialways_amd import ops
        torch.manual_seed(3)
        np.random.seed(3)
        if kind == "toy":
            tracks = sw.toy_tracks(n_samples=384)
            n_next = 2
        else:
            sizes = sw.ragged_scene_sizes(320, 8, seed=5)
            tracks = sw.synth_tracks(len(sizes), sizes, seed=21)
            n_next = 12
        data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], tracks.get("times"), device=DEV)
        tr = sw.SocialWaysTrainer(n_next, use_social=True, device=DEV)
        tr.train_epoch(data, 64)
        tr.release_graphs()
        batches, n = [], 0
        for a, b in data.test_batches:
            if n + int(b - a) > 64:
                break
            batches.append((int(a), int(b)))
            n += int(b - a)
        lo, hi = batches[0][0], batches[-1][1]
        groups = [(a - lo, b - lo) for a, b in batches]
        obsv, pred, K = data.obsv[lo:hi], data.pred[lo:hi], 20
        noise = torch.rand(K, hi - lo, tr.noise_len, device=DEV)
        ph = tr.G.sample(obsv, K, n_next, np.asarray(groups), noise)
        score, _ = tr.D.score_samples(obsv, ph)
        e = ((ph[..., :2].double() - pred.double().unsqueeze(0)) / float(data.ss)).pow(2).sum(-1).sqrt()
        err = torch.stack([e.mean(2), e[:, :, -1]], dim=2).float()
        torch.cuda.synchronize()
        assert 2 <= hi - lo <= 64 and len(groups) > 1
        _TRAINED[kind] = dict(pos=ph.cpu().numpy(), score=score.cpu().numpy(), err=err.cpu().numpy(), groups=groups,
                              inv_ss=1.0 / float(data.ss), tr=tr, data=data)
    return _TRAINED[kind]


def gap_radius(pos, groups, metric, inv_ss):
    """The midpoint of the widest gap between consecutive sorted pair distances (group distances D_g) from the 30 % to the 70 %
    quantile, and half that gap relative to it."""
    K = pos.shape[0]
    d = []
    for c in range(K):
        dc = pair_dist(pos, c, metric, inv_ss)
        d.append(np.stack([dc[c + 1:, a:b].max(axis=1) for a, b in groups], axis=1).ravel())
    d = np.sort(np.concatenate(d))
    mid = d[int(0.3 * len(d)):int(0.7 * len(d)) + 1]
    i = int(np.argmax(np.diff(mid)))
    radius = 0.5 * (mid[i] + mid[i + 1])
    return float(radius), float(0.5 * (mid[i + 1] - mid[i]) / radius)


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("metric", ["fde", "ade"])
@pytest.mark.parametrize("kind", ["toy", "synth"])
def test_kernel_on_real_draws(kind, metric, joint):
    t = trained(kind)
    pos, score, err = t["pos"], t["score"], t["err"]
    K, B = score.shape
    groups = t["groups"] if joint else [(a, a + 1) for a in range(B)]
    radius, half_gap = gap_radius(pos, groups, metric, t["inv_ss"])
    print("%s %s joint %d: B %d, radius %.6g, half gap / radius %.3g" % (kind, metric, joint, B, radius, half_gap))
    assert half_gap >= 1e-5, "no gap around the radius: %g" % half_gap
    best = err[..., 0].argmin(axis=0).astype(np.int32)
    M = 5
    slack = []
    want = nms_reference(pos, score, groups, M, radius, metric, t["inv_ss"], err=err, best=best, slack=slack)
    got = run_kernel(pos, score, K, M, radius, metric, groups=groups if joint else None, inv_ss=t["inv_ss"], err=err, best=best)
    order, count, weight, assign, per_row = got
    assert np.array_equal(count, want[1]) and np.array_equal(order, want[0])
    left = np.zeros_like(assign, dtype=bool)
    for g, k, d in slack:
        left[g, k] = True
        assert d[assign[g, k]] <= d.min() * (1 + 1e-5), (g, k, d, assign[g, k])
    assert np.array_equal(assign[~left], want[3][~left])
    for g in range(len(groups)):
        assert np.array_equal(weight[g], (np.bincount(assign[g], minlength=M)[:M] / K).astype(np.float32))
    assert count.mean() > 1
    # per_row from the device's own order / assign / weight: selections of err entries and that weight
    for g, (a, b) in enumerate(groups):
        picks = order[g, :count[g]]
        mb = assign[g, best[a:b]]
        rows = np.concatenate([err[picks[0], a:b], err[picks][:, a:b].min(axis=0), weight[g, mb][:, None],
                               mb[:, None].astype(np.float32)], axis=1)
        assert np.array_equal(per_row[a:b], rows), g


# ---- evaluate_diverse end to end -----------------------------------------------------------------------------------------------
def _held_out(test_sizes=(23, 1, 70, 6, 2, 17, 9, 1, 30)):
    import socialways_amd as sw
    train = sw.ragged_scene_sizes(200, 8, seed=11) * 3                 # SceneDataset holds out the last fifth of the scenes
    sizes = train[:4 * len(test_sizes)] + list(test_sizes)
    tracks = sw.synth_tracks(len(sizes), sizes, seed=99)
    data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], tracks["times"], device=DEV)
    assert len(data.test_batches) == len(test_sizes) > 8
    return data


def _diverse_from_public_pieces(tr, data, coll, K, M, radius, metric, joint, just_one=False):
    """The numbers of evaluate_diverse() without its kernel.  Per chunk of evaluate() the draws of Generator.sample on the
    host noise stream, the scores of Discriminator.score_samples, float64 errors; per group the numpy reference on them,
    which the record's order and count must equal wherever the radius is clear of every pair distance by 1e-5 (nearly
    everywhere: counted); the metrics from the record's own order / assign / weight, which are checked for consistency.
    Consumes the host RNG exactly like evaluate()."""
    keys = ("ade_div1", "fde_div1", "ade_divm", "fde_divm", "w_hit", "rank_hit")
    acc = dict.fromkeys(keys + ("n_modes", "w_first", "jade_divm", "jfde_divm"), 0.0)
    batches = [(int(b[0]), int(b[1])) for b in data.test_batches]
    if just_one:
        batches = batches[:1]
    inv_ss = 1.0 / float(data.ss)
    n_groups = clear = 0
    for i, j in tr.eval_chunks(batches, K, tr.TEST_CHUNK):
        lo, hi = batches[i][0], batches[j - 1][1]
        obsv, pred = data.obsv[lo:hi], data.pred[lo:hi]
        noise = tr.eval_noise(batches[i:j], K, tr.noise_len).to(DEV)
        sb = np.asarray([[a - lo, b - lo] for a, b in batches[i:j]], dtype=np.int64)
        ph = tr.G.sample(obsv, K, tr.n_next, sb, noise)
        score = tr.D.score_samples(obsv, ph)[0].cpu().numpy()
        e = ((ph[..., :2].double() - pred.double().unsqueeze(0)) * inv_ss).pow(2).sum(-1).sqrt()
        err_all = torch.stack([e.mean(2), e[:, :, -1]], dim=2).cpu().numpy()
        pos_all = ph.cpu().numpy()
        for si, (sa, sb_) in enumerate(sb):
            rec = coll[i + si]
            n = sb_ - sa
            assert rec["obsvs"].shape[0] == n and rec["preds_our"].shape[:2] == (K, n)
            pos, sc, err = pos_all[:, sa:sb_], score[:, sa:sb_], err_all[:, sa:sb_]
            best = err[..., 0].argmin(axis=0)
            groups = [(0, n)] if joint else [(a, a + 1) for a in range(n)]
            order, count, weight, assign = rec["order"], rec["count"], rec["weight"], rec["assign"]
            if joint:
                order, count, weight, assign = order[None], np.asarray([count]), weight[None], assign[None]
            assert order.shape == (len(groups), M) and assign.shape == (len(groups), K)
            for g, (a, b) in enumerate(groups):
                d = np.stack([pair_dist(pos[:, a:b], c, metric, inv_ss).max(axis=1) for c in range(K)])
                if np.abs(d - radius).min() >= 1e-5 * radius:
                    want = nms_reference(pos[:, a:b], sc[:, a:b], [(0, b - a)], M, radius, metric, inv_ss)
                    assert np.array_equal(order[g], want[0][0]) and count[g] == want[1][0], (i + si, g)
                    clear += 1
                picks = order[g, :count[g]]
                assert (picks >= 0).all() and (order[g, count[g]:] == -1).all() and (weight[g, count[g]:] == 0).all()
                assert np.array_equal(weight[g], (np.bincount(assign[g], minlength=M)[:M] / K).astype(np.float32))
                mb = assign[g, best[a:b]]
                acc["ade_div1"] += err[picks[0], a:b, 0].sum()
                acc["fde_div1"] += err[picks[0], a:b, 1].sum()
                acc["ade_divm"] += err[picks][:, a:b, 0].min(axis=0).sum()
                acc["fde_divm"] += err[picks][:, a:b, 1].min(axis=0).sum()
                acc["w_hit"] += weight[g, mb].astype(np.float64).sum()
                acc["rank_hit"] += mb.sum()
                acc["n_modes"] += count[g]
                acc["w_first"] += float(weight[g, 0])
                acc["jade_divm"] += (b - a) * err[picks][:, a:b, 0].mean(axis=1).min()
                acc["jfde_divm"] += (b - a) * err[picks][:, a:b, 1].mean(axis=1).min()
            n_groups += len(groups)
    assert clear > 0.9 * n_groups, (clear, n_groups)
    nt = data.n_test_samples
    out = {k: acc[k] / nt for k in keys + ("jade_divm", "jfde_divm")}
    out.update(n_modes=acc["n_modes"] / n_groups, w_first=acc["w_first"] / n_groups)
    return out, n_groups


@pytest.mark.parametrize("joint,metric,just_one,chunk", [(False, "fde", False, None), (True, "ade", False, 700),
                                                        (False, "ade", True, None), (True, "fde", False, None)])
def test_evaluate_diverse_end_to_end(joint, metric, just_one, chunk):
    import socialways_amd as sw
    data = _held_out()
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    K, M, radius = 20, 5, 0.5
    if chunk:
        tr.TEST_CHUNK = chunk
        assert len(list(tr.eval_chunks([(int(a), int(b)) for a, b in data.test_batches], K, chunk))) > 2
    torch.manual_seed(31)
    want4 = tr.evaluate(data, n_gen_samples=K, just_one=just_one)
    state = torch.get_rng_state()
    torch.manual_seed(31)
    coll = []
    res = tr.evaluate_diverse(data, n_gen_samples=K, top_m=M, radius=radius, metric=metric, joint=joint, just_one=just_one,
                              collect=coll)
    assert torch.equal(torch.get_rng_state(), state)
    keys = ("ade_avg", "fde_avg", "ade_min", "fde_min") + tr.DIVERSE_KEYS + ("n_agents", "n_groups", "K", "top_m", "radius", "metric")
    assert sorted(res) == sorted(keys + (("jade_divm", "jfde_divm") if joint else ()))
    assert (res["ade_avg"], res["fde_avg"], res["ade_min"], res["fde_min"]) == tuple(want4)       # Python floats, ==
    assert (res["K"], res["top_m"], res["radius"], res["metric"]) == (K, M, radius, metric)
    n_rec = 1 if just_one else len(data.test_batches)
    assert len(coll) == n_rec
    torch.manual_seed(31)
    want, n_groups = _diverse_from_public_pieces(tr, data, coll, K, M, radius, metric, joint, just_one)
    assert res["n_groups"] == n_groups and res["n_agents"] == sum(r["obsvs"].shape[0] for r in coll)
    for key, w in want.items():
        if key in res:
            print("%-10s evaluate_diverse %.9g   public pieces %.9g" % (key, res[key], w))
    for key, w in want.items():
        if key in res:
            assert abs(res[key] - w) <= 1e-5 * abs(w), (key, res[key], w)
    assert res["ade_min"] <= res["ade_divm"] <= res["ade_div1"] and res["fde_min"] <= res["fde_divm"] <= res["fde_div1"]
    assert 1.0 <= res["n_modes"] <= M and 0.0 < res["w_first"] <= 1.0 and 0.0 < res["w_hit"] <= 1.0
    assert 0.0 <= res["rank_hit"] <= M - 1
    if joint:
        assert res["ade_divm"] <= res["jade_divm"] and res["fde_divm"] <= res["jfde_divm"]
    torch.manual_seed(31)                              # without collect: the same numbers
    assert tr.evaluate_diverse(data, n_gen_samples=K, top_m=M, radius=radius, metric=metric, joint=joint, just_one=just_one) == res
    # per-row numbers do not depend on the chunking
    if chunk:
        tr.TEST_CHUNK = sw.SocialWaysTrainer.TEST_CHUNK
        torch.manual_seed(31)
        coll2 = []
        whole = tr.evaluate_diverse(data, n_gen_samples=K, top_m=M, radius=radius, metric=metric, joint=joint, collect=coll2)
        for a, b in zip(coll, coll2):
            for key in ("order", "count", "weight", "assign", "preds_our"):
                assert np.array_equal(a[key], b[key]), key
        for key in res:
            assert whole[key] == res[key] or abs(whole[key] - res[key]) <= 1e-12 * abs(res[key]), key
    with pytest.raises(ValueError):
        tr.evaluate_diverse(data, n_gen_samples=K, top_m=K + 1)
    with pytest.raises(ValueError):
        tr.evaluate_diverse(data, n_gen_samples=K, top_m=0)


def test_evaluate_diverse_relations():
    """The exact relations: radius 0 is evaluate_ranked() bit for bit, top_m = K at radius 0 is the minimum over all draws, a
    huge radius leaves one mode; two calls with a DeviceNoise agree.
    The held-out set has 256 agents.  evaluate() forms its means as sums * (1 / n_test_samples) (a tensor over a Python
    number), evaluate_ranked() as sums / n_test_samples (a tensor over a tensor); the two roundings differ in the last bit for
    a general n (measured on a set of another size: ade_divm 24.80178040373111 against ade_min 24.801780403731115 at top_m = K,
    radius 0, while the relations to evaluate_ranked() held), so one number can equal both to the bit only where 1 / n is
    exact.  The sums themselves are exact: a few hundred fp32 values of one magnitude in float64."""
    import socialways_amd as sw
    data = _held_out((23, 1, 70, 6, 2, 17, 9, 1, 30) + (8,) * 12 + (1,))
    assert data.n_test_samples == 256 and len(data.test_batches) > 8
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    K, M = 20, 5
    torch.manual_seed(31)
    ranked = tr.evaluate_ranked(data, n_gen_samples=K, top_m=M)
    torch.manual_seed(31)
    zero = tr.evaluate_diverse(data, n_gen_samples=K, top_m=M, radius=0.0)
    for a, b in (("ade_divm", "ade_topm"), ("fde_divm", "fde_topm"), ("ade_div1", "ade_top1"), ("fde_div1", "fde_top1")):
        assert zero[a] == ranked[b], (a, zero[a], ranked[b])
    assert zero["n_modes"] == M and 1.0 / K < zero["w_first"] < 1.0      # the K - M leftovers join their nearest pick
    for metric in ("fde", "ade"):
        torch.manual_seed(31)
        full = tr.evaluate_diverse(data, n_gen_samples=K, top_m=K, radius=0.0, metric=metric)
        assert full["ade_divm"] == full["ade_min"] and full["fde_divm"] == full["fde_min"]
        # every draw its own mode: each weight is fp32 1 / K; their float64 mean over the groups is that to a few ulp
        assert full["n_modes"] == K and abs(full["w_first"] - float(np.float32(1.0 / K))) <= 1e-12
        for joint in (False, True):
            torch.manual_seed(31)
            huge = tr.evaluate_diverse(data, n_gen_samples=K, top_m=M, radius=1e30, metric=metric, joint=joint)
            assert huge["n_modes"] == 1.0 and huge["w_first"] == 1.0 and huge["w_hit"] == 1.0 and huge["rank_hit"] == 0.0
            assert huge["ade_divm"] == huge["ade_div1"] and huge["fde_divm"] == huge["fde_div1"]
            if joint:
                assert huge["ade_div1"] <= huge["jade_divm"] or abs(huge["ade_div1"] - huge["jade_divm"]) <= 1e-12 * huge["jade_divm"]
    dn = sw.DeviceNoise(7)
    one = tr.evaluate_diverse(data, n_gen_samples=K, top_m=M, radius=0.5, joint=True, noise=dn)
    two = tr.evaluate_diverse(data, n_gen_samples=K, top_m=M, radius=0.5, joint=True, noise=dn)
    assert one == two and one["ade_min"] != zero["ade_min"]
    assert (one["ade_avg"], one["fde_avg"], one["ade_min"], one["fde_min"]) == tuple(tr.evaluate(data, n_gen_samples=K, noise=dn))
    assert one["ade_min"] <= one["ade_divm"] <= one["ade_div1"]


def test_evaluate_diverse_at_a_generic_width():
    """80 units, 3 latent codes (the layer-by-layer path): draws and scores from its own forward, selection from the kernel."""
    import socialways_amd as sw
    from socialways_amd import generic
    sizes = sw.ragged_scene_sizes(40, 6, seed=3)
    tracks = sw.synth_tracks(len(sizes), sizes, seed=7)
    data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], tracks["times"], device=DEV)
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, hidden_size=80, n_latent_codes=3, use_social=True, device=DEV)
    assert isinstance(tr, generic.GenericTrainer)
    K, M = 6, 3
    for joint in (False, True):
        torch.manual_seed(31)
        coll = []
        res = tr.evaluate_diverse(data, n_gen_samples=K, top_m=M, radius=0.3, joint=joint, collect=coll)
        assert all(np.isfinite(v) for v in res.values() if not isinstance(v, str))
        assert res["ade_min"] <= res["ade_divm"] <= res["ade_div1"] and 1.0 <= res["n_modes"] <= M
        assert res["n_agents"] == sum(int(b - a) for a, b in data.test_batches)
        torch.manual_seed(31)
        want, n_groups = _diverse_from_public_pieces(tr, data, coll, K, M, 0.3, "fde", joint)
        assert n_groups == res["n_groups"]
        for key, w in want.items():
            if key in res:
                assert abs(res[key] - w) <= 1e-5 * abs(w), (key, res[key], w)
    a, b = (int(x) for x in data.test_batches[0])
    trajs, weight, score, order, count = tr.sample_diverse(data.obsv[a:b], K, M, 0.05)
    assert trajs.shape == (M, b - a, 12, 4) and weight.shape == (b - a, M) and score.shape == (M, b - a)
    assert order.shape == (b - a, M) and count.shape == (b - a,)


# ---- sample_diverse ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("joint", [False, True])
def test_sample_diverse_returns_the_kept_draws(joint):
    import socialways_amd as sw
    from test_gpu_sample import crowd, SIZES
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    obsv, _, sb = crowd(SIZES)
    K, M, B = 20, 5, obsv.shape[0]
    noise = torch.rand(K, B, 32, device="cuda")
    draws = tr.G.sample(obsv, K, 12, sb, noise)
    all_scores, _ = tr.D.score_samples(obsv, draws)
    groups = [(int(a), int(b)) for a, b in np.asarray(sb)] if joint else [(a, a + 1) for a in range(B)]
    radius, half_gap = gap_radius(draws.cpu().numpy(), groups, "fde", 2.0)
    assert half_gap >= 1e-5
    trajs, weight, score, order, count = tr.sample_diverse(obsv, K, M, radius, "fde", joint, sb, noise, scale=2.0)
    G = len(groups)
    assert trajs.shape == (M, B, 12, 4) and score.shape == (M, B) and not trajs.requires_grad
    assert order.shape == (G, M) and order.dtype == torch.int32 and weight.shape == (G, M) and count.shape == (G,)
    want = nms_reference(draws.cpu().numpy(), all_scores.cpu().numpy(), groups, M, radius, "fde", 2.0)
    assert np.array_equal(order.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1])
    assert 1 <= int(count.min()) and int(count.max()) > 1
    gid = torch.as_tensor(np.repeat(np.arange(G), [b - a for a, b in groups]), device="cuda")
    ar = torch.arange(B, device="cuda")
    for m in range(M):
        k = order[gid, m].long()
        valid = k >= 0
        assert torch.equal(valid, m < count[gid])
        assert torch.equal(trajs[m][valid], draws[k.clamp(min=0), ar][valid]), m
        assert torch.equal(score[m][valid], all_scores[k.clamp(min=0), ar][valid]), m
        assert bool((trajs[m][~valid] == 0).all()) and bool((score[m][~valid] == float("-inf")).all())
        assert bool((weight[:, m][m >= count] == 0).all()) and bool((weight[:, m][m < count] > 0).all())
    assert torch.equal(weight.double().sum(dim=1).round(decimals=6), torch.ones(G, dtype=torch.float64, device="cuda"))
    if not joint:
        assert bool((score[1:] <= score[:-1]).all())                  # -inf padding included
    # a huge radius: one mode, every other slot is padding
    t1, w1, s1, o1, c1 = tr.sample_diverse(obsv, K, M, 1e30, "fde", joint, sb, noise, scale=2.0)
    assert bool((c1 == 1).all()) and bool((o1[:, 1:] == -1).all()) and bool((w1[:, 0] == 1).all()) and bool((w1[:, 1:] == 0).all())
    assert bool((t1[1:] == 0).all()) and bool((s1[1:] == float("-inf")).all())
    assert torch.equal(t1[0], draws[o1[gid, 0].long(), ar]) and torch.equal(s1[0], all_scores[o1[gid, 0].long(), ar])
    assert tr.sample_diverse(obsv, K, 2, radius, sub_batches=sb)[0].shape == (2, B, 12, 4)      # noise drawn on the device
    modes = sw.stats.sample_modes(draws, all_scores, radius, M, "fde", np.asarray(sb) if joint else None, scale=2.0)
    assert torch.equal(modes[0], order) and torch.equal(modes[1], count) and torch.equal(modes[2], weight)
    for bad in (0, K + 1):
        with pytest.raises(ValueError):
            tr.sample_diverse(obsv, K, bad, radius, sub_batches=sb, noise=noise)


# ---- argument checks with a device ---------------------------------------------------------------------------------------------
def test_c_abi_edges_on_the_device():
    from socialways_amd import _lib as L, ops
    lib = L.load()
    K, B, Tp, M = 6, 9, 4, 3
    t = lambda *s: torch.full(s, 7.0, device="cuda")
    ti = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")
    pos, score = torch.rand(K, B, Tp, 2, device="cuda"), torch.rand(K, B, device="cuda")
    order, count, weight, assign, per_row = ti(B, M), ti(B), t(B, M), ti(B, K), t(B, 6)
    p, st = L.ptr, L.stream()

    def call(B_=B, per_row_=None, err_=None, K_=K):
        return lib.sw_sample_nms(p(pos), 2, p(score), None, 0, B_, K_, Tp, M, 0, 1.0, 0.5, err_, None, p(order), p(count), p(weight),
                                 p(assign), per_row_, st)
    assert call(B_=0) == 0                                               # B == 0: SW_OK, nothing launched
    assert call(per_row_=p(per_row)) == -1 and call(K_=4097) == -2      # per_row needs err; K above the LDS budget
    torch.cuda.synchronize()
    assert int(order.min()) == 7 and int(count.min()) == 7 and float(weight.min()) == 7.0 and float(per_row.min()) == 7.0
    o0 = ops.sample_nms(pos[:, :0], score[:, :0], K, M, 0.5)
    assert o0[0].shape == (0, M) and o0[3].shape == (0, K) and o0[4] is None
    assert call() == 0                                                   # without err and best: the selection alone
    torch.cuda.synchronize()
    want = ops.sample_nms(pos, score, K, M, 0.5)
    assert torch.equal(order, want[0]) and torch.equal(count, want[1]) and torch.equal(weight, want[2]) and torch.equal(assign, want[3])
    # err without best: columns 4 and 5 are 0
    err = torch.rand(K, B, 2, device="cuda")
    pr = ops.sample_nms(pos, score, K, M, 0.5, err=err)[4]
    assert float(pr[:, 4:].abs().max()) == 0.0 and bool((pr[:, 2] <= pr[:, 0]).all())
