"""Composed scene futures on the GPU: sw_scene_compose against the float64 numpy implementation of its definition
(tests/_compose_ref.py, written from include/socialways_hip.h) - on constructed draws whose every cross clearance is far
from coll_dist (selection and counts exact), on a trainer's real draws with coll_dist placed in the widest gap of the cross
clearances - the bit-for-bit relations to sw_scene_clearance and sw_sample_rank, which need no threshold, and
SocialWaysTrainer.evaluate_composed() / sample_composed() against the same quantities from public pieces.

Tolerances: sel, sel0, per_scene, per_row exact (selections and integer counts; the constructed clearances are < 0.4 or > 0.6
at coll_dist 0.5, the real ones clear of coll_dist by an asserted 1e-5 of it, where an fp32 clearance is off by a few 1e-7 of
the coordinates); clear within clearance_bound of tests/test_gpu_scene.py, and equal to sw_scene_clearance on the selected
paths bit for bit.  The float64-summed means of evaluate_composed against evaluate_ranked: rtol 1e-5, the practice of
tests/test_gpu_rank.py."""
import numpy as np
import pytest
import torch

import _compose_ref as R
from test_compose_host import HAND
from test_gpu_scene import clearance_bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COLL = 0.5
MIX = [7, 1, 33, 2, 65, 7, 2, 1, 33, 5, 2, 7]      # 12 scenes: three times the waves of a workgroup


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def scene_list(sizes):
    o = np.concatenate([[0], np.cumsum(sizes)])
    return np.stack([o[:-1], o[1:]], axis=1).astype(np.int64)


def run(case, coll=COLL, sweeps=8, with_err=True):
    from socialways_amd import ops
    pos = dev(case["pos"])
    K, B = case["score"].shape
    scenes = ops.SceneIndex.get(scene_list(case["sizes"]), B, pos.device)
    out = ops.scene_compose(pos, dev(case["start"]), dev(case["score"]), scenes, K, coll, case["inv_ss"], sweeps,
                            lens=dev(case["lens"]), err=dev(case["err"]) if with_err else None)
    torch.cuda.synchronize()
    return out


def relations(case, out, coll):
    """What ties the outputs to the launches the project already has, bit for bit: no threshold, no reference."""
    from socialways_amd import ops
    sel, sel0, clear, per_scene, _ = out
    K, B = case["score"].shape
    pos, score = dev(case["pos"]), dev(case["score"])
    scenes = ops.SceneIndex.get(scene_list(case["sizes"]), B, pos.device)
    assert sel.dtype == sel0.dtype == per_scene.dtype == torch.int32 and clear.dtype == torch.float32
    assert 0 <= int(sel.min()) and int(sel.max()) < K
    picked = pos.gather(0, sel.long()[None, :, None, None].expand(1, B, pos.shape[2], pos.shape[3]))
    again = ops.scene_clearance(picked, dev(case["start"]), scenes, 1, case["inv_ss"], lens=dev(case["lens"]))[0]
    assert torch.equal(again, clear), "clear is sw_scene_clearance on the selected paths"
    assert torch.equal(sel0, ops.sample_rank(score, K, 1)[0][:, 0])
    off = scenes.scene_off.long()
    hit = torch.cat([torch.zeros(1, device=DEV), (clear < float(np.float32(coll))).float().cumsum(0)])
    any_hit = (hit[off[1:]] - hit[off[:-1]]) > 0
    assert torch.equal(per_scene[:, 1] > 0, any_hit)
    assert bool((per_scene[:, 1] <= per_scene[:, 0]).all()) and bool((per_scene >= 0).all())
    assert bool(((per_scene[:, 2] == 0) | (per_scene[:, 3] > 0)).all())
    single = torch.as_tensor(np.asarray(case["sizes"]) == 1, device=DEV)
    assert bool((per_scene[single] == 0).all())


CASES = {
    # name: (builder keywords, sweeps)
    "k20_start_p4": (dict(sizes=MIX, K=20, Tp=12, seed=11, stride=1, with_start=True, pstride=4, scores="quant"), 8),
    "k20_free_p2": (dict(sizes=MIX, K=20, Tp=12, seed=12), 8),
    "k20_start_p2": (dict(sizes=MIX, K=20, Tp=12, seed=12, stride=1, with_start=True), 8),
    "k20_start_cut": (dict(sizes=MIX, K=20, Tp=12, seed=12, stride=1, with_start=True), 1),
    "k1": (dict(sizes=[2, 7, 1, 33, 65], K=1, Tp=12, seed=13, spread=3), 8),
    "k65_tp17_ragged": (dict(sizes=[7, 33, 2, 65, 1, 7], K=65, Tp=17, seed=14, ragged=True, inv_ss=2.0, pstride=4), 8),
    "k65_tp17_start_ragged": (dict(sizes=[65, 7, 2, 33, 1], K=65, Tp=17, seed=15, stride=1, with_start=True, ragged=True,
                                   inv_ss=0.5, scores="quant"), 8),
    "k260_tp1_start": (dict(sizes=[2, 7, 33, 1, 7], K=260, Tp=1, seed=16, stride=1, spread=6, with_start=True, scores="quant"), 8),
    "k260_tp12": (dict(sizes=[7, 2, 33, 1], K=260, Tp=12, seed=17, inv_ss=4.0), 8),
    "k20_tp1_no_segment": (dict(sizes=[2, 7, 1, 33], K=20, Tp=1, seed=18, spread=1), 8),
    # 70 agents x 131 points do not fit the LDS budget: that scene reads its partners from global memory, the other is staged
    "global_paths": (dict(sizes=[70, 3], K=3, Tp=130, seed=19, ragged=True), 8),
    "dense_300": (dict(sizes=[300], K=4, Tp=3, seed=20), 8),
    # one path is longer than the LDS batch of candidate paths: candidates are read where they lie
    "long_horizon": (dict(sizes=[3, 2], K=3, Tp=1030, seed=21, spread=2), 8),
    # more candidates than one batch holds (78 paths of 13 points)
    "k200_batches": (dict(sizes=[7, 33], K=200, Tp=12, seed=22, stride=1, with_start=True), 8),
}
_REF = {}


def constructed(name):
    if name not in _REF:
        kw, sweeps = CASES[name]
        case = R.lane_case(**kw)
        _REF[name] = (case, sweeps, R.compose_reference(case["pos"], case["start"], case["score"], case["sizes"], COLL,
                                                        case["inv_ss"], sweeps, case["lens"], case["err"]))
    return _REF[name]


def compare(case, out, want):
    sel, sel0, clear, per_scene, per_row = (None if t is None else t.cpu().numpy() for t in out)
    assert np.array_equal(sel0, want["sel0"])
    assert np.array_equal(per_scene, want["per_scene"]), (per_scene, want["per_scene"])
    assert np.array_equal(sel, want["sel"])
    if per_row is not None:
        assert np.array_equal(per_row, want["per_row"])
    fin = np.isfinite(want["clear"])
    assert np.array_equal(np.isinf(clear) & (clear > 0), ~fin)
    M = float(np.nanmax(np.abs(case["pos"][..., :2])))
    if case["start"] is not None:
        M = max(M, float(np.abs(case["start"]).max()))
    d = np.abs(clear[fin] - want["clear"][fin])
    bound = clearance_bound(M, case["inv_ss"])
    print("clear: max |fp32 - float64| %.3g, bound %.3g" % (d.max() if d.size else 0.0, bound))
    assert (d <= bound).all()


@pytest.mark.parametrize("name", list(CASES))
def test_constructed_cases_against_the_reference(name):
    case, sweeps, want = constructed(name)
    big = sum(n * n for n in case["sizes"]) * max(case["K"] ** 2 * case["Tp"], 1000) > 2e7
    c = R.cross_clearances(case["pos"], case["start"], case["sizes"], case["inv_ss"], case["lens"],
                           max_tuples=200000 if big else None)
    assert ((c < 0.4) | (c > 0.6)).all(), "the constructed clearances stay clear of coll_dist"
    out = run(case, sweeps=sweeps)
    print(name, "pairs %d -> %d, moved %d of %d, sweeps up to %d" % (want["per_scene"][:, 0].sum(), want["per_scene"][:, 1].sum(),
                                                                    want["per_scene"][:, 2].sum(), len(want["sel"]),
                                                                    want["per_scene"][:, 3].max()))
    compare(case, out, want)
    relations(case, out, COLL)
    twice = run(case, sweeps=sweeps)
    for a, b in zip(out, twice):
        assert torch.equal(a, b), "two calls, the same bits"
    bare = run(case, sweeps=sweeps, with_err=False)
    assert bare[4] is None and all(torch.equal(a, b) for a, b in zip(out[:4], bare[:4]))
    zero = run(case, coll=0.0, sweeps=sweeps)
    assert torch.equal(zero[0], zero[1]) and torch.equal(zero[1], out[1]) and not bool(zero[3].any())
    relations(case, zero, 0.0)
    if name == "k20_tp1_no_segment":
        assert bool(torch.isinf(out[2]).all()) and torch.equal(out[0], out[1]) and not bool(out[3].any())
    if name == "k1":
        assert not bool(out[0].any()) and int(out[3][:, 0].sum()) > 0


def test_constructed_cases_reach_every_regime():
    """Over the launches above: scenes without conflict, resolved in the first sweep, resolved later, left in conflict, cut
    short by sweeps = 1; and the dense scene and the one read from global memory did move agents."""
    ps = np.concatenate([constructed(n)[2]["per_scene"] for n in CASES if n != "k20_start_cut"])
    assert ((ps[:, 0] == 0).any() and ((ps[:, 0] > 0) & (ps[:, 1] == 0) & (ps[:, 3] == 1)).any()
            and ((ps[:, 1] == 0) & (ps[:, 3] >= 2)).any() and (ps[:, 1] > 0).any())
    assert not np.array_equal(constructed("k20_start_cut")[2]["sel"], constructed("k20_start_p2")[2]["sel"])
    for name in ("global_paths", "dense_300", "k260_tp12", "k65_tp17_ragged"):
        assert constructed(name)[2]["per_scene"][0, 2] > 0, name


@pytest.mark.parametrize("name", list(HAND) + ["swap"])
def test_hand_built_cases(name):
    case = R.swap_case() if name == "swap" else R.hand_case(**HAND[name])
    for sweeps in (8, 1):
        want = R.compose_reference(case["pos"], case["start"], case["score"], case["sizes"], COLL, 1.0, sweeps, None, case["err"])
        out = run(case, sweeps=sweeps)
        compare(case, out, want)
        relations(case, out, COLL)
    if name == "swap":
        assert out[0].tolist() == [0, 1] and out[2].tolist() == [3.0, 3.0] and out[3].tolist() == [[1, 0, 1, 1]]


def test_ragged_clear_is_the_length_clearance_of_the_selected_paths():
    """Mixed lengths over two time chunks and two agent tiles (18 segments with the start point, a scene of 70): compose's
    clear equals sw_scene_clearance_len on the selected paths as raw bits, +inf where nothing counts (the scene of one)
    included.  Both walk a pair's chunk with the one SC_CHUNK of sw_scene_dev.h."""
    from socialways_amd import ops
    case = R.lane_case(sizes=[1, 2, 5, 70], K=3, Tp=18, seed=23, stride=1, with_start=True, ragged=True)
    lens = case["lens"]
    assert lens.min() >= 1 and lens.max() <= 18 and len(set(lens.tolist())) > 8 and (lens <= 16).any() and (lens > 16).any()
    sel, _, clear, _, _ = run(case, with_err=False)
    pos, B = dev(case["pos"]), len(lens)
    scenes = ops.SceneIndex.get(scene_list(case["sizes"]), B, pos.device)
    picked = pos.gather(0, sel.long()[None, :, None, None].expand(1, B, pos.shape[2], pos.shape[3]))
    again = ops.scene_clearance(picked, dev(case["start"]), scenes, 1, case["inv_ss"], lens=dev(lens))[0]
    assert torch.equal(again.view(torch.int32), clear.view(torch.int32))
    assert float(clear[0]) == float("inf") and bool(torch.isfinite(clear[1:]).all())


def test_stats_compose_scenes_is_the_public_form():
    from socialways_amd import stats
    case, sweeps, want = constructed("k65_tp17_start_ragged")
    out = run(case)
    got = stats.compose_scenes(case["pos"], case["score"], scene_list(case["sizes"]), COLL, start=case["start"],
                               scale=case["inv_ss"], lens=case["lens"])
    assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, out[:4]))
    one = R.lane_case([9], 5, 4, seed=3)
    got = stats.compose_scenes(torch.from_numpy(one["pos"]), one["score"], [], COLL)           # [] = one scene of all agents
    want = R.compose_reference(one["pos"], None, one["score"], [9], COLL)
    assert np.array_equal(got[0].cpu().numpy(), want["sel"]) and np.array_equal(got[3].cpu().numpy(), want["per_scene"])
    with pytest.raises(ValueError):
        stats.compose_scenes(one["pos"], one["score"], [], COLL, lens=np.full(9, 5))


# ---- a trainer's real draws ----------------------------------------------------------------------------------------------------
def gap_threshold(c, q=0.1):
    """The midpoint of the widest gap between consecutive sorted cross clearances around the q quantile (from q / 2 to
    3 q / 2), and half that gap relative to it."""
    c = np.sort(c)
    mid = c[int(0.5 * q * len(c)):int(1.5 * q * len(c)) + 1]
    i = int(np.argmax(np.diff(mid)))
    coll = 0.5 * (mid[i] + mid[i + 1])
    return float(coll), float(0.5 * (mid[i + 1] - mid[i]) / coll)


def test_kernel_on_real_draws():
    from test_gpu_nms import trained
    t = trained("synth")
    sizes = [b - a for a, b in t["groups"]]
    assert 2 <= max(sizes) <= 8 and t["score"].shape[0] == 20
    case = dict(pos=t["pos"], start=None, score=t["score"], sizes=sizes, lens=None, err=t["err"], inv_ss=t["inv_ss"])
    c = R.cross_clearances(case["pos"], None, sizes, case["inv_ss"])
    coll, half_gap = gap_threshold(c)
    print("B %d, coll_dist %.6g (share of cross clearances below: %.3f), half gap / coll_dist %.3g"
          % (sum(sizes), coll, (c < coll).mean(), half_gap))
    assert half_gap >= 1e-5, "no gap around coll_dist: %g" % half_gap
    want = R.compose_reference(case["pos"], None, case["score"], sizes, coll, case["inv_ss"], 8, None, case["err"])
    out = run(case, coll=coll)
    print("pairs %s -> %s, moved %s" % (want["per_scene"][:, 0].tolist(), want["per_scene"][:, 1].tolist(),
                                        want["per_scene"][:, 2].tolist()))
    assert want["per_scene"][:, 0].sum() > 0 and want["per_scene"][:, 2].sum() > 0
    assert np.array_equal(out[0].cpu().numpy(), want["sel"]) and np.array_equal(out[3].cpu().numpy(), want["per_scene"])
    assert np.array_equal(out[1].cpu().numpy(), want["sel0"]) and np.array_equal(out[4].cpu().numpy(), want["per_row"])
    relations(case, out, coll)
    relations(case, run(case, coll=0.0), 0.0)
    for a, b in zip(out, run(case, coll=coll)):
        assert torch.equal(a, b)


# ---- evaluate_composed / sample_composed ---------------------------------------------------------------------------------------
def _check_composed(tr, data, K, coll_dist, fused=True, **kw):
    """evaluate_composed() against evaluate(), evaluate_ranked(top_m=1) and its own collect records.  fused=False: a trainer
    whose evaluate() is test() - other expressions for the same four means, so they agree to rounding (1e-6) and the bits
    are those of evaluate_ranked(), which shares the sampling hook."""
    from socialways_amd import stats
    torch.manual_seed(31)
    records = []
    res = tr.evaluate_composed(data, n_gen_samples=K, coll_dist=coll_dist, collect=records, **kw)
    base = (res["ade_avg"], res["fde_avg"], res["ade_min"], res["fde_min"])
    torch.manual_seed(31)
    plain = tuple(tr.evaluate(data, n_gen_samples=K, **kw))
    torch.manual_seed(31)
    ranked = tr.evaluate_ranked(data, n_gen_samples=K, top_m=1, **kw)
    if fused:
        assert base == plain
    else:
        assert all(abs(a - b) <= 1e-6 * abs(b) for a, b in zip(base, plain)), (base, plain)
    assert base == (ranked["ade_avg"], ranked["fde_avg"], ranked["ade_min"], ranked["fde_min"])
    for key in ("ade_top1", "fde_top1"):
        assert abs(res[key] - ranked[key]) <= 1e-5 * abs(ranked[key]), (key, res[key], ranked[key])
    torch.manual_seed(31)
    assert tr.evaluate_composed(data, n_gen_samples=K, coll_dist=coll_dist, **kw) == res      # without collect: the same numbers
    # the collision shares rebuilt from the records: world coordinates, the public clearance call on the picked draws.  The
    # records are denormalised (one fp32 rounding of every coordinate), so a scene whose clearance lies within 1e-5 of
    # coll_dist may fall on either side: such scenes are counted and bracket the result
    n_multi, cnt, slack, pairs = 0, {"sel0": 0, "sel": 0}, {"sel0": 0, "sel": 0}, [0, 0]
    for rec in records:
        n = rec["obsvs"].shape[0]
        assert rec["sel"].shape == rec["sel0"].shape == rec["clear"].shape == (n,) and rec["per_scene"].shape == (4,)
        assert rec["sel"].dtype == np.int32 and rec["per_scene"].dtype == np.int32
        pairs[0] += int(rec["per_scene"][0])
        pairs[1] += int(rec["per_scene"][1])
        if n < 2:
            assert np.isinf(rec["clear"]).all() and not rec["per_scene"].any()
            continue
        n_multi += 1
        lens = rec.get("pred_len")
        for key in ("sel0", "sel"):
            path = rec["preds_our"][rec[key], np.arange(n)]
            if lens is None:
                c = stats.scene_clearance(path, [], start=rec["obsvs"][:, -1])
            else:
                c = stats.scene_clearance_len(path, [], lens, start=rec["obsvs"][:, -1])
            c = float(c.min())
            cnt[key] += c < coll_dist
            slack[key] += abs(c - coll_dist) <= 1e-5 * coll_dist
        assert (rec["per_scene"][1] > 0) == bool((rec["clear"] < np.float32(coll_dist)).any())
    assert n_multi == res["n_multi"] > 0 and res["n_scenes"] == len(records)
    for key, name in (("sel0", "col_top1"), ("sel", "col_comp")):
        print("%s %.6g, rebuilt %d / %d (within 1e-5 of coll_dist: %d)" % (name, res[name], cnt[key], n_multi, slack[key]))
        assert abs(res[name] * n_multi - cnt[key]) <= slack[key] + 1e-9
    assert abs(res["pairs_top1"] * n_multi - pairs[0]) <= 1e-9 * max(pairs[0], 1)
    assert abs(res["pairs_comp"] * n_multi - pairs[1]) <= 1e-9 * max(pairs[1], 1)
    assert res["col_comp"] <= res["col_top1"] and res["pairs_comp"] <= res["pairs_top1"] and res["score_comp"] <= res["score_top1"]
    assert 0.0 <= res["moved"] <= 1.0 and (res["moved"] == 0 or res["pairs_comp"] < res["pairs_top1"])
    assert res["K"] == K and res["coll_dist"] == coll_dist and res["sweeps"] == 8
    print("pairs %.4g -> %.4g per scene, moved %.4g, ADE %.6g -> %.6g, score %.4g -> %.4g" % (
        res["pairs_top1"], res["pairs_comp"], res["moved"], res["ade_top1"], res["ade_comp"], res["score_top1"], res["score_comp"]))
    return res


def test_evaluate_composed():
    import socialways_amd as sw
    from test_gpu_nms import _held_out
    data = _held_out()
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    K = 20
    res = _check_composed(tr, data, K, 0.3)
    assert res["pairs_top1"] > 0 and res["moved"] > 0, "the held-out scenes have collisions to resolve at this distance"
    assert res["ade_min"] <= res["ade_top1"] and res["ade_min"] <= res["ade_comp"]
    torch.manual_seed(31)
    free = tr.evaluate_composed(data, n_gen_samples=K, coll_dist=0.0)
    assert free["moved"] == 0 and free["col_top1"] == 0 and free["ade_comp"] == free["ade_top1"] == res["ade_top1"]
    assert free["score_comp"] == free["score_top1"]
    torch.manual_seed(31)
    one = tr.evaluate_composed(data, n_gen_samples=K, coll_dist=0.3, just_one=True)
    assert one["n_scenes"] == 1
    dn = sw.DeviceNoise(7)
    a = tr.evaluate_composed(data, n_gen_samples=K, coll_dist=0.3, noise=dn)
    assert a == tr.evaluate_composed(data, n_gen_samples=K, coll_dist=0.3, noise=dn) and a["ade_min"] != res["ade_min"]


def _small_tracks():
    import socialways_amd as sw
    sizes = sw.ragged_scene_sizes(240, 8, seed=3)
    return sw.synth_tracks(len(sizes), sizes, seed=7)


def test_evaluate_composed_on_ragged_datasets():
    """A dataset with obs_len (short histories) and one with pred_len (futures that end inside the horizon)."""
    import socialways_amd as sw
    t = _small_tracks()
    rng = np.random.RandomState(5)
    B = len(t["obsvs"])
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    short = sw.SceneDataset(t["obsvs"], t["preds"], t["batches"], t["times"], device=DEV, obs_len=rng.randint(2, 9, B))
    assert _check_composed(tr, short, 8, 1.0)["pairs_top1"] > 0
    ends = sw.SceneDataset(t["obsvs"], t["preds"], t["batches"], t["times"], device=DEV).set_pred_len(rng.randint(1, 13, B))
    assert _check_composed(tr, ends, 8, 1.0)["pairs_top1"] > 0


def test_evaluate_composed_at_a_generic_width():
    """80 units, 3 latent codes (the layer-by-layer path): draws and scores from its own forward, the selection from the
    inherited method and the same kernel."""
    import socialways_amd as sw
    from socialways_amd import generic
    t = _small_tracks()
    data = sw.SceneDataset(t["obsvs"], t["preds"], t["batches"], t["times"], device=DEV)
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, hidden_size=80, n_latent_codes=3, use_social=True, device=DEV)
    assert isinstance(tr, generic.GenericTrainer)
    assert _check_composed(tr, data, 6, 1.0, fused=False)["pairs_top1"] > 0
    a, b = (int(x) for x in data.test_batches[0])
    trajs, score, sel, clear, per_scene = tr.sample_composed(data.obsv[a:b], 6, 0.05)
    assert trajs.shape == (b - a, 12, 4) and score.shape == sel.shape == clear.shape == (b - a,) and per_scene.shape == (1, 4)


def test_sample_composed_returns_the_selected_draws():
    import socialways_amd as sw
    from socialways_amd import ops
    from test_gpu_sample import crowd, SIZES
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    obsv, _, sb = crowd(SIZES)
    K, B = 20, obsv.shape[0]
    noise = torch.rand(K, B, 32, device="cuda")
    draws = tr.G.sample(obsv, K, 12, sb, noise)
    all_scores, _ = tr.D.score_samples(obsv, draws)
    sizes = [int(b - a) for a, b in np.asarray(sb)]
    c = R.cross_clearances(draws.cpu().numpy(), obsv[:, -1].cpu().numpy(), sizes, 2.0)
    coll, half_gap = gap_threshold(c)
    assert half_gap >= 1e-5
    trajs, score, sel, clear, per_scene = tr.sample_composed(obsv, K, coll, sb, noise, scale=2.0)
    assert trajs.shape == (B, 12, 4) and score.shape == (B,) and not trajs.requires_grad
    assert sel.shape == (B,) and sel.dtype == torch.int32 and clear.shape == (B,) and per_scene.shape == (len(sizes), 4)
    ar = torch.arange(B, device="cuda")
    assert torch.equal(trajs, draws[sel.long(), ar]) and torch.equal(score, all_scores[sel.long(), ar])
    want = R.compose_reference(draws.cpu().numpy(), obsv[:, -1].cpu().numpy(), all_scores.cpu().numpy(), sizes, coll, 2.0)
    assert np.array_equal(sel.cpu().numpy(), want["sel"]) and np.array_equal(per_scene.cpu().numpy(), want["per_scene"])
    assert want["per_scene"][:, 2].sum() > 0
    scenes = ops.SceneIndex.get(np.asarray(sb, dtype=np.int64).reshape(-1, 2), B, obsv.device)
    assert torch.equal(ops.scene_clearance(trajs.unsqueeze(0), obsv[:, -1], scenes, 1, 2.0)[0], clear)
    s0 = tr.sample_composed(obsv, K, 0.0, sb, noise)
    assert torch.equal(s0[2], ops.sample_rank(all_scores, K, 1)[0][:, 0]) and not bool(s0[4].any())
    assert torch.equal(s0[0], tr.sample_ranked(obsv, K, 1, sb, noise)[0][0])
    assert tr.sample_composed(obsv, K, coll, sub_batches=sb)[0].shape == (B, 12, 4)              # noise drawn on the device
    modes = sw.stats.compose_scenes(draws, all_scores, np.asarray(sb), coll, start=obsv[:, -1], scale=2.0)
    assert torch.equal(modes[0], sel) and torch.equal(modes[2], clear) and torch.equal(modes[3], per_scene)
    for bad in (dict(coll_dist=-1.0), dict(sweeps=0)):
        with pytest.raises(ValueError):
            tr.sample_composed(obsv, K, **dict(dict(coll_dist=coll, sub_batches=sb, noise=noise), **bad))


# ---- argument checks with a device ---------------------------------------------------------------------------------------------
def test_c_abi_edges_on_the_device():
    from socialways_amd import _lib as L, ops
    lib = L.load()
    K, B, Tp = 6, 9, 4
    t = lambda *s: torch.full(s, 7.0, device="cuda")
    ti = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")
    one = R.lane_case([4, 5], K, Tp, seed=4)
    pos, score = dev(one["pos"]), dev(one["score"])
    off = torch.tensor([0, 4, 9], dtype=torch.int32, device="cuda")
    sel, clear, per_scene, per_row = ti(B), t(B), ti(2, 4), t(B, 4)
    p, st = L.ptr, L.stream()

    def call(B_=B, S_=2, per_row_=None, err_=None, K_=K, sel0_=None, off_=off):
        return lib.sw_scene_compose(p(pos), 2, None, 0, p(score), p(off_), None, S_, B_, K_, Tp, 1.0, COLL, 8, err_, p(sel), sel0_,
                                    p(clear), p(per_scene), per_row_, st)
    assert call(B_=0) == 0 and call(S_=0) == 0                           # SW_OK, nothing launched
    assert call(per_row_=p(per_row)) == -1 and call(K_=4097) == -2      # per_row needs err; K above the limit
    torch.cuda.synchronize()
    assert int(sel.min()) == 7 and float(clear.min()) == 7.0 and int(per_scene.min()) == 7 and float(per_row.min()) == 7.0
    assert call() == 0                                                   # without err and sel0: the selection alone
    torch.cuda.synchronize()
    scenes = ops.SceneIndex.get(scene_list([4, 5]), B, pos.device)
    want = ops.scene_compose(pos, None, score, scenes, K, COLL)
    assert torch.equal(sel, want[0]) and torch.equal(clear, want[2]) and torch.equal(per_scene, want[3]) and want[4] is None
    # offsets that leave the batch: that scene reads nothing, writes no row and reports zeros
    bad_off = torch.tensor([0, 4, 12], dtype=torch.int32, device="cuda")
    sel.fill_(7)
    assert call(off_=bad_off) == 0
    torch.cuda.synchronize()
    assert torch.equal(sel[:4], want[0][:4]) and int(sel[4:].min()) == 7 and not bool(per_scene[1].any())
