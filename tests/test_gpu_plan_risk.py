"""sw_plan_risk on the device: constructed cases against the float64 reference written from the header comment
(tests/_risk_ref.py; every clearance at least 0.1 away from coll_dist, so the counts are exact), threshold-free relations to
the launches the project already has on a trainer's real draws (bit for bit, no reference), repeatability, and the layers
above - trainer.plan_risk, evaluate_risk.
Bounds: risk within 2 (n + 1) 2^-24 of the float64 product (n divisions, n - 1 products, one subtraction on values in
[0, 1]) and exactly 0 / 1 where the counts say so; counts exact; clear_min within clearance_bound of tests/test_gpu_scene.py."""
import numpy as np
import pytest
import torch

import _risk_ref as R
from test_gpu_scene import clearance_bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COLL = R.COLL


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def scene_list(sizes):
    o = np.concatenate([[0], np.cumsum(sizes)])
    return np.stack([o[:-1], o[1:]], axis=1).astype(np.int64)


def run(case, coll=COLL):
    from socialways_amd import ops
    pos = dev(case["pos"])
    scenes = ops.SceneIndex.get(scene_list(case["sizes"]), pos.shape[1], pos.device)
    out = ops.plan_risk(pos, dev(case["start"]), scenes, case["K"], dev(case["plans"]), dev(case["plan_start"]), dev(case["q_scene"]),
                        dev(case["q_ego"]), coll, case["inv_ss"], lens=dev(case["lens"]), plan_lens=dev(case["plan_lens"]))
    torch.cuda.synchronize()
    return out


def compare(name, case, out, want):
    risk, clear, counts = (t.cpu().numpy() for t in out)
    Q, P = case["plans"].shape[:2]
    assert risk.shape == clear.shape == (Q, P) and counts.shape == (Q, P, 4)
    assert risk.dtype == clear.dtype == np.float32 and counts.dtype == np.int32
    assert np.array_equal(counts, want["counts"]), (name, counts[counts != want["counts"]][:8], want["counts"][counts != want["counts"]][:8])
    bound = R.risk_bound(want["n_other"])[:, None]
    d = np.abs(risk.astype(np.float64) - want["risk"])
    print("%s: risk max |fp32 - float64| %.3g (bound %.3g .. %.3g), share with 0 < risk < 1: %.2f"
          % (name, d.max(), bound.min(), bound.max(), ((want["risk"] > 0) & (want["risk"] < 1)).mean()))
    assert (d <= bound).all()
    assert (risk[want["hsum"] == 0] == 0.0).all() and (risk[want["hmax"] == case["K"]] == 1.0).all()
    fin = np.isfinite(want["clear_min"])
    assert np.array_equal(np.isinf(clear) & (clear > 0), ~fin)
    M = float(max(np.nanmax(np.abs(case["pos"][..., :2])), np.nanmax(np.abs(case["plans"]))))
    if case["start"] is not None:
        M = max(M, float(np.abs(case["start"]).max()), float(np.abs(case["plan_start"]).max()))
    e = np.abs(clear[fin] - want["clear_min"][fin])
    cb = clearance_bound(M, case["inv_ss"])
    print("%s: clear_min max |fp32 - float64| %.3g, bound %.3g" % (name, e.max() if e.size else 0.0, cb))
    assert (e <= cb).all()


CASES = dict(R.constructed_cases())


@pytest.mark.parametrize("name", list(CASES))
def test_constructed_cases_against_the_reference(name):
    case = CASES[name]
    want = R.run_reference(case)
    c = want["c"]
    assert ((c < 0.4) | (c > 0.6)).all(), "the constructed clearances stay clear of coll_dist"
    out = run(case)
    compare(name, case, out, want)
    for a, b in zip(out, run(case)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two calls, the same bits"
    if case["Tp"] == 1 and case["start"] is None:              # no segment at all
        assert bool(torch.isinf(out[1]).all()) and not bool(out[0].any()) and bool((out[2][..., 1] == -1).all())
    zero = run(case, coll=0.0)                                 # coll_dist = 0 admits no conflict; the clearances stay
    assert not bool(zero[0].any()) and not bool(zero[2][..., 0].any()) and torch.equal(zero[1], out[1])


def test_a_pair_counts_the_shorter_of_the_agents_and_the_plans_length():
    """Finite frames behind a length, not NaN (a NaN folds into no minimum and hits nothing, whatever the gate says): one agent
    and one plan per scene, Tp = 4, no start point, 2 apart on the first segment and 0.25 apart from frame 2 on.  Query 0: the
    agent has 4 frames and the plan 2, query 1 the other way round - one countable segment either way, so no conflict and a
    clearance of 2; with both at full length the same paths conflict at frame 2."""
    t = np.arange(4, dtype=np.float32)
    agent = np.stack([t, np.zeros(4, np.float32)], 1)
    plan = np.stack([t, np.array([2.0, 2.0, 0.25, 0.25], np.float32)], 1)
    case = dict(pos=np.stack([agent, agent])[None], start=None, plans=np.stack([plan, plan])[:, None], plan_start=None, sizes=[1, 1], K=1,
                Tp=4, inv_ss=1.0, q_scene=np.arange(2, dtype=np.int32), q_ego=None, lens=np.array([4, 2], np.int32),
                plan_lens=np.array([2, 4], np.int32))
    want = R.run_reference(case)
    assert (want["clear_min"] == 2.0).all() and (want["counts"] == [0, -1, -1, 0]).all() and not want["risk"].any()
    compare("shorter length", case, run(case), want)
    full = dict(case, lens=None, plan_lens=None)
    want = R.run_reference(full)
    assert (want["clear_min"] == 0.25).all() and (want["counts"] == [[[1, 2, 0, 1]], [[1, 2, 1, 1]]]).all() and (want["risk"] == 1.0).all()
    compare("full length", full, run(full), want)


def test_no_query_and_queries_that_name_no_scene():
    from socialways_amd import ops
    case = R.with_queries(CASES["p5"], [0, 1], None)
    pos = dev(case["pos"])
    scenes = ops.SceneIndex.get(scene_list(case["sizes"]), pos.shape[1], pos.device)
    none = ops.plan_risk(pos, None, scenes, case["K"], dev(case["plans"][:0]), None, dev(case["q_scene"][:0]), None, COLL)
    assert none[0].shape == (0, 5) and none[1].shape == (0, 5) and none[2].shape == (0, 5, 4)
    lost = ops.plan_risk(pos, None, scenes, case["K"], dev(case["plans"]), None, dev(np.array([0, 2], np.int32)), None, COLL)
    good = run(case)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(lost, good))
    assert not bool(lost[0][1].any()) and bool(torch.isinf(lost[1][1]).all()) and lost[2][1].tolist() == [[0, -1, -1, 0]] * 5
    # offsets that leave the batch: the query reads nothing
    broken = ops.SceneIndex(scene_list(case["sizes"]), pos.shape[1], pos.device)
    broken.scene_off = torch.tensor([0, 5, 9], dtype=torch.int32, device=DEV)
    lost = ops.plan_risk(pos, None, broken, case["K"], dev(case["plans"]), None, dev(case["q_scene"]), None, COLL)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(lost, good)) and lost[2][1].tolist() == [[0, -1, -1, 0]] * 5


def test_stats_plan_risk_is_the_public_form():
    from socialways_amd import stats
    for name in ("k65_tp17_ragged_start_half", "queries"):
        case = CASES[name]
        out = run(case)
        got = stats.plan_risk(case["pos"], scene_list(case["sizes"]), case["plans"], COLL, plan_start=case["plan_start"],
                              start=case["start"], scene=case["q_scene"] if name == "queries" else None, ego=case["q_ego"],
                              scale=case["inv_ss"], lens=case["lens"], plan_lens=case["plan_lens"])
        assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, out))


# ---- relations to the launches the project already has, on a trainer's real draws: bit for bit, no reference ---------------
@pytest.fixture(scope="module")
def drawn():
    import socialways_amd as sw
    from socialways_amd import ops
    from test_gpu_sample import crowd, SIZES
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    obsv, gt, sb = crowd(SIZES)
    K, B = 20, obsv.shape[0]
    noise = torch.rand(K, B, 32, device=DEV)
    draws = tr.G.sample(obsv, K, 12, sb, noise)
    other = tr.G.sample(obsv, 3, 12, sb, torch.rand(3, B, 32, device=DEV))     # the plans: three more draws of the ego
    sizes = [int(b - a) for a, b in np.asarray(sb)]
    scenes = ops.SceneIndex.get(np.asarray(sb, dtype=np.int64), B, obsv.device)
    egos = torch.tensor([int(a) + (int(b - a) // 2) for a, b in np.asarray(sb)], dtype=torch.int32, device=DEV)      # one per scene
    plans = other[:, egos.long(), :, :2].permute(1, 0, 2, 3).contiguous()      # (S, 3, Tp, 2)
    q_scene = torch.arange(len(sizes), dtype=torch.int32, device=DEV)
    inv_ss = 2.0
    first = ops.plan_risk(draws, obsv[:, -1], scenes, K, plans, obsv[egos.long(), -1], q_scene, egos, 0.0, inv_ss)
    fin = first[1][torch.isfinite(first[1])]
    coll = float(fin.median())                                                 # half the plans in conflict: any value serves, nothing is compared to a threshold
    out = ops.plan_risk(draws, obsv[:, -1], scenes, K, plans, obsv[egos.long(), -1], q_scene, egos, coll, inv_ss)
    return dict(tr=tr, obsv=obsv, gt=gt, sb=sb, sizes=sizes, scenes=scenes, K=K, B=B, noise=noise, draws=draws, egos=egos,
                plans=plans, q_scene=q_scene, inv_ss=inv_ss, coll=coll, out=out)


def test_the_plan_in_the_egos_row_gives_the_clearance_of_that_row(drawn):
    from socialways_amd import ops
    d = drawn
    risk, clear_min, counts = d["out"]
    assert int(counts[..., 0].max()) > 0 and bool((counts[..., 0] < d["K"]).any())
    e = d["egos"].long()
    for p in range(d["plans"].shape[1]):
        sub = d["draws"].clone()
        sub[:, e, :, :2] = d["plans"][None, :, p]
        clear = ops.scene_clearance(sub, d["obsv"][:, -1], d["scenes"], d["K"], d["inv_ss"])[:, e]      # (K, S)
        assert torch.equal(clear.min(0)[0].view(torch.int32), clear_min[:, p].view(torch.int32))
        assert torch.equal((clear < d["coll"]).sum(0).int(), counts[:, p, 0])


def test_two_row_scenes_give_the_per_agent_counts(drawn):
    from socialways_amd import ops
    d = drawn
    risk, _, counts = (t.cpu().numpy() for t in d["out"])
    K, draws, obsv = d["K"], d["draws"], d["obsv"]
    offs = np.concatenate([[0], np.cumsum(d["sizes"])])
    for s, n in enumerate(d["sizes"]):
        ego = int(d["egos"][s])
        rows = [r for r in range(offs[s], offs[s + 1]) if r != ego]
        for p in range(d["plans"].shape[1]):
            if not rows:
                assert risk[s, p] == 0 and counts[s, p].tolist() == [0, -1, -1, 0]
                continue
            m = len(rows)
            pair = torch.zeros(K, 2 * m, 12, 2, device=DEV)
            pair[:, 0::2] = d["plans"][s, p][None, None]
            pair[:, 1::2] = draws[:, rows, :, :2]
            start = torch.zeros(2 * m, 2, device=DEV)
            start[0::2] = obsv[ego, -1]
            start[1::2] = obsv[rows, -1]
            sc = ops.SceneIndex.get(scene_list([2] * m), 2 * m, obsv.device)
            clear = ops.scene_clearance(pair, start, sc, K, d["inv_ss"])[:, 0::2]
            h = (clear < d["coll"]).sum(0).cpu().numpy()
            b = int(np.argmax(h))
            assert counts[s, p, 3] == h[b] and counts[s, p, 2] == (rows[b] if h[b] else -1)
            want = 1.0 - np.prod((K - h).astype(np.float64) / K)
            assert abs(float(risk[s, p]) - want) <= R.risk_bound(m)
            assert (risk[s, p] == 0) == (h.max() == 0) and (risk[s, p] == 1) == (h.max() == K)
            assert counts[s, p, 0] <= min(K, h.sum()) and counts[s, p, 0] >= h.max()


def test_leave_one_out_on_a_single_draw_is_the_scene_clearance(drawn):
    from socialways_amd import ops
    d = drawn
    B = d["B"]
    for pos in (d["gt"], d["draws"][7, :, :, :2].contiguous()):
        q_scene, _ = d["scenes"].row_scene()
        ego = torch.arange(B, dtype=torch.int32, device=DEV)
        for start in (None, d["obsv"][:, -1]):
            _, clear_min, counts = ops.plan_risk(pos, start, d["scenes"], 1, pos[:, None].contiguous(),
                                                 None if start is None else start.contiguous(), q_scene, ego, d["coll"], d["inv_ss"])
            want = ops.scene_clearance(pos, start, d["scenes"], 1, d["inv_ss"])[0]
            assert torch.equal(clear_min[:, 0].view(torch.int32), want.view(torch.int32))
            assert torch.equal(counts[:, 0, 0] > 0, want < d["coll"])


def test_trainer_plan_risk_is_sample_plus_the_risk_launch(drawn):
    import socialways_amd as sw
    from socialways_amd import ops
    d = drawn
    tr, obsv, sb, K = d["tr"], d["obsv"], d["sb"], d["K"]
    risk, clear_min, counts, trajs = tr.plan_risk(obsv, d["plans"], K, d["coll"], sb, ego=d["egos"], noise=d["noise"], scale=d["inv_ss"])
    assert torch.equal(trajs, d["draws"]) and all(torch.equal(a, b) for a, b in zip((risk, clear_min, counts), d["out"]))
    assert not risk.requires_grad and trajs.shape == (K, d["B"], 12, 4)
    # a DeviceNoise, several queries on one scene, no ego: the plans start where they are told to
    scene = [5, 5, 2]
    pstart = obsv[[60, 61, 10], -1].clone()
    plans = d["plans"][[5, 5, 2]].contiguous()
    got = tr.plan_risk(obsv, plans, K, d["coll"], sb, scene=scene, plan_start=pstart, noise=sw.DeviceNoise(7), row0=3)
    ph = tr.G.sample(obsv, K, 12, sb, sw.DeviceNoise(7), row0=3)
    want = ops.plan_risk(ph, obsv[:, -1], d["scenes"], K, plans, pstart, torch.tensor(scene, dtype=torch.int32, device=DEV), None, d["coll"])
    assert torch.equal(got[3], ph) and all(torch.equal(a, b) for a, b in zip(got[:3], want))
    one = tr.plan_risk(obsv[:5], d["plans"][0], 4, d["coll"], ego=[2])          # (P, n_next, 2): one query, one scene; noise drawn on the device
    assert one[0].shape == (1, 3) and one[3].shape == (4, 5, 12, 4)


# ---- evaluate_risk ---------------------------------------------------------------------------------------------------------
def _check_risk(tr, data, K, coll_dist, fused=True, **kw):
    torch.manual_seed(31)
    records = []
    res = tr.evaluate_risk(data, n_gen_samples=K, coll_dist=coll_dist, collect=records, **kw)
    base = (res["ade_avg"], res["fde_avg"], res["ade_min"], res["fde_min"])
    torch.manual_seed(31)
    plain = tuple(tr.evaluate(data, n_gen_samples=K, **kw))
    if fused:
        assert base == plain
    else:
        assert all(abs(a - b) <= 1e-6 * abs(b) for a, b in zip(base, plain)), (base, plain)
    torch.manual_seed(31)
    assert tr.evaluate_risk(data, n_gen_samples=K, coll_dist=coll_dist, **kw) == res            # without collect: the same numbers
    from socialways_amd import stats
    r, dg, y, dt, slack = [], [], [], [], 0
    for rec in records:
        n = rec["obsvs"].shape[0]
        assert rec["risk"].shape == rec["risk_diag"].shape == rec["hit_gt"].shape == (n,) and rec["risk_counts"].shape == (n, 4)
        assert rec["risk_counts"].dtype == np.int32 and rec["hit_gt"].dtype == np.bool_
        assert np.array_equal(rec["risk_diag"], (rec["risk_counts"][:, 0].astype(np.float64) / K).astype(np.float32))
        assert ((rec["risk"] == 0) == (rec["risk_counts"][:, 3] == 0)).all() and ((rec["risk"] == 1) == (rec["risk_counts"][:, 3] == K)).all()
        if n < 2:
            assert not rec["risk"].any() and not rec["hit_gt"].any() and rec["risk_counts"].tolist() == [[0, -1, -1, 0]]
            continue
        r.append(rec["risk"].astype(np.float64))
        dg.append(rec["risk_counts"][:, 0].astype(np.float64) / K)
        y.append(rec["hit_gt"].astype(np.float64))
        # the true first conflict from the record's own (denormalised: one fp32 rounding per coordinate) ground truth, K = 1,
        # every agent against the others; an agent whose record says it collides and whose rebuilt paths do not is counted
        last, lens = rec["obsvs"][:, -1], rec.get("pred_len")
        true = stats.plan_risk(rec["preds_gtt"][None], [], rec["preds_gtt"][:, None], coll_dist, plan_start=last, start=last,
                               scene=np.zeros(n, np.int64), ego=np.arange(n), lens=lens, plan_lens=lens)[2][:, 0, 1].cpu().numpy()
        timed = rec["hit_gt"] & (rec["risk"] > 0)
        slack += int((timed & (true < 0)).sum())
        dt.append(np.abs(rec["risk_counts"][:, 1] - true)[timed & (true >= 0)].astype(np.float64))
    r, dg, y = np.concatenate(r), np.concatenate(dg), np.concatenate(y)
    want = dict(risk_mean=r.mean(), col_gt_agent=y.mean(), brier=((r - y) ** 2).mean(), brier_diag=((dg - y) ** 2).mean(),
                brier_base=((y.mean() - y) ** 2).mean(), risk_hit=r[y == 1].mean() if y.any() else 0.0,
                risk_miss=r[y == 0].mean() if (y == 0).any() else 0.0)
    for key, v in want.items():
        assert abs(res[key] - v) <= 1e-5 * abs(v) + 1e-12, (key, res[key], v)
    dt = np.concatenate(dt)
    n_timed = len(dt) + slack
    print("t_first_err %.6g, rebuilt from %d agents (collisions lost to the records' rounding: %d)" % (res["t_first_err"], len(dt), slack))
    assert abs(res["t_first_err"] * n_timed - dt.sum()) <= 12 * slack + 1e-9 * max(dt.sum(), 1.0)
    assert res["n_ego"] == len(r) > 0 and res["K"] == K and res["coll_dist"] == coll_dist and res["t_first_err"] >= 0
    print({k: res[k] for k in ("risk_mean", "col_gt_agent", "brier", "brier_diag", "brier_base", "risk_hit", "risk_miss", "t_first_err")})
    return res


def test_evaluate_risk():
    import socialways_amd as sw
    from test_gpu_nms import _held_out
    data = _held_out()
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    res = _check_risk(tr, data, 20, 0.3)
    assert 0 < res["col_gt_agent"] < 1 and 0 < res["risk_mean"] < 1, "the held-out scenes have collisions at this distance"
    torch.manual_seed(31)
    free = tr.evaluate_risk(data, n_gen_samples=20, coll_dist=0.0)
    assert free["risk_mean"] == 0 and free["col_gt_agent"] == 0 and free["brier"] == 0
    torch.manual_seed(31)
    assert tr.evaluate_risk(data, n_gen_samples=20, coll_dist=0.3, just_one=True)["n_ego"] == 23
    dn = sw.DeviceNoise(7)
    a = tr.evaluate_risk(data, n_gen_samples=20, coll_dist=0.3, noise=dn)
    assert a == tr.evaluate_risk(data, n_gen_samples=20, coll_dist=0.3, noise=dn) and a["ade_min"] != res["ade_min"]


def test_evaluate_risk_on_ragged_datasets_and_other_widths():
    import socialways_amd as sw
    from socialways_amd import generic
    from test_gpu_compose import _small_tracks
    t = _small_tracks()
    rng = np.random.RandomState(5)
    B = len(t["obsvs"])
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    short = sw.SceneDataset(t["obsvs"], t["preds"], t["batches"], t["times"], device=DEV, obs_len=rng.randint(2, 9, B))
    assert _check_risk(tr, short, 8, 1.0)["risk_mean"] > 0
    ends = sw.SceneDataset(t["obsvs"], t["preds"], t["batches"], t["times"], device=DEV).set_pred_len(rng.randint(1, 13, B))
    assert _check_risk(tr, ends, 8, 1.0)["risk_mean"] > 0
    torch.manual_seed(1)
    wide = sw.SocialWaysTrainer(12, hidden_size=96, device=DEV)
    assert isinstance(wide, generic.GenericTrainer)
    a, b = (int(x) for x in short.test_batches[0])
    obsv = short.obsv[a:b]
    out = wide.plan_risk(obsv, short.pred[a:b][:1, None, :, :2], 6, 1.0, ego=[0])
    assert out[0].shape == (1, 1) and out[2].shape == (1, 1, 4) and out[3].shape == (6, b - a, 12, 4)
    with pytest.raises(sw.SocialWaysHipError, match="pred_len"):
        wide.evaluate_risk(ends, n_gen_samples=2)
