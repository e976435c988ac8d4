"""sw_plan_refine on the device: constructed cases against the numpy reference written from the header comment
(tests/_refine_ref.py), a relation to sw_clearance_grad that needs no reference, bit-for-bit properties, and the layers above -
stats.refine_plans, trainer.refine_plans, evaluate_refine.
Bounds.  One iteration (n_iter = 1, no cap): the gradient (X0 - out) / (lr d0^2) and the costs within GRAD_REL (2e-5) of the
largest float64 entry.  32 iterations: per case max(4 d32, 2 N 2^-24 M), d32 = the largest difference between the float32 and
the float64 run of the REFERENCE on that case (computed here on the CPU, never from the kernel), M the largest coordinate:
one rounding of a coordinate per update, doubled; the factor 4 covers the kernel's tree sums against numpy's pairwise ones and
the 1-ulp hardware reciprocal behind tau.
Observed on an MI355X (pytest -s): one iteration, gradient max|err| / max|ref| up to 8.7e-7 (tp1), costs up to
2.4e-7; 32 iterations, out max|err| up to 7.3e-6 at M = 67.7 (sizes_k20_ps4_p5; d32 7.3e-6, bound 2.6e-4), the smallest margin k1:
1.3e-6 against 4.1e-5 (d32 1.2e-6); against the clearance-penalty launch the gradient within 4e-7 of its largest entry."""
import functools

import numpy as np
import pytest
import torch

import _refine_ref as R
from _ref64 import GRAD_REL
from _util import golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = dict(R.constructed_cases())
ONE = dict(n_iter=1, lr=1.0, w_track=0.05, w_smooth=0.02, max_move=1e6)      # lr (2 w_track + 32 w_smooth) = 0.74; no step is capped


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def scene_list(sizes):
    o = np.concatenate([[0], np.cumsum(sizes)])
    return np.stack([o[:-1], o[1:]], axis=1).astype(np.int64)


def run(case, **descent):
    from socialways_amd import ops
    pos = dev(case["pos"])
    scenes = ops.SceneIndex.get(scene_list(case["sizes"]), pos.shape[1], pos.device)
    out = ops.plan_refine(pos, dev(case["start"]), scenes, case["K"], dev(case["plans"]), dev(case["plan_start"]), dev(case["q_scene"]),
                          dev(case["q_ego"]), case["d0"], case["inv_ss"], lens=dev(case["lens"]), **descent)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def reference(name, dtype, one):
    return R.refine_reference(CASES[name], CASES[name]["d0"], dtype=dtype, **(ONE if one else {}))


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def largest(case):
    return float(max(np.nanmax(np.abs(case["pos"][..., :2])), np.abs(case["plans"]).max(), np.abs(case["start"]).max(),
                     np.abs(case["plan_start"]).max()))


# ---- against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_one_iteration_is_the_gradient(name):
    case, want = CASES[name], reference(name, np.float64, True)
    out, cost, moved = (t.cpu().numpy().astype(np.float64) for t in run(case, **ONE))
    Q, P = case["plans"].shape[:2]
    assert out.shape == (Q, P, case["Tp"], 2) and cost.shape == (Q, P, 2, 3) and moved.shape == (Q, P)
    d02 = float(case["d0"]) ** 2
    grad = (case["plans"].astype(np.float64) - out) / (ONE["lr"] * d02)
    ref = want["step0"] / d02
    eg, ec = np.abs(grad - ref).max(), np.abs(cost - want["cost"]).max()
    print("%s: gradient max|err| %.3g of max|ref| %.3g (%.3g), cost max|err| %.3g of %.3g (%.3g); bound %.1g"
          % (name, eg, np.abs(ref).max(), eg / np.abs(ref).max(), ec, np.abs(want["cost"]).max(), ec / np.abs(want["cost"]).max(), GRAD_REL))
    assert np.isfinite(out).all() and np.isfinite(cost).all()
    assert eg <= GRAD_REL * np.abs(ref).max()
    assert ec <= GRAD_REL * np.abs(want["cost"]).max()
    assert np.abs(moved - want["moved"]).max() <= GRAD_REL * max(want["moved"].max(), 1e-30) + 2.0 ** -23 * largest(case) * case["inv_ss"]


@pytest.mark.parametrize("name", list(CASES))
def test_32_iterations(name):
    case, w64, w32 = CASES[name], reference(name, np.float64, False), reference(name, np.float32, False)
    N, M = 32, largest(case)
    d32 = float(np.abs(w32["out"].astype(np.float64) - w64["out"]).max())
    bound = max(4 * d32, 2 * N * 2.0 ** -24 * M)
    out, cost, moved = (t.cpu().numpy().astype(np.float64) for t in run(case))
    err = np.abs(out - w64["out"]).max()
    print("%s: out max|fp32 kernel - float64| %.3g, reference fp32 - float64 %.3g, M %.3g, bound %.3g; cost max|err| %.3g of %.3g"
          % (name, err, d32, M, bound, np.abs(cost - w64["cost"]).max(), np.abs(w64["cost"]).max()))
    assert np.isfinite(out).all() and err <= bound
    assert np.array_equal(cost[..., 0, 1], np.zeros_like(cost[..., 0, 1])), "the original plan has not moved"
    assert (cost[..., 1, 0] <= cost[..., 0, 0]).all()            # holds for the reference on these inputs (tests/test_refine_host.py)
    none = w64["n_other"] == 0
    assert not cost[none][..., 0].any()                          # no agent, or the ego alone: no penalty


def test_against_the_clearance_penalty_launch():
    """No reference: w_track = w_smooth = 0, one iteration - the expected penalty and its gradient are (2 / K) sum_k loss and
    (1 / K) sum_k grad of row 0 of stats.clearance_penalty on the scene [plan, the agents of draw k]."""
    from socialways_amd import stats
    case = R.refine_case([6], 4, 12, seed=12, P=5)
    K, d0 = 4, case["d0"]
    out, cost, _ = run(case, n_iter=1, lr=1.0, w_track=0.0, w_smooth=0.0, max_move=1e6)
    for p in range(5):
        loss, grad = 0.0, 0.0
        for k in range(K):
            trajs = np.concatenate([case["plans"][0, p][None], case["pos"][k][..., :2]], 0)
            start = np.concatenate([case["plan_start"][:1], case["start"]], 0)
            lo, gr, _ = stats.clearance_penalty(trajs, [], d0, start=start)
            loss, grad = loss + 2.0 * float(lo[0]) / K, grad + gr[0].double().cpu().numpy() / K
        got = (case["plans"][0, p].astype(np.float64) - out[0, p].double().cpu().numpy()) / d0 ** 2
        print("plan %d: penalty %.6g against %.6g, gradient max|diff| %.3g of %.3g" % (p, float(cost[0, p, 0, 0]), loss,
                                                                                     np.abs(got - grad).max(), np.abs(grad).max()))
        assert loss > 0 and abs(float(cost[0, p, 0, 0]) - loss) <= GRAD_REL * loss
        assert np.abs(got - grad).max() <= GRAD_REL * np.abs(grad).max()


# ---- bit for bit -----------------------------------------------------------------------------------------------------------
def test_two_calls_and_permuted_queries():
    case = CASES["queries"]
    a = run(case)
    assert same(a, run(case))
    perm = np.random.RandomState(0).permutation(len(case["q_scene"]))
    b = run(dict(case, plans=case["plans"][perm], plan_start=case["plan_start"][perm], q_scene=case["q_scene"][perm],
                 q_ego=case["q_ego"][perm]))
    assert same([t[torch.from_numpy(perm).to(DEV)] for t in a], b)


def test_a_plan_alone_and_a_scene_alone():
    case = CASES["sizes_k20_ps4_p5"]
    full = run(case)
    for p in (0, 3):
        alone = run(dict(case, plans=np.ascontiguousarray(case["plans"][:, p:p + 1])))
        assert same([t[:, p:p + 1] for t in full], alone)
    off = np.concatenate([[0], np.cumsum(case["sizes"])])
    for s in (2, 4):                                             # the 7- and the 65-agent scene, cut out of the batch
        r = slice(off[s], off[s + 1])
        alone = run(dict(case, pos=np.ascontiguousarray(case["pos"][:, r]), start=case["start"][r].copy(), sizes=[case["sizes"][s]],
                         plans=case["plans"][s:s + 1].copy(), plan_start=case["plan_start"][s:s + 1].copy(),
                         q_scene=np.zeros(1, np.int32)))
        assert same([t[s:s + 1] for t in full], alone)


def test_the_egos_draws_and_the_padding_reach_nothing():
    case = CASES["queries"]
    base = run(case)
    pos = case["pos"].copy()
    egos = sorted({int(e) for e in case["q_ego"] if e >= 0})
    for i, (sc, e) in enumerate(zip(case["q_scene"], case["q_ego"])):      # one query at a time: its ego's draws are NaN
        off = np.concatenate([[0], np.cumsum(case["sizes"])])
        if not (0 <= sc < len(case["sizes"]) and off[sc] <= e < off[sc + 1]):
            continue
        pos = case["pos"].copy()
        pos[:, e] = np.nan
        got = run(dict(case, pos=pos))
        assert same([t[i:i + 1] for t in base], [t[i:i + 1] for t in got]) and bool(torch.isfinite(got[0][i]).all())
    assert len(egos) >= 3
    ragged = CASES["k65_tp17_ragged_x2"]                         # NaN behind every length already; other garbage there changes nothing
    a = run(ragged)
    pos = ragged["pos"].copy()
    pos[np.isnan(pos)] = 1e30
    assert same(a, run(dict(ragged, pos=pos))) and all(bool(torch.isfinite(t).all()) for t in a)


def test_no_iteration_and_no_force():
    case = CASES["sizes_k20_ps4_p5"]
    out, cost, moved = run(case, n_iter=0)
    assert torch.equal(bits(out), bits(dev(case["plans"]))) and not bool(moved.any())
    assert torch.equal(bits(cost[:, :, 0]), bits(cost[:, :, 1])) and bool((cost[..., 0, 0] > 0).any())
    first = run(case)[1][:, :, 0]
    assert torch.equal(bits(first), bits(cost[:, :, 0])), "the costs of the original do not depend on n_iter"
    # no agents (a scene index out of range) and zero weights: nothing acts on the plans
    lost = R.with_queries(case, [9, -1, 5, 7, 100], None)
    out, cost, moved = run(lost, w_track=0.0, w_smooth=0.0)
    assert torch.equal(bits(out), bits(dev(lost["plans"]))) and not bool(moved.any()) and not bool(cost[..., 0].any())
    from socialways_amd import ops
    pos = dev(case["pos"])
    scenes = ops.SceneIndex.get(scene_list(case["sizes"]), pos.shape[1], pos.device)
    none = ops.plan_refine(pos, dev(case["start"]), scenes, case["K"], dev(case["plans"][:0]), dev(case["plan_start"][:0]),
                           dev(case["q_scene"][:0]), None, case["d0"])
    assert none[0].shape == (0, 5, 12, 2) and none[1].shape == (0, 5, 2, 3) and none[2].shape == (0, 5)


# ---- the layers above --------------------------------------------------------------------------------------------------------
def test_stats_refine_plans_is_the_public_form():
    from socialways_amd import stats
    for name in ("k65_tp17_ragged_x2", "queries"):
        case = CASES[name]
        want = run(case, n_iter=5)
        got = stats.refine_plans(case["pos"], scene_list(case["sizes"]), case["plans"], R.D0_WORLD, case["plan_start"], case["start"],
                                 scene=case["q_scene"] if name == "queries" else None, ego=case["q_ego"], scale=case["inv_ss"],
                                 lens=case["lens"], n_iter=5)
        assert len(got) == 3 and same(got, want)


def test_trainer_refine_plans_is_sample_refine_and_risk():
    import socialways_amd as sw
    from socialways_amd import generic, ops
    from test_gpu_sample import crowd, SIZES
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=DEV)
    obsv, _, sb = crowd(SIZES)
    K, B = 20, obsv.shape[0]
    noise = torch.rand(K, B, 32, device=DEV)
    draws = tr.G.sample(obsv, K, 12, sb, noise)
    egos = np.array([int(a) + int(b - a) // 2 for a, b in np.asarray(sb)])
    plans = sw.predict_cv(obsv, 12)[egos][:, None, :, :2].repeat(1, 2, 1, 1)
    plans[:, 1] += 0.01                                          # two plans per query
    refined, risk, cost, moved, trajs = tr.refine_plans(obsv, plans, K, 0.1, coll_dist=0.05, sub_batches=sb, ego=egos, noise=noise,
                                                        scale=2.0, n_iter=8)
    assert torch.equal(trajs, draws) and refined.shape == plans.shape and risk.shape == (len(egos), 2, 2)
    want_risk = tr.plan_risk(obsv, plans, K, 0.05, sb, ego=egos, noise=noise, scale=2.0)[0]
    assert torch.equal(bits(risk[..., 0]), bits(want_risk)), "the risk of the original plans is plan_risk()'s"
    scenes = ops.SceneIndex.get(np.asarray(sb, dtype=np.int64), B, obsv.device)
    q_scene = torch.arange(len(egos), dtype=torch.int32, device=DEV)
    q_ego = torch.from_numpy(egos.astype(np.int32)).to(DEV)
    want = ops.plan_refine(draws, obsv[:, -1], scenes, K, plans, obsv[q_ego.long(), -1], q_scene, q_ego, 0.05, 2.0, n_iter=8)
    assert same((refined, cost, moved), want) and not refined.requires_grad
    after = ops.plan_risk(draws, obsv[:, -1], scenes, K, refined, obsv[q_ego.long(), -1], q_scene, q_ego, 0.05, 2.0)[0]
    assert torch.equal(bits(risk[..., 1]), bits(after))
    print("risk before %.4f after %.4f, penalty before %.4f after %.4f" % (float(risk[..., 0].mean()), float(risk[..., 1].mean()),
                                                                            float(cost[:, :, 0, 0].mean()), float(cost[:, :, 1, 0].mean())))
    # a DeviceNoise, no ego: the plans start where they are told to; (P, n_next, 2) is one query
    got = tr.refine_plans(obsv[:5], plans[1], 4, 0.1, plan_start=obsv[2:3, -1].clone(), noise=sw.DeviceNoise(7), row0=3)
    ph = tr.G.sample(obsv[:5], 4, 12, [], sw.DeviceNoise(7), row0=3)
    assert torch.equal(got[4], ph) and got[0].shape == (1, 2, 12, 2) and got[1].shape == (1, 2, 2)
    torch.manual_seed(1)
    wide = sw.SocialWaysTrainer(12, hidden_size=96, device=DEV)  # any hidden size: it needs only Generator.sample()
    assert isinstance(wide, generic.GenericTrainer)
    out = wide.refine_plans(obsv[:5], plans[1], 6, 0.1, ego=[2])
    assert out[0].shape == (1, 2, 12, 2) and out[4].shape == (6, 5, 12, 4) and bool(torch.isfinite(out[0]).all())


def test_evaluate_refine():
    import socialways_amd as sw
    g = golden("biwi_synth")
    data = sw.SceneDataset(g["obsvs"], g["preds"], g["batches"], g["times"], device=DEV)
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(data.pred.shape[1], use_social=True, device=DEV)
    torch.manual_seed(31)
    records = []
    res = tr.evaluate_refine(data, n_gen_samples=20, dist=0.5, coll_dist=0.1, collect=records)
    torch.manual_seed(31)
    plain = tuple(tr.evaluate(data, n_gen_samples=20))
    assert (res["ade_avg"], res["fde_avg"], res["ade_min"], res["fde_min"]) == plain
    torch.manual_seed(31)
    assert tr.evaluate_refine(data, n_gen_samples=20, dist=0.5, coll_dist=0.1) == res      # without collect: the same numbers
    print({k: res[k] for k in tr.REFINE_KEYS + ("n_ego",)})
    assert res["n_ego"] > 0 and res["K"] == 20 and res["dist"] == 0.5 and res["coll_dist"] == 0.1
    assert 0 <= res["risk_ref"] <= 1 and 0 <= res["risk_cv"] <= 1 and 0 <= res["pen_ref"] <= res["pen_cv"]
    assert 0 <= res["col_cv"] <= 1 and 0 <= res["col_ref"] <= 1 and res["moved"] >= 0
    # the sums, rebuilt from the records
    multi = [r for r in records if r["obsvs"].shape[0] > 1]
    n = sum(r["obsvs"].shape[0] for r in multi)
    assert n == res["n_ego"]
    for key, col in (("risk_cv", 0), ("risk_ref", 1)):
        v = sum(float(r["risk_plan"][:, col].astype(np.float64).sum()) for r in multi) / n
        assert abs(res[key] - v) <= 1e-9 + 1e-6 * abs(v)
    for key, col in (("col_cv", 0), ("col_ref", 1)):
        assert abs(res[key] - sum(int(r["hit_plan"][:, col].sum()) for r in multi) / n) <= 1e-12
    assert abs(res["moved"] - sum(float(r["moved"].astype(np.float64).sum()) for r in multi) / n) <= 1e-9 + 1e-6 * res["moved"]
    rec = multi[0]
    assert rec["plan_ref"].shape == rec["preds_lnr"].shape and np.isfinite(rec["plan_ref"]).all()
    torch.manual_seed(31)
    still = tr.evaluate_refine(data, n_gen_samples=20, dist=0.5, coll_dist=0.1, n_iter=0)
    assert still["moved"] == 0 and still["risk_ref"] == still["risk_cv"] == res["risk_cv"] and still["col_ref"] == still["col_cv"] == res["col_cv"]
