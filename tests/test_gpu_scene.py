"""Scene-level K-sample metrics on the GPU: sw_scene_clearance / sw_scene_reduce, ops.scene_metrics, stats.scene_clearance
and SocialWaysTrainer.evaluate_scenes() against a float64 numpy implementation of their definitions
(include/socialways_hip.h).

The one discontinuity, `clear < coll_dist`, is tested in two halves: the clearance against float64 within a rounding
bound, and everything downstream of the comparison against float64 formed from the kernel's own fp32 `clear`, where the
flags are exact.

Measured on one MI355X (test_clearance_against_float64 prints every figure; run with -s): the largest
|clearance - float64| over all 36 cases (K 1 / 3 / 20, Tp 1 / 12 / 30, strides 2 / 4, with and without start, recipe seeds
3 - 5, inv_ss = 15) is 1.34e-06, at K = 20, Tp = 12, against the asserted rounding bound 16 * 2^-23 * M * inv_ss = 3.2e-05 -
3.3e-05; a float32 numpy evaluation of the same formula differs from float64 by 1.34e-06 on the same inputs.  The flags
test leaves out at most 0.087 % of the finite entries (two of 2 300), 3.8 - 33.8 % of which collide.  On the reference's
recorded samples the clearance differs from float64 on the recorded pred_hat by at most 3.9e-06 (tolerance 2.2e-03).
"""
import numpy as np
import pytest
import torch

from _util import golden, assert_close
from test_gpu_sample import RT, AT, SIZES, eval_golden, scene_list

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23


# ---- input recipe and float64 reference ---------------------------------------------------------------------------------
def crowd(sizes, K, To=8, Tp=12, seed=3):
    rng = np.random.RandomState(seed)
    B = int(np.sum(sizes))
    start = rng.rand(B, 2)
    obs = start[:, None] + (rng.rand(B, To, 2) * 0.1 - 0.03).cumsum(1) * 0.2
    fut = obs[None, :, -1:, :] + (rng.rand(K, B, Tp, 2) * 0.1 - 0.03).cumsum(2) * 0.2
    return obs.astype(np.float32), fut.astype(np.float32)          # start = obs[:, -1]


def clearance(last, fut, sizes, inv_ss, dt=np.float64):
    """Definition 2 in `dt`: last (B, 2) or None (then the path is fut alone), fut (K, B, Tp, 2) -> (K, B)."""
    fut = fut.astype(dt)
    K, B, Tp, _ = fut.shape
    path = fut
    if last is not None:
        path = np.concatenate([np.broadcast_to(last.astype(dt)[None, :, None], (K, B, 1, 2)), fut], 2)
    out, o = np.full((K, B), np.inf, dt), 0
    if path.shape[2] < 2:
        return out
    for n in sizes:
        p = path[:, o:o + n]
        r0 = p[:, :, None, :-1] - p[:, None, :, :-1]
        dv = (p[:, :, None, 1:] - p[:, None, :, 1:]) - r0
        dd, rd = (dv * dv).sum(-1), (r0 * dv).sum(-1)
        tau = np.where(dd > 0, np.clip(-rd / np.where(dd > 0, dd, 1), 0, 1), 0).astype(dt)
        c = r0 + tau[..., None] * dv
        d = np.sqrt((c * c).sum(-1)).min(-1) * dt(inv_ss)
        d[:, np.arange(n), np.arange(n)] = np.inf
        out[:, o:o + n] = d.min(-1)
        o += n
    return out


def clearance_bound(M, inv_ss):
    """A rounding bound for the dozen fp32 operations of definition 2 on coordinates up to M (not a measurement)."""
    return 16 * EPS * M * inv_ss


def scene_reference(err, clear, sizes, coll):
    """Definitions 1 and 3 in float64 from fp32 inputs: err (K, B, 2), clear (K, B) or None (flags are exact: the
    comparison is the kernel's, fp32 against fp32).  -> per_scene (S, 6), sade (K, S)."""
    K = err.shape[0]
    e = err.astype(np.float64)
    out, sades, o = np.zeros((len(sizes), 6)), np.zeros((K, len(sizes))), 0
    for s, n in enumerate(sizes):
        sade, sfde = e[:, o:o + n, 0].mean(1), e[:, o:o + n, 1].mean(1)
        sades[:, s] = sade
        kb = int(np.argmin(sade))                       # first minimum
        out[s, :2] = sade.min(), sfde.min()
        out[s, 4] = np.inf
        if clear is not None and n > 1:
            c = clear[:, o:o + n]
            flags = c < np.float32(coll)
            sclear = c.min(1)
            out[s, 2:] = (sclear < np.float32(coll)).mean(), float(sclear[kb] < np.float32(coll)), sclear.min(), flags.mean()
        o += n
    return out, sades


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run_clearance(obs, fut, sizes, inv_ss, pstride=2, with_start=True):
    from socialways_amd import ops
    K, B = fut.shape[:2]
    pos = fut
    if pstride == 4:
        pos = np.concatenate([fut, np.full_like(fut, 1e3)], axis=-1)        # columns 2, 3 must not be read
    scenes = ops.SceneIndex.get(scene_list(sizes), B, torch.device("cuda", 0))
    start = dev(obs)[:, -1] if with_start else None                          # a strided view: read in place
    out = ops.scene_clearance(dev(pos), start, scenes, K, inv_ss)
    assert out.shape == (K, B) and out.dtype == torch.float32
    return out.cpu().numpy()


# ---- 1. the clearance kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_start", [True, False])
@pytest.mark.parametrize("pstride", [2, 4])
@pytest.mark.parametrize("Tp", [1, 12, 30])
@pytest.mark.parametrize("K", [1, 3, 20])
def test_clearance_against_float64(K, Tp, pstride, with_start):
    inv_ss = 15.0
    worst = 0.0
    for seed in (3, 4, 5):
        obs, fut = crowd(SIZES, K, Tp=Tp, seed=seed)
        got = run_clearance(obs, fut, SIZES, inv_ss, pstride, with_start)
        want = clearance(obs[:, -1] if with_start else None, fut, SIZES, inv_ss)
        M = max(float(np.abs(fut).max()), float(np.abs(obs[:, -1]).max()))
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin)                       # +inf exactly where the definition has it
        assert np.array_equal(got[~fin], want[~fin])
        if Tp == 1 and not with_start:
            assert not fin.any()                                           # a path of one point has no segment
            continue
        single = np.concatenate([np.full(n, n == 1) for n in SIZES])
        assert np.array_equal(~fin, np.broadcast_to(single, fin.shape))
        e = float(np.abs(got[fin] - want[fin]).max())
        worst = max(worst, e)
        print("clearance K=%d Tp=%d stride=%d start=%d seed=%d: max |err| %.3g, bound %.3g"
              % (K, Tp, pstride, with_start, seed, e, clearance_bound(M, inv_ss)))
        assert e <= clearance_bound(M, inv_ss)
    print("clearance K=%d Tp=%d stride=%d start=%d: worst %.3g" % (K, Tp, pstride, with_start, worst))


def test_clearance_semantics_on_a_hand_made_scene():
    """Scene 0: two agents that swap positions inside one segment (both sampled distances are 2).  Scene 1: two coincident
    agents moving together (dv.dv = 0) and a third one at distance 3 from them.  Scene 2: one agent."""
    sizes = [2, 3, 1]
    last = np.array([[0, 0], [2, 0], [5, 5], [5, 5], [5, 8], [9, 9]], np.float32)
    step = np.array([[2, 0], [-2, 0], [1, 1], [1, 1], [1, 1], [0, 1]], np.float32)
    fut = (last[:, None] + step[:, None] * np.arange(1, 3, dtype=np.float32)[None, :, None])[None]      # (1, 6, 2, 2)
    obs = np.repeat(last[:, None], 2, axis=1)
    tol = clearance_bound(11.0, 1.0)

    def check(got, want):
        want = np.asarray([want], np.float32)
        assert got.shape == want.shape and np.isinf(got[0, 5]) and got[0, 5] > 0, got
        assert np.abs(got[:, :5] - want[:, :5]).max() <= tol, got
    for pstride in (2, 4):
        check(run_clearance(obs, fut, sizes, 1.0, pstride), [0, 0, 0, 0, 3, np.inf])
    assert np.array_equal(clearance(last, fut, sizes, 1.0), np.array([[0, 0, 0, 0, 3, np.inf]]))
    # without the start point only the second segment is left: the swapped agents move apart from distance 2
    check(run_clearance(obs, fut, sizes, 0.5, 2, with_start=False), [1, 1, 0, 0, 1.5, np.inf])
    assert np.array_equal(clearance(None, fut, sizes, 0.5), np.array([[1, 1, 0, 0, 1.5, np.inf]]))


def test_stats_scene_clearance_is_the_public_form():
    from socialways_amd import stats
    obs, fut = crowd(SIZES, 3)
    sb = scene_list(SIZES)
    want = run_clearance(obs, fut, SIZES, 2.0)
    got = stats.scene_clearance(fut, sb, start=obs[:, -1], scale=2.0)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    four = np.concatenate([fut, np.zeros_like(fut)], -1)
    assert np.array_equal(stats.scene_clearance(torch.from_numpy(four), sb, start=obs[:, -1], scale=2.0).cpu().numpy(), want)
    one = stats.scene_clearance(fut[1], sb, start=obs[:, -1], scale=2.0)
    assert one.shape == (fut.shape[1],) and np.array_equal(one.cpu().numpy(), want[1])
    free = stats.scene_clearance(fut, sb)                                   # no start point: Tp - 1 segments
    assert_close(free.cpu().numpy()[:, 1:6], clearance(None, fut, SIZES, 1.0)[:, 1:6], 0, clearance_bound(2.0, 1.0))
    alone = stats.scene_clearance(fut, [])                                  # [] = one scene of all agents
    assert_close(alone.cpu().numpy(), clearance(None, fut, [fut.shape[1]], 1.0), 0, clearance_bound(2.0, 1.0))
    for bad in (fut[..., :1], fut[0, 0], np.zeros((2, 5, 3, 3), np.float32)):
        with pytest.raises(ValueError):
            stats.scene_clearance(bad, [])
    with pytest.raises(ValueError):
        stats.scene_clearance(fut, sb, start=obs[:3, -1])


# ---- 2. the collision flags against float64, away from the threshold ------------------------------------------------------
@pytest.mark.parametrize("coll", [0.1, 0.2, 0.5])
@pytest.mark.parametrize("seed", [3, 4, 5])
def test_collision_flags_against_float64(seed, coll):
    inv_ss, K = 15.0, 20
    obs, fut = crowd(SIZES, K, seed=seed)
    got = run_clearance(obs, fut, SIZES, inv_ss)
    want = clearance(obs[:, -1], fut, SIZES, inv_ss)
    M = max(float(np.abs(fut).max()), float(np.abs(obs[:, -1]).max()))
    fin = np.isfinite(want)
    far = fin & (np.abs(want - coll) > 4 * clearance_bound(M, inv_ss))
    left_out = 1.0 - far.sum() / fin.sum()
    share = (want[fin] < coll).mean()
    print("flags seed=%d coll=%.1f: %d finite, %.3f %% left out, %.1f %% collide" % (seed, coll, fin.sum(), 100 * left_out, 100 * share))
    assert left_out <= 0.01
    assert 0.035 <= share < 0.345                       # 4 - 34 % in whole per cent (float64 alone): both outcomes are exercised
    assert np.array_equal(got[far] < np.float32(coll), want[far] < coll)


# ---- 3. the scene reduction -----------------------------------------------------------------------------------------------
def run_reduce(err, clear, sizes, coll, want_best=True):
    from socialways_amd import _lib as L
    from socialways_amd import ops
    K, B = err.shape[:2]
    scenes = ops.SceneIndex.get(scene_list(sizes), B, torch.device("cuda", 0))
    e, c = dev(err), None if clear is None else dev(clear)
    per_scene, best = ops.scene_reduce(e, c, scenes, K, coll)
    assert per_scene.shape == (len(sizes), 6) and best.shape == (len(sizes),) and best.dtype == torch.int32
    again, best2 = ops.scene_reduce(e, c, scenes, K, coll)
    assert torch.equal(per_scene, again) and torch.equal(best, best2)           # fixed order: identical bits
    if not want_best:                                                          # best may be NULL
        ps = torch.full_like(per_scene, 7.0)
        L.call("sw_scene_reduce", L.ptr(e), L.ptr(c), L.ptr(scenes.scene_off), scenes.S, B, K, float(coll), L.ptr(ps), None, L.stream())
        assert torch.equal(ps, per_scene)
    return per_scene.cpu().numpy(), best.cpu().numpy()


def check_reduce(got, best, err, clear, sizes, coll):
    want, sades = scene_reference(err, clear, sizes, coll)
    K = err.shape[0]
    assert ((0 <= best) & (best < K)).all()
    at_best = sades[best, np.arange(len(sizes))]
    assert_close(at_best, sades.min(0), 1e-5, 0, "sade at the returned kbest")          # by value, not by index
    assert_close(got[:, :2], want[:, :2], 1e-5, 0, "jade, jfde")
    assert_close(got[:, 2], want[:, 2], 1e-5, 0, "share of colliding draws")
    assert_close(got[:, 5], want[:, 5], 1e-5, 0, "share of colliding (draw, agent)")
    assert np.array_equal(got[:, 4], want[:, 4].astype(np.float32)), "min_k sclear is exact"
    if clear is not None:                    # the flag of the RETURNED draw, exact
        o = np.concatenate([[0], np.cumsum(sizes)])
        flag = [float(n > 1 and clear[best[s], o[s]:o[s + 1]].min() < np.float32(coll)) for s, n in enumerate(sizes)]
        assert np.array_equal(got[:, 3], np.asarray(flag, np.float32))
    return want


@pytest.mark.parametrize("K", [1, 3, 20, 70])
def test_scene_reduce_against_float64(K):
    rng = np.random.RandomState(K)
    B = int(np.sum(SIZES))
    err = rng.rand(K, B, 2).astype(np.float32) + 0.1
    obs, fut = crowd(SIZES, K, seed=4)
    clear = run_clearance(obs, fut, SIZES, 15.0)
    for coll in (0.1, 0.5):
        got, best = run_reduce(err, clear, SIZES, coll, want_best=(coll == 0.1))
        want = check_reduce(got, best, err, clear, SIZES, coll)
        single = np.asarray(SIZES) == 1
        assert (got[single][:, [2, 3, 5]] == 0).all() and np.isinf(got[single][:, 4]).all()
        if K == 20:
            assert 0 < want[~single, 2].max() and want[~single, 2].min() < 1
            assert len(np.unique(best)) > 1
    got, best = run_reduce(err, None, SIZES, 0.5)                             # clear = NULL
    check_reduce(got, best, err, None, SIZES, 0.5)
    assert (got[:, [2, 3, 5]] == 0).all() and np.isinf(got[:, 4]).all()


def test_scene_reduce_first_k_on_an_exact_tie():
    rng = np.random.RandomState(0)
    K, B = 9, int(np.sum(SIZES))
    err = rng.rand(K, B, 2).astype(np.float32) + 1.0
    err[2] = err[7] = err[5] = rng.rand(B, 2).astype(np.float32) * 0.5          # three identical best draws
    clear = rng.rand(K, B).astype(np.float32)
    clear[2], clear[5], clear[7] = 1.0, 0.0, 0.0                                # only the FIRST of them does not collide
    got, best = run_reduce(err, clear, SIZES, 0.5)
    assert (best == 2).all()
    assert (got[:, 3] == 0).all()
    check_reduce(got, best, err, clear, SIZES, 0.5)


def clearances_on_the_threshold(K=20, coll=0.5):
    """err (K, B, 2) and clear (K, B) on the grid of 1/8 in [0, 1]: a ninth of the clearances EQUAL coll (a binary
    fraction: the fp32 comparison sees equality), and draw 0 of every scene has its smallest clearance exactly there."""
    rng = np.random.RandomState(8)
    B = int(np.sum(SIZES))
    err = rng.rand(K, B, 2).astype(np.float32) + 0.1
    clear = (rng.randint(0, 9, size=(K, B)) / 8.0).astype(np.float32)
    clear[0] = np.maximum(clear[0], np.float32(coll))
    clear[0, np.concatenate([[0], np.cumsum(SIZES)[:-1]])] = coll
    return err, clear, coll


def test_scene_reduce_a_clearance_equal_to_coll_dist_is_no_collision():
    """Definition 3 counts `clear < coll_dist`, strictly.  Random clearances never equal the threshold, so the seeded fault
    "`<=` in the per-agent count" (tools/mutants/scene_coll_strict.diff) passed every other case; here 11 % of the entries
    sit on it (tests/test_scene_host.py checks that the two readings differ by far more than the 1e-5 of check_reduce)."""
    err, clear, coll = clearances_on_the_threshold()
    got, best = run_reduce(err, clear, SIZES, coll)
    check_reduce(got, best, err, clear, SIZES, coll)
    got0, _ = run_reduce(err[:1], clear[:1], SIZES, coll)                       # draw 0 alone: nothing is below the threshold
    assert (got0[:, [2, 3, 5]] == 0).all()


def test_scene_c_abi_argument_checks_on_the_device():
    from socialways_amd import _lib as L
    lib = L.load()
    B, K, Tp, S = 6, 3, 12, 2
    t = lambda *s: torch.full(s, 7.0, device="cuda")
    pos, start, err, clear, ps = t(K, B, Tp, 4), t(B, 2), t(K, B, 2), t(K, B), t(S, 6)
    off = torch.tensor([0, 2, 6], dtype=torch.int32, device="cuda")
    p, st = L.ptr, L.stream()

    def cl(pos=pos, pstride=4, start=start, sstride=2, off=off, S=S, B=B, K=K, Tp=Tp, inv_ss=1.0, clear=clear):
        return lib.sw_scene_clearance(p(pos), pstride, p(start), sstride, p(off), S, B, K, Tp, inv_ss, p(clear), st)

    def rd(err=err, clear=clear, off=off, S=S, B=B, K=K, ps=ps):
        return lib.sw_scene_reduce(p(err), p(clear), p(off), S, B, K, 0.1, p(ps), None, st)
    for kw in (dict(pos=None), dict(off=None), dict(clear=None), dict(pstride=3), dict(sstride=1), dict(S=-1), dict(B=-1),
               dict(K=0), dict(Tp=0), dict(inv_ss=0.0)):
        assert cl(**kw) == -1, kw
    for kw in (dict(err=None), dict(off=None), dict(ps=None), dict(S=-1), dict(B=-1), dict(K=0)):
        assert rd(**kw) == -1, kw
    assert cl(B=0) == 0 and cl(S=0) == 0 and rd(B=0) == 0 and rd(S=0) == 0
    torch.cuda.synchronize()
    for out in (clear, ps):          # nothing was launched
        assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    assert cl(start=None) == 0 and rd() == 0
    torch.cuda.synchronize()
    assert float(clear.max()) == 0.0 and float(ps[:, 2].min()) == 1.0           # every agent sits on every other one


# ---- 4. against the reference's own samples -------------------------------------------------------------------------------
def test_scene_metrics_on_the_reference_samples():
    """tests/golden/test_eval.npz: noise and pred_hat of the unmodified reference for two held-out scenes, K = 4."""
    from socialways_amd import ops
    g, data, tr = eval_golden()
    K, G = 4, tr.G
    inv_ss = 1.0 / float(data.ss)
    for s, (a, b) in enumerate(data.test_batches):
        a, b = int(a), int(b)
        n = b - a
        noise = torch.from_numpy(np.stack([g["noise.%d.%d" % (s, k)] for k in range(K)])).cuda()
        obsv, gt = data.obsv[a:b], data.pred[a:b]
        pred4 = G.sample(obsv, K, 12, [], noise)
        assert pred4.shape == (K, n, 12, 4)
        scenes = ops.SceneIndex.get(np.asarray([[0, n]]), n, obsv.device)
        _, (_, _, err) = ops.gen_sample(G.encoder.packed(), G.feature_embedder.packed(), G.attention.packed(), G.decoder.packed(),
                                        obsv, noise.reshape(K * n, 32), scenes, 12, True, K, gt=gt, inv_ss=inv_ss,
                                        want_pred=False)
        per_scene, kbest, clear = ops.scene_metrics(err, pred4.reshape(K * n, 12, 4), obsv, scenes, K, 12, inv_ss, 0.1)
        ref = np.stack([g["pred_hat.%d.%d" % (s, k)] for k in range(K)])[..., :2].astype(np.float64)      # (K, n, 12, 2)
        last = obsv[:, -1].cpu().numpy()
        M = max(float(np.abs(ref).max()), float(np.abs(last).max()))
        pos_tol = RT * M + AT                                       # positions against the reference (test_gpu_sample.py)
        want = clearance(last, ref, [n], inv_ss)
        e = np.abs(clear.cpu().numpy() - want).max()
        print("golden scene %d: clearance max |err| %.3g (tolerance %.3g)" % (s, e, 2 * pos_tol * inv_ss + clearance_bound(M, inv_ss)))
        assert e <= 2 * pos_tol * inv_ss + clearance_bound(M, inv_ss)         # 1-Lipschitz in each of the two positions
        d = np.sqrt(((ref - gt.cpu().numpy().astype(np.float64)[None]) ** 2).sum(-1)) * inv_ss
        sade, sfde = d.mean(2).mean(1), d[:, :, -1].mean(1)
        got = per_scene.cpu().numpy()[0]
        assert_close(got[0], sade.min(), 1e-5, pos_tol * inv_ss, "jade")      # an error is 1-Lipschitz in its position
        assert_close(got[1], sfde.min(), 1e-5, pos_tol * inv_ss, "jfde")
        assert_close(sade[int(kbest[0])], sade.min(), 1e-5, 2 * pos_tol * inv_ss, "sade at kbest")


# ---- 5. evaluate_scenes ---------------------------------------------------------------------------------------------------
def records_reference(records, K, coll, n_test_samples):
    """Every joint / collision number of evaluate_scenes() in float64 from the records: collision flags from the records'
    fp32 `clear`, errors recomputed from the denormalised trajectories (world units)."""
    n_j = n_f = 0.0
    joint = best = agent = 0.0
    n_multi = agents_multi = 0
    for r in records:
        c = r["clear"]
        n = c.shape[1]
        d = np.sqrt(((r["preds_our"].astype(np.float64) - r["preds_gtt"].astype(np.float64)[None]) ** 2).sum(-1))   # (K, n, Tp)
        sade, sfde = d.mean(2).mean(1), d[:, :, -1].mean(1)
        n_j += n * sade.min()
        n_f += n * sfde.min()
        if n > 1:
            flags = c < np.float32(coll)
            n_multi += 1
            agents_multi += n
            joint += flags.any(1).mean()
            best += float(flags[r["kbest"]].any())
            agent += n * flags.mean()
    z = max(n_multi, 1)
    return dict(jade_min=n_j / n_test_samples, jfde_min=n_f / n_test_samples, col_joint=joint / z, col_best=best / z,
                col_agent=agent / max(agents_multi, 1), n_scenes=len(records), n_multi=n_multi)


def check_evaluate_scenes(tr, data, K, coll, just_one=False, bitwise=True, seed=31):
    torch.manual_seed(seed)
    four = tr.evaluate(data, n_gen_samples=K, just_one=just_one)
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    recs = []
    res = tr.evaluate_scenes(data, n_gen_samples=K, coll_dist=coll, just_one=just_one, collect=recs)
    assert torch.equal(torch.get_rng_state(), state)                           # the host noise stream of evaluate()
    torch.manual_seed(seed)
    assert tr.evaluate_scenes(data, n_gen_samples=K, coll_dist=coll, just_one=just_one) == res      # with and without collect
    got4 = (res["ade_avg"], res["fde_avg"], res["ade_min"], res["fde_min"])
    if bitwise:
        assert got4 == tuple(four)
    else:
        assert_close(np.asarray(got4), np.asarray(four), 1e-5, 0, "marginal numbers at a generic width")
    one = 1 + 4 * EPS
    assert res["ade_min"] <= res["jade_min"] * one and res["jade_min"] <= res["ade_avg"] * one
    assert res["fde_min"] <= res["jfde_min"] * one and res["jfde_min"] <= res["fde_avg"] * one
    batches = [(int(a), int(b)) for a, b in data.test_batches][:1 if just_one else None]
    assert len(recs) == len(batches) and res["n_scenes"] == len(batches)
    inv_ss = 1.0 / float(data.ss)
    gt_flags = []
    for r, (a, b) in zip(recs, batches):
        n = b - a
        assert r["clear"].shape == (K, n) and r["per_scene"].shape == (6,) and 0 <= r["kbest"] < K
        assert sorted(r) == ["clear", "kbest", "obsvs", "per_scene", "preds_gtt", "preds_lnr", "preds_our", "timestamp"]
        M = max(float(np.abs(r["preds_our"]).max()), float(np.abs(r["obsvs"]).max()))
        want = clearance(r["obsvs"][:, -1], r["preds_our"], [n], 1.0)          # world coordinates: scale 1
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(r["clear"]), fin) and fin.all() == (n > 1)
        if n > 1:
            assert np.abs(r["clear"] - want).max() <= 32 * EPS * M, (np.abs(r["clear"] - want).max(), 32 * EPS * M)
        # the ground truth: float64 on data.pred, flags compared where the threshold is not within the rounding bound
        o, p = data.obsv[a:b].cpu().numpy(), data.pred[a:b].cpu().numpy()
        g = clearance(o[:, -1], p[None], [n], inv_ss)[0].min()
        if n > 1:
            Mn = max(float(np.abs(o).max()), float(np.abs(p).max()))
            assert abs(g - coll) > 4 * clearance_bound(Mn, inv_ss), "ground truth of a scene sits on the threshold: choose another coll_dist"
            gt_flags.append(float(g < coll))
    want = records_reference(recs, K, coll, data.n_test_samples)
    M = max(float(np.abs(r["preds_our"]).max()) for r in recs)
    for k in ("jade_min", "jfde_min"):                   # recomputed from denormalised positions: one rounding each
        assert_close(res[k], want[k], 1e-5, 32 * EPS * M, k)
    for k in ("col_joint", "col_best", "col_agent"):
        assert_close(res[k], want[k], 1e-5, 0, k)
    assert res["n_multi"] == want["n_multi"] == len(gt_flags)
    assert res["col_gt"] == (float(np.mean(gt_flags)) if gt_flags else 0.0)
    # the record's per_scene row is the kernel's: its joint errors are those of the record
    for r in recs:
        d = np.sqrt(((r["preds_our"].astype(np.float64) - r["preds_gtt"].astype(np.float64)[None]) ** 2).sum(-1))
        assert_close(r["per_scene"][0], d.mean(2).mean(1).min(), 1e-5, 32 * EPS * M, "record jade")
        assert_close(d.mean(2).mean(1)[r["kbest"]], d.mean(2).mean(1).min(), 1e-5, 64 * EPS * M, "record kbest")
    return res, recs


def synth_set(sizes, n_scenes, seed=99):
    import socialways_amd as sw
    tracks = sw.synth_tracks(n_scenes, sizes, seed=seed)
    return sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], tracks["times"], device="cuda:0")


def test_evaluate_scenes_on_the_reference_set():
    g, data, tr = eval_golden()
    res, _ = check_evaluate_scenes(tr, data, 4, 0.1, seed=123)
    assert_close(np.asarray([res[k] for k in ("ade_avg", "fde_avg", "ade_min", "fde_min")]), g["metrics"], 2e-5, 2e-6, "reference metrics")
    assert res["n_scenes"] == 2 and res["n_multi"] == 2


@pytest.mark.parametrize("K,just_one,chunk", [(20, False, None), (20, False, 700), (1, False, None), (20, True, None)])
def test_evaluate_scenes_on_eight_agent_scenes(K, just_one, chunk):
    import socialways_amd as sw
    data = synth_set(8, 60)
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0")
    if chunk:
        tr.TEST_CHUNK = chunk
    res, _ = check_evaluate_scenes(tr, data, K, 0.2, just_one)
    assert res["n_multi"] == res["n_scenes"] == (1 if just_one else len(data.test_batches))
    if K == 1:
        assert_close(res["jade_min"], res["ade_min"], 1e-6, 0, "K = 1")
        assert_close(res["jade_min"], res["ade_avg"], 1e-6, 0, "K = 1")
        assert_close(res["jfde_min"], res["fde_min"], 1e-6, 0, "K = 1")


def ragged_set(largest=70):
    """The held-out fifth is the ragged SIZES of test_gpu_sample.py, its largest scene resized to `largest` agents."""
    import socialways_amd as sw
    held_out = [largest if n == max(SIZES) else n for n in SIZES]
    sizes = sw.ragged_scene_sizes(100, 8, seed=11) + [23, 1, 70, 6, 2, 17, 9, 1, 30] + held_out
    data = synth_set(sizes, len(sizes))
    assert [int(b - a) for a, b in data.test_batches] == held_out
    return data


def test_evaluate_scenes_on_ragged_scenes():
    """A chunk mixes scene sizes: single agents, more than one tile, more than 64 agents."""
    import socialways_amd as sw
    data = ragged_set()
    sizes = [int(b - a) for a, b in data.test_batches]
    assert 1 in sizes and max(sizes) > 64 and len(set(sizes)) > 4
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0")
    res, recs = check_evaluate_scenes(tr, data, 20, 0.2)
    assert 0 < res["n_multi"] < res["n_scenes"]
    assert res["jade_min"] > res["ade_min"]                                   # one k per scene is not one k per agent


def test_evaluate_scenes_at_a_generic_width():
    import socialways_amd as sw
    from socialways_amd import generic
    data = ragged_set(largest=40)                 # the generic social block takes scenes of up to 64 agents
    torch.manual_seed(2)
    tr = sw.SocialWaysTrainer(12, hidden_size=80, use_social=True, device="cuda:0")
    assert isinstance(tr, generic.GenericTrainer)
    check_evaluate_scenes(tr, data, 5, 0.2, bitwise=False)
