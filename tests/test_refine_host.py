"""Plan refinement without a GPU: the numpy reference (tests/_refine_ref.py, written from the header comment) against torch
float64 autograd of the same objective, its behaviour on the constructed cases the GPU tests use (conditions on the INPUTS,
asserted on the reference), sw_plan_refine's argument checks through the C ABI (they return before the device is touched),
and the argument errors of the Python layers."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _refine_ref as R


# ---- the closed-form gradient is the gradient of J ---------------------------------------------------------------------------
def torch_objective(A, lim, X, X0, xs, d0, w_track, w_smooth):
    """J of include/socialways_hip.h in torch float64, nothing shared with the reference: A (K, m, T + 1, 2), X (T, 2)."""
    K, m, T = A.shape[0], A.shape[1], X.shape[0]
    PX = torch.cat([xs[None], X], 0)
    pen = X.sum() * 0
    for s in range(1, T + 1):
        r0, r1 = A[:, :, s - 1] - PX[s - 1], A[:, :, s] - PX[s]
        dv = r1 - r0
        dd, rd = (dv * dv).sum(-1), (r0 * dv).sum(-1)
        tau = torch.where(dd > 0, (-rd / torch.where(dd > 0, dd, torch.ones_like(dd))).clamp(0, 1), torch.zeros_like(dd))
        c = r0 + tau[..., None] * dv
        u = (1 - (c * c).sum(-1) / d0 ** 2).clamp(min=0)
        on = torch.as_tensor(s <= lim)[None, :].expand(K, m)
        pen = pen + torch.where(on, u * u, torch.zeros_like(u)).sum() / K
    trk = ((X - X0) ** 2).sum()
    acc = PX[2:] - 2 * PX[1:-1] + PX[:-2]
    return pen + w_track / d0 ** 2 * trk + w_smooth / d0 ** 2 * (acc * acc).sum()


def test_closed_form_gradient_against_autograd():
    worst = 0.0
    for name in ("queries", "k65_tp17_ragged_x2", "tp1"):
        case = dict(R.constructed_cases())[name]
        d0 = case["d0"]
        ref = R.refine_reference(case, d0, n_iter=1, lr=1.0, w_track=0.05, w_smooth=0.02, max_move=1e6)
        K, B, Tp = case["pos"].shape[:3]
        off = np.concatenate([[0], np.cumsum(case["sizes"])])
        A = np.concatenate([np.broadcast_to(case["start"][None, :, None, :2], (K, B, 1, 2)), np.nan_to_num(case["pos"][..., :2])], 2)
        la = np.full(B, Tp) if case["lens"] is None else np.clip(case["lens"], 1, Tp)
        for q in range(case["plans"].shape[0]):
            s = int(case["q_scene"][q])
            ego = -1 if case["q_ego"] is None else int(case["q_ego"][q])
            rows = [r for r in range(off[s], off[s + 1]) if r != ego] if 0 <= s < len(case["sizes"]) else []
            for p in range(case["plans"].shape[1]):
                X0 = torch.tensor(case["plans"][q, p], dtype=torch.float64)
                X = X0.clone().requires_grad_(True)
                J = torch_objective(torch.tensor(A[:, rows], dtype=torch.float64), la[rows], X, X0,
                                    torch.tensor(case["plan_start"][q, :2], dtype=torch.float64), d0, 0.05, 0.02)
                J.backward()
                want = X.grad.numpy() * d0 ** 2                 # step0 = d0^2 dJ/dx
                got = ref["step0"][q, p]
                worst = max(worst, float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)))
                assert np.abs(got - want).max() <= 1e-9 * max(np.abs(want).max(), 1.0), (name, q, p)
                assert abs(ref["J"][q * case["plans"].shape[1] + p][0] - J.item()) <= 1e-12 * max(1.0, abs(J.item()))
    print("closed form against autograd: largest relative difference %.3g" % worst)


def test_no_iteration_is_the_identity():
    case = dict(R.constructed_cases())["queries"]
    for dtype in (np.float64, np.float32):
        r = R.refine_reference(case, case["d0"], dtype=dtype, n_iter=0)
        assert np.array_equal(r["out"], case["plans"].astype(dtype)) and not r["moved"].any()
        assert np.array_equal(r["cost"][:, :, 0], r["cost"][:, :, 1]) and not r["cost"][..., 1].any()


# ---- conditions on the constructed inputs, asserted on the reference ---------------------------------------------------------
def test_the_descent_lowers_the_objective_on_every_constructed_case():
    for name, case in R.constructed_cases():
        r = R.refine_reference(case, case["d0"])
        J = np.array(r["J"])
        assert J.shape[1] == 33 and (J[:, -1] <= J[:, 0]).all(), name
        cost = r["cost"]
        assert (cost[..., 0, 0] > 0).mean() >= 0.5, (name, (cost[..., 0, 0] > 0).mean())
        assert not cost[..., 0, 1].any() and np.abs(cost[..., 0, 2]).max() <= 1e-8, "straight plans: the start costs the penalty alone"
        assert np.isfinite(r["out"]).all() and (cost[..., 1, 0] <= cost[..., 0, 0]).all(), name
        none = r["n_other"] == 0                                 # no agent: no penalty, nothing to move a straight plan
        assert not cost[none][..., 0].any() and np.abs(r["out"][none] - case["plans"][none]).max(initial=0.0) <= 1e-6
        # no waypoint moves further than max_move d0 per iteration
        assert (r["moved"] <= 32 * 0.5 * case["d0"] * case["inv_ss"] * (1 + 1e-12)).all()
    names = [n for n, _ in R.constructed_cases()]
    assert {"queries", "tp1", "k1", "k260_n3"} <= set(names)


# ---- sw_plan_refine refuses bad arguments before the device is touched -----------------------------------------------------
def test_argument_validation_without_gpu():
    from socialways_amd import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15                       # host memory, 16-byte aligned: never dereferenced
    good = dict(pos=p, pstride=2, start=p, sstride=2, scene_off=p, len=None, S=1, B=2, K=4, Tp=3, plans=p, plan_start=p,
                q_scene=p, q_ego=None, Q=1, P=2, inv_ss=1.0, d0=0.5, n_iter=4, lr=0.1, w_track=0.05, w_smooth=0.5, max_move=0.5,
                out=p, cost=p, moved=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sw_plan_refine(*[a[k] for k in good])

    assert call(Q=0) == 0                                        # SW_OK without a launch
    assert call(Q=0, n_iter=0, lr=0.0, w_track=0.0, w_smooth=0.0, max_move=0.0) == 0
    assert call(Q=0, n_iter=1024, K=4096, Tp=1024) == 0
    for name in ("pos", "start", "scene_off", "plans", "plan_start", "q_scene", "out", "cost", "moved"):
        assert call(**{name: None}) == -1, name
    inf, nan = float("inf"), float("nan")
    for kw in (dict(S=-1), dict(B=-1), dict(Q=-1), dict(K=0), dict(Tp=0), dict(P=0), dict(pstride=3), dict(pstride=1),
               dict(pos=p + 4), dict(plans=p + 4), dict(sstride=1), dict(inv_ss=0.0), dict(inv_ss=-1.0), dict(inv_ss=nan),
               dict(n_iter=-1), dict(n_iter=1025), dict(d0=0.0), dict(d0=-1.0), dict(d0=nan), dict(d0=inf), dict(d0=1e-30),
               dict(d0=1e30), dict(lr=-0.1), dict(lr=nan), dict(lr=inf), dict(w_track=-1.0), dict(w_track=nan), dict(w_smooth=-1.0),
               dict(w_smooth=inf), dict(max_move=-0.5), dict(max_move=nan), dict(max_move=inf)):
        assert call(**kw) == -1, kw
        assert "Q" in kw or call(**dict(kw, Q=0)) == -1, kw      # the checks come before the early return
    for kw in (dict(K=4097), dict(Tp=1025)):
        assert call(**kw) == -2 and call(**dict(kw, Q=0)) == -2, kw      # SW_ESHAPE


# ---- the Python layers: errors before any launch, no CPU fallback ----------------------------------------------------------
BAD_DESCENT = (dict(n_iter=-1), dict(n_iter=1025), dict(n_iter=2.5), dict(lr=-0.1), dict(lr=float("nan")), dict(w_track=-1.0),
               dict(w_smooth=float("inf")), dict(max_move=-1.0), dict(lr=1.0), dict(lr=0.1, w_smooth=0.5, w_track=3.0),
               dict(lr=0.5, w_smooth=0.125, w_track=0.0))      # the last: lr (2 w_track + 32 w_smooth) = 2 exactly


def test_ops_and_stats_refuse_bad_arguments_and_cpu_tensors():
    import socialways_amd as sw
    from socialways_amd import ops
    K, B, Tp, Q, P = 3, 4, 5, 2, 2
    scenes = ops.SceneIndex.get([[0, 2], [2, 4]], B, "cpu")
    pos, plans = torch.zeros(K, B, Tp, 2), torch.zeros(Q, P, Tp, 2)
    start, pstart = torch.zeros(B, 2), torch.zeros(Q, 2)
    qs = torch.tensor([0, 1], dtype=torch.int32)
    a = dict(pos=pos, start=start, scenes=scenes, K=K, plans=plans, plan_start=pstart, q_scene=qs, q_ego=None, d0=0.5)
    for kw in (dict(d0=0.0), dict(d0=-1.0), dict(d0=float("nan")), dict(d0=1e-30), dict(inv_ss=0.0), dict(plans=torch.zeros(Q, P, Tp + 1, 2)),
               dict(plans=torch.zeros(Q, P, Tp, 3)), dict(plans=torch.zeros(Q, 0, Tp, 2)), dict(plans=plans.double()),
               dict(plan_start=None), dict(start=None), dict(start=None, plan_start=None), dict(plan_start=torch.zeros(Q + 1, 2)),
               dict(q_scene=qs.long()), dict(q_scene=qs[:1]), dict(q_ego=torch.zeros(Q)), dict(lens=torch.zeros(B)),
               dict(pos=torch.zeros(K, B + 1, Tp, 2)), dict(plans=plans[0], q_scene=qs)) + BAD_DESCENT:
        with pytest.raises(ValueError):
            ops.plan_refine(**dict(a, **kw))
    with pytest.raises(sw.SocialWaysHipError):                  # checked arguments on the CPU: refused, never computed on the host
        ops.plan_refine(**a)
    with pytest.raises(sw.SocialWaysHipError):
        ops.plan_refine(**dict(a, n_iter=0, lr=0.0, w_track=0.0, w_smooth=0.0, max_move=0.0))
    assert ops.check_descent(0.5) == (0.5, 32, 0.1, 0.05, 0.5, 0.5) and ops.check_descent(0.5, **ops.DESCENT_DEFAULTS)[1] == 32

    s = dict(trajs=np.zeros((K, B, Tp, 2)), sub_batches=[[0, 2], [2, 4]], plans=np.zeros((Q, P, Tp, 2)), dist=0.5,
             plan_start=np.zeros((Q, 2)), start=np.zeros((B, 2)), device="cpu")
    for kw in (dict(dist=0.0), dict(dist=float("inf")), dict(scale=0.0), dict(plans=np.zeros((3, P, Tp, 2))), dict(scene=[0, 1, 1]),
               dict(scene=[0.5, 1.0]), dict(ego=[0]), dict(start=None), dict(plan_start=None), dict(start=np.zeros((B + 1, 2))),
               dict(lens=[1, 2, 3, 9]), dict(trajs=np.zeros((B, Tp, 2)))) + BAD_DESCENT:
        with pytest.raises(ValueError):
            sw.stats.refine_plans(**dict(s, **kw))
    with pytest.raises(TypeError):
        sw.stats.refine_plans(**dict(s, plan_lens=[1, 2]))      # there is no plan length
    with pytest.raises(sw.SocialWaysHipError):
        sw.stats.refine_plans(**s)
    with pytest.raises(sw.SocialWaysHipError):
        sw.stats.refine_plans(**dict(s, plans=np.zeros((3, P, Tp, 2)), scene=[0, 1, 1], ego=[-1, 2, 0], plan_start=np.zeros((3, 2)),
                                     lens=[1, 2, 3, 5], scale=2.0, n_iter=3))


def test_the_trainers_refuse_bad_arguments_before_anything_is_sampled():
    import socialways_amd as sw
    from socialways_amd import generic, wide
    me = types.SimpleNamespace(_device_noise=lambda noise: None, device="cpu", n_next=5)      # no generator: sampling would raise AttributeError
    data = types.SimpleNamespace(ss=1.0)
    obsv, plans = torch.zeros(4, 8, 2), torch.zeros(2, 3, 5, 2)
    sb = [[0, 2], [2, 4]]
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        good = dict(obsv_p=obsv, plans=plans, n_samples=6, dist=0.5, sub_batches=sb, ego=[0, 3])
        for kw in (dict(dist=0.0), dict(dist=float("nan")), dict(coll_dist=-1.0), dict(n_samples=0), dict(scale=0.0),
                   dict(plans=torch.zeros(2, 3, 4, 2)), dict(plans=torch.zeros(3, 3, 5, 2)), dict(ego=None), dict(ego=[0, 4]), dict(ego=[0]),
                   dict(plan_start=torch.zeros(2, 2)), dict(ego=None, plan_start=torch.zeros(3, 2)), dict(scene=[0, 2]),
                   dict(scene=[0, 1, 1]), dict(sub_batches=[])) + BAD_DESCENT:
            with pytest.raises(ValueError):
                cls.refine_plans(me, **dict(good, **kw))
        with pytest.raises(sw.SocialWaysHipError):              # CPU observations: refused before the generator is touched
            cls.refine_plans(me, **good)
        with pytest.raises(sw.SocialWaysHipError):
            cls.refine_plans(me, **dict(good, ego=None, plan_start=torch.zeros(2, 2), scene=[1, 1], coll_dist=0.1, n_iter=0))
        for kw in (dict(coll_dist=-1.0), dict(coll_dist=float("nan")), dict(dist=0.0), dict(dist=float("nan"))) + BAD_DESCENT:
            with pytest.raises(ValueError):
                cls.evaluate_refine(me, data, n_gen_samples=6, **kw)
