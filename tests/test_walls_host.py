"""Walls without a GPU: the numpy reference (tests/_walls_ref.py, written from the header comment) against brute force and
central differences, the conditions on the INPUTS of the GPU tests (asserted here, on the reference, so that a GPU test cannot
hide behind them), the corridor scenario, the argument checks of sw_path_walls and sw_plan_refine_walls through the C ABI
(they return before the device is touched) and the argument errors of the Python layers."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _refine_ref as R
import _walls_ref as W

ONE = dict(n_iter=1, lr=1.0, w_track=0.05, w_smooth=0.02, max_move=1e6)      # tests/test_gpu_refine.py's
REFINE = dict(W.refine_cases())


@functools.lru_cache(maxsize=None)
def reference(name, one):
    return W.run_refine_reference(REFINE[name], **(ONE if one else {}))


# ---- the closest approach --------------------------------------------------------------------------------------------------
def hand_pairs():
    """(p0, p1, w0, w1, the squared distance where it is known): crossings, touches, posts, motionless segments, collinear."""
    return [((0, 0), (2, 0), (1, -1), (1, 1), 0.0),             # a proper crossing
            ((0, 0), (2, 0), (1, 0), (1, 1), 0.0),              # the wall's end touches the path
            ((0, 0), (1, 0), (1, -1), (1, 1), 0.0),             # the path's end touches the wall
            ((0, 0), (1, 0), (2, 0), (3, 0), 1.0),              # collinear, apart
            ((0, 0), (2, 0), (1, 0), (3, 0), 0.0),              # collinear, overlapping
            ((0, 0), (2, 0), (1, 1), (1, 1), 1.0),              # a post beside the path
            ((1, 1), (1, 1), (0, 0), (2, 0), 1.0),              # a motionless point beside a wall
            ((1, 1), (1, 1), (3, 1), (3, 1), 4.0),              # a motionless point and a post
            ((0, 0), (2, 0), (0, 1), (2, 1), 1.0),              # parallel
            ((0, 0), (2, 2), (3, 0), (5, 1), None)]


def test_closest_approach_against_brute_force():
    rng = np.random.RandomState(0)
    pairs = hand_pairs() + [tuple(rng.uniform(-1, 1, (4, 2))) + (None,) for _ in range(20)]
    worst = 0.0
    for p0, p1, w0, w1, known in pairs:
        p0, p1, w0, w1 = (np.asarray(x, np.float64) for x in (p0, p1, w0, w1))
        s, c, cc = W.closest(p0, p1, w0, w1)
        brute = W.brute_force(p0, p1, w0, w1)
        grid = (np.linalg.norm(p1 - p0) + np.linalg.norm(w1 - w0)) / 2000.0      # a grid point within half a step of the optimum
        assert cc <= brute + 1e-12 and np.sqrt(brute) - np.sqrt(cc) <= grid + 1e-12, (p0, p1, w0, w1, cc, brute)
        assert known is None or abs(cc - known) <= 1e-12
        assert 0.0 <= s <= 1.0 and abs((c * c).sum() - cc) <= 1e-15
        # c is the path point at s minus a point of the wall
        q = p0 + s * (p1 - p0) - c
        f = w1 - w0
        u = 0.0 if not f.any() else np.clip(((q - w0) * f).sum() / (f * f).sum(), 0, 1)
        assert np.abs(w0 + u * f - q).max() <= 1e-9
        worst = max(worst, np.sqrt(brute) - np.sqrt(cc))
    print("closest approach against a 1001 x 1001 grid: the grid lies at most %.3g above" % worst)


def test_the_order_of_the_candidates_decides_ties():
    s, c, cc = W.closest((0, 0), (2, 0), (0, 1), (2, 1))        # parallel: candidates 1 and 2 tie, the first stays
    assert s == 0.0 and cc == 1.0 and tuple(c) == (0.0, -1.0)
    s, c, cc = W.closest((1, 1), (1, 1), (0, 0), (2, 0))        # motionless: the same
    assert s == 0.0 and cc == 1.0
    s, c, cc = W.closest((0, 0), (2, 0), (0.5, -1), (0.5, 1))   # a crossing: c = 0, s = d1 / (d1 - d2)
    assert s == 0.25 and cc == 0.0 and not c.any()
    nan = float("nan")
    s, c, cc = W.closest((0, 0), (nan, nan), (0, 1), (2, 1))    # NaN replaces nothing: candidate 1 does not read p1
    assert s == 0.0 and cc == 1.0


# ---- the closed-form gradient is the gradient of the penalty --------------------------------------------------------------
def test_wall_gradient_against_central_differences():
    worst = 0.0
    for name in ("sizes_k20_ps2_m7", "k1_m7", "tp1_m7", "k65_tp17_ragged_x2_m130"):
        case = REFINE[name]
        dw = float(case["wall_d0"])
        walls = case["walls"].astype(np.float64)
        h = 1e-6 * dw
        for q in range(min(case["plans"].shape[0], 3)):
            for p in range(case["plans"].shape[1]):
                PX = np.concatenate([case["plan_start"][q:q + 1, :2], case["plans"][q, p]], 0).astype(np.float64)
                wal, g, share, _ = W.wall_penalty(PX, walls, dw, np.float64)
                assert np.allclose(share[:-1, :, 1].sum(1) + share[1:, :, 0].sum(1), g[:-1], atol=1e-12)      # the shares add up to g
                num = np.zeros_like(g)
                for t in range(1, PX.shape[0]):
                    for d in range(2):
                        up, dn = PX.copy(), PX.copy()
                        up[t, d] += h
                        dn[t, d] -= h
                        num[t - 1, d] = (W.wall_penalty(up, walls, dw, np.float64)[0] - W.wall_penalty(dn, walls, dw, np.float64)[0]) / (2 * h)
                if np.abs(g).max() > 0:
                    err = np.abs(g / dw ** 2 - num).max() / (np.abs(g).max() / dw ** 2)
                    worst = max(worst, err)
                    assert err <= 1e-4, (name, q, p, err)      # phi is C1: a candidate switch inside +-h costs O(h) of a second derivative
    assert worst > 0
    print("closed-form wall gradient against central differences: largest relative difference %.3g" % worst)


def test_the_gradient_vanishes_at_a_crossing_and_at_the_rim():
    walls = np.array([[[1.0, -1.0], [1.0, 1.0]]])
    PX = np.array([[0.0, 0.0], [2.0, 0.25], [2.5, 0.25]])
    wal, g, share, _ = W.wall_penalty(PX, walls, 0.5, np.float64)
    assert not share[0].any() and wal >= 1.0                    # the crossing segment: phi = 1, gradient exactly 0
    for eps in (1e-9, -1e-9):                                    # |c| = dw: phi and its gradient pass through 0
        PX = np.array([[0.0, 0.0], [0.5 - eps, 0.0]])
        wal, g, _, _ = W.wall_penalty(PX, walls, 0.5, np.float64)
        assert 0 <= wal <= 1e-15 and np.abs(g).max() <= 1e-8 and np.isfinite(g).all()


# ---- conditions on the constructed inputs of the GPU tests, asserted on the reference ---------------------------------------
@pytest.mark.parametrize("name", list(REFINE))
def test_refine_cases_keep_a_tie_gap(name):
    """Every general-position case, none left out: best against second-best |c|^2 over all contributing (segment, wall) pairs
    along the whole float64 descent and at the single iteration, a relative gap >= 1e-3 - only a candidate at the IDENTICAL s
    is not a runner-up -, so no flip between float32 and float64 decides where a gradient goes."""
    r32, r1 = reference(name, False), reference(name, True)
    print("%s: tie gap %.3g (32 iterations) %.3g (one)" % (name, r32["gap"], r1["gap"]))
    assert r32["gap"] >= 1e-3 and r1["gap"] >= 1e-3
    assert (r32["cost"][..., 0, 3] > 0).any(), "walls contribute"
    J = np.array(r32["J"])
    assert (J[:, -1] <= J[:, 0]).all() and np.isfinite(r32["out"]).all()


def test_refine_cases_cover_the_wall_counts():
    assert sorted({REFINE[n]["walls"].shape[0] for n in REFINE}) == [1, 7, 130]
    assert {n.rsplit("_m", 1)[0] for n in REFINE} == {n for n, _ in R.constructed_cases()}


@functools.lru_cache(maxsize=None)
def path_reference(name, dtype):
    return W.run_path_reference(dict(W.path_cases())[name], dtype)


@pytest.mark.parametrize("name", [n for n, _ in W.path_cases()])
def test_path_cases_decide_their_integers(name):
    """No |c| * inv_ss within a relative 1e-4 of dist, so first and nseg are decided; the float32 reference agrees."""
    r, r32 = path_reference(name, np.float64), path_reference(name, np.float32)
    print("%s: margin %.3g, %d pairs closer than dist, %d paths at distance 0" % (name, r["margin"], r["nseg"].sum(), (r["clear"] == 0).sum()))
    assert r["margin"] >= 1e-4
    assert np.array_equal(r["first"], r32["first"]) and np.array_equal(r["nseg"], r32["nseg"])


def test_path_cases_cover_the_shapes():
    cases = dict(W.path_cases())
    assert {c["K"] * c["B"] for c in cases.values()} >= {1, 63, 64, 65, 257}
    assert {c["Tp"] for c in cases.values()} >= {1, 12, 17, 33}
    assert {c["M"] for c in cases.values()} >= {0, 1, 33, W.WALLS_MAX}
    assert {c["pos"].shape[-1] for c in cases.values()} == {2, 4}
    assert any(c["start"] is None for c in cases.values()) and any(c["start"] is not None for c in cases.values())
    assert any(c["lens"] is not None and np.isnan(c["pos"]).any() for c in cases.values())
    hits = sum(int(path_reference(n, np.float64)["nseg"].sum()) for n in cases)
    zeros = sum(int((path_reference(n, np.float64)["clear"] == 0).sum()) for n in cases)
    assert hits > 500 and zeros > 50, "conflicts, and crossings or touches, occur"
    big = path_reference("r63_tp12_m1024", np.float64)
    assert (big["first"] >= 0).any()


# ---- M = 0 is the refinement without walls -----------------------------------------------------------------------------------
def test_no_walls_reproduces_the_refine_reference():
    for name in ("queries", "k65_tp17_ragged_x2", "tp1"):
        case = dict(R.constructed_cases())[name]
        for dtype in (np.float64, np.float32):
            a = R.refine_reference(case, case["d0"], dtype=dtype)
            b = W.refine_walls_reference(case, case["d0"], np.zeros((0, 2, 2)), case["d0"], 1.0, dtype=dtype)
            assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["moved"], b["moved"])
            assert np.array_equal(a["cost"], b["cost"][..., :3]) and not b["cost"][..., 3].any()
            assert np.array_equal(a["step0"], b["step0"])
    case = REFINE["queries_m130"]
    still = W.run_refine_reference(case, n_iter=0)
    assert np.array_equal(still["out"], case["plans"].astype(np.float64)) and np.array_equal(still["cost"][:, :, 0], still["cost"][:, :, 1])


# ---- the corridor ------------------------------------------------------------------------------------------------------------
def test_the_corridor_scenario():
    case, C = W.corridor_case(), W.CORRIDOR
    none = W.refine_walls_reference(case, case["d0"], np.zeros((0, 2, 2)), case["wall_d0"], 0.0)
    with_w = W.run_refine_reference(case)

    def clearance(out):
        return float(W.path_walls_reference(out[0][None], case["plan_start"], case["walls"], C["coll_dist"])["clear"][0, 0])

    before = clearance(case["plans"].astype(np.float64))
    c_none, c_with = clearance(none["out"]), clearance(with_w["out"])
    print("corridor: plan-to-wall clearance %.3f before, %.3f refined without walls, %.3f with; pedestrian penalty %.3f -> %.3f / %.3f"
          % (before, c_none, c_with, with_w["cost"][0, 0, 0, 0], none["cost"][0, 0, 1, 0], with_w["cost"][0, 0, 1, 0]))
    assert abs(before - 0.6 * C["dist"]) <= 0.02                 # the wall runs 0.6 dist from the plan
    assert c_none < C["coll_dist"] < c_with
    assert with_w["cost"][0, 0, 1, 0] < with_w["cost"][0, 0, 0, 0] and none["cost"][0, 0, 1, 0] < none["cost"][0, 0, 0, 0]


# ---- the entry points refuse bad arguments before the device is touched ------------------------------------------------------
def test_argument_validation_without_gpu():
    from socialways_amd import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15                       # host memory, 16-byte aligned: never dereferenced
    inf, nan = float("inf"), float("nan")
    good = dict(pos=p, pstride=2, start=p, sstride=2, len=None, K=4, B=0, Tp=3, walls=p, M=5, inv_ss=1.0, dist=0.5, clear=p, first=p,
                nseg=p, stream=None)

    def walls(**kw):
        a = dict(good, **kw)
        return lib.sw_path_walls(*[a[k] for k in good])

    assert walls() == 0 and walls(M=0, walls=None) == 0 and walls(start=None, sstride=0) == 0 and walls(M=L.WALLS_MAX) == 0      # B = 0: no launch
    for kw in (dict(pos=None), dict(clear=None), dict(first=None), dict(nseg=None), dict(walls=None), dict(K=0), dict(B=-1), dict(Tp=0),
               dict(M=-1), dict(pstride=3), dict(pos=p + 4), dict(sstride=1), dict(inv_ss=0.0), dict(inv_ss=nan), dict(dist=-1.0),
               dict(dist=nan)):
        assert walls(**kw) == -1, kw
    assert walls(M=L.WALLS_MAX + 1) == -2 and L.WALLS_MAX >= 1024
    for kw in (dict(pstride=3), dict(pos=p + 4), dict(sstride=1), dict(inv_ss=0.0), dict(clear=None)):
        assert walls(M=L.WALLS_MAX + 1, **kw) == -1, kw          # the argument checks come first

    good = dict(pos=p, pstride=2, start=p, sstride=2, scene_off=p, len=None, S=1, B=2, K=4, Tp=3, plans=p, plan_start=p,
                q_scene=p, q_ego=None, Q=0, P=2, inv_ss=1.0, d0=0.5, n_iter=4, lr=0.1, w_track=0.05, w_smooth=0.5, max_move=0.5,
                walls=p, M=3, dw=0.4, w_wall=1.0, out=p, cost=p, moved=p, stream=None)

    def refine(**kw):
        a = dict(good, **kw)
        return lib.sw_plan_refine_walls(*[a[k] for k in good])

    assert refine() == 0 and refine(M=0, walls=None) == 0 and refine(w_wall=0.0) == 0 and refine(M=L.WALLS_MAX, Tp=1024) == 0      # Q = 0
    for kw in (dict(pos=None), dict(out=None), dict(walls=None), dict(M=-1), dict(dw=0.0), dict(dw=-1.0), dict(dw=nan), dict(dw=inf),
               dict(dw=1e-30), dict(dw=1e30), dict(w_wall=-1.0), dict(w_wall=nan), dict(w_wall=inf), dict(w_wall=1e38, dw=1e-3, d0=1e3),
               dict(d0=0.0), dict(lr=-0.1), dict(n_iter=1025), dict(pstride=3)):
        assert refine(**kw) == -1, kw
    for kw in (dict(start=None), dict(sstride=1), dict(pos=p + 4), dict(plans=p + 4), dict(d0=1e-30), dict(d0=1e30), dict(d0=inf), dict(d0=nan)):
        assert refine(**kw) == -1 and refine(M=L.WALLS_MAX + 1, **kw) == -1, kw      # the argument checks come first
    for kw in (dict(M=L.WALLS_MAX + 1), dict(K=4097), dict(Tp=1025)):
        assert refine(**kw) == -2, kw


def test_the_python_layers_refuse_bad_arguments_and_cpu_tensors():
    import socialways_amd as sw
    from socialways_amd import ops, stats
    K, B, Tp, Q, P = 3, 4, 5, 2, 2
    pos, walls = torch.zeros(K, B, Tp, 2), torch.zeros(6, 2, 2)
    for kw in (dict(walls=torch.zeros(W.WALLS_MAX + 1, 2, 2)), dict(walls=torch.zeros(6, 4)), dict(walls=walls.double()), dict(dist=-1.0),
               dict(inv_ss=0.0), dict(start=torch.zeros(B + 1, 2)), dict(lens=torch.zeros(B)), dict(K=2)):
        with pytest.raises(ValueError):
            ops.path_walls(**dict(dict(pos=pos, start=None, K=K, walls=walls, dist=0.5), **kw))
    with pytest.raises(sw.SocialWaysHipError):                  # checked arguments on the CPU: refused, never computed on the host
        ops.path_walls(pos, None, K, walls, 0.5)
    with pytest.raises(sw.SocialWaysHipError):
        stats.path_walls(np.zeros((B, Tp, 2)), np.zeros((6, 4)), 0.5, device="cpu")
    for kw in (dict(walls=np.zeros((6, 3))), dict(dist=-1.0), dict(scale=0.0), dict(trajs=np.zeros((Tp, 2))), dict(lens=[1, 2, 3, 9])):
        with pytest.raises(ValueError):
            stats.path_walls(**dict(dict(trajs=np.zeros((K, B, Tp, 2)), walls=np.zeros((6, 2, 2)), dist=0.5, device="cpu"), **kw))

    scenes = ops.SceneIndex.get([[0, 2], [2, 4]], B, "cpu")
    qs = torch.tensor([0, 1], dtype=torch.int32)
    a = dict(pos=pos, start=torch.zeros(B, 2), scenes=scenes, K=K, plans=torch.zeros(Q, P, Tp, 2), plan_start=torch.zeros(Q, 2), q_scene=qs,
             q_ego=None, d0=0.5, walls=walls)
    for kw in (dict(walls=torch.zeros(W.WALLS_MAX + 1, 2, 2)), dict(walls=torch.zeros(6, 4)), dict(wall_d0=0.0), dict(wall_d0=float("nan")),
               dict(wall_d0=1e-30), dict(w_wall=-1.0), dict(w_wall=float("inf")), dict(lr=1.0)):
        with pytest.raises(ValueError):
            ops.plan_refine(**dict(a, **kw))
    with pytest.raises(sw.SocialWaysHipError):
        ops.plan_refine(**a)
    with pytest.raises(sw.SocialWaysHipError):
        ops.plan_refine(**dict(a, walls=torch.zeros(0, 2, 2), wall_d0=0.3, w_wall=0.0))
    assert ops.check_descent(0.5, wall_d0=0.4, w_wall=2.0) == ops.check_descent(0.5) == (0.5, 32, 0.1, 0.05, 0.5, 0.5)
    with pytest.raises(TypeError):
        ops.check_descent(0.5, plan_lens=3)
    s = dict(trajs=np.zeros((K, B, Tp, 2)), sub_batches=[[0, 2], [2, 4]], plans=np.zeros((Q, P, Tp, 2)), dist=0.5,
             plan_start=np.zeros((Q, 2)), start=np.zeros((B, 2)), device="cpu", walls=np.zeros((6, 4)))
    for kw in (dict(walls=np.zeros((6, 3))), dict(wall_dist=0.0), dict(w_wall=-1.0), dict(lr=1.0)):
        with pytest.raises(ValueError):
            stats.refine_plans(**dict(s, **kw))
    with pytest.raises(sw.SocialWaysHipError):
        stats.refine_plans(**s)
