"""numpy implementation of sw_plan_refine, written from the comment in include/socialways_hip.h alone: the objective, its
closed-form gradient, the capped iteration and the three outputs - parameterised by dtype, so that float64 (the reference)
and float32 (what an honest fp32 computation gives: the tests' measure of the problem's own sensitivity) run the same code -
and the constructed inputs the refine tests share.  Sees nothing of the device but inputs and outputs."""
import numpy as np

from _risk_ref import risk_case

DEFAULTS = dict(n_iter=32, lr=0.1, w_track=0.05, w_smooth=0.5, max_move=0.5)


def penalty(A, lim, X, xs, d0, dtype):
    """A (K, m, T + 1, 2) pedestrian paths (start point first), lim (m,) countable segments, X (T, 2) waypoints, xs (2,) the
    plan's start -> (pen, g (T, 2)): the expected penalty and d0^2 * its gradient.  Gated by selects: NaN behind lim is dropped."""
    T = X.shape[0]
    g = np.zeros((T, 2), dtype)
    if A.shape[1] == 0:
        return dtype(0), g
    K = A.shape[0]
    PX = np.concatenate([xs[None], X], 0)                                          # (T + 1, 2)
    r0 = A[:, :, :-1] - PX[None, None, :-1]
    r1 = A[:, :, 1:] - PX[None, None, 1:]
    dv = r1 - r0
    on = np.arange(T)[None, None, :] < lim[None, :, None]                          # (1, m, T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dd, rd = (dv * dv).sum(-1), (r0 * dv).sum(-1)
        tau = np.where(dd > 0, np.clip(-rd / np.where(dd > 0, dd, dtype(1)), dtype(0), dtype(1)), dtype(0))
        c = r0 + tau[..., None] * dv
        u = np.maximum(dtype(0), dtype(1) - (c * c).sum(-1) / (d0 * d0))
        on = on & (u > 0)                                                          # NaN compares false
        phi = np.where(on, u * u, dtype(0))
        w = dtype(4) * u[..., None] * c
        g1 = np.where(on[..., None], tau[..., None] * w, dtype(0)).sum((0, 1))     # to the segment's end point x_s, s = 1 .. T
        g0 = np.where(on[..., None], (dtype(1) - tau[..., None]) * w, dtype(0)).sum((0, 1))      # to x_{s-1}
    g += g1 / dtype(K)
    g[:-1] += g0[1:] / dtype(K)                                                    # x_0 is data: g0[0] goes nowhere
    return phi.sum() / dtype(K), g


def quadratic(X, X0, xs):
    """-> (trk, smo, gtrk (T, 2), gsmo (T, 2)): the two sums and their gradients."""
    T = X.shape[0]
    d = X - X0
    PX = np.concatenate([xs[None], X], 0)
    acc = np.zeros((T + 2, 2), X.dtype)                                            # acc[i], i = 0 .. T + 1; zero outside 1 .. T - 1
    if T > 1:
        acc[1:T] = PX[2:] - 2 * PX[1:-1] + PX[:-2]
    gs = 2 * (acc[0:T] - 2 * acc[1:T + 1] + acc[2:T + 2])
    return (d * d).sum(), (acc * acc).sum(), 2 * d, gs


def one_plan(A, lim, X0, xs, d0, n_iter, lr, w_track, w_smooth, max_move, dtype):
    """-> (X (T, 2), cost (2, 3), moved in the units of X, step0: the first iteration's uncapped step / lr = d0^2 dJ/dx at X0,
    J: the objective before every iteration and after the last)."""
    A, X0, xs = A.astype(dtype), X0.astype(dtype), xs.astype(dtype)
    d0, lr, w_track, w_smooth, cap = dtype(d0), dtype(lr), dtype(w_track), dtype(w_smooth), dtype(max_move) * dtype(d0)
    X = X0.copy()
    cost = np.zeros((2, 3), dtype)
    J, step0 = [], None
    for it in range(n_iter + 1):
        pen, g = penalty(A, lim, X, xs, d0, dtype)
        trk, smo, gt, gs = quadratic(X, X0, xs)
        J.append(float(pen) + float(w_track) * float(trk) / float(d0) ** 2 + float(w_smooth) * float(smo) / float(d0) ** 2)
        row = np.array([pen, trk / (d0 * d0), smo / (d0 * d0)], dtype)
        if it == 0:
            cost[0] = row
            step0 = g + w_track * gt + w_smooth * gs
        if it == n_iter:
            cost[1] = row
            break
        step = lr * (g + w_track * gt + w_smooth * gs)
        norm = np.sqrt((step * step).sum(-1))
        with np.errstate(invalid="ignore", divide="ignore"):
            step = np.where((norm > cap)[:, None], step * (cap / norm)[:, None], step)
        X = X - step
    moved = np.sqrt(((X - X0) ** 2).sum(-1)).max()
    return X, cost, moved, step0, J


def refine_reference(case, d0, dtype=np.float64, **descent):
    """case: a dict of refine_case().  -> dict(out (Q, P, Tp, 2), cost (Q, P, 2, 3), moved (Q, P) - times inv_ss -, step0
    (Q, P, Tp, 2), J: a list of n_iter + 1 objective values per (q, p), n_other (Q,))."""
    par = dict(DEFAULTS, **descent)
    pos, plans = np.asarray(case["pos"]), np.asarray(case["plans"])
    K, B, Tp = pos.shape[:3]
    Q, P = plans.shape[:2]
    sizes = case["sizes"]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    st = np.broadcast_to(np.asarray(case["start"])[None, :, None, :2], (K, B, 1, 2))
    A = np.concatenate([st, pos[..., :2]], axis=2)                                 # (K, B, Tp + 1, 2)
    la = np.full(B, Tp) if case["lens"] is None else np.clip(np.asarray(case["lens"]).astype(np.int64), 1, Tp)
    out, cost, moved = np.zeros((Q, P, Tp, 2), dtype), np.zeros((Q, P, 2, 3), dtype), np.zeros((Q, P), dtype)
    step0, J, n_other = np.zeros((Q, P, Tp, 2), dtype), [], np.zeros(Q, np.int64)
    for q in range(Q):
        s = int(case["q_scene"][q])
        ego = -1 if case["q_ego"] is None else int(case["q_ego"][q])
        rows = np.array([r for r in range(off[s], off[s + 1]) if r != ego] if 0 <= s < len(sizes) else [], np.int64)
        n_other[q] = len(rows)
        for p in range(P):
            X, c, m, s0, j = one_plan(A[:, rows], la[rows], plans[q, p], np.asarray(case["plan_start"])[q, :2], d0,
                                      par["n_iter"], par["lr"], par["w_track"], par["w_smooth"], par["max_move"], dtype)
            out[q, p], cost[q, p], moved[q, p], step0[q, p] = X, c, m * dtype(case["inv_ss"]), s0
            J.append(j)
    return dict(out=out, cost=cost, moved=moved, step0=step0, J=J, n_other=n_other)


# ---- constructed inputs ---------------------------------------------------------------------------------------------------
D0_WORLD = 0.5


def refine_case(sizes, K, Tp, seed, P=1, **kw):
    """A risk_case with a start point whose plans are replaced by STRAIGHT lines that cross the scene's lanes: plan p of query
    q runs from the start point of the case's plan (a place on the lane above the scene's agents) to a point at the horizon that has
    drifted in x as the scene's agents have and lies on a lane below, on or between theirs - so the plans have no acceleration, and what they
    cost at the start is the penalty alone.  No plan_lens: sw_plan_refine has none."""
    kw.setdefault("stride", 1)
    case = risk_case(sizes, K, Tp, seed, P=1, with_start=True, **kw)
    inv_ss = case["inv_ss"]
    Q = len(sizes)
    plans = np.zeros((Q, P, Tp, 2), np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for q, n in enumerate(sizes):
        s = case["plan_start"][q, :2].astype(np.float64)
        with np.errstate(invalid="ignore"):                                        # ragged cases: NaN behind an agent's length
            seen = np.where(np.isfinite(case["pos"][0, off[q]:off[q + 1], :, 0]))
        tl = seen[1].max()                                                         # the last frame somebody of the scene is present at
        ex = s[0] + (np.nanmean(case["pos"][0, off[q]:off[q + 1], tl, 0]) - s[0]) * Tp / (tl + 1.0)      # the scene's drift in x, carried to the horizon
        top = kw["stride"] * n                                                     # the lane the case's plan starts on
        for p in range(P):
            lane = -0.75 + top * p / max(P, 2)                                     # plan 0 ends below the lowest lane, the others fan up
            end = np.array([ex, s[1] + (lane - top) / inv_ss])
            plans[q, p] = s[None] + (end - s)[None] * (np.arange(1, Tp + 1)[:, None] / float(Tp))
    case.update(plans=plans, plan_lens=None, d0=D0_WORLD / inv_ss)
    return case


def with_queries(case, q_scene, q_ego):
    """The case asked other questions: query i = the plans of scene q_scene[i] (clamped into the case's scenes for the plans
    themselves) with q_ego[i] left out."""
    q_scene = np.asarray(q_scene, np.int32)
    src = np.clip(q_scene, 0, len(case["sizes"]) - 1)
    return dict(case, q_scene=q_scene, q_ego=None if q_ego is None else np.asarray(q_ego, np.int32),
                plans=np.ascontiguousarray(case["plans"][src]), plan_start=case["plan_start"][src].copy())


SIZES = [1, 2, 7, 33, 65]


def constructed_cases():
    """(name, case): the smallest shapes that cross every loop boundary of the kernel - one wave, under 256 lanes, agent groups,
    draw groups, two time chunks, ragged lengths with NaN padding, both row strides, every kind of query."""
    out = [("sizes_k20_ps2", refine_case(SIZES, 20, 12, seed=3, P=1, pstride=2)),
           ("sizes_k20_ps4_p5", refine_case(SIZES, 20, 12, seed=4, P=5, pstride=4)),
           ("k1", refine_case([5, 1, 9], 1, 12, seed=5, P=5, spread=3)),
           ("k65_tp17_ragged_x2", refine_case([6, 3], 65, 17, seed=6, P=5, ragged=True, inv_ss=2.0)),
           ("k65_tp33_ragged_half", refine_case([4, 9], 65, 33, seed=7, P=1, ragged=True, inv_ss=0.5, pstride=4)),
           ("k260_n3", refine_case([3], 260, 12, seed=8, P=5)),
           ("tp1", refine_case([7, 2], 20, 1, seed=9, P=5))]
    base = refine_case([4, 3, 1, 6], 8, 12, seed=10, P=5, spread=3)
    # scene 0: nobody left out / row 2 / a row of another scene; scene 3 with its rows 8 and 13; scene 1 minus row 4; a scene
    # index out of range (twice); the single-agent scene 2 whose agent (row 7) is the ego, and with it kept
    out.append(("queries", with_queries(base, [0, 0, 0, 3, 3, 1, 4, -1, 2, 2], [-1, 2, 5, 8, 13, 4, 0, -1, 7, -1])))
    return out
