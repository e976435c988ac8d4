"""numpy implementation of the WALLS section of include/socialways_hip.h, written from that comment alone: the five-candidate
closest approach of a moving point to a wall, the path-walls reduction (sw_path_walls) and the refinement objective with the
wall term (sw_plan_refine_walls; the pedestrian penalty, the quadratic terms and the iteration are tests/_refine_ref.py's) -
parameterised by dtype like _refine_ref.py, so that float64 (the reference) and float32 (the problem's own sensitivity) run the
same code - and the constructed inputs the wall tests share.  Sees nothing of the device but inputs and outputs.
TIE GAP.  Where two candidates at DIFFERENT places s on the path segment tie in |c|^2, the order decides which end point takes
the gradient, and a float32 run may decide otherwise than a float64 one.  The reference records, per case, the smallest
relative gap (|c|^2 of the runner-up - |c|^2 of the best) / |c|^2 of the runner-up over every contributing (segment, wall) pair
of the whole float64 descent; the runner-up is the best among the candidates whose s differs from the chosen one's (a
candidate with the identical s - "p1 against the wall's end" and "the wall's end against p1", both clamped - is the same
point twice); 1 without one."""
import numpy as np

import _refine_ref as R

WALLS_MAX = 1024


# ---- the closest approach -------------------------------------------------------------------------------------------------
def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def candidates(p0, p1, w0, w1, dtype):
    """p0, p1, w0, w1 (.., 2), broadcast against each other -> (s (5, ..), c (5, .., 2), cc (5, ..), ok (5, ..)): the five
    candidates in the header's order; ok = the candidate exists (the crossing only where the four cross products say so)."""
    p0, p1, w0, w1 = (np.asarray(x, dtype) for x in (p0, p1, w0, w1))
    one, zero = dtype(1), dtype(0)
    e, f = p1 - p0, w1 - w0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ee, ff = (e * e).sum(-1), (f * f).sum(-1)

        def on_wall(p):
            u = np.where(ff > 0, np.clip(((p - w0) * f).sum(-1) / np.where(ff > 0, ff, one), zero, one), zero)
            return p - (w0 + u[..., None] * f)

        def on_path(w):
            s = np.where(ee > 0, np.clip(((w - p0) * e).sum(-1) / np.where(ee > 0, ee, one), zero, one), zero)
            return s, p0 + s[..., None] * e - w

        c1, c2 = on_wall(p0), on_wall(p1)
        s3, c3 = on_path(w0)
        s4, c4 = on_path(w1)
        d1, d2 = _cross(f, p0 - w0), _cross(f, p1 - w0)
        d3, d4 = _cross(e, w0 - p0), _cross(e, w1 - p0)
        crossing = (((d1 < 0) & (d2 > 0)) | ((d1 > 0) & (d2 < 0))) & (((d3 < 0) & (d4 > 0)) | ((d3 > 0) & (d4 < 0)))
        s5 = np.where(crossing, d1 / np.where(crossing, d1 - d2, one), zero)
        shape = crossing.shape
        s = np.stack([np.broadcast_to(zero, shape), np.broadcast_to(one, shape), np.broadcast_to(s3, shape),
                      np.broadcast_to(s4, shape), s5]).astype(dtype)
        c = np.stack([np.broadcast_to(x, shape + (2,)) for x in (c1, c2, c3, c4, np.zeros(shape + (2,), dtype))]).astype(dtype)
        cc = (c * c).sum(-1)
        ok = np.stack([np.ones(shape, bool)] * 4 + [crossing])
    return s, c, cc, ok


def closest(p0, p1, w0, w1, dtype=np.float64, want_gap=False):
    """-> (s (..), c (.., 2), cc (..)[, gap (..)]): the best candidate by the header's rule - the first, replaced by a later one
    only if its |c|^2 is strictly smaller (NaN replaces nothing) - and the relative tie gap of the module docstring."""
    s, c, cc, ok = candidates(p0, p1, w0, w1, dtype)
    bs, bc, bcc = s[0].copy(), c[0].copy(), cc[0].copy()
    with np.errstate(invalid="ignore"):
        for i in range(1, 5):
            lt = ok[i] & (cc[i] < bcc)
            bs, bcc = np.where(lt, s[i], bs), np.where(lt, cc[i], bcc)
            bc = np.where(lt[..., None], c[i], bc)
        if not want_gap:
            return bs, bc, bcc
        other = np.where(ok & (s != bs[None]), cc, np.inf).min(0)                   # the runner-up at another place on the path
        gap = np.where(np.isfinite(other) & (other > 0), (other - bcc) / np.where(other > 0, other, 1), np.where(other == 0, 0.0, 1.0))
    return bs, bc, bcc, gap


def brute_force(p0, p1, w0, w1, n=1001):
    """The smallest |p(s) - w(u)|^2 over a dense (s, u) grid, float64: one pair."""
    p0, p1, w0, w1 = (np.asarray(x, np.float64) for x in (p0, p1, w0, w1))
    g = np.linspace(0.0, 1.0, n)
    P = p0[None] + g[:, None] * (p1 - p0)[None]
    W = w0[None] + g[:, None] * (w1 - w0)[None]
    return float((((P[:, None] - W[None]) ** 2).sum(-1)).min())


# ---- sw_path_walls ----------------------------------------------------------------------------------------------------------
def path_walls_reference(pos, start, walls, dist, inv_ss=1.0, lens=None, dtype=np.float64):
    """pos (K, B, Tp, >= 2), start (B, >= 2) or None, walls (M, 2, 2), lens (B,) or None -> dict(clear (K, B), first (K, B) int64,
    nseg (K, B) int64, margin: the smallest |d - dist| / dist over every counted segment-wall distance d).  The comparison with
    dist is made against its fp32 value.  Walls are taken 64 at a time: the (K, B, segments, M) table is never formed."""
    pos = np.asarray(pos)[..., :2].astype(dtype)
    K, B, Tp = pos.shape[:3]
    walls = np.asarray(walls, dtype).reshape(-1, 2, 2)
    M = walls.shape[0]
    first = 0 if start is not None else 1
    PA = pos if start is None else np.concatenate([np.broadcast_to(np.asarray(start, dtype)[None, :, None, :2], (K, B, 1, 2)), pos], 2)
    NS = PA.shape[2] - 1
    la = np.full(B, Tp) if lens is None else np.clip(np.asarray(lens).astype(np.int64), 1, Tp)
    on = (np.arange(NS)[None, :] + first) < la[:, None]                             # (B, NS): the segment's frame t < len
    clear = np.full((K, B), np.inf, dtype)
    nseg, any_t, margin = np.zeros((K, B), np.int64), np.zeros((K, B, NS), bool), np.inf
    lim = dtype(np.float32(dist))
    for m0 in range(0, M if NS else 0, 64):
        w = walls[m0:m0 + 64]
        _, _, cc = closest(PA[:, :, :-1, None], PA[:, :, 1:, None], w[None, None, None, :, 0], w[None, None, None, :, 1], dtype)
        with np.errstate(invalid="ignore"):
            d = np.where(on[None, :, :, None], np.sqrt(cc) * dtype(inv_ss), np.inf)     # (K, B, NS, <= 64)
        assert not np.isnan(d).any(), "a counted NaN does not occur in the cases"
        hit = d < lim
        clear = np.minimum(clear, d.min((2, 3)))
        nseg += hit.sum((2, 3))
        any_t |= hit.any(3)
        if dist > 0:
            margin = min(margin, float(np.abs(d[np.isfinite(d)].astype(np.float64) - float(lim)).min(initial=np.inf)) / float(lim))
    tfirst = np.where(any_t.any(2), any_t.argmax(2) + first, -1) if NS else np.full((K, B), -1)
    return dict(clear=clear, first=tfirst.astype(np.int64), nseg=nseg, margin=margin)


# ---- sw_plan_refine_walls -----------------------------------------------------------------------------------------------------
def wall_penalty(PX, walls, dw, dtype, want_gap=False):
    """PX (T + 1, 2) the plan with its start point in front, walls (M, 2, 2) -> (wal, g (T, 2), share (T, M, 2, 2), gap): the
    wall penalty sum, the sum over the walls of -4 u (s c of segment t + (1 - s) c of segment t + 1) per waypoint t = 1 .. T, the
    two end points' shares of every pair (.., 0, :) to the segment's first end, (.., 1, :) to its second, and the smallest tie gap
    over the contributing pairs."""
    T = PX.shape[0] - 1
    g = np.zeros((T, 2), dtype)
    if walls.shape[0] == 0:
        return dtype(0), g, np.zeros((T, 0, 2, 2), dtype), 1.0
    r = closest(PX[:-1, None], PX[1:, None], walls[None, :, 0], walls[None, :, 1], dtype, want_gap)
    s, c, cc = r[:3]
    with np.errstate(invalid="ignore"):
        on = cc < dw * dw
        u = np.maximum(dtype(0), dtype(1) - cc / (dw * dw))
        phi = np.where(on, u * u, dtype(0))
        w = dtype(-4) * u[..., None] * c
        g1 = np.where(on[..., None], s[..., None] * w, dtype(0))                    # (T, M, 2): to the segment's second end
        g0 = np.where(on[..., None], (dtype(1) - s[..., None]) * w, dtype(0))       # to its first end
    g += g1.sum(1)
    g[:-1] += g0[1:].sum(1)                                                         # x_0 is data: the first segment's g0 goes nowhere
    gap = float(np.where(on, r[3], 1.0).min()) if want_gap else 1.0
    return phi.sum(), g, np.stack([g0, g1], 2), gap


def one_plan(A, lim, X0, xs, d0, walls, dw, w_wall, n_iter, lr, w_track, w_smooth, max_move, dtype):
    """_refine_ref.one_plan with the wall term -> (X, cost (2, 4), moved, step0, J, gap)."""
    A, X0, xs, walls = A.astype(dtype), X0.astype(dtype), xs.astype(dtype), walls.astype(dtype)
    d0, dw, lr, w_track, w_smooth = dtype(d0), dtype(dw), dtype(lr), dtype(w_track), dtype(w_smooth)
    cap = dtype(max_move) * d0
    ww = dtype(w_wall) * (d0 * d0 / (dw * dw))
    X = X0.copy()
    cost = np.zeros((2, 4), dtype)
    J, step0, gap = [], None, 1.0
    for it in range(n_iter + 1):
        pen, g = R.penalty(A, lim, X, xs, d0, dtype)
        trk, smo, gt, gs = R.quadratic(X, X0, xs)
        wal, gw, _, gp = wall_penalty(np.concatenate([xs[None], X], 0), walls, dw, dtype, want_gap=dtype is np.float64)
        gap = min(gap, gp)
        J.append(float(pen) + (float(w_track) * float(trk) + float(w_smooth) * float(smo)) / float(d0) ** 2 + float(w_wall) * float(wal))
        row = np.array([pen, trk / (d0 * d0), smo / (d0 * d0), wal], dtype)
        full = g + ww * gw + w_track * gt + w_smooth * gs
        if it == 0:
            cost[0] = row
            step0 = full
        if it == n_iter:
            cost[1] = row
            break
        step = lr * full
        norm = np.sqrt((step * step).sum(-1))
        with np.errstate(invalid="ignore", divide="ignore"):
            step = np.where((norm > cap)[:, None], step * (cap / norm)[:, None], step)
        X = X - step
    moved = np.sqrt(((X - X0) ** 2).sum(-1)).max()
    return X, cost, moved, step0, J, gap


def refine_walls_reference(case, d0, walls, dw, w_wall=1.0, dtype=np.float64, **descent):
    """case: a dict of _refine_ref.refine_case(); walls (M, 2, 2) in the coordinates of the case -> dict(out, cost (Q, P, 2, 4),
    moved - times inv_ss -, step0, J, n_other, gap: the smallest tie gap of the case (float64 runs; 1 otherwise))."""
    par = dict(R.DEFAULTS, **descent)
    pos, plans = np.asarray(case["pos"]), np.asarray(case["plans"])
    walls = np.asarray(walls, np.float64).reshape(-1, 2, 2)
    K, B, Tp = pos.shape[:3]
    Q, P = plans.shape[:2]
    sizes = case["sizes"]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    st = np.broadcast_to(np.asarray(case["start"])[None, :, None, :2], (K, B, 1, 2))
    A = np.concatenate([st, pos[..., :2]], axis=2)
    la = np.full(B, Tp) if case["lens"] is None else np.clip(np.asarray(case["lens"]).astype(np.int64), 1, Tp)
    out, cost, moved = np.zeros((Q, P, Tp, 2), dtype), np.zeros((Q, P, 2, 4), dtype), np.zeros((Q, P), dtype)
    step0, J, n_other, gap = np.zeros((Q, P, Tp, 2), dtype), [], np.zeros(Q, np.int64), 1.0
    for q in range(Q):
        s = int(case["q_scene"][q])
        ego = -1 if case["q_ego"] is None else int(case["q_ego"][q])
        rows = np.array([r for r in range(off[s], off[s + 1]) if r != ego] if 0 <= s < len(sizes) else [], np.int64)
        n_other[q] = len(rows)
        for p in range(P):
            X, c, m, s0, j, gp = one_plan(A[:, rows], la[rows], plans[q, p], np.asarray(case["plan_start"])[q, :2], d0, walls, dw,
                                          w_wall, par["n_iter"], par["lr"], par["w_track"], par["w_smooth"], par["max_move"], dtype)
            out[q, p], cost[q, p], moved[q, p], step0[q, p] = X, c, m * dtype(case["inv_ss"]), s0
            J.append(j)
            gap = min(gap, gp)
    return dict(out=out, cost=cost, moved=moved, step0=step0, J=J, n_other=n_other, gap=gap)


# ---- constructed inputs: paths against walls --------------------------------------------------------------------------------
DIST = 0.5
BOX = 32.0


def paths_case(K, B, Tp, M, seed, pstride=2, with_start=False, ragged=False, inv_ss=1.0, near=24):
    """K * B random walks in a BOX x BOX world (steps of about half a unit, one step in eight motionless), M walls: at most
    `near` of them inside the box - lengths up to 3 units, every fourth a post, the first pinned with one end ON a path point
    and the second through one (endpoint touches) - scattered over the indices 0 .. M - 1 with the first and the last index
    among them; the others far outside, where their distances decide nothing.  Coordinates are multiples of 1 / 64 (in world
    units), so touches are exact; pos = world / inv_ss."""
    rng = np.random.RandomState(seed)
    p0 = rng.randint(0, int(BOX * 64), (K, B, 1, 2)) / 64.0
    step = rng.randint(-48, 49, (K, B, Tp + 1, 2)) / 64.0
    step[rng.rand(K, B, Tp + 1) < 0.125] = 0.0                                      # motionless segments
    world = p0 + np.cumsum(step, 2)                                                 # frame -1 (the start), then 0 .. Tp - 1
    walls = np.zeros((M, 2, 2))
    n_near = min(M, near)
    idx = np.sort(np.concatenate([[0, M - 1][:min(M, 2)], 1 + rng.permutation(max(M - 2, 0))[:max(n_near - 2, 0)]])).astype(int) \
        if M else np.zeros(0, int)
    far = np.setdiff1d(np.arange(M), idx)
    walls[far, 0] = 4 * BOX + rng.randint(0, int(BOX * 64), (len(far), 2)) / 64.0
    walls[far, 1] = walls[far, 0] + rng.randint(-128, 129, (len(far), 2)) / 64.0
    for n, i in enumerate(idx):
        w0 = rng.randint(0, int(BOX * 64), 2) / 64.0
        w1 = w0 + (0 if n % 4 == 3 else 1) * rng.randint(-192, 193, 2) / 64.0
        k, a, t = rng.randint(K), rng.randint(B), rng.randint(1, Tp + 1)
        if n == 0:                                                                  # one end on a path point
            w0 = world[k, a, t].copy()
        if n == 1:                                                                  # the wall's middle on a path point
            half = rng.randint(1, 65, 2) / 64.0
            w0, w1 = world[k, a, t] - half, world[k, a, t] + half
        walls[i] = [w0, w1]
    pos = np.zeros((K, B, Tp, pstride), np.float32)
    pos[..., :2] = world[:, :, 1:] / inv_ss
    if pstride == 4:
        pos[..., 2:] = rng.rand(K, B, Tp, 2)
    start = None
    if with_start:
        start = np.ascontiguousarray(world[0, :, 0] / inv_ss).astype(np.float32)    # one start point per agent, as the K draws have
    lens = None
    if ragged:
        lens = rng.randint(1, Tp + 1, B).astype(np.int32)
        for a in range(B):
            pos[:, a, lens[a]:] = np.nan
    return dict(pos=pos, start=start, walls=(walls / inv_ss).astype(np.float32), lens=lens, K=K, B=B, Tp=Tp, M=M, inv_ss=inv_ss,
                dist=DIST)


def path_cases():
    """(name, case): K * B of 1, 63, 64, 65 and 257; Tp of 1, 12, 17 and 33 (two time chunks); both row strides; with and
    without a start point; ragged lengths with NaN padding; M of 0, 1, 33 and WALLS_MAX."""
    return [("r1_tp12_m33", paths_case(1, 1, 12, 33, seed=1, with_start=True)),
            ("r63_tp12_m1024", paths_case(3, 21, 12, WALLS_MAX, seed=2, pstride=4)),
            ("r64_tp17_m33_start", paths_case(4, 16, 17, 33, seed=3, with_start=True, inv_ss=2.0)),
            ("r65_tp33_m33_ragged", paths_case(5, 13, 33, 33, seed=4, ragged=True, pstride=4, inv_ss=0.5)),
            ("r257_tp33_m33_start_ragged", paths_case(1, 257, 33, 33, seed=5, with_start=True, ragged=True)),
            ("r257_tp12_m1", paths_case(257, 1, 12, 1, seed=6)),
            ("r65_tp1_m33_start", paths_case(5, 13, 1, 33, seed=7, with_start=True)),
            ("r65_tp1_m33", paths_case(5, 13, 1, 33, seed=8)),
            ("r64_tp12_m0", paths_case(2, 32, 12, 0, seed=9, with_start=True)),
            ("r260_tp17_m33_dense", paths_case(20, 13, 17, 33, seed=10, with_start=True, near=33))]


def run_path_reference(case, dtype=np.float64):
    return path_walls_reference(case["pos"], case["start"], case["walls"], case["dist"], case["inv_ss"], case["lens"], dtype)


# ---- constructed inputs: refinement with walls ------------------------------------------------------------------------------
DW_WORLD = 0.4
W_WALL = 1.0


def walls_near_plans(case, M, seed, near=10):
    """M walls in the coordinates of the case.  At most `near` of them - scattered over the indices 0 .. M - 1, the first and the
    last among them - lie beside a random waypoint of a random plan: the middle 0.15 .. 0.45 world units off the waypoint in a
    random direction, a random orientation, 0.2 .. 1.2 units long, every fifth a post.  The others lie ten units and more
    outside the bounding box of the plans, where they are walked and contribute nothing."""
    rng = np.random.RandomState(seed)
    plans, inv_ss = case["plans"].astype(np.float64) * case["inv_ss"], case["inv_ss"]
    Q, P, Tp = plans.shape[:3]
    hi = plans.reshape(-1, 2).max(0)
    walls = np.zeros((M, 2, 2))
    walls[:, 0] = hi + 10.0 + 5.0 * rng.rand(M, 2)
    walls[:, 1] = walls[:, 0] + rng.rand(M, 2) - 0.5
    idx = np.unique(np.concatenate([[0, M - 1], rng.permutation(M)[:max(min(near, M) - 2, 0)]]))[:min(near, M)]
    for n, i in enumerate(idx):
        at = plans[rng.randint(Q), rng.randint(P), rng.randint(Tp)]
        th, ph = rng.rand(2) * 2 * np.pi
        mid = at + (0.15 + 0.3 * rng.rand()) * np.array([np.cos(th), np.sin(th)])
        half = (0.0 if n % 5 == 4 else 0.1 + 0.5 * rng.rand()) * np.array([np.cos(ph), np.sin(ph)])
        walls[i] = [mid - half, mid + half]
    return (walls / inv_ss).astype(np.float32)


def long_walls_near_plans(case, M, seed, near=12):
    """M walls of which `near` - at random indices, so that they fall into many wall slices - are LONG ones across the plans:
    each passes 0.1 .. 0.3 world units beside a random waypoint of a random plan at 25 .. 65 degrees to the plan's direction
    there and reaches 3 .. 5 units to either side, so that its ends lie far outside the wall distance of every plan and only
    its interior (and crossings) ever contributes: no wall end slides along a plan, and the tie gap stays wide with many
    contributing walls.  The others lie far outside, as in walls_near_plans."""
    rng = np.random.RandomState(seed)
    plans, inv_ss = case["plans"].astype(np.float64) * case["inv_ss"], case["inv_ss"]
    start = np.asarray(case["plan_start"], np.float64)[:, :2] * inv_ss
    Q, P, Tp = plans.shape[:3]
    hi = plans.reshape(-1, 2).max(0)
    walls = np.zeros((M, 2, 2))
    walls[:, 0] = hi + 10.0 + 5.0 * rng.rand(M, 2)
    walls[:, 1] = walls[:, 0] + rng.rand(M, 2) - 0.5
    for i in rng.permutation(M)[:near]:
        q, p, t = rng.randint(Q), rng.randint(P), rng.randint(Tp)
        at = plans[q, p, t]
        d = at - (plans[q, p, t - 1] if t else start[q])
        th = np.arctan2(d[1], d[0]) + rng.choice([-1, 1]) * np.deg2rad(25 + 40 * rng.rand())
        u = np.array([np.cos(th), np.sin(th)])
        mid = at + (0.1 + 0.2 * rng.rand()) * rng.choice([-1, 1]) * np.array([-u[1], u[0]])
        walls[i] = [mid - (3 + 2 * rng.rand()) * u, mid + (3 + 2 * rng.rand()) * u]
    return (walls / inv_ss).astype(np.float32)


LONG_WALLS = ("sizes_k20_ps4_p5", 130, 19, 12)      # (refine case, walls, seed, long walls across the plans)


# (refine case of _refine_ref.constructed_cases(), walls, seed of the walls, walls beside the plans): seeds for which the
# float64 descent keeps a tie gap of 1e-3 on EVERY case (asserted in tests/test_walls_host.py).  Few walls lie beside the
# plans - the others are walked and contribute nothing -, because every wall END that comes near a plan slides along it
# during the descent, and a wall's end that passes a waypoint closely is a near-tie; the case whose 50 plans share their
# walls takes one
REFINE_WALLS = [("sizes_k20_ps2", 1, 1001, 3), ("sizes_k20_ps2", 7, 1000, 3), ("sizes_k20_ps2", 130, 1011, 3),
                ("sizes_k20_ps4_p5", 130, 1009, 3), ("k1", 7, 1009, 3), ("k65_tp17_ragged_x2", 130, 1162, 3),
                ("k65_tp33_ragged_half", 7, 1001, 3), ("k260_n3", 1, 1000, 3), ("tp1", 7, 1000, 3), ("queries", 130, 2000, 1)]


def refine_cases():
    """(name, case): the constructed cases of _refine_ref with walls (1, 7 and 130 of them), wall_d0 and w_wall."""
    base = dict(R.constructed_cases())
    out = []
    for name, M, seed, near in REFINE_WALLS:
        case = dict(base[name])
        case.update(walls=walls_near_plans(case, M, seed, near), wall_d0=DW_WORLD / case["inv_ss"], w_wall=W_WALL)
        out.append(("%s_m%d" % (name, M), case))
    name, M, seed, near = LONG_WALLS
    case = dict(base[name])
    case.update(walls=long_walls_near_plans(case, M, seed, near), wall_d0=DW_WORLD / case["inv_ss"], w_wall=W_WALL)
    out.append(("%s_m%d_long" % (name, M), case))
    return out


def run_refine_reference(case, dtype=np.float64, **descent):
    return refine_walls_reference(case, case["d0"], case["walls"], case["wall_d0"], case["w_wall"], dtype=dtype, **descent)


# ---- the corridor: pedestrians on one side of a straight plan, a wall on the other --------------------------------------------
CORRIDOR = dict(dist=0.5, coll_dist=0.1, wall_off=0.3, w_wall=1.0)


def corridor_case(K=8, Tp=12, n=3, seed=0):
    """A straight plan along +x at y = 0; n oncoming pedestrians walk along -x at y = +0.15 .. +0.25 (K draws with a little
    jitter), and a wall runs along y = -0.6 dist = -0.3 under the whole plan.  Without the wall term the descent pushes the
    plan away from the pedestrians - into the wall."""
    rng = np.random.RandomState(seed)
    t = np.arange(0, Tp + 1)
    plan = np.stack([0.4 * t, np.zeros(Tp + 1)], 1)                                 # point 0 = the start
    ped = np.zeros((K, n, Tp + 1, 2))
    for a in range(n):
        x0 = 0.4 * Tp * (a + 1.5) / (n + 1)
        ped[:, a, :, 0] = x0 + 2.0 - 0.4 * t[None] + rng.uniform(-0.05, 0.05, (K, 1))
        ped[:, a, :, 1] = 0.15 + 0.1 * a / max(n - 1, 1) + rng.uniform(-0.02, 0.02, (K, Tp + 1))
    ped[:, :, 0] = ped[:1, :, 0]                                                    # one start point per agent
    walls = np.array([[[-1.0, -CORRIDOR["wall_off"]], [0.4 * Tp + 1.0, -CORRIDOR["wall_off"] + 1.0 / 64]]], np.float32)
    return dict(pos=ped[:, :, 1:].astype(np.float32), start=ped[0, :, 0].astype(np.float32), plans=plan[None, None, 1:].astype(np.float32),
                plan_start=plan[None, 0].astype(np.float32), lens=None, sizes=[n], K=K, Tp=Tp, inv_ss=1.0,
                q_scene=np.zeros(1, np.int32), q_ego=None, d0=CORRIDOR["dist"], walls=walls, wall_d0=CORRIDOR["dist"],
                w_wall=CORRIDOR["w_wall"])


def parallel_case(Tp=6):
    """An exactly parallel corridor and nobody else: a straight plan along +x at y = 0 with equal steps, one wall along
    y = -0.25 from under the first waypoint to beyond the last - every segment but the first ties between s = 0 and s = 1; the
    first (whose first end, the start point, is data and takes no gradient) has the wall's end under its second end alone, so
    the sum of the step over the waypoints does not depend on who wins a tie."""
    t = np.arange(0, Tp + 1)
    plan = np.stack([0.5 * t, np.zeros(Tp + 1)], 1)
    far = np.full((2, 1, Tp, 2), 100.0, np.float32)                                 # one pedestrian, far away
    return dict(pos=far, start=np.full((1, 2), 100.0, np.float32), plans=plan[None, None, 1:].astype(np.float32),
                plan_start=plan[None, 0].astype(np.float32), lens=None, sizes=[1], K=2, Tp=Tp, inv_ss=1.0,
                q_scene=np.zeros(1, np.int32), q_ego=None, d0=0.5, walls=np.array([[[0.5, -0.25], [0.5 * Tp + 1.0, -0.25]]], np.float32),
                wall_d0=0.5, w_wall=1.0)
