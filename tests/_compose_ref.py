"""float64 numpy implementation of sw_scene_compose, written from the comment in include/socialways_hip.h alone: the cross
clearance of two draws of two agents, the selection loop, all outputs - and the constructed inputs the compose tests share.
Sees nothing of the device but inputs and outputs.  No table over all (a, j, b, k) is formed by the reference itself: an
agent's candidates are evaluated against the current selection when the loop asks for them; cross_clearances() forms the
full table of a small case for the tests that assert the gap around coll_dist."""
import numpy as np


def _paths(pos, start):
    """pos (K, B, Tp, >= 2), start (B, >= 2) or None -> float64 paths (K, B, NP, 2), NP = Tp + 1 with a start point."""
    p = np.asarray(pos)[..., :2].astype(np.float64)
    if start is None:
        return p
    s = np.asarray(start)[:, :2].astype(np.float64)
    return np.concatenate([np.broadcast_to(s[None, :, None], (p.shape[0], p.shape[1], 1, 2)), p], axis=2)


def _countable(lens, B, Tp, first):
    """Countable segments per agent: the segment ending at frame t counts while t < len; segments start at frame `first`."""
    n = np.full(B, Tp) if lens is None else np.clip(np.asarray(lens).astype(np.int64), 1, Tp)
    return n - first


def pair_min(PA, PB, lim):
    """Minimum over the first `lim` segments of the squared closest approach of paths PA, PB (.., NP, 2), broadcast against
    each other; lim (..) integers.  +inf where no segment counts; what lies behind lim - NaN included - reaches nothing."""
    r0 = PA[..., :-1, :] - PB[..., :-1, :]
    dv = (PA[..., 1:, :] - PB[..., 1:, :]) - r0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dd, rd = (dv * dv).sum(-1), (r0 * dv).sum(-1)
        tau = np.where(dd > 0, np.clip(-rd / np.where(dd > 0, dd, 1.0), 0.0, 1.0), 0.0)
        c = r0 + tau[..., None] * dv
        d2 = (c * c).sum(-1)
    on = np.arange(d2.shape[-1]) < np.asarray(lim)[..., None]
    d2 = np.where(on, d2, np.inf)
    if d2.shape[-1] == 0:
        return np.full(d2.shape[:-1], np.inf)
    return d2.min(-1)


def compose_reference(pos, start, score, sizes, coll_dist, inv_ss=1.0, sweeps=8, lens=None, err=None):
    """-> dict(sel, sel0 (B,) int32, clear (B,) float64, per_scene (S, 4) int64, per_row (B, 4) or None, kept (S,) bool: some
    agent in conflict kept its draw because no draw had fewer conflicts, stuck (S,) bool: at the end some agent's every draw
    conflicts).  The comparison with coll_dist is made against its fp32 value, as the kernel makes it."""
    P = _paths(pos, start)
    K, B, NP, _ = P.shape
    Tp = np.asarray(pos).shape[2]
    first = 0 if start is not None else 1
    v = _countable(lens, B, Tp, first)
    sc = np.asarray(score).astype(np.float64)
    coll = float(np.float32(coll_dist))
    S = len(sizes)
    sel_all, sel0_all = np.zeros(B, np.int32), np.zeros(B, np.int32)
    clear, per_scene = np.full(B, np.inf), np.zeros((S, 4), np.int64)
    kept, stuck = np.zeros(S, bool), np.zeros(S, bool)
    o = 0
    for s, n in enumerate(sizes):
        Ps, vs, ss = P[:, o:o + n], v[o:o + n], sc[:, o:o + n]
        idx = np.arange(n)
        sel0 = np.argmax(ss, axis=0)                             # first maximum: the lowest k of equal scores
        sel = sel0.copy()

        def cvec(a, js):                                         # c(a, j; b, sel[b]) for j in js, all b -> (J, n), +inf at b = a
            m = pair_min(Ps[js, a][:, None], Ps[sel, idx][None], np.minimum(vs[a], vs)[None, :])
            c = np.sqrt(m) * float(inv_ss)
            c[:, a] = np.inf
            return c

        def pairs():
            return sum(int((cvec(a, [sel[a]]) < coll).sum()) for a in range(n)) // 2

        p0, swept = pairs(), 0
        for _ in range(int(sweeps)):
            changed = False
            for a in range(n):
                cur = int((cvec(a, [sel[a]]) < coll).sum())
                if cur == 0:
                    continue
                conf = (cvec(a, np.arange(K)) < coll).sum(1)
                js = min(range(K), key=lambda j: (conf[j], -ss[j, a], j))
                if conf[js] < cur:
                    sel[a] = js
                    changed = True
                else:
                    kept[s] = True
            if not changed:
                break
            swept += 1
        moved = int((sel != sel0).sum())
        for a in range(n):
            clear[o + a] = cvec(a, [sel[a]]).min() if n > 1 else np.inf
            if n > 1 and (cvec(a, np.arange(K)) < coll).any(axis=1).all():
                stuck[s] = True
        per_scene[s] = p0, pairs(), moved, swept
        sel_all[o:o + n], sel0_all[o:o + n] = sel, sel0
        o += n
    assert o == B
    per_row = None
    if err is not None:
        e, r = np.asarray(err), np.arange(B)
        per_row = np.concatenate([e[sel0_all, r], e[sel_all, r]], axis=1)
    return dict(sel=sel_all, sel0=sel0_all, clear=clear, per_scene=per_scene, per_row=per_row, kept=kept, stuck=stuck)


def cross_clearances(pos, start, sizes, inv_ss=1.0, lens=None, max_tuples=None, seed=0):
    """Every finite c(a, j; b, k), a < b of one scene, in float64 (flat array); with max_tuples a random sample of that many
    tuples instead (the large cases)."""
    P = _paths(pos, start)
    K, B, NP, _ = P.shape
    first = 0 if start is not None else 1
    v = _countable(lens, B, np.asarray(pos).shape[2], first)
    out, o = [], 0
    rng = np.random.RandomState(seed)
    for n in sizes:
        if n > 1 and max_tuples is None:
            for a in range(n):
                for b in range(a + 1, n):
                    m = pair_min(P[:, o + a][:, None], P[:, o + b][None], np.full((K, K), min(v[o + a], v[o + b])))
                    out.append(np.sqrt(m).ravel() * float(inv_ss))
        elif n > 1:
            cnt = max(1, max_tuples * n // B)
            a, b = rng.randint(0, n, cnt), rng.randint(0, n, cnt)
            j, k = rng.randint(0, K, cnt), rng.randint(0, K, cnt)
            keep = a != b
            a, b, j, k = a[keep], b[keep], j[keep], k[keep]
            m = pair_min(P[j, o + a], P[k, o + b], np.minimum(v[o + a], v[o + b]))
            out.append(np.sqrt(m) * float(inv_ss))
        o += n
    c = np.concatenate(out) if out else np.zeros(0)
    return c[np.isfinite(c)]


# ---- constructed inputs ---------------------------------------------------------------------------------------------------
# Every draw walks along one of a set of parallel lanes one unit apart (world units); all paths share one drift, so the
# motion of two paths relative to each other is their jitter alone: multiples of 1/64 within +-1/8 per coordinate.  Two draws
# on the same lane stay within sqrt(2) / 4 < 0.4 of each other, two on different lanes at least 0.75 > 0.6 apart.  With a
# start point, agent a starts on lane `stride * a` (stride >= 1: distinct places) and walks to its draw's lane during the
# first segment: two agents whose lanes are in the order of their starts keep 0.75 apart, two whose order is reversed or
# whose lanes are equal cross within 0.25 - still nothing between 0.4 and 0.6.  Positions are world / inv_ss with inv_ss a
# power of two.  Scores: "quant" (multiples of 1/4: ties), or continuous.
def lane_case(sizes, K, Tp, seed, stride=0, spread=None, with_start=False, pstride=2, inv_ss=1.0, ragged=False, scores="cont"):
    """spread: the lanes a draw of agent a picks from are stride * a + 0 .. spread - 1; None: 4 with a stride (neighbours
    overlap), else one and a half lanes per agent of the scene (conflicts are common and most can be resolved)."""
    rng = np.random.RandomState(seed)
    B = int(sum(sizes))
    assert not with_start or stride >= 1
    agent = np.concatenate([np.arange(n) for n in sizes])
    width = np.concatenate([np.full(n, spread if spread is not None else 4 if stride else max(2, 3 * n // 2)) for n in sizes])
    lane = stride * agent[None, :] + rng.randint(0, 1 << 30, (K, B)) % width[None, :]
    return lane_paths(lane, sizes, Tp, rng, start_lane=stride * agent if with_start else None, pstride=pstride, inv_ss=inv_ss,
                      ragged=ragged, scores=scores)


def lane_paths(lane, sizes, Tp, rng, start_lane=None, pstride=2, inv_ss=1.0, ragged=False, scores="cont", score=None):
    lane = np.asarray(lane)
    K, B = lane.shape
    drift = np.cumsum(rng.randint(-32, 33, (Tp + 1, 2)) / 64.0, axis=0)          # frame -1 (the start), then 0 .. Tp-1
    jit = rng.randint(-8, 9, (K, B, Tp, 2)) / 64.0
    world = drift[None, None, 1:] + jit
    world[..., 1] += lane[:, :, None]
    pos = np.zeros((K, B, Tp, pstride), np.float32)
    pos[..., :2] = world / inv_ss
    if pstride == 4:
        pos[..., 2:] = rng.rand(K, B, Tp, 2)                                     # the velocity columns: never read
    start = None
    if start_lane is not None:
        st = drift[None, 0] + rng.randint(-8, 9, (B, 2)) / 64.0
        st[:, 1] += start_lane
        start = (st / inv_ss).astype(np.float32)
    lens = None
    if ragged:
        lens = rng.randint(1, Tp + 1, B).astype(np.int32)
        for a in range(B):
            pos[:, a, lens[a]:] = np.nan
    if score is None:
        score = rng.randint(0, 4, (K, B)) / 4.0 if scores == "quant" else rng.rand(K, B)
    err = rng.rand(K, B, 2).astype(np.float32)
    return dict(pos=pos, start=start, score=np.asarray(score, np.float32), sizes=list(sizes), lens=lens, err=err, inv_ss=inv_ss,
                K=K, Tp=Tp, lane=lane)


def hand_case(lanes, order, Tp=3, seed=0):
    """One scene without a start point: lanes[a] = the lane of every draw of agent a (conflict = equal lanes), order[a] = its
    draws from the highest score down."""
    K, n = len(lanes[0]), len(lanes)
    lane = np.array(lanes).T
    score = np.zeros((K, n), np.float32)
    for a, od in enumerate(order):
        for r, k in enumerate(od):
            score[k, a] = 1.0 - r / 8.0
    return lane_paths(lane, [n], Tp, np.random.RandomState(seed), score=score)


def swap_case():
    """Two agents that swap places inside one segment: no frame is close, the clearance is 0.  Agent 1's second draw passes
    three units away."""
    pos = np.zeros((2, 2, 2, 2), np.float32)
    pos[:, 0] = [[0, 0], [2, 0]]
    pos[0, 1] = [[2, 0], [0, 0]]
    pos[1, 1] = [[2, 3], [0, 3]]
    score = np.array([[1.0, 1.0], [0.5, 0.5]], np.float32)
    return dict(pos=pos, start=None, score=score, sizes=[2], lens=None, err=np.zeros((2, 2, 2), np.float32), inv_ss=1.0, K=2,
                Tp=2)
