"""float64 numpy implementation of sw_plan_risk, written from the comment in include/socialways_hip.h alone: the segment
distances of a plan against every (draw, agent) path, the path clearances, the per-agent counts, the product and the four
integers - and the constructed inputs the plan-risk tests share.  Sees nothing of the device but inputs and outputs."""
import numpy as np

from _compose_ref import lane_case, pair_min


def _with_start(p, s):
    """p (.., Tp, 2), s (.., 2) or None -> (.., NP, 2) float64, the start point in front when there is one."""
    p = np.asarray(p)[..., :2].astype(np.float64)
    if s is None:
        return p
    s = np.asarray(s)[..., :2].astype(np.float64)
    return np.concatenate([s[..., None, :], p], axis=-2)


def segment_d2(PA, PB):
    """Squared closest approach per segment of paths PA, PB (.., NP, 2), broadcast against each other -> (.., NP - 1)."""
    r0 = PA[..., :-1, :] - PB[..., :-1, :]
    dv = (PA[..., 1:, :] - PB[..., 1:, :]) - r0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dd, rd = (dv * dv).sum(-1), (r0 * dv).sum(-1)
        tau = np.where(dd > 0, np.clip(-rd / np.where(dd > 0, dd, 1.0), 0.0, 1.0), 0.0)
        c = r0 + tau[..., None] * dv
        return (c * c).sum(-1)


def risk_reference(pos, start, sizes, plans, plan_start, q_scene, q_ego, coll_dist, inv_ss=1.0, lens=None, plan_lens=None):
    """pos (K, B, Tp, >= 2), start (B, >= 2) or None, plans (Q, P, Tp, 2), plan_start (Q, 2) or None, q_scene (Q,), q_ego (Q,) or
    None -> dict(risk (Q, P) float64 - the exact product -, clear_min (Q, P) float64, counts (Q, P, 4) int64, n_other (Q,): the
    agents of the query, hmax (Q, P), hsum (Q, P), c: every finite path clearance, flat).  The comparison with coll_dist is
    made against its fp32 value, as the kernel makes it."""
    pos, plans = np.asarray(pos), np.asarray(plans)
    K, B, Tp = pos.shape[:3]
    Q, P = plans.shape[:2]
    first = 0 if start is not None else 1
    A = _with_start(pos, None if start is None else np.broadcast_to(np.asarray(start)[None, :, :2], (K, B, 2)))      # (K, B, NP, 2)
    PL = _with_start(plans, None if plan_start is None else np.broadcast_to(np.asarray(plan_start)[:, None, :2], (Q, P, 2)))
    la = np.full(B, Tp) if lens is None else np.clip(np.asarray(lens).astype(np.int64), 1, Tp)
    lp = np.full(Q, Tp) if plan_lens is None else np.clip(np.asarray(plan_lens).astype(np.int64), 1, Tp)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    coll = float(np.float32(coll_dist))
    risk, clear_min = np.zeros((Q, P)), np.full((Q, P), np.inf)
    counts = np.tile(np.array([0, -1, -1, 0], np.int64), (Q, P, 1))
    n_other, hmax, hsum, allc = np.zeros(Q, np.int64), np.zeros((Q, P), np.int64), np.zeros((Q, P), np.int64), []
    for q in range(Q):
        s = int(q_scene[q])
        if not 0 <= s < len(sizes):
            continue
        ego = -1 if q_ego is None else int(q_ego[q])
        rows = np.array([r for r in range(off[s], off[s + 1]) if r != ego], np.int64)
        n_other[q] = len(rows)
        if len(rows) == 0:
            continue
        lim = np.minimum(la[rows], lp[q]) - first                                   # countable segments per agent
        PA, PP = A[:, rows][None], PL[q][:, None, None]                             # (1, K, m, NP, 2) and (P, 1, 1, NP, 2)
        d2 = segment_d2(PA, PP)                                                     # (P, K, m, NS)
        NS = d2.shape[-1]
        on = np.arange(NS)[None, None, None, :] < lim[None, None, :, None]
        with np.errstate(invalid="ignore"):
            d = np.where(on, np.sqrt(d2) * float(inv_ss), np.inf)
        d = np.where(np.isnan(d), np.inf, d)                                        # a counted NaN does not occur in the cases
        c = d.min(-1) if NS else np.full(d.shape[:-1], np.inf)                      # (P, K, m)
        m2 = pair_min(PA, PP, np.broadcast_to(lim[None, None, :], c.shape))
        assert np.array_equal(np.sqrt(m2) * float(inv_ss), c), "the two forms of the path clearance agree"
        allc.append(c[np.isfinite(c)])
        conf = c < coll
        h = conf.sum(1)                                                             # (P, m)
        hit = (d < coll)                                                            # (P, K, m, NS)
        for p in range(P):
            f = (K - h[p]).astype(np.float64) / K
            risk[q, p] = 1.0 - np.prod(f)
            clear_min[q, p] = c[p].min()
            counts[q, p, 0] = conf[p].any(1).sum()
            if hit[p].any():
                counts[q, p, 1] = np.nonzero(hit[p].any((0, 1)))[0][0] + first
            if h[p].max() > 0:
                b = int(np.argmax(h[p]))                                            # first maximum: the lowest row of equal ones
                counts[q, p, 2], counts[q, p, 3] = rows[b], h[p, b]
            hmax[q, p], hsum[q, p] = h[p].max(), h[p].sum()
    return dict(risk=risk, clear_min=clear_min, counts=counts, n_other=n_other, hmax=hmax, hsum=hsum,
                c=np.concatenate(allc) if allc else np.zeros(0))


def risk_bound(n):
    """n divisions, n - 1 products and one subtraction in fp32 on values in [0, 1]: a rounding bound, not a measurement."""
    return 2.0 * (n + 1) * 2.0 ** -24


# ---- constructed inputs ---------------------------------------------------------------------------------------------------
def risk_case(sizes, K, Tp, seed, P=None, **kw):
    """A lane_case with one agent more per scene; that agent's K draws are the plans of the scene's query (P plans: draw
    p % K), its start point their start, its length their length.  Plans are then lane paths, so every clearance is < 0.4 or
    > 0.6 in world units (tests/_compose_ref.py).  Q = S queries, query q on scene q, nobody left out."""
    big = lane_case([n + 1 for n in sizes], K, Tp, seed, **kw)
    last = np.cumsum([n + 1 for n in sizes]) - 1
    keep = np.setdiff1d(np.arange(int(sum(sizes)) + len(sizes)), last)
    P = K if P is None else P
    plans = np.ascontiguousarray(big["pos"][np.arange(P) % K][:, last, :, :2].transpose(1, 0, 2, 3))       # (Q, P, Tp, 2)
    return dict(pos=np.ascontiguousarray(big["pos"][:, keep]), start=None if big["start"] is None else big["start"][keep].copy(),
                plans=plans, plan_start=None if big["start"] is None else big["start"][last].copy(),
                lens=None if big["lens"] is None else big["lens"][keep].copy(),
                plan_lens=None if big["lens"] is None else big["lens"][last].copy(),
                sizes=list(sizes), K=K, Tp=Tp, inv_ss=big["inv_ss"], q_scene=np.arange(len(sizes), dtype=np.int32), q_ego=None)


def with_queries(case, q_scene, q_ego):
    """The case asked other questions: query i = the plans of scene q_scene[i] against that scene, q_ego[i] left out."""
    q_scene = np.asarray(q_scene, np.int32)
    out = dict(case, q_scene=q_scene, q_ego=None if q_ego is None else np.asarray(q_ego, np.int32))
    out["plans"] = np.ascontiguousarray(case["plans"][q_scene])
    for k in ("plan_start", "plan_lens"):
        out[k] = None if case[k] is None else case[k][q_scene].copy()
    return out


SIZES = [7, 1, 33, 2, 65]
COLL = 0.5


def constructed_cases():
    """(name, case): the smallest shapes that cross every loop boundary of the kernel - agent groups, draw groups, time chunks,
    plan tiles, a plan too long for LDS."""
    out = []
    for with_start in (False, True):
        for pstride in (2, 4):
            out.append(("sizes_start%d_ps%d" % (with_start, pstride),
                        risk_case(SIZES, 20, 12, seed=11 + pstride + with_start, stride=1 if with_start else 0,
                                  with_start=with_start, pstride=pstride)))
    out.append(("k1", risk_case([5, 1, 9], 1, 12, seed=20, spread=3)))
    out.append(("k65_tp17_ragged_x2", risk_case([6, 3], 65, 17, seed=21, ragged=True, inv_ss=2.0)))
    out.append(("k65_tp17_ragged_start_half", risk_case([4, 9], 65, 17, seed=22, stride=1, with_start=True, ragged=True, inv_ss=0.5)))
    out.append(("k260_tp1", risk_case([3, 2], 260, 1, seed=23, spread=1, P=3)))
    out.append(("k260_tp1_start", risk_case([3, 2], 260, 1, seed=24, stride=1, spread=2, with_start=True, P=3)))
    for P in (1, 5, 64, 65, 130):
        out.append(("p%d" % P, risk_case([5, 2], 6, 4, seed=30 + P, P=P, spread=4)))
    many = risk_case([2, 3], 4, 3, seed=39, P=65, spread=3)                           # enough queries for tiles of 64 plans
    out.append(("p65_q512", with_queries(many, np.arange(512) % 2, (np.arange(512) % 7) - 1)))
    out.append(("n300", risk_case([300], 4, 3, seed=40, spread=450)))
    out.append(("tp130_n70", risk_case([70], 3, 130, seed=41, P=2, spread=100)))
    out.append(("tp8200", risk_case([3], 2, 8200, seed=42, P=2, spread=2)))          # one plan is more than 64 KB
    out.append(("all_hit", risk_case([4, 2], 5, 6, seed=43, spread=1)))
    out.append(("all_clear", risk_case([4, 2], 5, 6, seed=44, stride=1, spread=1)))
    base = risk_case([4, 3, 6], 8, 12, seed=45, stride=1, with_start=True, spread=3)
    out.append(("queries", with_queries(base, [0, 0, 0, 2, 2, 1, 2], [-1, 2, 5, 7, 12, 0, 99])))
    return out


def run_reference(case, coll=COLL):
    return risk_reference(case["pos"], case["start"], case["sizes"], case["plans"], case["plan_start"], case["q_scene"],
                          case["q_ego"], coll, case["inv_ss"], case["lens"], case["plan_lens"])
