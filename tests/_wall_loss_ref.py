"""The wall penalty of the generator loss in float64, written from the sw_wall_grad comment of include/socialways_hip.h alone:
what sw_wall_grad, ops.wall_grad, stats.wall_penalty and the wall term of SocialWaysTrainer.step() are held to by
test_wall_loss_host.py (CPU) and test_gpu_wall_loss.py.  Sees nothing of the device but inputs and outputs.

`reference` is numpy, per path, on tests/_walls_ref.py (`closest`, `candidates`): (loss, count, grad) with start, lens and K,
and the two masks below.  `l_wall` is torch in any dtype: its five candidates are torch.where selections in the header's
order, so autograd differentiates it (the envelope terms vanish: a free parameter either minimises |c|^2 or sits on a clamp).

MASKS, from the float64 reference, per path:
  near   a pair of a gated-in segment, counted or not, with | |c|^2 / dw^2 - 1 | < NEAR: fp32 may count it the other way.
  split  a counted pair for which another existing candidate has (cc_other - cc_best) / cc_other <= TIE and
         |s_other - s_best| * 4 u |c| / dw^2 > GRAD_REL / 4 * max|g_ref|: just inside a clamp of s, |c|^2 is flat to second order
         in s, fp32 may pick the clamped twin, and that moves a visible part of the pair's gradient from one end point to the
         other - a property of the definition in fp32, not of a kernel.  Such a path is compared on loss, count and the SUM
         of g over its points, which does not depend on the split."""
import numpy as np
import torch

import _walls_ref as W
from _ref64 import GRAD_REL, SEEDS

DW = 0.5
NEAR = 1e-5
TIE = 1e-5
CAP_SPLIT, CAP_NEAR = 0.05, 0.01      # of the paths of a GPU case


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def walls_case(R, Tp, M, seed, box=None, K=1):
    """R = K * B random walks and M walls, rounded to fp32 -> dict(pts (K, B, Tp + 1, 2): point 0 the start of agent a - shared
    by its K draws - then the Tp positions, walls (M, 2, 2), dw).  Path: a point uniform in [0, box]^2 plus the cumulative sum
    of N(0, 0.3^2) steps; walls: w0 uniform in the box, w1 = w0 + N(0, 1.5^2), every fourth wall a post.  box 8, 40 at 1024
    walls."""
    assert R % K == 0
    box = (40.0 if M >= 1024 else 8.0) if box is None else box
    rng = np.random.RandomState(seed)
    B = R // K
    origin = rng.uniform(0, box, (1, B, 1, 2))
    steps = rng.normal(0, 0.3, (K, B, Tp + 1, 2))
    steps[:, :, 0] = 0
    pts = origin + np.cumsum(steps, 2)
    w0 = rng.uniform(0, box, (M, 2))
    w1 = w0 + rng.normal(0, 1.5, (M, 2))
    w1[3::4] = w0[3::4]
    walls = np.stack([w0, w1], 1).reshape(M, 2, 2)
    return dict(pts=pts.astype(np.float32), walls=walls.astype(np.float32), dw=DW, K=K, B=B, Tp=Tp, M=M, seed=seed)


def split_case(case, with_start):
    """-> (pos (K, B, Tp, 2) fp32, start (B, 2) fp32 or None)"""
    pts = case["pts"]
    return np.ascontiguousarray(pts[:, :, 1:]), (np.ascontiguousarray(pts[0, :, 0]) if with_start else None)


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def _path(pos, start, lens, r, B, Tp):
    """The counted points of path r: (PX (lim + 1, 2) float64, front, lim)"""
    a = r % B
    P = np.asarray(pos[r], np.float64)[:, :2]
    front = 0 if start is None else 1
    if front:
        P = np.concatenate([np.asarray(start[a], np.float64)[None, :2], P], 0)
    ln = Tp if lens is None else int(np.clip(int(lens[a]), 1, Tp))
    lim = ln - (1 - front)                                    # the segment that ends at frame t counts while t < len
    return P[:lim + 1], front, lim


def reference(pos, start, walls, dw, lens=None, K=1, want_masks=False):
    """pos (K * B, Tp, >= 2) or (K, B, Tp, >= 2), start (B, >= 2) or None, walls (M, 2, 2), lens (B,) or None ->
    dict(loss (R,), count (R,) int64, grad (R, Tp, 2), and with want_masks near (R,) bool, split (R,) bool, active (R,) bool);
    float64.  What lies behind a length is never read."""
    pos = np.asarray(pos)
    pos = pos.reshape((-1,) + pos.shape[-2:])
    R, Tp = pos.shape[:2]
    assert R % K == 0
    B = R // K
    walls = np.asarray(walls, np.float64).reshape(-1, 2, 2)
    M, dw2 = walls.shape[0], float(dw) ** 2
    loss, count, grad = np.zeros(R), np.zeros(R, np.int64), np.zeros((R, Tp, 2))
    near, effect = np.zeros(R, bool), np.zeros(R)
    for r in range(R):
        PX, front, lim = _path(pos, start, lens, r, B, Tp)
        if lim <= 0 or M == 0:
            continue
        s, c, cc = W.closest(PX[:-1, None], PX[1:, None], walls[None, :, 0], walls[None, :, 1], np.float64)    # (lim, M[, 2])
        on = cc < dw2
        u = np.maximum(0.0, 1.0 - cc / dw2)
        loss[r], count[r] = np.where(on, u * u, 0.0).sum(), on.sum()
        w = np.where(on[..., None], (-4.0 / dw2) * u[..., None] * c, 0.0)
        gp = np.zeros((lim + 1, 2))
        gp[1:] += (s[..., None] * w).sum(1)                                          # the segment that ends at the point
        gp[:-1] += ((1.0 - s[..., None]) * w).sum(1)                                 # the segment that starts at it
        grad[r, :lim + 1 - front] = gp[front:]                                       # the start point is data
        if want_masks:
            near[r] = bool((np.abs(cc / dw2 - 1.0) < NEAR).any())
            cs, _, ccs, ok = W.candidates(PX[:-1, None], PX[1:, None], walls[None, :, 0], walls[None, :, 1], np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                tie = ok & (ccs > 0) & ((ccs - cc[None]) / np.where(ccs > 0, ccs, 1.0) <= TIE)
            eff = np.abs(cs - s[None]) * (4.0 * u * np.sqrt(cc) / dw2)[None]
            effect[r] = np.where(tie & on[None], eff, 0.0).max()
    out = dict(loss=loss, count=count, grad=grad)
    if want_masks:
        gmax = float(np.abs(grad).max())
        out.update(near=near, split=effect > GRAD_REL / 4 * gmax, active=count > 0)
    return out


def pick_case(R, Tp, M, K=1, with_start=True, lens_of=None):
    """The first seed of SEEDS whose float64 reference keeps the split-ambiguous paths at 5 % and the near ones at 1 % of the
    paths -> (case, pos, start, lens, reference with masks).  lens_of(case, rng) -> lens (B,) or None."""
    for seed in SEEDS:
        case = walls_case(R, Tp, M, seed, K=K)
        pos, start = split_case(case, with_start)
        lens = None if lens_of is None else lens_of(case, np.random.RandomState(seed + 1000))
        ref = reference(pos, start, case["walls"], case["dw"], lens, K, want_masks=True)
        if ref["split"].sum() <= CAP_SPLIT * R and ref["near"].sum() <= CAP_NEAR * R:
            return case, pos, start, lens, ref
    raise AssertionError("no seed of %s keeps the caps for R = %d, Tp = %d, M = %d" % (SEEDS, R, Tp, M))


def compare(got_grad, got_loss, got_count, ref, scale=1.0, base=None):
    """The comparison rule -> (largest |err| of the gradient / max|ref|, of the loss / max|ref|); raises AssertionError.
    got_* numpy, gradient (R, Tp, 2) = base + scale * g: split paths on the sum over their points, the others point by point,
    loss everywhere, count off the near mask.  Bound: GRAD_REL of the tensor's largest entry."""
    R = ref["loss"].shape[0]
    want = scale * ref["grad"] + (0.0 if base is None else np.asarray(base, np.float64).reshape(ref["grad"].shape))
    got = np.asarray(got_grad, np.float64).reshape(want.shape)
    assert np.isfinite(got).all()
    split = ref.get("split", np.zeros(R, bool))
    near = ref.get("near", np.zeros(R, bool))
    gmax = max(float(np.abs(want).max()), 1e-300)
    e_pt = float(np.abs(got - want)[~split].max(initial=0.0))
    # a split path: the sum over its points (of what was added: the pre-fill is taken off, or its rounding would count T times)
    off = 0.0 if base is None else np.asarray(base, np.float64).reshape(want.shape)
    e_sum = float(np.abs((got - off).sum(1) - (want - off).sum(1))[split].max(initial=0.0))
    assert e_pt <= GRAD_REL * gmax, "gradient: max|err| %.3e > %.1e * max|ref| %.3e" % (e_pt, GRAD_REL, gmax)
    assert e_sum <= GRAD_REL * gmax, "gradient sums of split paths: %.3e (max|ref| %.3e)" % (e_sum, gmax)
    lmax = max(float(np.abs(ref["loss"]).max()), 1e-300)
    e_l = float(np.abs(np.asarray(got_loss, np.float64).reshape(-1) - ref["loss"]).max(initial=0.0))
    assert e_l <= GRAD_REL * lmax, "loss: max|err| %.3e > %.1e * max|ref| %.3e" % (e_l, GRAD_REL, lmax)
    differs = np.asarray(got_count).reshape(-1).astype(np.int64) != ref["count"]
    assert not (differs & ~near).any(), "count differs away from the threshold"
    return max(e_pt, e_sum) / gmax, e_l / lmax


# ---- torch, differentiable ------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def phi_table(P, walls, dw):
    """P (R, NP, 2) paths, walls (M, 2, 2) -> (phi (R, NP - 1, M), on bool, s, c): the five candidates selected by torch.where in
    the header's order, a later one replacing the best only by a strictly smaller |c|^2."""
    walls = torch.as_tensor(walls, dtype=P.dtype).reshape(-1, 2, 2)
    p0, p1 = P[:, :-1, None], P[:, 1:, None]
    w0, w1 = walls[None, None, :, 0], walls[None, None, :, 1]
    e, f = p1 - p0, w1 - w0
    ee, ff = _dot(e, e), _dot(f, f)
    one, zero = torch.ones_like(ee + ff), torch.zeros_like(ee + ff)
    ee, ff = ee + zero, ff + zero

    def on_wall(p):
        u = torch.where(ff > 0, (_dot(p - w0, f) / torch.where(ff > 0, ff, one)).clamp(0, 1), zero)
        return p - (w0 + u[..., None] * f)

    def on_path(w):
        s = torch.where(ee > 0, (_dot(w - p0, e) / torch.where(ee > 0, ee, one)).clamp(0, 1), zero)
        return s, p0 + s[..., None] * e - w
    c = on_wall(p0)
    cc, s = _dot(c, c), zero
    for sn, cn in ((one, on_wall(p1)), on_path(w0), on_path(w1)):
        ccn = _dot(cn, cn)
        lt = ccn < cc
        s, cc, c = torch.where(lt, sn, s), torch.where(lt, ccn, cc), torch.where(lt[..., None], cn, c)
    d1, d2 = _cross(f, p0 - w0), _cross(f, p1 - w0)
    d3, d4 = _cross(e, w0 - p0), _cross(e, w1 - p0)
    crossing = (((d1 < 0) & (d2 > 0)) | ((d1 > 0) & (d2 < 0))) & (((d3 < 0) & (d4 > 0)) | ((d3 > 0) & (d4 < 0)))
    lt = crossing & (cc > 0)
    s = torch.where(lt, d1 / torch.where(lt, d1 - d2, one), s)
    cc, c = torch.where(lt, zero, cc), torch.where(lt[..., None], torch.zeros_like(c), c)
    dw2 = float(dw) ** 2
    on = cc < dw2
    u = (1 - cc / dw2).clamp_min(0)
    return torch.where(on, u * u, zero), on, s, c


def penalty_torch(pos, start, walls, dw):
    """pos (B, Tp, 2 | 4), start (B, >= 2) or None -> (loss (B,), count (B,) int64): differentiable in pos."""
    P = pos[..., :2]
    if start is not None:
        P = torch.cat([start[:, None, :2].to(P.dtype), P], 1)
    if P.shape[1] < 2 or np.asarray(walls).size == 0:
        z = P.sum((1, 2)) * 0
        return z, torch.zeros(P.shape[0], dtype=torch.int64)
    phi, on, _, _ = phi_table(P, walls, dw)
    return phi.sum((1, 2)), on.sum((1, 2))


def l_wall(pred_hat, start, walls, dw, weight, Bg=None):
    """The loss term of the rows of a packed batch of Bg agents (default: these rows are the batch): weight / (Bg * Tp) * the
    sum over the agents, the Tp segments of a path that starts at `start`, and the walls of phi."""
    B, Tp = pred_hat.shape[0], pred_hat.shape[1]
    return weight / (float(B if Bg is None else Bg) * Tp) * penalty_torch(pred_hat, start, walls, dw)[0].sum()


# ---- the cases of test_gpu_wall_loss.py (their caps are checked on the host by test_wall_loss_host.py) --------------------------
def ragged_lens(case, rng):
    """Lengths 1 .. Tp, one beyond Tp and one below 1 (both clamped by the kernel)."""
    lens = rng.randint(1, case["Tp"] + 1, case["B"]).astype(np.int32)
    lens[0], lens[-1] = case["Tp"] + 5, 0
    return lens


# (K, B, Tp, M, with_start, ragged, pstride, dstride): R = K B of 1, 63, 64, 65, 129 (3 x 43: row % B matters) and 130; Tp of 1
# (no segment without start), 12 (one time chunk), 17 and 25 (two, and the point they share); M of 0, 1, 3 (fewer walls than
# waves), 5, 33, 130 (not multiples of 4) and 1024 (the maximum); both strides on both sides
GPU_CASES = [(1, 1, 12, 130, True, False, 2, 2), (1, 63, 12, 3, True, False, 4, 2), (1, 64, 17, 1, False, False, 2, 4),
             (1, 65, 17, 130, True, False, 4, 4), (1, 130, 25, 33, True, False, 2, 4), (1, 130, 12, 5, False, False, 4, 2),
             (3, 43, 25, 5, True, True, 4, 4), (3, 43, 17, 3, False, True, 2, 2), (1, 64, 12, 1024, True, False, 2, 2),
             (1, 65, 1, 5, True, False, 2, 4), (1, 65, 1, 5, False, False, 4, 2), (1, 130, 12, 0, True, False, 4, 4),
             (1, 130, 17, 33, True, True, 2, 2)]

_picked = {}


def gpu_case(K, B, Tp, M, with_start, ragged, *_):
    """pick_case for a row of GPU_CASES, computed once."""
    key = (K, B, Tp, M, with_start, ragged)
    if key not in _picked:
        _picked[key] = pick_case(K * B, Tp, M, K, with_start, ragged_lens if ragged else None)
    return _picked[key]
