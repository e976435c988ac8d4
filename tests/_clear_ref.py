"""The scene-clearance penalty in torch, in any dtype: what sw_clearance_grad, ops.clearance_grad, stats.clearance_penalty and
the clearance term of SocialWaysTrainer.step() are held to by test_clearance_host.py (CPU) and test_gpu_clearance_loss.py.

The path of agent a is P_a[0] = start[a] (when there is a start), then pos[a][0 .. Tp-1].  For two agents a != b of one scene
and the segment from point s - 1 to point s:  r0 = P_a[s-1] - P_b[s-1], r1 = P_a[s] - P_b[s], dv = r1 - r0,
tau = clamp(-(r0.dv) / (dv.dv), 0, 1) (0 when dv.dv = 0), c = r0 + tau dv, u = max(0, 1 - |c|^2 / d0^2), phi = u^2.
`terms` forms these for every ordered pair of a scene at once; `penalty` sums them (the gradient is autograd's),
`closed_form_grad` is the hand-derived gradient the kernel implements, `l_col` the loss term of the step."""
import numpy as np
import torch


def paths(pos, start=None):
    """(B, NP, 2): the start point in front of the x, y of pos (B, Tp, 2 | 4) when there is one."""
    P = pos[..., :2]
    return P if start is None else torch.cat([start[:, None, :2].to(P.dtype), P], 1)


def terms(P, d0):
    """P (n, NP, 2): one scene -> tau, c, cc, u, each (n, n, NS[, 2]) over ordered pairs (a, b) and segments; the diagonal
    a == b is formed like any pair and has to be masked by the caller."""
    r = P[:, None] - P[None, :]
    r0, r1 = r[:, :, :-1], r[:, :, 1:]
    dv = r1 - r0
    dd, rd = (dv * dv).sum(-1), (r0 * dv).sum(-1)
    moving = dd > 0
    tau = torch.where(moving, (-rd / torch.where(moving, dd, torch.ones_like(dd))).clamp(0, 1), torch.zeros_like(dd))
    c = r0 + tau[..., None] * dv
    cc = (c * c).sum(-1)
    u = (1 - cc / (d0 * d0)).clamp_min(0)
    return tau, c, cc, u


def _scenes(sb, B):
    sb = np.asarray(sb, dtype=np.int64).reshape(-1, 2)
    return [(0, B)] if len(sb) == 0 else [(int(lo), int(hi)) for lo, hi in sb]


def penalty(pos, start, sb, d0):
    """-> (loss (B,), count (B,) int64): loss[a] = 1/2 sum over b != a and s of phi (loss.sum() = the sum over pairs a < b),
    count[a] = the number of (b, s) with |c|^2 < d0^2.  Differentiable in pos."""
    P = paths(pos, start)
    loss, count = [], []
    for lo, hi in _scenes(sb, P.shape[0]):
        _, _, cc, u = terms(P[lo:hi], d0)
        off = ~torch.eye(hi - lo, dtype=torch.bool)[:, :, None]
        loss.append(0.5 * (u * u * off).sum((1, 2)))
        count.append(((cc < d0 * d0) & off).sum((1, 2)))
    return torch.cat(loss), torch.cat(count)


def closed_form_grad(pos, start, sb, d0):
    """d(penalty().loss.sum()) / d(pos[..., :2]) by the formula of include/socialways_hip.h, (B, Tp, 2):
    g_a[s] = sum over b != a of [ -(4 u_s / d0^2) tau_s c_s - (4 u_{s+1} / d0^2) (1 - tau_{s+1}) c_{s+1} ]."""
    P = paths(pos.detach(), None if start is None else start.detach())
    g = torch.zeros_like(P)
    for lo, hi in _scenes(sb, P.shape[0]):
        tau, c, _, u = terms(P[lo:hi], d0)
        off = ~torch.eye(hi - lo, dtype=torch.bool)[:, :, None, None]
        w = (-4.0 / (d0 * d0)) * u[..., None] * c * off
        g[lo:hi, 1:] += (tau[..., None] * w).sum(1)               # the r1 end of segment s: point s
        g[lo:hi, :-1] += ((1 - tau[..., None]) * w).sum(1)        # the r0 end of segment s: point s - 1
    return g if start is None else g[:, 1:]                       # P[0] = start is data


def l_col(pos, start, sb, d0, weight, global_B=None, global_row0=0):
    """The loss term of rows [global_row0, global_row0 + B) of a packed batch of global_B agents (default: the whole batch):
    weight / (Bg * Tp) * the sum over the shard's scenes, pairs a < b and segments of phi; sb in the rows of the packed
    batch.  Scenes are sharded whole, so the shards' terms add up to the full batch's."""
    B, Tp = pos.shape[0], pos.shape[1]
    Bg = float(B if global_B is None else global_B)
    local = np.asarray(sb, dtype=np.int64).reshape(-1, 2) - int(global_row0)
    return weight / (Bg * Tp) * penalty(pos, start, local, d0)[0].sum()


def shares(pos, start, sb, d0, eps=1e-5):
    """Of the reference's (ordered pair, segment)s: (share with |c|^2 < d0^2, number of agents that have one within eps of the
    threshold in |c|^2 / d0^2 (B,) bool)."""
    P = paths(pos, start)
    n_on = n_all = 0
    near = []
    for lo, hi in _scenes(sb, P.shape[0]):
        _, _, cc, _ = terms(P[lo:hi], d0)
        off = ~torch.eye(hi - lo, dtype=torch.bool)[:, :, None]
        n_on += int(((cc < d0 * d0) & off).sum())
        n_all += int(off.expand_as(cc).sum())
        near.append((((cc / (d0 * d0) - 1).abs() < eps) & off).any(2).any(1))
    return n_on / max(n_all, 1), torch.cat(near)
