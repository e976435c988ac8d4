#!/usr/bin/env python
"""Timing of the sw_plan_refine launch on one MI355X, by the method of tools/plan_risk_timing.py: host clock around calls that
end in a host synchronisation, warm-up, then `--repeats` timed calls of each side, ALTERNATING, same seed for every call;
median and min / max, ms per call of the route.

The draws are those of the first chunk evaluate() forms of each of the three shapes of tools/_timing.py, all at K = 20: 816
agents in 102 scenes of 8, one scene of 8, 768 agents in 12 scenes of 64.  Two forms of the question, 32 iterations each:
  P = 1   leave-one-out, Q = B: every agent is the ego once, its plan is the constant-velocity extrapolation of its
          observations (evaluate_refine());
  P = 64  Q = S: the middle agent of every scene is the ego with 64 candidate plans (64 more draws of it).
Against the route a user has without the kernel: the same iteration written in torch on the device, one batch of elementwise
launches over a (Q, P, K, n, T) tensor per iteration - once with the closed-form gradient of include/socialways_hip.h, once
with autograd on the float32 objective; the faster of the two is the baseline.  Both are checked against the kernel's result
before anything is timed.  Next to it evaluate_refine() against evaluate_risk() on the whole held-out set.  Nothing here passes
or fails.

    python tools/refine_timing.py [--repeats 9] [--out profiles/plan_refine_timing.txt]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import COLL, PER_LAUNCH, cell, host_chunks  # noqa: E402

K, P_MANY, DIST = 20, 64, 0.5


class TorchDescent:
    """The iteration of sw_plan_refine in torch ops.  paths (K, B, T, >= 2), start (B, >= 2); query q: scene q_scene[q], ego row
    q_ego[q]; plans (Q, P, T, 2), plan_start (Q, 2).  Scenes are padded to the largest one and masked."""

    def __init__(self, paths, start, scenes, plans, plan_start, q_scene, q_ego, d0, n_iter, lr, w_track, w_smooth, max_move):
        off = scenes.scene_off.long()
        sizes = off[1:] - off[:-1]
        n_max = int(sizes.max())
        idx = torch.arange(n_max, device=paths.device)
        qs = q_scene.long()
        rows = off[qs][:, None] + idx[None]                                      # (Q, n_max)
        self.mask = ((idx[None] < sizes[qs][:, None]) & (rows != q_ego.long()[:, None]))[:, None, None, :, None]      # (Q, 1, 1, n, 1)
        rows = rows.clamp(max=paths.shape[1] - 1)
        full = torch.cat([start[None, :, None, :2].expand(paths.shape[0], -1, -1, -1), paths[..., :2]], dim=2)       # (K, B, T + 1, 2)
        self.A = full[:, rows].permute(1, 0, 2, 3, 4)[:, None].contiguous()      # (Q, 1, K, n, T + 1, 2)
        self.X0, self.xs = plans.contiguous(), plan_start[:, None, None, :].expand(-1, plans.shape[1], -1, -1)
        self.K, self.d02, self.n_iter, self.lr, self.wt, self.ws, self.cap = paths.shape[0], d0 * d0, n_iter, lr, w_track, w_smooth, max_move * d0

    def closest(self, X):
        PX = torch.cat([self.xs, X], dim=2)[:, :, None, None]                    # (Q, P, 1, 1, T + 1, 2)
        r0 = self.A[..., :-1, :] - PX[..., :-1, :]
        dv = (self.A[..., 1:, :] - PX[..., 1:, :]) - r0
        dd, rd = (dv * dv).sum(-1), (r0 * dv).sum(-1)
        tau = torch.where(dd > 0, (-rd / torch.where(dd > 0, dd, torch.ones_like(dd))).clamp(0, 1), torch.zeros_like(dd))
        c = r0 + tau[..., None] * dv
        u = (1 - (c * c).sum(-1) / self.d02).clamp(min=0) * self.mask
        return PX[:, :, 0, 0], tau, c, u

    def quadratic_step(self, PX, X):
        acc = torch.zeros(X.shape[:2] + (X.shape[2] + 2, 2), device=X.device)
        acc[:, :, 1:-2] = PX[:, :, 2:] - 2 * PX[:, :, 1:-1] + PX[:, :, :-2]
        return 2 * self.wt * (X - self.X0) + 2 * self.ws * (acc[:, :, :-2] - 2 * acc[:, :, 1:-1] + acc[:, :, 2:])

    def objective(self, X):
        PX, _, _, u = self.closest(X)
        acc = PX[:, :, 2:] - 2 * PX[:, :, 1:-1] + PX[:, :, :-2]
        return ((u * u).sum() / self.K + (self.wt * ((X - self.X0) ** 2).sum() + self.ws * (acc * acc).sum()) / self.d02)

    def update(self, X, step):
        norm = step.norm(dim=-1, keepdim=True)
        return X - torch.where(norm > self.cap, step * (self.cap / norm.clamp(min=1e-30)), step)

    def closed_form(self):
        X = self.X0.clone()
        for _ in range(self.n_iter):
            PX, tau, c, u = self.closest(X)
            w = 4 * u[..., None] * c
            g = (tau[..., None] * w).sum((2, 3))
            g[:, :, :-1] += ((1 - tau[..., None]) * w).sum((2, 3))[:, :, 1:]
            X = self.update(X, self.lr * (g / self.K + self.quadratic_step(PX, X)))
        torch.cuda.synchronize()
        return X

    def autograd(self):
        X = self.X0.clone()
        for _ in range(self.n_iter):
            X = X.detach().requires_grad_(True)
            with torch.enable_grad():
                J = self.objective(X)                                            # the plans are independent: one sum, every plan's gradient
            g, = torch.autograd.grad(J, X)
            X = self.update(X.detach(), self.lr * self.d02 * g)
        torch.cuda.synchronize()
        return X


def launch_set(tr, data, just_one):
    ops = T.sw.ops
    _, obsv, pred, sb = next(host_chunks(tr, data, K, just_one))
    obsv = obsv.contiguous()
    B, dev = obsv.shape[0], obsv.device
    torch.manual_seed(5)
    ph = tr.G.sample(obsv, K, tr.n_next, sb, torch.rand(K, B, tr.noise_len, device=dev))
    scenes = ops.SceneIndex.get(sb, B, dev)
    ss = float(data.ss)
    d0, inv_ss = DIST * ss, 1.0 / ss
    start = obsv[:, -1]
    off = scenes.scene_off.long()
    sizes = off[1:] - off[:-1]
    q_scene, _ = scenes.row_scene()
    every = torch.arange(B, dtype=torch.int32, device=dev)
    loo_plans, loo_start = T.sw.predict_cv(obsv, tr.n_next)[:, None, :, :2].contiguous(), start[:, :2].contiguous()
    egos = (off[:-1] + sizes // 2).int()
    many = tr.G.sample(obsv, P_MANY, tr.n_next, sb, torch.rand(P_MANY, B, tr.noise_len, device=dev))
    many_plans = many[:, egos.long(), :, :2].permute(1, 0, 2, 3).contiguous()                     # (S, 64, Tp, 2)
    many_start = start[egos.long(), :2].contiguous()
    s_idx = torch.arange(scenes.S, dtype=torch.int32, device=dev)
    par = dict(ops.DESCENT_DEFAULTS)

    def kernel(plans, pstart, qs, qe):
        def run():
            out = ops.plan_refine(ph, start, scenes, K, plans, pstart, qs, qe, d0, inv_ss, **par)
            torch.cuda.synchronize()
            return out
        return run

    calls, info = {}, []
    with torch.no_grad():
        for tag, plans, pstart, qs, qe in (("p1", loo_plans, loo_start, q_scene, every), ("p64", many_plans, many_start, s_idx, egos)):
            td = TorchDescent(ph, start, scenes, plans, pstart, qs, qe, d0, **par)
            calls.update({"refine_" + tag: kernel(plans, pstart, qs, qe), "closed_" + tag: td.closed_form, "autograd_" + tag: td.autograd})
            got = calls["refine_" + tag]()
            for other in ("closed_", "autograd_"):                               # the three routes compute the same thing
                err = float((calls[other + tag]() - got[0]).abs().max())
                assert err <= 1e-3 * d0, (other + tag, err, d0)
            info.append((float(got[1][:, :, 0, 0].mean()), float(got[1][:, :, 1, 0].mean()), float(got[2].mean())))
    return calls, B, scenes.S, info


def main():
    a = T.parse(__doc__, 9, 9)
    T.load("refine_timing.py")
    tr = T.trainer()
    lines = ["sw_plan_refine (one launch for all 32 iterations, through ops.plan_refine) against the same iteration in torch ops on the "
             "device (closed-form gradient | autograd on the float32 objective) on the first evaluation chunk of each shape, K = %d, "
             "dist %.1f, default descent parameters; host clock, ms per call of the whole route; %d alternating repeats after %d warm-up "
             "calls; %s" % (K, DIST, a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "%-28s %5s %6s  %-5s %30s %30s %30s   %s" % ("shape (at K = 20)", "B", "scenes", "form", "plan_refine median [min, max]",
                                                          "torch closed form", "torch autograd", "penalty before -> after, mean moved")]
    evals = []
    for name, n_scenes, agents, _, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        calls, B, S, info = launch_set(tr, data, just_one)
        with torch.no_grad():
            ms, _ = T.alternate(calls, a.warmup, a.repeats)
        for tag, form, (p0, p1, mv) in (("p1", "P=1, Q=B", info[0]), ("p64", "P=64, Q=S", info[1])):
            lines.append("%-28s %5d %6d  %-10s %30s %30s %30s   %.4f -> %.4f, %.4f" % (
                name.split(":")[0] + ": first chunk", B, S, form, cell(ms["refine_" + tag], fmt=PER_LAUNCH),
                cell(ms["closed_" + tag], fmt=PER_LAUNCH), cell(ms["autograd_" + tag], fmt=PER_LAUNCH), p0, p1, mv))
        ev = {"evaluate_refine": lambda: tr.evaluate_refine(data, n_gen_samples=K, dist=DIST, coll_dist=COLL, just_one=just_one),
              "evaluate_risk": lambda: tr.evaluate_risk(data, n_gen_samples=K, coll_dist=COLL, just_one=just_one)}
        ems, last = T.alternate(ev, a.warmup, a.repeats)
        evals.append((name, ems, last["evaluate_refine"]))
    lines.append("(the torch routes are checked against the kernel's refined plans before timing; every column includes the route's "
                 "output allocations)")
    lines.append("")
    lines.append("evaluate_refine() against evaluate_risk() on the whole held-out set of each shape (K = %d; the latency shape: its first "
                 "scene only), ms per call" % K)
    lines.append("%-88s %30s %30s   %s" % ("shape", "evaluate_refine median [min, max]", "evaluate_risk",
                                           "risk_cv | risk_ref | col_cv | col_ref | pen_cv | pen_ref | n_ego"))
    for name, ems, res in evals:
        lines.append("%-88s %30s %30s   %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %d" % (
            name, cell(ems["evaluate_refine"]), cell(ems["evaluate_risk"]), res["risk_cv"], res["risk_ref"], res["col_cv"],
            res["col_ref"], res["pen_cv"], res["pen_ref"], res["n_ego"]))
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
