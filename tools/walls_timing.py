#!/usr/bin/env python
"""Timing of the wall launches on one MI355X, by the method of tools/refine_timing.py: host clock around calls that end in a
host synchronisation, warm-up, then `--repeats` timed calls of each side, ALTERNATING, same inputs for every call; median and
min / max, ms per call of the route.

The draws are those of the first chunk evaluate() forms of each of the three shapes of tools/_timing.py, all at K = 20: 816
agents in 102 scenes of 8, one scene of 8, 768 agents in 12 scenes of 64.  The map: M = 16 / 128 random segments inside the
bounding box of the chunk's observations.
  refine     ops.plan_refine, 32 iterations, P = 1 leave-one-out (Q = B) and P = 64 per scene (Q = S) as tools/refine_timing.py:
             without walls and with 16 / 128, and next to it the same iteration WITH the wall term in torch ops on the device
             (the closed-form route of tools/refine_timing.py plus the five-candidate closest approach over a (Q, P, T, M) tensor
             per iteration; its refined plans are compared with the kernel's before anything is timed and the difference is recorded);
  path_walls ops.path_walls on the K * B draws of the chunk at M = 16 / 128;
  evaluate_walls() at M = 128 against evaluate_scenes() on the whole held-out set of each shape.
--parent-tree DIR (a tree of the parent commit with its library built): ops.plan_refine WITHOUT walls - the same launch in both
builds - in child processes, one at a time, in the order parent, this, parent per round: the parent measured twice is the
control, and this build's median must sit inside the spread of the two.
Nothing here passes or fails.

    python tools/walls_timing.py [--repeats 9] [--parent-tree DIR [--rounds 3]] [--out profiles/walls_timing.txt]
"""
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import COLL, PER_LAUNCH, cell, host_chunks  # noqa: E402

from refine_timing import TorchDescent  # noqa: E402

K, P_MANY, DIST, MS = 20, 64, 0.5, (16, 128)


class TorchWallDescent(TorchDescent):
    """TorchDescent.closed_form with the wall term of sw_plan_refine_walls (w_wall = 1, wall_d0 = d0)."""

    def __init__(self, walls, *a, **kw):
        super().__init__(*a, **kw)
        self.w0, self.w1 = walls[None, None, None, :, 0], walls[None, None, None, :, 1]      # (1, 1, 1, M, 2)

    def wall_grad(self, PX):
        """PX (Q, P, T + 1, 2) -> the sum over the walls of -4 u (s c of segment t + (1 - s) c of segment t + 1), (Q, P, T, 2)."""
        p0, p1, w0, w1 = PX[:, :, :-1, None], PX[:, :, 1:, None], self.w0, self.w1
        e, f = p1 - p0, w1 - w0
        ee, ff = (e * e).sum(-1), (f * f).sum(-1)
        one, zero = torch.ones_like(ee), torch.zeros_like(ee)

        def on_wall(p):
            u = torch.where(ff > 0, (((p - w0) * f).sum(-1) / torch.where(ff > 0, ff, one)).clamp(0, 1), zero)
            return p - (w0 + u[..., None] * f)

        def on_path(w):
            s = torch.where(ee > 0, (((w - p0) * e).sum(-1) / torch.where(ee > 0, ee, one)).clamp(0, 1), zero)
            return s, p0 + s[..., None] * e - w

        def cross(a, b):
            return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]

        s3, c3 = on_path(w0)
        s4, c4 = on_path(w1)
        d1, d2, d3, d4 = cross(f, p0 - w0), cross(f, p1 - w0), cross(e, w0 - p0), cross(e, w1 - p0)
        crossing = (d1 * d2 < 0) & (d3 * d4 < 0)
        s, c = zero, on_wall(p0)
        cc = (c * c).sum(-1)
        for sk, ck in ((one, on_wall(p1)), (s3, c3), (s4, c4)):
            ck2 = (ck * ck).sum(-1)
            lt = ck2 < cc
            s, c, cc = torch.where(lt, sk, s), torch.where(lt[..., None], ck, c), torch.where(lt, ck2, cc)
        c = torch.where(crossing[..., None], torch.zeros_like(c), c)      # a crossing: c = 0, no gradient
        cc = torch.where(crossing, zero, cc)
        u = (1 - cc / self.d02).clamp(min=0)
        w = -4 * u[..., None] * c
        g = (s[..., None] * w).sum(3)
        g[:, :, :-1] += ((1 - s[..., None]) * w).sum(3)[:, :, 1:]
        return g

    def closed_form(self):
        X = self.X0.clone()
        for _ in range(self.n_iter):
            PX, tau, c, u = self.closest(X)
            w = 4 * u[..., None] * c
            g = (tau[..., None] * w).sum((2, 3))
            g[:, :, :-1] += ((1 - tau[..., None]) * w).sum((2, 3))[:, :, 1:]
            X = self.update(X, self.lr * (g / self.K + self.wall_grad(PX) + self.quadratic_step(PX, X)))
        torch.cuda.synchronize()
        return X


def random_walls(obsv, M, seed):
    """M segments inside the bounding box of the observations, a tenth of its side long at most."""
    g = torch.Generator().manual_seed(seed)
    xy = obsv[..., :2].reshape(-1, 2).cpu()
    lo, hi = xy.min(0)[0], xy.max(0)[0]
    a = lo + torch.rand(M, 2, generator=g) * (hi - lo)
    b = a + (torch.rand(M, 2, generator=g) - 0.5) * 0.2 * (hi - lo)
    return torch.stack([a, b], 1).float().to(obsv.device)


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
    walls = {M: random_walls(obsv, M, 7 + M) for M in MS}

    def refine(plans, pstart, qs, qe, w):
        def run():
            out = ops.plan_refine(ph, start, scenes, K, plans, pstart, qs, qe, d0, inv_ss, walls=w)
            torch.cuda.synchronize()
            return out
        return run

    def paths(w):
        def run():
            out = ops.path_walls(ph, start, K, w, COLL, inv_ss)
            torch.cuda.synchronize()
            return out
        return run

    calls, diff = {}, {}
    par = dict(ops.DESCENT_DEFAULTS)
    for tag, plans, pstart, qs, qe in (("p1", loo_plans, loo_start, q_scene, every), ("p64", many_plans, many_start, s_idx, egos)):
        calls["refine_%s_m-" % tag] = refine(plans, pstart, qs, qe, None)
        for M in MS:
            calls["refine_%s_m%d" % (tag, M)] = refine(plans, pstart, qs, qe, walls[M])
            td = TorchWallDescent(walls[M], ph, start, scenes, plans, pstart, qs, qe, d0, **par)
            calls["torch_%s_m%d" % (tag, M)] = td.closed_form
            # the two routes compute the same thing - up to the candidate order: on random walls inside the box near-ties occur,
            # and where float32 division and the kernel's reciprocal order two candidates differently a share of one pair's
            # gradient changes its end point.  The largest difference is recorded; only a gross one (5 % of d0) stops the tool
            diff["%s_m%d" % (tag, M)] = float((td.closed_form() - calls["refine_%s_m%d" % (tag, M)]()[0]).abs().max()) / d0
            assert diff["%s_m%d" % (tag, M)] <= 5e-2, (tag, M, diff)
    for M in MS:
        calls["paths_m%d" % M] = paths(walls[M])
    hit = {M: float((calls["paths_m%d" % M]()[1] >= 0).float().mean()) for M in MS}
    return calls, B, scenes.S, hit, walls[MS[-1]], diff


def main():
    def more(ap):
        T.parent_tree_args(ap)
        ap.add_argument("--child", action="store_true", help="(internal) one build's side of --parent-tree")
        ap.add_argument("--tree", default=T.HERE, help="(internal)")
    a = T.parse(__doc__, 9, 9, more)
    if a.child:
        return child(a)
    T.load("walls_timing.py")
    tr = T.trainer()
    lines = ["ops.plan_refine (one launch for all 32 iterations) without walls and with M = 16 / 128, and ops.path_walls on the K * B draws, on "
             "the first evaluation chunk of each shape, K = %d, dist %.1f, default descent parameters; host clock, ms per call of the whole "
             "route; %d alternating repeats after %d warm-up calls; %s" % (K, DIST, a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "%-28s %5s %6s  %-10s %30s %30s %30s %30s %30s" % ("shape (at K = 20)", "B", "scenes", "form", "no walls: median [min, max]",
                                                                "M = 16", "M = 128", "torch ops, M = 16", "torch ops, M = 128")]
    evals = []
    for name, n_scenes, agents, _, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        with torch.no_grad():
            calls, B, S, hit, walls, diff = launch_set(tr, data, just_one)
            ms, _ = T.alternate(calls, a.warmup, a.repeats)
        head = name.split(":")[0] + ": first chunk"
        for tag, form in (("p1", "P=1, Q=B"), ("p64", "P=64, Q=S")):
            lines.append("%-28s %5d %6d  %-10s %30s %30s %30s %30s %30s" % (
                head, B, S, form, cell(ms["refine_%s_m-" % tag], fmt=PER_LAUNCH), cell(ms["refine_%s_m16" % tag], fmt=PER_LAUNCH),
                cell(ms["refine_%s_m128" % tag], fmt=PER_LAUNCH), cell(ms["torch_%s_m16" % tag], fmt=PER_LAUNCH),
                cell(ms["torch_%s_m128" % tag], fmt=PER_LAUNCH))
                + "   max|torch - kernel| / d0: %.2g | %.2g" % (diff["%s_m16" % tag], diff["%s_m128" % tag]))
        lines.append("%-28s %5d %6d  %-10s %30s %30s %30s   draws within %.2f of a wall: %.3f | %.3f" % (
            head, B, S, "path_walls", "-", cell(ms["paths_m16"], fmt=PER_LAUNCH), cell(ms["paths_m128"], fmt=PER_LAUNCH), COLL, hit[16], hit[128]))
        ev = {"evaluate_walls": lambda: tr.evaluate_walls(data, walls, n_gen_samples=K, wall_dist=COLL, just_one=just_one),
              "evaluate_scenes": lambda: tr.evaluate_scenes(data, n_gen_samples=K, coll_dist=COLL, just_one=just_one)}
        ems, last = T.alternate(ev, a.warmup, a.repeats)
        evals.append((name, ems, last["evaluate_walls"]))
    lines.append("(every column includes the route's output allocations; the largest difference between the torch route's refined plans and the kernel's is in the last column)")
    lines.append("")
    lines.append("evaluate_walls() at M = 128 against evaluate_scenes() on the whole held-out set of each shape (K = %d; the latency shape: its "
                 "first scene only), ms per call" % K)
    lines.append("%-88s %30s %30s   %s" % ("shape", "evaluate_walls median [min, max]", "evaluate_scenes", "wall_draws | wall_agents | wall_gt | n_agents"))
    for name, ems, res in evals:
        lines.append("%-88s %30s %30s   %.4f | %.4f | %.4f | %d" % (name, cell(ems["evaluate_walls"]), cell(ems["evaluate_scenes"]),
                                                                     res["wall_draws"], res["wall_agents"], res["wall_gt"], res["n_agents"]))
    if a.parent_tree:
        lines += [""] + across_builds(a)
    T.write_out(lines, a.out)


# ---- the launch without walls at the parent build and at this one -------------------------------------------------------------
def child(a):
    """One build's side: ops.plan_refine without walls (the call both builds have) on the three chunks -> one JSON line."""
    T.load("walls_timing.py", a.tree)
    tr, out = T.trainer(), {}
    ops = T.sw.ops
    for name, n_scenes, agents, _, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        _, obsv, pred, sb = next(host_chunks(tr, data, K, just_one))
        obsv = obsv.contiguous()
        B, dev = obsv.shape[0], obsv.device
        with torch.no_grad():
            torch.manual_seed(5)
            ph = tr.G.sample(obsv, K, tr.n_next, sb, torch.rand(K, B, tr.noise_len, device=dev))
            scenes = ops.SceneIndex.get(sb, B, dev)
            ss = float(data.ss)
            start = obsv[:, -1]
            off = scenes.scene_off.long()
            egos = (off[:-1] + (off[1:] - off[:-1]) // 2).int()
            many = tr.G.sample(obsv, P_MANY, tr.n_next, sb, torch.rand(P_MANY, B, tr.noise_len, device=dev))
            sets = {"p1": (T.sw.predict_cv(obsv, tr.n_next)[:, None, :, :2].contiguous(), start[:, :2].contiguous(), scenes.row_scene()[0],
                           torch.arange(B, dtype=torch.int32, device=dev)),
                    "p64": (many[:, egos.long(), :, :2].permute(1, 0, 2, 3).contiguous(), start[egos.long(), :2].contiguous(),
                            torch.arange(scenes.S, dtype=torch.int32, device=dev), egos)}

            def run(plans, pstart, qs, qe):
                def f():
                    o = ops.plan_refine(ph, start, scenes, K, plans, pstart, qs, qe, DIST * ss, 1.0 / ss)
                    torch.cuda.synchronize()
                    return o
                return f
            ms, last = T.alternate({k: run(*v) for k, v in sets.items()}, a.warmup, a.repeats)
        for k in sets:
            out["%s|%s" % (name.split(":")[0], k)] = dict(ms=ms[k], sum=float(last[k][0].double().sum()))
    print("TIMING_CHILD " + json.dumps(out))


def across_builds(a):
    side = {"parent A": [], "this": [], "parent B": []}
    trees = {"parent A": os.path.abspath(a.parent_tree), "this": T.HERE, "parent B": os.path.abspath(a.parent_tree)}
    for _ in range(a.rounds):
        for build in side:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", trees[build], "--repeats", str(a.repeats),
                                "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit("child on %s failed (%d): %s" % (trees[build], p.returncode, p.stderr[-2000:]))
            side[build].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("TIMING_CHILD ")][-1][13:]))
    lines = ["ops.plan_refine WITHOUT walls (32 iterations), the parent build against this build: %d rounds of child processes in the order "
             "parent, this, parent, %d timed calls per child after %d warm-up calls; ms per call; the parent measured twice is the control"
             % (a.rounds, a.repeats, a.warmup),
             "%-22s %30s %30s %30s   %s" % ("chunk | form", "parent A median [min, max]", "this build", "parent B", "this inside the parents' spread | same refined plans")]
    for key in side["this"][0]:
        ms = {b: [t for r in side[b] for t in r[key]["ms"]] for b in side}
        both = ms["parent A"] + ms["parent B"]
        sums = {r[key]["sum"] for b in side for r in side[b]}
        lines.append("%-22s %30s %30s %30s   %s | %s" % (key, cell(ms["parent A"], fmt=PER_LAUNCH), cell(ms["this"], fmt=PER_LAUNCH),
                                                        cell(ms["parent B"], fmt=PER_LAUNCH), T.inside(both, ms["this"]), len(sums) == 1))
    return lines


if __name__ == "__main__":
    main()
