#!/usr/bin/env python
"""Timing of the sw_plan_risk launch on one MI355X, by the method of tools/compose_timing.py: host clock around calls that end
in a host synchronisation, warm-up, then `--repeats` timed calls of each side, ALTERNATING, same seed for every call; median
and min / max, ms per call of the route.

The draws are those of the first chunk evaluate() forms of each of the three shapes of tools/_timing.py, all at K = 20: 816
agents in 102 scenes of 8, one scene of 8, 768 agents in 12 scenes of 64.  Two forms of the question:
  P = 1   leave-one-out, Q = B: every agent is the ego once, its plan is its ground-truth future (evaluate_risk());
  P = 64  Q = S: the middle agent of every scene is the ego with 64 candidate plans (64 more draws of it).
Against the only route the parent commit offers for a path that is not a row of the draws: put the plan into the ego's row
of all K draws and launch sw_scene_clearance on that tensor, then reduce with torch ops (min over k, count below coll_dist).
One such launch serves one ego per scene, so the route needs as many launches as the largest scene has agents (P = 1) or as
there are plans (P = 64) - and it gives clear_min and the index-paired count only, not the per-agent counts and their product.
Next to it evaluate_risk() against evaluate_scenes() on the whole held-out set, and with --parent-tree evaluate_scenes() at
this build and at the parent as the control (child processes alternating between the trees).  Nothing here passes or fails.

    python tools/plan_risk_timing.py [--repeats 9] [--parent-tree DIR] [--out profiles/plan_risk_timing.txt]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import COLL, PER_LAUNCH, cell, host_chunks  # noqa: E402

K, P_MANY = 20, 64


def launch_set(tr, data, just_one):
    ops = T.sw.ops
    _, obsv, pred, sb = next(host_chunks(tr, data, K, just_one))
    obsv, pred = obsv.contiguous(), pred.contiguous()
    B, dev = obsv.shape[0], obsv.device
    torch.manual_seed(5)
    ph = tr.G.sample(obsv, K, tr.n_next, sb, torch.rand(K, B, tr.noise_len, device=dev))
    scenes = ops.SceneIndex.get(sb, B, dev)
    inv_ss = 1.0 / float(data.ss)
    start = obsv[:, -1]
    off = scenes.scene_off.long()
    sizes = (off[1:] - off[:-1])
    n_max = int(sizes.max())
    q_scene, _ = scenes.row_scene()
    every = torch.arange(B, dtype=torch.int32, device=dev)
    loo_plans, loo_start = pred[:, None, :, :2].contiguous(), start[:, :2].contiguous()
    egos = (off[:-1] + sizes // 2).int()
    many = tr.G.sample(obsv, P_MANY, tr.n_next, sb, torch.rand(P_MANY, B, tr.noise_len, device=dev))
    many_plans = many[:, egos.long(), :, :2].permute(1, 0, 2, 3).contiguous()                     # (S, 64, Tp, 2)
    many_start = start[egos.long(), :2].contiguous()
    s_idx = torch.arange(scenes.S, dtype=torch.int32, device=dev)

    def risk_loo():
        out = ops.plan_risk(ph, start, scenes, K, loo_plans, loo_start, q_scene, every, COLL, inv_ss)
        torch.cuda.synchronize()
        return out

    def risk_many():
        out = ops.plan_risk(ph, start, scenes, K, many_plans, many_start, s_idx, egos, COLL, inv_ss)
        torch.cuda.synchronize()
        return out

    def composed(rows_of, plan_of, n):
        """n launches: launch j puts plan_of(j) into the rows rows_of(j) (one per scene that has one) of every draw"""
        def run():
            clear_min = torch.full((n, scenes.S), float("inf"), device=dev)
            count = torch.zeros(n, scenes.S, dtype=torch.int32, device=dev)
            for j in range(n):
                has, rows = rows_of(j)
                sub = ph.clone()
                sub[:, rows, :, :2] = plan_of(j, has, rows)[None]
                c = ops.scene_clearance(sub, start, scenes, K, inv_ss)[:, rows]
                clear_min[j, has] = c.min(0)[0]
                count[j, has] = (c < COLL).sum(0).int()
            torch.cuda.synchronize()
            return clear_min, count
        return run

    def loo_rows(j):
        has = sizes > j
        return has, (off[:-1] + j)[has]
    calls = {"risk_p1": risk_loo, "composed_p1": composed(loo_rows, lambda j, has, rows: pred[rows, :, :2], n_max),
             "risk_p64": risk_many,
             "composed_p64": composed(lambda j: (torch.ones_like(sizes, dtype=torch.bool), egos.long()),
                                      lambda j, has, rows: many_plans[:, j], P_MANY)}
    # the two routes agree where both answer: the smallest clearance and the index-paired count, bit for bit
    r1, c1 = risk_loo(), calls["composed_p1"]()
    for j in range(n_max):
        has, rows = loo_rows(j)
        assert torch.equal(r1[1][rows, 0], c1[0][j, has]) and torch.equal(r1[2][rows, 0, 0], c1[1][j, has])
    r64, c64 = risk_many(), calls["composed_p64"]()
    assert torch.equal(r64[1], c64[0].t()) and torch.equal(r64[2][..., 0], c64[1].t())
    return calls, B, scenes.S, n_max, float(r1[0].mean()), float(r64[0].mean())


def main():
    a = T.parse(__doc__, 9, 9, T.parent_tree_args)
    T.load("plan_risk_timing.py")
    tr = T.trainer()
    lines = ["sw_plan_risk (one launch, through ops.plan_risk) against the composed route of the parent commit (substituted tensor + "
             "sw_scene_clearance per launch + torch reductions) on the first evaluation chunk of each shape, K = %d; host clock, ms per "
             "call of the whole route; %d alternating repeats after %d warm-up calls; coll_dist %.1f; %s"
             % (K, a.repeats, a.warmup, COLL, torch.cuda.get_device_name(0)),
             "%-28s %5s %6s %30s %36s %30s %36s   %s" % ("shape (at K = 20)", "B", "scenes", "plan_risk P=1, Q=B median [min, max]",
                                                       "composed P=1 (launches)", "plan_risk P=64, Q=S", "composed P=64 (64 launches)",
                                                       "mean risk P=1, P=64")]
    evals = []
    for name, n_scenes, agents, _, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        calls, B, S, n_max, m1, m64 = launch_set(tr, data, just_one)
        ms, _ = T.alternate(calls, a.warmup, a.repeats)
        lines.append("%-28s %5d %6d %30s %30s (%3d) %30s %36s   %.4f, %.4f" % (
            name.split(":")[0] + ": first chunk", B, S, cell(ms["risk_p1"], fmt=PER_LAUNCH), cell(ms["composed_p1"], fmt=PER_LAUNCH),
            n_max, cell(ms["risk_p64"], fmt=PER_LAUNCH), cell(ms["composed_p64"], fmt=PER_LAUNCH), m1, m64))
        ev = {"evaluate_risk": lambda: tr.evaluate_risk(data, n_gen_samples=K, coll_dist=COLL, just_one=just_one),
              "evaluate_scenes": lambda: tr.evaluate_scenes(data, n_gen_samples=K, coll_dist=COLL, just_one=just_one)}
        ems, last = T.alternate(ev, a.warmup, a.repeats)
        evals.append((name, ems, last["evaluate_risk"]))
    lines.append("(the composed route answers less: the smallest clearance and the index-paired count, which the tool checks against "
                 "sw_plan_risk bit for bit before timing; every column includes the wrapper's output allocations)")
    lines.append("")
    lines.append("evaluate_risk() against evaluate_scenes() on the whole held-out set of each shape (K = %d; the latency shape: its first scene "
                 "only), ms per call" % K)
    lines.append("%-88s %30s %30s   %s" % ("shape", "evaluate_risk median [min, max]", "evaluate_scenes", "brier | brier_diag | brier_base | n_ego"))
    for name, ems, res in evals:
        lines.append("%-88s %30s %30s   %.4f | %.4f | %.4f | %d" % (name, cell(ems["evaluate_risk"]), cell(ems["evaluate_scenes"]),
                                                                  res["brier"], res["brier_diag"], res["brier_base"], res["n_ego"]))
    if a.parent_tree:
        res = T.across_builds(a.parent_tree, a.rounds, a.repeats, a.warmup, ("evaluate_scenes",), ("host",))
        lines.append("")
        lines.append("control: evaluate_scenes() at the parent build and at this build, %d alternating child processes of each" % a.rounds)
        lines.append("%-88s %30s %30s %-8s %s" % ("shape", "parent median [min, max]", "this median [min, max]", "inside", "equal"))
        for (shape, _, _), r in res.items():
            p, t = r["parent"], r["this"]
            lines.append("%-88s %30s %30s %-8s %s" % (shape, cell(p["ms"]), cell(t["ms"]), T.inside(p["ms"], t["ms"]), T.equal(r)))
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
