#!/usr/bin/env python
"""Timing of SocialWaysTrainer.evaluate_diverse() and of the sw_sample_nms launch on one MI355X, on the three shapes of
tools/sample_timing.py and by its method: host clock around calls that end in a host synchronisation, warm-up, then
`--repeats` timed calls of each side, ALTERNATING, same seed for every call; median and min / max.

  (a) evaluate_diverse() (per agent and per scene) against the same numbers with the selection formed by torch ops on the
      device: the same chunks, host noise, sampling and scoring launches, then the (K, K, n) pair distances by broadcasting,
      top_m masked arg-max / suppress steps over all groups at once, float64 sums, one host sync at the end.
      evaluate_ranked() is timed next to both: it shares everything but the selection.
  (b) one sw_sample_nms launch against that torch-ops selection alone, on the draws and scores of the first chunk
      evaluate() forms of each shape.  One timed call = `--launches` selections back to back and a synchronisation; ms each.

    python tools/nms_timing.py [--repeats 9] [--out profiles/nms_timing.txt]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import METRIC, PER_LAUNCH, RADIUS, TOP_M, cell, first_chunk  # noqa: E402

NEW = ("ade_div1", "fde_div1", "ade_divm", "fde_divm", "n_modes", "w_first", "w_hit", "rank_hit")


def torch_nms(pos, score, M, radius, metric, inv_ss, scene_off=None):
    """The selection of sw_sample_nms with torch ops, all groups at once: (order (G, M), count (G,), weight (G, M),
    assign (G, K)).  Ties between equal scores go to the lowest k; equal leftover distances to whatever argmin returns."""
    K, n = score.shape
    p = pos.view(K, n, -1, pos.shape[-1])[..., :2]
    d = (p[:, None] - p[None]).pow(2).sum(-1).sqrt()                                   # (K, K, n, Tp)
    D = inv_ss * (d[..., -1] if metric == "fde" else d.mean(-1))                       # (K, K, n)
    s = score
    if scene_off is not None:
        S = scene_off.numel() - 1
        gid = torch.bucketize(torch.arange(n, device=pos.device), scene_off[1:].long(), right=True)
        D = torch.zeros(K, K, S, device=pos.device).scatter_reduce(2, gid.expand(K, K, n), D, "amax")
        s = torch.full((K, S), float("inf"), device=pos.device).scatter_reduce(1, gid.expand(K, n), score, "amin")
    G = s.shape[1]
    ks = torch.arange(K, device=pos.device)[:, None]
    alive = torch.ones(K, G, dtype=torch.bool, device=pos.device)
    assign = torch.full((K, G), -1, dtype=torch.long, device=pos.device)
    order, dist = [], []
    for m in range(M):
        sm = torch.where(alive, s, torch.full_like(s, float("-inf")))
        c = torch.where(alive & (sm == sm.max(dim=0)[0]), ks, K).min(dim=0)[0]           # (G,); K = nothing alive
        some = c < K
        Dc = D.gather(1, c.clamp(max=K - 1)[None, None, :].expand(K, 1, G))[:, 0]      # D[k, c_g, g]
        gone = alive & (Dc <= radius) & some
        assign = torch.where(gone, m, assign)
        alive = alive & ~gone
        order.append(torch.where(some, c, -1))
        dist.append(torch.where(some, Dc, torch.full_like(Dc, float("inf"))))
    order = torch.stack(order, dim=1)                                                  # (G, M)
    assign = torch.where(alive, torch.stack(dist).argmin(dim=0), assign).t()           # (G, K)
    count = (order >= 0).sum(dim=1)
    weight = (assign[:, None, :] == torch.arange(M, device=pos.device)[None, :, None]).sum(dim=2).float() / K
    return order, count, weight, assign


def torch_diverse(tr, data, K, M, radius, metric, joint, just_one):
    """The numbers of evaluate_diverse() with the selection and its read-out formed by torch ops: the chunks, draws and scores
    are the call's own (the trainer's chunk generator, Discriminator.score_samples)."""
    dev = tr.device
    base = T.sw.trainer._EvalSums(dev)
    acc = torch.zeros(8, dtype=torch.float64, device=dev)
    for c in tr._eval_draws(data, K, just_one, None, base):
        score, _ = tr.D.score_samples(c.obsv, c.ph)
        off = c.scenes.scene_off if joint else None
        order, count, weight, assign = torch_nms(c.ph, score, M, radius, metric, 1.0 / float(data.ss), off)
        rows = torch.arange(c.n, device=dev)
        gid = torch.bucketize(rows, off[1:].long(), right=True) if joint else rows
        ro = order[gid]                                                            # (n, M)
        e = c.err.permute(1, 0, 2).gather(1, ro.clamp(min=0)[:, :, None].expand(-1, -1, 2))
        e = torch.where((ro >= 0)[:, :, None], e, torch.full_like(e, float("inf")))
        mb = assign[gid, c.best.long()]
        acc += torch.cat([e[:, 0].double().sum(0), e.amin(1).double().sum(0),
                          torch.stack([count.double().sum(), weight[:, 0].double().sum(), weight[gid, mb].double().sum(),
                                       mb.double().sum()])])
    nt, n_agents = data.n_test_samples, sum(b - a for a, b in base.scenes)
    ng = len(base.scenes) if joint else n_agents
    out = base.result(data)
    out.update(zip(NEW, (acc / torch.tensor([nt] * 4 + [ng] * 2 + [nt] * 2, dtype=torch.float64, device=dev)).tolist()))
    return out


def launch_pair(tr, data, K, just_one, joint, launches):
    ops = T.sw.ops
    obsv, sb = first_chunk(tr, data, K, just_one)
    B = obsv.shape[0]
    torch.manual_seed(5)
    ph = tr.G.sample(obsv, K, tr.n_next, sb)
    score, _ = tr.D.score_samples(obsv, ph)
    scenes = ops.SceneIndex.get(sb, B, obsv.device) if joint else None
    inv_ss = 1.0 / float(data.ss)
    got = ops.sample_nms(ph, score, K, TOP_M, RADIUS, METRIC, scenes, inv_ss)
    want = torch_nms(ph, score, TOP_M, RADIUS, METRIC, inv_ss, scenes.scene_off if joint else None)
    same = float((got[0].long() == want[0]).double().mean())      # a distance within rounding of the radius may differ

    def kernel():
        for _ in range(launches):
            out = ops.sample_nms(ph, score, K, TOP_M, RADIUS, METRIC, scenes, inv_ss)
        torch.cuda.synchronize()
        return out

    def torch_ops():
        for _ in range(launches):
            out = torch_nms(ph, score, TOP_M, RADIUS, METRIC, inv_ss, scenes.scene_off if joint else None)
        torch.cuda.synchronize()
        return out
    return {"kernel": kernel, "torch": torch_ops}, B, same


def main():
    a = T.parse(__doc__, 9, 9, lambda ap: ap.add_argument("--launches", type=int, default=20, help="(b): selections per timed call"))
    T.load("nms_timing.py")
    tr = T.trainer()
    lines = ["(a) host clock around the call, ms; %d alternating repeats after %d warm-up calls of each; top_m %d, radius %.2f, %s; %s"
             % (a.repeats, a.warmup, TOP_M, RADIUS, METRIC, torch.cuda.get_device_name(0)),
             "%-88s %-6s %28s %28s %28s %9s %9s %s" % ("shape", "groups", "evaluate_ranked() median [min, max]", "evaluate_diverse()",
                                                       "same, selection by torch ops", "kernel", "torch", "max(kernel side) < min(torch side)")]
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        for joint in (False, True):
            calls = {"ranked": lambda: T.CALLS["evaluate_ranked"](tr, data, K, just_one),
                     "diverse": lambda: T.CALLS["evaluate_diverse, joint" if joint else "evaluate_diverse"](tr, data, K, just_one),
                     "torch": lambda: torch_diverse(tr, data, K, TOP_M, RADIUS, METRIC, joint, just_one)}
            ms, last = T.alternate(calls, a.warmup, a.repeats)
            med = {k: statistics.median(v) for k, v in ms.items()}
            lines.append("%-88s %-6s %28s %28s %28s %9.3f %9.3f %s" % (
                name, "scene" if joint else "agent", cell(ms["ranked"]), cell(ms["diverse"]), cell(ms["torch"]),
                med["diverse"] - med["ranked"], med["torch"] - med["ranked"], max(ms["diverse"]) < min(ms["torch"])))
            for k in ("diverse", "torch"):
                lines.append("    %-19s %s" % ("evaluate_diverse()" if k == "diverse" else "torch ops",
                                               " ".join("%s %.6f" % (x, last[k][x]) for x in NEW)))
    lines.append("    (columns `kernel` / `torch`: median minus evaluate_ranked()'s, which differs from both by its own ranking launch)")
    lines.append("")
    lines.append("(b) one sw_sample_nms launch vs the torch-ops selection on the same draws and scores; first chunk of each shape; ms per "
                 "selection, %d per timed call; %d alternating repeats after %d warm-up calls" % (a.launches, a.repeats, a.warmup))
    lines.append("%-88s %-6s %6s %5s %28s %28s %8s %12s" % ("shape", "groups", "B", "K", "sw_sample_nms median [min, max]", "torch ops",
                                                          "ratio", "equal picks"))
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        for joint in (False, True):
            calls, B, same = launch_pair(tr, data, K, just_one, joint, a.launches)
            ms, _ = T.alternate(calls, a.warmup, a.repeats)
            k, t = ([x / a.launches for x in ms[side]] for side in ("kernel", "torch"))
            lines.append("%-88s %-6s %6d %5d %28s %28s %8.3f %12.6f" % (
                name, "scene" if joint else "agent", B, K, cell(k, fmt=PER_LAUNCH),
                cell(t, fmt=PER_LAUNCH), statistics.median(k) / statistics.median(t), same))
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
