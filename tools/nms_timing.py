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
import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
import socialways_amd as sw  # noqa: E402
from socialways_amd import ops  # noqa: E402
from sample_timing import SHAPES, held_out_set, timed  # noqa: E402
from scene_timing import alternate, cell  # noqa: E402

TOP_M, RADIUS, METRIC = 5, 0.5, "fde"
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
    """The numbers of evaluate_diverse() with the selection and its read-out formed by torch ops."""
    ss, dev, Tp = float(data.ss), tr.device, tr.n_next
    batches = [(int(b[0]), int(b[1])) for b in data.test_batches][:1 if just_one else None]
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    acc = torch.zeros(8, dtype=torch.float64, device=dev)
    for i, j in tr.eval_chunks(batches, K, tr.TEST_CHUNK):
        lo, hi = batches[i][0], batches[j - 1][1]
        obsv, pred = data.obsv[lo:hi], data.pred[lo:hi]
        n = hi - lo
        with torch.no_grad():
            noise = tr.eval_noise(batches[i:j], K, tr.noise_len).to(dev)
            sb = np.asarray([[a - lo, b - lo] for a, b in batches[i:j]], dtype=np.int64)
            scenes = ops.SceneIndex.get(sb, n, obsv.device)
            ph, per_agent, err, best = tr._sample_chunk(obsv, pred, noise, scenes, sb, K, ss)
            score, _ = tr.D.score_samples(obsv, ph.view(K, n, Tp, 4))
            off = scenes.scene_off if joint else None
            order, count, weight, assign = torch_nms(ph, score, M, radius, metric, 1.0 / ss, off)
            rows = torch.arange(n, device=dev)
            gid = torch.bucketize(rows, off[1:].long(), right=True) if joint else rows
            ro = order[gid]                                                            # (n, M)
            e = err.permute(1, 0, 2).gather(1, ro.clamp(min=0)[:, :, None].expand(-1, -1, 2))
            e = torch.where((ro >= 0)[:, :, None], e, torch.full_like(e, float("inf")))
            mb = assign[gid, best.long()]
            acc += torch.cat([e[:, 0].double().sum(0), e.amin(1).double().sum(0),
                              torch.stack([count.double().sum(), weight[:, 0].double().sum(), weight[gid, mb].double().sum(),
                                           mb.double().sum()])])
            sums += per_agent.double().sum(0)
    nt, n_agents = data.n_test_samples, sum(b - a for a, b in batches)
    ng = len(batches) if joint else n_agents
    out = dict(zip(("ade_avg", "fde_avg", "ade_min", "fde_min"), (sums / nt).tolist()))
    out.update(zip(NEW, (acc / torch.tensor([nt] * 4 + [ng] * 2 + [nt] * 2, dtype=torch.float64, device=dev)).tolist()))
    return out


def first_chunk(tr, data, K, just_one):
    batches = [(int(b[0]), int(b[1])) for b in data.test_batches][:1 if just_one else None]
    i, j = next(iter(tr.eval_chunks(batches, K, tr.TEST_CHUNK)))
    lo, hi = batches[i][0], batches[j - 1][1]
    sb = np.asarray([[a - lo, b - lo] for a, b in batches[i:j]], dtype=np.int64)
    return data.obsv[lo:hi].contiguous(), sb


def launch_pair(tr, data, K, just_one, joint, launches):
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20, help="(b): selections per timed call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 9:
        ap.error("at least nine repeats")
    if not torch.cuda.is_available():
        sys.exit("nms_timing.py measures on an MI355X: no GPU found")
    torch.manual_seed(0)
    tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0")
    lines = ["(a) host clock around the call, ms; %d alternating repeats after %d warm-up calls of each; top_m %d, radius %.2f, %s; %s"
             % (a.repeats, a.warmup, TOP_M, RADIUS, METRIC, torch.cuda.get_device_name(0)),
             "%-88s %-6s %28s %28s %28s %9s %9s %s" % ("shape", "groups", "evaluate_ranked() median [min, max]", "evaluate_diverse()",
                                                       "same, selection by torch ops", "kernel", "torch", "max(kernel side) < min(torch side)")]
    for name, n_scenes, agents, K, just_one in SHAPES:
        data = held_out_set(n_scenes, agents, "cuda:0")
        for joint in (False, True):
            calls = {"ranked": lambda: tr.evaluate_ranked(data, n_gen_samples=K, top_m=TOP_M, just_one=just_one),
                     "diverse": lambda: tr.evaluate_diverse(data, n_gen_samples=K, top_m=TOP_M, radius=RADIUS, metric=METRIC,
                                                            joint=joint, just_one=just_one),
                     "torch": lambda: torch_diverse(tr, data, K, TOP_M, RADIUS, METRIC, joint, just_one)}
            ms, last = alternate(calls, timed, a.warmup, a.repeats)
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
    for name, n_scenes, agents, K, just_one in SHAPES:
        data = held_out_set(n_scenes, agents, "cuda:0")
        for joint in (False, True):
            calls, B, same = launch_pair(tr, data, K, just_one, joint, a.launches)
            ms, _ = alternate(calls, lambda fn: (timed(fn)[0] / a.launches, None), a.warmup, a.repeats)
            k, t = ms["kernel"], ms["torch"]
            lines.append("%-88s %-6s %6d %5d %28s %28s %8.3f %12.6f" % (
                name, "scene" if joint else "agent", B, K, "%9.4f [%8.4f, %8.4f]" % (statistics.median(k), min(k), max(k)),
                "%9.4f [%8.4f, %8.4f]" % (statistics.median(t), min(t), max(t)), statistics.median(k) / statistics.median(t), same))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
