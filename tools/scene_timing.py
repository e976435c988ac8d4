#!/usr/bin/env python
"""Timing of SocialWaysTrainer.evaluate_scenes() on one MI355X, on the three shapes of tools/sample_timing.py and by its
method: host clock around calls that end in a host synchronisation (the results come back as Python floats), warm-up, then
`--repeats` timed calls of each side, ALTERNATING, same seed for every call; median and min / max.

  (a) evaluate() of another build of the package (`--parent-tree DIR`: a tree of the parent commit with its library built)
      against evaluate() of this one.  Two trees cannot share a process, so each side runs in child processes of its own,
      one at a time and alternating; nothing on that path may differ, so each median should lie inside the other's range.
  (b) evaluate_scenes() against evaluate(): the price of the scene metrics.
  (c) evaluate_scenes() against the same numbers formed with torch ops on the device from Generator.sample() output,
      scene by scene - what a user of the library would have written without the two kernels.

    python tools/scene_timing.py [--repeats 7] [--parent-tree ab_old] [--out profiles/scene_metrics_ab.txt]
"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import COLL, cell  # noqa: E402

JOINT = ("jade_min", "jfde_min", "col_joint", "col_best", "col_agent", "col_gt")


def torch_scene_metrics(tr, data, K, coll, just_one):
    """The numbers of evaluate_scenes() with torch ops: evaluate()'s chunks and host noise, Generator.sample(), then per
    scene broadcasting over (K, n, n, Tp) pairs; float64 sums on the device, one host sync at the end."""
    ss, dev, Tp = float(data.ss), tr.device, tr.n_next
    acc = torch.zeros(10, dtype=torch.float64, device=dev)
    n_scenes = n_multi = agents_multi = 0

    def clearance(path):                                   # (K, n, Tp + 1, 2) -> (K, n)
        n = path.shape[1]
        r0 = path[:, :, None, :-1] - path[:, None, :, :-1]
        dv = (path[:, :, None, 1:] - path[:, None, :, 1:]) - r0
        dd, rd = (dv * dv).sum(-1), (r0 * dv).sum(-1)
        tau = torch.where(dd > 0, (-rd / torch.where(dd > 0, dd, torch.ones_like(dd))).clamp(0, 1), torch.zeros_like(dd))
        c = r0 + tau.unsqueeze(-1) * dv
        d = (c * c).sum(-1).sqrt().amin(-1) / ss
        d = d.masked_fill(torch.eye(n, dtype=torch.bool, device=dev), float("inf"))
        return d.amin(-1)
    for scenes, obsv, pred, sb in T.host_chunks(tr, data, K, just_one):
        lo = scenes[0][0]
        n_scenes += len(scenes)
        with torch.no_grad():
            noise = tr.eval_noise(scenes, K, tr.noise_len).to(dev)
            ph = tr.G.sample(obsv, K, Tp, sb, noise)[..., :2]
            e = ((ph - pred.unsqueeze(0)) / ss).pow(2).sum(-1).sqrt()                     # (K, n, Tp)
            ade, fde = e.mean(2), e[:, :, -1]
            four = torch.stack([ade.mean(0).sum(), fde.mean(0).sum(), ade.amin(0).sum(), fde.amin(0).sum()]).double()
            for a, b in scenes:
                r, n = slice(a - lo, b - lo), b - a
                sade, sfde = ade[:, r].mean(1), fde[:, r].mean(1)
                acc[4] += n * sade.amin().double()
                acc[5] += n * sfde.amin().double()
                if n > 1:
                    last = obsv[r, -1:]
                    c = clearance(torch.cat([last.unsqueeze(0).expand(K, n, 1, 2), ph[:, r]], 2))
                    flags = c < coll
                    acc[6] += flags.any(1).double().mean()
                    acc[7] += flags[sade.argmin()].any().double()
                    acc[8] += flags.double().sum() / K
                    acc[9] += (clearance(torch.cat([last, pred[r]], 1).unsqueeze(0)) < coll).any().double()
                    n_multi += 1
                    agents_multi += n
            acc[:4] += four
    v = acc.tolist()
    nt, z = data.n_test_samples, max(n_multi, 1)
    return dict(ade_avg=v[0] / nt, fde_avg=v[1] / nt, ade_min=v[2] / nt, fde_min=v[3] / nt, jade_min=v[4] / nt,
                jfde_min=v[5] / nt, col_joint=v[6] / z, col_best=v[7] / z, col_agent=v[8] / max(agents_multi, 1),
                col_gt=v[9] / z, n_scenes=n_scenes, n_multi=n_multi)


def across_builds(a, lines):
    res = T.across_builds(a.parent_tree, a.rounds, a.repeats, a.warmup)
    lines.append("(a) evaluate() of the parent build vs this build: %d alternating child processes of each, %d timed calls per child "
                 "after %d warm-up calls" % (a.rounds, a.repeats, a.warmup))
    lines.append("%-88s %28s %28s %s" % ("shape", "parent median [min, max]", "this median [min, max]", "each median inside the other's range"))
    for (name, _, _), r in res.items():
        p, t = r["parent"]["ms"], r["this"]["ms"]
        lines.append("%-88s %28s %28s %s" % (name, cell(p), cell(t), T.inside(p, t)))


def main():
    a = T.parse(__doc__, 7, 5, T.parent_tree_args)
    T.load("scene_timing.py")
    lines = []
    if a.parent_tree:
        across_builds(a, lines)
    tr = T.trainer()
    lines.append("(b), (c) host clock around the call, ms; %d alternating repeats after %d warm-up calls of each; coll_dist %.1f; %s"
                 % (a.repeats, a.warmup, COLL, torch.cuda.get_device_name(0)))
    lines.append("%-88s %28s %28s %28s %8s %8s" % ("shape", "evaluate() median [min, max]", "evaluate_scenes()", "torch ops, scene by scene",
                                                  "(b)", "(c)"))
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        calls = {"evaluate": lambda: T.CALLS["evaluate"](tr, data, K, just_one),
                 "scenes": lambda: T.CALLS["evaluate_scenes"](tr, data, K, just_one),
                 "torch": lambda: torch_scene_metrics(tr, data, K, COLL, just_one)}
        ms, last = T.alternate(calls, a.warmup, a.repeats)
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append("%-88s %28s %28s %28s %8.3f %8.3f" % (name, cell(ms["evaluate"]), cell(ms["scenes"]), cell(ms["torch"]),
                                                         med["scenes"] / med["evaluate"], med["scenes"] / med["torch"]))
        lines.append("    evaluate()          %s" % np.array2string(np.asarray(last["evaluate"]), precision=7))
        for k in ("scenes", "torch"):
            r = last[k]
            lines.append("    %-19s %s | %s | scenes %d, multi-agent %d" % (
                "evaluate_scenes()" if k == "scenes" else "torch ops",
                np.array2string(np.asarray([r[x] for x in ("ade_avg", "fde_avg", "ade_min", "fde_min")]), precision=7),
                " ".join("%s %.6f" % (x, r[x]) for x in JOINT), r["n_scenes"], r["n_multi"]))
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
