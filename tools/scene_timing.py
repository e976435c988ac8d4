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
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLL = 0.2
JOINT = ("jade_min", "jfde_min", "col_joint", "col_best", "col_agent", "col_gt")


def setup(tree):
    sys.path.insert(0, tree)
    import socialways_amd as sw
    sys.path.insert(0, os.path.join(HERE, "tools"))
    from sample_timing import SHAPES, held_out_set, timed
    if not torch.cuda.is_available():
        sys.exit("scene_timing.py measures on an MI355X: no GPU found")
    torch.manual_seed(0)
    return SHAPES, held_out_set, timed, sw.SocialWaysTrainer(12, use_social=True, device="cuda:0")


def alternate(calls, timed, warmup, repeats):
    for _ in range(warmup):
        for fn in calls.values():
            timed(fn)
    ms, last = {k: [] for k in calls}, {}
    for _ in range(repeats):
        for k, fn in calls.items():
            t, last[k] = timed(fn)
            ms[k].append(t)
    return ms, last


def cell(v):
    return "%9.3f [%8.3f, %8.3f]" % (statistics.median(v), min(v), max(v))


def torch_scene_metrics(tr, data, K, coll, just_one):
    """The numbers of evaluate_scenes() with torch ops: evaluate()'s chunks and host noise, Generator.sample(), then per
    scene broadcasting over (K, n, n, Tp) pairs; float64 sums on the device, one host sync at the end."""
    ss, dev, Tp = float(data.ss), tr.device, tr.n_next
    batches = [(int(b[0]), int(b[1])) for b in data.test_batches][:1 if just_one else None]
    acc = torch.zeros(10, dtype=torch.float64, device=dev)
    n_multi = agents_multi = 0

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
    for i, j in tr.eval_chunks(batches, K, tr.TEST_CHUNK):
        lo, hi = batches[i][0], batches[j - 1][1]
        obsv, pred = data.obsv[lo:hi], data.pred[lo:hi]
        with torch.no_grad():
            noise = tr.eval_noise(batches[i:j], K, tr.noise_len).to(dev)
            sb = np.asarray([[a - lo, b - lo] for a, b in batches[i:j]], dtype=np.int64)
            ph = tr.G.sample(obsv, K, Tp, sb, noise)[..., :2]
            e = ((ph - pred.unsqueeze(0)) / ss).pow(2).sum(-1).sqrt()                     # (K, n, Tp)
            ade, fde = e.mean(2), e[:, :, -1]
            four = torch.stack([ade.mean(0).sum(), fde.mean(0).sum(), ade.amin(0).sum(), fde.amin(0).sum()]).double()
            for a, b in batches[i:j]:
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
                col_gt=v[9] / z, n_scenes=len(batches), n_multi=n_multi)


def child(a):
    """evaluate() of the package under a.tree on the three shapes -> one JSON line {shape: [ms, ...]}."""
    SHAPES, held_out_set, timed, tr = setup(os.path.abspath(a.tree))
    out = {}
    for name, n_scenes, agents, K, just_one in SHAPES:
        data = held_out_set(n_scenes, agents, "cuda:0")
        ms, _ = alternate({"evaluate": lambda: tr.evaluate(data, n_gen_samples=K, just_one=just_one)}, timed, a.warmup, a.repeats)
        out[name] = ms["evaluate"]
    print("SCENE_TIMING " + json.dumps(out))


def across_builds(a, lines):
    trees = {"parent": os.path.abspath(a.parent_tree), "this": HERE}
    ms = {k: {} for k in trees}
    for _ in range(a.rounds):                  # one child at a time, alternating between the builds
        for k, tree in trees.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--repeats", str(a.repeats),
                                "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit("child on %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
            got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("SCENE_TIMING ")][-1][13:])
            for name, v in got.items():
                ms[k].setdefault(name, []).extend(v)
    lines.append("(a) evaluate() of the parent build vs this build: %d alternating child processes of each, %d timed calls per child "
                 "after %d warm-up calls" % (a.rounds, a.repeats, a.warmup))
    lines.append("%-88s %28s %28s %s" % ("shape", "parent median [min, max]", "this median [min, max]", "each median inside the other's range"))
    for name in ms["this"]:
        p, t = ms["parent"][name], ms["this"][name]
        mp, mt = statistics.median(p), statistics.median(t)
        lines.append("%-88s %28s %28s %s" % (name, cell(p), cell(t), min(t) <= mp <= max(t) and min(p) <= mt <= max(p)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="(a): child processes per build")
    ap.add_argument("--parent-tree", default=None, help="(a): a tree of the parent commit with its library built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("at least five repeats")
    if a.child:
        return child(a)
    lines = []
    if a.parent_tree:
        across_builds(a, lines)
    SHAPES, held_out_set, timed, tr = setup(HERE)
    lines.append("(b), (c) host clock around the call, ms; %d alternating repeats after %d warm-up calls of each; coll_dist %.1f; %s"
                 % (a.repeats, a.warmup, COLL, torch.cuda.get_device_name(0)))
    lines.append("%-88s %28s %28s %28s %8s %8s" % ("shape", "evaluate() median [min, max]", "evaluate_scenes()", "torch ops, scene by scene",
                                                  "(b)", "(c)"))
    for name, n_scenes, agents, K, just_one in SHAPES:
        data = held_out_set(n_scenes, agents, "cuda:0")
        calls = {"evaluate": lambda: tr.evaluate(data, n_gen_samples=K, just_one=just_one),
                 "scenes": lambda: tr.evaluate_scenes(data, n_gen_samples=K, coll_dist=COLL, just_one=just_one),
                 "torch": lambda: torch_scene_metrics(tr, data, K, COLL, just_one)}
        ms, last = alternate(calls, timed, a.warmup, a.repeats)
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
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
