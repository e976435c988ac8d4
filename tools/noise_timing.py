#!/usr/bin/env python
"""A/B timing of the reference's host noise streams against the device noise stream (DeviceNoise) on one MI355X.

Evaluation: SocialWaysTrainer.evaluate() and evaluate_ranked() with noise=None (eval_noise: K torch.rand calls per held-out
scene on the host, padded and copied) against noise=DeviceNoise (one fill launch per chunk), same trainer, same data, at the
three shapes of tools/sample_timing.py.  Training: train_epoch() per packed batch with and without trainer.noise at the m1
(256 scenes x 8 agents) and c4 (512 scenes x 64 agents) batch shapes of bench.py, two identically built trainers.  Every
timed call ends in a host synchronisation (metrics / losses come back as host numbers), so a host clock around it measures
the work.  Per shape: warm-up of both forms, then `--repeats` timed calls of each, ALTERNATING; median and min / max.

`--parent-tree DIR` (a tree of the parent commit with its library built): evaluate() on the host stream - the untouched
default path - of that build against this one.  Two trees cannot share a process, so each side runs in child processes of
its own, `--rounds` of each, alternating; medians with min / max over all their calls.

    python tools/noise_timing.py [--repeats 9] [--parent-tree ab_old] [--out profiles/noise_eval_ab.txt]
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import cell  # noqa: E402

# name, scenes per packed batch, agents per scene, packed batches per epoch
TRAIN_SHAPES = (("m1: 256 scenes x 8 agents per packed batch", 256, 8, 8),
                ("c4: 512 scenes x 64 agents per packed batch", 512, 64, 4))


def across_builds(a, lines):
    res = T.across_builds(a.parent_tree, a.rounds, a.repeats, a.warmup)
    lines.append("")
    lines.append("evaluate() on the host stream, parent build vs this build: %d alternating child processes of each, %d timed calls "
                 "per child after %d warm-up calls" % (a.rounds, a.repeats, a.warmup))
    lines.append("%-66s %28s %28s %s" % ("shape", "parent median [min, max]", "this median [min, max]", "each median inside the other's range"))
    for (name, _, _), r in res.items():
        p, t = r["parent"]["ms"], r["this"]["ms"]
        lines.append("%-66s %28s %28s %s" % (name.split(" (")[0], cell(p), cell(t), T.inside(p, t)))


def main():
    def more(ap):
        T.parent_tree_args(ap)
        ap.add_argument("--skip-train", action="store_true")
    a = T.parse(__doc__, 9, 5, more)
    sw = T.load("noise_timing.py")
    dev = "cuda:0"
    tr = T.trainer()
    head = "host clock around the call (every call returns host numbers), ms; %d alternating repeats after %d warm-up calls of " \
           "each; %s" % (a.repeats, a.warmup, torch.cuda.get_device_name(0))
    lines = []
    dn = sw.DeviceNoise(2019)
    lines.append("host noise stream vs DeviceNoise: " + head)
    lines.append("%-66s %-18s %28s %28s %8s" % ("shape", "call", "host stream median [min, max]", "DeviceNoise median [min, max]", "ratio"))
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        for what, fn in (("evaluate", lambda nz: tr.evaluate(data, n_gen_samples=K, just_one=just_one, noise=nz)),
                         ("evaluate_ranked", lambda nz: tr.evaluate_ranked(data, n_gen_samples=K, top_m=5, just_one=just_one,
                                                                           noise=nz))):
            ms, last = T.alternate({"host": lambda: fn(None), "device": lambda: fn(dn)}, a.warmup, a.repeats)
            lines.append("%-66s %-18s %28s %28s %8.3f" % (name.split(" (")[0], what + "()", cell(ms["host"]), cell(ms["device"]),
                                                          statistics.median(ms["device"]) / statistics.median(ms["host"])))
            if what == "evaluate":
                lines.append("    metrics, host stream %s" % np.array2string(np.asarray(last["host"]), precision=7))
                lines.append("    metrics, DeviceNoise %s" % np.array2string(np.asarray(last["device"]), precision=7))
        host, fill = [], []
        for _ in range(a.repeats):        # the two noise sources alone: host draws + padding + copy, and the fill launches
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for scenes, _, _, _ in T.host_chunks(tr, data, K, just_one):
                tr._pad_z(tr.eval_noise(scenes, K, tr.noise_len)).to(dev)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for scenes, obsv, _, _ in T.host_chunks(tr, data, K, just_one):
                dn.fill(obsv.shape[0], tr.noise_len, domain=sw.noise.EVAL, n_draws=K, row0=scenes[0][0], ld=tr.Z_COLS, device=dev)
            torch.cuda.synchronize()
            fill.append((time.perf_counter() - t0) * 1e3)
        lines.append("    z alone, to a synchronise: host draws + pad + copy median %.3f ms, fill launches median %.3f ms"
                     % (statistics.median(host), statistics.median(fill)))
    if not a.skip_train:
        lines.append("")
        lines.append("train_epoch() per packed batch (epoch wall time / batches), ms; 3 warm-up epochs of each (eager, eager, capture)")
        lines.append("%-52s %28s %28s %8s" % ("shape", "host z median [min, max]", "trainer.noise median [min, max]", "ratio"))
        for name, scenes, agents, n_batches in TRAIN_SHAPES:
            tracks = sw.synth_tracks(5 * scenes * n_batches // 4, agents, 8, 12, seed=4321)
            data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], device=dev)
            bs = scenes * agents
            steps = len(list(data.packed_steps(bs)))
            trs = {k: T.trainer() for k in ("host", "device")}
            trs["device"].noise = sw.DeviceNoise(2019)
            ms, _ = T.alternate({k: (lambda t=t: t.train_epoch(data, bs)) for k, t in trs.items()}, 3, a.repeats)
            lines.append("%-52s %28s %28s %8.3f" % ("%s, %d batches per epoch" % (name, steps), cell(ms["host"], steps),
                                                    cell(ms["device"], steps),
                                                    statistics.median(ms["device"]) / statistics.median(ms["host"])))
            for t in trs.values():
                t.release_graphs()
            del trs, data
            torch.cuda.empty_cache()
    del tr
    torch.cuda.empty_cache()
    if a.parent_tree:
        across_builds(a, lines)
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
