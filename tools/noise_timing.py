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
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sw = None      # socialways_amd, imported from --tree in main()

# name, held-out scenes, agents per scene, K, just_one
SHAPES = (("throughput: 256 held-out scenes x 8 agents, K = 20, full set", 256, 8, 20, False),
          ("latency: same set, K = 128, first scene only", 256, 8, 128, True),
          ("dense: 16 held-out scenes x 64 agents, K = 20, full set", 16, 64, 20, False))
# name, scenes per packed batch, agents per scene, packed batches per epoch
TRAIN_SHAPES = (("m1: 256 scenes x 8 agents per packed batch", 256, 8, 8),
                ("c4: 512 scenes x 64 agents per packed batch", 512, 64, 4))


def held_out_set(n_test_scenes, agents, device):
    """SceneDataset keeps the last fifth of the scenes for testing: 5 x n scenes give n held-out ones."""
    tracks = sw.synth_tracks(5 * n_test_scenes, agents, 8, 12, seed=4321)
    data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], tracks["times"], device=device)
    assert len(data.test_batches) == n_test_scenes
    return data


def timed(fn):
    torch.manual_seed(123)
    np.random.seed(123)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()                     # ends in a device -> host copy of the metrics / losses
    return (time.perf_counter() - t0) * 1e3, out


def ab(calls, warmup, repeats):
    """calls: {name: fn} -> ({name: [ms]}, {name: last result}); the forms alternate inside every repeat."""
    for _ in range(warmup):
        for fn in calls.values():
            timed(fn)
    ms, last = {k: [] for k in calls}, {}
    for _ in range(repeats):
        for k, fn in calls.items():
            t, last[k] = timed(fn)
            ms[k].append(t)
    return ms, last


def cell(v, scale=1.0):
    return "%9.3f [%8.3f, %8.3f]" % (statistics.median(v) / scale, min(v) / scale, max(v) / scale)


def child(a, tr):
    """evaluate() of the package under a.tree on the three shapes -> one JSON line {shape: [ms, ...]}."""
    out = {}
    for name, n_scenes, agents, K, just_one in SHAPES:
        data = held_out_set(n_scenes, agents, "cuda:0")
        ms, _ = ab({"evaluate": lambda: tr.evaluate(data, n_gen_samples=K, just_one=just_one)}, a.warmup, a.repeats)
        out[name] = ms["evaluate"]
    print("NOISE_TIMING " + json.dumps(out))


def across_builds(a, lines):
    trees = {"parent": os.path.abspath(a.parent_tree), "this": HERE}
    ms = {k: {} for k in trees}
    for _ in range(a.rounds):                  # one child at a time, alternating between the builds
        for k, tree in trees.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--repeats", str(a.repeats),
                                "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit("child on %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
            got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("NOISE_TIMING ")][-1][13:])
            for name, v in got.items():
                ms[k].setdefault(name, []).extend(v)
    lines.append("")
    lines.append("evaluate() on the host stream, parent build vs this build: %d alternating child processes of each, %d timed calls "
                 "per child after %d warm-up calls" % (a.rounds, a.repeats, a.warmup))
    lines.append("%-66s %28s %28s %s" % ("shape", "parent median [min, max]", "this median [min, max]", "each median inside the other's range"))
    for name in ms["this"]:
        p, t = ms["parent"][name], ms["this"][name]
        mp, mt = statistics.median(p), statistics.median(t)
        lines.append("%-66s %28s %28s %s" % (name, cell(p), cell(t), min(t) <= mp <= max(t) and min(p) <= mt <= max(p)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="--parent-tree: child processes per build")
    ap.add_argument("--parent-tree", default=None, help="a tree of the parent commit with its library built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("at least five repeats")
    if not torch.cuda.is_available():
        sys.exit("noise_timing.py measures on an MI355X: no GPU found")
    global sw
    sys.path.insert(0, os.path.abspath(a.tree))
    import socialways_amd as sw
    assert os.path.dirname(os.path.dirname(os.path.abspath(sw.__file__))) == os.path.abspath(a.tree), sw.__file__
    dev = "cuda:0"
    torch.manual_seed(0)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=dev)
    if a.child:
        return child(a, tr)
    head = "host clock around the call (every call returns host numbers), ms; %d alternating repeats after %d warm-up calls of " \
           "each; %s" % (a.repeats, a.warmup, torch.cuda.get_device_name(0))
    lines = []
    dn = sw.DeviceNoise(2019)
    lines.append("host noise stream vs DeviceNoise: " + head)
    lines.append("%-66s %-18s %28s %28s %8s" % ("shape", "call", "host stream median [min, max]", "DeviceNoise median [min, max]", "ratio"))
    for name, n_scenes, agents, K, just_one in SHAPES:
        data = held_out_set(n_scenes, agents, dev)
        for what, fn in (("evaluate", lambda nz: tr.evaluate(data, n_gen_samples=K, just_one=just_one, noise=nz)),
                         ("evaluate_ranked", lambda nz: tr.evaluate_ranked(data, n_gen_samples=K, top_m=5, just_one=just_one,
                                                                           noise=nz))):
            ms, last = ab({"host": lambda: fn(None), "device": lambda: fn(dn)}, a.warmup, a.repeats)
            lines.append("%-66s %-18s %28s %28s %8.3f" % (name, what + "()", cell(ms["host"]), cell(ms["device"]),
                                                          statistics.median(ms["device"]) / statistics.median(ms["host"])))
            if what == "evaluate":
                lines.append("    metrics, host stream %s" % np.array2string(np.asarray(last["host"]), precision=7))
                lines.append("    metrics, DeviceNoise %s" % np.array2string(np.asarray(last["device"]), precision=7))
        batches = [(int(b[0]), int(b[1])) for b in data.test_batches][:1 if just_one else None]
        host, fill = [], []
        for _ in range(a.repeats):        # the two noise sources alone: host draws + padding + copy, and the fill launches
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, j in tr.eval_chunks(batches, K, tr.TEST_CHUNK):
                tr._eval_z(None, batches[i:j], K, batches[i][0], batches[j - 1][1] - batches[i][0])
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for i, j in tr.eval_chunks(batches, K, tr.TEST_CHUNK):
                tr._eval_z(dn, batches[i:j], K, batches[i][0], batches[j - 1][1] - batches[i][0])
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
            trs = {}
            for k in ("host", "device"):
                torch.manual_seed(0)
                trs[k] = sw.SocialWaysTrainer(12, use_social=True, device=dev)
            trs["device"].noise = sw.DeviceNoise(2019)
            ms, _ = ab({k: (lambda t=t: t.train_epoch(data, bs)) for k, t in trs.items()}, 3, a.repeats)
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
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
