#!/usr/bin/env python
"""A/B timing of SocialWaysTrainer.test() against SocialWaysTrainer.evaluate() on one MI355X.

Both calls do the same job on the same trainer and data (K sampled futures per held-out scene -> avg / min-over-K ADE &
FDE): test() replicates the chunk K times through Generator.forward and reduces with torch ops, evaluate() encodes once,
rolls out the K copies in one sampling launch and reduces on the device.  Both end in a host synchronisation (the metrics
come back as Python floats), so a host clock around a call measures the work.  Per shape: warm-up of both, then `--repeats`
timed calls of each, ALTERNATING, same seed for every call; median and min / max are reported, and the metrics of the two
are printed next to each other.

    python tools/sample_timing.py [--repeats 7] [--out profiles/sample_eval_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import socialways_amd as sw  # noqa: E402

# name, held-out scenes, agents per scene, K, just_one
SHAPES = (("throughput: 256 held-out scenes x 8 agents, K = 20, full set", 256, 8, 20, False),
          ("latency: same set, K = 128, first scene only (the driver's call every five epochs)", 256, 8, 128, True),
          ("dense: 16 held-out scenes x 64 agents, K = 20, full set", 16, 64, 20, False))


def held_out_set(n_test_scenes, agents, device):
    """SceneDataset keeps the last fifth of the scenes for testing: 5 x n scenes give n held-out ones."""
    tracks = sw.synth_tracks(5 * n_test_scenes, agents, 8, 12, seed=4321)
    data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], tracks["times"], device=device)
    assert len(data.test_batches) == n_test_scenes
    return data


def timed(fn):
    torch.manual_seed(123)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()                     # ends in a device -> host copy of the metrics
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("at least five repeats")
    if not torch.cuda.is_available():
        sys.exit("sample_timing.py measures on an MI355X: no GPU found")
    dev = "cuda:0"
    torch.manual_seed(0)
    tr = sw.SocialWaysTrainer(12, use_social=True, device=dev)
    lines = ["test() vs evaluate(): host clock around the call (both return host floats), ms; %d alternating repeats after %d "
             "warm-up calls of each; %s" % (a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "%-88s %28s %28s %8s" % ("shape", "test() median [min, max]", "evaluate() median [min, max]", "ratio")]
    for name, n_scenes, agents, K, just_one in SHAPES:
        data = held_out_set(n_scenes, agents, dev)
        calls = {"test": lambda: tr.test(data, n_gen_samples=K, just_one=just_one),
                 "evaluate": lambda: tr.evaluate(data, n_gen_samples=K, just_one=just_one)}
        for _ in range(a.warmup):
            for fn in calls.values():
                timed(fn)
        ms = {k: [] for k in calls}
        last = {}
        for _ in range(a.repeats):
            for k, fn in calls.items():
                t, last[k] = timed(fn)
                ms[k].append(t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        cell = lambda k: "%9.3f [%8.3f, %8.3f]" % (med[k], min(ms[k]), max(ms[k]))
        lines.append("%-88s %28s %28s %8.3f" % (name, cell("test"), cell("evaluate"), med["evaluate"] / med["test"]))
        batches = [(int(b[0]), int(b[1])) for b in data.test_batches][:1 if just_one else None]
        host = []
        for _ in range(a.repeats):        # the part both calls share: the reference's host noise stream (train.py:584)
            t0 = time.perf_counter()
            for i, j in tr.eval_chunks(batches, K, tr.TEST_CHUNK):
                tr.eval_noise(batches[i:j], K, tr.noise_len)
            host.append((time.perf_counter() - t0) * 1e3)
        lines.append("    host noise draws alone (in both calls): median %.3f ms" % statistics.median(host))
        lines.append("    metrics test()     %s" % np.array2string(np.asarray(last["test"]), precision=7))
        lines.append("    metrics evaluate() %s" % np.array2string(np.asarray(last["evaluate"]), precision=7))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
