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
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402


def main():
    a = T.parse(__doc__, 7, 5)
    T.load("sample_timing.py")
    tr = T.trainer()
    lines = ["test() vs evaluate(): host clock around the call (both return host floats), ms; %d alternating repeats after %d "
             "warm-up calls of each; %s" % (a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "%-88s %28s %28s %8s" % ("shape", "test() median [min, max]", "evaluate() median [min, max]", "ratio")]
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        ms, last = T.alternate({k: (lambda k=k: T.CALLS[k](tr, data, K, just_one)) for k in ("test", "evaluate")}, a.warmup, a.repeats)
        lines.append("%-88s %28s %28s %8.3f" % (name, T.cell(ms["test"]), T.cell(ms["evaluate"]),
                                                statistics.median(ms["evaluate"]) / statistics.median(ms["test"])))
        host = []
        for _ in range(a.repeats):        # the part both calls share: the reference's host noise stream (train.py:584)
            t0 = time.perf_counter()
            for scenes, _, _, _ in T.host_chunks(tr, data, K, just_one):
                tr.eval_noise(scenes, K, tr.noise_len)
            host.append((time.perf_counter() - t0) * 1e3)
        lines.append("    host noise draws alone (in both calls): median %.3f ms" % statistics.median(host))
        lines.append("    metrics test()     %s" % np.array2string(np.asarray(last["test"]), precision=7))
        lines.append("    metrics evaluate() %s" % np.array2string(np.asarray(last["evaluate"]), precision=7))
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
