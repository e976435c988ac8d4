#!/usr/bin/env python
"""Timing of the sw_scene_compose launch on one MI355X, by the method of tools/nms_timing.py (b): host clock around calls
that end in a host synchronisation, warm-up, then `--repeats` timed calls of each side, ALTERNATING, same seed for every call;
median and min / max.  One timed call = `--launches` calls of the wrapper back to back and a synchronisation; ms each.

The draws and scores are those of the first chunk evaluate() forms of each of the three shapes of tools/_timing.py, all at
K = 20: 816 agents in 102 scenes of 8, one scene of 8, 768 agents in 12 scenes of 64.  Next to the compose launch, on the
same chunk: Generator.sample() (the encoder, the social block and the sampling launch that produced the draws),
ops.scene_clearance() (sw_scene_clearance over all K joint draws) and ops.sample_rank() (sw_sample_rank, top 1).  There is
no earlier implementation to compare with, so nothing here passes or fails; what the composition did to the chunk is
printed next to the times.

    python tools/compose_timing.py [--repeats 9] [--out profiles/compose_timing.txt]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import COLL, PER_LAUNCH, cell, first_chunk  # noqa: E402

K, SWEEPS = 20, 8
SIDES = ("compose", "sample", "clearance", "rank")


def launch_set(tr, data, just_one, launches):
    ops = T.sw.ops
    obsv, sb = first_chunk(tr, data, K, just_one)
    B = obsv.shape[0]
    torch.manual_seed(5)
    noise = torch.rand(K, B, tr.noise_len, device=obsv.device)
    ph = tr.G.sample(obsv, K, tr.n_next, sb, noise)
    score, _ = tr.D.score_samples(obsv, ph)
    scenes = ops.SceneIndex.get(sb, B, obsv.device)
    inv_ss = 1.0 / float(data.ss)
    start = obsv[:, -1]
    per_scene = ops.scene_compose(ph, start, score, scenes, K, COLL, inv_ss, SWEEPS)[3].long().sum(0).tolist()

    def many(fn):
        def run():
            for _ in range(launches):
                out = fn()
            torch.cuda.synchronize()
            return out
        return run
    calls = {"compose": many(lambda: ops.scene_compose(ph, start, score, scenes, K, COLL, inv_ss, SWEEPS)),
             "sample": many(lambda: tr.G.sample(obsv, K, tr.n_next, sb, noise)),
             "clearance": many(lambda: ops.scene_clearance(ph, start, scenes, K, inv_ss)),
             "rank": many(lambda: ops.sample_rank(score, K, 1))}
    return calls, B, scenes.S, per_scene


def main():
    a = T.parse(__doc__, 9, 9, lambda ap: ap.add_argument("--launches", type=int, default=20, help="calls per timed call"))
    T.load("compose_timing.py")
    tr = T.trainer()
    lines = ["one call of each wrapper on the first evaluation chunk of each shape, K = %d; host clock, ms per call, %d calls per "
             "timed call; %d alternating repeats after %d warm-up calls; coll_dist %.1f, sweeps %d; %s"
             % (K, a.launches, a.repeats, a.warmup, COLL, SWEEPS, torch.cuda.get_device_name(0)),
             "%-60s %6s %6s %30s %30s %30s %30s   %s" % ("shape (at K = 20)", "B", "scenes", "scene_compose median [min, max]",
                                                        "Generator.sample", "scene_clearance", "sample_rank",
                                                        "conflicting pairs top-1 -> composed, agents moved, sweeps")]
    for name, n_scenes, agents, _, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        calls, B, S, ps = launch_set(tr, data, just_one, a.launches)
        ms, _ = T.alternate(calls, a.warmup, a.repeats)
        per = {k: [x / a.launches for x in ms[k]] for k in SIDES}
        lines.append("%-60s %6d %6d %30s %30s %30s %30s   %d -> %d, %d, %d" % (
            name.split(":")[0] + ": first chunk", B, S, cell(per["compose"], fmt=PER_LAUNCH), cell(per["sample"], fmt=PER_LAUNCH),
            cell(per["clearance"], fmt=PER_LAUNCH), cell(per["rank"], fmt=PER_LAUNCH), ps[0], ps[1], ps[2], ps[3]))
    lines.append("(every column is the Python wrapper: its output allocations are inside the time; the last column sums per_scene "
                 "over the chunk's scenes, sweeps = the sum of the sweeps that changed something)")
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
