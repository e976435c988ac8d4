#!/usr/bin/env python
"""Timing of ragged futures (pred_len) on one MI355X, on the first evaluation chunk of the three shapes of tools/_timing.py
(816 / 8 / 768 agents at K = 20) and by the method of tools/ragged_timing.py: host clock around calls that end in a host
synchronisation, warm-up, then `--repeats` timed calls of each side, ALTERNATING; median and min / max.

  (a) the sampling launch with its encoder and social block (ops.gen_sample, errors only, as evaluate() calls it): dense,
      pred_len all 12, pred_len uniform in 1 .. 12.  The length-aware kernel runs the same Tp steps, so the expectation is
      about equal.  The results at full length are compared bit for bit first.
  (b) the clearance launch on the K draws of the same chunk (ops.scene_clearance, start = the last observed position): dense,
      lens all 12, lens uniform in 1 .. 12.  One timed call = `--launches` launches back to back and a synchronisation; ms per
      launch.  Same comparison first.
  (c) the control: evaluate() on a dataset WITHOUT pred_len at this commit and at the parent commit (--parent-tree: a tree of
      the parent with its library built).  The kernels are the same; the spread of this pair is what (a) and (b) are read
      against.  Two trees cannot share a process: tools/_timing.py's child processes, alternating.

    python tools/ragged_next_timing.py [--repeats 9] [--parent-tree ab_old] [--out profiles/ragged_next_timing.txt]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import PER_LAUNCH, cell  # noqa: E402

K = 20


def sample_sides(tr, obsv, pred, sb, noise, full, mixed):
    ops, G = T.sw.ops, tr.G
    scenes = ops.SceneIndex.get(sb, obsv.shape[0], obsv.device)

    def side(pred_len):
        def call():
            _, red = ops.gen_sample(G.encoder.packed(), G.feature_embedder.packed(), G.attention.packed(), G.decoder.packed(), obsv,
                                    noise, scenes, tr.n_next, G.use_social, K, gt=pred, inv_ss=1.0, want_pred=False, pred_len=pred_len)
            return float(red[0].double().sum()), red[2]      # the host synchronisation
        return call
    sides = {"dense": side(None), "full": side(full), "mixed": side(mixed)}
    assert torch.equal(sides["dense"]()[1], sides["full"]()[1])
    return sides


def clearance_sides(tr, obsv, sb, noise, full, mixed, launches):
    ops = T.sw.ops
    B = obsv.shape[0]
    scenes = ops.SceneIndex.get(sb, B, obsv.device)
    ph = tr.G.sample(obsv, K, tr.n_next, sb, noise.view(K, B, 32)).view(K * B, tr.n_next, 4)

    def side(lens):
        def call():
            for _ in range(launches):
                out = ops.scene_clearance(ph, obsv[:, -1], scenes, K, 1.0, lens=lens)
            torch.cuda.synchronize()
            return out
        return call
    sides = {"dense": side(None), "full": side(full), "mixed": side(mixed)}
    assert torch.equal(sides["dense"](), sides["full"]())
    return sides


def main():
    def more(ap):
        ap.add_argument("--launches", type=int, default=20, help="(b): launches per timed call")
        T.parent_tree_args(ap)
    a = T.parse(__doc__, 9, 9, more)
    T.load("ragged_next_timing.py")
    tr = T.trainer()
    head = "%-88s %6s %28s %28s %8s %28s %8s %s"
    la = ["(a) ops.gen_sample (encoder, social block, sampling launch, best-of-K reduction; errors only) at K = %d: dense, pred_len all "
          "12, pred_len uniform in 1 .. 12; host clock around the call, ms; %d alternating repeats after %d warm-up calls of each; %s"
          % (K, a.repeats, a.warmup, torch.cuda.get_device_name(0)),
          head % ("shape", "B", "dense median [min, max]", "pred_len all 12", "/dense", "pred_len uniform 1 .. 12", "/dense",
                  "each median inside the dense range")]
    lb = ["", "(b) ops.scene_clearance on the K = %d draws of the same chunk, start = the last observed position: dense, lens all 12, "
          "lens uniform in 1 .. 12; ms per launch, %d launches per timed call; %d alternating repeats after %d warm-up calls"
          % (K, a.launches, a.repeats, a.warmup),
          head % ("shape", "B", "dense median [min, max]", "lens all 12", "/dense", "lens uniform 1 .. 12", "/dense",
                  "each median inside the dense range")]
    for name, n_scenes, agents, _, just_one in T.SHAPES:
        _, obsv, pred, sb = next(T.host_chunks(tr, T.held_out_set(n_scenes, agents), K, just_one))
        obsv, pred = obsv.contiguous(), pred.contiguous()
        B = obsv.shape[0]
        gen = torch.Generator(device="cuda").manual_seed(7)
        noise = torch.rand(K * B, 32, device="cuda", generator=gen)
        mixed = torch.randint(1, tr.n_next + 1, (B,), device="cuda", generator=gen, dtype=torch.int32)
        full = torch.full((B,), tr.n_next, dtype=torch.int32, device="cuda")
        ms, _ = T.alternate(sample_sides(tr, obsv, pred, sb, noise, full, mixed), a.warmup, a.repeats)
        med = {k: statistics.median(v) for k, v in ms.items()}
        la.append(head % (name, "%d" % B, cell(ms["dense"]), cell(ms["full"]), "%.3f" % (med["full"] / med["dense"]), cell(ms["mixed"]),
                          "%.3f" % (med["mixed"] / med["dense"]), (T.inside(ms["dense"], ms["full"]), T.inside(ms["dense"], ms["mixed"]))))
        ms, _ = T.alternate(clearance_sides(tr, obsv, sb, noise, full, mixed, a.launches), a.warmup, a.repeats)
        per = {k: [t / a.launches for t in v] for k, v in ms.items()}
        med = {k: statistics.median(v) for k, v in per.items()}
        lb.append(head % (name, "%d" % B, cell(per["dense"], fmt=PER_LAUNCH), cell(per["full"], fmt=PER_LAUNCH),
                          "%.3f" % (med["full"] / med["dense"]), cell(per["mixed"], fmt=PER_LAUNCH), "%.3f" % (med["mixed"] / med["dense"]),
                          (T.inside(per["dense"], per["full"]), T.inside(per["dense"], per["mixed"]))))
    lc = ["", "(c) control: evaluate() on a dataset without pred_len, parent build vs this build (the same kernels)"]
    if a.parent_tree:
        per_child = max(5, a.repeats // a.rounds)      # tools/_timing.py's child takes no fewer than 5
        res = T.across_builds(a.parent_tree, a.rounds, per_child, a.warmup)
        lc[-1] += ": %d alternating child processes of each, %d timed calls per child after %d warm-up calls; ms" % (
            a.rounds, per_child, a.warmup)
        lc.append("%-88s %28s %28s %8s %-8s %s" % ("shape", "parent median [min, max]", "this median [min, max]", "ratio", "inside", "equal"))
        for (shape, _, _), r in res.items():
            p, t = r["parent"]["ms"], r["this"]["ms"]
            lc.append("%-88s %28s %28s %8.3f %-8s %s" % (shape, cell(p), cell(t), statistics.median(t) / statistics.median(p), T.inside(p, t),
                                                       T.equal(r)))
    else:
        lc.append("not run: no --parent-tree given")
    T.write_out(la + lb + lc, a.out)


if __name__ == "__main__":
    main()
