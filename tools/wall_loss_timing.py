#!/usr/bin/env python
"""Timing of the wall term of the generator loss (SocialWaysTrainer.set_wall_loss()) on one MI355X, on the packed batches of
tools/ragged_timing.py (c) - the rows and futures of the first evaluation chunk of the three shapes of tools/_timing.py as ONE
packed batch: 816, 8 and 768 agents - and by the method of tools/clearance_timing.py: host clock around a step that ends in the
host read of its sums, warm-up (the graph is captured on the third call), then timed calls of every side, ALTERNATING, same z
and label noise for every call; median and min / max.

  (a) the graph-captured training step: (i) the PARENT commit's plain step, (ii) the same again - the control: what two
      measurements of one build differ by - and (iii) its use_l2_loss=True step - a tree of the parent with its library built,
      --parent-tree -, (iv) this build's plain step (the term off: the launches of (i)), (v) the step with the wall term on and
      M = 16 walls, (vi) with M = 128 (dist 0.2, weight 1; the walls random segments inside the bounding box of the batch's
      futures).  (iii), (v) and (vi) run the same un-fused route - the generator-phase D pass as a launch of its own - plus one
      small launch on d/d(pred_hat) each; (iv) is expected inside (i).  Two trees cannot share a process: every side runs in
      child processes of its tree, --rounds of each, one at a time and alternating, --repeats / --rounds timed calls per child
      after its warm-up; a child holds three trainers and alternates them.
  (b) sw_wall_grad alone on the step's own shapes (pos and dpos 4 floats wide, start = the last observed frame read in place,
      loss and count written), M = 16, 128 and 1024: us per launch, `--launches` launches back to back and a synchronisation
      per timed call.

    python tools/wall_loss_timing.py --parent-tree ab_old [--rounds 3] [--repeats 9] [--out profiles/wall_loss_timing.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import cell  # noqa: E402
from ragged_timing import packed_batches  # noqa: E402

DIST, WEIGHT = 0.2, 1.0
SIDES = ("plain", "walls16", "walls128")     # this build's sides of (a)
PARENT_SIDES = ("plain", "plain again", "l2")


def box_walls(pred, M, seed=7):
    """M random segments inside the bounding box of the futures, up to a fifth of its size long, every fourth a post."""
    g = torch.Generator().manual_seed(seed)
    xy = pred[..., :2].reshape(-1, 2).float().cpu()
    lo, hi = xy.min(0).values, xy.max(0).values
    w0 = lo + (hi - lo) * torch.rand(M, 2, generator=g)
    w1 = w0 + 0.2 * (hi - lo) * (torch.rand(M, 2, generator=g) - 0.5)
    w1[3::4] = w0[3::4]
    return torch.stack([w0, w1], 1).to(pred.device)


def child(a):
    """One tree's sides of (a) on the three packed batches -> one JSON line {shape: {side: [ms per step]}}."""
    sw = T.load("wall_loss_timing.py", a.tree)
    out = {}
    for name, obsv, pred, sb, _ in packed_batches(T.trainer()):
        z = torch.rand(obsv.shape[0], 32, device=obsv.device, generator=torch.Generator(device="cuda").manual_seed(11))

        def side(k):
            torch.manual_seed(0)
            tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0", use_l2_loss=(k == "l2"))
            if k.startswith("walls"):
                tr.set_wall_loss(box_walls(pred, int(k[5:])), DIST, WEIGHT)

            def call():
                return float(tr.step(obsv, pred, sb, 0.04, 0.93, z, 1.0).sum())      # the host synchronisation
            return call
        ms, _ = T.alternate({k: side(k) for k in a.sides.split(",")}, max(a.warmup, 4), a.repeats)
        out[name] = ms
    print("TIMING_CHILD " + json.dumps(out))


def kernel_alone(obsv, pred, M, launches):
    ops = T.sw.ops
    B, Tp = pred.shape[0], pred.shape[1]
    pos = torch.zeros(B, Tp, 4, device=obsv.device)
    pos[..., :2] = pred
    walls = box_walls(pred, M)
    dpos, loss = torch.zeros_like(pos), torch.zeros(B, device=obsv.device)
    count = torch.zeros(B, dtype=torch.int32, device=obsv.device)

    def call():
        for _ in range(launches):
            ops.wall_grad(pos, obsv[:, -1], 1, walls, DIST, 1.0 / (B * Tp), dpos, loss, count)
        torch.cuda.synchronize()
        return int(count.sum())
    return call


def main():
    def more(ap):
        ap.add_argument("--launches", type=int, default=50, help="(b): launches per timed call")
        T.parent_tree_args(ap)
        ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
        ap.add_argument("--tree", default=T.HERE, help=argparse.SUPPRESS)
        ap.add_argument("--sides", default="plain", help=argparse.SUPPRESS)
    a = T.parse(__doc__, 9, 1 if "--child" in sys.argv else 9, more)
    if a.child:
        return child(a)
    if not a.parent_tree or a.rounds < 1 or a.repeats % a.rounds:
        sys.exit("needs --parent-tree (a tree of the parent commit with its library built) and --repeats a multiple of --rounds")
    T.load("wall_loss_timing.py")
    res = {}
    for _ in range(a.rounds):      # one child at a time, alternating between the trees
        for tree, sides in ((os.path.abspath(a.parent_tree), ",".join(PARENT_SIDES)), (T.HERE, ",".join(SIDES))):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--sides", sides, "--repeats",
                                str(a.repeats // a.rounds), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.exit("child on %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
            got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("TIMING_CHILD ")][-1][13:])
            for shape, ms in got.items():
                for k, v in ms.items():
                    res.setdefault(shape, {}).setdefault(("parent " if tree != T.HERE else "") + k, []).extend(v)
    cols = (("parent plain", "(i) parent, plain"), ("parent plain again", "(ii) parent, plain again"),
            ("parent l2", "(iii) parent, use_l2_loss"), ("plain", "(iv) plain, term off"), ("walls16", "(v) wall term, M = 16"),
            ("walls128", "(vi) wall term, M = 128"))
    lines = ["(a) the graph-captured training step on one packed batch: the parent commit's build and this build; host clock around "
             "calls that end in a host read, ms per step; %d child processes of each tree, alternating, %d timed calls per child after "
             "%d warm-up calls; wall term: dist %.1f, weight %.1f; %s"
             % (a.rounds, a.repeats // a.rounds, max(a.warmup, 4), DIST, WEIGHT, torch.cuda.get_device_name(0)),
             "%-88s %6s " % ("shape", "B") + " ".join("%28s" % c for _, c in cols) + "  (v) / (iii)  (vi) / (iii)  (iv) inside (i) + (ii)"]
    tr = T.trainer()
    batches = list(packed_batches(tr))
    for name, obsv, pred, sb, _ in batches:
        r = res[name]
        l2 = statistics.median(r["parent l2"])
        lines.append("%-88s %6d " % (name, obsv.shape[0]) + " ".join("%28s" % cell(r[k]) for k, _ in cols)
                     + "  %11.3f  %12.3f  %s" % (statistics.median(r["walls16"]) / l2, statistics.median(r["walls128"]) / l2,
                                                 T.inside(r["parent plain"] + r["parent plain again"], r["plain"])))
    lines += ["", "(b) sw_wall_grad alone on the same batches (dw %.1f in the units of the tracks); us per launch, %d launches per "
              "timed call; %d repeats after %d warm-up calls" % (DIST, a.launches, a.repeats, a.warmup),
              "%-88s %6s %6s %30s %s" % ("shape", "B", "M", "median [min, max]", "(segment, wall)s closer than dw")]
    for name, obsv, pred, sb, _ in batches:
        for M in (16, 128, 1024):
            ms, last = T.alternate({"k": kernel_alone(obsv, pred, M, a.launches)}, a.warmup, a.repeats)
            lines.append("%-88s %6d %6d %30s %d" % (name, obsv.shape[0], M, cell([1e3 * t / a.launches for t in ms["k"]]), last["k"]))
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
