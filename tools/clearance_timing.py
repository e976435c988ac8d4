#!/usr/bin/env python
"""Timing of the scene-clearance term of the generator loss (SocialWaysTrainer.set_clearance_loss()) on one MI355X, on the
packed batches of tools/ragged_timing.py (c) - the rows and futures of the first evaluation chunk of the three shapes of
tools/_timing.py as ONE packed batch: 816, 8 and 768 agents - and by its method: host clock around a step that ends in the
host read of its sums, warm-up (the graph is captured on the third call), then timed calls of every side, ALTERNATING, same z
and label noise for every call; median and min / max.

  (a) the graph-captured training step: (i) the PARENT commit's plain step and (ii) its use_l2_loss=True step - a tree of the
      parent with its library built, --parent-tree -, (iii) this build's plain step (the term off: the launches of (i)),
      (iv) this build's use_l2_loss=True step, (v) the step with the clearance term on (dist 0.2, weight 1).  (ii), (iv) and (v)
      run the same un-fused route - the generator-phase D pass as a launch of its own - plus one small launch on
      d/d(pred_hat) each, so (v) is expected beside (ii), and (iii) inside (i).  Two trees cannot share a process: every side
      runs in child processes of its tree, --rounds of each, one at a time and alternating, --repeats / --rounds timed calls
      per child after its warm-up.  A child holds three trainers and alternates them; the parent's third is a second
      use_l2_loss trainer (timed, not reported), so that the children of both trees do the same work around a timed call.
  (b) sw_clearance_grad alone on the step's own shapes (pos and dpos 4 floats wide, start = the last observed frame read in
      place, loss and count written): us per launch, `--launches` launches back to back and a synchronisation per timed call.

    python tools/clearance_timing.py --parent-tree ab_old [--rounds 3] [--repeats 9] [--out profiles/clearance_loss_timing.txt]
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
SIDES = ("plain", "l2", "clear")     # this build's sides of (a)
PARENT_SIDES = ("plain", "l2", "l2 again")


def child(a):
    """One tree's sides of (a) on the three packed batches -> one JSON line {shape: {side: [ms per step]}}."""
    sw = T.load("clearance_timing.py", a.tree)
    out = {}
    for name, obsv, pred, sb, _ in packed_batches(T.trainer()):
        z = torch.rand(obsv.shape[0], 32, device=obsv.device, generator=torch.Generator(device="cuda").manual_seed(11))

        def side(k):
            torch.manual_seed(0)
            tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0", use_l2_loss=k.startswith("l2"))
            if k == "clear":
                tr.set_clearance_loss(DIST, WEIGHT)

            def call():
                return float(tr.step(obsv, pred, sb, 0.04, 0.93, z, 1.0).sum())      # the host synchronisation
            return call
        ms, _ = T.alternate({k: side(k) for k in a.sides.split(",")}, max(a.warmup, 4), a.repeats)
        out[name] = ms
    print("TIMING_CHILD " + json.dumps(out))


def kernel_alone(obsv, pred, sb, launches):
    ops = T.sw.ops
    B, Tp = pred.shape[0], pred.shape[1]
    scenes = ops.SceneIndex.get(sb, B, obsv.device)
    pos = torch.zeros(B, Tp, 4, device=obsv.device)
    pos[..., :2] = pred
    dpos, loss = torch.zeros_like(pos), torch.zeros(B, device=obsv.device)
    count = torch.zeros(B, dtype=torch.int32, device=obsv.device)

    def call():
        for _ in range(launches):
            ops.clearance_grad(pos, obsv[:, -1], scenes, DIST, 1.0 / (B * Tp), dpos, loss, count)
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
    T.load("clearance_timing.py")
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
    cols = (("parent plain", "(i) parent, plain"), ("parent l2", "(ii) parent, use_l2_loss"), ("plain", "(iii) plain, term off"),
            ("l2", "(iv) use_l2_loss"), ("clear", "(v) clearance term on"))
    lines = ["(a) the graph-captured training step on one packed batch: the parent commit's build and this build; host clock around "
             "calls that end in a host read, ms per step; %d child processes of each tree, alternating, %d timed calls per child after "
             "%d warm-up calls; clearance term: dist %.1f, weight %.1f; %s"
             % (a.rounds, a.repeats // a.rounds, max(a.warmup, 4), DIST, WEIGHT, torch.cuda.get_device_name(0)),
             "%-88s %6s " % ("shape", "B") + " ".join("%28s" % c for _, c in cols) + "  (v) / (ii)  (iii) inside (i)"]
    tr = T.trainer()
    batches = list(packed_batches(tr))
    for name, obsv, pred, sb, _ in batches:
        r = res[name]
        lines.append("%-88s %6d " % (name, obsv.shape[0]) + " ".join("%28s" % cell(r[k]) for k, _ in cols)
                     + "  %10.3f  %s" % (statistics.median(r["clear"]) / statistics.median(r["parent l2"]),
                                         T.inside(r["parent plain"], r["plain"])))
    lines += ["", "(b) sw_clearance_grad alone on the same batches (d0 %.1f in the units of the tracks); us per launch, %d launches per "
              "timed call; %d repeats after %d warm-up calls" % (DIST, a.launches, a.repeats, a.warmup),
              "%-88s %6s %7s %30s %s" % ("shape", "B", "scenes", "median [min, max]", "(partner, segment)s closer than d0")]
    for name, obsv, pred, sb, _ in batches:
        ms, last = T.alternate({"k": kernel_alone(obsv, pred, sb, a.launches)}, a.warmup, a.repeats)
        lines.append("%-88s %6d %7d %30s %d" % (name, obsv.shape[0], len(sb), cell([1e3 * t / a.launches for t in ms["k"]]), last["k"]))
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
