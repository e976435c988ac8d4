#!/usr/bin/env python
"""Timing of the grid-indexed wall kernels (socialways_amd.WallGrid: sw_wall_grad_grid, sw_path_walls_grid) against the flat
ones on one MI355X, on the packed batches of tools/wall_loss_timing.py (816, 8 and 768 agents, Tp 12) and by its method: host
clock, warm-up, then timed calls of every side, ALTERNATING; median and min / max; a synchronisation around every timed call.

The maps: M = 16, 128, 1024 random segments inside the bounding box of the batch's futures (wall_loss_timing.box_walls), and the
TRACED map - data.synth_occupancy(seed 0), 480 x 640 with 40 rectangles and 30 discs, through trace_occupancy(), its pixels laid
over the same bounding box - as it is (2 274 runs from 7 106 unit edges) and with every run cut into four (the same geometry from four times
as many walls).  dist 0.2 m, reach 0.25 m: WORLD units - the tracks are normalised into the unit square (SceneDataset), so
the launches see dist * ss and reach * ss; at tools/wall_loss_timing.py's dist of 0.2 in the units of the TRACKS, a fifth of the
whole scene, every wall is within reach of every path and a grid has nothing to leave out.

  (a) the graph-captured training step: (i) the PARENT commit's plain step, (ii) the same again - the control -, a tree of the
      parent with its library built, --parent-tree -, (iii) this build's plain step (the launches of (i)), (iv) the step with the
      flat wall term at M = 1024, (v) with the traced map under a grid (default cell).  Every side in child processes of its
      tree, --rounds of each, one at a time and alternating.
  (b) the gradient launch alone on the step's own shapes (pos and dpos 4 floats wide, start read in place, loss and count
      written): flat against grid at M = 16, 128, 1024, the grid at cell = reach, 2 reach, 4 reach; the grid alone on the two
      traced maps.  us per launch, `--launches` launches back to back and a synchronisation per timed call.
  (c) path_walls on K * B draws of the same chunks (the futures plus N(0, (0.3 m)^2) noise per draw): the same sides.

    python tools/wall_grid_timing.py --parent-tree ab_old [--rounds 3] [--repeats 9] [--out profiles/wall_grid_timing.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import cell  # noqa: E402
from wall_loss_timing import box_walls  # noqa: E402

DIST, WEIGHT, REACH = 0.2, 1.0, 0.25         # world units
CELLS = (1.0, 2.0, 4.0)                      # in units of reach
SIDES = ("plain", "walls1024", "grid")       # this build's sides of (a)
PARENT_SIDES = ("plain", "plain again")


def traced_walls(pred, pieces=1):
    """The traced synthetic image laid over the bounding box of the futures -> (M, 2, 2) float32 tensor on the device of pred;
    pieces: every run cut into that many equal parts."""
    from socialways_amd.data import synth_occupancy
    occ = synth_occupancy(0)
    seg = T.sw.trace_occupancy(occ).astype(np.float64)
    if pieces > 1:
        t = np.arange(pieces + 1) / pieces
        a, b = seg[:, None, :2], seg[:, None, 2:]
        pts = a + t[None, :, None] * (b - a)                                   # (M, pieces + 1, 2)
        seg = np.concatenate([pts[:, :-1], pts[:, 1:]], 2).reshape(-1, 4)
    xy = pred[..., :2].reshape(-1, 2).double().cpu().numpy()
    lo, hi = xy.min(0), xy.max(0)
    k = (hi - lo) / np.array([occ.shape[1], occ.shape[0]])
    seg = seg.reshape(-1, 2, 2) * k + lo
    return torch.from_numpy(seg.astype(np.float32)).to(pred.device)


def packed_batches(tr):
    """ragged_timing.packed_batches with the scale of the dataset: per shape (name, obsv, pred, sb, ss)."""
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        _, obsv, pred, sb = next(T.host_chunks(tr, data, K, just_one))
        yield name, obsv.contiguous(), pred.contiguous(), sb, float(data.ss)


def child(a):
    """One tree's sides of (a) on the three packed batches -> one JSON line {shape: {side: [ms per step]}}."""
    sw = T.load("wall_grid_timing.py", a.tree)
    out = {}
    for name, obsv, pred, sb, ss in packed_batches(T.trainer()):
        z = torch.rand(obsv.shape[0], 32, device=obsv.device, generator=torch.Generator(device="cuda").manual_seed(11))

        def side(k):
            torch.manual_seed(0)
            tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0")
            if k == "walls1024":
                tr.set_wall_loss(box_walls(pred, 1024), DIST, WEIGHT)
            if k == "grid":
                tr.set_wall_loss(sw.WallGrid(traced_walls(pred), REACH * ss, device="cuda:0"), DIST, WEIGHT)

            def call():
                return float(tr.step(obsv, pred, sb, 0.04, 0.93, z, ss).sum())       # the host synchronisation
            return call
        ms, _ = T.alternate({k: side(k) for k in a.sides.split(",")}, max(a.warmup, 4), a.repeats)
        out[name] = ms
    print("TIMING_CHILD " + json.dumps(out))


def grad_alone(obsv, pred, walls, ss, launches):
    ops = T.sw.ops
    B, Tp = pred.shape[0], pred.shape[1]
    pos = torch.zeros(B, Tp, 4, device=obsv.device)
    pos[..., :2] = pred
    dpos, loss = torch.zeros_like(pos), torch.zeros(B, device=obsv.device)
    count = torch.zeros(B, dtype=torch.int32, device=obsv.device)

    def call():
        for _ in range(launches):
            ops.wall_grad(pos, obsv[:, -1], 1, walls, DIST * ss, 1.0 / (B * Tp), dpos, loss, count)
        torch.cuda.synchronize()
        return int(count.sum())
    return call


def draws_alone(obsv, draws, K, walls, ss, launches):
    ops = T.sw.ops

    def call():
        for _ in range(launches):
            out = ops.path_walls(draws, obsv[:, -1], K, walls, DIST, 1.0 / ss)
        torch.cuda.synchronize()
        return int(out[2].sum())
    return call


def tables(title, what, batches, make, a, launches):
    """One table of (b) or (c): make(shape index, walls) -> the timed call; flat and the three grids per M, then the two traced
    maps under the three grids."""
    W = T.sw.WallGrid
    lines = ["", title, "%-88s %6s %-22s %6s %9s %30s %s" % ("shape", "B", "map", "M", "side", "median [min, max]", what)]
    for i, (name, obsv, pred, sb, ss) in enumerate(batches):
        maps = [("random, M = %d" % M, box_walls(pred, M), True) for M in (16, 128, 1024)]
        maps += [("traced", traced_walls(pred), False), ("traced, runs in four", traced_walls(pred, 4), False)]
        for label, walls, flat in maps:
            sides = {"flat": make(i, walls)} if flat else {}
            grids = {}
            for c in CELLS:
                grids[c] = W(walls, REACH * ss, c * REACH * ss, device="cuda:0")
                sides["grid %gr" % c] = make(i, grids[c])
            us, last = T.alternate(sides, a.warmup, a.repeats)
            assert len(set(last.values())) == 1, (label, last)              # every side counts the same pairs
            print("%s | %s done" % (name[:12], label), file=sys.stderr, flush=True)
            for k in sides:
                g = grids.get(float(k[5:-1])) if k != "flat" else None
                lines.append("%-88s %6d %-22s %6d %9s %30s %d%s" % (
                    name, obsv.shape[0], label, walls.shape[0], k, cell([1e3 * t / launches for t in us[k]]), last[k],
                    "" if g is None else "   (%d x %d cells, %d list entries)" % (g.nx, g.ny, g.L)))
    return lines


def main():
    def more(ap):
        ap.add_argument("--launches", type=int, default=50, help="(b), (c): launches per timed call")
        T.parent_tree_args(ap)
        ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
        ap.add_argument("--tree", default=T.HERE, help=argparse.SUPPRESS)
        ap.add_argument("--sides", default="plain", help=argparse.SUPPRESS)
    a = T.parse(__doc__, 9, 1 if "--child" in sys.argv else 9, more)
    if a.child:
        return child(a)
    if not a.parent_tree or a.rounds < 1 or a.repeats % a.rounds:
        sys.exit("needs --parent-tree (a tree of the parent commit with its library built) and --repeats a multiple of --rounds")
    T.load("wall_grid_timing.py")
    res = {}
    for _ in range(a.rounds):      # one child at a time, alternating between the trees
        for tree, sides in ((os.path.abspath(a.parent_tree), ",".join(PARENT_SIDES)), (T.HERE, ",".join(SIDES))):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--sides", sides, "--repeats",
                                str(a.repeats // a.rounds), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.exit("child on %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
            got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("TIMING_CHILD ")][-1][13:])
            print("(a) child of %s done" % tree, file=sys.stderr, flush=True)
            for shape, ms in got.items():
                for k, v in ms.items():
                    res.setdefault(shape, {}).setdefault(("parent " if tree != T.HERE else "") + k, []).extend(v)
    cols = (("parent plain", "(i) parent, plain"), ("parent plain again", "(ii) parent, plain again"), ("plain", "(iii) plain, term off"),
            ("walls1024", "(iv) flat term, M = 1024"), ("grid", "(v) traced map, grid"))
    lines = ["(a) the graph-captured training step on one packed batch: the parent commit's build and this build; host clock around "
             "calls that end in a host read, ms per step; %d child processes of each tree, alternating, %d timed calls per child after "
             "%d warm-up calls; wall term: dist %.2f m, weight %.1f, reach %.2f m, cell %g reach; %s"
             % (a.rounds, a.repeats // a.rounds, max(a.warmup, 4), DIST, WEIGHT, REACH, T.sw.WallGrid.DEFAULT_CELL,
                torch.cuda.get_device_name(0)),
             "%-88s %6s " % ("shape", "B") + " ".join("%28s" % c for _, c in cols) + "  (v) / (iv)  (v) / (iii)  (iii) inside (i) + (ii)"]
    tr = T.trainer()
    batches = list(packed_batches(tr))
    for name, obsv, pred, sb, _ in batches:
        r = res[name]
        lines.append("%-88s %6d " % (name, obsv.shape[0]) + " ".join("%28s" % cell(r[k]) for k, _ in cols)
                     + "  %10.3f  %11.3f  %s" % (statistics.median(r["grid"]) / statistics.median(r["walls1024"]),
                                                 statistics.median(r["grid"]) / statistics.median(r["plain"]),
                                                 T.inside(r["parent plain"] + r["parent plain again"], r["plain"])))
    few = max(1, a.launches // 5)                                             # (c): K times as many paths per launch
    head = "us per launch, %d launches per timed call; " + "%d repeats after %d warm-up calls; dist %.2f m, reach %.2f m, cell in units " \
           "of reach (r)" % (a.repeats, a.warmup, DIST, REACH)
    lines += tables("(b) the gradient launch alone on the same batches, sw_wall_grad against sw_wall_grad_grid; " + head % a.launches,
                    "(segment, wall)s closer than dw", batches,
                    lambda i, walls: grad_alone(batches[i][1], batches[i][2], walls, batches[i][4], a.launches), a, a.launches)
    gen = torch.Generator(device="cuda").manual_seed(5)
    draws = []
    for (name, n_scenes, agents, K, just_one), (_, obsv, pred, sb, _) in zip(T.SHAPES, batches):
        draws.append((K, (pred[None, ..., :2] + 0.3 * batches[len(draws)][4] * torch.randn(K, *pred[..., :2].shape, device=pred.device, generator=gen)).contiguous()))
    lines += tables("(c) path_walls on the K * B draws of the same chunks (K = %s), sw_path_walls against sw_path_walls_grid; "
                    % ", ".join(str(k) for k, _ in draws) + head % few, "(segment, wall)s closer than dist", batches,
                    lambda i, walls: draws_alone(batches[i][1], draws[i][1], draws[i][0], walls, batches[i][4], few), a, few)
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
