#!/usr/bin/env python
"""What the K-sample timing tools share (sample_timing, scene_timing, rank_timing, nms_timing, noise_timing): the three
shapes, the held-out set, the timed call (host clock around a call that ends in a host synchronisation, same seeds for every
call), the alternation of the sides, the table cell, evaluate()'s chunks re-derived from its public pieces, the command line
and the write-out - and the A/B of two BUILDS of the package: two trees cannot share a process, so each side runs in child
processes of its own, one at a time and alternating, and this file is the child.

Run by itself it is that A/B over the whole evaluation family: test(), evaluate(),
evaluate_scenes(), evaluate_ranked(), evaluate_diverse() (per agent and per scene), evaluate_history(), evaluate_horizon(),
evaluate_composed(), evaluate_risk(), evaluate_refine() (without and with walls) and evaluate_walls() on the host noise stream
and on a DeviceNoise(2019), what every call returns (repr, equal or not) and its time in both builds (each median inside the
other's range or not).

    python tools/_timing.py --parent-tree ab_old [--rounds 3] [--repeats 7] [--out profiles/eval_refactor_ab.txt]
"""
import argparse
import ast
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sw = None      # socialways_amd of the tree given to load()

# name, held-out scenes, agents per scene, K, just_one
SHAPES = (("throughput: 256 held-out scenes x 8 agents, K = 20, full set", 256, 8, 20, False),
          ("latency: same set, K = 128, first scene only (the driver's call every five epochs)", 256, 8, 128, True),
          ("dense: 16 held-out scenes x 64 agents, K = 20, full set", 16, 64, 20, False))
COLL, TOP_M, RADIUS, METRIC = 0.2, 5, 0.5, "fde"      # the settings the tools time the family with
SWEEPS, DIST = 8, 0.5                                 # evaluate_composed(); evaluate_refine()
PER_LAUNCH = "%9.4f [%8.4f, %8.4f]"                   # cell(fmt=): ms per launch
# the map of the two wall calls, world coordinates (x0 y0 x1 y1): six segments through the square synth_tracks starts its agents in
WALLS = ((2.0, 0.0, 2.0, 6.0), (5.0, 4.0, 5.0, 10.0), (8.0, 0.0, 8.0, 6.0), (0.0, 8.0, 4.0, 8.0), (6.0, 2.0, 10.0, 2.0),
         (3.0, 3.0, 7.0, 7.0))

# the evaluation family: name -> (trainer, data, K, just_one) -> what it returns
CALLS = {
    "test": lambda tr, data, K, one: tr.test(data, n_gen_samples=K, just_one=one),
    "evaluate": lambda tr, data, K, one: tr.evaluate(data, n_gen_samples=K, just_one=one),
    "evaluate_scenes": lambda tr, data, K, one: tr.evaluate_scenes(data, n_gen_samples=K, coll_dist=COLL, just_one=one),
    "evaluate_ranked": lambda tr, data, K, one: tr.evaluate_ranked(data, n_gen_samples=K, top_m=TOP_M, just_one=one),
    "evaluate_diverse": lambda tr, data, K, one: tr.evaluate_diverse(data, n_gen_samples=K, top_m=TOP_M, radius=RADIUS,
                                                                     metric=METRIC, joint=False, just_one=one),
    "evaluate_diverse, joint": lambda tr, data, K, one: tr.evaluate_diverse(data, n_gen_samples=K, top_m=TOP_M, radius=RADIUS,
                                                                            metric=METRIC, joint=True, just_one=one),
    "evaluate_history": lambda tr, data, K, one: tr.evaluate_history(data, n_gen_samples=K, just_one=one),
    "evaluate_horizon": lambda tr, data, K, one: tr.evaluate_horizon(data, n_gen_samples=K, just_one=one),
    "evaluate_composed": lambda tr, data, K, one: tr.evaluate_composed(data, n_gen_samples=K, coll_dist=COLL, sweeps=SWEEPS,
                                                                       just_one=one),
    "evaluate_risk": lambda tr, data, K, one: tr.evaluate_risk(data, n_gen_samples=K, coll_dist=COLL, just_one=one),
    "evaluate_refine": lambda tr, data, K, one: tr.evaluate_refine(data, n_gen_samples=K, dist=DIST, coll_dist=COLL, just_one=one),
    "evaluate_refine, walls": lambda tr, data, K, one: tr.evaluate_refine(data, n_gen_samples=K, dist=DIST, coll_dist=COLL,
                                                                          just_one=one, walls=data.timing_walls),
    "evaluate_walls": lambda tr, data, K, one: tr.evaluate_walls(data, data.timing_walls, n_gen_samples=K, wall_dist=COLL,
                                                                 just_one=one),
}


def load(tool, tree=HERE):
    """socialways_amd of `tree` (this tree, or a built tree of another commit); no GPU: the tool ends here."""
    global sw
    if not torch.cuda.is_available():
        sys.exit("%s measures on an MI355X: no GPU found" % tool)
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import socialways_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(socialways_amd.__file__))) == tree, socialways_amd.__file__
    sw = socialways_amd
    return sw


def trainer():
    torch.manual_seed(0)
    return sw.SocialWaysTrainer(12, use_social=True, device="cuda:0")


def held_out_set(n_test_scenes, agents, device="cuda:0"):
    """SceneDataset keeps the last fifth of the scenes for testing: 5 x n scenes give n held-out ones.  timing_walls: WALLS in
    the dataset's coordinates, for the two wall calls of CALLS."""
    tracks = sw.synth_tracks(5 * n_test_scenes, agents, 8, 12, seed=4321)
    data = sw.SceneDataset(tracks["obsvs"], tracks["preds"], tracks["batches"], tracks["times"], device=device)
    assert len(data.test_batches) == n_test_scenes
    data.timing_walls = data.walls_from_world(WALLS)
    return data


def timed(fn):
    torch.manual_seed(123)
    np.random.seed(123)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()                     # ends in a device -> host copy of the metrics / losses
    return (time.perf_counter() - t0) * 1e3, out


def alternate(calls, warmup, repeats):
    """calls: {name: fn} -> ({name: [ms]}, {name: last result}); the sides alternate inside every repeat."""
    for _ in range(warmup):
        for fn in calls.values():
            timed(fn)
    ms, last = {k: [] for k in calls}, {}
    for _ in range(repeats):
        for k, fn in calls.items():
            t, last[k] = timed(fn)
            ms[k].append(t)
    return ms, last


def cell(v, scale=1.0, fmt="%9.3f [%8.3f, %8.3f]"):
    return fmt % (statistics.median(v) / scale, min(v) / scale, max(v) / scale)


def inside(p, t):
    """Each side's median inside the other's [min, max]: the criterion for a path on which nothing may differ."""
    return min(t) <= statistics.median(p) <= max(t) and min(p) <= statistics.median(t) <= max(p)


def host_chunks(tr, data, K, just_one):
    """evaluate()'s chunks from its public pieces, for the torch-ops baselines: (the scenes' row ranges, obsv, pred, the
    chunk-local ranges) per chunk."""
    batches = [(int(b[0]), int(b[1])) for b in data.test_batches][:1 if just_one else None]
    for i, j in tr.eval_chunks(batches, K, tr.TEST_CHUNK):
        lo, hi = batches[i][0], batches[j - 1][1]
        yield batches[i:j], data.obsv[lo:hi], data.pred[lo:hi], np.asarray([[a - lo, b - lo] for a, b in batches[i:j]], dtype=np.int64)


def first_chunk(tr, data, K, just_one):
    _, obsv, _, sb = next(host_chunks(tr, data, K, just_one))
    return obsv.contiguous(), sb


def parse(doc, repeats, at_least, more=lambda ap: None):
    """The tools' command line: --repeats (default, minimum), --warmup, --out, and what `more(ap)` adds."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=repeats)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    more(ap)
    a = ap.parse_args()
    if a.repeats < at_least:
        ap.error("at least %d repeats" % at_least)
    return a


def parent_tree_args(ap):
    ap.add_argument("--rounds", type=int, default=3, help="--parent-tree: child processes per build")
    ap.add_argument("--parent-tree", default=None, help="a tree of the parent commit with its library built")


def write_out(lines, out):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)


# ---- two builds ------------------------------------------------------------------------------------------------------------
def child(a):
    """One build's side: the calls of a.calls with the streams of a.streams on the three shapes -> one JSON line, a list of
    {shape, stream, call, ms: [...], repr: what the last call returned}."""
    load("tools/_timing.py", a.tree)
    tr, out = trainer(), []
    for name, n_scenes, agents, K, just_one in SHAPES:
        data = held_out_set(n_scenes, agents)
        for stream in a.streams.split(","):
            if stream == "device":      # reaches every call of the family; test() stays on the host stream
                tr.noise = sw.DeviceNoise(2019)
            calls = {c: (lambda c=c: CALLS[c](tr, data, K, just_one)) for c in a.calls.split(";")}
            ms, last = alternate(calls, a.warmup, a.repeats)
            out += [dict(shape=name, stream=stream, call=c, ms=ms[c], repr=repr(last[c])) for c in calls]
            tr.noise = None
    print("TIMING_CHILD " + json.dumps(out))


def across_builds(parent_tree, rounds, repeats, warmup, calls=("evaluate",), streams=("host",)):
    """{(shape, stream, call): {"parent" | "this": {"ms": all timed calls, "repr": the distinct results}}}: `rounds` child
    processes of each build, one at a time, alternating between the builds.  A child that fails ends the run."""
    res = {}
    for _ in range(rounds):
        for build, tree in (("parent", os.path.abspath(parent_tree)), ("this", HERE)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--repeats", str(repeats),
                                "--warmup", str(warmup), "--calls", ";".join(calls), "--streams", ",".join(streams)],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit("child on %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
            for r in json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("TIMING_CHILD ")][-1][13:]):
                side = res.setdefault((r["shape"], r["stream"], r["call"]), {}).setdefault(build, dict(ms=[], repr=[]))
                side["ms"] += r["ms"]
                if r["repr"] not in side["repr"]:
                    side["repr"].append(r["repr"])
    return res


def equal(r):
    """Every child of both builds returned the same values by == (Python floats, ints and strings, read back from repr)."""
    p, t = r["parent"]["repr"], r["this"]["repr"]
    return len(p) == 1 and len(t) == 1 and ast.literal_eval(p[0]) == ast.literal_eval(t[0])


def main():
    def more(ap):
        parent_tree_args(ap)
        ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
        ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
        ap.add_argument("--calls", default="evaluate", help=argparse.SUPPRESS)
        ap.add_argument("--streams", default="host", help=argparse.SUPPRESS)
    a = parse(__doc__, 7, 5, more)
    if a.child:
        return child(a)
    if not a.parent_tree or a.rounds < 3 or a.repeats < 7:
        sys.exit("the A/B of the evaluation family needs --parent-tree, at least 3 rounds and at least 7 repeats")
    res = across_builds(a.parent_tree, a.rounds, a.repeats, a.warmup, tuple(CALLS), ("host", "device"))
    lines = ["the evaluation family, parent build vs this build: %d alternating child processes of each, %d timed calls per child "
             "after %d warm-up calls; host clock around the call, ms; seed 123 before every call, device stream DeviceNoise(2019); "
             "coll_dist %.1f, top_m %d, radius %.2f, %s, %d sweeps, dist %.1f, a map of %d walls"
             % (a.rounds, a.repeats, a.warmup, COLL, TOP_M, RADIUS, METRIC, SWEEPS, DIST, len(WALLS)),
             "%-88s %-6s %-24s %28s %28s %-8s %s" % ("shape", "stream", "call", "parent median [min, max]", "this median [min, max]",
                                                   "inside", "equal")]
    for (shape, stream, call), r in res.items():
        p, t = r["parent"], r["this"]
        lines.append("%-88s %-6s %-24s %28s %28s %-8s %s" % (shape, stream, call, cell(p["ms"]), cell(t["ms"]), inside(p["ms"], t["ms"]),
                                                           equal(r)))
        lines += ["    parent %s" % x for x in p["repr"]] + ["    this   %s" % x for x in t["repr"]]
    lines.append("inside: each build's median lies inside the other's [min, max]; equal: every child of both builds returned the same "
                 "values by ==")
    lines.append("all inside: %s; all equal: %s" % (all(inside(r["parent"]["ms"], r["this"]["ms"]) for r in res.values()),
                                                     all(equal(r) for r in res.values())))
    write_out(lines, a.out)


if __name__ == "__main__":
    main()
