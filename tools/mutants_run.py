#!/usr/bin/env python3
"""Run the suite against seeded-fault libraries, one GPU process at a time (on an MI355X, after tools/mutants_build.py):

    python tools/mutants_run.py --out FILE [--logs DIR] [--no-full] [--only-full] [--tests T ... --] [--deselect ID] name ...

Per name: the test modules that cover the touched file (COVER below) run once under SW_LIB_PATH=variants/lib_<name>.so with
`-m gpu -x`, under `timeout -k 10` sized to that subset (SECONDS below: wall time of each module on the unmodified library).
pytest exit 1 = killed (the first failing test id is recorded), exit 0 = survived the subset; a survivor then gets one run
of the whole `-m gpu` suite (not with --no-full; --only-full skips the subset) before it counts as SURVIVED.  --tests replaces
the covering subset (the rerun of survivors against tests added for them), --deselect leaves a test id out (the suite as it
stood before a test was added).  The loop ends, and the script exits 2, at the
first run that ends with any other status or whose output holds a HIP error string: a seeded fault must fail a test, never
the GPU.  One row per run is appended to --out as it ends: name, file:line, what it models, tests run, outcome, seconds."""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = "tests/test_gpu_%s.py"
# test modules by touched file, the most specific first (-x stops at the first failure)
COVER = {
    "sw_misc.hip": ["launch_tails", "stats", "kernels", "sample", "rank", "modules_reference", "gen_images"],
    "sw_lstm.hip": ["modules_reference", "gen_reference", "kernels", "lstm_zero_state", "ragged", "ragged_train"],
    "sw_lstm_dev.h": ["gen_reference", "disc_reference", "modules_reference", "kernels", "ragged", "ragged_train", "ragged_fused"],
    "sw_decoder.hip": ["gen_reference", "kernels", "sample", "ragged_next", "modules_reference", "ragged", "ragged_train"],
    "sw_social.hip": ["gen_reference", "modules_reference", "scene_wg", "kernels"],
    "sw_disc.hip": ["disc_reference", "kernels", "rank", "ragged", "ragged_train", "ragged_fused"],
    "sw_disc_dev.h": ["disc_reference", "kernels", "rank", "ragged", "ragged_train", "ragged_fused"],
    "sw_wide.hip": ["wide_reference", "wide_step_reference"],
    "sw_wgrad.hip": ["wgrad_bounds", "wgrad_fixed", "disc_reference", "gen_reference"],
    "sw_wgrad_dev.h": ["wgrad_bounds", "wgrad_fixed", "disc_reference", "gen_reference"],
    "sw_wgrad.h": ["kernels", "disc_reference", "step_reference", "launch_tails"],
    "sw_clearance_grad.hip": ["clearance_loss"],
    "sw_scene.hip": ["scene"],
    "sw_scene_dev.h": ["scene", "compose", "clearance_loss", "plan_risk", "wall_loss", "wall_grid", "walls", "ragged_next"],
    "sw_compose.hip": ["compose"],
    "sw_plan_risk.hip": ["plan_risk"],
    "sw_plan_refine.hip": ["refine", "walls"],
    "sw_walls.hip": ["walls"],
    "sw_wall_dev.h": ["walls", "wall_loss", "wall_grid"],
    "sw_wall_grad.hip": ["wall_loss"],
    "sw_wall_grid.hip": ["wall_grid"],
    "sw_nms.hip": ["nms"],
    "sw_noise.hip": ["noise"],
    "sw_generic.hip": ["modules_reference", "wide_reference", "trainer"],
    "sw_modules.hip": ["modules_reference", "trainer"],
    "sw_common.h": ["kernels", "gen_reference", "disc_reference", "wide_reference"],
}
# wall seconds of each module on the unmodified library (pytest --durations, rounded up); a module not listed counts 120
SECONDS = {T % m: s for m, s in {
    "clearance_loss": 3, "compose": 6, "disc_reference": 3, "gen_images": 1, "gen_reference": 8, "kernels": 10, "launch_tails": 1,
    "lstm_zero_state": 1, "modules_reference": 2, "nms": 1, "noise": 1, "plan_risk": 1, "ragged": 5, "ragged_fused": 3,
    "ragged_next": 4, "ragged_train": 6, "rank": 1, "refine": 2, "sample": 5, "scene": 4, "scene_wg": 1, "stats": 1,
    "step_reference": 6, "trainer": 28, "wall_grid": 10, "wall_loss": 9, "walls": 8, "wgrad_bounds": 1,
    "wgrad_fixed": 1, "wide_reference": 5, "wide_step_reference": 7}.items()}
FULL_SECONDS = 900       # the whole -m gpu suite: 315 s
HIP_ERRORS = ("HIP error", "hipError", "illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "Aborted", "Segmentation fault")


def describe(name):
    """(file:line, what it models) from the diff: its first line and the first changed line of its hunk."""
    diff = os.path.join(ROOT, "tools", "mutants", name + ".diff")
    lines = open(diff).read().split("\n")
    what = lines[0].lstrip("# ").strip()
    f = [l[6:].strip() for l in lines if l.startswith("+++ b/")][0]
    hunk = next(i for i, l in enumerate(lines) if l.startswith("@@ -"))
    line = int(re.match(r"@@ -(\d+)", lines[hunk]).group(1))
    for l in lines[hunk + 1:]:
        if l.startswith("-"):
            break
        line += 1
    return os.path.basename(f), line, what


def run(name, tests, limit, log):
    env = dict(os.environ, SW_LIB_PATH=os.path.join(ROOT, "variants", "lib_%s.so" % name))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-rf", "-p", "no:cacheprovider"]
    t0 = time.time()
    r = subprocess.run(cmd + tests, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if log:
        with open(log, "w") as fh:
            fh.write(r.stdout)
    first = re.search(r"^FAILED (\S+)", r.stdout, re.M)
    return r.returncode, first.group(1) if first else None, [e for e in HIP_ERRORS if e in r.stdout], time.time() - t0, r.stdout


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("names", nargs="+")
    ap.add_argument("--out", required=True)
    ap.add_argument("--logs")
    ap.add_argument("--no-full", action="store_true")
    ap.add_argument("--only-full", action="store_true")
    ap.add_argument("--tests", nargs="+")
    ap.add_argument("--deselect", action="append", default=[], help="test id left out (the suite as it stood before a test was added)")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.logs:
        os.makedirs(a.logs, exist_ok=True)

    def record(*cols):
        with open(a.out, "a") as fh:
            fh.write("\t".join(str(c) for c in cols) + "\n")
        print(*cols, flush=True)

    for name in a.names:
        if not os.path.exists(os.path.join(ROOT, "variants", "lib_%s.so" % name)):
            sys.exit("variants/lib_%s.so is not built (tools/mutants_build.py)" % name)
        f, line, what = describe(name)
        stages = []
        if not a.only_full:
            mods = a.tests or [T % m for m in COVER[f]]
            stages.append((mods, 60 + 2 * sum(SECONDS.get(m, 120) for m in mods)))
        if not a.no_full:
            stages.append((["tests"], FULL_SECONDS))
        outcome = None
        for i, (tests, limit) in enumerate(stages):
            log = os.path.join(a.logs, "%s.%d.log" % (name, i)) if a.logs else None
            rc, first, errs, secs, out = run(name, ["--deselect=" + d for d in a.deselect] + tests, limit, log)
            if rc not in (0, 1) or errs or (rc == 1 and not first):
                record(name, "%s:%d" % (f, line), what, " ".join(tests), "STOPPED: exit %d %s" % (rc, " ".join(errs)), "%.0f" % secs)
                print(out[-3000:])
                sys.exit(2)
            outcome = "killed by " + first if rc == 1 else "SURVIVED"
            record(name, "%s:%d" % (f, line), what, " ".join(tests), outcome + ("" if rc or tests == ["tests"] else " (subset)"),
                   "%.0f" % secs)
            if rc == 1:
                break


if __name__ == "__main__":
    main()
