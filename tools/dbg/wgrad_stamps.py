"""Where the time of a weight-gradient launch goes: per-workgroup wall-clock marks of wgrad_partial_kernel and
wgrad_reduce_kernel (csrc/sw_wgrad.hip, csrc/sw_wgrad_dev.h behind -DSW_WG_STAMP; 100 MHz wall clock).

    bash tools/build_variant.sh stamp "-DSW_WG_STAMP"
    SW_LIB_PATH=variants/lib_stamp.so python tools/dbg/wgrad_stamps.py [--workload m1|c2] [--old-layout]

Runs a few eager training steps of a bench.py workload and reads the marks of the step's last generator launch (more than 12
problems) and last discriminator launch.  Per problem: jobs, and the medians over its jobs of the time from the workgroup's
start to each mark - found (record fetched), descriptors built, first group arrived, loop left, first LDS sum done, stores
issued, end - in us.  For the reduction: problem found, state requested, sums done, end.
--old-layout: a stamp build from before the marks existed (start, end, problem, total_jobs per workgroup; launches under
400 jobs in the second half): durations only."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TICK_US = 0.01          # wall_clock64: 100 MHz
MARKS = ("found", "descr", "group1", "loop", "ldssum", "stores", "end")
RMARKS = ("found", "request", "sums", "end")


def table(rows, names, what):
    """rows: (n, 2 + len(names)) = problem, then us from the start to each mark."""
    print("%-8s %5s  %s" % (what, "WGs", "  ".join("%7s" % n for n in names)))
    for p in sorted(set(rows[:, 0].astype(int))):
        r = rows[rows[:, 0] == p][:, 1:]
        print("%-8d %5d  %s" % (p, len(r), "  ".join("%7.2f" % v for v in np.median(r, axis=0))))
    print("%-8s %5d  %s" % ("all", len(rows), "  ".join("%7.2f" % v for v in np.median(rows[:, 1:], axis=0))))
    print("%-8s %5s  %s" % ("max", "", "  ".join("%7.2f" % v for v in rows[:, 1:].max(axis=0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="m1")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--old-layout", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    from socialways_amd import _lib as L
    lib = L.load()
    if not hasattr(lib, "sw_debug_wg_stamps"):
        sys.exit("this library was not built with -DSW_WG_STAMP (SW_LIB_PATH=%s)" % os.environ.get("SW_LIB_PATH"))
    lib.sw_debug_wg_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.sw_debug_wg_stamps.restype = ctypes.c_int
    leg = bench.Leg(args.workload, torch.device("cuda:0"), None, 1, 0, "weak", 0, 1, use_graph=False)
    for i in range(args.steps):
        leg.one_step(i)
    torch.cuda.synchronize()
    W = 4 if args.old_layout else 10
    n = 2 * 2048 * W + (0 if args.old_layout else 2 * 2048 * 6)
    buf = np.zeros(n, dtype=np.uint64)
    assert lib.sw_debug_wg_stamps(buf.ctypes.data, n) == 0
    print("workload %s, B %d, library %s" % (args.workload, leg.B, L.LIB_PATH))
    for half, name in ((0, "generator launch"), (1, "discriminator launch")):
        g = buf[half * 2048 * W:(half + 1) * 2048 * W].reshape(2048, W).astype(np.float64)
        g = g[g[:, 0] > 0]
        if not len(g):
            print("\n%s: no stamps (at this shape every launch has fewer than 400 jobs)" % name if args.old_layout else
                  "\n%s: no stamps" % name)
            continue
        t0 = g[:, 0].min()
        print("\n%s: %d jobs of %d stamped, starts within %.2f us, span %.2f us" %
              (name, len(g), int(g[0, 3]), (g[:, 0].max() - t0) * TICK_US, (g[:, 1].max() - t0) * TICK_US))
        if args.old_layout:
            table(np.column_stack([g[:, 2], (g[:, 1] - g[:, 0]) * TICK_US]), ("end",), "problem")
            continue
        rel = (np.column_stack([g[:, 4:10], g[:, 1]]) - g[:, :1]) * TICK_US
        table(np.column_stack([g[:, 2], rel]), MARKS, "problem")
        r = buf[2 * 2048 * W + half * 2048 * 6:2 * 2048 * W + (half + 1) * 2048 * 6].reshape(2048, 6).astype(np.float64)
        r = r[r[:, 0] > 0]
        if len(r):
            print("its reduction: %d workgroups stamped, span %.2f us" % (len(r), (r[:, 4].max() - r[:, 0].min()) * TICK_US))
            table(np.column_stack([r[:, 5], (r[:, 1:5] - r[:, :1]) * TICK_US]), RMARKS, "problem")


if __name__ == "__main__":
    main()
