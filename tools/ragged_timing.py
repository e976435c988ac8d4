#!/usr/bin/env python
"""Timing of ragged observation histories on one MI355X, on the first evaluation chunk of the three shapes of tools/_timing.py
and by the method of tools/rank_timing.py: host clock around calls that end in a host synchronisation, warm-up, then
`--repeats` timed calls of each side, ALTERNATING, same seed for every call; median and min / max.

  (a) Generator.sample() + Discriminator.score_samples() with obs_len=None against the same rows with history lengths drawn
      uniformly from 2 .. 8 (obs_len on the device: what a ragged SceneDataset hands to evaluate*()).  A tile runs its To
      steps either way, so the expectation is about equal.
  (b) the ragged entry points against the existing ones at FULL length (obs_len all To): sw_enc_lstm_fwd_ragged vs
      sw_enc_lstm_fwd, sw_disc_score_ragged vs sw_disc_score - what the select per step costs.  One timed call = `--launches`
      launches back to back and a synchronisation; ms per launch.  The results are compared bit for bit first.

  (c) training on ragged histories, on the rows and futures of the same chunks as ONE packed batch: SocialWaysTrainer.step()
      eager and dense, against step(obs_len=all To), against step(obs_len=uniform 2 .. 8), against the graph-captured dense
      step.  The first gap is the price of the ragged step's unfused route (no sw_disc_update, no D observation pass in the
      decode launch, no D pass inside the decode BPTT), the second what the lengths themselves cost, the third what a ragged
      sw_disc_update and a captured ragged step could win back.  Every side has a trainer of its own from the same seed and
      takes the same z and label noise; a timed call ends in the host read of the step's sums.  And, as in (b),
      sw_enc_lstm_fwd_ragged_save against sw_enc_lstm_fwd with saves at full length: what the selects on the saved row cost.
      Written to --train-out.

  (d) the fused ragged step (SocialWaysTrainer(ragged_fused=True)), on the packed batches of (c) with obs_len uniform in
      2 .. 8: (i) the PARENT commit's step(obs_len=) - a tree of the parent with its library built, --parent-tree -, (ii) this
      build with the switch off, (iii) ragged_fused=True single steps, (iv) ragged_fused=True through step_many of 4 (ms per
      step), and the captured dense step as the floor.  Two trees cannot share a process: every side runs in child processes
      of its tree, --rounds of each, one at a time and alternating, --repeats / --rounds timed calls per child after its
      warm-up.  And sw_disc_update_ragged at full length against sw_disc_update (same bits) and against sw_disc_fwd_ragged +
      sw_disc_bwd_gan_adam, us per launch.  Written to --fused-out.

    python tools/ragged_timing.py [--repeats 9] [--legs abc] [--out profiles/ragged_timing.txt]
                                  [--train-out profiles/ragged_train_timing.txt]
    python tools/ragged_timing.py --legs d --parent-tree ab_old [--rounds 3] [--fused-out profiles/ragged_fused_timing.txt]
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
from _timing import PER_LAUNCH, cell, first_chunk  # noqa: E402


def sample_and_score(tr, obsv, sb, K, noise, obs_len):
    def call():
        ph = tr.G.sample(obsv, K, tr.n_next, sb, noise, obs_len=obs_len)
        score = tr.D.score_samples(obsv, ph, obs_len=obs_len)[0]
        return float(score.double().sum())      # the host synchronisation
    return call


def launch_pairs(tr, obsv, sb, K, launches):
    """{name: fn} of the four entry points at full length, `launches` launches and a synchronisation each."""
    L, ops = T.sw._lib, T.sw.ops
    B, To = obsv.shape[0], obsv.shape[1]
    enc_w, d_w, st = tr.G.encoder.packed(), tr.D.packed(), L.stream()
    full = torch.full((B,), To, dtype=torch.int32, device=obsv.device)
    ph = tr.G.sample(obsv, K, tr.n_next, sb)
    hT, cT = torch.empty(B, 64, device=obsv.device), torch.empty(B, 64, device=obsv.device)
    hR, cR = torch.empty_like(hT), torch.empty_like(cT)

    def enc():
        for _ in range(launches):
            L.call("sw_enc_lstm_fwd", L.ptr(obsv), 0, L.ptr(enc_w), None, None, B, To, L.ptr(hT), L.ptr(cT), None, None, None, 0, st)
        torch.cuda.synchronize()

    def enc_ragged():
        for _ in range(launches):
            L.call("sw_enc_lstm_fwd_ragged", L.ptr(obsv), 0, L.ptr(enc_w), L.ptr(full), B, To, L.ptr(hR), L.ptr(cR), st)
        torch.cuda.synchronize()

    def score():
        for _ in range(launches):
            out = ops.disc_score(d_w, obsv, ph, K)
        torch.cuda.synchronize()
        return out

    def score_ragged():
        for _ in range(launches):
            out = ops.disc_score(d_w, obsv, ph, K, obs_len=full)
        torch.cuda.synchronize()
        return out
    enc(), enc_ragged()
    assert torch.equal(hT, hR) and torch.equal(cT, cR)
    assert all(torch.equal(x, y) for x, y in zip(score(), score_ragged()))
    return {"enc": enc, "enc_ragged": enc_ragged, "score": score, "score_ragged": score_ragged}


def step_sides(obsv, pred, sb, full, mixed):
    """{name: fn} of the four training steps of (c); every side owns a trainer drawn from the same seed."""
    sw = T.sw
    B = obsv.shape[0]
    z = torch.rand(B, 32, device=obsv.device, generator=torch.Generator(device="cuda").manual_seed(11))

    def side(use_graph, obs_len):
        torch.manual_seed(0)
        tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0", use_graph=use_graph)

        def call():
            out = tr.step(obsv, pred, sb, 0.04, 0.93, z, 1.0, obs_len=obs_len)
            return float(out.sum())      # the host synchronisation
        return call
    return {"eager": side(False, None), "full": side(False, full), "mixed": side(False, mixed), "graph": side(True, None)}


def enc_save_pair(tr, obsv, launches):
    """sw_enc_lstm_fwd with saves against sw_enc_lstm_fwd_ragged_save at full length, `launches` launches and a synchronisation."""
    L = T.sw._lib
    B, To = obsv.shape[0], obsv.shape[1]
    enc_w, st = tr.G.encoder.packed(), L.stream()
    full = torch.full((B,), To, dtype=torch.int32, device=obsv.device)
    bufs = [[torch.empty(B, 64, device=obsv.device), torch.empty(B, 64, device=obsv.device),
             torch.empty(To, B, 384, device=obsv.device), torch.empty(To, B, 4, device=obsv.device)] for _ in range(2)]

    def enc():
        hT, cT, act, x4s = bufs[0]
        for _ in range(launches):
            L.call("sw_enc_lstm_fwd", L.ptr(obsv), 0, L.ptr(enc_w), None, None, B, To, L.ptr(hT), L.ptr(cT), None, L.ptr(act),
                   L.ptr(x4s), 0, st)
        torch.cuda.synchronize()

    def enc_ragged():
        hT, cT, act, x4s = bufs[1]
        for _ in range(launches):
            L.call("sw_enc_lstm_fwd_ragged_save", L.ptr(obsv), 0, L.ptr(enc_w), L.ptr(full), B, To, L.ptr(hT), L.ptr(cT),
                   L.ptr(act), L.ptr(x4s), st)
        torch.cuda.synchronize()
    enc(), enc_ragged()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*bufs))
    return {"enc": enc, "enc_ragged": enc_ragged}


def train_leg(a, tr):
    lines = ["(c) SocialWaysTrainer.step() on the first evaluation chunk as one packed batch: eager dense, step(obs_len=all To), "
             "step(obs_len=uniform 2 .. 8), graph-captured dense; host clock around the call, ms; %d alternating repeats after %d "
             "warm-up calls of each; %s" % (a.repeats, max(a.warmup, 4), torch.cuda.get_device_name(0)),
             "%-88s %6s %28s %28s %8s %28s %8s %28s %8s" % ("shape", "B", "eager dense median [min, max]", "obs_len = all To",
                                                          "/eager", "obs_len uniform 2 .. 8", "/full", "graph dense", "/full")]
    enc_lines = ["", "sw_enc_lstm_fwd_ragged_save at full length (obs_len all To) vs sw_enc_lstm_fwd with saves, same bits; ms per "
                 "launch, %d launches per timed call; %d alternating repeats after %d warm-up calls" % (a.launches, a.repeats, a.warmup),
                 "%-88s %6s %28s %28s %8s" % ("shape", "B", "sw_enc_lstm_fwd median [min, max]", "sw_enc_lstm_fwd_ragged_save", "ratio")]
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        _, obsv, pred, sb = next(T.host_chunks(tr, T.held_out_set(n_scenes, agents), K, just_one))
        obsv, pred = obsv.contiguous(), pred.contiguous()
        B, To = obsv.shape[0], obsv.shape[1]
        gen = torch.Generator(device="cuda").manual_seed(7)
        mixed = torch.randint(2, To + 1, (B,), device="cuda", generator=gen, dtype=torch.int32)
        full = torch.full((B,), To, dtype=torch.int32, device="cuda")
        ms, _ = T.alternate(step_sides(obsv, pred, sb, full, mixed), max(a.warmup, 4), a.repeats)      # the graph is captured on the third call
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append("%-88s %6d %28s %28s %8.3f %28s %8.3f %28s %8.3f"
                     % (name, B, cell(ms["eager"]), cell(ms["full"]), med["full"] / med["eager"], cell(ms["mixed"]),
                        med["mixed"] / med["full"], cell(ms["graph"]), med["graph"] / med["full"]))
        ms, _ = T.alternate(enc_save_pair(tr, obsv, a.launches), a.warmup, a.repeats)
        per = {k: [t / a.launches for t in v] for k, v in ms.items()}
        enc_lines.append("%-88s %6d %28s %28s %8.3f" % (name, B, cell(per["enc"], fmt=PER_LAUNCH), cell(per["enc_ragged"], fmt=PER_LAUNCH),
                                                      statistics.median(per["enc_ragged"]) / statistics.median(per["enc"])))
    T.write_out(lines + enc_lines, a.train_out)


def packed_batches(tr):
    """(c)'s packed batches: per shape (name, obsv, pred, sb, lengths uniform in 2 .. 8)."""
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        _, obsv, pred, sb = next(T.host_chunks(tr, T.held_out_set(n_scenes, agents), K, just_one))
        gen = torch.Generator(device="cuda").manual_seed(7)
        mixed = torch.randint(2, obsv.shape[1] + 1, (obsv.shape[0],), device="cuda", generator=gen, dtype=torch.int32)
        yield name, obsv.contiguous(), pred.contiguous(), sb, mixed


FUSED_SIDES = ("off", "fused", "many4", "dense")     # this build's sides of (d); the parent tree runs "off" alone


def fused_child(a):
    """One tree's sides of (d) on the three packed batches -> one JSON line {shape: {side: [ms per step]}}."""
    sw = T.load("ragged_timing.py", a.tree)
    out = {}
    for name, obsv, pred, sb, mixed in packed_batches(T.trainer()):
        z = torch.rand(obsv.shape[0], 32, device=obsv.device, generator=torch.Generator(device="cuda").manual_seed(11))

        def side(k):
            torch.manual_seed(0)
            tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0", **(dict(ragged_fused=True) if k in ("fused", "many4") else {}))

            def call():
                if k == "many4":
                    outs = tr.step_many([(obsv, pred, 0.04, 0.93, z)] * 4, sb, 1.0, obs_len=[mixed] * 4)
                    return float(sum(o.sum() for o in outs))
                out = tr.step(obsv, pred, sb, 0.04, 0.93, z, 1.0, **({} if k == "dense" else dict(obs_len=mixed)))
                return float(out.sum())      # the host synchronisation
            return call
        ms, _ = T.alternate({k: side(k) for k in a.sides.split(",")}, max(a.warmup, 4), a.repeats)      # captured on the third call
        out[name] = {k: [t / (4 if k == "many4" else 1) for t in v] for k, v in ms.items()}
    print("TIMING_CHILD " + json.dumps(out))


def update_kernels(tr, obsv, pred, launches):
    """{name: fn}: sw_disc_update, sw_disc_update_ragged at full length, and the two ragged launches it replaces; `launches`
    update passes (with the fused Adam) and a synchronisation each.  The bits are compared first."""
    L, ops, sw = T.sw._lib, T.sw.ops, T.sw
    B, To, Tp = obsv.shape[0], obsv.shape[1], pred.shape[1]
    dev = obsv.device
    gen = torch.Generator(device="cuda").manual_seed(5)
    preds = [sw.get_traj_4d(obsv, pred)[1].contiguous(), (torch.randn(B, Tp, 4, device=dev, generator=gen) * 0.1).contiguous()]
    z = torch.rand(B, 32, device=dev, generator=gen)
    full = torch.full((B,), To, dtype=torch.int32, device=dev)
    targets = torch.tensor([0.04, 0.93], device=dev)
    D, w0 = tr.D, tr.D._flat.clone()
    ws = ops.Workspaces(dev)
    state = [torch.zeros_like(D._flat) for _ in range(3)]      # g, m, v
    step = torch.ones((), device=dev)

    def passes(kind, n):
        D._flat.copy_(w0)
        for t in state:
            t.zero_()
        L.call("sw_disc_images", L.ptr(D._flat), L.ptr(tr._dimg), L.ptr(tr._dtab), Tp, L.stream())
        g, m, v = state
        adam = (m, v, step, 1e-3, 0.9, 0.999, 1e-8)
        try:
            for _ in range(n):
                if kind == "two":
                    labels, codes, ctx = ops.disc_forward(D._flat, obsv, preds, save=True, ws=ws, save_lstm=1, obs_len=full)
                    ops.disc_backward_gan(D._flat, ctx, labels, codes, targets, (0, 1), z, 1.0 / B, 0.25 / B, g, (), ws=ws, adam=adam)
                else:
                    ops.disc_update(D._flat, obsv, preds, targets, (0, 1), z, 1.0 / B, 0.25 / B, g, ws, adam=adam,
                                    **(dict(obs_len=full) if kind == "ragged" else {}))
            torch.cuda.synchronize()
        finally:
            L.call("sw_disc_images", None, None, None, 0, None)
        return [D._flat.clone(), g.clone(), m.clone(), v.clone()]
    ref = passes("dense", 2)
    for kind in ("ragged", "two"):
        assert all(torch.equal(x, y) for x, y in zip(ref, passes(kind, 2))), kind
    calls = {k: (lambda k=k: passes(k, launches)) for k in ("dense", "ragged", "two")}
    return calls, lambda: D._flat.copy_(w0)


def fused_leg(a, tr):
    if not a.parent_tree or a.rounds < 1 or a.repeats % a.rounds:
        sys.exit("leg d needs --parent-tree (a tree of the parent commit with its library built) and --repeats a multiple of --rounds")
    res = {}
    for _ in range(a.rounds):      # one child at a time, alternating between the trees
        for tree, sides in ((os.path.abspath(a.parent_tree), "off"), (T.HERE, ",".join(FUSED_SIDES))):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--fused-child", "--tree", tree, "--sides", sides, "--repeats",
                                str(a.repeats // a.rounds), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.exit("child on %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
            got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("TIMING_CHILD ")][-1][13:])
            for shape, ms in got.items():
                for k, v in ms.items():
                    res.setdefault(shape, {}).setdefault("parent" if tree != T.HERE else k, []).extend(v)
    cols = (("parent", "(i) parent step(obs_len)"), ("off", "(ii) switch off"), ("fused", "(iii) ragged_fused"),
            ("many4", "(iv) step_many of 4, per step"), ("dense", "captured dense step"))
    lines = ["(d) the ragged training step on the packed batches of (c), obs_len uniform in 2 .. 8: the parent commit's build, this build "
             "with the switch off, ragged_fused=True single steps and through step_many of 4, and the captured dense step; host clock "
             "around calls that end in a host read, ms per step; %d child processes of each tree, alternating, %d timed calls per child "
             "after %d warm-up calls; %s" % (a.rounds, a.repeats // a.rounds, max(a.warmup, 4), torch.cuda.get_device_name(0)),
             "%-88s %6s " % ("shape", "B") + " ".join("%30s" % c for _, c in cols) + "  (ii) inside (i)   (iii) max < (i) min   (iv) max < (i) min"]
    for name, obsv, pred, sb, mixed in packed_batches(tr):
        r = res[name]
        lines.append("%-88s %6d " % (name, obsv.shape[0]) + " ".join("%30s" % cell(r[k]) for k, _ in cols)
                     + "  %-17s %-21s %s" % (min(r["parent"]) <= statistics.median(r["off"]) <= max(r["parent"]),
                                             max(r["fused"]) < min(r["parent"]), max(r["many4"]) < min(r["parent"])))
    lines += ["", "sw_disc_update_ragged at full length (obs_len all To) vs sw_disc_update (same bits) and vs sw_disc_fwd_ragged + "
              "sw_disc_bwd_gan_adam, each with the weight-gradient GEMM and the fused Adam; us per update pass, %d passes per timed call; "
              "%d alternating repeats after %d warm-up calls" % (a.launches, a.repeats, a.warmup),
              "%-88s %6s %30s %30s %8s %30s %8s" % ("shape", "B", "sw_disc_update median [min, max]", "sw_disc_update_ragged", "/dense",
                                                  "the two ragged launches", "/ragged")]
    for name, obsv, pred, sb, mixed in packed_batches(tr):
        calls, restore = update_kernels(tr, obsv, pred, a.launches)
        ms, _ = T.alternate(calls, a.warmup, a.repeats)
        restore()
        per = {k: [1e3 * t / a.launches for t in v] for k, v in ms.items()}
        med = {k: statistics.median(v) for k, v in per.items()}
        lines.append("%-88s %6d %30s %30s %8.3f %30s %8.3f" % (name, obsv.shape[0], cell(per["dense"]), cell(per["ragged"]),
                                                            med["ragged"] / med["dense"], cell(per["two"]), med["two"] / med["ragged"]))
    T.write_out(lines, a.fused_out)


def main():
    def more(ap):
        ap.add_argument("--launches", type=int, default=20, help="(b), (c), (d): launches per timed call")
        ap.add_argument("--legs", default="abc", help="the legs to run, any of a, b, c, d")
        ap.add_argument("--train-out", default=None, help="(c): where its table is written")
        ap.add_argument("--fused-out", default=None, help="(d): where its tables are written")
        T.parent_tree_args(ap)
        ap.add_argument("--fused-child", action="store_true", help=argparse.SUPPRESS)
        ap.add_argument("--tree", default=T.HERE, help=argparse.SUPPRESS)
        ap.add_argument("--sides", default="off", help=argparse.SUPPRESS)
    a = T.parse(__doc__, 9, 1 if "--fused-child" in sys.argv else 9, more)
    if a.fused_child:
        return fused_child(a)
    T.load("ragged_timing.py")
    tr = T.trainer()
    if "d" in a.legs:
        fused_leg(a, tr)
    if "c" in a.legs:
        train_leg(a, tr)
    if not set("ab") & set(a.legs):
        return
    chunks = []
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        obsv, sb = first_chunk(tr, T.held_out_set(n_scenes, agents), K, just_one)
        chunks.append((name, obsv, sb, K))
    lines = ["(a) Generator.sample() + score_samples() on the first evaluation chunk, obs_len=None vs lengths uniform in 2 .. 8; host "
             "clock around the call, ms; %d alternating repeats after %d warm-up calls of each; %s"
             % (a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "%-88s %6s %5s %28s %28s %8s %s" % ("shape", "B", "K", "obs_len=None median [min, max]", "lengths 2 .. 8", "ratio",
                                                "each median inside the other's range")]
    for name, obsv, sb, K in chunks:
        B = obsv.shape[0]
        gen = torch.Generator(device="cuda").manual_seed(7)
        noise = torch.rand(K, B, 32, device="cuda", generator=gen)
        obs_len = torch.randint(2, obsv.shape[1] + 1, (B,), device="cuda", generator=gen, dtype=torch.int32)
        ms, _ = T.alternate({"dense": sample_and_score(tr, obsv, sb, K, noise, None),
                             "ragged": sample_and_score(tr, obsv, sb, K, noise, obs_len)}, a.warmup, a.repeats)
        lines.append("%-88s %6d %5d %28s %28s %8.3f %s" % (name, B, K, cell(ms["dense"]), cell(ms["ragged"]),
                                                        statistics.median(ms["ragged"]) / statistics.median(ms["dense"]),
                                                        T.inside(ms["dense"], ms["ragged"])))
    lines.append("")
    lines.append("(b) the ragged entry points at full length (obs_len all To) vs the existing ones, same bits; ms per launch, %d launches "
                 "per timed call; %d alternating repeats after %d warm-up calls" % (a.launches, a.repeats, a.warmup))
    lines.append("%-88s %6s %5s %28s %28s %8s %28s %28s %8s" % ("shape", "B", "K", "sw_enc_lstm_fwd median [min, max]",
                                                              "sw_enc_lstm_fwd_ragged", "ratio", "sw_disc_score", "sw_disc_score_ragged",
                                                              "ratio"))
    for name, obsv, sb, K in chunks:
        ms, _ = T.alternate(launch_pairs(tr, obsv, sb, K, a.launches), a.warmup, a.repeats)
        per = {k: [t / a.launches for t in v] for k, v in ms.items()}
        med = {k: statistics.median(v) for k, v in per.items()}
        lines.append("%-88s %6d %5d %28s %28s %8.3f %28s %28s %8.3f"
                     % (name, obsv.shape[0], K, cell(per["enc"], fmt=PER_LAUNCH), cell(per["enc_ragged"], fmt=PER_LAUNCH),
                        med["enc_ragged"] / med["enc"], cell(per["score"], fmt=PER_LAUNCH), cell(per["score_ragged"], fmt=PER_LAUNCH),
                        med["score_ragged"] / med["score"]))
    lines.append("")
    lines.append("not measured: skipping the steps in front of a tile's earliest start - the loop runs To steps for every tile.")
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
