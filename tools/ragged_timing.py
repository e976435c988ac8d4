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

    python tools/ragged_timing.py [--repeats 9] [--out profiles/ragged_timing.txt]
"""
import os
import statistics
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


def main():
    a = T.parse(__doc__, 9, 9, lambda ap: ap.add_argument("--launches", type=int, default=20, help="(b): launches per timed call"))
    T.load("ragged_timing.py")
    tr = T.trainer()
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
    lines.append("(c) not measured: skipping the steps in front of a tile's earliest start - the loop runs To steps for every tile.")
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
