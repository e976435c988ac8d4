#!/usr/bin/env python
"""Timing of SocialWaysTrainer.evaluate_ranked() and of the scoring launch on one MI355X, on the three shapes of
tools/sample_timing.py and by its method: host clock around calls that end in a host synchronisation, warm-up, then
`--repeats` timed calls of each side, ALTERNATING, same seed for every call; median and min / max.

  (a) evaluate_ranked() against the same numbers without the scoring and ranking kernels - what a user of the library had
      before them: evaluate()'s chunks and host noise, Generator.sample(), K calls of Discriminator.forward, then torch
      sort / gather / reductions on the device, float64 sums, one host sync at the end.  evaluate() is timed next to both:
      the part that scores and ranks is what each adds to it.
  (b) one sw_disc_score launch against ONE sw_disc_fwd(nb = 1) launch on the K * B rows with obsv replicated K times (the
      replication itself is not timed) - the single-launch alternative - on the first chunk evaluate() forms of each shape.
      One timed call = `--launches` launches back to back and a synchronisation; ms per launch.

    python tools/rank_timing.py [--repeats 9] [--out profiles/rank_eval_ab.txt]
"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402
from _timing import PER_LAUNCH, TOP_M, cell, first_chunk  # noqa: E402

NEW = ("ade_top1", "fde_top1", "ade_topm", "fde_topm", "best_rank", "score_draws", "score_gt", "code_mse")


def torch_ranked(tr, data, K, M, just_one):
    """The numbers of evaluate_ranked() from Generator.sample(), K calls of Discriminator.forward and torch ops."""
    ss, dev, Tp = float(data.ss), tr.device, tr.n_next
    acc = torch.zeros(12, dtype=torch.float64, device=dev)
    for scenes, obsv, pred, sb in T.host_chunks(tr, data, K, just_one):
        with torch.no_grad():
            noise = tr.eval_noise(scenes, K, tr.noise_len).to(dev)
            ph = tr.G.sample(obsv, K, Tp, sb, noise)
            e = ((ph[..., :2] - pred.unsqueeze(0)) / ss).pow(2).sum(-1).sqrt()                  # (K, n, Tp)
            err = torch.stack([e.mean(2), e[:, :, -1]], dim=2)                                   # (K, n, 2)
            o4, p4 = T.sw.get_traj_4d(obsv, pred)
            outs = [tr.D(o4, ph[k]) for k in range(K)]
            score, code = torch.stack([l[:, 0] for l, _ in outs]), torch.stack([c for _, c in outs])
            order = torch.sort(score.t().contiguous(), dim=1, descending=True, stable=True)[1]  # (n, K)
            top = torch.gather(err.permute(1, 0, 2), 1, order[:, :M, None].expand(-1, -1, 2))    # (n, M, 2)
            rank = (order == err[..., 0].argmin(dim=0)[:, None]).double().argmax(dim=1)
            csq = (code - noise[:, :, :2]).double().pow(2).mean(dim=2)
            acc += torch.cat([err.mean(0).double().sum(0), err.amin(0).double().sum(0), top[:, 0].double().sum(0),
                              top.amin(1).double().sum(0),
                              torch.stack([rank.double().sum(), score.double().sum(), tr.D(o4, p4)[0].double().sum(), csq.sum()])])
    nt = data.n_test_samples
    v = (acc / torch.tensor([nt] * 9 + [K * nt, nt, K * nt], dtype=torch.float64, device=dev)).tolist()
    return dict(zip(("ade_avg", "fde_avg", "ade_min", "fde_min") + NEW, v))


def launch_pair(tr, data, K, just_one, launches):
    """(calls, B): `launches` scoring launches, and as many sw_disc_fwd(nb = 1) launches on the replicated rows."""
    ops = T.sw.ops
    obsv, sb = first_chunk(tr, data, K, just_one)
    B = obsv.shape[0]
    torch.manual_seed(5)
    ph = tr.G.sample(obsv, K, tr.n_next, sb)
    rows, rep, d_w = ph.view(K * B, tr.n_next, 4), obsv.repeat(K, 1, 1).contiguous(), tr.D.packed()
    got = ops.disc_score(d_w, obsv, ph, K)
    labels, codes, _ = ops.disc_forward(d_w, rep, [rows], save=False)
    assert torch.equal(got[0].view(-1), labels[0].view(-1)) and torch.equal(got[1].view(-1, 2), codes[0])

    def score():
        for _ in range(launches):
            out = ops.disc_score(d_w, obsv, ph, K)
        torch.cuda.synchronize()
        return out

    def replicated():
        for _ in range(launches):
            out = ops.disc_forward(d_w, rep, [rows], save=False)
        torch.cuda.synchronize()
        return out
    return {"score": score, "replicated": replicated}, B


def main():
    a = T.parse(__doc__, 9, 9, lambda ap: ap.add_argument("--launches", type=int, default=20, help="(b): launches per timed call"))
    T.load("rank_timing.py")
    tr = T.trainer()
    lines = ["(a) host clock around the call, ms; %d alternating repeats after %d warm-up calls of each; top_m %d; %s"
             % (a.repeats, a.warmup, TOP_M, torch.cuda.get_device_name(0)),
             "%-88s %28s %28s %28s %9s %9s %s" % ("shape", "evaluate() median [min, max]", "evaluate_ranked()",
                                                "sample + K x forward + torch", "new part", "old part", "max(new) < min(old)")]
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        calls = {"evaluate": lambda: T.CALLS["evaluate"](tr, data, K, just_one),
                 "ranked": lambda: T.CALLS["evaluate_ranked"](tr, data, K, just_one),
                 "torch": lambda: torch_ranked(tr, data, K, TOP_M, just_one)}
        ms, last = T.alternate(calls, a.warmup, a.repeats)
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append("%-88s %28s %28s %28s %9.3f %9.3f %s" % (name, cell(ms["evaluate"]), cell(ms["ranked"]), cell(ms["torch"]),
                                                            med["ranked"] - med["evaluate"], med["torch"] - med["evaluate"],
                                                            max(ms["ranked"]) < min(ms["torch"])))
        lines.append("    evaluate()          %s" % np.array2string(np.asarray(last["evaluate"]), precision=7))
        for k in ("ranked", "torch"):
            r = last[k]
            lines.append("    %-19s %s | %s" % (
                "evaluate_ranked()" if k == "ranked" else "torch ops",
                np.array2string(np.asarray([r[x] for x in ("ade_avg", "fde_avg", "ade_min", "fde_min")]), precision=7),
                " ".join("%s %.6f" % (x, r[x]) for x in NEW)))
    lines.append("")
    lines.append("(b) one scoring launch vs one sw_disc_fwd(nb = 1) launch on K * B rows with obsv replicated; first chunk of each "
                 "shape; ms per launch, %d launches per timed call; %d alternating repeats after %d warm-up calls"
                 % (a.launches, a.repeats, a.warmup))
    lines.append("%-88s %6s %5s %28s %28s %8s %s" % ("shape", "B", "K", "sw_disc_score median [min, max]", "sw_disc_fwd, K * B rows",
                                                   "ratio", "score - fwd <= spread of fwd"))
    for name, n_scenes, agents, K, just_one in T.SHAPES:
        data = T.held_out_set(n_scenes, agents)
        calls, B = launch_pair(tr, data, K, just_one, a.launches)
        ms, _ = T.alternate(calls, a.warmup, a.repeats)
        s, f = ([t / a.launches for t in ms[k]] for k in ("score", "replicated"))
        lines.append("%-88s %6d %5d %28s %28s %8.3f %s" % (name, B, K, cell(s, fmt=PER_LAUNCH), cell(f, fmt=PER_LAUNCH),
                                                        statistics.median(s) / statistics.median(f),
                                                        statistics.median(s) - statistics.median(f) <= max(f) - min(f)))
    lines.append("")
    lines.append("(c) not measured: the scoring and ranking kernels are new code next to the existing ones (disc_score_kernel in "
                 "sw_disc.hip, sample_rank_kernel in sw_misc.hip); disc_fwd_tile and every shared phase are unchanged.")
    T.write_out(lines, a.out)


if __name__ == "__main__":
    main()
