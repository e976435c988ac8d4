"""Is a change of the observation-LSTM forward loop (csrc/sw_lstm_dev.h lstm_obs_loop, enc_lstm_fwd_kernel, the unrolled To = 8 loop
of disc_update_kernel) a refactor?  The same seeded calls in two builds, bit for bit.

    python tools/dbg/lstm_ab.py --dump FILE.npz        on an MI355X, in each of the two built trees (the tree is the one this file lies
                                                       in: copy it into a built `git archive` of the other commit, ab_old/ by
                                                       convention).  Dump the parent twice first: an array that differs between those
                                                       two is not deterministic in the parent and tells nothing.
    python tools/dbg/lstm_ab.py --compare A.npz B.npz  no GPU: every array equal by ==, exit status 1 if one is not

Shapes: B = 1, 16, 17, 40 (one live lane, a full tile, a tile of replicas of the last agent, three tiles); T = 2, 3, 5, 8 and, for 4-d
input, 1.  Ragged lengths are mixed and include 0, 1 and T + 3, which the device clamps; outputs are pre-filled with NaN.

The instances of the loop and the calls that reach them (X = x_mode 0 | 1; every encoder call with and without the registered images):
    enc_lstm_fwd_kernel<X, act, y, x4s, false>     enc.*: all 8 output combinations (T <= 3; three of them above), no state / h0 + c0 at
      (lstm_obs_loop<X, NONE | TILE, false, x4s>)    t0 = 0 / h0 + c0 at t0 = 2
                                                   (x_mode 0, act + x4s, no y, images: enc_lstm_fwd8_kernel, not this loop)
    enc_lstm_fwd_kernel<X, false, false, false, true>   encr.*: sw_enc_lstm_fwd_ragged, mixed lengths and NULL
    enc_lstm_fwd_kernel<X, true, false, true, true>     encs.*: sw_enc_lstm_fwd_ragged_save, the same
    lstm_obs_loop<X, SAVE_NONE, false>             dfwd.*.sl0 (disc_fwd_kernel), score.* (disc_score_kernel<false>)
    lstm_obs_loop<X, SAVE_ROWS, false>             dfwd.*.sl1 (sl2 reads those rows back); x_mode 0 also: upd.To5.pre0
                                                   (disc_update_kernel<false>), gen.dobs (disc_obs_lstm_tile in the decode launch's
                                                   rider workgroups), step.dense
    lstm_obs_loop<X, SAVE_NONE, true>              dfwd.*.rag.sl0 (disc_fwd_ragged_kernel), score.*.rag (disc_score_kernel<true>)
    lstm_obs_loop<X, SAVE_ROWS, true>              dfwd.*.rag.sl1; x_mode 0 also: upd.To5.rag (disc_update_kernel<true>), step.ragged
    the unrolled To = 8 loop of disc_update_kernel upd.To8.pre0 (dense), upd.To8.rag; upd.*.pre1 skips the loop (rows from a forward)
    step.dense / step.ragged                       one SocialWaysTrainer(use_graph=False) step each (the second with ragged_fused):
                                                   the returned sums and both packed weight buffers afterwards"""
import argparse
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from social_ab import batches, compare, generator, images          # noqa: E402  (puts the tree's root on sys.path)

BS, TP = (1, 16, 17, 40), 12
NAN = float("nan")


def lengths(B, T, seed):
    """Mixed lengths with the values the device clamps (0, 1, T + 3) and a full and a shortest row where there is room."""
    ln = np.random.RandomState(seed).randint(0, T + 4, size=B).astype(np.int32)
    ln[0] = T
    ln[-1] = 2 if B > 1 else T
    return ln


def track(B, T, cols, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, cols, generator=g) * 0.1).cumsum(1).cuda().contiguous()


def encoder_arrays(out):
    import torch
    from socialways_amd import _lib as L
    dev = torch.device("cuda:0")
    G, _ = generator(dev)
    enc = G.encoder._flat
    p = L.ptr

    def nan(*shape):
        return torch.full(shape, NAN, device=dev)

    for img, x_mode, B in itertools.product((False, True), (0, 1), BS):
        for T in ((2, 3, 5, 8) if x_mode == 0 else (1, 2, 3, 5, 8)):
            x = track(B, T, 2 if x_mode == 0 else 4, 1000 * T + 10 * B + x_mode)
            g = torch.Generator().manual_seed(B + T)
            h0, c0 = (torch.randn(B, 64, generator=g) * 0.5).to(dev), (torch.randn(B, 64, generator=g) * 0.5).to(dev)
            base = "%s.x%d.B%d.T%d" % ("img" if img else "plain", x_mode, B, T)
            with images(G, img, dev):
                for (state, t0), n in itertools.product(((False, 0), (True, 0), (True, 2)), range(4)):
                    for want in itertools.combinations(("y", "act", "x4s"), n):
                        if T > 3 and want not in ((), ("act", "x4s"), ("y", "act", "x4s")):     # the full sweep at T <= 3
                            continue
                        o = {"hT": nan(B, 64), "cT": nan(B, 64)}
                        if "y" in want:
                            o["y"] = nan(B, T, 64)
                        if "act" in want:
                            o["act"] = nan(t0 + T, B, 384)
                        if "x4s" in want:
                            o["x4s"] = nan(t0 + T, B, 4)
                        L.call("sw_enc_lstm_fwd", p(x), x_mode, p(enc), p(h0) if state else None, p(c0) if state else None, B, T,
                               p(o["hT"]), p(o["cT"]), p(o.get("y")), p(o.get("act")), p(o.get("x4s")), t0, L.stream())
                        for k, v in o.items():
                            out["enc.%s.%s.t%d.%s.%s" % (base, "h0" if state else "zero", t0, "+".join(want) or "none", k)] = v
                for tag, ln in (("mixed", torch.from_numpy(lengths(B, T, B + 7 * T)).to(dev)), ("null", None)):
                    hT, cT = nan(B, 64), nan(B, 64)
                    L.call("sw_enc_lstm_fwd_ragged", p(x), x_mode, p(enc), p(ln), B, T, p(hT), p(cT), L.stream())
                    out["encr.%s.%s.hT" % (base, tag)], out["encr.%s.%s.cT" % (base, tag)] = hT, cT
                    hT, cT, act, x4s = nan(B, 64), nan(B, 64), nan(T, B, 384), nan(T, B, 4)
                    L.call("sw_enc_lstm_fwd_ragged_save", p(x), x_mode, p(enc), p(ln), B, T, p(hT), p(cT), p(act), p(x4s), L.stream())
                    for k, v in (("hT", hT), ("cT", cT), ("act", act), ("x4s", x4s)):
                        out["encs.%s.%s.%s" % (base, tag, k)] = v
                torch.cuda.synchronize()


def disc_arrays(out):
    import torch
    import socialways_amd as sw
    from socialways_amd import _lib as L
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(2013)
    D = sw.Discriminator(TP, 64, 2, device=dev)
    w0 = D._flat.clone()
    lib = L.load()
    tab_h = np.empty((D._flat.numel(), 2), dtype=np.int32)
    assert lib.sw_disc_image_table(TP, tab_h.ctypes.data) == 0
    tab, img = torch.from_numpy(tab_h).to(dev), torch.zeros(lib.sw_disc_image_floats(TP), device=dev)
    for cols, B, To in itertools.product((2, 4), BS, (2, 3, 5, 8)):
        base = "x%d.B%d.T%d" % (cols // 4, B, To)
        obsv = track(B, To, cols, 77 * To + B + cols)
        g = torch.Generator().manual_seed(B * To)
        fake, real = (torch.randn(B, TP, 4, generator=g) * 0.1).to(dev), (torch.randn(B, TP, 4, generator=g) * 0.1).to(dev)
        z = torch.rand(B, 32, generator=g).to(dev)
        ln = torch.from_numpy(lengths(B, To, 3 * B + To)).to(dev)
        rows = To * B * 388                       # act | x4s: the head of the save buffer
        for rag in (False, True):
            kw = dict(obs_len=ln) if rag else {}
            tag = base + (".rag" if rag else "")
            for sl in ((0, 1) if rag else (0, 1, 2)):      # 2 reads the rows save_lstm = 1 left in the same workspace
                ws = ops.Workspaces(dev) if sl < 2 else ws
                labels, codes, ctx = ops.disc_forward(D._flat, obsv, [fake, real], save=True, ws=ws, save_lstm=sl, **kw)
                torch.cuda.synchronize()
                for k in range(2):
                    out["dfwd.%s.sl%d.label%d" % (tag, sl, k)], out["dfwd.%s.sl%d.code%d" % (tag, sl, k)] = labels[k], codes[k]
                if sl:
                    out["dfwd.%s.sl%d.rows" % (tag, sl)] = ctx.dsave[:rows].clone()
            score, code = ops.disc_score(D._flat, obsv, torch.stack([fake, real, fake * 0.5]), 3, **kw)
            out["score.%s.score" % tag], out["score.%s.code" % tag] = score, code
        if cols == 4 or To not in (5, 8):
            continue
        targets = torch.tensor([0.05, 0.95], device=dev)
        for mode in ("pre0", "pre1", "rag"):
            D._flat.copy_(w0)
            ws = ops.Workspaces(dev)
            L.call("sw_disc_images", L.ptr(D._flat), L.ptr(img), L.ptr(tab), TP, L.stream())
            try:
                assert ops.disc_update_supported(D._flat, B, To, TP)
                if mode == "pre1":
                    ops.disc_forward(D._flat, obsv, [fake, real], save=True, ws=ws, save_lstm=1)
                gr = torch.full_like(D._flat, NAN)
                m, v = torch.zeros_like(D._flat), torch.zeros_like(D._flat)
                part = torch.full(((B + 15) // 16, 3), NAN, device=dev)
                adam = (m, v, torch.ones((), device=dev), 1e-3, 0.9, 0.999, 1e-8)
                labels, codes = ops.disc_update(D._flat, obsv, [fake, real], targets, (0, 1), z, 1.0 / B, 0.25 / B, gr, ws,
                                                obs_pre=mode == "pre1", loss_part=part, adam=adam,
                                                **(dict(obs_len=ln) if mode == "rag" else {}))
                torch.cuda.synchronize()
            finally:
                L.call("sw_disc_images", None, None, None, 0, None)
            tag = "upd.To%d.B%d.%s." % (To, B, mode)
            for k in range(2):
                out[tag + "label%d" % k], out[tag + "code%d" % k] = labels[k].clone(), codes[k].clone()
            out[tag + "part"], out[tag + "grad"], out[tag + "w"], out[tag + "m"], out[tag + "v"] = part, gr, D._flat.clone(), m, v
    D._flat.copy_(w0)
    # the observation pass of D in the rider workgroups of the decode launch (few tiles: CUs are idle)
    G, mods = generator(dev)
    enc, emb, att, dec = mods
    B, To = 40, 8
    obsv, z = track(B, To, 2, 5), torch.rand(B, 32, generator=torch.Generator().manual_seed(5)).to(dev)
    ws = ops.Workspaces(dev)
    pre = ops.d_obs_buffer(ws, B, To, TP)
    assert pre is not None
    pre.fill_(NAN)
    scenes = ops.SceneIndex.get(batches([8] * 5), B, dev)
    pred, _ = ops.gen_forward(enc._flat, emb._flat, att._flat, dec._flat, obsv, z, scenes, TP, True, save=True, ws=ws, d_obs=(D._flat, pre))
    torch.cuda.synchronize()
    out["gen.dobs.pred"], out["gen.dobs.rows"] = pred, pre[:To * B * 388].clone()


def step_arrays(out):
    import torch
    import socialways_amd as sw
    sizes = [1, 5, 17, 8, 3, 9]
    B, To = sum(sizes), 8
    g = torch.Generator().manual_seed(43)
    tr_ = (torch.randn(B, To + TP, 2, generator=g) * 0.1).cumsum(1)
    obsv, gt, z = tr_[:, :To].cuda().contiguous(), tr_[:, To:].cuda().contiguous(), torch.rand(B, 32, generator=g)
    ln = lengths(B, To, 9).clip(2, To)
    for name, kw, skw in (("dense", {}, {}), ("ragged", dict(ragged_fused=True), dict(obs_len=ln))):
        torch.manual_seed(51)
        tr = sw.SocialWaysTrainer(TP, use_social=True, device="cuda:0", use_graph=False, **kw)
        o = tr.step(obsv, gt, batches(sizes), 0.04, 0.96, z, 1.0, **skw)
        torch.cuda.synchronize()
        out["step.%s.out" % name], out["step.%s.G" % name], out["step.%s.D" % name] = o, tr.G._flat_all.clone(), tr.D._flat.clone()


def dump(path):
    out = {}
    encoder_arrays(out)
    disc_arrays(out)
    step_arrays(out)
    np.savez(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print("%d arrays -> %s" % (len(out), path))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="FILE.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.dump:
        dump(args.dump)
