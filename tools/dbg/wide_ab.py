"""Is a change of the wide path (csrc/sw_wide.hip, socialways_amd/wide.py) a refactor?  The same seeded calls in two builds, bit for bit.

    python tools/dbg/wide_ab.py --dump FILE.npz        on an MI355X, in each of the two built trees (the tree is the one this file lies
                                                       in: copy it and social_ab.py into a built `git archive` of the other commit,
                                                       ab_old/ by convention).  Dump the parent twice first: an array that differs
                                                       between those two is not deterministic in the parent and tells nothing.
    python tools/dbg/wide_ab.py --compare A.npz B.npz  no GPU: every array equal by ==, exit status 1 if one is not

--dump, part 1: a WideTrainer(use_graph=False) per row of CONFIGS - every (seq, decloop, heads) combination of launch forms that
tests/_ref64.WIDE_CASES names, and use_social=False - on scenes of SIZES agents (B = 17: one full 16-agent tile and a one-agent
tile).  _gen_forward and _gen_backward on a seeded cotangent; one D update (_disc_forward(nb = 2, loss) + _disc_backward); the
generator's pass through D (_disc_forward(nb = 1, loss) + _disc_heads_backward(want_dpred)).  Saved: the rollout, every saved-row
and delta buffer (GEN_KEYS, DISC_KEYS, GD_KEYS of the workspace), gp.gflat and dp.gflat (pre-filled with NaN).
Part 2: the entry points no such trainer reaches, at shapes of tests/test_gpu_wide_reference.py.

The 26 kernel instances of sw_wide.hip and the calls that reach them:
    wide_smallk_kernel                      every trainer (the 3-wide pair features, the K = 1 composition products)
    wide_gemm_lds_kernel<1, true / false>   every trainer (its layers at 17 .. 93 rows); gemm.lds1-ov, gemm.lds1-scalar
    wide_gemm_lds_kernel<2, true / false>   gemm.lds2-ov, gemm.lds2-scalar (1 230 rows x 640 columns: 390 blocks of 32 rows)
    wide_gemm_kernel<1,1,1> <1,1,0>         gemm.plain-TTT, gemm.plain-TTF (fewer than 16 rows)
    wide_gemm_kernel<1,0,1> <0,1,1> <0,0,0> every trainer (Wx, WxT, bxc and their way back); gemm.plain-TFT / -FTT / -FFF
    wide_lstm_fwd_kernel                    h96, h160-tp10, h96-nosocial (per-step LSTM); h64-nl3 (the re-fed steps)
    wide_lstm_bwd_kernel<1>                 the same trainers
    wide_lstm_bwd_kernel<2>                 lstm_bwd2 (B = 4 070, H = 256: 512 workgroups, exactly the threshold)
    wide_lstm_seq_fwd / _bwd_kernel<1>      h64-nl3; seq64 (T = 8, B = 17, every optional input given)
    wide_lstm_seq_fwd / _bwd_kernel<2>      h128, h128-nl17
    wide_dec_loop_fwd / _bwd_kernel         h128, h128-nl17
    wide_disc_heads_fwd / _bwd_kernel       h128, h96, h64-nl3, h96-nosocial
    wide_out_fwd / _bwd_kernel              h96, h64-nl3, h160-tp10, h96-nosocial (per-step decode); out (B = 17, D3 = 100)
    wide_sum_steps_kernel                   every trainer (dS); the GEMM-heads trainers once more (docode)
    wide_transpose_kernel, wide_opimage_kernel   every trainer"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from social_ab import batches, compare          # noqa: E402  (puts the tree's root on sys.path)

# (name, hidden size, latent codes, Tp, use_social) -> (seq, decloop, heads)
CONFIGS = (("h128", 128, 2, 12, True),             # (1, 1, 1)
           ("h96", 96, 2, 12, True),               # (0, 0, 1)
           ("h64-nl3", 64, 3, 12, True),           # (1, 0, 1)
           ("h128-nl17", 128, 17, 12, True),       # (1, 1, 0): 17 latent codes are past the heads' limit -> GEMM heads
           ("h160-tp10", 160, 2, 10, True),        # (0, 0, 0)
           ("h96-nosocial", 96, 2, 12, False))
SIZES, TO = [1, 2, 5, 8, 1], 8
TARGETS, W_INFO = (0.03, 0.96), 0.5
GEN_KEYS = ("pred4", "x4", "hs", "cs", "gates", "cat", "u", "a1", "a2", "a3", "S", "attn", "dgates", "dv", "dz3", "dz2", "dz1", "dhcat",
            "dc", "dS")
DISC_KEYS = ("d_hs", "d_cs", "d_gates", "o1", "q1", "both", "c1", "l1", "label", "code", "dlab", "dcod", "dc1", "dl1", "dboth", "dq1",
             "docode", "do1", "d_dhT", "d_dgates", "d_dc", "lpart", "sums")
GD_KEYS = ("q1", "both", "c1", "l1", "label", "code", "dlab", "dcod", "dc1", "dl1", "dboth", "dq1", "dpx", "lpart", "sums")


def trainer_arrays(k, name, H, nl, Tp, social, out):
    import torch
    from socialways_amd import _lib as L
    from socialways_amd.model import _scene_index
    from socialways_amd.wide import WideTrainer, _off
    dev = torch.device("cuda:0")
    torch.manual_seed(2012 + k)
    tr = WideTrainer(Tp, hidden_size=H, n_latent_codes=nl, use_social=social, device="cuda:0", use_graph=False)
    B, nlp, U = sum(SIZES), (nl + 3) // 4 * 4, tr.n_unrolling_steps
    g = torch.Generator().manual_seed(300 + k)
    track = (torch.randn(B, TO + Tp, 2, generator=g) * 0.1).cumsum(1)
    z, cot = torch.rand(B, H // 2, generator=g), torch.randn(B, Tp, 4, generator=g) * 0.1
    sc = _scene_index(batches(SIZES), B, dev)
    w = tr._buffers(B, TO, sc.P)
    # what step() and _step_device do in front of the generator: inputs, label targets, 4-d rows
    w["obsv"].copy_(track[:, :TO])
    w["pred"].copy_(track[:, TO:])
    w["noise"].copy_(z)
    w["scal"][:2].copy_(torch.tensor(TARGETS))
    L.call("sw_traj_4d", L.ptr(w["obsv"]), L.ptr(w["pred"]), B, TO, Tp, L.ptr(w["o4"]), L.ptr(w["p4"]), L.stream())
    forms = (int(tr.seq), int(tr.decloop), int(tr.heads))

    def keep(phase, keys, flat=None):
        torch.cuda.synchronize()
        for key in keys:
            out["%s.%s.%s" % (name, phase, key)] = w[key].clone()
        if flat is not None:
            out["%s.%s.gflat" % (name, phase)] = flat.clone()

    tr._gen_forward(w, sc, B, TO)
    tr.gp.gflat.fill_(float("nan"))
    tr._gen_backward(w, sc, B, TO, cot.to(dev))
    keep("gen", GEN_KEYS, tr.gp.gflat)
    gl, gc = 2.0 / B, W_INFO * 2.0 / (nl * B)
    sums, tg = w["sums"], w["targets"]
    if not tr._disc_forward(w, B, TO, 2, loss=(0, 1, gl, gc, w["lpart"][0])):
        tr._sq(w["label"], 1, None, 0, tg, 0, B, 1, gl, _off(sums, 0), w["dlab"], 4)
        tr._sq(_off(w["label"], B), 1, None, 0, tg, 1, B, 1, gl, _off(sums, 2), _off(w["dlab"], 4 * B), 4)
        tr._sq(w["code"], nl, w["noise"], H // 2, None, 0, B, nl, gc, _off(sums, 1), w["dcod"], nlp)
    tr.dp.gflat.fill_(float("nan"))
    tr._disc_backward(w, B, TO)
    keep("disc", DISC_KEYS, tr.dp.gflat)
    if not tr._disc_forward(w, B, TO, 1, loss=(1, 1, gl, gc, w["lpart"][U + 1])):
        tr._sq(w["label"], 1, None, 0, tg, 1, B, 1, gl, _off(sums, 3 * (U + 1)), w["dlab"], 4)
        tr._sq(w["code"], nl, w["noise"], H // 2, None, 0, B, nl, gc, _off(sums, 3 * (U + 1) + 1), w["dcod"], nlp)
    tr._disc_heads_backward(w, B, 1, True)
    keep("gd", GD_KEYS)
    return forms


# (tag, R, K, N, epi, bias, cin, x transposed, w transposed, extra y_ld): rows of GEMM_CASES of tests/test_gpu_wide_reference.py
GEMM = (("lds1-ov", 31, 640, 128, 3, False, False, False, False, 0), ("lds1-scalar", 63, 100, 100, 1, True, False, False, False, 1),
        ("lds2-ov", 1230, 36, 640, 2, True, False, False, False, 0), ("lds2-scalar", 1230, 36, 638, 0, True, False, False, False, 2),
        ("plain-TTT", 15, 100, 128, 2, True, True, False, False, 0), ("plain-TTF", 15, 640, 65, 1, True, False, False, False, 0),
        ("plain-TFT", 17, 100, 64, 0, False, False, False, True, 0), ("plain-FTT", 63, 20, 64, 3, True, True, True, False, 0),
        ("plain-FFF", 65, 10, 63, 2, True, True, False, False, 0))


def direct_arrays(out):
    import torch
    from socialways_amd import _lib as L
    dev = torch.device("cuda:0")
    st = L.stream()
    held = []

    def dv(t):
        held.append(t.to(dev))
        return held[-1]

    def rand(g, *shape, scale=1.0):
        return dv(torch.randn(*shape, generator=g) * scale)

    def zeros(*shape):
        return torch.zeros(*shape, device=dev)

    p = L.ptr
    for tag, R, K, N, epi, bias, cin, xt, wt, extra in GEMM:
        g = torch.Generator().manual_seed(R * 1000 + K * 10 + N + epi)
        x, wm = rand(g, *((K, R) if xt else (R, K))), rand(g, *((K, N) if wt else (N, K)), scale=K ** -0.5)
        y_ld = N + extra
        bv, aux, cv, y = rand(g, N), rand(g, R, y_ld), rand(g, R, y_ld), zeros(R, y_ld)
        L.call("sw_wide_gemm", p(x), *((1, R) if xt else (K, 1)), p(wm), *((1, N) if wt else (K, 1)), p(bv) if bias else None,
               p(cv) if cin else None, y_ld if cin else 0, p(aux) if epi >= 3 else None, y_ld if epi >= 3 else 0, R, K, N, p(y), y_ld, epi,
               st)
        out["gemm." + tag] = y
    # wide_lstm_bwd_kernel<2>: ((B + 31) / 32) * ((H + 63) / 64) = 128 * 4 = 512 workgroups, a ragged last block of 6 agents
    B, H = 4070, 256
    g = torch.Generator().manual_seed(H + B)
    gates = dv(torch.cat([torch.sigmoid(torch.randn(B, H, generator=g)), torch.sigmoid(torch.randn(B, H, generator=g)),
                          torch.tanh(torch.randn(B, H, generator=g)), torch.sigmoid(torch.randn(B, H, generator=g))], 1))
    c, cp, dh1, dh2 = rand(g, B, H, scale=0.7), rand(g, B, H, scale=0.7), rand(g, B, H + 4), rand(g, B, 2 * H + H // 2)
    dgn, dcin, WhhT = rand(g, B, 4 * H, scale=0.5), rand(g, B, H), rand(g, H, 4 * H, scale=H ** -0.5)
    dg, dc = zeros(B, 4 * H), zeros(B, H)
    L.call("sw_wide_lstm_bwd", p(dh1), H + 4, p(dh2), 2 * H + H // 2, p(dgn), p(WhhT), p(gates), p(c), p(cp), p(dcin), B, H, p(dg), p(dc), st)
    out["lstm_bwd2.dgates"], out["lstm_bwd2.dc"] = dg, dc
    # the sequence kernels at 64 units: forward, then the BPTT over the rows it left
    H, T, B = 64, 8, 17
    g = torch.Generator().manual_seed(H + 10 * T + B)
    x4, Wx, b1, b2 = rand(g, T, B, 4), rand(g, 4 * H, 4, scale=0.5), rand(g, 4 * H, scale=0.1), rand(g, 4 * H, scale=0.1)
    Whh = rand(g, 4 * H, H, scale=H ** -0.5)
    tab = dv(torch.tensor([[0, 4 * H, H, 0, 0, 0], [0, H, 4 * H, 4 * H * H, 1, 0]], dtype=torch.int32))
    img = zeros(2 * 4 * H * H)
    L.call("sw_wide_opimage", p(Whh), p(tab), 2, 2 * 4 * H * H // 4, p(img), st)
    h2_ld = 2 * H + H // 2
    gates, cs, hs, hl2 = zeros(T, B, 4 * H), zeros(T, B, H), zeros(T + 1, B, H), zeros(B, h2_ld)
    hs[0].copy_(rand(g, B, H, scale=0.5))
    L.call("sw_wide_lstm_seq_fwd", p(x4), p(Wx), p(b1), p(b2), p(img), B, H, T, p(gates), p(cs), p(hs), p(hl2), h2_ld, st)
    dh1, dh2, dgi, dci = rand(g, B, H + 4), rand(g, B, h2_ld), rand(g, B, 4 * H, scale=0.5), rand(g, B, H)
    dg = zeros(T, B, 4 * H)
    L.call("sw_wide_lstm_seq_bwd", p(dh1), H + 4, p(dh2), h2_ld, p(dgi), p(dci), L.ptr(img) + 4 * 4 * H * H, p(gates), p(cs), B, H, T,
           p(dg), st)
    for key, v in (("gates", gates), ("cs", cs), ("hs", hs), ("h_last2", hl2), ("dgates", dg)):
        out["seq64." + key] = v
    # the last decoder layer + integration and its backward, on their own
    B, D3, Tp, i, H4 = 17, 100, 3, 1, 4 * 96
    g = torch.Generator().manual_seed(B)
    a3, W4, b4, pos = rand(g, B, D3), rand(g, 2, D3, scale=0.1), rand(g, 2), rand(g, B, 2)
    pred4, x4r = zeros(B, Tp, 4), zeros(B, 4)
    L.call("sw_wide_out_fwd", p(a3), D3, p(W4), p(b4), p(pos), B, p(pred4) + 16 * i, 4 * Tp, p(x4r), st)
    dpred, dgv, WxT, dprun = rand(g, B, Tp, 4), rand(g, B, H4, scale=0.2), rand(g, 4, H4, scale=0.2), rand(g, B, 2)
    dvb, dz3 = zeros(B, 4), zeros(B, D3)
    L.call("sw_wide_out_bwd", p(dpred) + 16 * i, 4 * Tp, p(dgv), p(WxT), H4, p(dprun), B, p(dvb), p(W4), D3, p(dz3), st)
    for key, v in (("pos", pos), ("pred4", pred4), ("x4", x4r), ("dp_run", dprun), ("dv", dvb), ("dz3", dz3)):
        out["out." + key] = v
    torch.cuda.synchronize()


def dump(path):
    out = {}
    for k, cfg in enumerate(CONFIGS):
        print("%-14s (seq, decloop, heads) = %s" % (cfg[0], trainer_arrays(k, *cfg, out)))
    direct_arrays(out)
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
