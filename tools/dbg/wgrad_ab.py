"""Is a change of the grouped weight-gradient GEMM (csrc/sw_wgrad.hip, csrc/sw_wgrad_dev.h) a refactor?  The same seeded calls in two
builds, bit for bit.

    python tools/dbg/wgrad_ab.py --dump FILE.npz         on an MI355X, in each of the two built trees (the tree is the one this file
                                                         lies in: copy it and social_ab.py into a built `git archive` of the other
                                                         commit, ab_old/ by convention).  Dump the parent twice first: an array that
                                                         differs between those two is not deterministic in the parent and tells nothing.
    python tools/dbg/wgrad_ab.py --compare A.npz B.npz   no GPU: every array equal by ==, exit status 1 if one is not

--dump:
  gen.*    sw_gen_wgrad(part 0) at B = 2048 and B = 264 (To 8, Tp 12) on random saved rows / delta rows: the generator's own
           problems (tail segment, row0 > 0, 64 + 16 delta columns, several column blocks); d_enc_w, d_dec_w, tmp pre-filled
           with NaN.
  disc.*   one discriminator update (ops.disc_update) at B = 2048 and B = 17 with Adam in the reduction (db2, the image table):
           gradients, weights, both moments, images.
  wide.*   sw_wide_wgrad: a batch of exactly 24 problems (SW_WG_MAXP) of 1 .. 64 delta columns x 4 .. 64 act columns over 1 .. 193
           rows, and one problem of 256 x 160 over 515 rows."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from social_ab import compare          # noqa: E402  (puts the tree's root on sys.path)

ROWS = (1, 3, 4, 5, 13, 17, 127, 128, 129)


def gen_arrays(out):
    import torch
    from socialways_amd import _lib as L
    dev = torch.device("cuda:0")
    lib = L.load()
    To, Tp = 8, 12
    for B in (2048, 264):
        g = torch.Generator().manual_seed(B)
        rnd = lambda n, s=0.3: (torch.randn(n, generator=g) * s).to(dev)
        enc_w, dec_w = rnd(lib.sw_param_count(0, 1)), rnd(lib.sw_param_count(3, 1))
        gsave, gdelta = rnd(L.workspace_floats(L.WS_GSAVE, B, To, Tp)), rnd(L.workspace_floats(L.WS_GDELTA, B, To, Tp))
        z, S = torch.rand(B, 32, generator=g).to(dev), rnd(B * 64).view(B, 64)
        d_enc, d_dec = torch.full_like(enc_w, float("nan")), torch.full_like(dec_w, float("nan"))
        tmp = torch.full((2048,), float("nan"), device=dev)
        ws = torch.empty(L.workspace_floats(L.WS_WGRAD, B, To, Tp), device=dev)
        L.call("sw_gen_wgrad", L.ptr(enc_w), L.ptr(dec_w), L.ptr(gsave), L.ptr(gdelta), L.ptr(z), L.ptr(S), B, To, Tp, L.ptr(d_enc),
               L.ptr(d_dec), 0, L.ptr(ws), L.ptr(tmp), None, L.stream())
        torch.cuda.synchronize()
        out["gen.B%d.d_enc_w" % B], out["gen.B%d.d_dec_w" % B], out["gen.B%d.tmp" % B] = d_enc, d_dec, tmp


def disc_arrays(out):
    import torch
    import socialways_amd as sw
    from socialways_amd import _lib as L
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    lib = L.load()
    for B in (2048, 17):
        torch.manual_seed(B)
        D = sw.Discriminator(12, 64, 2, device=dev)
        obsv = torch.randn(B, 8, 2, device=dev).cumsum(1) * 0.1
        fake, real = torch.randn(B, 12, 4, device=dev) * 0.1, torch.randn(B, 12, 4, device=dev) * 0.1
        z, targets = torch.rand(B, 32, device=dev), torch.tensor([0.05, 0.95], device=dev)
        n = D._flat.numel()
        tab_h = np.empty((n, 2), dtype=np.int32)
        assert lib.sw_disc_image_table(12, tab_h.ctypes.data) == 0
        tab, img = torch.from_numpy(tab_h).to(dev), torch.zeros(lib.sw_disc_image_floats(12), device=dev)
        L.call("sw_disc_images", L.ptr(D._flat), L.ptr(img), L.ptr(tab), 12, L.stream())
        try:
            grad = torch.full_like(D._flat, float("nan"))
            m, v, step = torch.randn(n, device=dev) * 0.01, torch.rand(n, device=dev) * 1e-4, torch.full((), 3.0, device=dev)
            ops.disc_update(D._flat, obsv, [fake, real], targets, (0, 1), z, 1.0 / B, 0.25 / B, grad, ops.Workspaces(dev),
                            adam=(m, v, step, 1e-3, 0.9, 0.999, 1e-8))
            torch.cuda.synchronize()
        finally:
            L.call("sw_disc_images", None, None, None, 0, None)
        for key, t in (("grad", grad), ("w", D._flat), ("m", m), ("v", v), ("img", img)):
            out["disc.B%d.%s" % (B, key)] = t.clone()


def wide_arrays(out):
    import torch
    from socialways_amd import _lib as L
    dev = torch.device("cuda:0")
    batches = {"wide.max": [(ROWS[i % len(ROWS)] + 16 * (i % 5), (1, 2, 16, 32, 64)[i % 5], 4 * (1 + (7 * i) % 16), i % 3 != 0)
                            for i in range(24)],
               "wide.big": [(515, 256, 160, True)]}
    ws = torch.empty(L.workspace_floats(L.WS_WGRAD, 1, 2, 1), device=dev)
    for name, shapes in batches.items():
        g = torch.Generator().manual_seed(len(shapes))
        arr = (ctypes.c_longlong * (10 * len(shapes)))()
        held = []
        for i, (R, N, K, bias) in enumerate(shapes):
            delta, act = torch.randn(R, (N + 3) // 4 * 4, generator=g).to(dev), torch.randn(R, K, generator=g).to(dev)
            dW, db = torch.full((N, K), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)
            held.append((delta, act, dW, db))
            for j, val in enumerate((L.ptr(delta), delta.shape[1], L.ptr(act), K, R, N, K, L.ptr(dW), K, L.ptr(db) if bias else 0)):
                arr[10 * i + j] = int(val)
        assert L.load().sw_wide_wgrad(ctypes.cast(arr, ctypes.c_void_p), len(shapes), L.ptr(ws), L.stream()) == 0
        torch.cuda.synchronize()
        for i, (_, _, dW, db) in enumerate(held):
            out["%s.%d.dW" % (name, i)], out["%s.%d.db" % (name, i)] = dW, db


def dump(path):
    out = {}
    gen_arrays(out)
    disc_arrays(out)
    wide_arrays(out)
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
