"""Is a change of the social block (csrc/sw_social.hip) a refactor?  The same seeded calls in two builds, compared bit for bit.

    python tools/dbg/social_ab.py --dump FILE.npz     on an MI355X, in each of the two built trees (the tree is the one this file lies in:
                                                      copy it into a built `git archive` of the other commit, ab_old/ by convention)
    python tools/dbg/social_ab.py --compare A.npz B.npz   no GPU: every array equal by ==, exit status 1 if one is not
    python tools/dbg/social_ab.py --time              HIP events around the entry points that no bench workload runs: the row-block
                                                      kernels (scenes above 64 agents) and the module API's embedder; median us.
                                                      Run the two trees alternating, three times each.

--dump: ops.gen_forward(save=True) + ops.gen_backward at To 8, Tp 12 for the scene-size sets of SETS (every kernel of the file:
single agents and the rows path, the in-register path across a 16-agent block edge, 64 agents, row-block scenes alone and beside
small ones), each with and without the registered weight images: pred, S, attn and every generator gradient; then
EmbedSocialFeatures / AttentionPooling, forward and backward, on one scene of 5 agents (25 pair rows: no multiple of 16)."""
import argparse
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SETS = ([1, 1, 2, 3, 8, 5], [15, 16, 17], [33, 64], [65], [70, 5, 130, 64, 1])
TO, TP = 8, 12


def batches(sizes):
    ends = np.cumsum(sizes)
    return np.stack([ends - np.asarray(sizes), ends], 1).astype(np.int64)


@contextlib.contextmanager
def images(G, on, dev):
    import torch
    from socialways_amd import _lib as L
    if not on:
        yield
        return
    img = torch.empty(L.load().sw_gen_image_floats(), device=dev)
    L.call("sw_gen_images", L.ptr(G.encoder._flat), L.ptr(G.decoder._flat), L.ptr(G.feature_embedder._flat),
           L.ptr(G.attention._flat), L.ptr(img), L.stream())
    try:
        yield
    finally:
        torch.cuda.synchronize()
        L.call("sw_gen_images", None, None, None, None, None, None)


def generator(dev):
    import torch
    import socialways_amd as sw
    torch.manual_seed(2012)
    G = sw.Generator(hidden_size=64, use_social=True, device=dev)
    G.unify()
    return G, (G.encoder, G.feature_embedder, G.attention, G.decoder)


def inputs(B, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(B, TO, 2, generator=g) * 0.1).cumsum(1), torch.rand(B, 32, generator=g),
            torch.randn(B, TP, 4, generator=g) * 0.1)


def dump(path):
    import torch
    import socialways_amd as sw
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    G, mods = generator(dev)
    enc, emb, att, dec = mods
    out = {}
    for k, sizes in enumerate(SETS):
        B = sum(sizes)
        obsv, z, cot = inputs(B, 100 + k)
        scenes = ops.SceneIndex.get(batches(sizes), B, dev)
        for img in (False, True):
            grads = [torch.full_like(m._flat, float("nan")) for m in mods]
            ws = ops.Workspaces(dev)
            with images(G, img, dev):
                pred, ctx = ops.gen_forward(enc._flat, emb._flat, att._flat, dec._flat, obsv.to(dev), z.to(dev), scenes, TP, True,
                                            save=True, ws=ws)
                ops.gen_backward(enc._flat, emb._flat, att._flat, dec._flat, ctx, cot.to(dev), *grads, ws=ws)
                torch.cuda.synchronize()
            tag = "set%d.%s." % (k, "img" if img else "plain")
            out[tag + "pred"], out[tag + "S"], out[tag + "attn"] = pred, ctx.S, ctx.attn
            for name, g in zip(("encoder", "feature_embedder", "attention", "decoder"), grads):
                out[tag + "d_" + name] = g
    # the module API, one scene of 5 agents
    torch.manual_seed(5)
    fe, at = sw.EmbedSocialFeatures(3, 64, device=dev), sw.AttentionPooling(64, 64, device=dev)
    sb, B = batches([5]), 5
    x = (torch.rand(B, B, 3) * 2 - 0.5).to(dev).requires_grad_()
    h = (torch.randn(B, 64) * 0.5).to(dev).requires_grad_()
    wS, wE = torch.randn(B, 64).to(dev), (torch.randn(B, B, 64) * 0.01).to(dev)
    e = fe(x, sb)
    S = at(e, h, sb)
    ((S * wS).sum() + (e * wE).sum()).backward()
    out.update({"mod.emb": e, "mod.S": S, "mod.dx": x.grad, "mod.dh": h.grad})
    for what, m in (("fe", fe), ("att", at)):
        for name, p in m.named_parameters():
            out["mod.%s.d_%s" % (what, name)] = p.grad
    torch.cuda.synchronize()
    np.savez(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print("%d arrays -> %s" % (len(out), path))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        # == on the bits: NaN equals NaN (a gradient buffer is pre-filled with it), -0 differs from +0
        if A[k].shape != B[k].shape or not np.array_equal(A[k].view(np.uint32), B[k].view(np.uint32)):
            bad.append(k)
    print("%d arrays, %s" % (len(A.files), "ALL EQUAL" if not bad else "DIFFERENT: " + ", ".join(bad)))
    return 1 if bad else 0


def timed(fn, reps=30, warm=5):
    import torch
    t = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warm:
            t.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(t))


def time_calls():
    import torch
    from socialways_amd import ops, _lib as L
    dev = torch.device("cuda:0")
    G, mods = generator(dev)
    enc, emb, att, dec = mods
    sizes = [200, 130, 70] * 8        # row-block scenes only: social_wh, social_big_fwd / _bwd / _finish
    B = sum(sizes)
    obsv, z, cot = inputs(B, 7)
    sc = ops.SceneIndex.get(batches(sizes), B, dev)
    ws = ops.Workspaces(dev)
    grads = [torch.empty_like(m._flat) for m in mods]
    pred, ctx = ops.gen_forward(enc._flat, emb._flat, att._flat, dec._flat, obsv.to(dev), z.to(dev), sc, TP, True, save=True, ws=ws)
    ops.gen_backward(enc._flat, emb._flat, att._flat, dec._flat, ctx, cot.to(dev), *grads, ws=ws)     # sizes every workspace
    S, attn = torch.empty_like(ctx.S), torch.empty_like(ctx.attn)
    dS, dh = torch.randn(B, 64, device=dev), torch.zeros(B, 64, device=dev)
    pws, wgrad, bigp = ws.get("pairs", 0), ws.get("wgrad", 0), ws.get("bigpart", 0)
    st = L.stream()

    def fwd():
        L.call("sw_social_pool_fwd_aux", L.ptr(ctx.obsv), TO, L.ptr(ctx.hT), L.ptr(sc.scene_off), sc.S, B, sc.amax, L.ptr(emb._flat),
               L.ptr(att._flat), L.ptr(S), L.ptr(attn), L.ptr(sc.big_blocks), sc.NB, L.ptr(ctx.wh), L.ptr(ctx.ml), None, None, 0, st)

    def bwd():       # the weight-gradient launch stays pending (the next call drops it): the social kernels alone
        L.call("sw_social_pool_bwd", L.ptr(ctx.obsv), TO, L.ptr(ctx.hT), L.ptr(sc.scene_off), L.ptr(sc.pair_off), sc.S, B, sc.amax,
               sc.P, L.ptr(emb._flat), L.ptr(att._flat), L.ptr(ctx.attn), L.ptr(dS), L.ptr(dh), L.ptr(grads[1]), L.ptr(grads[2]),
               L.ptr(pws), L.ptr(wgrad), L.ptr(sc.big_blocks), sc.NB, L.ptr(ctx.wh), L.ptr(ctx.ml), L.ptr(ctx.S), L.ptr(bigp),
               ws.wgrad_batch, st)

    R = 1 << 16
    feat, dout = torch.rand(R, 3, device=dev), torch.randn(R, 64, device=dev)
    rows, dfeat = torch.empty(R * 196, device=dev), torch.empty(R, 3, device=dev)

    def ebwd():
        L.call("sw_embed_features_bwd", L.ptr(feat), R, L.ptr(emb._flat), L.ptr(dout), L.ptr(rows), L.ptr(dfeat), st)

    for name, fn in (("row-block forward  (social_wh + social_big_fwd), %d agents" % B, fwd),
                     ("row-block backward (social_big_bwd + _finish), %d agents" % B, bwd),
                     ("embed_features_bwd, %d rows" % R, ebwd)):
        print("%-64s %9.1f us" % (name, timed(fn)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="FILE.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.dump:
        dump(args.dump)
    if args.time:
        time_calls()
