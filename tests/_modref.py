"""Inputs, float64 references and comparisons of the stand-alone module API and of the loss-gradient kernels, shared by
tests/test_gpu_modules_reference.py (the HIP modules, on the GPU) and tests/test_modules_ref_host.py (the fp32 oracle standing
in for them, on the CPU).  Method of tests/_ref64.py: the reference is the oracle's module (oracle/sw_oracle.py) built under
_f64(), loaded with the weights of the code under test and fed the exact fp32 inputs cast to double; outputs are held to
OUT_RT / OUT_AT (_close_out), every gradient tensor to GRAD_REL of its largest entry (_close_grad).

One `run_*` function per group drives an implementation through the reference's call surface (SocialFeatures(x, sb),
fe(f, sb), att(f, h, sb), enc.init_lstm / enc(x) / enc.lstm_h, dec(h, s, z)); the float64 oracle, the fp32 oracle and the HIP
modules all go through the same function, so the three compute the same loss from the same inputs.  A result is
{"out": {name: tensor}, "grad": {name: tensor}}; parameter gradients are in the reference's shapes (`true_view`).

Weights: `oracle32(kind, H)` draws the oracle module from `weight_seed(kind, H)`.  A HIP module constructed after
torch.manual_seed of the same seed has the same weights (it builds the reference-shaped layers first, on the CPU generator),
which the GPU tests assert: what the host file establishes about seeds and fp32 error then holds for the GPU cases.

(Leaky)ReLU kinks (embedder, decoder): `_pick` with `_kink_margin`, the first seed of SEEDS whose float64 forward keeps every
kink input MARGIN away from 0.  Attention, encoder, features and the loss gradients have no kinks: fixed seeds."""
import numpy as np
import torch

import sw_oracle as O
from _ref64 import GRAD_REL, MARGIN, _close_grad, _close_out, _f64, _kink_margin, _pick, scene_rows  # noqa: F401

KINDS = ("emb", "att", "enc", "dec")
_MAKE = {"emb": lambda H: O.EmbedSocialFeatures(3, H), "att": lambda H: O.AttentionPooling(H, H),
         "enc": lambda H: O.EncoderLstm(H, 1), "dec": lambda H: O.DecoderFC(H + H + H // 2)}
FIXED_SEED = 1      # groups without kinks


def weight_seed(kind, H):
    return 4000 + 100 * KINDS.index(kind) + H


def oracle32(kind, H):
    torch.manual_seed(weight_seed(kind, H))
    return _MAKE[kind](H)


def cpu_state(mod):
    return {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}


def oracle64(kind, H, state):
    with _f64():
        m = _MAKE[kind](H)
    m.double().load_state_dict({k: v.detach().cpu().double() for k, v in state.items()})
    return m


def same_weights(state, mod):
    """True iff `state` (of a HIP module) equals the state_dict of the oracle module `mod`, bit for bit."""
    ref = mod.state_dict()
    return set(state) == set(ref) and all(torch.equal(state[k].cpu(), ref[k]) for k in ref)


def pgrads(mod, prefix=""):
    """{prefix + name: gradient in the reference's shape} of every parameter (zeros where autograd left none)."""
    out = {}
    for i, (k, p) in enumerate(mod.named_parameters()):
        g = torch.zeros_like(p) if p.grad is None else p.grad
        if hasattr(mod, "true_view"):
            g = mod.true_view(i, g)
        out[prefix + k] = g.detach().cpu().clone()
    return out


def _put(t, dev, dtype):
    """A fresh leaf on `dev`: never the caller's tensor (a CPU fp32 .to() would return the input itself)."""
    return t.detach().to(dev, dtype).clone()


def _zero(*mods):
    for m in mods:
        m.zero_grad(set_to_none=True)


def _detach(res):
    return {kind: {k: v.detach().cpu().clone() for k, v in d.items()} for kind, d in res.items()}


def compare(got, ref, group, tag, rel=None):
    """Every output of `ref` with _close_out, every gradient with _close_grad (rel: {name: bound}, default GRAD_REL).
    -> {name: max|err| / max|ref|} of the gradients."""
    assert set(got["out"]) == set(ref["out"]) and set(got["grad"]) == set(ref["grad"]), (
        sorted(got["out"]), sorted(ref["out"]), sorted(got["grad"]), sorted(ref["grad"]))
    ratios = {}
    for k, r in ref["out"].items():
        assert bool(torch.isfinite(got["out"][k]).all()), "%s: non-finite entries (%s)" % (k, tag)
        _close_out(got["out"][k], r, k, group, tag)
    for k, r in ref["grad"].items():
        g = got["grad"][k].detach().cpu().double()
        sc = float(r.abs().max())
        if sc > 0 and g.shape == r.shape:
            ratios[k] = float((g - r.double()).abs().max()) / sc
        _close_grad(got["grad"][k], r, "d/d" + k, group, tag, (rel or {}).get(k, GRAD_REL))
    return ratios


def random_walk(B, T, g, p0=0.0):
    start = torch.rand(B, 1, 2, generator=g) * p0
    return start + (torch.randn(B, T, 2, generator=g) * 0.1).cumsum(1)


# ---- features: get_traj_4d, SocialFeatures ------------------------------------------------------------------------------------
TRAJ_CASES = [(2, 1), (8, 12)]
FEATURE_B = [1, 2, 17, 300]     # 17^2 = 289: a partial second block of 256 pairs


def traj_inputs(To, Tp, B=37):
    g = torch.Generator().manual_seed(FIXED_SEED)
    walk = random_walk(B, To + Tp, g, 10.0)
    return walk[:, :To].contiguous(), walk[:, To:].contiguous()


def run_traj(fn, obsv, pred, dev, dtype):
    o, p = _put(obsv, dev, dtype), _put(pred, dev, dtype)
    o4, p4 = fn(o, p)
    return _detach({"out": {"obsv_4d": o4, "pred_4d": p4, "obsv_4d (no future)": fn(o, [])}, "grad": {}})


def feature_inputs(B):
    """(B, 3, 4) 4-d states of a random walk from p0 ~ U[0, 10)^2: SocialFeatures reads the last step."""
    g = torch.Generator().manual_seed(FIXED_SEED + B)
    return O.get_traj_4d(random_walk(B, 3, g, 10.0), [])


def designed_features_batch():
    """The last states of one batch that holds the edge cases of the feature arithmetic."""
    rows = [[0.0, 0.0, 0.0, 0.0],          # 0: a standing agent: |v| = 0, its bearing is 0 / 1e-6
            [1.0, 2.0, 0.3, 0.1],          # 1
            [1.0, 2.0, -0.2, 0.4],         # 2: at the position of 1: dist 0, bearing 0 / 1e-6
            [3.0, 1.0, 0.3, 0.1],          # 3: the velocity of 1: dv = 0, ttca = x / 1e-6
            [0.0, 5.0, 0.5, 0.0],          # 4
            [4.0, 5.0, -0.5, 0.0],         # 5: head-on with 4: dca = |dp + ttca dv| by cancellation
            [1000.0, 3.0, 0.1, -0.2]]      # 6: 1e3 away from everybody
    return torch.tensor(rows, dtype=torch.float32).view(len(rows), 1, 4)


def run_features(fn, x4, dev, dtype):
    return _detach({"out": {"features": fn(_put(x4, dev, dtype), None)}, "grad": {}})


# ---- embed ------------------------------------------------------------------------------------------------------------------------
EMBED_ROWS = [1, 15, 16, 17, 63, 64, 65, "walk"]      # rows R of an (R, 3) tensor; "walk": (40, 40, 3) real features
EMBED_PATHS = ("nograd", "grad", "grad_nofeat")
HIDDEN_2 = [64, 32]


def embed_inputs(rows, H):
    def make(seed):
        g = torch.Generator().manual_seed(seed)
        if rows == "walk":
            feat = O.SocialFeatures(O.get_traj_4d(random_walk(40, 8, g, 10.0), []), None)
        else:
            feat = torch.rand(rows, 3, generator=g) * 2 - 0.5
        return feat, torch.randn(*feat.shape[:-1], H, generator=g)
    return make


def run_embed(fe, inp, path, dev, dtype):
    feat, cot = (_put(t, dev, dtype) for t in inp)
    if path == "nograd":
        with torch.no_grad():
            return _detach({"out": {"emb": fe(feat, None)}, "grad": {}})
    _zero(fe)
    feat.requires_grad_(path == "grad")
    out = fe(feat, None)
    (out * cot).sum().backward()
    grads = pgrads(fe)
    if path == "grad":
        grads["features"] = feat.grad
    return _detach({"out": {"emb": out}, "grad": grads})


def margin_of(mod64, fn):
    """Smallest |kink input| of the float64 forward fn() through mod64."""
    with torch.no_grad(), _f64(), _kink_margin(*(mod64 if isinstance(mod64, (list, tuple)) else [mod64])) as box:
        fn()
    return box[0]


def embed_case(rows, H, state=None):
    """-> dict(inp, seed, tag, ref {path: result}, o32)."""
    o32 = oracle32("emb", H)
    if state is not None:
        assert same_weights(state, o32), "the module under test was not drawn from weight_seed('emb', %d)" % H
    o64 = oracle64("emb", H, state or cpu_state(o32))
    seed, inp, m = _pick(embed_inputs(rows, H), lambda inp: margin_of(o64, lambda: o64(inp[0].double(), None)))
    ref = {p: run_embed(o64, inp, p, "cpu", torch.float64) for p in EMBED_PATHS}
    return dict(inp=inp, seed=seed, tag="R %s H %d seed %d margin %.1e" % (rows, H, seed, m), ref=ref, o32=o32)


# ---- attention --------------------------------------------------------------------------------------------------------------------
ATT_SCENES = [[2], [1, 1, 1], [64], [63, 1, 2], [64, 1, 16, 17], [65], [256], [257], [300, 3, 1]]
ATT_CASES = [(s, 64) for s in ATT_SCENES] + [([63, 1, 2], 32)]
ATT_DIRECT = [[257], [63, 1, 2]]


def block_mask(sizes):
    B = int(np.sum(sizes))
    m = torch.zeros(B, B, dtype=torch.bool)
    for s0, s1 in scene_rows(sizes):
        m[s0:s1, s0:s1] = True
    return m


def att_inputs(sizes, H):
    """f (B, B, H) random inside the scene blocks and NaN everywhere else ("only in-scene blocks are read"), h, cotangent."""
    B = int(np.sum(sizes))
    g = torch.Generator().manual_seed(FIXED_SEED)
    f = torch.randn(B, B, H, generator=g) * 0.5
    f[~block_mask(sizes)] = float("nan")
    return f, torch.randn(B, H, generator=g) * 0.5, torch.randn(B, H, generator=g)


def run_att(att, inp, sizes, dev, dtype, grad=True, diagonal=True):
    """diagonal=False (oracle modules only): the softmax WITHOUT the -1000 diagonal, a mutation the comparison must reject."""
    f, h, cot = (_put(t, dev, dtype) for t in inp)
    sb = scene_rows(sizes)
    fwd = att if diagonal else (lambda f_, h_, sb_: _att_no_diagonal(att, f_, h_, sb_))
    if not grad:
        with torch.no_grad():
            return _detach({"out": {"S": fwd(f, h, sb)}, "grad": {}})
    _zero(att)
    f.requires_grad_()
    h.requires_grad_()
    S = fwd(f, h, sb)
    loss = (S * cot).sum()
    if loss.requires_grad:      # the oracle's S of single-agent scenes alone is a constant 0: every gradient is 0
        loss.backward()
    grads = pgrads(att)
    grads.update(f=torch.zeros_like(f) if f.grad is None else f.grad, h=torch.zeros_like(h) if h.grad is None else h.grad)
    return _detach({"out": {"S": S}, "grad": grads})


def _att_no_diagonal(att, f, h, sb):
    Wh, S = att.W(h), torch.zeros_like(h)
    for s0, s1 in sb:
        if s1 - s0 > 1:
            a = torch.softmax((f[s0:s1, s0:s1] * Wh[s0:s1][None]).sum(-1), dim=1)
            S[s0:s1] = a @ h[s0:s1]
    return S


def att_weights(att, inp, sizes, dtype=torch.float64, diagonal=True):
    """(B, B) attention weights of an oracle module: softmax over each scene block with the -1000 diagonal, 0 elsewhere
    (a single-agent scene's own entry included: train.py:165 skips it)."""
    f, h = inp[0].to(dtype), inp[1].to(dtype)
    B = h.shape[0]
    a = torch.zeros(B, B, dtype=dtype)
    with torch.no_grad():
        Wh = att.W(h)
        for s0, s1 in scene_rows(sizes):
            n = int(s1 - s0)
            if n > 1:
                sigma = (f[s0:s1, s0:s1] * Wh[s0:s1][None]).sum(-1)
                if diagonal:
                    sigma = sigma.masked_fill(torch.eye(n, dtype=torch.bool), -1000.0)
                a[s0:s1, s0:s1] = torch.softmax(sigma, dim=1)
    return a


def check_df_outside(df, sizes, tag):
    out = df.detach().cpu()[~block_mask(sizes)]
    assert bool((out == 0).all()), "d/df outside the scene blocks is not exactly 0 (%s)" % tag


_att_cases = {}     # (sizes, H) -> case: the float64 backward of a 300-agent scene takes seconds, tests share it (never modified)


def att_case(sizes, H, state=None):
    o32 = oracle32("att", H)
    if state is not None:
        assert same_weights(state, o32), "the module under test was not drawn from weight_seed('att', %d)" % H
    key = (tuple(sizes), H)
    if key not in _att_cases:
        _att_cases[key] = _att_case(sizes, H, o32, state)
    return _att_cases[key]


def _att_case(sizes, H, o32, state):
    o64 = oracle64("att", H, state or cpu_state(o32))
    inp = att_inputs(sizes, H)
    ref = run_att(o64, inp, sizes, "cpu", torch.float64)
    return dict(inp=inp, tag="scenes %s H %d" % (sizes, H), ref=ref, ref_nograd={"out": ref["out"], "grad": {}},
                weights=att_weights(o64, inp, sizes), o32=o32, o64=o64)


# ---- encoder ----------------------------------------------------------------------------------------------------------------------
ENC_SHAPES = [(1, 1), (16, 2), (17, 8), (37, 6)]
ENC_H = [64, 48, 8]
ENC_FORMS = ("y", "state", "all", "step")     # the loss on y only / on lstm_h[0], lstm_h[1] only / on all three / a sequence
#                                               followed by one more step from the carried state, loss on everything


def enc_inputs(B, T, H):
    g = torch.Generator().manual_seed(FIXED_SEED)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(B, T, 4) * 0.5, x1=r(B, 4) * 0.5, h0=r(1, B, H) * 0.3, c0=r(1, B, H) * 0.3, wy=r(B, T, H), wy1=r(B, 1, H),
                wh=r(1, B, H), wc=r(1, B, H))


def run_enc(enc, inp, form, need_x, dev, dtype, drop_c=False):
    """drop_c: leave the cell state's term out of the loss (what a backward that drops dcT computes): a mutation."""
    t = {k: _put(v, dev, dtype) for k, v in inp.items()}
    x, x1, h0, c0 = t["x"].requires_grad_(need_x), t["x1"].requires_grad_(need_x), t["h0"].requires_grad_(), t["c0"].requires_grad_()
    _zero(enc)
    enc.init_lstm(h0, c0)
    y = enc(x)
    out = {"y": y}
    loss = 0.0
    if form != "state":
        loss = loss + (y * t["wy"]).sum()
    if form == "step":
        out["y1"] = enc(x1)
        loss = loss + (out["y1"] * t["wy1"]).sum()
    hT, cT = enc.lstm_h
    out.update(hT=hT, cT=cT)
    if form != "y":
        loss = loss + (hT * t["wh"]).sum()
        if not drop_c:
            loss = loss + (cT * t["wc"]).sum()
    loss.backward()
    grads = pgrads(enc)
    grads.update(h0=h0.grad, c0=c0.grad)
    if need_x:
        grads["x"] = x.grad
        if form == "step":
            grads["x1"] = x1.grad
    return _detach({"out": out, "grad": grads})


def enc_case(B, T, H, state=None):
    o32 = oracle32("enc", H)
    if state is not None:
        assert same_weights(state, o32), "the module under test was not drawn from weight_seed('enc', %d)" % H
    o64 = oracle64("enc", H, state or cpu_state(o32))
    inp = enc_inputs(B, T, H)
    ref = {(form, nx): run_enc(o64, inp, form, nx, "cpu", torch.float64) for form in ENC_FORMS for nx in (True, False)}
    return dict(inp=inp, tag="B %d T %d H %d" % (B, T, H), ref=ref, o32=o32, o64=o64)


# ---- decoder ----------------------------------------------------------------------------------------------------------------------
DEC_B = [1, 16, 17, 37]


def dec_inputs(B, H):
    def make(seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(B, H, generator=g) * 0.5, torch.randn(B, H, generator=g) * 0.5, torch.rand(B, H // 2, generator=g),
                torch.randn(B, 2, generator=g))
    return make


def run_dec(dec, inp, need_z, dev, dtype):
    h, s, z, wv = (_put(t, dev, dtype) for t in inp)
    h.requires_grad_()
    s.requires_grad_()
    z.requires_grad_(need_z)
    _zero(dec)
    v = dec(h, s, z)
    (v * wv).sum().backward()
    grads = pgrads(dec)
    grads.update(h=h.grad, s=s.grad)
    if need_z:
        grads["z"] = z.grad
    return _detach({"out": {"v": v}, "grad": grads})


def dec_case(B, H, state=None):
    o32 = oracle32("dec", H)
    if state is not None:
        assert same_weights(state, o32), "the module under test was not drawn from weight_seed('dec', %d)" % H
    o64 = oracle64("dec", H, state or cpu_state(o32))
    seed, inp, m = _pick(dec_inputs(B, H), lambda inp: margin_of(o64, lambda: o64(inp[0].double(), inp[1].double(), inp[2].double())))
    ref = {nz: run_dec(o64, inp, nz, "cpu", torch.float64) for nz in (True, False)}
    return dict(inp=inp, seed=seed, tag="B %d H %d seed %d margin %.1e" % (B, H, seed, m), ref=ref, o32=o32)


# ---- composed: SocialFeatures -> EmbedSocialFeatures -> AttentionPooling -> DecoderFC ----------------------------------------------
COMPOSED_SCENES = [5, 1, 70, 24]
COMPOSED_KINDS = ("emb", "att", "dec")


def composed_inputs(H, sizes=COMPOSED_SCENES):
    B = int(np.sum(sizes))

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        x4 = O.get_traj_4d(random_walk(B, 8, g, 10.0), [])
        return (x4, torch.randn(B, H, generator=g) * 0.5, torch.rand(B, H // 2, generator=g), torch.randn(B, 2, generator=g),
                torch.randn(B, H, generator=g))
    return make


def run_composed(features, mods, inp, sizes, dev, dtype):
    """mods = (fe, att, dec).  Loss <v, wv> + <S, wS>; the features carry no gradient (they are track data)."""
    fe, att, dec = mods
    x4, h, z, wv, wS = (_put(t, dev, dtype) for t in inp)
    sb = scene_rows(sizes)
    h.requires_grad_()
    z.requires_grad_()
    _zero(fe, att, dec)
    feats = features(x4, sb)
    emb = fe(feats, sb)
    S = att(emb, h, sb)
    v = dec(h, S, z)
    ((v * wv).sum() + (S * wS).sum()).backward()
    grads = dict(h=h.grad, z=z.grad)
    for name, m in zip(COMPOSED_KINDS, mods):
        grads.update(pgrads(m, name + "."))
    return _detach({"out": {"features": feats, "emb": emb, "S": S, "v": v}, "grad": grads})


def composed_case(H, states=None, sizes=COMPOSED_SCENES):
    o32 = [oracle32(k, H) for k in COMPOSED_KINDS]
    if states is not None:
        for k, st, m in zip(COMPOSED_KINDS, states, o32):
            assert same_weights(st, m), "the module under test was not drawn from weight_seed(%r, %d)" % (k, H)
    o64 = [oracle64(k, H, st) for k, st in zip(COMPOSED_KINDS, states or [cpu_state(m) for m in o32])]

    def forward(inp):
        x4, h, z = inp[0].double(), inp[1].double(), inp[2].double()
        sb = scene_rows(sizes)
        o64[2](h, o64[1](o64[0](O.SocialFeatures(x4, sb), sb), h, sb), z)

    seed, inp, m = _pick(composed_inputs(H, sizes), lambda inp: margin_of(o64, lambda: forward(inp)))
    ref = run_composed(O.SocialFeatures, o64, inp, sizes, "cpu", torch.float64)
    return dict(inp=inp, seed=seed, tag="scenes %s H %d seed %d margin %.1e" % (sizes, H, seed, m), ref=ref, o32=o32)


# ---- loss gradients: closed forms --------------------------------------------------------------------------------------------------
L2_SMALL = (37, 12)
L2_WINDOWS = [(0, 37), (19, 20), (36, 37), (5, 5)]
L2_BIG = (22000, 12)            # 264 000 elements > 1024 blocks x 256 threads: the grid-stride loop takes a second trip
LOSS_W = 0.5


def l2_inputs(B, Tp):
    """pred4 (B, Tp, 4), ground truth (B, Tp, 2), the gradient buffer's random contents before the call (B, Tp, 4)."""
    g = torch.Generator().manual_seed(FIXED_SEED)
    return torch.randn(B, Tp, 4, generator=g), torch.randn(B, Tp, 2, generator=g), torch.randn(B, Tp, 4, generator=g)


def l2_scale(B, Tp):
    return float(np.float32(LOSS_W / (B * Tp)))     # the kernel takes a C float


def l2_ref(inp, row0, row1, scale, dtype=torch.float64):
    """dpred4[b, t, 0:2] += scale * (p_hat - p) for rows b in [row0, row1), in `dtype`."""
    pred4, gt, d0 = (t.to(dtype) for t in inp)
    d = d0.clone()
    d[row0:row1, :, :2] += scale * (pred4[row0:row1, :, :2] - gt[row0:row1])
    return d


def check_l2(got, inp, row0, row1, scale, group, tag):
    got, d0 = got.detach().cpu(), inp[2]
    keep = torch.ones_like(d0, dtype=torch.bool)
    keep[row0:row1, :, :2] = False
    assert torch.equal(got[keep], d0[keep]), "rows outside [%d, %d) or columns 2:4 changed (%s)" % (row0, row1, tag)
    if row1 > row0:
        _close_out(got[row0:row1, :, :2], l2_ref(inp, row0, row1, scale)[row0:row1, :, :2], "dpred4", group, tag)


VARIETY_K = [1, 2, 20, 63, 64]
VARIETY_B = [1, 5, 1000]
VARIETY_TP = [1, 12, 70]
TIE_REL = 1e-5      # agents whose two smallest float64 errors are closer than this (relative) are left out: fp32 may pick either


def variety_inputs(K, B, Tp, duplicates=None):
    """predK (K * B, Tp, 4), gt (B, Tp, 2), dpredK before the call.  duplicates = (a, b): copies a and b are the same
    near-perfect prediction, the best for every agent."""
    g = torch.Generator().manual_seed(FIXED_SEED + 7 * K + Tp)
    gt = torch.randn(B, Tp, 2, generator=g)
    predK = torch.randn(K, B, Tp, 4, generator=g) * 0.3
    predK[..., :2] += gt
    if duplicates is not None:
        a, b = duplicates
        predK[a, :, :, :2] = gt + torch.randn(B, Tp, 2, generator=g) * 0.01
        predK[b] = predK[a]
    return predK.view(K * B, Tp, 4).contiguous(), gt, torch.randn(K * B, Tp, 4, generator=g)


def variety_ref(inp, K, scale, dtype=torch.float64, with_d=False):
    """-> dict(l2 (K, B), kmin (B,) the lowest k of the smallest error, l2min (B,), left_out (B,) bool; with_d: d, the
    whole buffer after the call)."""
    predK, gt = inp[0].to(dtype), inp[1].to(dtype)
    B, Tp = gt.shape[0], gt.shape[1]
    diff = predK.view(K, B, Tp, 4)[..., :2] - gt
    l2 = (diff ** 2).mean(dim=(2, 3))
    kmin = torch.from_numpy(np.argmin(l2.numpy(), axis=0))      # numpy: the first of equal minima
    l2min = l2.gather(0, kmin[None])[0]
    left_out = torch.zeros(B, dtype=torch.bool)
    if K > 1:
        two = l2.sort(dim=0).values[:2]
        left_out = (two[1] - two[0]) < TIE_REL * two[1]
    out = dict(l2=l2, kmin=kmin, l2min=l2min, left_out=left_out, scale=scale)
    if with_d:
        d = inp[2].to(dtype).clone().view(K, B, Tp, 4)
        ar = torch.arange(B)
        d[kmin, ar, :, :2] += scale * diff[kmin, ar]
        out["d"] = d.view(K * B, Tp, 4)
    return out


def left_out_cap(B):
    return max(B // 100, 10)        # 1 % of the agents or 10 agents, whichever is larger


def check_variety(got_d, got_kmin, got_l2min, inp, K, ref, group, tag, exact_ties=False):
    """exact_ties: exactly equal errors must go to the lowest k, nobody is left out."""
    gt, d0 = inp[1], inp[2]
    B, Tp = gt.shape[0], gt.shape[1]
    got_d, kmin, l2min = got_d.detach().cpu(), got_kmin.detach().cpu().long(), got_l2min.detach().cpu()
    left = torch.zeros(B, dtype=torch.bool) if exact_ties else ref["left_out"]
    assert int(left.sum()) <= left_out_cap(B), "%d agents left out (%s)" % (int(left.sum()), tag)
    assert bool(((kmin >= 0) & (kmin < K)).all()), "kmin out of range (%s)" % tag
    _close_out(l2min, ref["l2min"], "l2min", group, tag)
    keep = ~left
    assert torch.equal(kmin[keep], ref["kmin"][keep]), "kmin differs from the float64 argmin for agents %s (%s)" % (
        (kmin != ref["kmin"])[keep].nonzero().flatten().tolist()[:8], tag)
    # a left-out agent may take either of its near-equal copies, nothing else
    ar = torch.arange(B)
    chosen = ref["l2"][kmin, ar]
    assert bool((chosen - ref["l2min"] <= TIE_REL * chosen)[left].all()), "a left-out agent took a copy that is not near the best"
    got4, d04, predK = got_d.view(K, B, Tp, 4), d0.view(K, B, Tp, 4), inp[0].view(K, B, Tp, 4)
    same = got4 == d04
    same[kmin, ar, :, :2] = True
    assert bool(same.all()), "dpredK changed outside the rows kmin[b] * B + b (%s)" % tag
    want = d04[kmin, ar, :, :2].double() + ref["scale"] * (predK[kmin, ar, :, :2].double() - gt.double())
    _close_out(got4[kmin, ar, :, :2], want, "dpredK", group, tag)


def variety_fp32(inp, K, scale):
    """The honest fp32 computation that stands in for the kernel on the CPU: (d, kmin, l2min)."""
    r = variety_ref(inp, K, scale, dtype=torch.float32, with_d=True)
    return r["d"], r["kmin"], r["l2min"]
