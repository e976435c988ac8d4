"""The WIDE path (socialways_amd/wide.py, csrc/sw_wide.hip and its use of csrc/sw_wgrad.hip: hidden sizes above 64) against
a FLOAT64 reference.  The float64 side is the oracle's modules (oracle/sw_oracle.py) cast to double and loaded from the
trainer's state_dicts, or a few lines of torch in double; it runs on the CPU from the exact fp32 inputs and weights of the
code under test.  The wide path is never compared with itself.

Part 1 drives a WideTrainer(use_graph=False) through its own pieces on buffers from _buffers(B, To, P) - the staging of
step() (sw_traj_4d, the noise copy, the label targets) is done here - for every row of _ref64.WIDE_CASES:
  a. generator: _gen_forward, then _gen_backward on a random cotangent with gp.gflat pre-filled with NaN: the rollout, hs[To],
     cs[To-1], S and the attention weights per scene (_close_out); every generator gradient (close_grads_branch_consistent)
  b. one discriminator update: _disc_forward(nb = 2, loss) + _disc_backward with dp.gflat pre-filled with NaN: label / code of
     both branches, the three loss sums, EVERY D parameter gradient against the LSGAN + info loss of train.py:484-494
  c. generator phase through D: _disc_forward(nb = 1, loss) + _disc_heads_backward(want_dpred): w["dpx"] against the float64
     d(g_loss)/d(pred4)
Each row asserts the launch forms it was chosen for (tr.seq, tr.decloop, tr.heads, the truth of _disc_forward's return).
Seed rule: pick_fewest over SEEDS, at most MAX_AMBIGUOUS kink inputs within MARGIN of 0 (tests/test_ref64_host.py checks that
condition on the CPU).  Bounds: OUT_RT / OUT_AT and GRAD_REL of tests/_ref64.py, unchanged.

Part 2 calls the C ABI directly (L.call) at the shapes whose launch forms Part 1 cannot reach at small sizes and compares
with float64 torch on the same fp32 inputs; every output buffer is pre-filled with a sentinel, every element inside the
logical shape must be written and every element outside it must be bit-unchanged: sw_wide_gemm (every dispatch branch of
the host function, asserted by shape arithmetic), sw_wide_lstm_fwd / _bwd (both backward forms; the <2> form at exactly 512
workgroups), sw_wide_lstm_seq_fwd / _bwd and sw_wide_dec_loop_fwd / _bwd on their own with every saved row the header promises,
sw_wide_disc_heads_fwd / _bwd on both sides of each limit of sw_wide_disc_heads_supported, sw_wide_transpose / sw_wide_opimage
(bit-exact against the header's index formulas), sw_wide_sum_steps, sw_wide_out_fwd / _bwd, sw_wide_wgrad (splits, the 64 + 16
column split, more than one 24-problem batch in a call, refusals asserted) and the generic pieces both wider paths share
(sw_pair_features, sw_attn_pairs_fwd / _bwd, sw_lstm_point_*, sw_act_*, sw_sqdiff).

The module's report (pytest -s) lists per group the largest output and gradient error as a fraction of max|ref|.
Observed on an MI355X, largest max|err| / max|ref| per group (outputs; gradients): 1a.gen 8.8e-7; 1.63e-5 (the metric shape has
14 ambiguous units at its best seed, none flipped; every other row has a seed without one).  1b.disc 2.64e-6 (the fake-branch
label of the 288-unit row, which carries OUT_AT_LABEL; 7.9e-7 without it); 5.5e-7.  1c.gphase 1.3e-6 (the same label; the rest
within 1e-6).  2.gemm 1.2e-6, 2.lstm 1.2e-6, 2.seq 7.2e-7, 2.decloop 8.7e-7, 2.heads 6.1e-7, 2.out 1.5e-7, 2.wgrad 2.2e-7,
2.generic 6.7e-7 (elementwise rtol OUT_RT on top of OUT_AT: a group may show more than 1e-6 and pass).  

What the module turned up: sw_wide_wgrad refused (SW_ESHAPE) delta widths whose last block of up to 64 columns is 17, 19, ... 63
wide and neither even up to 32 nor a multiple of 4 - n_latent_codes = 17 could not run a discriminator update on the wide path.
It now cuts such a block at its last multiple of 16 (rows h128-nl17, test_wide_wgrad_against_float64 N = 17 / 63 / 273)."""
import ctypes

import numpy as np
import pytest
import torch

import sw_oracle as O
from _ref64 import (G_NAMES, GRAD_REL, MARGIN, OUT_AT, OUT_RT, TARGETS, W_INFO, WIDE_CASES, _close_grad, _close_out, _f64, _note,  # noqa: F401
                    _report, close_grads_branch_consistent, gen_mods, gen_params, run64, scene_rows, wide_oracle64, wide_oracles,
                    wide_pick, wide_torch_seed)

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _L():
    from socialways_amd import _lib
    return _lib


# =============================================================================================================================
# Part 1: the engine, phase by phase
# =============================================================================================================================
def _trainer(H, nl, Tp, use_social=True):
    from socialways_amd.wide import WideTrainer
    torch.manual_seed(wide_torch_seed(H, nl, Tp))
    tr = WideTrainer(Tp, hidden_size=H, n_latent_codes=nl, use_social=use_social, device="cuda:0", use_graph=False)
    assert tr.loss_info_w == W_INFO and tr.use_info_loss
    return tr


def _stage(tr, w, obsv, real, z):
    """What step() does in front of _step_device, and _step_device in front of the generator: inputs, targets, 4-d rows."""
    L = _L()
    B, To = obsv.shape[0], obsv.shape[1]
    w["obsv"].copy_(obsv)
    w["pred"].copy_(real)
    w["noise"].copy_(z)
    w["scal"][:2].copy_(torch.tensor(TARGETS))
    L.call("sw_traj_4d", L.ptr(w["obsv"]), L.ptr(w["pred"]), B, To, tr.n_next, L.ptr(w["o4"]), L.ptr(w["p4"]), L.stream())


def _state64(orc, o):
    enc = orc.encoder
    with torch.no_grad(), _f64():
        B = o.shape[0]
        enc.init_lstm(torch.zeros(1, B, enc.hidden_size), torch.zeros(1, B, enc.hidden_size))
        enc(O.get_traj_4d(o, []))
        return enc.lstm_h[0].squeeze(0).clone(), enc.lstm_h[1].squeeze(0).clone()


def _attn64(orc, o, hT, sb):
    """Attention weights of every scene of 2..64 agents: [(scene, n, (n, n) weights: row i over the scene's agents j)]."""
    out = []
    with torch.no_grad(), _f64():
        last4 = O.get_traj_4d(o, [])[:, -1]
        Wh = orc.attention.W(hT)
        for s, (s0, s1) in enumerate(np.asarray(sb).reshape(-1, 2)):
            s0, n = int(s0), int(s1 - s0)
            if n < 2:
                continue
            st = last4[s0:s0 + n]
            emb = orc.feature_embedder(O.pair_features(st[:, None, :], st[None, :, :]), None)
            sigma = (emb * Wh[s0:s0 + n][None, :, :]).sum(-1).masked_fill(torch.eye(n, dtype=torch.bool), -1000.0)
            out.append((s, n, torch.softmax(sigma, dim=1)))
    return out


# The bound of the labels of the 288-unit row.  With default-initialised weights and To = 2 its labels nearly cancel: the largest
# is 8.8e-3 (2.2e-2 on the real branch) where a row's |c1_k w_k| + |b| add up to 0.149, 17 times that, and the rows of `both` / c1
# that feed the sum are 0.28 / 0.11 large, so their own fp32 rounding (a few 1e-8) is already a few 1e-6 of the largest label.
# The fp32 CPU oracle's D, fed the device's rollout, misses the float64 fake-branch labels of this very case and seed by
# LABEL_288_ORACLE = 1.105e-6 of the largest label (real branch 5.9e-7, code_hat 2.2e-7: those keep OUT_AT); the
# GEMM heads (K = 144 on the MFMA) by 2.64e-6: no term is missing (one average term is 1.0e-3, over 40 000 times the error).  Two
# fp32 evaluation orders: the bound is 4 x the oracle's error, and the kernel's error does not enter it.  Every other tensor
# of the row, and every other row, keeps OUT_AT.
LABEL_288_ORACLE = 1.105e-6
OUT_AT_LABEL = {"h288": {"fake": 4 * LABEL_288_ORACLE}}          # the fake branch (D update and generator phase) only


def _d_forward64(Dref, o4, fake, real):
    lf, cf = Dref(o4, fake)
    lr, cr = Dref(o4, real)
    return lf, cf, lr, cr


def _sums_of(tr, w, row, took_heads):
    return (w["lpart"][row].sum(0) if took_heads else w["sums"][row]).detach().cpu().double()


def _gen_phase(tr, w, sc, orc, obsv, z, cot, sb, seed, tag, use_social=True):
    B, To, Tp = obsv.shape[0], obsv.shape[1], tr.n_next
    o64, z64, c64 = obsv.double(), z.double(), cot.double()

    def fn():
        pred = orc.predict(o64, z64, Tp, sb)
        return (pred * c64).sum(), (pred.detach(), orc.last["S"].detach().clone())

    run, (pred64, S64) = run64(gen_params(orc), gen_mods(orc), fn, seed)
    tr.gp.gflat.fill_(float("nan"))
    tr._gen_backward(w, sc, B, To, cot.to(_dev()))
    torch.cuda.synchronize()
    g = "1a.gen"
    _close_out(w["pred4"], pred64, "rollout", g, tag)
    hT64, cT64 = _state64(orc, o64)
    _close_out(w["hs"][To], hT64, "hs[To]", g, tag)
    _close_out(w["cs"][To - 1], cT64, "cs[To-1]", g, tag)
    _close_out(w["S"], S64, "S", g, tag)
    if use_social and sc.P > 0:
        attn, poff = w["attn"].cpu(), sc.pair_off.cpu().tolist()
        for s, n, a64 in _attn64(orc, o64, hT64, sb):
            _close_out(attn[poff[s]:poff[s] + n * n].view(n, n), a64, "attention weights of scene %d" % s, g, tag)
    got = {}
    for name in G_NAMES:
        for k, p in getattr(tr.G, name).named_parameters():
            got[name + "." + k] = tr.gp.g(p).clone()
    close_grads_branch_consistent(got, run, g, tag)
    if not use_social or sc.P == 0:
        assert not bool(w["S"].any())
        for k, v in got.items():
            if k.startswith(("feature_embedder.", "attention.")):
                assert not bool(v.any()), "d/d%s must be exactly zero (%s)" % (k, tag)


def _disc_update_phase(tr, w, orc, obsv, real, z, took_heads_expected, seed, tag, at_label={}):
    from socialways_amd.wide import _off
    B, To, Tp, nl, H = obsv.shape[0], obsv.shape[1], tr.n_next, tr.n_latent_codes, tr.H
    nlp = (nl + 3) // 4 * 4
    gl, gc = 2.0 / B, W_INFO * 2.0 / (nl * B)
    sums, tg = w["sums"], w["targets"]
    took = bool(tr._disc_forward(w, B, To, 2, loss=(0, 1, gl, gc, w["lpart"][0])))
    assert took == took_heads_expected == tr.heads
    if not took:
        tr._sq(w["label"], 1, None, 0, tg, 0, B, 1, gl, _off(sums, 0), w["dlab"], 4)
        tr._sq(_off(w["label"], B), 1, None, 0, tg, 1, B, 1, gl, _off(sums, 2), _off(w["dlab"], 4 * B), 4)
        tr._sq(w["code"], nl, w["noise"], H // 2, None, 0, B, nl, gc, _off(sums, 1), w["dcod"], nlp)
    tr.dp.gflat.fill_(float("nan"))
    tr._disc_backward(w, B, To)
    torch.cuda.synchronize()
    Dref = orc.D
    o4, p4 = O.get_traj_4d(obsv.double(), real.double())
    fake = w["pred4"].detach().cpu().double()          # D's fake input is what the device rolled out, exactly
    z2 = z.double()[:, :nl]
    t0, t1 = (float(torch.tensor(t, dtype=torch.float32)) for t in TARGETS)

    def fn():
        lf, cf, lr, cr = _d_forward64(Dref, o4, fake, p4)
        loss = ((lf - t0) ** 2).mean() + ((lr - t1) ** 2).mean() + W_INFO * ((cf - z2) ** 2).mean()     # train.py:484-494
        s3 = torch.stack([((lf - t0) ** 2).sum(), ((cf - z2) ** 2).sum(), ((lr - t1) ** 2).sum()]).detach()
        return loss, (lf.detach(), cf.detach(), lr.detach(), cr.detach(), s3)

    run, (lf, cf, lr, cr, s3) = run64(list(Dref.named_parameters()), [Dref], fn, seed)
    g = "1b.disc"
    _close_out(w["label"][:B], lf, "label (fake)", g, tag, at_label.get("fake", OUT_AT))
    _close_out(w["label"][B:], lr, "label (real)", g, tag, at_label.get("real", OUT_AT))
    _close_out(w["code"][:B], cf, "code (fake)", g, tag)
    _close_out(w["code"][B:], cr, "code (real)", g, tag)
    _close_out(_sums_of(tr, w, 0, took), s3, "loss sums", g, tag)
    got = {k: tr.dp.g(p).clone() for k, p in tr.D.named_parameters()}
    close_grads_branch_consistent(got, run, g, tag)


def _gen_through_disc_phase(tr, w, orc, obsv, z, took_heads_expected, tag, at_label={}):
    from socialways_amd.wide import _off
    B, To, Tp, nl, H = obsv.shape[0], obsv.shape[1], tr.n_next, tr.n_latent_codes, tr.H
    nlp = (nl + 3) // 4 * 4
    U = tr.n_unrolling_steps
    gl, gc = 2.0 / B, W_INFO * 2.0 / (nl * B)
    sums, tg = w["sums"], w["targets"]
    w["dpx"].fill_(float("nan"))
    took = bool(tr._disc_forward(w, B, To, 1, loss=(1, 1, gl, gc, w["lpart"][U + 1])))
    assert took == took_heads_expected
    if not took:
        tr._sq(w["label"], 1, None, 0, tg, 1, B, 1, gl, _off(sums, 3 * (U + 1)), w["dlab"], 4)
        tr._sq(w["code"], nl, w["noise"], H // 2, None, 0, B, nl, gc, _off(sums, 3 * (U + 1) + 1), w["dcod"], nlp)
    tr._disc_heads_backward(w, B, 1, True)
    torch.cuda.synchronize()
    Dref = orc.D
    o4 = O.get_traj_4d(obsv.double(), [])
    p = w["pred4"].detach().cpu().double().requires_grad_()
    z2 = z.double()[:, :nl]
    t1 = float(torch.tensor(TARGETS[1], dtype=torch.float32))
    with _f64():
        label, code = Dref(o4, p)
    (((label - t1) ** 2).mean() + W_INFO * ((code - z2) ** 2).mean()).backward()                        # train.py:512-523
    s2 = torch.stack([((label - t1) ** 2).sum(), ((code - z2) ** 2).sum()]).detach()
    g = "1c.gphase"
    _close_out(w["label"][:B], label, "label", g, tag, at_label.get("fake", OUT_AT))
    _close_out(w["code"][:B], code, "code", g, tag)
    _close_out(_sums_of(tr, w, U + 1, took)[:2], s2, "loss sums", g, tag)
    _close_out(w["dpx"].view(B, Tp, 4), p.grad, "d(g_loss)/d(pred4)", g, tag)


@pytest.mark.parametrize("case", WIDE_CASES, ids=[c[0] for c in WIDE_CASES])
def test_wide_engine_phases_against_float64(case):
    from socialways_amd.model import _scene_index
    name, H, nl, Tp, To, sizes, (seq, decloop, heads), gen_checked = case
    B, sb = int(np.sum(sizes)), scene_rows(sizes)
    tr = _trainer(H, nl, Tp)
    assert (tr.seq, tr.decloop, tr.heads) == (seq, decloop, heads), "launch forms of %s: %s" % (name, (tr.seq, tr.decloop, tr.heads))
    o32, _ = wide_oracles(H, nl, Tp)          # same torch seed, same construction order: the trainer's initial weights
    for n in G_NAMES:
        for k, v in getattr(o32, n).state_dict().items():
            assert torch.equal(getattr(tr.G, n).state_dict()[k].cpu(), v), (n, k)
    orc = wide_oracle64(tr.G, tr.D)
    seed, (obsv, real, z, cot), n_amb = wide_pick(orc, B, To, Tp, H, sb)
    tag = "%s, seed %d, %d kink inputs within %.1e of 0" % (name, seed, n_amb, MARGIN)
    sc = _scene_index(sb, B, _dev())
    w = tr._buffers(B, To, sc.P)
    _stage(tr, w, obsv, real, z)
    tr._gen_forward(w, sc, B, To)
    if gen_checked:
        _gen_phase(tr, w, sc, orc, obsv, z, cot, sb, seed, tag)
    at_label = OUT_AT_LABEL.get(name, {})
    _disc_update_phase(tr, w, orc, obsv, real, z, heads, seed, tag, at_label)
    _gen_through_disc_phase(tr, w, orc, obsv, z, heads, tag, at_label)


def test_wide_engine_without_the_social_block_against_float64():
    """use_social=False: S is zeros, no social launch, the embedder and attention gradients are exact zeros."""
    from socialways_amd.model import _scene_index
    H, nl, Tp, To, sizes = 96, 2, 12, 8, [5, 1, 9, 16, 3, 2]
    B, sb = int(np.sum(sizes)), scene_rows(sizes)
    tr = _trainer(H, nl, Tp, use_social=False)
    orc = wide_oracle64(tr.G, tr.D)
    assert not orc.use_social
    seed, (obsv, real, z, cot), n_amb = wide_pick(orc, B, To, Tp, H, sb)
    tag = "no social, seed %d, %d kink inputs within %.1e of 0" % (seed, n_amb, MARGIN)
    sc = _scene_index(sb, B, _dev())
    w = tr._buffers(B, To, sc.P)
    _stage(tr, w, obsv, real, z)
    tr._gen_forward(w, sc, B, To)
    _gen_phase(tr, w, sc, orc, obsv, z, cot, sb, seed, tag, use_social=False)


# =============================================================================================================================
# Part 2: the entry points, called directly
# =============================================================================================================================
SENT = -1.7014118e38          # a value no kernel here produces; compared bit for bit


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _sentinel(n):
    return torch.full((int(n),), SENT, device=_dev())


def _view(buf, off, rows, ld):
    return buf[off:off + rows * ld].view(rows, ld)


def _untouched(buf, written):
    """Every element of the flat buffer `buf` outside the boolean mask `written` still holds the sentinel's bits."""
    b = buf.detach().cpu()
    keep = ~written.reshape(-1)
    assert bool((b[keep].view(torch.int32) == torch.tensor(SENT).view(torch.int32)).all()), "wrote outside the logical shape"


def _mask2d(total, off, rows, cols, ld):
    m = torch.zeros(total, dtype=torch.bool)
    idx = off + (torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]).reshape(-1)
    m[idx] = True
    return m


class _Keep:
    """Host tensor -> device, kept alive until the test ends (a pointer handed to a kernel must outlive its temporary)."""

    def __init__(self):
        self.held = []

    def __call__(self, t):
        if t is None:
            return None
        t = t.to(_dev())
        self.held.append(t)
        return t


def _p(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


# ---- sw_wide_gemm ---------------------------------------------------------------------------------------------------------
def _gemm_branch(R, K, N, x_rs, x_cs, w_rs, w_cs, y_ld, y_al, cin_ld, cin_al, aux_ld, aux_al):
    """The dispatch of the host function sw_wide_gemm, restated: which kernel instantiation a call takes."""
    xv = x_cs == 1 and x_rs % 4 == 0 and K % 4 == 0
    wv = w_cs == 1 and w_rs % 4 == 0 and K % 4 == 0
    ov = (N % 4 == 0 and y_ld % 4 == 0 and y_al and (cin_ld is None or (cin_ld % 4 == 0 and cin_al))
          and (aux_ld is None or (aux_ld % 4 == 0 and aux_al)))
    if K <= 8:
        return "smallk"
    if xv and wv and R >= 16:
        b2 = ((R + 31) // 32) * ((N + 63) // 64)
        return "lds%d-%s" % (2 if b2 >= 384 else 1, "ov" if ov else "scalar")
    if xv and wv and ov:
        return "plain-TTT"
    if xv and wv:
        return "plain-TTF"
    if xv and ov:
        return "plain-TFT"
    if wv and ov:
        return "plain-FTT"
    return "plain-FFF"


GEMM_BRANCHES = {"smallk", "lds1-ov", "lds1-scalar", "lds2-ov", "lds2-scalar", "plain-TTT", "plain-TTF", "plain-TFT", "plain-FTT",
                 "plain-FFF"}
# (R, K, N, epi, bias, cin: None / "own" / "alias", x transposed (x_cs != 1), w transposed (w_cs != 1), extra y_ld, y offset in
#  floats, expected branch)
GEMM_CASES = [
    # wide_smallk_kernel: K of 1, 3, 4, 8; the composition products of wide.py (K = 1 with cin aliasing y, transposed operands)
    (36, 1, 96, 0, False, "alias", False, False, 0, 0, "smallk"), (17, 3, 32, 1, True, None, False, False, 0, 0, "smallk"),
    (33, 4, 65, 4, False, None, False, False, 3, 0, "smallk"), (65, 8, 2, 2, True, "own", True, True, 0, 1, "smallk"),
    # LDS form, one agent tile: float4 epilogue and the scalar one (N = 100 with y_ld 101; a y pointer offset by one float)
    (16, 20, 64, 2, True, None, False, False, 0, 0, "lds1-ov"), (17, 100, 64, 0, False, "own", False, False, 4, 0, "lds1-ov"),
    (31, 640, 128, 3, False, None, False, False, 0, 0, "lds1-ov"), (33, 20, 4, 4, True, "alias", False, False, 0, 0, "lds1-ov"),
    (63, 100, 100, 1, True, None, False, False, 1, 0, "lds1-scalar"), (65, 20, 64, 0, True, "own", False, False, 4, 1, "lds1-scalar"),
    (17, 12, 1, 0, False, None, False, False, 0, 0, "lds1-scalar"), (16, 640, 63, 2, True, None, False, False, 0, 0, "lds1-scalar"),
    (33, 100, 65, 4, False, "own", False, False, 2, 0, "lds1-scalar"), (31, 20, 2, 3, True, None, False, False, 0, 0, "lds1-scalar"),
    # LDS form, two agent tiles: 39 x 10 = 390 >= 384 blocks of 32 rows, the last row block holds 14 rows
    (1230, 36, 640, 2, True, None, False, False, 0, 0, "lds2-ov"), (1230, 36, 640, 4, False, "own", False, False, 0, 1, "lds2-scalar"),
    (1230, 36, 638, 0, True, None, False, False, 2, 0, "lds2-scalar"),
    # fewer than 16 rows, and strided operands: wide_gemm_kernel's five instantiations
    (1, 20, 64, 0, True, None, False, False, 0, 0, "plain-TTT"), (15, 100, 128, 2, True, "own", False, False, 0, 0, "plain-TTT"),
    (15, 640, 65, 1, True, None, False, False, 0, 0, "plain-TTF"), (1, 20, 1, 0, False, None, False, False, 0, 0, "plain-TTF"),
    (17, 100, 64, 0, False, None, False, True, 0, 0, "plain-TFT"), (512, 128, 4, 0, False, None, False, True, 0, 0, "plain-TFT"),
    (4, 128, 512, 0, False, None, True, False, 0, 0, "plain-FTT"), (63, 20, 64, 3, True, "alias", True, False, 0, 0, "plain-FTT"),
    (128, 512, 4, 0, False, None, True, True, 0, 0, "plain-FFF"), (65, 10, 63, 2, True, "own", False, False, 0, 0, "plain-FFF"),
    (31, 10, 2, 4, False, None, True, False, 1, 0, "plain-FFF"), (16, 100, 65, 0, True, None, False, True, 0, 0, "plain-FFF"),
]


def test_gemm_table_visits_every_dispatch_branch():
    assert {c[-1] for c in GEMM_CASES} == GEMM_BRANCHES
    assert {c[3] for c in GEMM_CASES} == {0, 1, 2, 3, 4}
    assert {16, 17, 31, 33, 63, 65, 1, 15} <= {c[0] for c in GEMM_CASES}
    assert {1, 2, 63, 64, 65} <= {c[2] for c in GEMM_CASES} and {1, 3, 4, 8, 10, 20, 100, 640} <= {c[1] for c in GEMM_CASES}


@pytest.mark.parametrize("case", GEMM_CASES, ids=["%dx%dx%d-epi%d-%s" % (c[0], c[1], c[2], c[3], c[-1]) for c in GEMM_CASES])
def test_wide_gemm_against_float64(case):
    L = _L()
    R, K, N, epi, bias, cin, xt, wt, ld_extra, y_off, branch = case
    g = torch.Generator().manual_seed(R * 1000 + K * 10 + N + epi)
    x, wm = _rand(g, R, K), _rand(g, N, K, scale=K ** -0.5)
    bv = _rand(g, N) if bias else None
    y_ld = N + ld_extra
    aux = _rand(g, R, y_ld) if epi >= 3 else None
    cin_own = _rand(g, R, y_ld) if cin == "own" else None
    ybuf = _sentinel(R * y_ld + 8)
    yv = _view(ybuf, y_off, R, y_ld)
    y0 = None
    if cin == "alias":                      # the in-place += of wide.py: cin and y are the same rows
        y0 = _rand(g, R, N)
        yv[:, :N] = y0.to(_dev())
    xd = (x.t().contiguous() if xt else x).to(_dev())
    wd = (wm.t().contiguous() if wt else wm).to(_dev())
    x_rs, x_cs = (1, R) if xt else (K, 1)
    w_rs, w_cs = (1, N) if wt else (K, 1)
    bd = None if bv is None else bv.to(_dev())
    ad = None if aux is None else aux.to(_dev())
    cd = None if cin_own is None else cin_own.to(_dev())
    cin_ptr, cin_ld = (_p(ybuf, y_off), y_ld) if cin == "alias" else ((_p(cd), y_ld) if cd is not None else (None, 0))
    al = lambda p: p is not None and p % 16 == 0
    got_branch = _gemm_branch(R, K, N, x_rs, x_cs, w_rs, w_cs, y_ld, al(_p(ybuf, y_off)), cin_ld if cin else None, al(cin_ptr),
                              y_ld if ad is not None else None, al(_p(ad)))
    assert xd.data_ptr() % 16 == 0 and wd.data_ptr() % 16 == 0
    assert got_branch == branch, (got_branch, branch)
    L.call("sw_wide_gemm", _p(xd), x_rs, x_cs, _p(wd), w_rs, w_cs, _p(bd), cin_ptr, cin_ld, _p(ad), y_ld if ad is not None else 0,
           R, K, N, _p(ybuf, y_off), y_ld, epi, L.stream())
    torch.cuda.synchronize()
    ref = x.double() @ wm.double().t()
    if bv is not None:
        ref = ref + bv.double()
    if cin == "own":
        ref = ref + cin_own.double()[:, :N]
    elif cin == "alias":
        ref = ref + y0.double()
    if epi == 1:
        ref = ref.clamp_min(0)
    elif epi == 2:
        ref = torch.where(ref > 0, ref, 0.2 * ref)
    elif epi == 3:
        ref = torch.where(aux.double()[:, :N] > 0, ref, torch.zeros_like(ref))
    elif epi == 4:
        ref = torch.where(aux.double()[:, :N] > 0, ref, 0.2 * ref)
    _close_out(yv[:, :N], ref, "y", "2.gemm", "%s" % (case,))
    _untouched(ybuf, _mask2d(ybuf.numel(), y_off, R, N, y_ld))


# ---- sw_wide_lstm_fwd / _bwd ----------------------------------------------------------------------------------------------
def _lstm64(x4, h, c, Wx, b1, b2, Whh):
    pre = x4 @ Wx.t() + b1 + (b2 if b2 is not None else 0) + (h @ Whh.t() if h is not None else 0)
    H = Wx.shape[0] // 4
    i, f, gg, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
    cn = f * (c if c is not None else 0) + i * gg
    return torch.cat([i, f, gg, o], 1), cn, o * torch.tanh(cn)


@pytest.mark.parametrize("H,B,prev,h2", [(32, 1, True, False), (32, 65, False, True), (96, 15, True, True), (96, 64, False, False),
                                         (160, 17, True, False), (160, 63, True, True), (256, 65, True, True), (256, 1, False, False),
                                         (96, 65, True, False), (256, 17, True, False)])
def test_wide_lstm_fwd_against_float64(H, B, prev, h2):
    L = _L()
    g = torch.Generator().manual_seed(H + B)
    x4, Wx, b1, b2 = _rand(g, B, 4), _rand(g, 4 * H, 4, scale=0.5), _rand(g, 4 * H, scale=0.1), _rand(g, 4 * H, scale=0.1)
    Whh = _rand(g, 4 * H, H, scale=H ** -0.5)
    hp, cp = (_rand(g, B, H, scale=0.5), _rand(g, B, H, scale=0.5)) if prev else (None, None)
    use_b2 = B % 2 == 1
    x_ld, hp_ld, h_ld, h2_ld = 8, H + 4, H + 8, 2 * H + H // 2
    xd = torch.zeros(B, x_ld)
    xd[:, :4] = x4
    hpd = None
    if prev:
        hpd = torch.zeros(B, hp_ld)
        hpd[:, :H] = hp
    dv = _Keep()
    xd, hpd, cpd, Wxd, b1d, b2d, Whhd = dv(xd), dv(hpd), dv(cp), dv(Wx), dv(b1), dv(b2 if use_b2 else None), dv(Whh)
    gates, cout, hout = _sentinel(B * 4 * H + 4), _sentinel(B * H + 4), _sentinel(B * h_ld)
    hout2 = _sentinel(B * h2_ld) if h2 else None
    L.call("sw_wide_lstm_fwd", _p(xd), x_ld, _p(hpd), hp_ld if prev else 0, _p(cpd), _p(Wxd), _p(b1d), _p(b2d), _p(Whhd), B, H,
           _p(gates), _p(cout), _p(hout), h_ld, _p(hout2), h2_ld if h2 else 0, L.stream())
    torch.cuda.synchronize()
    d = lambda t: None if t is None else t.double()
    g64, c64, h64 = _lstm64(d(x4), d(hp), d(cp), d(Wx), d(b1), d(b2) if use_b2 else None, d(Whh))
    tag = "H %d B %d prev %s" % (H, B, prev)
    _close_out(_view(gates, 0, B, 4 * H), g64, "gates", "2.lstm", tag)
    _close_out(_view(cout, 0, B, H), c64, "c", "2.lstm", tag)
    _close_out(_view(hout, 0, B, h_ld)[:, :H], h64, "h", "2.lstm", tag)
    _untouched(gates, _mask2d(gates.numel(), 0, B, 4 * H, 4 * H))
    _untouched(cout, _mask2d(cout.numel(), 0, B, H, H))
    _untouched(hout, _mask2d(hout.numel(), 0, B, H, h_ld))
    if h2:
        _close_out(_view(hout2, 0, B, h2_ld)[:, :H], h64, "h (second copy)", "2.lstm", tag)
        _untouched(hout2, _mask2d(hout2.numel(), 0, B, H, h2_ld))


def _lstm_bwd_form(B, H):
    nub = (H + 63) // 64
    return 2 if ((B + 31) // 32) * nub >= 512 else 1


# every NULL combination of dh_ext, dh_ext2, dg_next, dc_in (bits of `null`), both launch forms
_BWD = [(32, 1, 0), (32, 17, 1), (96, 15, 2), (96, 65, 3), (160, 63, 4), (160, 64, 5), (256, 17, 6), (256, 65, 7),
        (32, 64, 8), (96, 17, 9), (160, 1, 10), (256, 15, 11), (96, 63, 12), (160, 65, 13), (256, 64, 14), (32, 15, 15),
        (256, 4070, 0), (96, 8170, 2)]


@pytest.mark.parametrize("H,B,null", _BWD)
def test_wide_lstm_bwd_against_float64(H, B, null):
    L = _L()
    form = _lstm_bwd_form(B, H)
    assert form == (2 if B > 1000 else 1)
    if B == 4070:
        assert ((B + 31) // 32) * 4 == 512 and B % 32 == 6                      # exactly the threshold, ragged last block
    if B == 8170:
        assert ((B + 31) // 32) * 2 == 512 and B % 32 == 10 and H % 64 == 32    # ... and a half-filled unit block
    g = torch.Generator().manual_seed(H + B + null)
    gates = torch.cat([torch.sigmoid(_rand(g, B, H)), torch.sigmoid(_rand(g, B, H)), torch.tanh(_rand(g, B, H)), torch.sigmoid(_rand(g, B, H))], 1)
    c, c_prev = _rand(g, B, H, scale=0.7), (_rand(g, B, H, scale=0.7) if null != 15 else None)
    dhe_ld, dhe2_ld = H + 4, 2 * H + H // 2
    dh1 = None if null & 1 else _rand(g, B, H)
    dh2 = None if null & 2 else _rand(g, B, H)
    dgn = None if null & 4 else _rand(g, B, 4 * H, scale=0.5)
    dcin = None if null & 8 else _rand(g, B, H)
    Whh = _rand(g, 4 * H, H, scale=H ** -0.5)

    def padded(t, ld):
        if t is None:
            return None
        o = torch.zeros(t.shape[0], ld)
        o[:, :t.shape[1]] = t
        return dv(o)

    dv = _Keep()
    dg, dc = _sentinel(B * 4 * H + 4), _sentinel(B * H + 4)
    WhhT = Whh.t().contiguous()
    L.call("sw_wide_lstm_bwd", _p(padded(dh1, dhe_ld)), dhe_ld, _p(padded(dh2, dhe2_ld)), dhe2_ld, _p(dv(dgn)), _p(dv(WhhT)),
           _p(dv(gates)), _p(dv(c)), _p(dv(c_prev)), _p(dv(dcin)), B, H, _p(dg), _p(dc), L.stream())
    torch.cuda.synchronize()
    d = lambda t: 0 if t is None else t.double()
    dh = d(dh1) + d(dh2) + (dgn.double() @ Whh.double() if dgn is not None else 0) + torch.zeros(B, H, dtype=torch.float64)
    gi, gf, gg, go = (gates.double()[:, k * H:(k + 1) * H] for k in range(4))
    tc = torch.tanh(c.double())
    dct = dh * go * (1 - tc * tc) + d(dcin)
    ref = torch.cat([dct * gg * gi * (1 - gi), dct * d(c_prev) * gf * (1 - gf), dct * gi * (1 - gg * gg), dh * tc * go * (1 - go)], 1)
    tag = "H %d B %d null %d form <%d>" % (H, B, null, form)
    _close_out(_view(dg, 0, B, 4 * H), ref, "dgates", "2.lstm", tag)
    _close_out(_view(dc, 0, B, H), dct * gf, "dc_prev", "2.lstm", tag)
    _untouched(dg, _mask2d(dg.numel(), 0, B, 4 * H, 4 * H))
    _untouched(dc, _mask2d(dc.numel(), 0, B, H, H))


# ---- sw_wide_transpose / sw_wide_opimage: bit-exact against the index formulas of include/socialways_hip.h --------------------
def test_wide_transpose_is_bit_exact():
    L = _L()
    g = torch.Generator().manual_seed(4)
    shapes = [(1, 1), (31, 33), (32, 32), (33, 100), (100, 31), (1, 100), (32, 1), (100, 100)]
    src = _rand(g, sum(r * c for r, c in shapes) + 3 * len(shapes) + 5)
    tab, want, so, do = [], [], 2, 1
    for r, c in shapes:
        tab.append((so, r, c, do))
        want.append((do, src[so:so + r * c].view(r, c).t().contiguous().reshape(-1)))
        so += r * c + 3
        do += r * c + 2
    dst = _sentinel(do + 7)
    tiles = sum(((r + 31) // 32) * ((c + 31) // 32) for r, c in shapes)
    tab_d = torch.tensor(tab, dtype=torch.int32).to(_dev())
    src_d = src.to(_dev())
    L.call("sw_wide_transpose", _p(src_d), _p(tab_d), len(tab), tiles, _p(dst), L.stream())
    torch.cuda.synchronize()
    out, m = dst.cpu(), torch.zeros(dst.numel(), dtype=torch.bool)
    for o, v in want:
        assert torch.equal(out[o:o + v.numel()], v), "transpose at %d" % o
        m[o:o + v.numel()] = True
    _untouched(dst, m)


def _opimage_ref(M, R, K):
    """Image of Mx [R][K]: the float4 Mx[16 t + (l & 15)][16 j + 4 (l >> 4) ..] at ((t K/16 + j) 64 + l) 4."""
    img = torch.empty(R * K)
    KJ = K // 16
    for t in range(R // 16):
        for j in range(KJ):
            for l in range(64):
                o = ((t * KJ + j) * 64 + l) * 4
                img[o:o + 4] = M[16 * t + (l & 15), 16 * j + 4 * (l >> 4):16 * j + 4 * (l >> 4) + 4]
    return img


def test_wide_opimage_is_bit_exact():
    L = _L()
    g = torch.Generator().manual_seed(5)
    # (R, K, transposed, source row stride or 0): Mx [R][K] = M, a column block of a wider M, or M^T of M [K][R]
    entries = [(16, 16, 0, 0), (48, 32, 0, 0), (32, 48, 1, 0), (16, 64, 0, 80), (64, 16, 1, 0), (32, 32, 1, 40)]
    srcs, tab, want, so, do = [], [], [], 4, 0
    for R, K, tr, ld in entries:
        rows, cols = (K, R) if tr else (R, K)
        stride = ld or cols
        M = _rand(g, rows, stride)
        srcs.append((so, M))
        Mx = M[:, :cols].t() if tr else M[:, :cols]
        tab.append((so, R, K, do, tr, ld))
        want.append((do, _opimage_ref(Mx, R, K)))
        so += rows * stride + 4
        do += R * K
    src = torch.zeros(so)
    for o, M in srcs:
        src[o:o + M.numel()] = M.reshape(-1)
    dst = _sentinel(do + 8)
    tab_d = torch.tensor(tab, dtype=torch.int32).to(_dev())
    src_d = src.to(_dev())
    L.call("sw_wide_opimage", _p(src_d), _p(tab_d), len(tab), do // 4, _p(dst), L.stream())
    torch.cuda.synchronize()
    out = dst.cpu()
    for (o, v), e in zip(want, entries):
        assert torch.equal(out[o:o + v.numel()], v), "image of %s" % (e,)
    m = torch.zeros(dst.numel(), dtype=torch.bool)
    m[:do] = True
    _untouched(dst, m)


# ---- sw_wide_sum_steps, sw_wide_out_fwd / _bwd ----------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 16, 17])
def test_wide_sum_steps_and_out_layers_against_float64(B):
    L = _L()
    g = torch.Generator().manual_seed(B)
    dv = _Keep()
    tag = "B %d" % B
    # sum over T steps of an [R][C] block with strides
    T, C, in_ld, out_ld = 5, 50, 52, 51
    t_stride = B * in_ld + 3
    src = _rand(g, T * t_stride)
    out = _sentinel(B * out_ld + 2)
    L.call("sw_wide_sum_steps", _p(dv(src)), t_stride, in_ld, T, B, C, _p(out), out_ld, L.stream())
    ref = sum(src[t * t_stride:t * t_stride + B * in_ld].view(B, in_ld)[:, :C].double() for t in range(T))
    torch.cuda.synchronize()
    _close_out(_view(out, 0, B, out_ld)[:, :C], ref, "sum over steps", "2.out", tag)
    _untouched(out, _mask2d(out.numel(), 0, B, C, out_ld))
    # last decoder layer + integration
    D3, Tp, i = 100, 3, 1
    a3, W4, b4, p = _rand(g, B, D3), _rand(g, 2, D3, scale=0.1), _rand(g, 2), _rand(g, B, 2)
    pd, pred4, x4 = dv(p.clone()), _sentinel(B * 4 * Tp + 4), _sentinel(B * 4 + 4)
    L.call("sw_wide_out_fwd", _p(dv(a3)), D3, _p(dv(W4)), _p(dv(b4)), _p(pd), B, _p(pred4, 4 * i), 4 * Tp, _p(x4), L.stream())
    torch.cuda.synchronize()
    v = a3.double() @ W4.double().t() + b4.double()
    pn = p.double() + v
    row = torch.cat([pn, v], 1)
    _close_out(_view(pred4, 4 * i, B, 4 * Tp)[:, :4], row, "prediction row", "2.out", tag)
    _close_out(_view(x4, 0, B, 4), row, "x4 row", "2.out", tag)
    _close_out(pd, pn, "running position", "2.out", tag)
    _untouched(pred4, _mask2d(pred4.numel(), 4 * i, B, 4, 4 * Tp))
    _untouched(x4, _mask2d(x4.numel(), 0, B, 4, 4))
    # ... and its backward, dg NULL and given
    H4 = 4 * 96
    for have_dg in (False, True):
        dpred, dgv, WxT, dprun = _rand(g, B, Tp, 4), _rand(g, B, H4, scale=0.2), _rand(g, 4, H4, scale=0.2), _rand(g, B, 2)
        dpr, dvb, dz3 = dv(dprun.clone()), _sentinel(B * 4 + 4), _sentinel(B * D3 + 4)
        dpd = dv(dpred)
        L.call("sw_wide_out_bwd", _p(dpd, 4 * i), 4 * Tp, _p(dv(dgv)) if have_dg else None, _p(dv(WxT)), H4, _p(dpr), B, _p(dvb),
               _p(dv(W4)), D3, _p(dz3), L.stream())
        torch.cuda.synchronize()
        gsum = dpred[:, i].double() + (dgv.double() @ WxT.double().t() if have_dg else 0)
        dp = gsum[:, :2] + dprun.double()
        dvel = gsum[:, 2:] + dp
        _close_out(dpr, dp, "dp_run", "2.out", tag)
        _close_out(_view(dvb, 0, B, 4), torch.cat([dvel, torch.zeros(B, 2, dtype=torch.float64)], 1), "dv", "2.out", tag)
        _close_out(_view(dz3, 0, B, D3), dvel @ W4.double(), "dz3", "2.out", tag)
        _untouched(dvb, _mask2d(dvb.numel(), 0, B, 4, 4))
        _untouched(dz3, _mask2d(dz3.numel(), 0, B, D3, D3))


# ---- sw_wide_wgrad ----------------------------------------------------------------------------------------------------------
def _wgrad_call(problems):
    L = _L()
    arr = (ctypes.c_longlong * (10 * len(problems)))()
    for i, pr in enumerate(problems):
        for j, v in enumerate(pr):
            arr[10 * i + j] = 0 if v is None else int(v)
    ws = torch.empty(L.workspace_floats(L.WS_WGRAD, 1, 2, 1), device=_dev())
    rc = L.load().sw_wide_wgrad(ctypes.cast(arr, ctypes.c_void_p), len(problems), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    return rc


def _wgrad_problem(g, R, N, K, bias, ldd_extra, lda_extra, ldw_extra):
    ldd, lda, ldw = (N + 3) // 4 * 4 + ldd_extra, (K + 3) // 4 * 4 + lda_extra, K + ldw_extra
    delta, act = _rand(g, R, ldd, scale=0.5), _rand(g, R, lda, scale=0.5)
    dW = torch.full((N * ldw + 4,), float("nan"), device=_dev())
    db = torch.full((N + 4,), float("nan"), device=_dev()) if bias else None
    dd, ad = delta.to(_dev()), act.to(_dev())
    keep = (dd, ad)
    desc = (_p(dd), ldd, _p(ad), lda, R, N, K, _p(dW), ldw, _p(db))
    return desc, keep, (delta, act, dW, db, ldw)


def _wgrad_check(R, N, K, parts, tag):
    delta, act, dW, db, ldw = parts
    d64, a64 = delta.double()[:, :N], act.double()[:, :K]
    ref = d64.t() @ a64
    ref32 = delta[:, :N].t() @ act[:, :K]
    # bound: OUT_RT / OUT_AT; a long fp32 sum over R rows that does not fit gets 4 x the error of torch's fp32 CPU product
    scale = float(ref.abs().max())
    got = dW.cpu()[:N * ldw].view(N, ldw)
    assert bool(torch.isfinite(got[:, :K]).all()), "dW: elements left unwritten (%s)" % tag
    _close_out(got[:, :K], ref, "dW", "2.wgrad", tag)
    assert bool(torch.isnan(got[:, K:]).all()) and bool(torch.isnan(dW.cpu()[N * ldw:]).all()), "wrote outside dW (%s)" % tag
    if db is not None:
        _close_out(db.cpu()[:N], d64.sum(0), "db", "2.wgrad", tag)
        assert bool(torch.isnan(db.cpu()[N:]).all())
    return float((ref32.double() - ref).abs().max()) / max(scale, 1e-30)


# widths the grouped GEMM's lane vectors cannot split (a last <= 64-column block of 17 .. 63 columns that is neither a
# multiple of 4 nor an even number up to 32) used to be refused (SW_ESHAPE); sw_wide_wgrad now cuts such a block at its last
# multiple of 16
@pytest.mark.parametrize("R,N,K,bias,extra", [
    (1, 1, 1, True, 0), (5, 2, 3, False, 4), (127, 80, 4, True, 0), (129, 100, 60, True, 4), (5, 256, 64, False, 0),
    (127, 257, 65, True, 0), (129, 640, 640, True, 4), (24576, 80, 64, True, 0), (24576, 2, 640, False, 4), (129, 1, 640, True, 0),
    (127, 17, 60, True, 0), (5, 63, 65, True, 4), (129, 273, 3, False, 0)])
def test_wide_wgrad_against_float64(R, N, K, bias, extra):
    g = torch.Generator().manual_seed(R + N + K)
    desc, keep, parts = _wgrad_problem(g, R, N, K, bias, extra, extra, extra)
    assert _wgrad_call([desc]) == 0
    _wgrad_check(R, N, K, parts, "R %d N %d K %d" % (R, N, K))


def test_wide_wgrad_flushes_a_full_batch_and_continues():
    """40 problems of one 64-column block each (more than the 24 a batch holds) and one of 30 blocks in ONE call."""
    g = torch.Generator().manual_seed(9)
    shapes = [(33 + i, 16 + (i % 3) * 16, 4 * (1 + i % 16), i % 2 == 0) for i in range(40)] + [(65, 640, 640, True)]
    built = [_wgrad_problem(g, R, N, K, b, 0, 4, 0) for R, N, K, b in shapes]
    assert sum((K + 63) // 64 for _, _, K, _ in shapes) > 2 * 24
    assert _wgrad_call([b[0] for b in built]) == 0
    for (R, N, K, _), b in zip(shapes, built):
        _wgrad_check(R, N, K, b[2], "flush: R %d N %d K %d" % (R, N, K))


def test_wide_wgrad_refuses_what_it_cannot_run():
    g = torch.Generator().manual_seed(10)
    desc, keep, parts = _wgrad_problem(g, 8, 4, 4, True, 0, 0, 0)
    bad = list(desc)
    bad[1] = 6                                # a delta row stride that is no multiple of 4
    assert _wgrad_call([tuple(bad)]) == -2    # SW_ESHAPE
    bad = list(desc)
    bad[4] = 0                                # no rows
    assert _wgrad_call([tuple(bad)]) == -1    # SW_EARG
    assert bool(torch.isnan(parts[2]).all()) and bool(torch.isnan(parts[3]).all())


# ---- sw_wide_lstm_seq_fwd / _bwd, sw_wide_dec_loop_fwd / _bwd: on their own, outside the trainer ----------------------------------
def _images(src_flat, entries):
    """sw_wide_opimage of entries (source offset, R, K, transposed, source row stride or 0) -> list of image tensors."""
    L = _L()
    tab, off = [], 0
    for so, R, K, tr, ld in entries:
        tab.append((so, R, K, off, tr, ld))
        off += R * K
    dst = torch.zeros(off, device=_dev())
    tab_d = torch.tensor(tab, dtype=torch.int32).to(_dev())
    L.call("sw_wide_opimage", _p(src_flat), _p(tab_d), len(tab), off // 4, _p(dst), L.stream())
    return [dst[t[3]:t[3] + t[1] * t[2]] for t in tab]


def _cell_bwd64(dh, dc, gates, c, c_prev):
    H = c.shape[1]
    gi, gf, gg, go = (gates[:, k * H:(k + 1) * H] for k in range(4))
    tc = torch.tanh(c)
    dct = dh * go * (1 - tc * tc) + dc
    return torch.cat([dct * gg * gi * (1 - gi), dct * c_prev * gf * (1 - gf), dct * gi * (1 - gg * gg), dh * tc * go * (1 - go)], 1), dct * gf


@pytest.mark.parametrize("H,T,B,null", [(64, 1, 1, 0), (64, 2, 17, 7), (64, 8, 33, 2), (64, 8, 16, 5), (128, 1, 17, 3), (128, 2, 16, 4),
                                        (128, 8, 1, 6), (128, 8, 33, 0), (128, 2, 33, 1), (64, 2, 16, 0)])
def test_wide_lstm_sequence_kernels_against_float64(H, T, B, null):
    """null: bit 0 dg_init, bit 1 dc_init, bit 2 dh_ext2 NULL; the forward's second copy of h_T (stride 2.5 H) and its
    second bias are given where bit 0 is clear."""
    L = _L()
    assert L.load().sw_wide_lstm_seq_supported(H) == 1 and L.load().sw_wide_lstm_seq_supported(96) == 0
    g = torch.Generator().manual_seed(H + 10 * T + B)
    dv = _Keep()
    x4, Wx, b1, b2 = _rand(g, T, B, 4), _rand(g, 4 * H, 4, scale=0.5), _rand(g, 4 * H, scale=0.1), _rand(g, 4 * H, scale=0.1)
    Whh, h0 = _rand(g, 4 * H, H, scale=H ** -0.5), _rand(g, B, H, scale=0.5)
    second = not null & 1
    whh_d = dv(Whh)
    img, imgT = _images(whh_d, [(0, 4 * H, H, 0, 0), (0, H, 4 * H, 1, 0)])
    h2_ld = 2 * H + H // 2
    gates, cs, hs = _sentinel(T * B * 4 * H + 4), _sentinel(T * B * H + 4), _sentinel((T + 1) * B * H + 4)
    hs[:B * H] = dv(h0).reshape(-1)
    hl2 = _sentinel(B * h2_ld) if second else None
    L.call("sw_wide_lstm_seq_fwd", _p(dv(x4)), _p(dv(Wx)), _p(dv(b1)), _p(dv(b2)) if second else None, _p(img), B, H, T, _p(gates), _p(cs),
           _p(hs), _p(hl2), h2_ld if second else 0, L.stream())
    torch.cuda.synchronize()
    d = lambda t: t.double()
    h, c, G64, C64, H64 = d(h0), None, [], [], []
    for t in range(T):
        gt, c, h = _lstm64(d(x4[t]), h, c, d(Wx), d(b1), d(b2) if second else None, d(Whh))
        G64.append(gt), C64.append(c), H64.append(h)
    tag = "H %d T %d B %d null %d" % (H, T, B, null)
    _close_out(_view(gates, 0, T * B, 4 * H), torch.cat(G64), "gates", "2.seq", tag)
    _close_out(_view(cs, 0, T * B, H), torch.cat(C64), "cs", "2.seq", tag)
    _close_out(_view(hs, B * H, T * B, H), torch.cat(H64), "hs", "2.seq", tag)
    assert torch.equal(hs[:B * H].cpu(), h0.reshape(-1)), "slab 0 of hs is an input"
    for buf, n in ((gates, T * B * 4 * H), (cs, T * B * H), (hs, (T + 1) * B * H)):
        _untouched(buf, torch.arange(buf.numel()) < n)
    if second:
        _close_out(_view(hl2, 0, B, h2_ld)[:, :H], H64[-1], "second copy of h_T", "2.seq", tag)
        _untouched(hl2, _mask2d(hl2.numel(), 0, B, H, h2_ld))
    # backward on the rows the forward left (its exact fp32 values are the float64 side's inputs)
    gsv, csv = _view(gates, 0, T * B, 4 * H).cpu().view(T, B, 4 * H), _view(cs, 0, T * B, H).cpu().view(T, B, H)
    dhe_ld, dhe2_ld = H + 4, h2_ld
    dh1, dh2 = _rand(g, B, H), (None if null & 4 else _rand(g, B, H))
    dgi, dci = (None if null & 1 else _rand(g, B, 4 * H, scale=0.5)), (None if null & 2 else _rand(g, B, H))

    def padded(t, ld):
        if t is None:
            return None
        o = torch.zeros(t.shape[0], ld)
        o[:, :t.shape[1]] = t
        return dv(o)

    dg = _sentinel(T * B * 4 * H + 4)
    gd, cd = gates[:T * B * 4 * H].clone(), cs[:T * B * H].clone()
    L.call("sw_wide_lstm_seq_bwd", _p(padded(dh1, dhe_ld)), dhe_ld, _p(padded(dh2, dhe2_ld)), dhe2_ld, _p(dv(dgi)), _p(dv(dci)), _p(imgT),
           _p(gd), _p(cd), B, H, T, _p(dg), L.stream())
    torch.cuda.synchronize()
    W = d(Whh)
    dh = d(dh1) + (d(dh2) if dh2 is not None else 0) + (d(dgi) @ W if dgi is not None else 0)
    dc = d(dci) if dci is not None else torch.zeros(B, H, dtype=torch.float64)
    ref = [None] * T
    for t in range(T - 1, -1, -1):
        cp = d(csv[t - 1]) if t > 0 else torch.zeros(B, H, dtype=torch.float64)
        ref[t], dc = _cell_bwd64(dh, dc, d(gsv[t]), d(csv[t]), cp)
        dh = ref[t] @ W
    _close_out(_view(dg, 0, T * B, 4 * H), torch.cat(ref), "dgates", "2.seq", tag)
    _untouched(dg, torch.arange(dg.numel()) < T * B * 4 * H)


def _lrelu64(x):
    return torch.where(x > 0, x, 0.2 * x)


@pytest.mark.parametrize("B,Tp,To", [(1, 1, 2), (16, 2, 8), (17, 5, 2), (17, 1, 8), (1, 5, 8), (16, 5, 2), (17, 2, 2)])
def test_wide_decode_loop_kernels_against_float64(B, Tp, To):
    L = _L()
    H, D1, D2, D3 = 128, 320, 160, 80
    assert L.load().sw_wide_dec_loop_supported(H) == 1 and L.load().sw_wide_dec_loop_supported(256) == 0
    Ta = To + Tp - 1
    g = torch.Generator().manual_seed(100 * B + 10 * Tp + To)
    dv = _Keep()
    d = lambda t: t.double()
    W1, W2, W3, W4 = _rand(g, D1, D1, scale=D1 ** -0.5), _rand(g, D2, D1, scale=D1 ** -0.5), _rand(g, D3, D2, scale=D2 ** -0.5), _rand(g, 2, D3, scale=0.1)
    b2, b3, b4 = _rand(g, D2, scale=0.1), _rand(g, D3, scale=0.1), _rand(g, 2, scale=0.1)
    Whh, Wx, bx1, bx2 = _rand(g, 4 * H, H, scale=H ** -0.5), _rand(g, 4 * H, 4, scale=0.5), _rand(g, 4 * H, scale=0.1), _rand(g, 4 * H, scale=0.1)
    u, p0 = _rand(g, B, D1, scale=0.5), _rand(g, B, 2)
    hT, cT = _rand(g, B, H, scale=0.5), _rand(g, B, H, scale=0.5)
    # one packed source buffer for the images: W1 | W2 | W3 | Whh | WxT padded to 16 rows
    mats = [W1, W2, W3, Whh, torch.cat([Wx.t(), torch.zeros(12, 4 * H)])]
    offs = np.cumsum([0] + [m.numel() for m in mats]).tolist()
    flat = dv(torch.cat([m.reshape(-1) for m in mats]))
    w1h, w2i, w3i, whi, whhT, w3T, w2T, w1hT, wxT = _images(flat, [
        (offs[0], D1, H, 0, D1), (offs[1], D2, D1, 0, 0), (offs[2], D3, D2, 0, 0), (offs[3], 4 * H, H, 0, 0),
        (offs[3], H, 4 * H, 1, 0), (offs[2], D2, D3, 1, 0), (offs[1], D1, D2, 1, 0), (offs[0], H, D1, 1, D1), (offs[4], 16, 4 * H, 0, 0)])
    p0_ld = 2 * To
    p0d = torch.zeros(B, p0_ld)
    p0d[:, :2] = p0
    a1, a2, a3 = _sentinel(Tp * B * D1 + 4), _sentinel(Tp * B * D2 + 4), _sentinel(Tp * B * D3 + 4)
    pred4, x4 = _sentinel(B * Tp * 4 + 4), _sentinel((Ta + 1) * B * 4 + 4)
    gates, cs, hs, cat = _sentinel(Ta * B * 4 * H + 4), _sentinel(Ta * B * H + 4), _sentinel((Ta + 1) * B * H + 4), _sentinel(Tp * B * D1 + 4)
    cs[(To - 1) * B * H:To * B * H] = dv(cT).reshape(-1)
    hs[To * B * H:(To + 1) * B * H] = dv(hT).reshape(-1)
    L.call("sw_wide_dec_loop_fwd", _p(w1h), _p(w2i), _p(w3i), _p(whi), _p(dv(u)), _p(dv(b2)), _p(dv(b3)), _p(dv(W4)), _p(dv(b4)), _p(dv(Wx)),
           _p(dv(bx1)), _p(dv(bx2)), _p(dv(p0d)), p0_ld, _p(a1), _p(a2), _p(a3), _p(pred4), _p(x4), _p(gates), _p(cs), _p(hs), _p(cat),
           B, H, To, Tp, L.stream())
    torch.cuda.synchronize()
    h, c, p = d(hT), d(cT), d(p0)
    A1, A2, A3, P4, G64, C64, H64 = [], [], [], [], [], [], []
    for i in range(Tp):
        x1 = _lrelu64(h @ d(W1)[:, :H].t() + d(u))
        x2 = _lrelu64(x1 @ d(W2).t() + d(b2))
        x3 = x2 @ d(W3).t() + d(b3)
        v = x3 @ d(W4).t() + d(b4)
        p = p + v
        A1.append(x1), A2.append(x2), A3.append(x3), P4.append(torch.cat([p, v], 1))
        if i + 1 < Tp:
            gt, c, h = _lstm64(P4[-1], h, c, d(Wx), d(bx1), d(bx2), d(Whh))
            G64.append(gt), C64.append(c), H64.append(h)
    tag = "B %d Tp %d To %d" % (B, Tp, To)
    gr = "2.decloop"
    _close_out(_view(a1, 0, Tp * B, D1), torch.cat(A1), "a1", gr, tag)
    _close_out(_view(a2, 0, Tp * B, D2), torch.cat(A2), "a2", gr, tag)
    _close_out(_view(a3, 0, Tp * B, D3), torch.cat(A3), "a3", gr, tag)
    _close_out(_view(pred4, 0, B, Tp * 4).view(B, Tp, 4), torch.stack(P4, 1), "pred4", gr, tag)
    _close_out(_view(x4, To * B * 4, Tp * B, 4), torch.cat(P4), "x4 rows To..", gr, tag)
    written = {"a1": (a1, [(0, Tp * B * D1)]), "a2": (a2, [(0, Tp * B * D2)]), "a3": (a3, [(0, Tp * B * D3)]),
               "pred4": (pred4, [(0, B * Tp * 4)]), "x4": (x4, [(To * B * 4, (To + Tp) * B * 4)]),
               "gates": (gates, [(To * B * 4 * H, Ta * B * 4 * H)]), "cs": (cs, [((To - 1) * B * H, Ta * B * H)]),
               "hs": (hs, [(To * B * H, (Ta + 1) * B * H)])}
    if Tp > 1:
        n = Tp - 1
        _close_out(_view(gates, To * B * 4 * H, n * B, 4 * H), torch.cat(G64), "gates rows To..", gr, tag)
        _close_out(_view(cs, To * B * H, n * B, H), torch.cat(C64), "cs rows To..", gr, tag)
        _close_out(_view(hs, (To + 1) * B * H, n * B, H), torch.cat(H64), "hs rows To + 1..", gr, tag)
        catv = _view(cat, 0, Tp * B, D1).view(Tp, B, D1)
        _close_out(catv[1:, :, :H].reshape(n * B, H), torch.cat(H64), "h into cat", gr, tag)
    for name, (buf, spans) in written.items():
        m = torch.zeros(buf.numel(), dtype=torch.bool)
        for lo, hi in spans:
            m[lo:hi] = True
        _untouched(buf, m)
    m = torch.zeros(cat.numel(), dtype=torch.bool)
    for i in range(1, Tp):
        m |= _mask2d(cat.numel(), i * B * D1, B, H, D1)
    _untouched(cat, m)
    # ---- backward on the rows the forward left ----
    a1v, a2v = _view(a1, 0, Tp * B, D1).cpu().view(Tp, B, D1), _view(a2, 0, Tp * B, D2).cpu().view(Tp, B, D2)
    gsv = torch.zeros(Ta, B, 4 * H)
    csv = torch.zeros(Ta, B, H)
    csv[To - 1] = cT
    if Tp > 1:
        gsv[To:] = _view(gates, To * B * 4 * H, (Tp - 1) * B, 4 * H).cpu().view(Tp - 1, B, 4 * H)
        csv[To:] = _view(cs, To * B * H, (Tp - 1) * B, H).cpu().view(Tp - 1, B, H)
    dpred = _rand(g, B, Tp, 4, scale=0.5)
    dg, dvb = _sentinel(Ta * B * 4 * H + 4), _sentinel(Tp * B * 4 + 4)
    dz3, dz2, dz1 = _sentinel(Tp * B * D3 + 4), _sentinel(Tp * B * D2 + 4), _sentinel(Tp * B * D1 + 4)
    dhc, dco = _sentinel(B * H + 4), _sentinel(B * H + 4)
    L.call("sw_wide_dec_loop_bwd", _p(whhT), _p(w3T), _p(w2T), _p(w1hT), _p(wxT), _p(dv(W4)), _p(dv(dpred)), _p(dv(a1v)), _p(dv(a2v)),
           _p(dv(gsv)), _p(dv(csv)), _p(dg), _p(dvb), _p(dz3), _p(dz2), _p(dz1), _p(dhc), _p(dco), B, H, To, Tp, L.stream())
    torch.cuda.synchronize()
    dprun = torch.zeros(B, 2, dtype=torch.float64)
    dc = torch.zeros(B, H, dtype=torch.float64)
    dhcat, DG, DV, DZ3, DZ2, DZ1 = None, {}, [None] * Tp, [None] * Tp, [None] * Tp, [None] * Tp
    for i in range(Tp - 1, -1, -1):
        t_in = To + i
        gsum = d(dpred[:, i])
        if i + 1 < Tp:
            dh = dhcat + (DG[t_in + 1] @ d(Whh) if t_in + 1 < Ta else 0)
            DG[t_in], dc = _cell_bwd64(dh, dc, d(gsv[t_in]), d(csv[t_in]), d(csv[t_in - 1]))
            gsum = gsum + DG[t_in] @ d(Wx)
        dp = gsum[:, :2] + dprun
        dvel = gsum[:, 2:] + dp
        dprun = dp
        DV[i] = torch.cat([dvel, torch.zeros(B, 2, dtype=torch.float64)], 1)
        DZ3[i] = dvel @ d(W4)
        DZ2[i] = (DZ3[i] @ d(W3)) * torch.where(d(a2v[i]) > 0, 1.0, 0.2)
        DZ1[i] = (DZ2[i] @ d(W2)) * torch.where(d(a1v[i]) > 0, 1.0, 0.2)
        dhcat = DZ1[i] @ d(W1)[:, :H]
    _close_out(_view(dvb, 0, Tp * B, 4), torch.cat(DV), "dv", gr, tag)
    _close_out(_view(dz3, 0, Tp * B, D3), torch.cat(DZ3), "dz3", gr, tag)
    _close_out(_view(dz2, 0, Tp * B, D2), torch.cat(DZ2), "dz2", gr, tag)
    _close_out(_view(dz1, 0, Tp * B, D1), torch.cat(DZ1), "dz1", gr, tag)
    _close_out(_view(dhc, 0, B, H), dhcat, "dhcat_out", gr, tag)
    for buf, n in ((dvb, Tp * B * 4), (dz3, Tp * B * D3), (dz2, Tp * B * D2), (dz1, Tp * B * D1), (dhc, B * H)):
        _untouched(buf, torch.arange(buf.numel()) < n)
    m = torch.zeros(dg.numel(), dtype=torch.bool)
    if Tp > 1:
        _close_out(_view(dg, To * B * 4 * H, (Tp - 1) * B, 4 * H), torch.cat([DG[To + i] for i in range(Tp - 1)]), "dgates rows To..", gr, tag)
        m[To * B * 4 * H:Ta * B * 4 * H] = True
    _untouched(dg, m)
    _close_out(_view(dco, 0, B, H), dc, "dc_out", gr, tag)          # (Tp = 1: no re-fed step, zeros)
    _untouched(dco, torch.arange(dco.numel()) < B * H)


# ---- sw_wide_disc_heads_fwd / _bwd ----------------------------------------------------------------------------------------------
def test_wide_disc_heads_limits():
    ok = _L().load().sw_wide_disc_heads_supported
    assert ok(256, 48, 2) == 1 and ok(288, 48, 2) == 0          # WH_MAXH
    assert ok(32, 48, 2) == 1 and ok(16, 48, 2) == 0 and ok(48, 48, 2) == 0
    assert ok(128, 16, 2) == 1 and ok(128, 8, 2) == 0 and ok(128, 24, 2) == 0 and ok(128, 40, 2) == 0
    assert ok(128, 48, 16) == 1 and ok(128, 48, 17) == 0 and ok(128, 48, 1) == 1 and ok(128, 48, 0) == 0


def _heads64(D, hT, px, nb, B):
    """float64 forward of D's heads on hT [B][H] and px [nb B][K4], every pre-activation kept: dict of tensors with a graph."""
    of, pe, cl, la = D.obsv_encoder_fc, D.pred_encoder, D.classifier, D.latent_decoder
    lin = lambda m, x: x @ m.weight.t() + m.bias
    t = {}
    t["o1p"] = lin(of[0], hT)
    t["oc"] = lin(of[2], _lrelu64(t["o1p"]))
    t["q1p"] = lin(pe[0], px)
    t["pc"] = lin(pe[2], _lrelu64(t["q1p"]))
    t["both"] = torch.cat([t["oc"].repeat(nb, 1), t["pc"]], 1)
    t["both"].retain_grad()
    t["c1p"] = lin(cl[0], t["both"])
    t["l1p"] = lin(la[0], t["both"])
    t["label"] = lin(cl[2], _lrelu64(t["c1p"]))
    t["code"] = lin(la[2], _lrelu64(t["l1p"]))
    return t


@pytest.mark.parametrize("H,K4,nl,nb,B,need_obs,want_dpred,loss", [
    (32, 16, 2, 2, 17, True, False, 1), (32, 48, 16, 1, 1, False, True, 0), (96, 48, 3, 2, 16, True, True, 0),
    (96, 16, 2, 1, 17, False, True, 1), (256, 48, 2, 2, 17, True, False, 1), (256, 16, 16, 1, 16, True, True, 0),
    (256, 48, 3, 2, 1, False, False, 0), (96, 48, 16, 2, 17, False, True, 1)])
def test_wide_disc_heads_against_float64(H, K4, nl, nb, B, need_obs, want_dpred, loss):
    from socialways_amd.wide import WideTrainer
    from _ref64 import SEEDS
    L = _L()
    torch.manual_seed(H + K4 + nl)
    tr = WideTrainer(K4 // 4, hidden_size=H, n_latent_codes=nl, device="cuda:0", use_graph=False)
    assert tr.heads
    with _f64():
        Dref = O.Discriminator(K4 // 4, H, nl)
    Dref.double().load_state_dict({k: v.detach().cpu().double() for k, v in tr.D.state_dict().items()})
    H2, nlp, To = H // 2, (nl + 3) // 4 * 4, 2
    gl, gc = 2.0 / B, W_INFO * 2.0 / (nl * B)
    t_idx = (0, 1) if nb == 2 else (1, 1)
    for seed in SEEDS:          # (Leaky)ReLU kinks: the first seed whose float64 pre-activations all stay MARGIN away from 0
        g = torch.Generator().manual_seed(seed)
        hT, px, z = _rand(g, B, H, scale=0.5), _rand(g, 2 * B, K4, scale=0.3), torch.rand(B, H2, generator=g)
        dlab, dcod = _rand(g, nb * B, 1), _rand(g, nb * B, nl)
        h64, p64 = hT.double().requires_grad_(), px[:nb * B].double().requires_grad_()
        with _f64():
            t = _heads64(Dref, h64, p64, nb, B)
        if min(float(t[k].detach().abs().min()) for k in ("o1p", "q1p", "c1p", "l1p")) > MARGIN:
            break
    else:
        raise AssertionError("no seed keeps the kink inputs away from 0")
    tag = "H %d K4 %d nl %d nb %d B %d seed %d" % (H, K4, nl, nb, B, seed)
    w = tr._buffers(B, To, 0)
    w["d_hs"][To].copy_(hT)
    w["px"].copy_(px)
    w["noise"].copy_(z)
    w["scal"][:2].copy_(torch.tensor(TARGETS))
    outs = ("o1", "q1", "both", "c1", "l1", "label", "code", "dlab", "dcod")
    for k in outs:
        w[k].fill_(SENT)
    part = torch.full(((B + 15) // 16, 3), SENT, device=_dev())
    tr._images(tr._dI_args)
    L.call("sw_wide_disc_heads_fwd", tr._heads_args(w, B, To, nb, False, False, False, (t_idx[0], t_idx[1], gl, gc, part) if loss else None),
           L.stream())
    torch.cuda.synchronize()
    R, gr = nb * B, "2.heads"
    sent_bits = torch.tensor(SENT).view(torch.int32)
    rows_untouched = lambda buf, r0: bool((buf[r0:].cpu().view(torch.int32) == sent_bits).all())
    ref = {"o1": _lrelu64(t["o1p"]), "q1": _lrelu64(t["q1p"]), "both": t["both"], "c1": _lrelu64(t["c1p"]), "l1": _lrelu64(t["l1p"]),
           "label": t["label"], "code": t["code"]}
    for k, v in ref.items():
        rows = B if k == "o1" else R
        _close_out(w[k][:rows], v, k, gr, tag)
        assert rows_untouched(w[k], rows), "%s: rows past %d written (%s)" % (k, rows, tag)
    t0, t1 = (float(torch.tensor(TARGETS[i], dtype=torch.float32)) for i in t_idx)
    if loss:
        lab, code, z2 = t["label"].detach(), t["code"].detach(), z.double()[:, :nl]
        dl64 = torch.cat([gl * (lab[:B] - t0)] + ([gl * (lab[B:] - t1)] if nb == 2 else []))
        dc64 = torch.cat([gc * (code[:B] - z2)] + ([torch.zeros(B, nl, dtype=torch.float64)] if nb == 2 else []))
        _close_out(w["dlab"][:R, :1], dl64, "dlab", gr, tag)
        _close_out(w["dcod"][:R, :nl], dc64, "dcod", gr, tag)
        assert bool((w["dlab"][:, 1:].cpu().view(torch.int32) == sent_bits).all()) and rows_untouched(w["dlab"], R)
        assert bool((w["dcod"][:, nl:].cpu().view(torch.int32) == sent_bits).all()) and rows_untouched(w["dcod"], R)
        sq = torch.stack([(lab[:B] - t0) ** 2, ((code[:B] - z2) ** 2).sum(1, keepdim=True),
                          (lab[B:] - t1) ** 2 if nb == 2 else torch.zeros(B, 1, dtype=torch.float64)], 1).view(B, 3)
        tiles = (B + 15) // 16
        pad = torch.zeros(tiles * 16, 3, dtype=torch.float64)
        pad[:B] = sq
        _close_out(part, pad.view(tiles, 16, 3).sum(1), "per-tile loss sums", gr, tag)
        dlab, dcod = dl64.float(), dc64.float()          # the backward's inputs are the rows the forward left
        dlab_d, dcod_d = w["dlab"][:R, :1].cpu(), w["dcod"][:R, :nl].cpu()
    else:
        assert all(rows_untouched(w[k], 0) for k in ("dlab", "dcod")) and rows_untouched(part, 0)
        w["dlab"].zero_()
        w["dcod"].zero_()
        w["dlab"][:R, :1] = dlab.to(_dev())
        w["dcod"][:R, :nl] = dcod.to(_dev())
        dlab_d, dcod_d = dlab, dcod
    deltas = ("dc1", "dl1", "dboth", "dq1", "docode", "do1", "d_dhT", "dpx")
    for k in deltas:
        w[k].fill_(SENT)
    L.call("sw_wide_disc_heads_bwd", tr._heads_args(w, B, 0, nb, True, need_obs, want_dpred), L.stream())
    torch.cuda.synchronize()
    obj = (t["label"] * dlab_d.double()).sum() + (t["code"] * dcod_d.double()).sum()
    gs = torch.autograd.grad(obj, [t["c1p"], t["l1p"], t["both"], t["q1p"], t["oc"], t["o1p"], h64, p64])
    want = dict(zip(deltas, gs))
    want["dpx"] = want["dpx"][:B]
    for k in ("dc1", "dl1", "dboth", "dq1"):
        _close_out(w[k][:R], want[k], k, gr, tag)
        assert rows_untouched(w[k], R), k
    for k in ("docode", "do1", "d_dhT"):
        if need_obs:
            _close_out(w[k][:B], want[k], k, gr, tag)
            assert rows_untouched(w[k], B), k
        else:
            assert rows_untouched(w[k], 0), "%s written without need_obs" % k
    if want_dpred:
        _close_out(w["dpx"], want["dpx"], "dpx", gr, tag)
    else:
        assert rows_untouched(w["dpx"], 0), "dpx written without want_dpred"


# ---- the generic pieces both wider paths share -----------------------------------------------------------------------------------
_SCENES = [1, 2, 17, 64]


@pytest.mark.parametrize("F", [96, 128])
def test_pair_features_and_attention_pairs_against_float64(F):
    from socialways_amd.model import _scene_index
    L = _L()
    H = F
    B, sb = int(np.sum(_SCENES)), scene_rows(_SCENES)
    sc = _scene_index(sb, B, _dev())
    P = sc.P
    assert P == 4 + 17 * 17 + 64 * 64
    g = torch.Generator().manual_seed(F)
    dv = _Keep()
    last4 = torch.cat([_rand(g, B, 2), _rand(g, B, 2, scale=0.1)], 1)
    feat = _sentinel(P * 4 + 4)
    L.call("sw_pair_features", _p(dv(last4)), _p(sc.scene_off), _p(sc.pair_off), sc.S, _p(feat), L.stream())
    torch.cuda.synchronize()
    poff = sc.pair_off.cpu().tolist()
    l64 = last4.double()
    f64 = []
    for s, (s0, s1) in enumerate(sb):
        n = int(s1 - s0)
        if n > 1:
            st = l64[s0:s1]
            f64.append(O.pair_features(st[:, None, :], st[None, :, :]).reshape(n * n, 3))
    f64 = torch.cat(f64)
    gr, tag = "2.generic", "F %d" % F
    fv = _view(feat, 0, P, 4)
    _close_out(fv[:, :3], f64, "pair features", gr, tag)
    assert not bool(fv[:, 3].any()), "the fourth column is zero"
    _untouched(feat, torch.arange(feat.numel()) < P * 4)
    # attention on pair rows: f [P][F], wh [B][F], h [B][H]
    f, wh, h, dS = _rand(g, P, F, scale=0.3), _rand(g, B, F, scale=0.3), _rand(g, B, H, scale=0.5), _rand(g, B, H)
    attn, S = _sentinel(P + 4), _sentinel(B * H + 4)
    fd, whd, hd = dv(f), dv(wh), dv(h)
    L.call("sw_attn_pairs_fwd", _p(fd), _p(whd), _p(hd), _p(sc.scene_off), _p(sc.pair_off), sc.S, B, F, H, _p(attn), _p(S), L.stream())
    torch.cuda.synchronize()
    f6, w6, h6 = f.double().requires_grad_(), wh.double().requires_grad_(), h.double().requires_grad_()
    S64, A64 = torch.zeros(B, H, dtype=torch.float64), []
    for s, (s0, s1) in enumerate(sb):
        n = int(s1 - s0)
        if n > 1:
            sig = (f6[poff[s]:poff[s] + n * n].view(n, n, F) * w6[s0:s1][None]).sum(-1).masked_fill(torch.eye(n, dtype=torch.bool), -1000.0)
            a = torch.softmax(sig, 1)
            A64.append(a.reshape(-1))
            S64 = S64.index_put((torch.arange(s0, s1),), a @ h6[s0:s1])
    _close_out(_view(attn, 0, 1, P)[0], torch.cat(A64), "attention weights", gr, tag)
    _close_out(_view(S, 0, B, H), S64, "pooled states", gr, tag)
    _untouched(attn, torch.arange(attn.numel()) < P)
    _untouched(S, torch.arange(S.numel()) < B * H)
    (S64 * dS.double()).sum().backward()
    dsig, df, dwh, dh = _sentinel(P + 4), _sentinel(P * F + 4), _sentinel(B * F + 4), _sentinel(B * H + 4)
    L.call("sw_attn_pairs_bwd", _p(fd), _p(whd), _p(hd), _p(attn), _p(dv(dS)), _p(sc.scene_off), _p(sc.pair_off), sc.S, B, F, H, _p(dsig),
           _p(df), _p(dwh), _p(dh), L.stream())
    torch.cuda.synchronize()
    _close_out(_view(df, 0, P, F), f6.grad, "df", gr, tag)
    _close_out(_view(dwh, 0, B, F), w6.grad, "dwh", gr, tag)
    _close_out(_view(dh, 0, B, H), h6.grad, "dh", gr, tag)
    for buf, n in ((df, P * F), (dwh, B * F), (dh, B * H), (dsig, P)):
        _untouched(buf, torch.arange(buf.numel()) < n)


@pytest.mark.parametrize("H", [96, 128])
@pytest.mark.parametrize("B", _SCENES)
def test_lstm_point_act_and_sqdiff_against_float64(H, B):
    L = _L()
    g = torch.Generator().manual_seed(H + B)
    dv = _Keep()
    gr, tag = "2.generic", "H %d B %d" % (H, B)
    d = lambda t: t.double()
    pre, cp = _rand(g, B, 4 * H), _rand(g, B, H, scale=0.7)
    for have_c in (True, False):
        gates, c, h = _sentinel(B * 4 * H + 4), _sentinel(B * H + 4), _sentinel(B * H + 4)
        L.call("sw_lstm_point_fwd", _p(dv(pre)), _p(dv(cp)) if have_c else None, B, H, _p(gates), _p(c), _p(h), L.stream())
        torch.cuda.synchronize()
        p6 = d(pre)
        G = torch.cat([torch.sigmoid(p6[:, :H]), torch.sigmoid(p6[:, H:2 * H]), torch.tanh(p6[:, 2 * H:3 * H]), torch.sigmoid(p6[:, 3 * H:])], 1)
        cn = G[:, H:2 * H] * (d(cp) if have_c else 0) + G[:, :H] * G[:, 2 * H:3 * H]
        _close_out(_view(gates, 0, B, 4 * H), G, "gates", gr, tag)
        _close_out(_view(c, 0, B, H), cn, "c", gr, tag)
        _close_out(_view(h, 0, B, H), G[:, 3 * H:] * torch.tanh(cn), "h", gr, tag)
        for buf, n in ((gates, B * 4 * H), (c, B * H), (h, B * H)):
            _untouched(buf, torch.arange(buf.numel()) < n)
        # backward from the rows the forward left; dh / dc each NULL and given
        gs, cs_ = _view(gates, 0, B, 4 * H).cpu(), _view(c, 0, B, H).cpu()
        for null in range(3):          # 0: both given, 1: dh NULL, 2: dc NULL
            dh, dc = (None if null == 1 else _rand(g, B, H)), (None if null == 2 else _rand(g, B, H))
            dpre, dcp = _sentinel(B * 4 * H + 4), _sentinel(B * H + 4)
            L.call("sw_lstm_point_bwd", _p(dv(gs)), _p(dv(cs_)), _p(dv(cp)) if have_c else None, _p(dv(dh)), _p(dv(dc)), B, H, _p(dpre),
                   _p(dcp), L.stream())
            torch.cuda.synchronize()
            z = torch.zeros(B, H, dtype=torch.float64)
            want, wcp = _cell_bwd64(d(dh) if dh is not None else z, d(dc) if dc is not None else z, d(gs), d(cs_), d(cp) if have_c else z)
            _close_out(_view(dpre, 0, B, 4 * H), want, "dpre", gr, tag)
            _close_out(_view(dcp, 0, B, H), wcp, "dc_prev", gr, tag)
            _untouched(dpre, torch.arange(dpre.numel()) < B * 4 * H)
            _untouched(dcp, torch.arange(dcp.numel()) < B * H)
    # activations: kind 0 ReLU, 1 LeakyReLU(0.2); the backward takes the activated values
    n = B * H + 3
    x, dy = _rand(g, n), _rand(g, n)
    for kind in (0, 1):
        y, dx = _sentinel(n + 4), _sentinel(n + 4)
        L.call("sw_act_fwd", _p(dv(x)), n, kind, _p(y), L.stream())
        torch.cuda.synchronize()
        y64 = d(x).clamp_min(0) if kind == 0 else _lrelu64(d(x))
        _close_out(y[:n], y64, "act", gr, tag)
        yv = y[:n].cpu()
        L.call("sw_act_bwd", _p(dv(yv)), _p(dv(dy)), n, kind, _p(dx), L.stream())
        torch.cuda.synchronize()
        slope = 0.0 if kind == 0 else 0.2
        _close_out(dx[:n], d(dy) * torch.where(d(yv) > 0, 1.0, slope), "act backward", gr, tag)
        _untouched(y, torch.arange(n + 4) < n)
        _untouched(dx, torch.arange(n + 4) < n)
    # squared differences: against a second block, against a device scalar; sum and scaled difference each NULL and given
    C, lda, ldb, ldda = 5, 8, H // 2, 7
    a, b2, tg = _rand(g, B, lda), _rand(g, B, ldb), torch.tensor(TARGETS)
    for against_b in (True, False):
        for want_sum, want_da in ((True, True), (True, False), (False, True)):
            out, da = _sentinel(4), _sentinel(B * ldda + 4)
            L.call("sw_sqdiff", _p(dv(a)), lda, _p(dv(b2)) if against_b else None, ldb if against_b else 0, None if against_b else _p(dv(tg)), 1,
                   B, C, 0.25, _p(out) if want_sum else None, _p(da) if want_da else None, ldda, L.stream())
            torch.cuda.synchronize()
            diff = d(a)[:, :C] - (d(b2)[:, :C] if against_b else float(tg[1]))
            if want_sum:
                _close_out(out[:1], (diff ** 2).sum().reshape(1), "sum of squares", gr, tag)
                _untouched(out, torch.arange(4) < 1)
            if want_da:
                _close_out(_view(da, 0, B, ldda)[:, :C], 0.25 * diff, "scaled difference", gr, tag)
                _untouched(da, _mask2d(da.numel(), 0, B, C, ldda))
