"""The stand-alone module API (model.py: get_traj_4d, SocialFeatures, EmbedSocialFeatures, AttentionPooling, EncoderLstm,
DecoderFC called one by one, with and without autograd) and the loss-gradient kernels sw_l2_grad / sw_variety_grad against a
FLOAT64 reference: the oracle's modules (oracle/sw_oracle.py) built under _f64(), loaded from the HIP modules' state_dicts and
fed the exact fp32 inputs; closed forms in float64 for the two loss gradients.  Outputs are held to OUT_RT / OUT_AT, every
gradient tensor - inputs and parameters alike - to GRAD_REL = 2e-5 of its largest entry, the bound of the other three
reference suites; the fp32 module tests of test_gpu_kernels.py compare two fp32 computations at 2e-4.

Inputs, references and comparisons live in tests/_modref.py and are shared with tests/test_modules_ref_host.py, which shows
on the CPU that the seed rule finds a seed for every case with (Leaky)ReLU kinks and that an honest fp32 computation stays
within HALF of every bound used here: no tensor has a bound of its own.  The shapes are the smallest that reach each branch:
row counts around the 16-row wave and the 64-row block of the embedder kernels, scenes around the 64 agents one workgroup
stages in LDS and the 256 threads of the row kernels (a scene of 257 takes a second trip through their loops), batches of 1,
16, 17 for the LSTM and decoder tiles, the four ways a loss can reach _EncFn, the grid-stride loop of sw_l2_grad, K = 1 .. 64
of sw_variety_grad.  The dense f of the attention cases is NaN outside the scene blocks: nothing there may be read.

Every case records the names passed to socialways_amd._lib.call and asserts that the entry points it means to exercise were
the ones called, so a later change of dispatch cannot quietly move a case onto another kernel.

The module's report (pytest -s) lists per group the largest output and gradient error.  The fp32 oracle on the same inputs
(host file) shows, largest max|err| / max|ref| (outputs; gradients): features 1.1e-7; embed 2.6e-7; 5.3e-7.  attention 1.3e-6;
1.06e-6.  encoder 3.2e-7; 7.2e-7.  decoder 2.6e-7; 7.3e-7.  composed 3.2e-7; 8.1e-7.  l2 4.0e-8, variety 1.9e-7.  The figures of
the kernels on an MI355X are not recorded yet: this module has not run on one."""
import pytest
import torch

import sw_oracle as O
import _modref as M
from _ref64 import _close_out, _f64, _report      # noqa: F401  (_report: module fixture, the observed errors with pytest -s)

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def _dev():
    return torch.device("cuda:0")


@pytest.fixture
def calls(monkeypatch):
    """[(entry point, args)] of every socialways_amd._lib.call made while the test runs."""
    from socialways_amd import _lib as L
    seen, real = [], L.call

    def recorded(name, *args):
        seen.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(L, "call", recorded)
    return seen


def _names(calls):
    return [n for n, _ in calls]


def _called(calls, *names, absent=()):
    got = _names(calls)
    for n in names:
        assert n in got, "%s was not called: %s" % (n, got)
    for n in absent:
        assert n not in got, "%s was called: %s" % (n, got)
    del calls[:]


def _hip(kind, H):
    """The HIP module drawn from the seed the oracle of tests/_modref.py is drawn from (`*_case` asserts equal weights)."""
    import socialways_amd as sw
    torch.manual_seed(M.weight_seed(kind, H))
    make = {"emb": lambda: sw.EmbedSocialFeatures(3, H, device=_dev()), "att": lambda: sw.AttentionPooling(H, H, device=_dev()),
            "enc": lambda: sw.EncoderLstm(H, 1, device=_dev()), "dec": lambda: sw.DecoderFC(H + H + H // 2, device=_dev())}
    return make[kind]()


# ---- features -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("To,Tp", M.TRAJ_CASES)
def test_traj_4d(To, Tp, calls):
    import socialways_amd as sw
    obsv, pred = M.traj_inputs(To, Tp)
    with _f64():
        ref = M.run_traj(O.get_traj_4d, obsv, pred, "cpu", F64)
    M.compare(M.run_traj(sw.get_traj_4d, obsv, pred, _dev(), F32), ref, "features", "To %d Tp %d" % (To, Tp))
    _called(calls, "sw_traj_4d")


@pytest.mark.parametrize("B", M.FEATURE_B + ["designed"])
def test_social_features(B, calls):
    """B = 17: 289 pairs, a partial second block.  "designed": a standing agent, two agents at one position, two with one
    velocity, a head-on pair, a pair 1e3 apart - every value finite and equal to the float64 arithmetic."""
    import socialways_amd as sw
    x4 = M.designed_features_batch() if B == "designed" else M.feature_inputs(B)
    ref = M.run_features(O.SocialFeatures, x4, "cpu", F64)
    M.compare(M.run_features(sw.SocialFeatures, x4, _dev(), F32), ref, "features", "B %s" % B)
    _called(calls, "sw_social_features")


# ---- embed ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", M.HIDDEN_2)
@pytest.mark.parametrize("rows", M.EMBED_ROWS)
def test_embed(rows, H, calls):
    """R rows around the 16-row wave and the 64-row block (clamped tail rows), and 1600 rows of real features: the no-grad
    path, autograd with d/d features written, autograd with dfeat = NULL."""
    fe = _hip("emb", H)
    c = M.embed_case(rows, H, state=M.cpu_state(fe))
    for path in M.EMBED_PATHS:
        del calls[:]
        got = M.run_embed(fe, c["inp"], path, _dev(), F32)
        M.compare(got, c["ref"][path], "embed", c["tag"] + " " + path)
        if path == "nograd":
            assert _names(calls) == ["sw_embed_features"], _names(calls)
        else:
            dfeat = [a[5] for n, a in calls if n == "sw_embed_features_bwd"]
            assert len(dfeat) == 1 and (dfeat[0] is not None) == (path == "grad"), dfeat
            assert _names(calls).count("sw_linear_wgrad") == 3
            _called(calls, "sw_embed_features", "sw_embed_features_bwd", "sw_linear_wgrad")


# ---- attention ------------------------------------------------------------------------------------------------------------------
_ATT_IDS = ["%s-h%d" % ("_".join(map(str, s)), h) for s, h in M.ATT_CASES]


@pytest.mark.parametrize("sizes,H", M.ATT_CASES, ids=_ATT_IDS)
def test_attention(sizes, H, calls):
    """f is NaN outside the scene blocks.  Autograd path (one workgroup per agent): S, d/df - exactly 0 outside the blocks -
    d/dh, d/dW, d/db.  No-grad path: one workgroup per scene where every scene has at most 64 agents, else the row kernels."""
    att = _hip("att", H)
    c = M.att_case(sizes, H, state=M.cpu_state(att))
    got = M.run_att(att, c["inp"], sizes, _dev(), F32)
    M.check_df_outside(got["grad"]["f"], sizes, c["tag"])
    M.compare(got, c["ref"], "attention", c["tag"])
    _called(calls, "sw_attention_dense_fwd", "sw_attention_dense_bwd", "sw_linear_wgrad", absent=["sw_attention_pool_dense"])
    got = M.run_att(att, c["inp"], sizes, _dev(), F32, grad=False)
    M.compare(got, c["ref_nograd"], "attention", c["tag"] + " no-grad")
    if max(sizes) <= 64:
        _called(calls, "sw_attention_pool_dense", absent=["sw_attention_dense_fwd"])
    else:
        _called(calls, "sw_attention_dense_fwd", absent=["sw_attention_pool_dense"])
    for s0, s1 in M.scene_rows(sizes):
        if s1 - s0 == 1:
            assert float(got["out"]["S"][s0].abs().max()) == 0.0


@pytest.mark.parametrize("sizes", M.ATT_DIRECT, ids=["257", "63_1_2"])
def test_attention_weights_of_the_row_kernel(sizes, calls):
    """sw_attention_dense_fwd called directly, outputs pre-filled with NaN: the attention weights of every scene block
    against the float64 softmax with the -1000 diagonal; a single-agent scene's own entry is 0."""
    from socialways_amd import _lib as L
    att = _hip("att", 64)
    c = M.att_case(sizes, 64, state=M.cpu_state(att))
    sb = M.scene_rows(sizes)
    B = int(sb[-1, 1])
    f, h = c["inp"][0].to(_dev()), c["inp"][1].to(_dev())
    w = att.packed()
    wh = torch.empty(B, 64, device=_dev())
    L.call("sw_rows_gemm", L.ptr(h), 64, L.ptr(w), 1, 64, w.data_ptr() + 4 * 4096, B, 64, 64, L.ptr(wh), 64, 0, L.stream())
    scene_off = torch.tensor([0] + [int(e) for e in sb[:, 1]], dtype=torch.int32, device=_dev())
    attn = torch.full((B, B), float("nan"), device=_dev())
    S = torch.full((B, 64), float("nan"), device=_dev())
    L.call("sw_attention_dense_fwd", L.ptr(f), L.ptr(h), L.ptr(wh), L.ptr(scene_off), len(sizes), B, L.ptr(attn), L.ptr(S),
           L.stream())
    _called(calls, "sw_attention_dense_fwd")
    attn, S = attn.cpu(), S.cpu()
    assert bool(torch.isfinite(S).all())
    _close_out(S, c["ref"]["out"]["S"], "S", "attention", c["tag"] + " direct")
    for s0, s1 in sb:
        block = attn[s0:s1, s0:s1]
        assert bool(torch.isfinite(block).all())
        if s1 - s0 == 1:
            assert float(block[0, 0]) == 0.0
        else:
            _close_out(block, c["weights"][s0:s1, s0:s1], "attention weights", "attention", c["tag"] + " scene at %d" % s0)
            assert float(block.diagonal().abs().max()) == 0.0


@pytest.mark.parametrize("score", [40.0, 100.0])
def test_a_two_agent_scene_with_a_large_pair_score_subtracts_the_row_maximum(score, calls):
    """One scene of 2 agents whose two pair scores are `score` (f_ij = score Wh_j / |Wh_j|^2; the diagonal is masked to
    -1000), through the no-grad path - sw_attention_pool_dense, the scene kernels' softmax.  The float64 reference is finite
    (asserted): the weights are (0, 1) to the last bit and S_i = h_j.  exp(40) = 2.4e17 is an fp32 number, so at 40 a softmax
    without the subtraction of the row maximum still gives exp(40) / exp(40) = 1; exp(100) = 2.7e43 is not (fp32 ends at
    3.4e38, exp(88.7)), and there it gives inf / inf: 40 holds the peaked weights to the reference, 100 the subtraction itself."""
    att = _hip("att", 64)
    o64 = M.oracle64("att", 64, M.cpu_state(att))
    _, h, cot = M.att_inputs([2], 64)
    with torch.no_grad():
        Wh = o64.W(h.double())
    f = (score * Wh / (Wh * Wh).sum(-1, keepdim=True))[None].expand(2, 2, 64).float().contiguous()
    sigma = (f.double() * Wh[None]).sum(-1)
    assert float((sigma - score).abs().max()) < 1e-3, "both pair scores are `score` after the rounding of f to fp32"
    inp = (f, h, cot)
    ref = M.run_att(o64, inp, [2], "cpu", F64, grad=False)
    assert bool(torch.isfinite(ref["out"]["S"]).all()) and torch.equal(ref["out"]["S"], h.double().flip(0)), "S_i = h_j exactly"
    got = M.run_att(att, inp, [2], _dev(), F32, grad=False)
    _called(calls, "sw_attention_pool_dense", absent=["sw_attention_dense_fwd"])
    M.compare(got, ref, "attention", "2 agents, pair score %g" % score)


# ---- encoder --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", M.ENC_H)
@pytest.mark.parametrize("B,T", M.ENC_SHAPES)
def test_encoder(B, T, H, calls):
    """Non-zero h0, c0.  The loss on y only (dhT, dcT zero-filled), on the carried state only, on all three, and a sequence
    followed by one more step from the carried state; x with and without a gradient.  y, the carried state, d/dx, d/dh0,
    d/dc0 and the six parameter gradients."""
    enc = _hip("enc", H)
    c = M.enc_case(B, T, H, state=M.cpu_state(enc))
    for (form, need_x), ref in c["ref"].items():
        tag = "%s loss on %s%s" % (c["tag"], form, "" if need_x else ", x without a gradient")
        del calls[:]
        M.compare(M.run_enc(enc, c["inp"], form, need_x, _dev(), F32), ref, "encoder", tag)
        n = _names(calls)
        assert n.count("sw_enc_lstm_bwd") == n.count("sw_enc_lstm_wgrad") == n.count("sw_enc_lstm_fwd") == (2 if form == "step" else 1), n
        assert ("sw_rows_gemm" in n) == need_x, n      # the input gradient is two small products, made only when asked for


# ---- decoder, composed ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", M.HIDDEN_2)
@pytest.mark.parametrize("B", M.DEC_B)
def test_decoder(B, H, calls):
    """v, d/dh, d/ds, d/dz and the eight parameter gradients; once more with z not requiring a gradient: no sw_dec_fc_dz."""
    dec = _hip("dec", H)
    c = M.dec_case(B, H, state=M.cpu_state(dec))
    M.compare(M.run_dec(dec, c["inp"], True, _dev(), F32), c["ref"][True], "decoder", c["tag"])
    _called(calls, "sw_dec_rollout_fwd", "sw_dec_rollout_bwd", "sw_dec_fc_dz", "sw_dec_fc_wgrad")
    M.compare(M.run_dec(dec, c["inp"], False, _dev(), F32), c["ref"][False], "decoder", c["tag"] + ", z without a gradient")
    _called(calls, "sw_dec_rollout_fwd", "sw_dec_rollout_bwd", "sw_dec_fc_wgrad", absent=["sw_dec_fc_dz"])


@pytest.mark.parametrize("H", M.HIDDEN_2)
def test_composed(H, calls):
    """SocialFeatures -> EmbedSocialFeatures -> AttentionPooling -> DecoderFC with autograd through the chain, scenes of 5,
    1, 70 and 24 agents: every output, d/dh, d/dz and the sixteen parameter gradients."""
    import socialways_amd as sw
    mods = [_hip(k, H) for k in M.COMPOSED_KINDS]
    c = M.composed_case(H, states=[M.cpu_state(m) for m in mods])
    got = M.run_composed(sw.SocialFeatures, mods, c["inp"], M.COMPOSED_SCENES, _dev(), F32)
    M.compare(got, c["ref"], "composed", c["tag"])
    _called(calls, "sw_social_features", "sw_embed_features", "sw_embed_features_bwd", "sw_attention_dense_fwd",
            "sw_attention_dense_bwd", "sw_linear_wgrad", "sw_dec_rollout_fwd", "sw_dec_rollout_bwd", "sw_dec_fc_dz",
            "sw_dec_fc_wgrad")


# ---- loss gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Tp,windows", [M.L2_SMALL + (M.L2_WINDOWS,), M.L2_BIG + ([(0, M.L2_BIG[0])],)],
                         ids=["windows", "grid-stride"])
def test_l2_grad(B, Tp, windows, calls):
    """dpred4 pre-filled with random values: rows outside the window and columns 2:4 everywhere stay bit-identical, rows
    inside match float64.  22 000 x 12 elements are more than 1024 blocks x 256 threads: the grid-stride loop runs."""
    from socialways_amd import _lib as L
    inp, scale = M.l2_inputs(B, Tp), M.l2_scale(B, Tp)
    pred4, gt = inp[0].to(_dev()), inp[1].to(_dev())
    for row0, row1 in windows:
        d = inp[2].to(_dev())
        L.call("sw_l2_grad", L.ptr(pred4), L.ptr(gt), B, Tp, row0, row1, scale, L.ptr(d), L.stream())
        M.check_l2(d, inp, row0, row1, scale, "l2", "B %d Tp %d rows [%d, %d)" % (B, Tp, row0, row1))
    _called(calls, "sw_l2_grad")


def _variety(inp, K, scale):
    from socialways_amd import _lib as L
    predK, gt, d = (t.to(_dev()) for t in inp)
    B, Tp = gt.shape[0], gt.shape[1]
    kmin = torch.full((B,), -1, dtype=torch.int32, device=_dev())
    l2min = torch.full((B,), float("nan"), device=_dev())
    L.call("sw_variety_grad", L.ptr(predK), L.ptr(gt), K, B, Tp, scale, L.ptr(d), L.ptr(kmin), L.ptr(l2min), L.stream())
    return d, kmin, l2min


@pytest.mark.parametrize("K", M.VARIETY_K)
def test_variety_grad(K, calls):
    """B = 1, 5, 1000 x Tp = 1, 12, 70 (the lane loop over Tp > 64): l2min, kmin = the float64 argmin (agents whose two
    smallest errors are within TIE_REL left out: the host file holds their number to the cap), dpredK changed only in the
    rows kmin[b] * B + b, by the reference's amount."""
    for B in M.VARIETY_B:
        for Tp in M.VARIETY_TP:
            inp, scale = M.variety_inputs(K, B, Tp), M.l2_scale(B, Tp)
            ref = M.variety_ref(inp, K, scale)
            d, kmin, l2min = _variety(inp, K, scale)
            M.check_variety(d, kmin, l2min, inp, K, ref, "variety", "K %d B %d Tp %d" % (K, B, Tp))
    _called(calls, "sw_variety_grad")


def test_variety_ties_go_to_the_lowest_copy(calls):
    K, B, Tp = 20, 37, 12
    inp, scale = M.variety_inputs(K, B, Tp, duplicates=(3, 7)), M.l2_scale(B, Tp)
    ref = M.variety_ref(inp, K, scale)
    d, kmin, l2min = _variety(inp, K, scale)
    assert bool((kmin.cpu() == 3).all()), kmin.cpu().tolist()
    M.check_variety(d, kmin, l2min, inp, K, ref, "variety", "copies 3 and 7 equal", exact_ties=True)
    _called(calls, "sw_variety_grad")


def test_variety_refuses_65_copies(calls):
    from socialways_amd import _lib as L
    K, B, Tp = 65, 5, 12
    inp = M.variety_inputs(K, B, Tp)
    predK, gt, d = (t.to(_dev()) for t in inp)
    kmin = torch.full((B,), -1, dtype=torch.int32, device=_dev())
    l2min = torch.full((B,), -2.0, device=_dev())
    with pytest.raises(L.SocialWaysHipError, match="unsupported shape"):
        L.call("sw_variety_grad", L.ptr(predK), L.ptr(gt), K, B, Tp, M.l2_scale(B, Tp), L.ptr(d), L.ptr(kmin), L.ptr(l2min),
               L.stream())
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), inp[2]) and bool((kmin.cpu() == -1).all()) and bool((l2min.cpu() == -2.0).all())
    _called(calls, "sw_variety_grad")
