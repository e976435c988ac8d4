"""The float64 comparison of tests/test_gpu_modules_reference.py, checked on the CPU: the fp32 oracle modules stand in for
the HIP modules (same weights, same inputs, same `run_*` drivers of tests/_modref.py), an fp32 torch computation stands in for
the loss-gradient kernels.  Shown here, before a GPU is involved:

  * the seed rule (`_pick` with `_kink_margin`) finds a seed for every embedder, decoder and composed case;
  * an honest fp32 computation passes OUT_RT / OUT_AT and GRAD_REL at every group and shape of the GPU file, the designed
    feature batch and the 257-agent scene included - and is nowhere further than HALF the bound from the float64 reference
    (`_within_half`), so no tensor needs a bound of its own.  Largest fp32-oracle gradient error seen here, of max|ref|:
    embed 5.3e-7, attention 1.06e-6, encoder 7.2e-7, decoder 7.3e-7, composed 8.1e-7 (GRAD_REL / 2 = 1e-5; pytest -s prints them);
  * the comparison rejects a gradient entry moved by 1e-4 of the tensor's largest, a softmax without the -1000 diagonal, an
    encoder gradient computed with dcT dropped, and an L2 gradient scaled by 1 / B instead of 1 / (B Tp);
  * the best-of-K cases leave out (two smallest float64 errors within TIE_REL) no more agents than their cap allows.

The 22 000-row L2 case of the GPU file is run at 300 rows here: its size only matters to the kernel's grid."""
import pytest
import torch

import sw_oracle as O
import _modref as M
import _ref64 as R
from _ref64 import _report      # noqa: F401  (module fixture: the observed errors, printed with pytest -s)

CPU, F32 = "cpu", torch.float32
_worst = {}     # group -> (ratio, tensor, tag): the fp32 oracle's largest gradient error, printed per test with pytest -s


def _within_half(ratios, group, tag, rel=None):
    """The rule of the bounds: a tensor whose fp32-oracle error exceeds half its bound needs a named constant of twice that
    error.  None does; this assertion is what says so."""
    for k, r in ratios.items():
        bound = (rel or {}).get(k, R.GRAD_REL)
        assert r <= bound / 2, "fp32 oracle error of d/d%s is %.2e of max|ref| > half its bound %.1e (%s)" % (k, r, bound, tag)
        if r > _worst.get(group, (0.0,))[0]:
            _worst[group] = (r, k, tag)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for group, w in sorted(_worst.items()):
        print("fp32 oracle, %-10s largest gradient error %.2e of max|ref| (d/d%s, %s)" % ((group,) + w))


def _passes(got, ref, group, tag):
    _within_half(M.compare(got, ref, group, tag), group, tag)


def _rejects(got, ref, tag):
    with pytest.raises(AssertionError, match=r"max\|err\|"):
        M.compare(got, ref, "mutations", tag)
    R._observed.pop("mutations", None)


# ---- features -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("To,Tp", M.TRAJ_CASES)
def test_traj_4d(To, Tp):
    obsv, pred = M.traj_inputs(To, Tp)
    with R._f64():
        ref = M.run_traj(O.get_traj_4d, obsv, pred, CPU, torch.float64)
    _passes(M.run_traj(O.get_traj_4d, obsv, pred, CPU, F32), ref, "features", "To %d Tp %d" % (To, Tp))


@pytest.mark.parametrize("B", M.FEATURE_B + ["designed"])
def test_social_features(B):
    x4 = M.designed_features_batch() if B == "designed" else M.feature_inputs(B)
    ref = M.run_features(O.SocialFeatures, x4, CPU, torch.float64)
    assert bool(torch.isfinite(ref["out"]["features"]).all())
    _passes(M.run_features(O.SocialFeatures, x4, CPU, F32), ref, "features", "B %s" % B)
    if B != 1:      # the restatement on explicit pairs agrees with the dense one
        last = x4[:, -1].double()
        _passes({"out": {"features": O.pair_features(last[:, None, :], last[None, :, :])}, "grad": {}}, ref, "features", "pairs")


# ---- embed ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", M.HIDDEN_2)
@pytest.mark.parametrize("rows", M.EMBED_ROWS)
def test_embed(rows, H):
    c = M.embed_case(rows, H)       # raises if no seed of SEEDS keeps the kink inputs MARGIN away from 0
    for path in M.EMBED_PATHS:
        _passes(M.run_embed(c["o32"], c["inp"], path, CPU, F32), c["ref"][path], "embed", c["tag"] + " " + path)


# ---- attention --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,H", M.ATT_CASES, ids=["%s-h%d" % ("_".join(map(str, s)), h) for s, h in M.ATT_CASES])
def test_attention(sizes, H):
    c = M.att_case(sizes, H)
    got = M.run_att(c["o32"], c["inp"], sizes, CPU, F32)
    M.check_df_outside(got["grad"]["f"], sizes, c["tag"])
    M.check_df_outside(c["ref"]["grad"]["f"], sizes, c["tag"])
    _passes(got, c["ref"], "attention", c["tag"])
    _passes(M.run_att(c["o32"], c["inp"], sizes, CPU, F32, grad=False), c["ref_nograd"], "attention", c["tag"] + " no-grad")
    R._close_out(M.att_weights(c["o32"], c["inp"], sizes, F32), c["weights"], "attention weights", "attention", c["tag"])
    # the vectorised softmax of `att_weights` is the oracle's per-agent loop
    S = c["weights"] @ c["inp"][1].double()
    R._close_out(S, c["ref"]["out"]["S"], "S from the weights", "attention", c["tag"])
    for s0, s1 in M.scene_rows(sizes):
        if s1 - s0 == 1:
            assert float(c["weights"][s0, s0]) == 0.0 and float(c["ref"]["out"]["S"][s0].abs().max()) == 0.0


@pytest.mark.parametrize("sizes", M.ATT_DIRECT, ids=["257", "63_1_2"])
def test_rejects_a_softmax_without_the_diagonal(sizes):
    c = M.att_case(sizes, 64)
    _rejects(M.run_att(c["o32"], c["inp"], sizes, CPU, F32, grad=False, diagonal=False), c["ref_nograd"], c["tag"])
    with pytest.raises(AssertionError, match="attention weights"):
        R._close_out(M.att_weights(c["o32"], c["inp"], sizes, F32, diagonal=False), c["weights"], "attention weights",
                     "mutations", c["tag"])
    R._observed.pop("mutations", None)


# ---- encoder ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", M.ENC_H)
@pytest.mark.parametrize("B,T", M.ENC_SHAPES)
def test_encoder(B, T, H):
    c = M.enc_case(B, T, H)
    for (form, need_x), ref in c["ref"].items():
        tag = "%s loss on %s%s" % (c["tag"], form, "" if need_x else ", x without a gradient")
        _passes(M.run_enc(c["o32"], c["inp"], form, need_x, CPU, F32), ref, "encoder", tag)


@pytest.mark.parametrize("B,T", M.ENC_SHAPES)
def test_rejects_an_encoder_gradient_without_dcT(B, T):
    c = M.enc_case(B, T, 64)
    for form in ("state", "all", "step"):
        _rejects(M.run_enc(c["o32"], c["inp"], form, True, CPU, F32, drop_c=True), c["ref"][(form, True)], c["tag"])


# ---- decoder, composed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", M.HIDDEN_2)
@pytest.mark.parametrize("B", M.DEC_B)
def test_decoder(B, H):
    c = M.dec_case(B, H)
    for need_z in (True, False):
        _passes(M.run_dec(c["o32"], c["inp"], need_z, CPU, F32), c["ref"][need_z], "decoder", c["tag"])


@pytest.mark.parametrize("H", M.HIDDEN_2)
def test_composed(H):
    c = M.composed_case(H)
    _passes(M.run_composed(O.SocialFeatures, c["o32"], c["inp"], M.COMPOSED_SCENES, CPU, F32), c["ref"], "composed", c["tag"])


def test_rejects_one_moved_gradient_entry():
    """One entry of one gradient tensor moved by 1e-4 of the tensor's largest: five times the bound."""
    c = M.dec_case(17, 64)
    got = M.run_dec(c["o32"], c["inp"], True, CPU, F32)
    for k in sorted(got["grad"]):
        bad = {"out": got["out"], "grad": {n: g.clone() for n, g in got["grad"].items()}}
        bad["grad"][k].view(-1)[bad["grad"][k].numel() // 2] += 1e-4 * float(c["ref"][True]["grad"][k].abs().max())
        _rejects(bad, c["ref"][True], c["tag"] + " d/d" + k)


# ---- loss gradients ---------------------------------------------------------------------------------------------------------------
L2_HOST_BIG = (300, 12)


@pytest.mark.parametrize("B,Tp,windows", [M.L2_SMALL + (M.L2_WINDOWS,), L2_HOST_BIG + ([(0, L2_HOST_BIG[0])],)])
def test_l2_grad(B, Tp, windows):
    inp, scale = M.l2_inputs(B, Tp), M.l2_scale(B, Tp)
    for row0, row1 in windows:
        tag = "B %d Tp %d rows [%d, %d)" % (B, Tp, row0, row1)
        M.check_l2(M.l2_ref(inp, row0, row1, scale, F32), inp, row0, row1, scale, "l2", tag)
        if row1 > row0:     # the scale off by Tp
            with pytest.raises(AssertionError, match="dpred4"):
                M.check_l2(M.l2_ref(inp, row0, row1, scale * Tp, F32), inp, row0, row1, scale, "mutations", tag)
            if row1 - row0 < B:     # a window one row too long (or, at the end, one row too early)
                r0, r1 = (row0, row1 + 1) if row1 < B else (row0 - 1, row1)
                with pytest.raises(AssertionError, match="outside"):
                    M.check_l2(M.l2_ref(inp, r0, r1, scale, F32), inp, row0, row1, scale, "mutations", tag)
    R._observed.pop("mutations", None)


@pytest.mark.parametrize("K", M.VARIETY_K)
def test_variety_grad_and_its_left_out_share(K):
    for B in M.VARIETY_B:
        for Tp in M.VARIETY_TP:
            inp, scale = M.variety_inputs(K, B, Tp), M.l2_scale(B, Tp)
            ref = M.variety_ref(inp, K, scale)
            n_left = int(ref["left_out"].sum())
            assert n_left <= M.left_out_cap(B), (K, B, Tp, n_left)
            tag = "K %d B %d Tp %d (%d left out)" % (K, B, Tp, n_left)
            M.check_variety(*M.variety_fp32(inp, K, scale), inp, K, ref, "variety", tag)


def test_variety_ties_go_to_the_lowest_copy():
    K, B, Tp = 20, 37, 12
    inp, scale = M.variety_inputs(K, B, Tp, duplicates=(3, 7)), M.l2_scale(B, Tp)
    ref = M.variety_ref(inp, K, scale)
    assert bool((ref["kmin"] == 3).all()) and bool((ref["l2"][3] == ref["l2"][7]).all())
    d, kmin, l2min = M.variety_fp32(inp, K, scale)
    M.check_variety(d, kmin, l2min, inp, K, ref, "variety", "ties", exact_ties=True)
    with pytest.raises(AssertionError, match="kmin differs"):       # the tie given to the higher copy
        M.check_variety(d, torch.full_like(kmin, 7), l2min, inp, K, ref, "mutations", "ties", exact_ties=True)
    R._observed.pop("mutations", None)
