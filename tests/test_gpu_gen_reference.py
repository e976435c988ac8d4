"""The generator kernels (sw_enc_lstm_fwd / _bwd, sw_social_pool_fwd / _bwd with their pair-row and row-block forms,
sw_dec_rollout_fwd / _bwd, sw_gen_wgrad) against a FLOAT64 reference: the oracle's modules (oracle/sw_oracle.py) cast to
double, loaded from the HIP modules' state_dicts, fed the exact fp32 inputs.  ops.gen_forward(save=True) / ops.gen_backward
(and the K-copy pair gen_forward_k / gen_backward_k) are called directly, on gradient buffers pre-filled with NaN: every
element must be written.  The other generator tests compare with the fp32 oracle at 2e-4 .. 3e-4 of a tensor's largest
entry; here every gradient tensor is held to GRAD_REL = 2e-5, the bound of the discriminator tests.

Outputs (_close_out): the rollout, the encoder state ctx.hT / ctx.cT, the pooled vector ctx.S and, for scenes of at most 64
agents, the attention weights ctx.attn (padding columns ignored).  Gradients: close_grads_branch_consistent (tests/_ref64.py):
large cases have a handful of (Leaky)ReLU inputs within MARGIN of 0 at every seed, where fp32 and float64 may take different
branches; a case passes iff its gradients equal the reference's under one binary choice of branch for those units.  Seed
rule: the first seed of SEEDS without such a unit, else the seed with the fewest; at most 16 per case.

The module's report (pytest -s) lists per group the largest output and gradient error, the ambiguous units, how many were
assigned flipped, and the gradient error before the assignment.  Observed on an MI355X, largest max|err| / max|ref|
(outputs; gradients): a.plain 6.3e-7; 1.74e-5.  b.scenes 6.8e-7; 2.17e-5 ([200, 3], which carries REL_200_3), at
most 6 ambiguous units per case, none flipped.  c.nosocial 5.3e-7; 4.5e-7.  d.forms 6.4e-7; 2.3e-6, 9 ambiguous units,
none flipped.  e.kcopies 6.3e-7; 7.3e-6.  f.degenerate 4.9e-7; 9.5e-7.  g.hidden 1.7e-7; 1.52e-5.  Fused-D form on big scenes
(test_gpu_disc_reference.py, gen_phase): 5.3e-7; 1.35e-5 with one unit flipped, 8.9e-5 before.  """
import contextlib

import numpy as np
import pytest
import torch

import sw_oracle as O
from _ref64 import (G_NAMES, GRAD_REL, MARGIN, _close_out, _f64, _report, close_grads_branch_consistent, gen_ambiguous, gen_mods,  # noqa: F401
                    gen_params, pick_fewest, run64, scene_rows)

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _pair(Tp, use_social=True, H=64):
    """The HIP generator and the float64 oracle with its weights."""
    import socialways_amd as sw
    torch.manual_seed(2000 + Tp + H)
    G = sw.Generator(hidden_size=H, use_social=use_social, device=_dev())
    if H == 64:
        G.unify()
    with _f64():
        orc = O.SocialWaysOracle(Tp, hidden_size=H, use_social=use_social)
    for name in G_NAMES:
        m = getattr(orc, name).double()
        m.load_state_dict({k: v.detach().cpu().double() for k, v in getattr(G, name).state_dict().items()})
    return G, orc


@contextlib.contextmanager
def _images(G, on):
    """Register the generator's weight images (sw_gen_images) as the training step does; dropped on exit.  The eight-wave
    encoder forward and the two-column-block decode forward exist only with them."""
    from socialways_amd import _lib as L
    if not on:
        yield
        return
    img = torch.empty(L.load().sw_gen_image_floats(), device=_dev())
    L.call("sw_gen_images", L.ptr(G.encoder._flat), L.ptr(G.decoder._flat), L.ptr(G.feature_embedder._flat),
           L.ptr(G.attention._flat), L.ptr(img), L.stream())
    try:
        yield
    finally:
        torch.cuda.synchronize()
        L.call("sw_gen_images", None, None, None, None, None, None)


def _random_walk(B, To, g):
    return (torch.randn(B, To, 2, generator=g) * 0.1).cumsum(1)


def _inputs(B, To, Tp, obsv_of=_random_walk, K=1, noise_len=32):
    def make(seed):
        g = torch.Generator().manual_seed(seed)
        return obsv_of(B, To, g), torch.rand(K * B, noise_len, generator=g), torch.randn(K * B, Tp, 4, generator=g) * 0.1
    return make


# ---- the float64 side -------------------------------------------------------------------------------------------------------
def _state64(orc, o):
    """Encoder state after the observed steps: (hT, cT)."""
    enc = orc.encoder
    with torch.no_grad(), _f64():
        B = o.shape[0]
        enc.init_lstm(torch.zeros(1, B, enc.hidden_size), torch.zeros(1, B, enc.hidden_size))
        enc(O.get_traj_4d(o, []))
        return enc.lstm_h[0].squeeze(0).clone(), enc.lstm_h[1].squeeze(0).clone()


def _attn64(orc, o, hT, sb):
    """Attention weights of every scene of 2..64 agents: [(s0, n, (n, n) weights, row i over the scene's agents j)]."""
    out = []
    with torch.no_grad(), _f64():
        last4 = O.get_traj_4d(o, [])[:, -1]
        Wh = orc.attention.W(hT)
        for s0, s1 in np.asarray(sb).reshape(-1, 2):
            s0, n = int(s0), int(s1 - s0)
            if n < 2 or n > 64:
                continue
            st = last4[s0:s0 + n]
            emb = orc.feature_embedder(O.pair_features(st[:, None, :], st[None, :, :]), None)
            sigma = (emb * Wh[s0:s0 + n][None, :, :]).sum(-1).masked_fill(torch.eye(n, dtype=torch.bool), -1000.0)
            out.append((s0, n, torch.softmax(sigma, dim=1)))
    return out


def _reference(orc, obsv, z, cot, sb, Tp, seed, K=1):
    """float64 of sum_k <predict(obsv, z_k), cot_k>: (RefRun, rollout (K * B, Tp, 4), S)."""
    o, B = obsv.double(), obsv.shape[0]
    zk, ck = z.double().view(K, B, -1), cot.double().view(K, B, Tp, 4)

    def fn():
        preds, S = [], None
        for k in range(K):
            preds.append(orc.predict(o, zk[k], Tp, sb))
            S = orc.last["S"].detach().clone()
        pred = torch.cat(preds)
        return (pred * ck.reshape(K * B, Tp, 4)).sum(), (pred.detach(), S)

    run, (pred, S) = run64(gen_params(orc), gen_mods(orc), fn, seed)
    return run, pred, S


def _pick_inputs(orc, make, sb, Tp, K=1):
    def ambiguous_of(inp):
        o, zk = inp[0].double(), inp[1].double().view(K, inp[0].shape[0], -1)
        return gen_ambiguous(orc, lambda: [orc.predict(o, zk[k], Tp, sb) for k in range(K)])
    seed, inp, n_amb = pick_fewest(make, ambiguous_of)
    return seed, inp, "seed %d, %d kink inputs within %.1e of 0" % (seed, n_amb, MARGIN)


# ---- the device side --------------------------------------------------------------------------------------------------------
def _nan_grads(G):
    return {m: torch.full_like(m._flat, float("nan")) for m in (G.encoder, G.feature_embedder, G.attention, G.decoder)}


def _named(G, grads):
    got = {}
    for name in G_NAMES:
        m = getattr(G, name)
        got.update(zip([name + "." + k for k, _ in m.named_parameters()], m.split_grad(grads[m])))
    return got


def _device(G, obsv, z, cot, sb, Tp, images=False, K=1):
    """ops.gen_forward(save=True) + ops.gen_backward (K > 1: the K-copy pair) -> (rollout, context, {name: gradient})."""
    from socialways_amd import ops
    dev = _dev()
    enc, emb, att, dec = G.encoder, G.feature_embedder, G.attention, G.decoder
    grads = _nan_grads(G)
    ws = ops.Workspaces(dev)
    B = obsv.shape[0]
    scenes = ops.SceneIndex.get(sb if len(sb) else np.zeros((0, 2), np.int64), B, dev)
    with _images(G, images):
        if K == 1:
            pred, ctx = ops.gen_forward(enc._flat, emb._flat, att._flat, dec._flat, obsv.to(dev), z.to(dev), scenes, Tp,
                                        G.use_social, save=True, ws=ws)
            ops.gen_backward(enc._flat, emb._flat, att._flat, dec._flat, ctx, cot.to(dev), grads[enc], grads[emb], grads[att],
                             grads[dec], ws=ws)
        else:
            pred, ctxk = ops.gen_forward_k(enc._flat, emb._flat, att._flat, dec._flat, obsv.to(dev), z.to(dev), scenes, Tp,
                                           G.use_social, K, ws)
            ops.gen_backward_k(enc._flat, emb._flat, att._flat, dec._flat, ctxk, cot.to(dev), grads[enc], grads[emb],
                               grads[att], grads[dec], ws)
            ctx = ctxk.one
        torch.cuda.synchronize()
    return pred, ctx, _named(G, grads)


def _check(group, sizes, To, Tp, use_social=True, images=False, K=1, obsv_of=_random_walk, one_scene=False, rel=GRAD_REL):
    B = int(np.sum(sizes))
    sb = [] if one_scene else scene_rows(sizes)       # []: predict()'s default, the whole batch is one scene
    G, orc = _pair(Tp, use_social)
    seed, (obsv, z, cot), tag = _pick_inputs(orc, _inputs(B, To, Tp, obsv_of, K), sb, Tp, K)
    pred, ctx, got = _device(G, obsv, z, cot, sb, Tp, images, K)
    run, pred64, S64 = _reference(orc, obsv, z, cot, sb, Tp, seed, K)
    _close_out(pred, pred64, "rollout", group, tag)
    hT64, cT64 = _state64(orc, obsv.double())
    _close_out(ctx.hT, hT64, "hT", group, tag)
    _close_out(ctx.cT, cT64, "cT", group, tag)
    _close_out(ctx.S, S64, "S", group, tag)
    if use_social:
        attn = ctx.attn.cpu()
        for s0, n, a64 in _attn64(orc, obsv.double(), hT64, sb if len(sb) else [[0, B]]):
            _close_out(attn[s0:s0 + n, :n], a64, "attention weights of the scene at %d" % s0, group, tag)
    else:
        assert ctx.attn is None and not bool(ctx.S.any())
    close_grads_branch_consistent(got, run, group, tag, rel)
    if not use_social or max(sizes) == 1 and not one_scene:      # no pair anywhere: exact zeros, not small numbers
        for k, g in got.items():
            if k.startswith(("feature_embedder.", "attention.")):
                assert not bool(g.any()), "d/d%s must be exactly zero (%s)" % (k, tag)


# ---- a. the plain cotangent path: gen_backward(dpred4=random, dfuse=None) -> sw_dec_rollout_bwd_aux ----------------------------
# Every To of {2, 3, 5, 8, 12} and every Tp of {1, 2, 5, 12, 13, 24, 25, 32, 64} against a ragged batch ([5, 1, 9, 4, 2]: 21
# agents, a partial second tile) and an aligned one ([8] * 4: two full tiles).  Tp 13 / 25 sit just past the decode kernels'
# 12- and 24-step staging forms; 25 is where training leaves the fused-D pass for this path.
_RAGGED, _ALIGNED = [5, 1, 9, 4, 2], [8] * 4
@pytest.mark.parametrize("To,Tp,sizes,images", [
    (2, 1, _RAGGED, False), (2, 13, _ALIGNED, True), (3, 2, _ALIGNED, False), (3, 25, _RAGGED, True),
    (5, 5, _RAGGED, True), (5, 24, _ALIGNED, False), (8, 12, _ALIGNED, True), (8, 64, _RAGGED, False),
    (12, 32, _ALIGNED, False), (12, 12, _RAGGED, True), (8, 1, _ALIGNED, True), (5, 2, _RAGGED, False),
    (2, 5, _ALIGNED, True), (12, 13, _RAGGED, False), (8, 24, _RAGGED, True), (3, 64, _ALIGNED, True),
    (5, 32, _RAGGED, True), (8, 25, _ALIGNED, False)])
def test_plain_cotangent_path_against_float64(To, Tp, sizes, images):
    _check("a.plain", sizes, To, Tp, images=images)


# ---- b. scene classes of the social block --------------------------------------------------------------------------------------
# The bound of [200, 3].  Its d/d feature_embedder.fc.4.bias = sum over 40 009 pairs of dsigma_ij Wh_j, where every row of
# dsigma sums to zero: the terms' absolute values add up to 679 times the largest entry of the result.  The fp32 CPU oracle
# misses the float64 value by 6.71e-6 of that entry on this very case (seed 1), the row-block kernel - which sums over i
# first, db3 = sum_j Wh_j sd_j - by 2.17e-5: 0.53 units of fp32 roundoff (2^-24) of the terms' absolute sum, 1 / 780 of ONE
# average term, so no term is wrong or missing; the other embedder gradients of the case, fed by the same dsigma, are
# within 6.4e-6, all other tensors within 1.7e-6.  Two fp32 sums in different orders: the bound is 4 x the oracle's error
# (a tree sum against a chain), 2.68e-5, and the kernel's error does not enter it.
REL_200_3 = 4 * 6.71e-6


@pytest.mark.parametrize("sizes,one_scene,rel", [
    ([1] * 19, False, GRAD_REL),                         # single-agent scenes only: no pair, emb / att gradients exact zeros
    ([2, 3, 4, 5, 6, 7, 8], False, GRAD_REL),            # 2..8 agents: the pair-row path
    ([15, 16, 17], False, GRAD_REL), ([31, 32, 33], False, GRAD_REL),    # both sides of every 16-agent block edge of the
    ([47, 48, 49], False, GRAD_REL), ([63, 64], False, GRAD_REL),        # one-workgroup scene kernel (dense 41..64 included)
    ([65], False, GRAD_REL), ([80], False, GRAD_REL),    # row-block kernels: one agent past AMAX; exactly five blocks
    ([70, 5, 130, 64, 1], False, GRAD_REL),              # row-block scenes mixed with small ones
    ([200, 3], False, REL_200_3),                        # a 13-block scene
    ([12], True, GRAD_REL),                              # sub_batches=[]: the whole batch is one scene
    ([8] * 256, False, GRAD_REL),                        # the metric shape
    ("ragged2048", False, GRAD_REL)])                    # a real-shaped packed batch (ragged_scene_sizes(2048, 8, seed=77))
def test_scene_classes_of_the_social_block_against_float64(sizes, one_scene, rel):
    if sizes == "ragged2048":
        import socialways_amd as sw
        sizes = sw.ragged_scene_sizes(2048, 8, seed=77)
    _check("b.scenes", sizes, 8, 12, one_scene=one_scene, rel=rel)


# ---- c. use_social=False: S is zeros, no social launch, emb / att gradients are zeros -----------------------------------------
@pytest.mark.parametrize("To,Tp,sizes", [(8, 12, [5, 1, 9, 4, 2]), (3, 25, [8] * 6)])
def test_without_the_social_block_against_float64(To, Tp, sizes):
    _check("c.nosocial", sizes, To, Tp, use_social=False)


# ---- d. launch forms chosen by the batch size (weight images registered, SW_ENC8 / SW_DEC_FWD2 at their defaults) ------------
@pytest.mark.parametrize("sizes", [
    [8] * 40,        # 20 tiles <= one per CU: the eight-wave encoder forward (enc_lstm_fwd8_kernel), one-tile decode forward
    [8] * 521])      # 261 tiles > 256: the four-wave encoder forward, the two-column-block decode forward (fwd2)
def test_launch_forms_chosen_by_batch_size_against_float64(sizes):
    _check("d.forms", sizes, 8, 12, images=True)


# ---- e. K copies: gen_forward_k / gen_backward_k against K float64 predict() calls, loss sum_k <pred_k, cot_k> -------------
@pytest.mark.parametrize("K,To,Tp,sizes", [
    (3, 8, 12, [5, 1, 9, 4, 2]),         # ragged K * B rows
    (20, 5, 12, [8, 3, 1, 4]),           # the variety loss' K
    (3, 8, 12, [66, 3]),                 # a row-block scene under the K-copy backward
    (20, 2, 25, [2, 6])])                # long horizon
def test_k_copies_against_float64(K, To, Tp, sizes):
    _check("e.kcopies", sizes, To, Tp, K=K)


# ---- f. degenerate social inputs (the eps regime of pair_feat, train.py:212,225) --------------------------------------------
def _degenerate(B, To, g):
    """Random walks whose last two frames give agents 0..31 these 4-d states (positions / velocities on a binary grid, so
    that equal means bit-equal in fp32): 0-3 stationary; 4-7 = 8-11 (same position, same velocity); 12-15 at the positions
    of 16-19 with other velocities; 20-23 with the velocities of 24-27 (dv = 0); 28 / 29 head-on (closest approach 0);
    30-31 at 1e-4 of the others' speed."""
    assert B >= 32
    obsv = _random_walk(B, To, g)
    p = (torch.randn(B, 2, generator=g) * 2 * 256).round() / 256
    v = (torch.randn(B, 2, generator=g) * 0.1 * 1024).round() / 1024
    v[0:4] = 0
    p[4:8], v[4:8] = p[8:12], v[8:12]
    p[12:16] = p[16:20]
    v[20:24] = v[24:28]
    p[28], v[28] = torch.tensor([0.0, 0.0]), torch.tensor([0.125, 0.0])
    p[29], v[29] = torch.tensor([1.0, 0.0]), torch.tensor([-0.125, 0.0])
    v[30:32] *= 1e-4
    obsv[:, -1] = p
    obsv[:, -2] = p - v
    return obsv


@pytest.mark.parametrize("sizes", [
    [48, 5],         # the one-workgroup scene kernel
    [80],            # the row-block kernels
    [8] * 4])        # the pair-row path: each kind of degenerate pair inside one 8-agent scene
def test_degenerate_social_inputs_against_float64(sizes):
    _check("f.degenerate", sizes, 8, 12, obsv_of=_degenerate)


# ---- g. hidden sizes 32 and 48 through the public Generator (zero-padded onto the 64-unit kernels) --------------------------
@pytest.mark.parametrize("H", [32, 48])
def test_smaller_hidden_sizes_against_float64(H):
    To, Tp, sizes = 8, 12, [5, 1, 9, 4, 2, 17]
    B, sb = int(np.sum(sizes)), scene_rows(sizes)
    G, orc = _pair(Tp, True, H)
    seed, (obsv, z, cot), tag = _pick_inputs(orc, _inputs(B, To, Tp, noise_len=H // 2), sb, Tp)
    pred = G(obsv.to(_dev()), z.to(_dev()), Tp, sb)
    pred.backward(cot.to(_dev()))
    torch.cuda.synchronize()
    run, pred64, _ = _reference(orc, obsv, z, cot, sb, Tp, seed)
    _close_out(pred, pred64, "rollout", "g.hidden", tag)
    got = {}
    for name in G_NAMES:
        m = getattr(G, name)
        for i, (k, p) in enumerate(m.named_parameters()):
            got[name + "." + k] = m.true_view(i, p.grad)
    close_grads_branch_consistent(got, run, "g.hidden", tag)
