"""Training on ragged observation histories on the GPU: sw_enc_lstm_fwd_ragged_save / sw_disc_fwd_ragged /
sw_disc_dpred_ragged and what is built on them (ops.gen_forward / gen_forward_k / disc_forward / disc_dpred with obs_len,
SocialWaysTrainer.step(obs_len=...), train_epoch_ragged).

1. the saved rows: zeros in front of a row's start, the dense kernels' bits on the truncated buffers from it on;
2. the padding is never read (NaN against a repeated frame, bit for bit, through the whole ops-level pipeline);
3. full length is the dense code path downstream (bit for bit);
4. every gradient against float64 (tests/_ragged_ref.py through tests/_ref64.py, GRAD_REL = 2e-5);
5. the step against the dense step at full length, and a mixed-length step that differs;
6. the epoch on the ragged synthetic recording.

Shapes: the 117 agents of tests/test_gpu_sample.py (a partial last tile, one scene above 64 agents), To = 8, Tp = 12;
(To, Tp) = (3, 2) in 1 and 4; 21 agents at Tp = 25 - the generator phase without sw_disc_dpred - in 4 and 5."""
import numpy as np
import pytest
import torch

import sw_oracle as O
from _ragged_ref import disc_ragged, predict_ragged
from _ref64 import (G_NAMES, GRAD_REL, MARGIN, _close_grad, _close_out, _f64, _kink_margin, _pick, _report,  # noqa: F401
                    close_grads_branch_consistent, gen_ambiguous, gen_mods, gen_params, pick_fewest, run64, scene_rows)
from _util import assert_close
from test_gpu_disc_reference import TARGETS, W_INFO, _d64, _disc, _grads_of, _tile_sums
from test_gpu_ragged import B, To, Tp, disc_images, gen_images, groups, inputs, lengths, padded
from test_gpu_sample import SIZES, crowd

pytestmark = pytest.mark.gpu

NAN = float("nan")
SMALL = [5, 1, 9, 4, 2]        # 21 agents: the shape of the Tp = 25 cases


def bits(a, b):
    """Bit for bit: -0 is not +0, and a NaN equals the same NaN."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def zero_bits(a):
    return not bool(a.contiguous().view(torch.int32).any())


def dev_len(ln):
    return torch.from_numpy(np.asarray(ln, dtype=np.int32)).cuda()


def mixes_a_tile_and_a_scene(ln, sb, T):
    """A row of length 2 and a row of length T share a 16-row tile and a scene."""
    ln = np.asarray(ln)
    for a, b in np.asarray(sb):
        for t0 in range(int(a) // 16 * 16, int(b), 16):
            lo, hi = max(int(a), t0), min(int(b), t0 + 16)
            if hi > lo and (ln[lo:hi] == 2).any() and (ln[lo:hi] == T).any():
                return True
    return False


@pytest.fixture(scope="module")
def G():
    import socialways_amd as sw
    torch.manual_seed(0)
    g = sw.Generator(use_social=True, device="cuda:0")
    g.unify()
    return g


# ---- 1. the saved rows ------------------------------------------------------------------------------------------------------------
def enc_save_dense(G, x, x_mode):
    from socialways_amd import _lib as L
    n, T = x.shape[0], x.shape[1]
    hT, cT = torch.full((n, 64), NAN, device="cuda"), torch.full((n, 64), NAN, device="cuda")
    act, x4s = torch.full((T, n, 384), NAN, device="cuda"), torch.full((T, n, 4), NAN, device="cuda")
    L.call("sw_enc_lstm_fwd", L.ptr(x.contiguous()), x_mode, L.ptr(G.encoder._flat), None, None, n, T, L.ptr(hT), L.ptr(cT), None,
           L.ptr(act), L.ptr(x4s), 0, L.stream())
    return hT, cT, act, x4s


def enc_save_ragged(G, x, x_mode, ln):
    from socialways_amd import _lib as L
    n, T = x.shape[0], x.shape[1]
    hT, cT = torch.full((n, 64), NAN, device="cuda"), torch.full((n, 64), NAN, device="cuda")
    act, x4s = torch.full((T, n, 384), NAN, device="cuda"), torch.full((T, n, 4), NAN, device="cuda")
    L.call("sw_enc_lstm_fwd_ragged_save", L.ptr(x.contiguous()), x_mode, L.ptr(G.encoder._flat), L.ptr(ln), n, T, L.ptr(hT),
           L.ptr(cT), L.ptr(act), L.ptr(x4s), L.stream())
    return hT, cT, act, x4s


def check_rows(act, x4s, ln, dense_of, T=To):
    """act (T, B, 384) / x4s (T, B, 4) of a ragged pass against dense_of(n, idx) -> (act (n, m, 384), x4s (n, m, 4)) of the
    dense entry on the truncated buffer of each length group."""
    for n, idx in groups(ln):
        s = T - n
        assert zero_bits(act[:s, idx]) and zero_bits(x4s[:s, idx]), n
        aD, xD = dense_of(n, idx)
        assert bits(act[s:, idx], aD) and bits(x4s[s:, idx], xD), n
        assert bool(torch.isfinite(aD).all()) and float(aD.abs().max()) > 0


@pytest.mark.parametrize("variant", ["cycle", "tile2", "tile8"])
@pytest.mark.parametrize("x_mode", [0, 1])
@pytest.mark.parametrize("images", [False, True])
def test_encoder_saves_zero_rows_then_the_dense_rows_of_the_truncated_buffers(G, images, x_mode, variant):
    lo = 2 if x_mode == 0 else 1
    ln = lengths(variant, lo)
    x = inputs(x_mode)
    with gen_images(G, images):
        hT, cT, act, x4s = enc_save_ragged(G, padded(x, ln, NAN), x_mode, dev_len(ln))
        assert sorted(n for n, _ in groups(ln)) == list(range(lo, To + 1))
        dense = {}

        def dense_of(n, idx):
            dense[n] = enc_save_dense(G, x[idx, To - n:], x_mode)
            return dense[n][2], dense[n][3]
        check_rows(act, x4s, ln, dense_of)
        for n, idx in groups(ln):
            assert bits(hT[idx], dense[n][0]) and bits(cT[idx], dense[n][1]), n
        # NULL and all-To: the dense launch's saves
        hD, cD, aD, xD = enc_save_dense(G, x, x_mode)
        for full in (None, dev_len(np.full(B, To))):
            got = enc_save_ragged(G, x, x_mode, full)
            assert all(bits(a, b) for a, b in zip(got, (hD, cD, aD, xD)))
    assert bool(torch.isfinite(act).all()) and bool(torch.isfinite(x4s).all())


def dsave_parts(dsave, n, T, tp, nb):
    """The regions of a discriminator save buffer (dsave_layout, csrc/sw_disc_dev.h), agents on dimension -2."""
    out, o = {}, 0
    for name, shape in (("act", (T, n, 384)), ("x4s", (T, n, 4)), ("o1", (n, 32)), ("both", (nb, n, 64)), ("q1", (nb, n, 32)),
                        ("c1", (nb, n, 32)), ("l1", (nb, n, 32)), ("px", (nb, n, 4 * tp))):
        k = int(np.prod(shape))
        out[name] = dsave[o:o + k].view(shape)
        o += k
    return out


def disc_pass(D, x, preds, z, ln):
    """disc_forward(save) + disc_backward_gan with weight gradients on NaN-prefilled buffers -> everything the pass leaves."""
    from socialways_amd import _lib as L, ops
    n, T, tp, nb = x.shape[0], x.shape[1], preds[0].shape[1], len(preds)
    ws = ops.Workspaces(x.device)
    ws.get("d.dsave", L.workspace_floats(L.WS_DSAVE, n, T, tp, nb)).fill_(NAN)
    targets = torch.tensor(TARGETS, device=x.device)
    dflat = torch.full_like(D._flat, NAN)
    part = torch.full(((n + 15) // 16, 3), NAN, device=x.device)
    labels, codes, ctx = ops.disc_forward(D._flat, x, preds, save=True, ws=ws, obs_len=ln)
    dpreds = ops.disc_backward_gan(D._flat, ctx, labels, codes, targets, (0, 1), z, 1.0 / n, W_INFO / (2.0 * n), dflat,
                                   (True,) * nb, ws=ws, loss_part=part)
    torch.cuda.synchronize()
    return dict(labels=labels, codes=codes, dpreds=dpreds, dflat=dflat, part=part, save=dsave_parts(ctx.dsave, n, T, tp, nb), ws=ws)


@pytest.mark.parametrize("T,tp", [(To, Tp), (3, 2)])
@pytest.mark.parametrize("x_mode", [0, 1])
@pytest.mark.parametrize("images", [False, True])
def test_discriminator_saves_zero_rows_and_gives_the_dense_bits_per_agent(images, x_mode, T, tp):
    from socialways_amd import ops
    D = _disc(tp)
    lo = 2 if x_mode == 0 else 1
    x = inputs(x_mode, T=T, seed=11)
    gen = torch.Generator(device="cuda").manual_seed(5)
    preds = [(torch.rand(B, tp, 4, device="cuda", generator=gen) * 0.2 - 0.1).contiguous() for _ in range(2)]
    z = torch.rand(B, 32, device="cuda", generator=gen)
    targets = torch.tensor(TARGETS, device="cuda")
    with disc_images(D, images):
        for variant in ("cycle", "tile2", "tile8"):
            ln = lengths(variant, lo, T=T)
            got = disc_pass(D, padded(x, ln, NAN), preds, z, dev_len(ln))
            dp_part = torch.full(((B + 15) // 16, 3), NAN, device="cuda")
            dpred = ops.disc_dpred(D._flat, padded(x, ln, NAN), preds[0], targets, 1, z, 1.0 / B, W_INFO / (2.0 * B),
                                   loss_part=dp_part, obs_len=dev_len(ln))
            want, sums, dp_sums = {}, torch.zeros(3, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
            for n, idx in groups(ln):
                pk = [p[idx].contiguous() for p in preds]
                want[n] = w = disc_pass(D, x[idx, T - n:].contiguous(), pk, z[idx].contiguous(), None)
                for k in range(2):      # agents are columns of the products: the dense bits, whoever shares the tile
                    assert bits(got["labels"][k][idx], w["labels"][k]) and bits(got["codes"][k][idx], w["codes"][k]), (variant, n)
                for name in ("o1", "both", "q1", "c1", "l1", "px"):
                    assert bits(got["save"][name][..., idx, :], w["save"][name]), (variant, n, name)
                sums += w["part"].double().sum(0).cpu()
                wp = torch.full(((len(idx) + 15) // 16, 3), NAN, device="cuda")
                dD = ops.disc_dpred(D._flat, x[idx, T - n:].contiguous(), pk[0], targets, 1, z[idx].contiguous(), 1.0 / B,
                                    W_INFO / (2.0 * B), loss_part=wp)
                assert bits(dpred[idx], dD), (variant, n)
                dp_sums += wp[:, :2].double().sum(0).cpu()
            check_rows(got["save"]["act"], got["save"]["x4s"], ln, lambda n, idx: (want[n]["save"]["act"], want[n]["save"]["x4s"]), T)
            # the per-tile loss partials cover other agents: compared as sums ("fused vs literal losses", test_gpu_trainer.py)
            assert_close(got["part"].double().sum(0).cpu().numpy(), sums.numpy(), 1e-5, 1e-7, "loss sums of the update pass")
            assert_close(dp_part[:, :2].double().sum(0).cpu().numpy(), dp_sums.numpy(), 1e-5, 1e-7, "loss sums of the generator phase")
            assert all(bool(torch.isfinite(g).all()) for g in _grads_of(D, got["dflat"]).values()) and bool(torch.isfinite(dpred).all())
            if variant != "tile8":
                dense = disc_pass(D, x, preds, z, None)
                assert not bits(got["labels"][0][16:32], dense["labels"][0][16:32])


# ---- 2. / 3. the ops-level pipeline -----------------------------------------------------------------------------------------------
def pipeline(G, D, obsv, pred4, z, cot, sb, ln, dense_calls=False):
    """gen_forward(save) + gen_backward, disc_forward + disc_backward_gan, disc_dpred on NaN-prefilled gradient buffers ->
    {name: tensor} of every output, saved LSTM row, loss partial and gradient.  dense_calls: the calls without obs_len."""
    from socialways_amd import ops
    dev = obsv.device
    n, T, tp = obsv.shape[0], obsv.shape[1], pred4.shape[1]
    kw = {} if dense_calls else dict(obs_len=ln)
    enc, emb, att, dec = G.encoder, G.feature_embedder, G.attention, G.decoder
    grads = {m: torch.full_like(m._flat, NAN) for m in (enc, emb, att, dec)}
    ws = ops.Workspaces(dev)
    scenes = ops.SceneIndex.get(sb, n, dev)
    targets = torch.tensor(TARGETS, device=dev)
    out = {}
    pred, ctx = ops.gen_forward(enc._flat, emb._flat, att._flat, dec._flat, obsv, z, scenes, tp, True, save=True, ws=ws, **kw)
    out["g.act"] = ctx.gsave[:T * n * 384].clone()
    out["g.x4s"] = ctx.gsave[(T + tp - 1) * n * 384:(T + tp - 1) * n * 384 + T * n * 4].clone()
    ops.gen_backward(enc._flat, emb._flat, att._flat, dec._flat, ctx, cot, grads[enc], grads[emb], grads[att], grads[dec], ws=ws)
    out.update(pred=pred, hT=ctx.hT, cT=ctx.cT, S=ctx.S)
    for name, m in zip(G_NAMES, (enc, emb, att, dec)):      # per parameter: the packed buffers have alignment gaps nobody writes
        out.update(zip(["dG.%s.%s" % (name, k) for k, _ in m.named_parameters()], m.split_grad(grads[m])))
    dflat = torch.full_like(D._flat, NAN)
    part = torch.full(((n + 15) // 16, 3), NAN, device=dev)
    labels, codes, dctx = ops.disc_forward(D._flat, obsv, [pred, pred4], save=True, ws=ws, **kw)
    ops.disc_backward_gan(D._flat, dctx, labels, codes, targets, (0, 1), z, 1.0 / n, W_INFO / (2.0 * n), dflat, (), ws=ws,
                          loss_part=part)
    sv = dsave_parts(dctx.dsave, n, T, tp, 2)
    out.update({"d.label%d" % k: labels[k] for k in range(2)})
    out.update({"d.code%d" % k: codes[k] for k in range(2)})
    out.update({"d.act": sv["act"].clone(), "d.x4s": sv["x4s"].clone(), "d.part": part})
    out.update({"dD." + k: g for k, g in _grads_of(D, dflat).items()})
    gp = torch.full(((n + 15) // 16, 2), NAN, device=dev)
    gp3 = torch.full(((n + 15) // 16, 3), NAN, device=dev)
    out["g.dpred"] = ops.disc_dpred(D._flat, obsv, pred, targets, 1, z, 1.0 / n, W_INFO / (2.0 * n), loss_part=gp3, **kw)
    gp.copy_(gp3[:, :2])
    out["g.part"] = gp
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def pipe_inputs():
    obsv, gt, sb = crowd(SIZES)
    from socialways_amd import get_traj_4d
    gen = torch.Generator(device="cuda").manual_seed(21)
    z = torch.rand(B, 32, device="cuda", generator=gen)
    cot = (torch.randn(B, Tp, 4, device="cuda", generator=gen) * 0.1).contiguous()
    return obsv, get_traj_4d(obsv, gt)[1].contiguous(), z, cot, sb


@pytest.mark.parametrize("images", [False, True])
def test_the_padding_is_never_read(G, pipe_inputs, images):
    obsv, pred4, z, cot, sb = pipe_inputs
    D = _disc(Tp)
    ln = lengths("cycle")
    with gen_images(G, images), disc_images(D, images):
        a = pipeline(G, D, padded(obsv, ln, "repeat"), pred4, z, cot, sb, dev_len(ln))
        b = pipeline(G, D, padded(obsv, ln, NAN), pred4, z, cot, sb, dev_len(ln))
    assert set(a) == set(b) and len(a) > 40
    for k in a:
        assert not bool(torch.isnan(b[k]).any()), k
        assert bits(a[k], b[k]), k
    full = pipeline(G, D, obsv, pred4, z, cot, sb, None)
    for k in ("pred", "dG.encoder.lstm.weight_hh_l0", "dG.decoder.fc1.0.weight", "dD.obsv_encoder_lstm.weight_hh_l0", "g.dpred"):
        assert not bits(a[k], full[k]), k


@pytest.mark.parametrize("images", [False, True])
def test_full_length_is_the_dense_code_path_downstream(G, pipe_inputs, images):
    obsv, pred4, z, cot, sb = pipe_inputs
    D = _disc(Tp)
    with gen_images(G, images), disc_images(D, images):
        dense = pipeline(G, D, obsv, pred4, z, cot, sb, None, dense_calls=True)
        for ln in (None, dev_len(np.full(B, To))):
            got = pipeline(G, D, obsv, pred4, z, cot, sb, ln)
            for k in dense:
                assert bits(got[k], dense[k]), (k, ln is None)
    assert all(bool(torch.isfinite(v).all()) for v in dense.values())


# ---- 4. gradients against float64 ------------------------------------------------------------------------------------------------
def _gen_pair(tp, use_social):
    import socialways_amd as sw
    torch.manual_seed(2000 + tp)
    g = sw.Generator(use_social=use_social, device="cuda:0")
    g.unify()
    with _f64():
        orc = O.SocialWaysOracle(tp, use_social=use_social)
    for name in G_NAMES:
        getattr(orc, name).double().load_state_dict({k: v.detach().cpu().double() for k, v in getattr(g, name).state_dict().items()})
    return g, orc


@pytest.mark.parametrize("use_social,K,T,tp,sizes", [(True, 1, To, Tp, SIZES), (False, 1, To, Tp, SIZES), (True, 3, To, Tp, SIZES),
                                                     (True, 1, 3, 2, SIZES), (True, 1, To, 25, SMALL)])
def test_generator_gradients_at_mixed_lengths_against_float64(use_social, K, T, tp, sizes):
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    n = int(np.sum(sizes))
    sb = scene_rows(sizes)
    ln = lengths("cycle", 2, T=T, n=n)
    if n < B:
        ln[5:8] = (2, T, 2)         # the small batch: a short and a full row inside its 9-agent scene
    assert mixes_a_tile_and_a_scene(ln, sb, T)
    G_, orc = _gen_pair(tp, use_social)

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        return ((torch.randn(n, T, 2, generator=g) * 0.1).cumsum(1), torch.rand(K * n, 32, generator=g),
                torch.randn(K * n, tp, 4, generator=g) * 0.1)

    def rollouts(o, zk):
        return [predict_ragged(orc, o, ln, zk[k], tp, sb) for k in range(K)]
    seed, (obsv, z, cot), n_amb = pick_fewest(make, lambda inp: gen_ambiguous(
        orc, lambda: rollouts(inp[0].double(), inp[1].double().view(K, n, -1))))
    tag = "seed %d, %d kink inputs within %.1e of 0" % (seed, n_amb, MARGIN)
    enc, emb, att, dec = G_.encoder, G_.feature_embedder, G_.attention, G_.decoder
    grads = {m: torch.full_like(m._flat, NAN) for m in (enc, emb, att, dec)}
    ws = ops.Workspaces(dev)
    scenes = ops.SceneIndex.get(sb, n, dev)
    o_dev = padded(obsv, ln, NAN).to(dev)
    if K == 1:
        pred, ctx = ops.gen_forward(enc._flat, emb._flat, att._flat, dec._flat, o_dev, z.to(dev), scenes, tp, use_social, save=True,
                                    ws=ws, obs_len=dev_len(ln))
        ops.gen_backward(enc._flat, emb._flat, att._flat, dec._flat, ctx, cot.to(dev), grads[enc], grads[emb], grads[att],
                         grads[dec], ws=ws)
    else:
        pred, ctxk = ops.gen_forward_k(enc._flat, emb._flat, att._flat, dec._flat, o_dev, z.to(dev), scenes, tp, use_social, K, ws,
                                       obs_len=dev_len(ln))
        ops.gen_backward_k(enc._flat, emb._flat, att._flat, dec._flat, ctxk, cot.to(dev), grads[enc], grads[emb], grads[att],
                           grads[dec], ws)
        ctx = ctxk.one
    torch.cuda.synchronize()

    def fn():
        p = torch.cat(rollouts(obsv.double(), z.double().view(K, n, -1)))
        state = tuple(orc.last[k].detach().clone() for k in ("hT", "cT", "S"))
        return (p * cot.double()).sum(), (p.detach(), state)
    run, (pred64, (hT64, cT64, S64)) = run64(gen_params(orc), gen_mods(orc), fn, seed)
    group = "ragged.gen"
    _close_out(pred, pred64, "rollout", group, tag)
    _close_out(ctx.hT, hT64, "hT", group, tag)
    _close_out(ctx.cT, cT64, "cT", group, tag)
    _close_out(ctx.S, S64, "S", group, tag)
    got = {}
    for name in G_NAMES:
        m = getattr(G_, name)
        got.update(zip([name + "." + k for k, _ in m.named_parameters()], m.split_grad(grads[m])))
    close_grads_branch_consistent(got, run, group, tag, GRAD_REL)


def _disc_make(n, T, tp, nb):
    def make(seed):
        g = torch.Generator().manual_seed(seed)
        return ((torch.randn(n, T, 2, generator=g) * 0.1).cumsum(1), [torch.randn(n, tp, 4, generator=g) * 0.2 for _ in range(nb)],
                torch.rand(n, 32, generator=g))
    return make


def _disc64(Dref, obsv, ln, preds):
    p64 = [p.detach().cpu().double().requires_grad_() for p in preds]
    with _f64(), _kink_margin(Dref) as margin:
        outs = [disc_ragged(Dref, obsv.double(), ln, p) for p in p64]
    return [l for l, _ in outs], [c for _, c in outs], p64, margin


@pytest.mark.parametrize("T,tp", [(To, Tp), (3, 2)])
def test_discriminator_update_gradients_at_mixed_lengths_against_float64(T, tp):
    """Every weight gradient of a two-branch update pass (disc_forward(obs_len=) + disc_backward_gan)."""
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    ln = lengths("cycle", 2, T=T)
    assert mixes_a_tile_and_a_scene(ln, [[0, B]], T)
    D = _disc(tp)
    Dref = _d64(D)
    seed, (obsv, preds, z), margin = _pick(_disc_make(B, T, tp, 2), lambda inp: _disc64(Dref, inp[0], ln, inp[1])[3][0])
    tag = "seed %d, kink margin %.2e" % (seed, margin)
    ws = ops.Workspaces(dev)
    targets = torch.tensor(TARGETS, device=dev)
    dflat = torch.full_like(D._flat, NAN)
    part = torch.full(((B + 15) // 16, 3), NAN, device=dev)
    with disc_images(D, True):
        labels, codes, ctx = ops.disc_forward(D._flat, padded(obsv, ln, NAN).to(dev), [p.to(dev) for p in preds], save=True, ws=ws,
                                              obs_len=dev_len(ln))
        ops.disc_backward_gan(D._flat, ctx, labels, codes, targets, (0, 1), z.to(dev), 1.0 / B, W_INFO / (2.0 * B), dflat, (),
                              ws=ws, loss_part=part)
        torch.cuda.synchronize()
    rl, rc, p64, _ = _disc64(Dref, obsv, ln, preds)
    z2 = z.double()[:, :2]
    t0, t1 = (float(torch.tensor(t, dtype=torch.float32)) for t in TARGETS)
    (((rl[0] - t0) ** 2).mean() + ((rl[1] - t1) ** 2).mean() + W_INFO * ((rc[0] - z2) ** 2).mean()).backward()
    for k in range(2):
        _close_out(labels[k], rl[k], "label[%d]" % k, "ragged.disc", tag)
        _close_out(codes[k], rc[k], "code[%d]" % k, "ragged.disc", tag)
    got = _grads_of(D, dflat)
    for k, q in Dref.named_parameters():
        _close_grad(got[k], q.grad, "dD/d%s" % k, "ragged.disc", tag)
    parts64 = torch.stack([((rl[0] - t0) ** 2).sum(1), ((rc[0] - z2) ** 2).sum(1), ((rl[1] - t1) ** 2).sum(1)], 1).detach()
    for c in range(3):
        _close_out(part[:, c], _tile_sums(parts64[:, c], B), "loss_part column %d" % c, "ragged.disc", tag)


@pytest.mark.parametrize("T,tp,n", [(To, Tp, B), (3, 2, B), (To, 25, 21)])
def test_generator_phase_dpred_at_mixed_lengths_against_float64(T, tp, n):
    """d/d(pred) of the generator phase: disc_dpred(obs_len=) and, at Tp = 25, disc_forward(save_lstm=0, obs_len=) +
    disc_backward_gan - the route of the step where sw_disc_dpred does not fit."""
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    ln = lengths("cycle", 2, T=T, n=n)
    assert mixes_a_tile_and_a_scene(ln, [[0, n]], T)
    assert ops.disc_dpred_supported(tp) == (tp <= 24)
    D = _disc(tp)
    Dref = _d64(D)
    seed, (obsv, preds, z), margin = _pick(_disc_make(n, T, tp, 1), lambda inp: _disc64(Dref, inp[0], ln, inp[1])[3][0])
    tag = "seed %d, kink margin %.2e" % (seed, margin)
    targets = torch.tensor(TARGETS, device=dev)
    part = torch.full(((n + 15) // 16, 3), NAN, device=dev)
    o, p, zd = padded(obsv, ln, NAN).to(dev), preds[0].to(dev), z.to(dev)
    with disc_images(D, True):
        if tp <= 24:
            dpred = ops.disc_dpred(D._flat, o, p, targets, 1, zd, 1.0 / n, W_INFO / (2.0 * n), loss_part=part, obs_len=dev_len(ln))
        else:
            ws = ops.Workspaces(dev)
            labels, codes, ctx = ops.disc_forward(D._flat, o, [p], save=True, ws=ws, save_lstm=0, obs_len=dev_len(ln))
            dpred = ops.disc_backward_gan(D._flat, ctx, labels, codes, targets, (1,), zd, 1.0 / n, W_INFO / (2.0 * n), None,
                                          (True,), ws=ws, loss_part=part)[0]
        torch.cuda.synchronize()
    rl, rc, p64, _ = _disc64(Dref, obsv, ln, preds)
    z2 = z.double()[:, :2]
    t1 = float(torch.tensor(TARGETS[1], dtype=torch.float32))
    (((rl[0] - t1) ** 2).mean() + W_INFO * ((rc[0] - z2) ** 2).mean()).backward()
    _close_out(dpred, p64[0].grad, "d/dpred", "ragged.dpred", tag)
    parts64 = torch.stack([((rl[0] - t1) ** 2).sum(1), ((rc[0] - z2) ** 2).sum(1)], 1).detach()
    for c in range(2):
        _close_out(part[:, c], _tile_sums(parts64[:, c], n), "loss_part column %d" % c, "ragged.dpred", tag)


# ---- 5. the step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tp,sizes,kw", [(Tp, SIZES, {}), (25, SMALL, {}), (Tp, SIZES, dict(use_l2_loss=True, n_unrolling_steps=2))])
def test_step_with_full_length_obs_len_follows_the_dense_step(tp, sizes, kw):
    import socialways_amd as sw

    def trainer():
        torch.manual_seed(31)
        return sw.SocialWaysTrainer(tp, use_social=True, device="cuda:0", use_graph=False, **kw)
    obsv, gt, sb = crowd(sizes, Tp=tp)
    n = obsv.shape[0]
    z = torch.rand(n, 32, generator=torch.Generator().manual_seed(4))
    ln = lengths("cycle", n=n)

    def run(tr, obs_len, o=obsv):
        out = tr.step(o, gt, sb, 0.04, 0.93, z, 1.0, **({} if obs_len is None else dict(obs_len=obs_len)))
        torch.cuda.synchronize()
        return tr.losses_from(out, [n], tp, 1.0)[0], out.cpu()
    a, b, c = trainer(), trainer(), trainer()
    assert all(torch.equal(p, q) for p, q in zip(a.G.state_dict().values(), b.G.state_dict().values()))
    la, oa = run(a, None)
    lb, ob = run(b, np.full(n, To))
    assert np.isfinite(la).all() and np.isfinite(lb).all()
    assert_close(lb, la, 1e-5, 1e-7, "losses: step(obs_len=full) against step()")
    for ma, mb in ((a.G, b.G), (a.D, b.D)):
        for (k, pa), (_, pb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            bad = (pb - pa).abs() > 1e-6 + 1e-4 * pa.abs()
            assert bad.float().mean().item() <= 1e-3, (k, (pa - pb).abs().max().item())
    assert not torch.equal(a.G.encoder._flat, trainer().G.encoder._flat), "the step moved the weights"
    # mixed lengths: another step - and the padding does not enter it
    lc, oc = run(c, ln, padded(obsv, ln, NAN))
    assert np.isfinite(lc).all() and bool(torch.isfinite(c.G._flat_all).all()) and bool(torch.isfinite(c.D._flat).all())
    assert np.abs(lc - la).max() > 1e-4 * np.abs(la).max()
    assert not torch.equal(c.G.encoder._flat, a.G.encoder._flat) and not torch.equal(c.D._flat, a.D._flat)
    d = trainer()
    ld, od = run(d, torch.from_numpy(ln), padded(obsv, ln, "repeat"))
    assert torch.equal(od, oc) and torch.equal(d.G._flat_all, c.G._flat_all) and torch.equal(d.D._flat, c.D._flat)


def test_step_with_obs_len_never_takes_the_graph():
    import socialways_amd as sw
    torch.manual_seed(32)
    tr = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0")
    assert tr.use_graph
    obsv, gt, sb = crowd(SIZES)
    z = torch.rand(B, 32)
    for _ in range(4):          # the dense step would capture on its third call
        out = tr.step(obsv, gt, sb, 0.04, 0.93, z, 1.0, obs_len=lengths("cycle"))
    assert not tr._graphs and bool(torch.isfinite(out).all())
    for bad in ([2] * (B - 1), [1] + [8] * (B - 1), [9] + [8] * (B - 1), np.full(B, 8.0)):
        with pytest.raises(ValueError, match="obs_len"):
            tr.step(obsv, gt, sb, 0.04, 0.93, z, 1.0, obs_len=bad)


# ---- 6. the epoch ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_data(tmp_path_factory):
    """The ragged synthetic recording, built the way the ragged_eval fixture of tests/test_gpu_ragged.py builds it."""
    import socialways_amd as sw
    from socialways_amd import data as Dt
    path = str(tmp_path_factory.mktemp("ragged_train") / "obsmat.txt")
    Dt.write_biwi_obsmat(path, *Dt.synth_crowd_frames())
    p_data, t_data, interval = Dt.parse_biwi(path)
    o, p, t, b, n = Dt.create_dataset_ragged(p_data, t_data, range(int(t_data[0][0]), int(t_data[-1][-1]), interval), min_past=2)
    return sw.SceneDataset(o, p, b, t, device="cuda:0", obs_len=n)


def _state(tr):
    return torch.cat([tr.G._flat_all.detach().flatten(), tr.D._flat.detach().flatten()]).clone()


def test_train_epoch_ragged_on_the_ragged_recording(ragged_data):
    import socialways_amd as sw
    data = ragged_data
    short = data.obs_len[:data.n_train_samples] < 8
    assert int(short.sum()) > 50 and int((~short).sum()) > 50

    def run(seed=41):
        torch.manual_seed(seed)
        tr = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0")
        w0 = _state(tr)
        draws = np.random.RandomState(5)
        gen = torch.Generator().manual_seed(6)

        def draw(bs):
            return float(draws.uniform(0, 0.1)), float(draws.uniform(0.9, 1.0)), torch.rand(bs, 32, generator=gen)
        res = [tr.train_epoch_ragged(data, 64, draw=draw) for _ in range(2)]
        return tr, w0, res
    tr, w0, res = run()
    assert tr.epoch == 2 and not tr._graphs
    for ade, fde, losses, sizes in res:
        assert np.isfinite([ade, fde]).all() and ade > 0 and np.isfinite(losses).all()
        assert losses.shape == (len(sizes), 9) and sum(s[0] for s in sizes) == data.n_train_samples and len(sizes) > 2
    w1 = _state(tr)
    assert bool(torch.isfinite(w1).all()) and float((w1 != w0).float().mean()) > 0.5
    tr2, w02, res2 = run()
    assert torch.equal(w02, w0) and torch.equal(_state(tr2), w1)
    for (a, f, l, s), (a2, f2, l2, s2) in zip(res, res2):
        assert (a, f, s) == (a2, f2, s2) and np.array_equal(l, l2)
    with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
        tr.train_epoch(data, 64)
    assert tr.epoch == 2 and torch.equal(_state(tr), w1)
    hist = tr.evaluate_history(data, n_gen_samples=3)
    assert np.isfinite(hist["ade_min"]) and sum(v["count"] for v in hist["by_len"].values()) == data.n_test_samples
    # a dataset without obs_len is train_epoch()'s
    plain = sw.SceneDataset(data.obsv.cpu().numpy(), data.pred.cpu().numpy(), data.the_batches, device="cuda:0")
    with pytest.raises(sw.SocialWaysHipError, match="train_epoch"):
        tr.train_epoch_ragged(plain, 64)


def test_train_epoch_ragged_with_device_noise_repeats(ragged_data):
    import socialways_amd as sw
    data = ragged_data

    def run():
        torch.manual_seed(43)
        np.random.seed(9)
        tr = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0")
        tr.noise = sw.DeviceNoise(77)
        res = tr.train_epoch_ragged(data, 64)
        return res, _state(tr), tr.noise.step
    (a, sa, na), (b, sb_, nb) = run(), run()
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3] and torch.equal(sa, sb_)
    assert na == nb == len(a[3]) and np.isfinite(a[2]).all()


def test_train_epoch_ragged_with_the_fixed_variety_loss(ragged_data):
    import socialways_amd as sw
    data = ragged_data
    torch.manual_seed(44)
    np.random.seed(10)
    tr = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0", use_variety_loss="fixed", variety_k=3)
    ade, fde, losses, sizes = tr.train_epoch_ragged(data, 64)
    assert np.isfinite(losses).all() and np.isfinite([ade, fde]).all() and tr.epoch == 1
    l2min, kmin = tr.last_variety
    assert tuple(l2min.shape) == (sizes[-1][0],) == tuple(kmin.shape) and bool(torch.isfinite(l2min).all())
    assert int(kmin.min()) >= 0 and int(kmin.max()) < 3
