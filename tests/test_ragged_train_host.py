"""Host side of training on ragged observation histories (no GPU): the three training entry points are declared and bound
and reject bad arguments before the device is touched; step / gen_forward / gen_forward_k / disc_forward / disc_dpred take
obs_len last; train_epoch_ragged exists on the three trainers (the wide and the generic one refuse), train_epoch still
refuses a ragged dataset; and the comparison the GPU tests rest on - "all-zero saved rows in front of a row's start + the
dense BPTT" equals autograd through the per-length runs of tests/_ragged_ref.py - holds in float64 on the CPU."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

import sw_oracle as O
from _ragged_ref import bptt_zero_rows, disc_obs_ragged, encode_ragged, length_groups
from _ref64 import _f64
from test_sample_host import declared_arguments

EARG, ESHAPE = -1, -2


def test_header_and_binding_agree_on_the_training_entry_points():
    from socialways_amd import _lib as L
    lib = L.load()
    for name, n in (("sw_enc_lstm_fwd_ragged_save", 11), ("sw_disc_fwd_ragged", 15), ("sw_disc_dpred_ragged", 18)):
        assert name in L.PROTOTYPES, name
        res, args = L.PROTOTYPES[name]
        assert declared_arguments(name) == len(args) == n, name
        assert res is L._i and args[-1] is L._vp
        assert hasattr(lib, name)
    # obs_len sits between x_mode and pred4, as in sw_disc_score_ragged: one argument more than the dense entries
    assert len(L.PROTOTYPES["sw_disc_fwd_ragged"][1]) == len(L.PROTOTYPES["sw_disc_fwd"][1]) + 1
    assert len(L.PROTOTYPES["sw_disc_dpred_ragged"][1]) == len(L.PROTOTYPES["sw_disc_dpred"][1]) + 1


def test_argument_validation_without_gpu():
    """`p` is a non-NULL address nobody dereferences (the pointer arrays hold it too): every call returns from its argument
    checks, B == 0 with SW_OK and no launch."""
    from socialways_amd import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(128)
    p = (ctypes.addressof(buf) + 15) & ~15
    arr2 = (ctypes.c_void_p * 2)(p, p)
    pp = ctypes.cast(arr2, ctypes.c_void_p)
    hole = (ctypes.c_void_p * 2)(p, None)
    ph = ctypes.cast(hole, ctypes.c_void_p)

    def enc(x=p, x_mode=0, enc_w=p, obs_len=p, B=0, T=8, hT=p, cT=p, act=p, x4s=p):
        return lib.sw_enc_lstm_fwd_ragged_save(x, x_mode, enc_w, obs_len, B, T, hT, cT, act, x4s, None)
    assert enc() == 0 and enc(obs_len=None) == 0 and enc(x_mode=1) == 0 and enc(T=2) == 0 and enc(x_mode=1, T=1) == 0
    for kw in (dict(x=None), dict(enc_w=None), dict(hT=None), dict(cT=None), dict(act=None), dict(x4s=None), dict(B=-1), dict(T=0),
               dict(T=-3), dict(x_mode=2), dict(x_mode=-1), dict(T=1)):
        assert enc(**kw) == EARG, kw
        if "B" not in kw:
            assert enc(B=7, **kw) == EARG, kw
            assert enc(B=7, obs_len=None, **kw) == EARG, kw

    def fwd(obsv=p, To=8, x_mode=0, obs_len=p, pred4=pp, nb=2, d_w=p, B=0, Tp=12, label=pp, code=pp, dsave=p, save_lstm=1, snap=None):
        return lib.sw_disc_fwd_ragged(obsv, To, x_mode, obs_len, pred4, nb, d_w, B, Tp, label, code, dsave, save_lstm, snap, None)

    def fwd_dense(obsv=p, To=8, x_mode=0, obs_len=None, pred4=pp, nb=2, d_w=p, B=0, Tp=12, label=pp, code=pp, dsave=p, save_lstm=1,
                  snap=None):
        return lib.sw_disc_fwd(obsv, To, x_mode, pred4, nb, d_w, B, Tp, label, code, dsave, save_lstm, snap, None)
    assert fwd() == 0 and fwd(obs_len=None) == 0 and fwd(save_lstm=0) == 0 and fwd(nb=1) == 0 and fwd(dsave=None, save_lstm=0) == 0
    assert fwd(x_mode=1, To=1) == 0 and fwd(To=2) == 0 and fwd(Tp=64) == 0 and fwd(snap=p) == 0
    bad = (dict(obsv=None), dict(pred4=None), dict(d_w=None), dict(label=None), dict(code=None), dict(nb=0), dict(nb=3), dict(B=-1),
           dict(To=0), dict(Tp=0), dict(x_mode=2), dict(x_mode=-1), dict(To=1), dict(save_lstm=-1), dict(save_lstm=3),
           dict(pred4=ph), dict(label=ph), dict(code=ph))
    for kw in bad:      # the same checks as sw_disc_fwd, case by case
        assert fwd(**kw) == EARG == fwd_dense(**kw), kw
        if "B" not in kw:
            assert fwd(B=7, **kw) == EARG == fwd_dense(B=7, **kw), kw
    # save_lstm = 2: the dense entry reads a precomputed observation pass, the ragged one has none
    assert fwd_dense(save_lstm=2) == 0
    assert fwd(save_lstm=2) == EARG and fwd(save_lstm=2, B=7) == EARG and fwd(save_lstm=2, obs_len=None) == EARG
    assert fwd(Tp=65) == ESHAPE == fwd_dense(Tp=65) and fwd(B=7, Tp=65) == ESHAPE
    assert fwd(Tp=65, nb=0) == EARG                        # the argument checks come first

    def dpred(obsv=p, To=8, x_mode=0, obs_len=p, pred4=p, d_w=p, B=0, Tp=12, targets=p, t_idx=1, z=p, dpred4=p, label=None,
              code=None, part=None):
        return lib.sw_disc_dpred_ragged(obsv, To, x_mode, obs_len, pred4, d_w, B, Tp, targets, t_idx, z, 0.5, 0.25, dpred4, label,
                                        code, part, None)

    def dpred_dense(obsv=p, To=8, x_mode=0, obs_len=None, pred4=p, d_w=p, B=0, Tp=12, targets=p, t_idx=1, z=p, dpred4=p, label=None,
                    code=None, part=None):
        return lib.sw_disc_dpred(obsv, To, x_mode, pred4, d_w, B, Tp, targets, t_idx, z, 0.5, 0.25, dpred4, label, code, part, None)
    assert dpred() == 0 and dpred(obs_len=None) == 0 and dpred(label=p, code=p, part=p) == 0 and dpred(x_mode=1, To=1) == 0
    assert dpred(Tp=24) == 0 and dpred(Tp=64) == 0         # B == 0 returns before the LDS size is looked at, as sw_disc_dpred
    for kw in (dict(obsv=None), dict(pred4=None), dict(d_w=None), dict(targets=None), dict(z=None), dict(dpred4=None), dict(B=-1),
               dict(To=0), dict(Tp=0), dict(t_idx=-1), dict(x_mode=2), dict(x_mode=-1), dict(To=1)):
        assert dpred(**kw) == EARG == dpred_dense(**kw), kw
        if "B" not in kw:
            assert dpred(B=7, **kw) == EARG == dpred_dense(B=7, **kw), kw
    assert dpred(Tp=65) == ESHAPE == dpred_dense(Tp=65)
    assert dpred(B=7, Tp=25) == ESHAPE == dpred_dense(B=7, Tp=25)      # the pass does not fit one workgroup's LDS from Tp = 25 on


def test_obs_len_is_the_last_parameter_of_the_training_calls():
    import socialways_amd as sw
    from socialways_amd import ops
    last = lambda f: list(inspect.signature(f).parameters.values())[-1]
    for f in (sw.SocialWaysTrainer.step, ops.gen_forward, ops.gen_forward_k, ops.disc_forward, ops.disc_dpred):
        assert last(f).name == "obs_len" and last(f).default is None, f      # appended: the positions in front are unchanged
    names = list(inspect.signature(sw.SocialWaysTrainer.step).parameters)
    assert names[-2] == "variety_noise"
    for f in (ops.gen_backward, ops.gen_backward_k, ops.disc_backward, ops.disc_backward_gan, sw.SocialWaysTrainer.step_many):
        assert "obs_len" not in inspect.signature(f).parameters, f           # the backward side needs no change
    assert list(inspect.signature(sw.SocialWaysTrainer.train_epoch_ragged).parameters) == \
        list(inspect.signature(sw.SocialWaysTrainer.train_epoch).parameters) == ["self", "data", "batch_size", "draw"]


def test_ops_refuse_what_a_ragged_pass_cannot_do():
    """With an obs_len: noise_src, d_obs and save_lstm=2 are ValueErrors, and so is an obs_len that is not an int32 (B,)
    tensor on the device of obsv - all before the device is looked at (a well-formed call on CPU tensors gets as far as
    the "no CPU fallback" refusal)."""
    import socialways_amd as sw
    from socialways_amd import ops
    B, To, Tp = 5, 8, 12
    ol = torch.tensor([2, 8, 3, 5, 8], dtype=torch.int32)
    w = torch.zeros(8)
    obsv, z, pred = torch.zeros(B, To, 2), torch.zeros(B, 32), torch.zeros(B, Tp, 4)
    gen = lambda **kw: ops.gen_forward(w, w, w, w, obsv, z, None, Tp, True, True, **kw)
    with pytest.raises(ValueError, match="noise_src"):
        gen(obs_len=ol, noise_src=4096)
    with pytest.raises(ValueError, match="d_obs"):
        gen(obs_len=ol, d_obs=(w, w))
    with pytest.raises(ValueError, match="save_lstm"):
        ops.disc_forward(w, obsv, [pred], save=True, save_lstm=2, obs_len=ol)
    calls = (lambda o: gen(obs_len=o), lambda o: ops.gen_forward_k(w, w, w, w, obsv, z.repeat(3, 1), None, Tp, True, 3, None, obs_len=o),
             lambda o: ops.disc_forward(w, obsv, [pred], save=False, obs_len=o),
             lambda o: ops.disc_dpred(w, obsv, pred, w, 1, z, 1.0, 0.5, obs_len=o))
    for call in calls:
        for bad in (ol[:4], ol.long(), ol.float(), ol.tolist(), ol.numpy(), ol[None]):
            with pytest.raises(ValueError, match="obs_len"):
                call(bad)
        with pytest.raises(sw.SocialWaysHipError, match="no CPU fallback"):
            call(ol)


def test_train_epoch_ragged_on_the_three_trainers():
    import socialways_amd as sw
    from socialways_amd import generic, wide
    ragged = types.SimpleNamespace(obs_len=torch.tensor([2, 8], dtype=torch.int32))
    plain = types.SimpleNamespace(obs_len=None)
    me = types.SimpleNamespace()
    for cls in (sw.SocialWaysTrainer, generic.GenericTrainer, wide.WideTrainer):
        assert callable(cls.train_epoch_ragged)
        with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
            cls.train_epoch(me, ragged, 64)                     # as before: train_epoch() refuses a ragged dataset
    for cls in (generic.GenericTrainer, wide.WideTrainer):      # no ragged kernels on these paths: refused, no device needed
        for d in (ragged, plain):
            with pytest.raises(sw.SocialWaysHipError, match="obs_len"):
                cls.train_epoch_ragged(me, d, 64)
    # a dataset without obs_len belongs to train_epoch(), and the message says so
    with pytest.raises(sw.SocialWaysHipError, match=r"obs_len.*train_epoch\(\)"):
        sw.SocialWaysTrainer.train_epoch_ragged(me, plain, 64)
    with pytest.raises(sw.SocialWaysHipError, match=r"obs_len.*train_epoch\(\)"):
        sw.SocialWaysTrainer.train_epoch_ragged(me, types.SimpleNamespace(), 64)
    # train_epoch()'s refusal names the new call
    with pytest.raises(sw.SocialWaysHipError, match="train_epoch_ragged"):
        sw.SocialWaysTrainer.train_epoch(me, ragged, 64)


def test_held_out_can_build_a_training_set_in_another_datasets_coordinates():
    import socialways_amd as sw
    t = sw.synth_tracks(6, [3, 1, 4, 2, 5, 2], seed=5)
    like = sw.SceneDataset(t["obsvs"], t["preds"], t["batches"], t["times"], device="cpu")
    rows = np.arange(0, 8)
    ln = np.array([2, 8, 3, 8, 8, 5, 8, 8], dtype=np.int32)
    ev = sw.SceneDataset.held_out(like, t["obsvs"][rows], t["preds"][rows], t["batches"][:3], t["times"][rows], ln)
    trn = sw.SceneDataset.held_out(like, t["obsvs"][rows], t["preds"][rows], t["batches"][:3], t["times"][rows], ln, train=True)
    assert ev.n_train_samples == 0 and ev.n_test_samples == 8 and len(list(ev.packed_steps(64))) == 0
    assert trn.n_train_samples == 8 and trn.n_test_samples == 0 and len(trn.test_batches) == 0
    assert np.array_equal(trn.train_batches, t["batches"][:3]) and trn.ss == like.ss and trn.scale is like.scale
    assert torch.equal(trn.obsv, like.obsv[:8]) and torch.equal(trn.obs_len, torch.from_numpy(ln))
    assert [(a, b, sb.tolist()) for a, b, sb in trn.packed_steps(4)] == [(0, 4, [[0, 3], [3, 4]]), (4, 8, [[0, 4]])]
    assert [(a, b) for a, b, _ in trn.packed_steps(64)] == [(0, 8)]


# ---- the comparison itself, in float64 on the CPU ----------------------------------------------------------------------------
B, To, H = 37, 8, 64


def _lengths():
    ln = (np.arange(B) % (To - 1)) + 2          # 2 .. To row by row
    ln[16:20] = 2
    ln[20:24] = To
    return ln.astype(np.int32)


def _positions(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, To, 2, generator=g, dtype=torch.float64) * 0.1).cumsum(1), \
        torch.randn(B, H, generator=g, dtype=torch.float64), torch.randn(B, H, generator=g, dtype=torch.float64)


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("which", ["encoder", "discriminator"])
def test_zero_saved_rows_and_the_dense_bptt_give_the_per_length_gradients(which):
    """The oracle's LSTM at mixed lengths.  Reference: autograd through the per-length runs of _ragged_ref (no padding
    exists there).  Candidate: bptt_zero_rows - every row runs all To steps, selects the zero state and saves an all-zero
    row in front of its start, and the dense backward (lstm_cell_bwd's formulas, the dense weight-gradient sums) runs over
    everything.  Both to 1e-12 relative; the dgates rows and saved inputs in front of each start are exactly zero, and the
    padding (NaN here) is never read."""
    ln = _lengths()
    assert sorted(n for n, _ in length_groups(ln)) == list(range(2, To + 1))
    obsv, dh, dc = _positions(7)
    torch.manual_seed(11)
    with _f64():
        if which == "encoder":
            mod = O.EncoderLstm(H, 1).double()
            lstm, embed = mod.lstm, (mod.embed.weight.detach(), mod.embed.bias.detach())
            hT, cT, _ = encode_ragged(mod, obsv, ln)
            (hT * dh).sum().add((cT * dc).sum()).backward()
        else:
            mod = O.Discriminator(12, H, 2).double()
            lstm, embed = mod.obsv_encoder_lstm, None
            hT = disc_obs_ragged(mod, obsv, ln)
            cT, dc = None, torch.zeros_like(dc)                # D reads the last output only
            (hT * dh).sum().backward()
    nan_pad = obsv.clone()
    for r, n in enumerate(ln):
        nan_pad[r, :To - n] = float("nan")
    w = {k: getattr(lstm, k + "_l0").detach() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    h2, c2, grads, dgates, x4s = bptt_zero_rows(w["weight_ih"], w["weight_hh"], w["bias_ih"], w["bias_hh"], nan_pad, ln, dh, dc, embed)
    assert _rel(h2, hT.detach()) <= 1e-12
    if cT is not None:
        assert _rel(c2, cT.detach()) <= 1e-12
    for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
        ref = getattr(lstm, k + "_l0").grad
        assert float(ref.abs().max()) > 0 and bool(torch.isfinite(grads[k]).all())
        assert _rel(grads[k], ref) <= 1e-12, (k, _rel(grads[k], ref))
    if embed is not None:
        assert _rel(grads["embed.weight"], mod.embed.weight.grad) <= 1e-12
        assert _rel(grads["embed.bias"], mod.embed.bias.grad) <= 1e-12
    n_front = 0
    for r, n in enumerate(ln):
        s = To - int(n)
        assert not bool(dgates[:s, r].any()) and not bool(x4s[:s, r].any()), (r, n)       # exactly zero, sign aside
        assert bool(dgates[s:, r].any(1).all()), (r, n)                                   # ... and only there
        n_front += s
    assert n_front > 2 * B
    # the selects matter: the same dense backward on rows computed THROUGH the padding (the first valid frame repeated,
    # nothing selected) is a different gradient
    rep = obsv.clone()
    for r, n in enumerate(ln):
        rep[r, :To - n] = obsv[r, To - n]
    _, _, dense, _, _ = bptt_zero_rows(w["weight_ih"], w["weight_hh"], w["bias_ih"], w["bias_hh"], rep, np.full(B, To), dh, dc, embed)
    assert _rel(dense["weight_hh"], lstm.weight_hh_l0.grad) > 1e-3
