"""Host side of the fused ragged training step (no GPU): sw_disc_update_ragged and sw_stage_step_ragged are declared, bound
and reject bad arguments before the device is touched; ops.disc_update / step_many / the trainers take the new keywords and
refuse what they cannot do before any device call."""
import ctypes
import inspect
import os

import pytest
import torch

from test_sample_host import declared_arguments

EARG, ESHAPE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree_on_the_new_entry_points():
    from socialways_amd import _lib as L
    lib = L.load()
    for name, n in (("sw_disc_update_ragged", 30), ("sw_stage_step_ragged", 22)):
        assert name in L.PROTOTYPES, name
        res, args = L.PROTOTYPES[name]
        assert declared_arguments(name) == len(args) == n, name
        assert res is L._i and args[-1] is L._vp
        assert hasattr(lib, name)
    # sw_disc_update's arguments without obs_pre, plus obs_len; sw_stage_step_zdev's plus obs_len_dst
    assert len(L.PROTOTYPES["sw_disc_update_ragged"][1]) == len(L.PROTOTYPES["sw_disc_update"][1]) == declared_arguments("sw_disc_update")
    assert len(L.PROTOTYPES["sw_stage_step_ragged"][1]) == len(L.PROTOTYPES["sw_stage_step_zdev"][1]) + 1
    hdr = open(os.path.join(ROOT, "include", "socialways_hip.h")).read()
    assert "#define SW_STAGE_HEADER_RAGGED 12" in hdr and "#define SW_STAGE_HEADER 8" in hdr


def _addresses():
    buf = ctypes.create_string_buffer(128)
    p = (ctypes.addressof(buf) + 15) & ~15
    arr2 = (ctypes.c_void_p * 2)(p, p)
    hole = (ctypes.c_void_p * 2)(p, None)
    return buf, p, arr2, ctypes.cast(arr2, ctypes.c_void_p), hole, ctypes.cast(hole, ctypes.c_void_p)


def test_disc_update_ragged_argument_validation_without_gpu():
    """`p` is a non-NULL address nobody dereferences: every call returns from its argument checks, B == 0 with SW_OK and no
    launch; B > 0 without registered weight images is SW_ESHAPE (sw_disc_update_supported), still before any device call."""
    from socialways_amd import _lib as L
    lib = L.load()
    _keep, p, _a, pp, _h, ph = _addresses()

    def upd(obsv=p, To=8, obs_len=p, pred4=pp, d_w=p, B=0, Tp=12, label=pp, code=pp, dsave=p, snap=None, targets=p, t0=0, t1=1,
            z=p, ddelta=p, d_d_w=p, wgrad=p, part=None, aw=None, am=None, av=None, astep=None):
        return lib.sw_disc_update_ragged(obsv, To, obs_len, pred4, d_w, B, Tp, label, code, dsave, snap, targets, t0, t1, z, 0.5, 0.25,
                                         ddelta, d_d_w, wgrad, part, aw, am, av, astep, 1e-3, 0.9, 0.999, 1e-8, None)

    def dense(obsv=p, To=8, obs_len=None, pred4=pp, d_w=p, B=0, Tp=12, label=pp, code=pp, dsave=p, snap=None, targets=p, t0=0, t1=1,
              z=p, ddelta=p, d_d_w=p, wgrad=p, part=None, aw=None, am=None, av=None, astep=None):
        return lib.sw_disc_update(obsv, To, pred4, d_w, B, Tp, label, code, dsave, 0, snap, targets, t0, t1, z, 0.5, 0.25,
                                  ddelta, d_d_w, wgrad, part, aw, am, av, astep, 1e-3, 0.9, 0.999, 1e-8, None)
    assert upd() == 0 and upd(snap=p, part=p) == 0 and upd(To=2) == 0 and upd(aw=p, am=p, av=p, astep=p) == 0
    assert upd(obs_len=None) == EARG and upd(obs_len=None, B=7) == EARG      # ... while the dense entry has none to miss
    assert dense() == 0
    bad = (dict(obsv=None), dict(pred4=None), dict(pred4=ph), dict(d_w=None), dict(label=None), dict(label=ph), dict(code=None),
           dict(code=ph), dict(dsave=None), dict(targets=None), dict(z=None), dict(ddelta=None), dict(d_d_w=None), dict(wgrad=None),
           dict(t0=-1), dict(t1=-1), dict(To=1), dict(aw=p), dict(aw=p, am=p, av=p), dict(aw=p, am=p, av=p, astep=p, d_w=p + 16))
    for kw in bad:          # the same checks as sw_disc_update, case by case
        assert upd(**kw) == EARG == dense(**kw), kw
        assert upd(B=7, **kw) == EARG == dense(B=7, **kw), kw
    # the shape rule is sw_disc_update_supported's: Tp <= 12 and registered images (none here)
    assert lib.sw_disc_update_supported(p, 7, 8, 12) == 0
    assert upd(B=7) == ESHAPE == dense(B=7) and upd(B=7, Tp=13) == ESHAPE == dense(B=7, Tp=13)
    assert upd(B=7, Tp=13, obs_len=None) == EARG            # the argument checks come first


def test_stage_step_ragged_argument_validation_without_gpu():
    from socialways_amd import _lib as L
    lib = L.load()
    _keep, p, _a, _pp, _h, _ph = _addresses()

    def stage(slot=p, B=5, To=8, Tp=12, obsv=p, pred=p, pred4=p, targets=p, z=p, steps=p, n_d=2, enc=None, dec=None, emb=None, att=None,
              img=None, d_w=None, d_img=None, d_tab=None, zdev=0, ol=p):
        return lib.sw_stage_step_ragged(slot, B, To, Tp, obsv, pred, pred4, targets, z, steps, n_d, enc, dec, emb, att, img, d_w, d_img,
                                        d_tab, zdev, ol, None)
    for kw in (dict(ol=None), dict(z=None), dict(ol=None, zdev=1), dict(z=None, zdev=1), dict(slot=None), dict(obsv=None), dict(pred=None),
               dict(pred4=None), dict(targets=None), dict(B=0), dict(To=1), dict(Tp=0), dict(n_d=-1), dict(n_d=255),
               dict(img=p), dict(img=p, enc=p, dec=p, emb=p), dict(d_img=p), dict(d_img=p, d_w=p)):
        assert stage(**kw) == EARG, kw
    # (sw_stage_step_zdev takes a NULL z_dst while z travels in the slot - the encoder launch pulls it; this entry never does)
    assert lib.sw_stage_step_zdev(p, 5, 8, 12, p, p, p, p, None, p, 2, None, None, None, None, None, None, None, None, 1, None) == EARG


def test_python_keywords_and_refusals_without_gpu():
    import socialways_amd as sw
    from socialways_amd import generic, ops, wide
    last = lambda f: list(inspect.signature(f).parameters.values())[-1]
    assert last(ops.disc_update).name == "obs_len" and last(ops.disc_update).default is None      # appended: positions unchanged
    # step_many keeps the dense call's named parameters; obs_len is the one further keyword it takes
    assert list(inspect.signature(sw.SocialWaysTrainer.step_many).parameters)[:7] == \
        ["self", "batches", "sub_batches", "ss", "global_B", "out", "global_row0"]
    with pytest.raises(TypeError, match="obs_lens"):
        sw.SocialWaysTrainer.step_many(None, [], None, obs_lens=[])
    assert last(sw.SocialWaysTrainer.__init__).name == "ragged_fused" and last(sw.SocialWaysTrainer.__init__).default is False
    assert sw.SocialWaysTrainer.ragged_fused is False
    # ops.disc_update: no precomputed observation pass for ragged rows; obs_len is an int32 (B,) tensor on obsv's device
    B, To, Tp = 5, 8, 12
    ol = torch.tensor([2, 8, 3, 5, 8], dtype=torch.int32)
    w = torch.zeros(8)
    obsv, z, pred = torch.zeros(B, To, 2), torch.zeros(B, 32), torch.zeros(B, Tp, 4)
    upd = lambda **kw: ops.disc_update(w, obsv, [pred, pred], w, (0, 1), z, 1.0, 0.5, w, None, **kw)
    with pytest.raises(ValueError, match="obs_pre"):
        upd(obs_len=ol, obs_pre=True)
    for bad in (ol[:4], ol.long(), ol.float(), ol.tolist(), ol.numpy(), ol[None]):
        with pytest.raises(ValueError, match="obs_len"):
            upd(obs_len=bad)
    with pytest.raises(sw.SocialWaysHipError, match="no CPU fallback"):
        upd(obs_len=ol)
    # step_many: one obs_len per batch or none at all - checked before anything of the trainer is touched (no trainer here)
    batches = [(obsv, pred[:, :, :2], 0.0, 1.0, z)] * 3
    for bad in ([ol, ol], [ol] * 4, [], [ol, None, ol], [None, ol, ol]):
        with pytest.raises(ValueError, match="obs_len"):
            sw.SocialWaysTrainer.step_many(None, batches, None, obs_len=bad)
    # the wide and the generic trainer take the keyword and refuse the switch, before they look at the device
    for cls, H in ((wide.WideTrainer, 128), (generic.GenericTrainer, 80)):
        with pytest.raises(sw.SocialWaysHipError, match="ragged_fused"):
            cls(12, hidden_size=H, device="cpu", ragged_fused=True)
        with pytest.raises(sw.SocialWaysHipError, match="ragged_fused"):
            sw.SocialWaysTrainer(12, hidden_size=H, device="cpu", ragged_fused=True)       # ... reached through the front door
        with pytest.raises(sw.SocialWaysHipError, match="no CPU fallback"):
            cls(12, hidden_size=H, device="cpu", ragged_fused=False)                       # False is accepted: the next refusal
