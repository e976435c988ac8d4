"""Kernel sequencing for the two differentiable functions of the reference's train():
`predict()` (train.py:392-432) and `Discriminator.forward` (train.py:294-309).

These are thin host wrappers: they own the workspaces (torch allocator), put the C-ABI calls of
include/socialways_hip.h in order on the current stream and nothing else.  Both the autograd
Functions of model.py and the fused training step of trainer.py go through them.
"""
import os

import numpy as np
import torch

from . import _lib as L
from .data import WallGrid, check_obs_len, wall_segments


class SceneIndex:
    """Device-side form of the reference's `sub_batches` ((S,2) [start,end) rows, train.py:446-461):
    int32 prefix offsets; scenes of up to AMAX agents: int64 pair offsets (n^2 per scene with n > 1) and
    their largest size; larger scenes: the row-block records of include/socialways_hip.h (`big_blocks`)."""

    def __init__(self, sub_batches, B, device):
        sb = np.asarray(sub_batches, dtype=np.int64).reshape(-1, 2)
        if len(sb) == 0:                                   # predict() default: one scene (train.py:405-406)
            sb = np.array([[0, B]], dtype=np.int64)
        if sb[0, 0] != 0 or sb[-1, 1] != B or (sb[1:, 0] != sb[:-1, 1]).any():
            raise ValueError("sub_batches must tile [0, B) contiguously")
        n = sb[:, 1] - sb[:, 0]
        if (n <= 0).any():
            raise ValueError("empty scene in sub_batches")
        self.S = len(sb)
        self.B = int(B)
        small = n <= L.AMAX
        self.amax = int(n[small].max()) if small.any() else 0      # largest one-workgroup scene
        pairs = np.where((n > 1) & small, n * n, 0)
        recs, row = [], 0
        for sc in np.nonzero(~small)[0]:                          # scenes above AMAX agents: blocks of 16 query agents
            ns = int(n[sc])
            nblk = (ns + 15) // 16
            for k in range(nblk):
                recs.append((sc, 16 * k, row + k * ns, row, nblk, k, 0, 0))
            row += nblk * ns
        self.NB, self.big_rows = len(recs), row
        self.big_blocks = torch.tensor(recs, dtype=torch.int32).reshape(-1, 8).to(device) if recs else None
        poff = np.concatenate([[0], np.cumsum(pairs)]).astype(np.int64)
        self.P = int(poff[-1])
        off = np.concatenate([sb[:, 0], [B]]).astype(np.int32)
        self.scene_off = torch.from_numpy(off).to(device)
        self.pair_off = torch.from_numpy(poff).to(device)
        self.sizes = n

    def row_scene(self):
        """(scene of every row (B,) int32, is that scene one of two or more agents (B,) bool) on the device, made once."""
        if getattr(self, "_rows", None) is None:
            sc = np.repeat(np.arange(self.S, dtype=np.int32), self.sizes)
            dev = self.scene_off.device
            self._rows = (torch.from_numpy(sc).to(dev), torch.from_numpy(np.repeat(self.sizes > 1, self.sizes)).to(dev))
        return self._rows

    _cache = {}

    @classmethod
    def get(cls, sub_batches, B, device):
        """The cached index of `sub_batches`, given as anything numpy reads as (S, 2) integer rows; [] = one scene of all B rows."""
        sb = np.ascontiguousarray(np.asarray(sub_batches, dtype=np.int64).reshape(-1, 2))
        key = (sb.tobytes(), int(B), str(device))
        hit = cls._cache.get(key)
        if hit is None:
            if len(cls._cache) > 4096:
                cls._cache.clear()
            hit = cls._cache[key] = cls(sb, B, device)
            hit.key = key
        return hit


class Workspaces:
    """Grow-only fp32 scratch buffers keyed by name (saves, deltas, split-K partials) and the host-side handle
    that lets the weight-gradient problems of one backward pass share a launch."""

    def __init__(self, device):
        self.device = device
        self.buf = {}
        self._wgb = None
        # Growth protocol: a captured step graph has the ADDRESSES of these buffers baked in.  When a larger batch
        # layout needs more space the old tensor is not released - it moves to `retired`, so graphs captured for
        # smaller layouts keep replaying on live memory - and `version` is bumped; the owner of the graphs
        # (SocialWaysTrainer) drops its graphs and then calls `release_retired()` at its next safe point.
        self.retired = []
        self.version = 0

    @property
    def wgrad_batch(self):
        if self._wgb is None:
            lib = L.load()
            self._wgb, self._free = lib.sw_wgrad_batch_new(), lib.sw_wgrad_batch_free
        return self._wgb

    def __del__(self):      # may run at interpreter shutdown, when module globals are already gone
        if getattr(self, "_wgb", None):
            self._free(self._wgb)
            self._wgb = None

    def get(self, name, nfloats):
        t = self.buf.get(name)
        if t is None or t.numel() < nfloats:
            if t is not None:
                self.retired.append(t)
                self.version += 1
            # geometric growth: ragged datasets with slowly increasing batch sizes would otherwise retire a buffer per step
            n = max(int(nfloats), 1) if t is None else max(int(nfloats), int(1.25 * t.numel()))
            t = torch.empty(n, dtype=torch.float32, device=self.device)
            self.buf[name] = t
        return t

    def release_retired(self):
        """Only when nothing captured can still reference the outgrown buffers."""
        self.retired.clear()


_default_ws = {}


def default_ws(device):
    key = str(device)
    if key not in _default_ws:
        _default_ws[key] = Workspaces(device)
    return _default_ws[key]


class GenCtx:
    __slots__ = ("obsv", "noise", "scenes", "hT", "cT", "S", "attn", "gsave", "B", "To", "Tp", "use_social", "wh", "ml", "ragged")


def _ragged_arg(obs_len, B, device, noise_src=None, d_obs=None):
    """The obs_len of the training-side calls: None or an int32 tensor (B,) on `device` (obs_len_arg makes one).  Ragged rows
    have no z pull in the encoder launch and no precomputed D observation pass."""
    if obs_len is None:
        return None
    if noise_src is not None:
        raise ValueError("obs_len: the ragged encoder launch pulls no z - noise_src must be None (the caller copies z)")
    if d_obs is not None:
        raise ValueError("obs_len: there is no precomputed observation pass for ragged rows - d_obs must be None")
    return _check_obs_len_tensor(obs_len, B, device)


SCENE_WG = True                # few small scenes: social backward + observation BPTT as one launch of a workgroup per scene (off: A/B)
SCENE_WG_MAX_AGENTS = 16       # a scene is the columns of ONE 16-agent tile
SCENE_WG_MAX_SCENES = 256      # one CU per scene workgroup (sw_scene_wg_max_scenes)
SOCIAL_ROWS_MAX_PAIRS = 256    # mean pairs per scene below which the social backward leaves per-pair rows (sw_social_rows_max_pairs)


def scene_wg(scenes, use_social, ragged=False):
    """Does the backward pass of a training step on this batch layout run sw_social_enc_bwd in place of the social-backward
    and observation-BPTT launches?  Decided once per layout: the switch and the social block are on, the histories are dense
    (ragged rows keep their launches), every scene has at most SCENE_WG_MAX_AGENTS agents, there are at most
    SCENE_WG_MAX_SCENES scenes, and the social backward is the per-pair-rows one, whose results the launch reproduces bit for
    bit (0 < P < SOCIAL_ROWS_MAX_PAIRS * S).  Part of the captured step's key."""
    return bool(SCENE_WG and use_social and not ragged and scenes.NB == 0 and 0 < scenes.amax <= SCENE_WG_MAX_AGENTS
                and scenes.S <= SCENE_WG_MAX_SCENES and 0 < scenes.P < SOCIAL_ROWS_MAX_PAIRS * scenes.S)


def _enc_save(obsv, enc_w, B, To, hT, cT, gsave, x4s_ptr, obs_len, aux, st):
    """The encoder launch of a training forward pass: the dense kernel (aux = (src, dst, n): its z pull) or, with obs_len,
    the saving ragged kernel - the same rows in the same places, zeros in front of a row's start."""
    if obs_len is None:
        L.call("sw_enc_lstm_fwd_aux", L.ptr(obsv), 0, L.ptr(enc_w), None, None, B, To, L.ptr(hT), L.ptr(cT), None,
               L.ptr(gsave), x4s_ptr, 0, aux[0], aux[1], aux[2], st)
    elif gsave is None:
        L.call("sw_enc_lstm_fwd_ragged", L.ptr(obsv), 0, L.ptr(enc_w), L.ptr(obs_len), B, To, L.ptr(hT), L.ptr(cT), st)
    else:
        L.call("sw_enc_lstm_fwd_ragged_save", L.ptr(obsv), 0, L.ptr(enc_w), L.ptr(obs_len), B, To, L.ptr(hT), L.ptr(cT),
               L.ptr(gsave), x4s_ptr, st)


def gen_forward(enc_w, emb_w, att_w, dec_w, obsv, noise, scenes, n_next, use_social, save, ws=None, tag="g", ade=None,
                noise_src=None, d_obs=None, obs_len=None):
    """predict(): encode obs (train.py:397-404), social pooling (408-413), decode loop (415-432).
    Returns pred_hat_4d (B, n_next, 4) and, if `save`, the context backward needs.
    ade = (gt (B,n_next,2), 1/ss, out (ceil(B/16),3)): the decode kernel also leaves the per-tile ADE/FDE
    partial sums of train.py:546-551 in `out`.
    noise_src: address `noise` is filled from (pinned host memory) by idle workgroups of the encoder launch.
    d_obs = (packed D weights, dsave buffer): idle workgroups of the decode launch run the discriminator's
    observation LSTM for the next disc_forward(..., save_lstm=2) on the same obsv (see d_obs_buffer).
    obs_len (B,) int32 on the device: ragged histories - row a holds obs_len[a] valid frames right-aligned in obsv and trains
    as if its encoder ran on those frames alone from the zero state (sw_enc_lstm_fwd_ragged_save in place of the encoder
    launch: zero saved rows in front of a row's start, so gen_backward is unchanged; the social block and the rollout read
    the last two frames and are the same launches).  noise_src and d_obs must be None then.  None: the dense launch."""
    obs_len = _ragged_arg(obs_len, obsv.shape[0], obsv.device, noise_src, d_obs)
    L.require_gpu(obsv)
    obsv = obsv.contiguous()
    noise = noise.contiguous()
    B, To = obsv.shape[0], obsv.shape[1]
    if noise.shape != (B, 32):
        raise ValueError("noise must be (B, 32)")
    dev = obsv.device
    st = L.stream()
    hT = torch.empty(B, 64, device=dev)
    cT = torch.empty(B, 64, device=dev)
    pred4 = torch.empty(B, n_next, 4, device=dev)
    gsave = None
    if save:   # ws=None (autograd path): a private save buffer per call, several may be alive
        nfl = L.workspace_floats(L.WS_GSAVE, B, To, n_next)
        gsave = ws.get(tag + ".gsave", nfl) if ws is not None else torch.empty(nfl, device=dev)
    # act rows live at offset 0 of gsave, x4s right behind (sw_common.h:gsave_layout)
    x4s_off = (To + n_next - 1) * B * 384
    # z (256 KB over PCIe: ~16 us, request-bound) is first read by the decode launch.  The encoder launch leaves half of
    # the CUs idle for ~20 us at the metric shape: its spare workgroups pull z for free.
    # (Dense crowds: 4 MB of z at c4 are ~170 us of request-bound PCIe reads against 113 us of encoder work.  Splitting the
    # pull over this launch and the social block's moved the cost, 168 + 148 -> 135 + 185 us: the CUs that host the pulling
    # workgroups serve their tiles / scenes late.  A caller that wants it gone hands z over in device memory.)
    z_in_enc, z_in_soc, n_enc = noise_src, None, noise.numel() if noise_src else 0
    _enc_save(obsv, enc_w, B, To, hT, cT, gsave, (gsave.data_ptr() + 4 * x4s_off) if save else None, obs_len,
              (z_in_enc, L.ptr(noise) if z_in_enc else None, n_enc), st)
    attn = wh = ml = None
    if use_social:
        S = torch.empty(B, 64, device=dev)
        attn = torch.empty(B, L.AMAX, device=dev) if save else None
        if scenes.NB:          # scenes above AMAX agents: W h + b per agent and the softmax statistics of every row
            wh = torch.empty(B * 132, device=dev)       # Wh | v | c rows of the row-block kernels (sw_social_pool_fwd)
            ml = torch.empty(B, 2, device=dev) if save else None
        L.call("sw_social_pool_fwd_aux", L.ptr(obsv), To, L.ptr(hT), L.ptr(scenes.scene_off), scenes.S, B, scenes.amax,
               L.ptr(emb_w), L.ptr(att_w), L.ptr(S), L.ptr(attn), L.ptr(scenes.big_blocks), scenes.NB, L.ptr(wh), L.ptr(ml),
               z_in_soc, (noise.data_ptr() + 4 * n_enc) if z_in_soc else None, (noise.numel() - n_enc) if z_in_soc else 0, st)
    else:
        S = torch.zeros(B, 64, device=dev)                                   # train.py:413
    L.call("sw_dec_rollout_fwd_aux", L.ptr(obsv), To, L.ptr(noise), L.ptr(S), L.ptr(hT), L.ptr(cT), L.ptr(enc_w),
           L.ptr(dec_w), B, n_next, L.ptr(pred4), None, None, L.ptr(gsave),
           L.ptr(ade[0]) if ade else None, float(ade[1]) if ade else 0.0, L.ptr(ade[2]) if ade else None,
           L.ptr(d_obs[0]) if d_obs else None, L.ptr(d_obs[1]) if d_obs else None, st)
    if not save:
        return pred4, None
    ctx = GenCtx()
    ctx.obsv, ctx.noise, ctx.scenes, ctx.hT, ctx.cT, ctx.S, ctx.attn = obsv, noise, scenes, hT, cT, S, attn
    ctx.gsave, ctx.B, ctx.To, ctx.Tp, ctx.use_social = gsave, B, To, n_next, use_social
    ctx.wh, ctx.ml, ctx.ragged = wh, ml, obs_len is not None
    return pred4, ctx


DFUSE = True     # generator-phase D pass inside the decode BPTT launch (a test compares it with the two launches)


def gen_backward(enc_w, emb_w, att_w, dec_w, ctx, dpred4, d_enc, d_emb, d_att, d_dec, ws=None, tag="g", aux=None, adam=None,
                 dfuse=None):
    """Backward of predict(): decode BPTT -> social block -> obs BPTT -> ONE grouped weight-gradient GEMM launch
    (the social block's problems ride in it).  d_* are the packed gradient buffers (overwritten).
    aux = (src, dst, mask): masked copy dst = mask > 0 ? src : dst done by idle workgroups of the decode BPTT
    launch.  (Running part of the weight GEMMs on a side stream under the BPTT was measured slower: it takes
    CUs from the latency-bound chain and every cross-stream edge of a captured graph costs 5-10 us.)
    adam = (w_all, g_all, m, v, step scalar, lr, beta1, beta2, eps): the kernels that finish the gradients also apply
    the generator's Adam update (sw_gen_wgrad_adam; the four weight / gradient buffers are views of w_all / g_all)."""
    dev = ctx.obsv.device
    ws = ws or default_ws(dev)
    B, To, Tp = ctx.B, ctx.To, ctx.Tp
    gdelta = ws.get(tag + ".gdelta", L.workspace_floats(L.WS_GDELTA, B, To, Tp))
    wgrad = ws.get("wgrad", L.workspace_floats(L.WS_WGRAD, B, To, Tp))
    tmp = ws.get(tag + ".dwx", 2048)
    dhT = torch.empty(B, 64, device=dev)
    dcT = torch.empty(B, 64, device=dev)
    dS = torch.empty(B, 64, device=dev)
    aux_late = None
    if dfuse is not None:
        # dfuse = (d_w, pred_hat, targets, t_idx, z, g_label, g_code, loss_part): the generator-phase D pass (disc_dpred) runs
        # inside the decode BPTT launch, tile by tile; that launch READS D's weights, so the masked copy that restores them
        # (aux) moves to the observation BPTT launch
        d_w, pred_hat, targets, t_idx, z, g_label, g_code, loss_part = dfuse
        dscr = ws.get(tag + ".dpred", B * Tp * 4)
        L.call("sw_dec_rollout_bwd_dfuse", L.ptr(ctx.obsv), L.ptr(pred_hat), L.ptr(d_w), L.ptr(targets), int(t_idx), L.ptr(z),
               g_label, g_code, L.ptr(loss_part), L.ptr(dscr), L.ptr(enc_w), L.ptr(dec_w), L.ptr(ctx.gsave), B, To, Tp,
               L.ptr(gdelta), L.ptr(dhT), L.ptr(dcT), L.ptr(dS), L.stream())
        aux_late = aux
    else:
        dpred4 = dpred4.contiguous()
        L.call("sw_dec_rollout_bwd_aux", L.ptr(dpred4), L.ptr(enc_w), L.ptr(dec_w), L.ptr(ctx.gsave), B, To, Tp,
               L.ptr(gdelta), L.ptr(dhT), L.ptr(dcT), L.ptr(dS), L.ptr(aux[0]) if aux else None, L.ptr(aux[1]) if aux else None,
               L.ptr(aux[2]) if aux else None, aux[1].numel() if aux else 0, L.stream())
    pending = None
    fused = scene_wg(ctx.scenes, ctx.use_social, ctx.ragged)
    if fused:
        # few small scenes: one launch, a workgroup per scene keeps dh_T + its social gradient on chip and runs the BPTT on it
        sc = ctx.scenes
        pending = ws.wgrad_batch
        pws = ws.get("pairs", L.workspace_floats(L.WS_PAIRS, B, To, Tp, 1, sc.P))
        L.call("sw_social_enc_bwd", L.ptr(ctx.obsv), To, L.ptr(ctx.hT), L.ptr(sc.scene_off), L.ptr(sc.pair_off), sc.S, B, sc.amax,
               sc.P, L.ptr(emb_w), L.ptr(att_w), L.ptr(ctx.attn), L.ptr(dS), L.ptr(dhT), L.ptr(dcT), L.ptr(d_emb), L.ptr(d_att),
               L.ptr(pws), L.ptr(wgrad), L.ptr(enc_w), L.ptr(ctx.gsave), L.ptr(gdelta),
               L.ptr(aux_late[0]) if aux_late else None, L.ptr(aux_late[1]) if aux_late else None,
               L.ptr(aux_late[2]) if aux_late else None, aux_late[1].numel() if aux_late else 0, pending, L.stream())
    elif ctx.use_social and (ctx.scenes.P > 0 or ctx.scenes.NB > 0):
        sc = ctx.scenes
        pending = ws.wgrad_batch
        pws = ws.get("pairs", L.workspace_floats(L.WS_PAIRS, B, To, Tp, 1, sc.P))
        bigp = ws.get("bigpart", sc.big_rows * 132) if sc.NB else None      # scenes above AMAX agents: per-block partial rows
        L.call("sw_social_pool_bwd", L.ptr(ctx.obsv), To, L.ptr(ctx.hT), L.ptr(sc.scene_off), L.ptr(sc.pair_off), sc.S,
               B, sc.amax, sc.P, L.ptr(emb_w), L.ptr(att_w), L.ptr(ctx.attn), L.ptr(dS), L.ptr(dhT), L.ptr(d_emb),
               L.ptr(d_att), L.ptr(pws), L.ptr(wgrad), L.ptr(sc.big_blocks), sc.NB, L.ptr(ctx.wh), L.ptr(ctx.ml),
               L.ptr(ctx.S), L.ptr(bigp), pending, L.stream())
    else:
        d_emb.zero_()
        d_att.zero_()
    if not fused:
        L.call("sw_enc_lstm_bwd_aux", L.ptr(enc_w), L.ptr(ctx.gsave), None, L.ptr(dhT), L.ptr(dcT), None, B, To, 0,
               L.ptr(gdelta), None, None, L.ptr(aux_late[0]) if aux_late else None, L.ptr(aux_late[1]) if aux_late else None,
               L.ptr(aux_late[2]) if aux_late else None, aux_late[1].numel() if aux_late else 0, L.stream())
    if adam is not None:
        w_all, g_all, m, v, step, lr, b1, b2, eps = adam
        L.call("sw_gen_wgrad_adam", L.ptr(enc_w), L.ptr(dec_w), L.ptr(ctx.gsave), L.ptr(gdelta), L.ptr(ctx.noise), L.ptr(ctx.S),
               B, To, Tp, L.ptr(d_enc), L.ptr(d_dec), L.ptr(wgrad), L.ptr(tmp), pending, L.ptr(w_all), L.ptr(m), L.ptr(v),
               L.ptr(g_all), w_all.numel(), L.ptr(step), lr, b1, b2, eps, L.stream())
        return
    L.call("sw_gen_wgrad", L.ptr(enc_w), L.ptr(dec_w), L.ptr(ctx.gsave), L.ptr(gdelta), L.ptr(ctx.noise), L.ptr(ctx.S), B, To, Tp,
           L.ptr(d_enc), L.ptr(d_dec), 0, L.ptr(wgrad), L.ptr(tmp), pending, L.stream())


class GenCtxK:
    """Context of K rollouts that share the observation encoding (gen_forward_k)."""
    __slots__ = ("one", "K", "obsv_k", "noise_k", "S_k", "gsave_k")


def gen_forward_k(enc_w, emb_w, att_w, dec_w, obsv, noise_k, scenes, n_next, use_social, K, ws, tag="gv", obs_len=None):
    """K rollouts of predict() on the SAME observations with K noise draws (the best-of-K variety term, train.py:527-536
    with its intended semantics): EncoderLstm over the observed steps and the social pooling do not depend on z, so they run
    ONCE on the B agents; only the decode loop runs on the K*B copies (copy k = rows [k*B, (k+1)*B)).
    obs_len (B,) int32 on the device: ragged histories, as gen_forward() - the one encoder launch is the saving ragged one.
    Returns pred_hat_4d (K*B, n_next, 4) and the context for gen_backward_k."""
    obs_len = _ragged_arg(obs_len, obsv.shape[0], obsv.device)
    L.require_gpu(obsv)
    obsv = obsv.contiguous()
    noise_k = noise_k.contiguous()
    B, To = obsv.shape[0], obsv.shape[1]
    KB = K * B
    if noise_k.shape != (KB, 32):
        raise ValueError("noise must be (K * B, 32)")
    dev = obsv.device
    st = L.stream()
    hT, cT = torch.empty(B, 64, device=dev), torch.empty(B, 64, device=dev)
    gsave_1 = ws.get(tag + ".gsave1", L.workspace_floats(L.WS_GSAVE, B, To, n_next))
    gsave_k = ws.get(tag + ".gsave", L.workspace_floats(L.WS_GSAVE, KB, To, n_next))
    Ta = To + n_next - 1
    _enc_save(obsv, enc_w, B, To, hT, cT, gsave_1, gsave_1.data_ptr() + 4 * Ta * B * 384, obs_len, (None, None, 0), st)
    attn = wh = ml = None
    if use_social:
        S = torch.empty(B, 64, device=dev)
        attn = torch.empty(B, L.AMAX, device=dev)
        if scenes.NB:
            wh, ml = torch.empty(B * 132, device=dev), torch.empty(B, 2, device=dev)
        L.call("sw_social_pool_fwd_aux", L.ptr(obsv), To, L.ptr(hT), L.ptr(scenes.scene_off), scenes.S, B, scenes.amax,
               L.ptr(emb_w), L.ptr(att_w), L.ptr(S), L.ptr(attn), L.ptr(scenes.big_blocks), scenes.NB, L.ptr(wh), L.ptr(ml),
               None, None, 0, st)
    else:
        S = torch.zeros(B, 64, device=dev)
    # the K copies: state / pooled context / last observed point of every agent, and the saved LSTM row of the last observed
    # step in the K*B layout (the decode BPTT and the weight-gradient rows of decode step 0 read c / h of step To - 1 there)
    obsv_k, hT_k, cT_k, S_k = obsv.repeat(K, 1, 1), hT.repeat(K, 1), cT.repeat(K, 1), S.repeat(K, 1)
    row = gsave_1[(To - 1) * B * 384: To * B * 384].view(1, B, 384)
    gsave_k[(To - 1) * KB * 384: To * KB * 384].view(K, B, 384).copy_(row.expand(K, B, 384))
    pred4 = torch.empty(KB, n_next, 4, device=dev)
    L.call("sw_dec_rollout_fwd_aux", L.ptr(obsv_k), To, L.ptr(noise_k), L.ptr(S_k), L.ptr(hT_k), L.ptr(cT_k), L.ptr(enc_w),
           L.ptr(dec_w), KB, n_next, L.ptr(pred4), None, None, L.ptr(gsave_k), None, 0.0, None, None, None, st)
    one = GenCtx()
    one.obsv, one.noise, one.scenes, one.hT, one.cT, one.S, one.attn = obsv, noise_k[:B], scenes, hT, cT, S, attn
    one.gsave, one.B, one.To, one.Tp, one.use_social, one.wh, one.ml = gsave_1, B, To, n_next, use_social, wh, ml
    one.ragged = obs_len is not None
    ctx = GenCtxK()
    ctx.one, ctx.K, ctx.obsv_k, ctx.noise_k, ctx.S_k, ctx.gsave_k = one, K, obsv_k, noise_k, S_k, gsave_k
    return pred4, ctx


def gen_backward_k(enc_w, emb_w, att_w, dec_w, ctx, dpred4_k, d_enc, d_emb, d_att, d_dec, ws, tag="gv", aux=None):
    """Backward of gen_forward_k: decode BPTT on the K*B copies, their gradients w.r.t. the shared state / pooled context
    summed over the copies (back-propagation is linear in the upstream gradient), then the social block and the observation
    BPTT ONCE on the B agents.  Weight gradients: the decode phase's problems over K*B rows (sw_gen_wgrad part 1), the
    observation phase's over B rows on top (part 2)."""
    one, K = ctx.one, ctx.K
    dev = dpred4_k.device
    B, To, Tp = one.B, one.To, one.Tp
    KB = K * B
    dpred4_k = dpred4_k.contiguous()
    gdelta_k = ws.get(tag + ".gdelta", L.workspace_floats(L.WS_GDELTA, KB, To, Tp))
    gdelta_1 = ws.get(tag + ".gdelta1", L.workspace_floats(L.WS_GDELTA, B, To, Tp))
    wgrad = ws.get("wgrad", L.workspace_floats(L.WS_WGRAD, B, To, Tp))
    tmp = ws.get(tag + ".dwx", 2048)
    dh_k, dc_k, dS_k = (torch.empty(KB, 64, device=dev) for _ in range(3))
    L.call("sw_dec_rollout_bwd_aux", L.ptr(dpred4_k), L.ptr(enc_w), L.ptr(dec_w), L.ptr(ctx.gsave_k), KB, To, Tp,
           L.ptr(gdelta_k), L.ptr(dh_k), L.ptr(dc_k), L.ptr(dS_k), L.ptr(aux[0]) if aux else None,
           L.ptr(aux[1]) if aux else None, L.ptr(aux[2]) if aux else None, aux[1].numel() if aux else 0, L.stream())
    dhT, dcT, dS = (t.view(K, B, 64).sum(0) for t in (dh_k, dc_k, dS_k))
    L.call("sw_gen_wgrad", L.ptr(enc_w), L.ptr(dec_w), L.ptr(ctx.gsave_k), L.ptr(gdelta_k), L.ptr(ctx.noise_k), L.ptr(ctx.S_k),
           KB, To, Tp, L.ptr(d_enc), L.ptr(d_dec), 1, L.ptr(wgrad), L.ptr(tmp), None, L.stream())
    pending = None
    if one.use_social and (one.scenes.P > 0 or one.scenes.NB > 0):
        sc = one.scenes
        pending = ws.wgrad_batch
        pws = ws.get("pairs", L.workspace_floats(L.WS_PAIRS, B, To, Tp, 1, sc.P))
        bigp = ws.get("bigpart", sc.big_rows * 132) if sc.NB else None
        L.call("sw_social_pool_bwd", L.ptr(one.obsv), To, L.ptr(one.hT), L.ptr(sc.scene_off), L.ptr(sc.pair_off), sc.S,
               B, sc.amax, sc.P, L.ptr(emb_w), L.ptr(att_w), L.ptr(one.attn), L.ptr(dS), L.ptr(dhT), L.ptr(d_emb),
               L.ptr(d_att), L.ptr(pws), L.ptr(wgrad), L.ptr(sc.big_blocks), sc.NB, L.ptr(one.wh), L.ptr(one.ml),
               L.ptr(one.S), L.ptr(bigp), pending, L.stream())
    else:
        d_emb.zero_()
        d_att.zero_()
    L.call("sw_enc_lstm_bwd", L.ptr(enc_w), L.ptr(one.gsave), None, L.ptr(dhT), L.ptr(dcT), None, B, To, 0,
           L.ptr(gdelta_1), None, None, L.stream())
    L.call("sw_gen_wgrad", L.ptr(enc_w), L.ptr(dec_w), L.ptr(one.gsave), L.ptr(gdelta_1), L.ptr(one.noise), L.ptr(one.S), B, To, Tp,
           L.ptr(d_enc), L.ptr(d_dec), 2, L.ptr(wgrad), L.ptr(tmp), pending, L.stream())


def obs_len_arg(obs_len, B, To, lo, device):
    """The obs_len of the model-level calls - None, an integer tensor, a numpy array or a list: valid frames per row of a
    right-aligned (B, To, .) observation buffer - checked and moved to `device` once -> int32 tensor (B,) or None.
    ValueError for a wrong shape or a non-integer dtype, and for host data (list, numpy, CPU tensor) outside lo .. To; a
    device tensor is not read back (the kernels clamp it into the range)."""
    if obs_len is None:
        return None
    if isinstance(obs_len, torch.Tensor) and obs_len.device.type != "cpu":
        if obs_len.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise ValueError("obs_len must hold integers, got dtype %s" % obs_len.dtype)
        if tuple(obs_len.shape) != (B,):
            raise ValueError("obs_len must be (B,) = (%d,), got %s" % (B, tuple(obs_len.shape)))
        return obs_len.to(device=device, dtype=torch.int32).contiguous()
    host = obs_len.numpy() if isinstance(obs_len, torch.Tensor) else obs_len
    return torch.from_numpy(check_obs_len(host, B, To, lo)).to(device)


def _check_obs_len_tensor(obs_len, B, device):
    """What gen_sample / disc_score take as obs_len: an int32 tensor (B,) on `device` (obs_len_arg makes one)."""
    if not isinstance(obs_len, torch.Tensor) or obs_len.dtype != torch.int32 or tuple(obs_len.shape) != (B,) \
            or obs_len.device != device:
        raise ValueError("obs_len must be an int32 tensor (B,) = (%d,) on %s" % (B, device))
    return obs_len.contiguous()


def _check_pred_len_tensor(pred_len, B, device, name="pred_len"):
    """What gen_sample / scene_clearance take as future lengths: an int32 tensor (B,) on `device` (SceneDataset.set_pred_len
    makes one; the kernels clamp it into 1 .. Tp)."""
    if not isinstance(pred_len, torch.Tensor) or pred_len.dtype != torch.int32 or tuple(pred_len.shape) != (B,) \
            or pred_len.device != device:
        raise ValueError("%s must be an int32 tensor (B,) = (%d,) on %s" % (name, B, device))
    return pred_len.contiguous()


_sample_img = {}      # device -> the image buffer the sampling path owns (sw_gen_images)


def gen_sample(enc_w, emb_w, att_w, dec_w, obsv, noise_k, scenes, n_next, use_social, K, gt=None, inv_ss=1.0,
               want_pred=True, keep_pred=False, pred_len=None, obs_len=None):
    """K sampled futures of predict() for B agents (test(), train.py:563-616): the encoder over the observed steps and the
    social block run ONCE on the B agents, then ONE sampling launch rolls out the K * B rows (row k * B + a = draw k of
    agent a) reading the encoding per agent - nothing is replicated.  noise_k (K * B, 32).
    gt (B, n_next, 2): the per-row errors are formed in the launch and reduced over k on the device.
    keep_pred: pred4 is written and returned although the caller wants no trajectories (want_pred False) - it stays on
    the device for a consumer there (scene_metrics).
    pred_len (B,) int32 on the device: ragged futures - row a of gt holds pred_len[a] valid frames, left-aligned, and its
    errors are the mean over those frames and the error at the last of them (sw_dec_sample_fwd_plen; the rollout and pred4
    are the dense launch's, the padding of gt reaches no output).  Needs gt.  None: the dense sampling launch.
    obs_len (B,) int32 on the device: ragged histories - row a holds obs_len[a] valid frames right-aligned in obsv and its
    encoding is that of those frames alone (sw_enc_lstm_fwd_ragged in place of the encoder launch; the social block and
    the rollout read the last frames and are the same launches).  None: the dense encoder launch.
    Returns (pred4 (K * B, n_next, 4) or None when neither want_pred nor keep_pred,
             (per_agent (B, 4) = mean_k ADE | mean_k FDE | min_k ADE | min_k FDE, best (B,) int32, err (K, B, 2)) or None).
    The launches run with the weight images registered, the protocol of the training step: derived into a buffer this path
    owns in front of them, dropped behind them on the same host thread - no image outlives a weight change."""
    L.require_gpu(obsv)
    obsv = obsv.contiguous()
    noise_k = noise_k.contiguous()
    B, To = obsv.shape[0], obsv.shape[1]
    if K < 1:
        raise ValueError("K must be at least 1")
    if noise_k.shape != (K * B, 32):
        raise ValueError("noise must be (K * B, 32)")
    want_pred = want_pred or keep_pred
    if gt is None and not want_pred:
        raise ValueError("nothing asked for: neither trajectories nor errors")
    if gt is not None:
        gt = gt.contiguous()
        if gt.shape != (B, n_next, 2):
            raise ValueError("gt must be (B, n_next, 2)")
    dev = obsv.device
    if pred_len is not None:
        if gt is None:
            raise ValueError("pred_len describes gt: it needs one")
        pred_len = _check_pred_len_tensor(pred_len, B, dev)
    if obs_len is not None:
        obs_len = _check_obs_len_tensor(obs_len, B, dev)
    st = L.stream()
    pred4 = torch.empty(K * B, n_next, 4, device=dev) if want_pred else None
    if B == 0:
        return pred4, None
    img = _sample_img.get(str(dev))
    if img is None:
        img = _sample_img[str(dev)] = torch.empty(L.load().sw_gen_image_floats(), device=dev)
    hT, cT = torch.empty(B, 64, device=dev), torch.empty(B, 64, device=dev)
    err = torch.empty(K, B, 2, device=dev) if gt is not None else None
    L.call("sw_gen_images", L.ptr(enc_w), L.ptr(dec_w), L.ptr(emb_w), L.ptr(att_w), L.ptr(img), st)
    try:
        if obs_len is None:
            L.call("sw_enc_lstm_fwd_aux", L.ptr(obsv), 0, L.ptr(enc_w), None, None, B, To, L.ptr(hT), L.ptr(cT), None,
                   None, None, 0, None, None, 0, st)
        else:
            L.call("sw_enc_lstm_fwd_ragged", L.ptr(obsv), 0, L.ptr(enc_w), L.ptr(obs_len), B, To, L.ptr(hT), L.ptr(cT), st)
        S = None                                                                 # NULL = zeros (train.py:413)
        if use_social:
            S = torch.empty(B, 64, device=dev)
            wh = torch.empty(B * 132, device=dev) if scenes.NB else None
            L.call("sw_social_pool_fwd_aux", L.ptr(obsv), To, L.ptr(hT), L.ptr(scenes.scene_off), scenes.S, B, scenes.amax,
                   L.ptr(emb_w), L.ptr(att_w), L.ptr(S), None, L.ptr(scenes.big_blocks), scenes.NB, L.ptr(wh), None,
                   None, None, 0, st)
        if pred_len is None:
            L.call("sw_dec_sample_fwd", L.ptr(obsv), To, L.ptr(noise_k), L.ptr(S), L.ptr(hT), L.ptr(cT), L.ptr(enc_w),
                   L.ptr(dec_w), B, K, n_next, L.ptr(pred4), L.ptr(gt), float(inv_ss), L.ptr(err), st)
        else:
            L.call("sw_dec_sample_fwd_plen", L.ptr(obsv), To, L.ptr(noise_k), L.ptr(S), L.ptr(hT), L.ptr(cT), L.ptr(enc_w),
                   L.ptr(dec_w), B, K, n_next, L.ptr(pred4), L.ptr(gt), L.ptr(pred_len), float(inv_ss), L.ptr(err), st)
    finally:
        L.call("sw_gen_images", None, None, None, None, None, None)
    if err is None:
        return pred4, None
    per_agent = torch.empty(B, 4, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    L.call("sw_sample_reduce", L.ptr(err), B, K, L.ptr(per_agent), L.ptr(best), st)
    return pred4, (per_agent, best, err)


def _check_pos(pos, K, B=None, score=None):
    """The K draws' positions as the scene-level wrappers take them, checked without touching the device: pos (K * B, Tp, 2 | 4)
    or (K, B, Tp, 2 | 4), x and y first, on the device of `score` when one is given -> (B, Tp, pstride).  B None: as many
    agents as pos holds - K >= 1 divides the rows of a 3-d pos (path_walls, wall_grad)."""
    sh = tuple(pos.shape)
    if B is None:
        if len(sh) not in (3, 4) or K < 1 or (len(sh) == 3 and sh[0] % K):
            raise ValueError("pos must be (K * B, Tp, 2 or 4) or (K, B, Tp, 2 or 4) with K = %d, got %s" % (K, sh))
        B = sh[1] if len(sh) == 4 else sh[0] // K
    if len(sh) not in (3, 4) or sh[-1] not in (2, 4) or sh[-2] < 1 or (sh[:2] != (K, B) if len(sh) == 4 else sh[0] != K * B):
        raise ValueError("pos must be (K * B, Tp, 2 or 4) or (K, B, Tp, 2 or 4) with K = %d, B = %d, got %s" % (K, B, sh))
    if score is not None and pos.device != score.device:
        raise ValueError("pos must be on the device of score")
    return B, sh[-2], sh[-1]


def _start_arg(start, B, device, of="pos"):
    """start (B, >= 2) or None - the point in front of the Tp positions, on `device` (that of the argument `of`) - checked without
    touching the device -> (start, sstride) as the kernels read it: float32 rows of any stride >= 2 in place (a view such as
    obsv[:, -1]), anything else as a packed copy of its first two columns; (None, 0) without one."""
    if start is None:
        return None, 0
    if start.dim() != 2 or start.shape[0] != B or start.shape[1] < 2 or start.device != device:
        raise ValueError("start must be (B, >= 2) = (%d, >= 2) on the device of %s, got %s" % (B, of, tuple(start.shape)))
    if start.dtype != torch.float32 or start.stride(1) != 1 or start.stride(0) < 2:
        start = start[:, :2].float().contiguous()
    return start, start.stride(0)


def _lens_arg(lens, B, device):
    """lens (B,) int32 on `device` or None - ragged futures, as _check_pred_len_tensor takes them."""
    return None if lens is None else _check_pred_len_tensor(lens, B, device, "lens")


def check_positive(name, v):
    """The scale of a distance (inv_ss): > 0."""
    if not float(v) > 0.0:
        raise ValueError("%s must be > 0, got %r" % (name, v))


def check_distance(name, v):
    """A threshold on a distance (coll_dist, radius, dist): >= 0."""
    if not float(v) >= 0.0:
        raise ValueError("%s must be >= 0, got %r" % (name, v))


def check_penalty_distance(d, what="the distance", fp32=True):
    """The distance of a penalty max(0, 1 - |c|^2 / d^2)^2: finite and > 0 -> float; fp32: its square and the inverse of that are
    fp32 numbers as well (what the entry points demand; the gradient calls leave that part to them)."""
    d = float(d)
    ok = d > 0.0 and np.isfinite(d)
    if ok and fp32:
        with np.errstate(over="ignore", divide="ignore"):
            d2 = np.float32(d) * np.float32(d)
            ok = d2 > 0 and np.isfinite(d2) and np.isfinite(np.float32(1) / d2)
    if not ok:
        raise ValueError("%s must be finite and > 0%s, got %r"
                         % (what, " (its square and the inverse of it fp32 numbers)" if fp32 else "", d))
    return d


def _grad_scalars(name, d, scale):
    """d0 / dw and scale of the gradient calls -> floats: the distance finite and > 0, scale finite."""
    d, scale = check_penalty_distance(d, name, fp32=False), float(scale)
    if not np.isfinite(scale):
        raise ValueError("scale must be finite, got %r" % (scale,))
    return d, scale


def _check_grad_outputs(pos, dpos, leads, loss, count, shapes):
    """What the gradient calls write: dpos float32 like pos - its leading axes one of `leads`, 2 or 4 wide, contiguous (it is
    accumulated into in place), on the device of pos - and loss float32 / count int32 or None, contiguous, one of `shapes`, on
    that device -> dstride."""
    if tuple(dpos.shape[:-1]) not in leads or dpos.shape[-1] not in (2, 4):
        raise ValueError("dpos must hold the paths and steps of pos %s, 2 or 4 wide, got %s" % (leads[0], tuple(dpos.shape)))
    if pos.dtype != torch.float32 or dpos.dtype != torch.float32:
        raise ValueError("pos and dpos must be float32")
    if not dpos.is_contiguous():
        raise ValueError("dpos is accumulated into in place: it must be contiguous")
    if dpos.device != pos.device:
        raise ValueError("dpos must be on the device of pos")
    for name, t, dt in (("loss", loss, torch.float32), ("count", count, torch.int32)):
        if t is not None and (tuple(t.shape) not in shapes or t.dtype != dt or not t.is_contiguous() or t.device != pos.device):
            raise ValueError("%s must be a contiguous %s tensor %s on the device of pos" % (name, dt, " or ".join(map(str, shapes))))
    return dpos.shape[-1]


def scene_clearance(pos, start, scenes, K, inv_ss=1.0, lens=None):
    """clear (K, B): per draw and agent the closest approach to another agent of its scene, times inv_ss; +inf in
    single-agent scenes (sw_scene_clearance).  pos (K * B, Tp, 2 | 4) or (K, B, Tp, 2 | 4), x and y first; start (B, >= 2) or
    None: the point in front of the Tp positions (any row stride: a view such as obsv[:, -1] is read in place).
    lens (B,) int32 on the device: ragged futures - agent a is present for its first lens[a] frames (in every draw), and the
    segment of a pair that ends at frame t counts only if both are present at t; +inf where nothing counts
    (sw_scene_clearance_len).  None: the dense launch."""
    B, Tp, pstride = _check_pos(pos, K, scenes.B)
    start, sstride = _start_arg(start, B, pos.device)
    lens = _lens_arg(lens, B, pos.device)
    L.require_gpu(pos)
    pos = pos.contiguous()
    clear = torch.empty(K, B, device=pos.device)
    L.call("sw_scene_clearance_len", L.ptr(pos), pstride, L.ptr_strided(start), sstride, L.ptr(scenes.scene_off), L.ptr(lens),
           scenes.S, B, K, Tp, float(inv_ss), L.ptr(clear), L.stream())                  # lens NULL: forwards to sw_scene_clearance
    return clear


def clearance_grad(pos, start, scenes, d0, scale, dpos, loss=None, count=None):
    """The scene-clearance penalty and its gradient (sw_clearance_grad): dpos[a, t, 0:2] += scale * d/d(pos[a, t]) of the sum
    over the pairs a < b of every scene and the segments of max(0, 1 - |c|^2 / d0^2)^2, c the closest approach of the pair
    within the segment (the quantity scene_clearance measures).  pos (B, Tp, 2 | 4) and dpos (B, Tp, 2 | 4), x and y
    first, contiguous; dpos is accumulated into in place and returned; columns 2 and 3 of a 4-wide dpos are not touched.
    start (B, >= 2) or None: the point in front of the Tp positions (any row stride: a view such as obsv[:, -1] is read in
    place); it is data and takes no gradient.  d0 > 0 in the units of pos.  loss (B,) float32 / count (B,) int32 or None:
    written with the agent's share of the unscaled penalty (loss.sum() = the penalty) and its number of (partner, segment)s
    closer than d0.  Rows of agents with nothing closer than d0 are not written."""
    if pos.dim() != 3:
        raise ValueError("pos must be float32 (B, Tp, 2 or 4) with B = %d, got %s" % (scenes.B, tuple(pos.shape)))
    B, Tp, pstride = _check_pos(pos, 1, scenes.B)
    dstride = _check_grad_outputs(pos, dpos, ((B, Tp),), loss, count, ((B,),))
    d0, scale = _grad_scalars("d0", d0, scale)
    start, sstride = _start_arg(start, B, pos.device)
    L.require_gpu(pos)
    pos = pos.contiguous()
    L.call("sw_clearance_grad", L.ptr(pos), pstride, L.ptr_strided(start), sstride, L.ptr(scenes.scene_off), scenes.S, B, Tp,
           d0, scale, L.ptr(dpos), dstride, L.ptr(loss), L.ptr(count), L.stream())
    return dpos


def scene_reduce(err, clear, scenes, K, coll_dist):
    """per_scene (S, 6) = joint min ADE | joint min FDE | share of colliding draws | does draw kbest collide | min_k of the
    scene's clearance | share of colliding (draw, agent), and kbest (S,) int32 (sw_scene_reduce); clear may be None."""
    L.require_gpu(err)
    err = err.contiguous()
    B = scenes.B
    if err.numel() != K * B * 2 or (clear is not None and tuple(clear.shape) != (K, B)):
        raise ValueError("err must be (K, B, 2) and clear (K, B)")
    per_scene = torch.empty(scenes.S, 6, device=err.device)
    kbest = torch.empty(scenes.S, dtype=torch.int32, device=err.device)
    L.call("sw_scene_reduce", L.ptr(err), L.ptr(clear), L.ptr(scenes.scene_off), scenes.S, B, K, float(coll_dist),
           L.ptr(per_scene), L.ptr(kbest), L.stream())
    return per_scene, kbest


def scene_metrics(err, pred4, obsv, scenes, K, n_next, inv_ss, coll_dist):
    """Scene-level metrics of K joint draws (draw k of a scene = draw k of each of its agents) behind gen_sample, two
    launches: the clearance of every (draw, agent) along pred4 (K * B, n_next, 4), each path starting at the agent's last
    observed position, and the reduction per scene.  err (K, B, 2) = the row errors of gen_sample.
    Returns (per_scene (S, 6), kbest (S,) int32, clear (K, B)) - the columns of scene_reduce."""
    return scene_metrics_len(err, pred4, obsv, scenes, K, n_next, inv_ss, coll_dist)


def scene_metrics_len(err, pred4, obsv, scenes, K, n_next, inv_ss, coll_dist, lens=None):
    """scene_metrics() with future lengths (its own argument list is pinned): lens (B,) int32 on the device - the clearance
    counts a pair's segment only while both agents are present (scene_clearance(lens=...)), and err is expected to be
    gen_sample(pred_len=...)'s.  lens None: the dense launches."""
    if pred4.shape[-2] != n_next:
        raise ValueError("pred4 must hold n_next = %d steps" % n_next)
    clear = scene_clearance(pred4, obsv[:, -1], scenes, K, inv_ss, lens=lens)
    per_scene, kbest = scene_reduce(err, clear, scenes, K, coll_dist)
    return per_scene, kbest, clear


class DiscCtx:
    __slots__ = ("dsave", "B", "To", "Tp", "nb")


D_OBS_MAX_TILES = 128      # the decode launch has idle CUs for the D observation LSTM up to this many 16-agent tiles


def d_obs_buffer(ws, B, To, Tp, nb=2, tag="d"):
    """The save buffer disc_forward(tag, nb branches) will use, or None when the decode launch has no idle CUs to
    precompute the observation LSTM in (gen_forward(d_obs=...) / disc_forward(save_lstm=2))."""
    if (B + 15) // 16 > D_OBS_MAX_TILES:
        return None
    return ws.get(tag + ".dsave", L.workspace_floats(L.WS_DSAVE, B, To, Tp, nb))


def disc_forward(d_w, obsv, preds, save, ws=None, tag="d", save_lstm=True, w_snapshot=None, obs_len=None):
    """Discriminator.forward for 1 or 2 future branches sharing the observation encoding.
    Returns ([label_k (B,1)], [code_k (B,2)], ctx).  save_lstm=2: the LSTM rows are already in the save buffer
    (gen_forward(d_obs=...)).
    obs_len (B,) int32 on the device: ragged histories - row a's observation LSTM runs over its obs_len[a] valid frames alone
    (sw_disc_fwd_ragged: zero saved rows in front of a row's start, so disc_backward* are unchanged); save_lstm=2 is
    refused then.  None: sw_disc_fwd."""
    if obs_len is not None:
        obs_len = _check_obs_len_tensor(obs_len, obsv.shape[0], obsv.device)
        if int(save_lstm) == 2:
            raise ValueError("obs_len: there is no precomputed observation pass for ragged rows - save_lstm=2 is refused")
    L.require_gpu(obsv)
    obsv = obsv.contiguous()
    preds = [p.contiguous() for p in preds]
    B, To = obsv.shape[0], obsv.shape[1]
    x_mode = {2: 0, 4: 1}[obsv.shape[2]]        # positions (B,To,2) or obsv_4d (B,To,4)
    Tp = preds[0].shape[1]
    nb = len(preds)
    dev = obsv.device
    labels = [torch.empty(B, 1, device=dev) for _ in preds]
    codes = [torch.empty(B, 2, device=dev) for _ in preds]
    dsave = None
    if save:
        nfl = L.workspace_floats(L.WS_DSAVE, B, To, Tp, nb)
        dsave = ws.get(tag + ".dsave", nfl) if ws is not None else torch.empty(nfl, device=dev)
    pp, _k1 = L.ptr_array(preds)
    lp, _k2 = L.ptr_array(labels)
    cp, _k3 = L.ptr_array(codes)
    if obs_len is None:
        L.call("sw_disc_fwd", L.ptr(obsv), To, x_mode, pp, nb, L.ptr(d_w), B, Tp, lp, cp, L.ptr(dsave), int(save_lstm),
               L.ptr(w_snapshot), L.stream())
    else:
        L.call("sw_disc_fwd_ragged", L.ptr(obsv), To, x_mode, L.ptr(obs_len), pp, nb, L.ptr(d_w), B, Tp, lp, cp, L.ptr(dsave),
               int(save_lstm), L.ptr(w_snapshot), L.stream())
    if not save:
        return labels, codes, None
    ctx = DiscCtx()
    ctx.dsave, ctx.B, ctx.To, ctx.Tp, ctx.nb = dsave, B, To, Tp, nb
    return labels, codes, ctx


def disc_score(d_w, obsv, pred4, K, want_code=True, obs_len=None):
    """Discriminator.forward on K futures per agent in ONE launch (sw_disc_score): obsv (B, To, 2 | 4) is read per agent -
    its LSTM and fc run once per 16-agent tile -, pred4 (K * B, Tp, 4) or (K, B, Tp, 4) per row (row k * B + a = draw k of
    agent a: what gen_sample returns, scored where it lies).  Returns (score (K, B) raw LSGAN score, code_hat (K, B, 2) or
    None): the bits of K calls of disc_forward on the draws, with the weight images a caller has registered or without.
    obs_len (B,) int32 on the device: ragged histories, as gen_sample() - row a's observation LSTM runs over its obs_len[a]
    valid frames alone (sw_disc_score_ragged); None: sw_disc_score."""
    if K < 1:
        raise ValueError("K must be at least 1")
    if obsv.dim() != 3 or obsv.shape[2] not in (2, 4) or (obsv.shape[2] == 2 and obsv.shape[1] < 2) or obsv.shape[1] < 1:
        raise ValueError("obsv must be (B, To >= 2, 2) or (B, To >= 1, 4), got %s" % (tuple(obsv.shape),))
    B, To = obsv.shape[0], obsv.shape[1]
    if pred4.dim() not in (3, 4) or pred4.shape[-1] != 4 or pred4.shape[-2] < 1 or pred4.numel() != K * B * pred4.shape[-2] * 4 \
            or (pred4.dim() == 4 and tuple(pred4.shape[:2]) != (K, B)):
        raise ValueError("pred4 must be (K * B, Tp, 4) or (K, B, Tp, 4) with K = %d, B = %d, got %s" % (K, B, tuple(pred4.shape)))
    if pred4.device != obsv.device:
        raise ValueError("pred4 must be on the device of obsv")
    L.require_gpu(obsv)
    if obs_len is not None:
        obs_len = _check_obs_len_tensor(obs_len, B, obsv.device)
    obsv, pred4 = obsv.float().contiguous(), pred4.float().contiguous()
    Tp = pred4.shape[-2]
    score = torch.empty(K, B, device=obsv.device)
    code = torch.empty(K, B, 2, device=obsv.device) if want_code else None
    if B == 0:
        return score, code
    x_mode = {2: 0, 4: 1}[obsv.shape[2]]
    if obs_len is None:
        L.call("sw_disc_score", L.ptr(obsv), To, x_mode, L.ptr(pred4), L.ptr(d_w), B, K, Tp, L.ptr(score), L.ptr(code), L.stream())
    else:
        L.call("sw_disc_score_ragged", L.ptr(obsv), To, x_mode, L.ptr(obs_len), L.ptr(pred4), L.ptr(d_w), B, K, Tp, L.ptr(score),
               L.ptr(code), L.stream())
    return score, code


RANK_MAX_K = 4096      # sw_sample_rank holds an agent's K scores in LDS


def _check_picks(score, K, M, err, best=None):
    """The arguments sample_rank, sample_nms and scene_compose (M None: it picks one draw per agent) share, checked without
    touching the device -> (B, best made contiguous)."""
    if score.dim() != 2 or score.shape[0] != K or K < 1:
        raise ValueError("score must be (K, B) with K = %d >= 1, got %s" % (K, tuple(score.shape)))
    B = score.shape[1]
    if M is not None and not 1 <= M <= K:
        raise ValueError("M must lie in 1 .. K = %d, got %d" % (K, M))
    if K > RANK_MAX_K:
        raise ValueError("K must be at most %d, got %d" % (RANK_MAX_K, K))
    if err is not None and (tuple(err.shape) != (K, B, 2) or err.device != score.device):
        raise ValueError("err must be (K, B, 2) = (%d, %d, 2) on the device of score, got %s" % (K, B, tuple(err.shape)))
    if best is not None:
        if err is None:
            raise ValueError("best is only used with err")
        if tuple(best.shape) != (B,) or best.dtype != torch.int32 or best.device != score.device:
            raise ValueError("best must be (B,) = (%d,) int32 on the device of score, got %s %s" % (B, tuple(best.shape), best.dtype))
        best = best.contiguous()
    return B, best


def sample_rank(score, K, M, err=None, best=None):
    """order (B, M) int32: per agent its M highest-scored draws of K, best first, equal scores by ascending k - the first M
    columns of a stable descending sort of score (K, B) over k (sw_sample_rank).  With err (K, B, 2), the row errors of
    gen_sample, also per_agent (B, 5) = ADE | FDE of the top-scored draw, min over the top M of ADE | of FDE, the rank the
    scores give draw best[a] (best (B,) int32, the min-ADE draw of gen_sample; 0 without it).  Returns (order, per_agent or None)."""
    B, best = _check_picks(score, K, M, err, best)
    L.require_gpu(score)
    score = score.float().contiguous()
    order = torch.empty(B, M, dtype=torch.int32, device=score.device)
    per_agent = None
    if err is not None:
        err = err.float().contiguous()
        per_agent = torch.empty(B, 5, device=score.device)
    if B == 0:
        return order, per_agent
    L.call("sw_sample_rank", L.ptr(score), L.ptr(err), L.ptr(best), B, K, M, L.ptr(order), L.ptr(per_agent), L.stream())
    return order, per_agent


NMS_METRICS = {"fde": 0, "ade": 1}


def sample_nms(pos, score, K, M, radius, metric="fde", scenes=None, inv_ss=1.0, err=None, best=None):
    """Diverse top-M of K draws (sw_sample_nms): greedy suppression in score order - the highest-scored draw is kept, every
    draw within `radius` of it (metric "fde": inv_ss * the distance at the last step, "ade": inv_ss * the mean distance over
    the steps) joins its mode, and so on among the rest, M times at most.  pos (K * B, Tp, 2 | 4) or (K, B, Tp, 2 | 4), x and y
    first; score (K, B).  scenes (a SceneIndex): a group is a scene - draw k of a scene is draw k of each of its agents, two
    joint draws are one mode only if every agent is within the radius, and a joint draw scores as its lowest-scored agent;
    None: every row is a group.  With G groups returns (order (G, M) int32: the kept draws, best first, -1 past count;
    count (G,) int32; weight (G, M): the share of the K draws assigned to each kept mode, rows sum to 1; assign (G, K) int32:
    the mode of every draw; per_row (B, 6) or None without err: ADE | FDE of the first pick, min over the picks of ADE | of
    FDE, the weight | the index of the mode that holds draw best[a]).  err (K, B, 2) and best (B,) int32 as gen_sample
    returns them."""
    B, best = _check_picks(score, K, M, err, best)
    if metric not in NMS_METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(NMS_METRICS), metric))
    check_distance("radius", radius)
    check_positive("inv_ss", inv_ss)
    _, Tp, pstride = _check_pos(pos, K, B, score)
    if scenes is not None and scenes.B != B:
        raise ValueError("scenes index %d rows, score has B = %d" % (scenes.B, B))
    L.require_gpu(score)
    score, pos = score.float().contiguous(), pos.float().contiguous()
    dev = score.device
    G = scenes.S if scenes is not None else B
    order = torch.empty(G, M, dtype=torch.int32, device=dev)
    count = torch.empty(G, dtype=torch.int32, device=dev)
    weight = torch.empty(G, M, device=dev)
    assign = torch.empty(G, K, dtype=torch.int32, device=dev)
    per_row = None
    if err is not None:
        err = err.float().contiguous()
        per_row = torch.empty(B, 6, device=dev)
    if B == 0:
        return order, count, weight, assign, per_row
    L.call("sw_sample_nms", L.ptr(pos), pstride, L.ptr(score), L.ptr(scenes.scene_off) if scenes is not None else None,
           G if scenes is not None else 0, B, K, Tp, M, NMS_METRICS[metric], float(inv_ss), float(radius), L.ptr(err),
           L.ptr(best), L.ptr(order), L.ptr(count), L.ptr(weight), L.ptr(assign), L.ptr(per_row), L.stream())
    return order, count, weight, assign, per_row


def scene_compose(pos, start, score, scenes, K, coll_dist, inv_ss=1.0, sweeps=8, lens=None, err=None):
    """A joint future per scene put together from the per-agent draws (sw_scene_compose): every agent starts on its
    highest-scored draw (sel0), and in up to `sweeps` sweeps over a scene's agents one that comes closer than coll_dist to
    another's selected path - inv_ss * the closest approach along the paths, both moving linearly between frames - moves to
    the draw with the fewest such conflicts, the highest score among equals, if that is fewer than it has.  Given the
    observations the draws of different agents are independent, so any such tuple is a joint sample of the generator.
    pos (K * B, Tp, 2 | 4) or (K, B, Tp, 2 | 4), x and y first; start (B, >= 2) or None: the point in front of the Tp positions
    (any row stride, as scene_clearance); score (K, B), higher = better; scenes: a SceneIndex; lens (B,) int32 on the device:
    ragged futures, as scene_clearance(lens=...); err (K, B, 2): the row errors of gen_sample.
    Returns (sel (B,) int32, sel0 (B,) int32, clear (B,): the closest approach of every agent's selected path to the other
    selected paths of its scene, +inf in single-agent scenes; per_scene (S, 4) int32: conflicting pairs under sel0 | under sel |
    agents that moved | sweeps that changed something; per_row (B, 4) or None without err: ADE | FDE of draw sel0, ADE | FDE
    of draw sel)."""
    B, _ = _check_picks(score, K, None, err)
    check_distance("coll_dist", coll_dist)
    check_positive("inv_ss", inv_ss)
    if int(sweeps) < 1:
        raise ValueError("sweeps must be at least 1, got %r" % (sweeps,))
    _, Tp, pstride = _check_pos(pos, K, B, score)
    if scenes.B != B:
        raise ValueError("scenes index %d rows, score has B = %d" % (scenes.B, B))
    start, sstride = _start_arg(start, B, score.device, "score")
    lens = _lens_arg(lens, B, score.device)
    L.require_gpu(score)
    score, pos = score.float().contiguous(), pos.float().contiguous()
    dev = score.device
    sel = torch.empty(B, dtype=torch.int32, device=dev)
    sel0 = torch.empty(B, dtype=torch.int32, device=dev)
    clear = torch.empty(B, device=dev)
    per_scene = torch.empty(scenes.S, 4, dtype=torch.int32, device=dev)
    per_row = None
    if err is not None:
        err = err.float().contiguous()
        per_row = torch.empty(B, 4, device=dev)
    if B == 0:
        return sel, sel0, clear, per_scene, per_row
    L.call("sw_scene_compose", L.ptr(pos), pstride, L.ptr_strided(start), sstride, L.ptr(score), L.ptr(scenes.scene_off),
           L.ptr(lens), scenes.S, B, K, Tp, float(inv_ss), float(coll_dist), int(sweeps), L.ptr(err), L.ptr(sel),
           L.ptr(sel0), L.ptr(clear), L.ptr(per_scene), L.ptr(per_row), L.stream())
    return sel, sel0, clear, per_scene, per_row


def _check_query_tensor(t, Q, device, name):
    """What plan_risk takes per query: an int32 tensor (Q,) on `device`."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (Q,) or t.device != device:
        raise ValueError("%s must be an int32 tensor (Q,) = (%d,) on %s" % (name, Q, device))
    return t.contiguous()


def _check_queries(pos, Tp, plans, plan_start, q_scene, q_ego, plan_lens=None):
    """What plan_risk and plan_refine take per query, checked without touching the device: plans float32 (Q, P >= 1, Tp, 2) or
    (P, Tp, 2) for Q = 1, plan_start (Q, 2) or None, q_scene and, when given, q_ego and plan_lens int32 (Q,), all on the device of
    pos -> (plans (Q, P, Tp, 2), plan_start float32 contiguous, q_scene, q_ego, plan_lens, Q, P)."""
    if not isinstance(plans, torch.Tensor) or plans.dtype != torch.float32 or plans.dim() not in (3, 4) or plans.device != pos.device:
        raise ValueError("plans must be a float32 tensor (Q, P, Tp, 2) or (P, Tp, 2) on the device of pos")
    if plans.dim() == 3:
        plans = plans.unsqueeze(0)
    Q, P = plans.shape[0], plans.shape[1]
    if P < 1 or tuple(plans.shape[2:]) != (Tp, 2):
        raise ValueError("plans must be (Q, P >= 1, Tp, 2) with Tp = %d, got %s" % (Tp, tuple(plans.shape)))
    if plan_start is not None:
        if not isinstance(plan_start, torch.Tensor) or tuple(plan_start.shape) != (Q, 2) or plan_start.device != pos.device:
            raise ValueError("plan_start must be (Q, 2) = (%d, 2) on the device of pos" % Q)
        plan_start = plan_start.float().contiguous()
    q_scene = _check_query_tensor(q_scene, Q, pos.device, "q_scene")
    if q_ego is not None:
        q_ego = _check_query_tensor(q_ego, Q, pos.device, "q_ego")
    if plan_lens is not None:
        plan_lens = _check_query_tensor(plan_lens, Q, pos.device, "plan_lens")
    return plans.contiguous(), plan_start, q_scene, q_ego, plan_lens, Q, P


def plan_risk(pos, start, scenes, K, plans, plan_start, q_scene, q_ego, coll_dist, inv_ss=1.0, lens=None, plan_lens=None):
    """The risk of candidate ego paths against the K sampled futures of a scene (sw_plan_risk): how likely is a plan - a path
    that is NOT one of the draws - to come closer than coll_dist to somebody, inv_ss * the closest approach along the paths,
    both moving linearly between frames.  The draws are open-loop: the pedestrians do not react to the plan.
    pos (K * B, Tp, 2 | 4) or (K, B, Tp, 2 | 4), x and y first; start (B, >= 2) or None: the point in front of the Tp positions
    (any row stride, as scene_clearance); scenes: a SceneIndex; lens (B,) int32 on the device: ragged futures, as
    scene_clearance(lens=...).  Query q names scene q_scene[q] (int32 (Q,) on the device), an ego row q_ego[q] to leave out
    (int32 (Q,) or None; an absolute row of the batch; -1 or a row outside the scene: nobody) and P plans: plans (Q, P, Tp, 2),
    or (P, Tp, 2) for Q = 1, float32; plan_start (Q, 2), given exactly when start is: the point in front of the plans of
    query q; plan_lens (Q,) int32 or None: a segment counts only while both the agent and the plan are present.
    Returns (risk (Q, P): 1 - the product over the scene's other agents of the share of each agent's draws that stay clear of
    the plan - given the observations the agents' draws are independent, so this is the share of all K^n tuples; exactly 0 / 1
    when no draw / every draw of some agent conflicts;  clear_min (Q, P): the closest approach to any draw of any agent, +inf
    without one;  counts (Q, P, 4) int32: draws k in which some agent's draw k conflicts (the index-paired estimate is
    counts[..., 0] / K) | the frame at which the earliest conflicting segment ends, -1 without | the absolute row with the most
    conflicting draws, the lowest of equal ones, -1 without | that row's number of conflicting draws)."""
    B, Tp, pstride = _check_pos(pos, K, scenes.B)
    check_distance("coll_dist", coll_dist)
    check_positive("inv_ss", inv_ss)
    if (start is None) != (plan_start is None):
        raise ValueError("start and plan_start go together: a point in front of the paths and of the plans, or of neither")
    plans, plan_start, q_scene, q_ego, plan_lens, Q, P = _check_queries(pos, Tp, plans, plan_start, q_scene, q_ego, plan_lens)
    start, sstride = _start_arg(start, B, pos.device)
    lens = _lens_arg(lens, B, pos.device)
    L.require_gpu(pos)
    pos = pos.float().contiguous()
    dev = pos.device
    risk = torch.empty(Q, P, device=dev)
    clear_min = torch.empty(Q, P, device=dev)
    counts = torch.empty(Q, P, 4, dtype=torch.int32, device=dev)
    if Q == 0:
        return risk, clear_min, counts
    L.call("sw_plan_risk", L.ptr(pos), pstride, L.ptr_strided(start), sstride, L.ptr(scenes.scene_off), L.ptr(lens), scenes.S, B,
           K, Tp, L.ptr(plans), L.ptr(plan_start), L.ptr(plan_lens), L.ptr(q_scene), L.ptr(q_ego), Q, P, float(inv_ss),
           float(coll_dist), L.ptr(risk), L.ptr(clear_min), L.ptr(counts), L.stream())
    return risk, clear_min, counts


DESCENT_DEFAULTS = dict(n_iter=32, lr=0.1, w_track=0.05, w_smooth=0.5, max_move=0.5)


def check_walls(walls, device=None):
    """The map of a call, checked without touching the device: walls (M, 2, 2) float32 - the segments [w0, w1] in the
    coordinates of the paths, M = 0 .. 1024 (SW_WALLS_MAX), on `device` when one is given -> (walls contiguous, M)."""
    if not isinstance(walls, torch.Tensor) or walls.dtype != torch.float32 or walls.dim() != 3 or tuple(walls.shape[1:]) != (2, 2):
        raise ValueError("walls must be a float32 tensor (M, 2, 2): the segments [w0, w1]")
    if device is not None and walls.device != device:
        raise ValueError("walls must be on the device of pos")
    M = walls.shape[0]
    if M > L.WALLS_MAX:
        raise ValueError("a call takes at most %d walls, got %d" % (L.WALLS_MAX, M))
    return walls.contiguous(), M


def walls_arg(walls, device):
    """The map as the layers above take it - a tensor (SceneDataset.walls_from_world) or host data, (M, 2, 2) or (M, 4), M = 0
    included, in the coordinates of the paths - checked without touching the device -> float32 (M, 2, 2) on `device`."""
    if isinstance(walls, WallGrid):                           # the indexed form passes through: it was checked when it was built
        return check_wall_grid_arg(walls, L.indexed_device(device))
    w = torch.as_tensor(walls if isinstance(walls, torch.Tensor) else np.asarray(walls), dtype=torch.float32)
    return check_walls(wall_segments(w))[0].to(device)


def check_wall_grid_arg(grid, device, within=None, what="the distance"):
    """A WallGrid as the map of a call, checked without touching the device: its tensors on `device`, and `within` - the
    distance the call asks about, in the walls' coordinates, as the entry sees it - below the grid's reach by the relative
    margin 1e-5 (sw_path_walls_grid) -> the grid."""
    if grid.device != device:
        raise ValueError("the WallGrid must be on the device of pos, got %s and %s" % (grid.device, device))
    if within is not None and not float(within) <= grid.reach * (1.0 - 1e-5):
        raise ValueError("%s %r is not below the reach %r of the WallGrid (by a relative 1e-5): build the grid with a larger reach"
                         % (what, float(within), grid.reach))
    return grid


def refuse_wall_grid(walls, what):
    """The refinement keeps its walls in LDS: a call that feeds it refuses a WallGrid, before anything is sampled or launched."""
    if isinstance(walls, WallGrid):
        raise ValueError("%s does not take a WallGrid: the refinement keeps its walls in LDS (a tensor of at most %d walls)"
                         % (what, L.WALLS_MAX))


def _grid_c_args(g):
    """walls, M and the grid as sw_path_walls_grid / sw_wall_grad_grid take them"""
    return (L.ptr(g.walls), g.M, L.ptr(g.cell_ptr), L.ptr(g.cell_walls), L.ptr(g.wall_cells), g.nx, g.ny, g.origin[0], g.origin[1],
            g.inv_cell, g.reach)


def path_walls(pos, start, K, walls, dist, inv_ss=1.0, lens=None):
    """The clearance of paths - the K draws, true futures, ego plans - to a static map of line segments (sw_path_walls), one
    launch for all K * B paths.  pos (K * B, Tp, 2 | 4) or (K, B, Tp, 2 | 4), x and y first; start (B, >= 2) or None: the point
    in front of the Tp positions (any row stride, as scene_clearance), giving Tp segments instead of Tp - 1; walls (M, 2, 2)
    float32 on the device of pos, M = 0 .. 1024: the segments [w0, w1] in the coordinates of pos, a zero-length one being a
    post; lens (B,) int32 on the device: ragged futures, as scene_clearance(lens=...).  Within a segment the path point moves
    linearly and the wall stands still.
    Returns (clear (K, B): inv_ss * the smallest distance to any wall, +inf without walls or counted segments; first (K, B)
    int32: the frame at which the first segment closer than dist ends, -1 without; nseg (K, B) int32: the (segment, wall) pairs
    closer than dist)."""
    B, Tp, pstride = _check_pos(pos, K)
    check_distance("dist", dist)
    check_positive("inv_ss", inv_ss)
    grid = walls if isinstance(walls, WallGrid) else None
    if grid is not None:
        check_wall_grid_arg(grid, pos.device, float(np.float32(dist)) / float(np.float32(inv_ss)), "dist / inv_ss")
    else:
        walls, M = check_walls(walls, pos.device)
    start, sstride = _start_arg(start, B, pos.device)
    lens = _lens_arg(lens, B, pos.device)
    L.require_gpu(pos)
    pos = pos.float().contiguous()
    clear = torch.empty(K, B, device=pos.device)
    first = torch.empty(K, B, dtype=torch.int32, device=pos.device)
    nseg = torch.empty(K, B, dtype=torch.int32, device=pos.device)
    if B == 0:
        return clear, first, nseg
    if grid is not None:
        L.call("sw_path_walls_grid", L.ptr(pos), pstride, L.ptr_strided(start), sstride, L.ptr(lens), K, B, Tp, *_grid_c_args(grid),
               float(inv_ss), float(dist), L.ptr(clear), L.ptr(first), L.ptr(nseg), L.stream())
        return clear, first, nseg
    L.call("sw_path_walls", L.ptr(pos), pstride, L.ptr_strided(start), sstride, L.ptr(lens), K, B, Tp, L.ptr(walls), M,
           float(inv_ss), float(dist), L.ptr(clear), L.ptr(first), L.ptr(nseg), L.stream())
    return clear, first, nseg


def wall_grad(pos, start, K, walls, dw, scale, dpos, loss=None, count=None, lens=None):
    """The wall penalty and its gradient (sw_wall_grad): dpos[r, t, 0:2] += scale * d/d(pos[r, t]) of the sum over the path's
    counted segments and the M walls of max(0, 1 - |c|^2 / dw^2)^2, c the closest approach of the segment to the wall (the
    quantity path_walls measures).  pos and dpos (K * B, Tp, 2 | 4) or (K, B, Tp, 2 | 4), float32, x and y first; dpos is
    contiguous, accumulated into in place and returned; columns 2 and 3 of a 4-wide dpos are not touched.  start (B, >= 2) or
    None: the point in front of the Tp positions (any row stride: a view such as obsv[:, -1] is read in place); it is data and
    takes no gradient.  walls (M, 2, 2) float32 on the device of pos, M = 0 .. 1024; dw > 0 in the units of pos; lens (B,)
    int32 on the device: ragged futures, as path_walls(lens=...).  loss float32 / count int32, (K, B) or (K * B,), or None:
    written with the path's unscaled penalty and its number of (segment, wall)s closer than dw.  Rows of paths with nothing
    closer than dw - every row when M = 0 - are not written."""
    B, Tp, pstride = _check_pos(pos, K)
    dstride = _check_grad_outputs(pos, dpos, ((K * B, Tp), (K, B, Tp)), loss, count, ((K, B), (K * B,)))
    dw, scale = _grad_scalars("dw", dw, scale)
    grid = walls if isinstance(walls, WallGrid) else None
    if grid is not None:
        check_wall_grid_arg(grid, pos.device, float(np.float32(dw)), "dw")
    else:
        walls, M = check_walls(walls, pos.device)
    start, sstride = _start_arg(start, B, pos.device)
    lens = _lens_arg(lens, B, pos.device)
    L.require_gpu(pos)
    pos = pos.contiguous()
    if B == 0:
        return dpos
    if grid is not None:
        L.call("sw_wall_grad_grid", L.ptr(pos), pstride, L.ptr_strided(start), sstride, L.ptr(lens), K, B, Tp, *_grid_c_args(grid),
               dw, scale, L.ptr(dpos), dstride, L.ptr(loss), L.ptr(count), L.stream())
        return dpos
    L.call("sw_wall_grad", L.ptr(pos), pstride, L.ptr_strided(start), sstride, L.ptr(lens), K, B, Tp, L.ptr(walls), M, dw, scale,
           L.ptr(dpos), dstride, L.ptr(loss), L.ptr(count), L.stream())
    return dpos


def check_descent(d0, n_iter=32, lr=0.1, w_track=0.05, w_smooth=0.5, max_move=0.5, **wall):
    """The descent parameters of plan_refine, checked on the host before anything is sampled or launched -> (d0, n_iter, lr,
    w_track, w_smooth, max_move).  Beyond what sw_plan_refine itself refuses: the quadratic part of the objective must be
    stable: lr (2 w_track + 32 w_smooth) < 2 (the largest eigenvalue of the acceleration operator is 16; below 1 no mode of
    the quadratic part overshoots, between 1 and 2 the stiffest ones alternate while they decay).  The wall term of
    plan_refine(walls=...) is bounded and not quadratic: it leaves the rule as it is; its keywords wall_d0 (> 0, finite, its
    square and the inverse fp32 numbers) and w_wall (>= 0, finite) are checked here when given and are not returned."""
    if set(wall) - {"wall_d0", "w_wall"}:
        raise TypeError("check_descent() got unexpected keyword arguments %s" % sorted(set(wall) - {"wall_d0", "w_wall"}))
    if wall.get("wall_d0") is not None:
        check_penalty_distance(wall["wall_d0"], "the wall distance")
    if "w_wall" in wall and not (float(wall["w_wall"]) >= 0.0 and np.isfinite(float(wall["w_wall"]))):
        raise ValueError("w_wall must be finite and >= 0, got %r" % (wall["w_wall"],))
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or not 0 <= int(n_iter) <= 1024:
        raise ValueError("n_iter must be an integer in 0 .. 1024, got %r" % (n_iter,))
    d0 = check_penalty_distance(d0)
    vals = dict(lr=float(lr), w_track=float(w_track), w_smooth=float(w_smooth), max_move=float(max_move))
    for name, v in vals.items():
        if not (v >= 0.0 and np.isfinite(v)):
            raise ValueError("%s must be finite and >= 0, got %r" % (name, v))
    if not vals["lr"] * (2.0 * vals["w_track"] + 32.0 * vals["w_smooth"]) < 2.0:
        raise ValueError("unstable descent: lr (2 w_track + 32 w_smooth) must be < 2, got %r"
                         % (vals["lr"] * (2.0 * vals["w_track"] + 32.0 * vals["w_smooth"]),))
    return d0, int(n_iter), vals["lr"], vals["w_track"], vals["w_smooth"], vals["max_move"]


def plan_refine(pos, start, scenes, K, plans, plan_start, q_scene, q_ego, d0, inv_ss=1.0, lens=None, n_iter=32, lr=0.1,
                w_track=0.05, w_smooth=0.5, max_move=0.5, walls=None, wall_d0=None, w_wall=1.0):
    """Candidate ego paths moved away from the K sampled futures of a scene (sw_plan_refine): n_iter steps of gradient descent,
    all in one launch, on  J(X) = the expected clearance penalty - per pedestrian draw and segment max(0, 1 - |c|^2 / d0^2)^2 of
    the closest approach c, averaged over the K draws; given the observations the agents' draws are independent, so this is
    the mean over all K^n joint futures -  + (w_track / d0^2) sum |x_t - x0_t|^2  + (w_smooth / d0^2) sum |x_{t+1} - 2 x_t +
    x_{t-1}|^2.  Every iteration moves all waypoints by lr d0^2 dJ/dx_t, no waypoint further than max_move d0.  The draws are
    open-loop: the pedestrians do not react to the plan.
    pos, start, scenes, K, plans, plan_start, q_scene, q_ego, inv_ss, lens as ops.plan_risk, but start and plan_start are
    REQUIRED (the start point is data and does not move) and there are no plan_lens.  d0 > 0 in the coordinates of pos; lr,
    w_track, w_smooth, max_move are dimensionless, lr (2 w_track + 32 w_smooth) < 2.
    Returns (refined (Q, P, Tp, 2); cost (Q, P, 2, 3): before | after x expected penalty | sum |x - x0|^2 / d0^2 | sum |acc|^2 /
    d0^2, unweighted; moved (Q, P): inv_ss * the largest displacement of a waypoint).  n_iter = 0 returns the plans' bits.
    walls (M, 2, 2) float32 on the device of pos, M = 0 .. 1024 (as path_walls): the objective gains  w_wall * the sum over the
    plan's segments and the walls of max(0, 1 - |c|^2 / wall_d0^2)^2, c the closest approach of the moving waypoint to the
    wall - no 1 / K: walls are certain - inside the same single launch (sw_plan_refine_walls), and cost is (Q, P, 2, 4) with the
    unweighted wall sum last.  wall_d0 (default d0) in the coordinates of pos; w_wall >= 0.  The wall gradient is exactly 0
    where a segment of the plan CROSSES a wall (c = 0): descent cannot undo a crossing - crossings are reported (path_walls),
    not repaired.  walls=None: the launch without walls and its (Q, P, 2, 3) cost; an empty tensor takes the new entry point
    and returns the same bits in refined, moved and cost[..., :3]."""
    B, Tp, pstride = _check_pos(pos, K, scenes.B)
    M = -1
    refuse_wall_grid(walls, "plan_refine")
    if walls is not None:
        wall_d0 = float(d0 if wall_d0 is None else wall_d0)
        check_descent(d0, n_iter, lr, w_track, w_smooth, max_move, wall_d0=wall_d0, w_wall=w_wall)
        walls, M = check_walls(walls, pos.device)
    d0, n_iter, lr, w_track, w_smooth, max_move = check_descent(d0, n_iter, lr, w_track, w_smooth, max_move)
    check_positive("inv_ss", inv_ss)
    if K > 4096 or Tp > 1024:
        raise ValueError("plan_refine takes K <= 4096 draws and Tp <= 1024 steps, got K = %d, Tp = %d" % (K, Tp))
    if start is None or plan_start is None:
        raise ValueError("plan_refine needs a start point in front of the paths (start) and of the plans (plan_start)")
    plans, plan_start, q_scene, q_ego, _, Q, P = _check_queries(pos, Tp, plans, plan_start, q_scene, q_ego)
    start, sstride = _start_arg(start, B, pos.device)
    lens = _lens_arg(lens, B, pos.device)
    L.require_gpu(pos)
    pos = pos.float().contiguous()
    dev = pos.device
    refined = torch.empty(Q, P, Tp, 2, device=dev)
    cost = torch.empty(Q, P, 2, 3 if walls is None else 4, device=dev)
    moved = torch.empty(Q, P, device=dev)
    if Q == 0:
        return refined, cost, moved
    if walls is not None:
        L.call("sw_plan_refine_walls", L.ptr(pos), pstride, L.ptr_strided(start), sstride, L.ptr(scenes.scene_off), L.ptr(lens),
               scenes.S, B, K, Tp, L.ptr(plans), L.ptr(plan_start), L.ptr(q_scene), L.ptr(q_ego), Q, P, float(inv_ss), d0, n_iter,
               lr, w_track, w_smooth, max_move, L.ptr(walls), M, wall_d0, float(w_wall), L.ptr(refined), L.ptr(cost),
               L.ptr(moved), L.stream())
        return refined, cost, moved
    L.call("sw_plan_refine", L.ptr(pos), pstride, L.ptr_strided(start), sstride, L.ptr(scenes.scene_off), L.ptr(lens), scenes.S, B,
           K, Tp, L.ptr(plans), L.ptr(plan_start), L.ptr(q_scene), L.ptr(q_ego), Q, P, float(inv_ss), d0, n_iter, lr, w_track,
           w_smooth, max_move, L.ptr(refined), L.ptr(cost), L.ptr(moved), L.stream())
    return refined, cost, moved


def disc_backward(d_w, ctx, dlabels, dcodes, d_d_w=None, want_dpred=(), ws=None, tag="d"):
    """Backward of Discriminator.forward.  d_d_w (packed, overwritten) None = no weight gradients;
    want_dpred[k] True = return d loss / d pred4 of branch k."""
    dev = dlabels[0].device
    ws = ws or default_ws(dev)
    B, To, Tp, nb = ctx.B, ctx.To, ctx.Tp, ctx.nb
    dlabels = [t.contiguous() for t in dlabels]
    dcodes = [t.contiguous() for t in dcodes]
    want = list(want_dpred) + [False] * (nb - len(want_dpred))
    dpreds = [torch.empty(B, Tp, 4, device=dev) if w else None for w in want]
    ddelta = wgrad = None
    if d_d_w is not None:
        ddelta = ws.get(tag + ".ddelta", L.workspace_floats(L.WS_DDELTA, B, To, Tp, nb))
        wgrad = ws.get("wgrad", L.workspace_floats(L.WS_WGRAD, B, To, Tp))
    lp, _k1 = L.ptr_array(dlabels)
    cp, _k2 = L.ptr_array(dcodes)
    dp, _k3 = L.ptr_array(dpreds)
    L.call("sw_disc_bwd", L.ptr(d_w), L.ptr(ctx.dsave), lp, cp, nb, B, To, Tp, L.ptr(ddelta), L.ptr(d_d_w), dp,
           L.ptr(wgrad), L.stream())
    return dpreds


def disc_dpred(d_w, obsv, pred_hat, targets, t_idx, z, g_label, g_code, loss_part=None, obs_len=None):
    """Generator phase: D(obsv, pred_hat) forward + the backward of its prediction heads in one launch;
    returns d(g_loss)/d(pred_hat) (B,Tp,4).  obs_len (B,) int32 on the device: ragged histories, as disc_forward()
    (sw_disc_dpred_ragged); None: sw_disc_dpred."""
    if obs_len is not None:
        obs_len = _check_obs_len_tensor(obs_len, obsv.shape[0], obsv.device)
    L.require_gpu(obsv)
    obsv, pred_hat = obsv.contiguous(), pred_hat.contiguous()
    B, To, Tp = obsv.shape[0], obsv.shape[1], pred_hat.shape[1]
    x_mode = {2: 0, 4: 1}[obsv.shape[2]]
    dpred = torch.empty(B, Tp, 4, device=obsv.device)
    if obs_len is None:
        L.call("sw_disc_dpred", L.ptr(obsv), To, x_mode, L.ptr(pred_hat), L.ptr(d_w), B, Tp, L.ptr(targets), int(t_idx), L.ptr(z),
               g_label, g_code, L.ptr(dpred), None, None, L.ptr(loss_part), L.stream())
    else:
        L.call("sw_disc_dpred_ragged", L.ptr(obsv), To, x_mode, L.ptr(obs_len), L.ptr(pred_hat), L.ptr(d_w), B, Tp, L.ptr(targets),
               int(t_idx), L.ptr(z), g_label, g_code, L.ptr(dpred), None, None, L.ptr(loss_part), L.stream())
    return dpred


def disc_dpred_supported(Tp):
    """Does the generator-phase D pass (disc_dpred, gen_backward(dfuse=...)) fit one workgroup's LDS at this horizon?
    (Tp <= 24; longer horizons form d/dpred with disc_forward + disc_backward_gan.)"""
    return bool(L.load().sw_disc_dpred_supported(int(Tp)))


def disc_backward_gan(d_w, ctx, labels, codes, targets, t_idx, z, g_label, g_code, d_d_w=None, want_dpred=(), ws=None,
                      tag="d", loss_part=None, adam=None):
    """disc_backward with the LSGAN / InfoGAN loss gradients formed inside the kernel from the forward
    outputs `labels` / `codes` (targets = device [2] label-noise scalars, t_idx = target index per branch).
    loss_part (ceil(B/16),3): receives the per-tile sums of the squared errors (the reported MSE terms)."""
    dev = labels[0].device
    ws = ws or default_ws(dev)
    B, To, Tp, nb = ctx.B, ctx.To, ctx.Tp, ctx.nb
    want = list(want_dpred) + [False] * (nb - len(want_dpred))
    dpreds = [torch.empty(B, Tp, 4, device=dev) if w else None for w in want]
    ddelta = wgrad = None
    if d_d_w is not None:
        ddelta = ws.get(tag + ".ddelta", L.workspace_floats(L.WS_DDELTA, B, To, Tp, nb))
        wgrad = ws.get("wgrad", L.workspace_floats(L.WS_WGRAD, B, To, Tp))
    lp, _k1 = L.ptr_array(labels)
    cp, _k2 = L.ptr_array(codes)
    dp, _k3 = L.ptr_array(dpreds)
    t0, t1 = (list(t_idx) + [0])[:2]
    if adam is not None:      # (m, v, step scalar, lr, beta1, beta2, eps): the update rides in the gradient reduction
        m, v, step, lr, b1, b2, eps = adam
        L.call("sw_disc_bwd_gan_adam", L.ptr(d_w), L.ptr(ctx.dsave), lp, cp, L.ptr(targets), t0, t1, L.ptr(z), g_label, g_code,
               nb, B, To, Tp, L.ptr(ddelta), L.ptr(d_d_w), dp, L.ptr(wgrad), L.ptr(loss_part), L.ptr(d_w), L.ptr(m), L.ptr(v),
               L.ptr(step), float(lr), float(b1), float(b2), float(eps), L.stream())
        return dpreds
    L.call("sw_disc_bwd_gan", L.ptr(d_w), L.ptr(ctx.dsave), lp, cp, L.ptr(targets), t0, t1, L.ptr(z), g_label, g_code, nb,
           B, To, Tp, L.ptr(ddelta), L.ptr(d_d_w), dp, L.ptr(wgrad), L.ptr(loss_part), L.stream())
    return dpreds


def disc_update_supported(d_w, B, To, Tp):
    """Can one discriminator update pass run as ONE launch (sw_disc_update: shapes that leave CUs idle, registered images)?"""
    return bool(L.load().sw_disc_update_supported(L.ptr(d_w), int(B), int(To), int(Tp)))


def disc_update(d_w, obsv, preds, targets, t_idx, z, g_label, g_code, d_d_w, ws, tag="d", obs_pre=False, w_snapshot=None,
                loss_part=None, adam=None, obs_len=None):
    """disc_forward(obsv, [fake, real]) + disc_backward_gan(...) of one D update (train.py:476-495) as one launch
    (sw_disc_update) + the weight-gradient GEMM (+ the Adam update).  Returns (labels, codes).
    obs_len (B,) int32 on the device: ragged histories, as disc_forward() - sw_disc_update_ragged, the bits of
    disc_forward(obs_len=) + disc_backward_gan(); there is no precomputed observation pass for ragged rows, so obs_pre is
    refused then.  None: sw_disc_update."""
    if obs_len is not None:
        obs_len = _check_obs_len_tensor(obs_len, obsv.shape[0], obsv.device)
        if obs_pre:
            raise ValueError("obs_len: there is no precomputed observation pass for ragged rows - obs_pre=True is refused")
    L.require_gpu(obsv)
    obsv = obsv.contiguous()
    preds = [p.contiguous() for p in preds]
    B, To, Tp = obsv.shape[0], obsv.shape[1], preds[0].shape[1]
    dev = obsv.device
    labels = [torch.empty(B, 1, device=dev) for _ in preds]
    codes = [torch.empty(B, 2, device=dev) for _ in preds]
    dsave = ws.get(tag + ".dsave", L.workspace_floats(L.WS_DSAVE, B, To, Tp, 2))
    ddelta = ws.get(tag + ".ddelta", L.workspace_floats(L.WS_DDELTA, B, To, Tp, 2))
    wgrad = ws.get("wgrad", L.workspace_floats(L.WS_WGRAD, B, To, Tp))
    pp, _k1 = L.ptr_array(preds)
    lp, _k2 = L.ptr_array(labels)
    cp, _k3 = L.ptr_array(codes)
    m = v = step = None
    lr = b1 = b2 = eps = 0.0
    if adam is not None:
        m, v, step, lr, b1, b2, eps = adam
    tail = (L.ptr(w_snapshot), L.ptr(targets), int(t_idx[0]), int(t_idx[1]), L.ptr(z), g_label, g_code, L.ptr(ddelta), L.ptr(d_d_w),
            L.ptr(wgrad), L.ptr(loss_part), L.ptr(d_w) if adam is not None else None, L.ptr(m), L.ptr(v), L.ptr(step), float(lr),
            float(b1), float(b2), float(eps), L.stream())
    if obs_len is None:
        L.call("sw_disc_update", L.ptr(obsv), To, pp, L.ptr(d_w), B, Tp, lp, cp, L.ptr(dsave), int(bool(obs_pre)), *tail)
    else:
        L.call("sw_disc_update_ragged", L.ptr(obsv), To, L.ptr(obs_len), pp, L.ptr(d_w), B, Tp, lp, cp, L.ptr(dsave), *tail)
    return labels, codes
