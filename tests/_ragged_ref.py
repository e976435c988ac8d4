"""Shared builders of the tests of training on ragged observation histories (test_ragged_train_host.py,
test_gpu_ragged_train.py): the reference with autograd on, in the dtype of its inputs (float64 in every caller).

The method is that of `oracle_ragged` in tests/test_gpu_ragged.py: per history length the oracle's EncoderLstm (and the
oracle discriminator's LSTM) runs on the truncated rows `obsv[idx, To - n:]` from the zero state - no padding exists on this
side -, the states are scattered back into batch order, and the block-diagonal social pool, predict()'s decode loop and the
discriminator's heads run on the whole batch.  Everything stays differentiable, so tests/_ref64.py (run64, pick_fewest,
close_grads_branch_consistent) takes these functions as it takes orc.predict / orc.D.

`bptt_zero_rows` is the other side of the host comparison: the formulation the device code uses - every row runs every
step, a row in front of its start SELECTS the zero state and saves an all-zero row, and the DENSE backward (the formulas of
lstm_cell_bwd, csrc/sw_lstm_dev.h) runs over all To steps of all rows - written out in torch without autograd."""
import numpy as np
import torch

import sw_oracle as O


def length_groups(ln):
    """[(n, LongTensor of the rows with n valid frames)] in ascending n."""
    ln = np.asarray(ln)
    return [(int(n), torch.from_numpy(np.flatnonzero(ln == n))) for n in np.unique(ln)]


def gather_groups(parts, idxs):
    """Per-group row blocks -> batch order (differentiable: one cat, one index)."""
    order = torch.cat(idxs)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(len(order))
    return torch.cat(parts)[inv]


def encode_ragged(enc, obsv, ln):
    """The oracle's EncoderLstm per history length on the truncated positions, from the zero state ->
    (hT (B, H), cT (B, H), last 4-d state (B, 4))."""
    To, H = obsv.shape[1], enc.hidden_size
    hs, cs, ls, idxs = [], [], [], []
    for n, idx in length_groups(ln):
        o4 = O.get_traj_4d(obsv[idx, To - n:], [])
        enc.init_lstm(torch.zeros(1, len(idx), H, dtype=obsv.dtype), torch.zeros(1, len(idx), H, dtype=obsv.dtype))
        enc(o4)
        hs.append(enc.lstm_h[0][0])
        cs.append(enc.lstm_h[1][0])
        ls.append(o4[:, -1])
        idxs.append(idx)
    return gather_groups(hs, idxs), gather_groups(cs, idxs), gather_groups(ls, idxs)


def predict_ragged(orc, obsv, ln, noise, n_next, sub_batches=[]):
    """orc.predict() (train.py:392-432) with every row encoded over its ln[row] valid frames alone; the social pool and
    the decode loop are predict()'s.  Leaves orc.last like predict() (+ "cT").  -> pred_hat_4d (B, n_next, 4)."""
    bs = obsv.shape[0]
    enc = orc.encoder
    hT, cT, last4 = encode_ragged(enc, obsv, ln)
    if len(sub_batches) == 0:
        sub_batches = [[0, bs]]
    if orc.use_social:
        S = O.social_pool_blockdiag(last4, hT, sub_batches, orc.feature_embedder, orc.attention)
    else:
        S = torch.zeros_like(hT)
    enc.init_lstm(hT.unsqueeze(0), cT.unsqueeze(0))
    last, steps = last4, []
    for _ in range(n_next):
        v = orc.decoder(enc.lstm_h[0].view(bs, -1), S.view(bs, -1), noise).view(bs, 2)
        last = torch.cat([v + last[:, :2], v], dim=1)
        steps.append(last)
        enc(last)
    orc.last["hT"], orc.last["cT"], orc.last["S"] = hT, cT, S
    return torch.stack(steps, 1)


def disc_obs_ragged(D, obsv, ln):
    """The last output of the oracle discriminator's observation LSTM per history length, from the zero state (B, H).
    obsv (B, To, 2): positions, the 4-d states formed on the valid frames; (B, To, 4): 4-d states as they are."""
    To = obsv.shape[1]
    hs, idxs = [], []
    for n, idx in length_groups(ln):
        cut = obsv[idx, To - n:]
        o4 = O.get_traj_4d(cut, []) if obsv.shape[2] == 2 else cut
        z = torch.zeros(1, len(idx), D.lstm_dim, dtype=obsv.dtype)
        y, _ = D.obsv_encoder_lstm(o4, (z, z.clone()))
        hs.append(y[:, -1])
        idxs.append(idx)
    return gather_groups(hs, idxs)


def disc_ragged(D, obsv, ln, pred):
    """Discriminator.forward (train.py:294-309) with the observation encoded per history length -> (label, code_hat)."""
    obsv_code = D.obsv_encoder_fc(disc_obs_ragged(D, obsv, ln))
    pred_code = D.pred_encoder(pred.reshape(-1, D.n_next * 4))
    both = torch.cat([obsv_code, pred_code], dim=1)
    return D.classifier(both), D.latent_decoder(both)


# ---- the device formulation, in torch: selected zero rows + the dense BPTT -----------------------------------------------------
def x4_from(obsv, ln, t):
    """The 4-d input of step t as the ragged loop forms it (obs_x4_load_from): the time index clamped to the row's start
    s = To - n, the first-frame rule v_s := v_{s+1} at s.  Nothing in front of s is indexed.  obsv (B, To, 2) -> (B, 4)."""
    B, To = obsv.shape[0], obsv.shape[1]
    s = To - torch.as_tensor(np.asarray(ln), dtype=torch.long)
    r = torch.arange(B)
    te = torch.clamp(torch.full((B,), t, dtype=torch.long), min=s)
    tt = torch.where(te == s, s + 1, te)
    return torch.cat([obsv[r, te], obsv[r, tt] - obsv[r, tt - 1]], dim=1)


def bptt_zero_rows(w_ih, w_hh, b_ih, b_hh, obsv, ln, dhT, dcT, embed=None):
    """Forward of a one-layer LSTM (gate order i f g o) over positions obsv (B, To, 2) where row b starts from the zero state
    at step s_b = To - ln[b], saving per step the SELECTED row (gates | c | h and the 4-d input from s_b on, zeros in front),
    then the DENSE backward over all To steps of all rows with the formulas of lstm_cell_bwd and the weight-gradient sums
    of the dense kernels.  embed = (W (H, 4), b (H,)): the encoder's Linear in front of the LSTM, else the 4-d input feeds
    w_ih (the discriminator).  No autograd.  -> (hT, cT, {name: gradient}, dgates (To, B, 4H), saved x4s (To, B, 4))."""
    B, To, H = obsv.shape[0], obsv.shape[1], w_hh.shape[1]
    s = To - torch.as_tensor(np.asarray(ln), dtype=torch.long)
    zero = torch.zeros(B, H, dtype=obsv.dtype)
    h, c = zero, zero
    gates, cs, hs, xs = [], [], [], []
    with torch.no_grad():
        for t in range(To):
            x = x4_from(obsv, ln, t)
            inp = x @ embed[0].t() + embed[1] if embed is not None else x
            pre = inp @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
            i, f, g, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), \
                torch.sigmoid(pre[:, 3 * H:])
            cn = f * c + i * g
            hn = o * torch.tanh(cn)
            on = (t >= s)[:, None]
            c, h = torch.where(on, cn, zero), torch.where(on, hn, zero)
            gates.append(torch.where(on, torch.cat([i, f, g, o], 1), torch.zeros(B, 4 * H, dtype=obsv.dtype)))
            xs.append(torch.where(on, x, torch.zeros(B, 4, dtype=obsv.dtype)))
            cs.append(c)
            hs.append(h)
        hT, cT = h, c
        # dense BPTT over the saved rows: lstm_cell_bwd, then dh_{t-1} = dgates W_hh
        dh, dc = dhT.clone(), dcT.clone()
        dgates = [None] * To
        for t in range(To - 1, -1, -1):
            i, f, g, o = (gates[t][:, k * H:(k + 1) * H] for k in range(4))
            cprev = cs[t - 1] if t > 0 else zero
            tc = torch.tanh(cs[t])
            d_o = dh * tc
            dct = dh * o * (1.0 - tc * tc) + dc
            dg = torch.cat([dct * g * i * (1.0 - i), dct * cprev * f * (1.0 - f), dct * i * (1.0 - g * g), d_o * o * (1.0 - o)], 1)
            dc = dct * f
            dh = dg @ w_hh
            dgates[t] = dg
        dgates = torch.stack(dgates)
        x4s = torch.stack(xs)
        # weight gradients: sums over (t, b) of dgates (x) (input | h_{t-1})
        dg2 = dgates.reshape(To * B, 4 * H)
        grads = {"weight_hh": dgates[1:].reshape(-1, 4 * H).t() @ torch.stack(hs[:-1]).reshape(-1, H) if To > 1
                 else torch.zeros_like(w_hh)}
        grads["bias_ih"] = grads["bias_hh"] = dg2.sum(0)
        x2 = x4s.reshape(To * B, 4)
        if embed is not None:
            emb = x2 @ embed[0].t() + embed[1]
            demb = dg2 @ w_ih
            grads["weight_ih"] = dg2.t() @ emb
            grads["embed.weight"], grads["embed.bias"] = demb.t() @ x2, demb.sum(0)
        else:
            grads["weight_ih"] = dg2.t() @ x2
    return hT, cT, grads, dgates, x4s
