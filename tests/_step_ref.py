"""The float64 training step: what SocialWaysTrainer.step() / step_many() / _train_epoch() are held to by
test_step_ref_host.py (CPU), test_gpu_step_reference.py (one process) and test_gpu_step_dp_reference.py (process groups), and
WideTrainer.step() / GenericTrainer.step() by test_gpu_wide_step_reference.py: the info term's mean runs over the latent-code
count of the discriminator handed in (`n_codes`: 2 on the fused path), and `wide_grads` / `tap_updates` / `generic_grads` read
those two engines' gradients in the reference's names and shapes.

The reference is the oracle's modules (oracle/sw_oracle.py) cast to double and loaded from the trainer's state_dicts
(`oracle_of`), run through the arithmetic of SocialWaysOracle.train_step() (oracle/sw_oracle.py:372-475) WITHOUT the optimizer
steps (`step64`): with lr_g = lr_d = 0 the trainer's weights never move (wg_adam_fin: w - 0 * m / denom = w), so the U + 1
discriminator passes and the generator phase of every step of an epoch differentiate at the same known weights, and one
float64 evaluation of the full packed batch gives every gradient the step forms.  Ragged histories replace orc.predict / orc.D
by predict_ragged / disc_ragged of tests/_ragged_ref.py.  Gradients are taken by tests/_ref64.run64, so a (Leaky)ReLU input
within MARGIN of 0 - in the generator's modules or in D's, the generator loss passes through D - is handled by
close_grads_branch_consistent as everywhere else; the seed rule is _ref64.pick_fewest over SEEDS (`pick_draws`).

Shard semantics (`global_B`, `global_row0`): the loss of rows [r0, r1) of a packed batch of Bg agents is the batch's loss
restricted to those rows - every mean divides by Bg, agent 19 of the as-written variety term is row 19 - r0 of the shard, if
it lies in it - so the shard losses and gradients add up to the full batch's (test_step_ref_host.py checks this to 1e-12)."""
import contextlib
import copy
from types import SimpleNamespace

import numpy as np
import torch

import sw_oracle as O
import _ragged_ref as RR
from _ref64 import G_NAMES, RefRun, _f64, count_ambiguous, gen_mods, gen_params, pick_fewest, recording, run64

W_INFO, W_L2 = 0.5, 0.5     # the constructor defaults of loss_info_w / loss_l2_w (train.py:65, 69)
NL = 2                      # latent codes of the fused path, and of any discriminator that does not say otherwise


def flags(U=1, info=True, l2=False, variety=False, variety_k=20):
    """The switches of a step: unrolling depth, info loss, L2 term, variety term False / True (train.py:527-536 as written) /
    "fixed" (best of variety_k)."""
    assert variety in (False, True, "fixed")
    return SimpleNamespace(U=int(U), info=bool(info), l2=bool(l2), variety=variety, variety_k=int(variety_k))


def trainer_kw(f):
    """The constructor arguments of SocialWaysTrainer / SocialWaysOracle that `f` stands for."""
    return dict(n_unrolling_steps=f.U, use_info_loss=f.info, use_l2_loss=f.l2, use_variety_loss=f.variety, variety_k=f.variety_k)


def n_codes(D):
    """The latent-code count of a discriminator: the width of its latent_decoder's last layer, as _ref64.wide_oracle64 reads
    it; NL where D has no such layer."""
    try:
        return int(D.latent_decoder[2].out_features)
    except (AttributeError, IndexError, TypeError):
        return NL


def oracle_of(G, D, Tp, hidden_size=64, use_social=True, dtype=torch.float64):
    """The oracle with the weights of G (anything that has the four generator modules: a trainer's G, an oracle) and of the
    discriminator D - whose latent-code count it takes -, in `dtype` - float64: built under _f64() and cast, as _pair /
    wide_oracle64 do."""
    with (_f64() if dtype == torch.float64 else contextlib.nullcontext()):
        orc = O.SocialWaysOracle(Tp, hidden_size=hidden_size, use_social=use_social, n_latent_codes=n_codes(D))
    for name, src in [(n, getattr(G, n)) for n in G_NAMES] + [("D", D)]:
        m = getattr(orc, name).to(dtype)
        m.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in src.state_dict().items()})
    return orc


def make_draws(sizes, To, Tp, noise_len=32, n_steps=1, n_extra=0):
    """seed -> [n_steps draws]: (obsv (B, To, 2) and real future (B, Tp, 2): one random walk, zeros_val, ones_val, z (B,
    noise_len), the ((n_extra) * B, noise_len) z of the extra "fixed" samples or None), all from one CPU generator."""
    B = int(np.sum(sizes))

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        out = []
        for _ in range(n_steps):
            walk = (torch.randn(B, To + Tp, 2, generator=g) * 0.1).cumsum(1)
            lab = torch.rand(2, generator=g)
            out.append((walk[:, :To].contiguous(), walk[:, To:].contiguous(), float(lab[0]) * 0.1, 0.9 + float(lab[1]) * 0.1,
                        torch.rand(B, noise_len, generator=g),
                        torch.rand(n_extra * B, noise_len, generator=g) if n_extra else None))
        return out
    return make


def _f32(v):
    """A label-noise scalar as the step holds it: rounded to float32 (torch.zeros(bs, 1) + zeros_val, train.py:471-472)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _forms(orc, D, o, p, sb, ln, Tp):
    """predict(z) and disc(D, future) of the dense (ln None) or the ragged step, and the real future's 4-d form."""
    if ln is None:
        o4, p4 = O.get_traj_4d(o, p)
        return (lambda z: orc.predict(o, z, Tp, sb)), (lambda D_, f: D_(o4, f)), p4
    p4 = O.get_traj_4d(o[:, -2:], p)[1]            # chains from the last observed frame, which every row has
    return (lambda z: RR.predict_ragged(orc, o, ln, z, Tp, sb)), (lambda D_, f: RR.disc_ragged(D_, o, ln, f)), p4


def _len(obs_len):
    if obs_len is None:
        return None
    return np.asarray(obs_len.detach().cpu() if isinstance(obs_len, torch.Tensor) else obs_len).astype(np.int64)


def step_ambiguous(orc, D64, obsv, pred, sb, z, *, obs_len=None, variety_noise=None, flags):
    """Kink inputs within MARGIN of 0 in the float64 forward of everything a step differentiates: the rollout(s), D on the
    fake and on the real future."""
    o, p, zz = obsv.detach().cpu().double(), pred.detach().cpu().double(), z.detach().cpu().double()
    predict, disc, p4 = _forms(orc, D64, o, p, sb, _len(obs_len), orc.n_next)
    with torch.no_grad(), _f64(), recording(*gen_mods(orc), D64) as rec:
        disc(D64, predict(zz))
        disc(D64, p4)
        if flags.variety == "fixed":
            for v in variety_noise.detach().cpu().double().view(flags.variety_k - 1, o.shape[0], -1):
                predict(v)
    return count_ambiguous(rec)


def pick_draws(make, orc, sb, flags, lens=None):
    """The seed rule of tests/_ref64.py over a list of draws (make(seed), `lens`: the obs_len of each, default dense): the
    first seed of SEEDS none of whose draws has an ambiguous unit, else the seed with the fewest in all
    -> (seed, draws, ambiguous units)."""
    def ambiguous_of(draws):
        ls = lens if lens is not None else [None] * len(draws)
        return sum(step_ambiguous(orc, orc.D, d[0], d[1], sb, d[4], obs_len=ln, variety_noise=d[5], flags=flags)
                   for d, ln in zip(draws, ls))
    return pick_fewest(make, ambiguous_of)


def _run(params, mods, fn, seed, dtype):
    if dtype == torch.float64:
        run, outs = run64(params, mods, fn, seed)
    else:                                    # run64 in the default dtype (the host comparison with the fp32 oracle)
        for _, q in params:
            q.grad = None
        with recording(*mods) as rec:
            loss, outs = fn()
        loss.backward(retain_graph=True)
        run = RefRun(params, rec, seed)
    # RefRun.grads() reads the leaves' .grad when it is called; the next run on the same oracle overwrites them: keep this run's
    snap = run.grads()
    run.grads = lambda: {k: v.clone() for k, v in snap.items()}
    return run, outs


def step64(orc, D64, obsv, pred, sb, zv, ov, z, *, ss, obs_len=None, variety_noise=None, flags, global_B=None, global_row0=0,
           seed=0, dtype=torch.float64):
    """One training step at fixed weights on rows [global_row0, global_row0 + B) of a packed batch of global_B agents
    (default: the whole batch) ->
      losses  the 3 (U + 1) + 3 MSE terms in the order of losses_from(): [d_fake, d_info, d_real] x (U + 1) - the passes
              are identical at fixed weights -, [g_l2, g_fool, g_info];
      ade, fde  the sums of train.py:546-551 (sum err / Tp, sum err[:, -1]);
      d_run, g_run  _ref64.RefRun of the D loss over every D parameter / of the G loss over every generator parameter;
      pred_hat, and with "fixed": l2_k (K, B) and kmin (B,), the reference's arg-min sample."""
    f = flags
    Tp, B = orc.n_next, obsv.shape[0]
    Bg, row0 = float(B if global_B is None else global_B), int(global_row0)
    o, p, zz = (t.detach().cpu().to(dtype) for t in (obsv, pred, z))
    t0, t1 = _f32(zv), _f32(ov)
    w_info = W_INFO if f.info else 0.0
    predict, disc, p4 = _forms(orc, D64, o, p, sb, _len(obs_len), Tp)
    nl = n_codes(D64)                               # the info term's mean runs over nl codes per agent (train.py:486, 516)
    res = SimpleNamespace(kmin=None, l2_k=None)

    def d_fn():                                     # train.py:476-495
        with torch.no_grad():
            ph = predict(zz)
        fl, fc = disc(D64, ph)
        rl, _ = disc(D64, p4)
        d_fake, d_real = ((fl - t0) ** 2).sum() / Bg, ((rl - t1) ** 2).sum() / Bg
        d_info = ((fc - zz[:, :nl]) ** 2).sum() / (nl * Bg)
        return d_fake + d_real + w_info * d_info, [float(v.detach()) for v in (d_fake, d_info, d_real)]

    res.d_run, d_terms = _run(list(D64.named_parameters()), [D64], d_fn, seed, dtype)
    Dg = copy.deepcopy(D64).requires_grad_(False)    # the G loss passes through D and leaves D's gradients alone

    def g_fn():                                     # train.py:503-536
        ph = predict(zz)
        gl, gc = disc(Dg, ph)
        sq = (ph[:, :, :2] - p) ** 2
        g_fool, g_info, g_l2 = ((gl - t1) ** 2).sum() / Bg, ((gc - zz[:, :nl]) ** 2).sum() / (nl * Bg), sq.sum() / (2 * Tp * Bg)
        loss = g_fool + w_info * g_info
        if f.l2:
            loss = loss + W_L2 * g_l2
        if f.variety == "fixed":                    # per agent the smallest mean squared error over the K samples
            vn = variety_noise.detach().cpu().to(dtype).view(f.variety_k - 1, B, -1)
            l2_k = torch.stack([sq.mean(dim=(1, 2))] + [((predict(v)[:, :, :2] - p) ** 2).mean(dim=(1, 2)) for v in vn])
            l2_min, res.kmin = torch.min(l2_k, dim=0)
            res.l2_k = l2_k.detach()
            loss = loss + W_L2 * l2_min.sum() / Bg
        elif f.variety:                             # as written: the L2 of agent 19 of the packed batch, not divided by Bg
            r = 19 - row0
            if 0 <= r < B:
                loss = loss + W_L2 * sq[r].mean()
        err = (sq.detach() / (ss * ss)).sum(2).sqrt()
        return loss, ([float(v.detach()) for v in (g_l2, g_fool, g_info)], float(err.sum() / Tp), float(err[:, -1].sum()), ph.detach())

    res.g_run, (g_terms, res.ade, res.fde, res.pred_hat) = _run(gen_params(orc), gen_mods(orc) + [Dg], g_fn, seed, dtype)
    res.losses = np.asarray(d_terms * (f.U + 1) + g_terms, dtype=np.float64)
    res.n_ambiguous = count_ambiguous(res.d_run.rec) + count_ambiguous(res.g_run.rec)
    return res


# ---- the trainer's side -------------------------------------------------------------------------------------------------------
def trainer_grads(tr):
    """({name: p.grad} of D, {module.name: p.grad} of the generator) in the reference's shapes (a zero-padded hidden size is cut
    to its true entries), float64 on the host."""
    d = {k: tr.D.true_view(i, q.grad).detach().double().cpu() for i, (k, q) in enumerate(tr.D.named_parameters())}
    g = {}
    for n in G_NAMES:
        m = getattr(tr.G, n)
        for i, (k, q) in enumerate(m.named_parameters()):
            g[n + "." + k] = m.true_view(i, q.grad).detach().double().cpu()
    return d, g


def bucket_grads(tr, d_bucket=None, g_bucket=None):
    """A packed gradient bucket of a trainer laid out like `tr` (D._gflat / G._gflat_all, as the all-reduce sees it) cut into
    named tensors through the packed slices -> {name: gradient} in the reference's shapes, float64."""
    if d_bucket is not None:
        flat = torch.as_tensor(d_bucket).double()
        return {k: tr.D.true_view(i, flat[off:off + n].view(q.shape))
                for i, ((off, n), (k, q)) in enumerate(zip(tr.D._slices, tr.D.named_parameters()))}
    flat = torch.as_tensor(g_bucket).double()
    out, base = {}, tr.G._flat_all.data_ptr()
    for name in G_NAMES:
        m = getattr(tr.G, name)
        moff = (m._flat.data_ptr() - base) // 4
        for i, ((off, n), (k, q)) in enumerate(zip(m._slices, m.named_parameters())):
            out[name + "." + k] = m.true_view(i, flat[moff + off:moff + off + n].view(q.shape))
    return out


# ---- ... of the wide and the generic engine (socialways_amd/wide.py, generic.py): same names and shapes, no padding -----------
def _g_named(tr):
    """[(module.name, parameter)] of the generator of a trainer (tr.G) or of an oracle, which holds the four modules itself."""
    G = getattr(tr, "G", tr)
    return [(n + "." + k, q) for n in G_NAMES for k, q in getattr(G, n).named_parameters()]


def wide_grads(tr, d_flat=None, g_flat=None):
    """WideTrainer: a packed D / generator gradient buffer (default: dp.gflat / gp.gflat as the step left them - the LAST D
    update's gradient, the generator phase forms no D weight gradient, and the G gradient) cut into named tensors through the
    offsets of _Flat -> ({name: gradient} of D, of the generator), float64 on the host."""
    def cut(fl, flat, named):
        flat = flat.detach().double().cpu()
        assert flat.numel() == fl.gflat.numel()
        return {k: flat[fl.off[id(q)]:fl.off[id(q)] + q.numel()].view(q.shape).clone() for k, q in named}
    return (cut(tr.dp, tr.dp.gflat if d_flat is None else d_flat, list(tr.D.named_parameters())),
            cut(tr.gp, tr.gp.gflat if g_flat is None else g_flat, _g_named(tr)))


def tap_updates(tr):
    """Record what every update of the next steps is made from -> (d_taps, g_taps), lists the caller clears between steps.
    WideTrainer: the packed buffers an eager step hands to _allreduce (U + 1 x dp.gflat, then gp.gflat; a step replayed from
    a graph in one process hands over nothing).  GenericTrainer: D's p.grad in front of _reduce_grads(D_optimizer) - it is set
    to None at the end of the step - and the generator's in front of _reduce_grads(predictor_optimizer)."""
    d_taps, g_taps = [], []
    if hasattr(tr, "dp"):
        def tap(buf):
            (d_taps if buf.data_ptr() == tr.dp.gflat.data_ptr() else g_taps).append(buf.detach().clone())
        tr._allreduce = tap
    else:
        real = tr._reduce_grads

        def tap(optim):
            named, taps = (list(tr.D.named_parameters()), d_taps) if optim is tr.D_optimizer else (_g_named(tr), g_taps)
            taps.append({k: (torch.zeros_like(q) if q.grad is None else q.grad).detach().double().cpu() for k, q in named})
            real(optim)
        tr._reduce_grads = tap
    return d_taps, g_taps


def generic_grads(tr, d_tap):
    """GenericTrainer: D's gradient as tap_updates recorded it, the generator's p.grad, which survives the step (a parameter
    the step formed no gradient for - the social block of a batch without a pair - reads as zeros)."""
    return d_tap, {k: (torch.zeros_like(q) if q.grad is None else q.grad).detach().double().cpu() for k, q in _g_named(tr)}
