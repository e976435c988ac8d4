"""The float64 training step of tests/_step_ref.py, checked on the CPU before a GPU is compared with it.

a. step64 run in float32 against SocialWaysOracle.train_step(record=...) with lr = 0 optimizers: the same losses, ADE/FDE sums
   and recorded gradients (every D pass, the G phase) to fp32 roundoff - U in {0, 1, 2}, the L2 term, the variety term as
   written and "fixed".  Both sides are the same fp32 operations in a slightly different order (sum / Bg for mean, one
   rollout for the as-written variety term's second one), so the bound is a few hundred fp32 roundings, 1e-5 of a tensor's
   largest entry; observed 2.1e-6 (the as-written variety term), 0 elsewhere.
b. shard additivity in float64: the losses and gradients of the shards of shard_scenes(sb, 2) and (sb, 3), normalised by the
   global batch with row 19 addressed globally, add up to the full batch to 1e-12 - the semantics of global_B / global_row0
   that the sharded GPU steps are held to.
c. obs_len = To on every row is the dense reference.
d. the three per-tensor bounds of test_gpu_step_dp_reference.py (REL_OF) are 4 x the fp32 CPU oracle's own error on those very
   cases: the figures in their derivation are recomputed here."""
import numpy as np
import pytest
import torch

import sw_oracle as O
import _step_ref as S
from _ref64 import scene_rows

SIZES43 = [1, 5, 17, 8, 3, 9]
To, Tp = 8, 12
SS = 0.25
FP32_REL = 1e-5
ADD_REL = 1e-12


def _ragged_len(B):
    return (2 + (5 * np.arange(B)) % 7).astype(np.int64)


def _oracle32(f):
    torch.manual_seed(77)
    return O.SocialWaysOracle(Tp, lr_g=0.0, lr_d=0.0, use_social=True, **S.trainer_kw(f))


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-300)


@pytest.mark.parametrize("name,f", [
    ("u0", S.flags(U=0)), ("u1", S.flags()), ("u2", S.flags(U=2)), ("noinfo", S.flags(info=False)), ("l2", S.flags(l2=True)),
    ("variety", S.flags(variety=True)), ("fixed", S.flags(variety="fixed", variety_k=3, l2=True))])
def test_step64_in_float32_is_the_oracles_train_step(name, f):
    o32 = _oracle32(f)
    w0 = {k: v.clone() for m in S.G_NAMES + ("D",) for k, v in getattr(o32, m).state_dict(prefix=m + ".").items()}
    n_extra = f.variety_k - 1 if f.variety == "fixed" else 0
    obsv, pred, zv, ov, z, vn = S.make_draws(SIZES43, To, Tp, n_extra=n_extra)(5)[0]
    sb = scene_rows(SIZES43)
    ref = S.step64(o32, o32.D, obsv, pred, sb, zv, ov, z, ss=SS, variety_noise=vn, flags=f, dtype=torch.float32)
    d_ref, g_ref = ref.d_run.grads(), ref.g_run.grads()
    rec = {}
    losses, ade, fde = o32.train_step(obsv, pred, sb, zv, ov, z, SS, record=rec, variety_noise=vn)
    for m in S.G_NAMES + ("D",):                                     # lr = 0: the premise of every comparison at fixed weights
        for k, v in getattr(o32, m).state_dict(prefix=m + ".").items():
            assert torch.equal(v, w0[k]), k
    assert len(losses) == len(ref.losses) == 3 * (f.U + 1) + 3 and len(rec["d_grads"]) == f.U + 1
    worst = _rel(torch.tensor(ref.losses), torch.tensor(losses))
    worst = max(worst, abs(ref.ade - ade) / ade, abs(ref.fde - fde) / fde)
    assert worst <= FP32_REL, ("losses, ADE/FDE", worst)
    for u, dg in enumerate(rec["d_grads"]):
        assert set(dg) == set(d_ref)
        for k in dg:
            assert float(dg[k].abs().max()) > 0 or (not f.info and k.startswith("latent_decoder.")), k     # no info loss: no such gradient
            worst = max(worst, _rel(d_ref[k], dg[k]))
            assert _rel(d_ref[k], dg[k]) <= FP32_REL, ("D pass %d" % u, k, _rel(d_ref[k], dg[k]))
    assert set(rec["g_grads"]) == set(g_ref)
    for k, g in rec["g_grads"].items():
        assert float(g.abs().max()) > 0
        worst = max(worst, _rel(g_ref[k], g))
        assert _rel(g_ref[k], g) <= FP32_REL, ("G phase", k, _rel(g_ref[k], g))
    assert _rel(ref.pred_hat, rec["pred_hat_4d"]) <= FP32_REL
    if f.variety == "fixed":
        assert torch.equal(ref.kmin, rec["variety_kmin"])
    print("step64 (float32) against train_step, %s: largest relative difference %.2e" % (name, worst))


@pytest.fixture(scope="module")
def o64():
    torch.manual_seed(78)
    o32 = O.SocialWaysOracle(Tp, use_social=True)
    return S.oracle_of(o32, o32.D, Tp)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,f,ragged", [
    ("plain", S.flags(), False), ("ragged", S.flags(), True), ("variety", S.flags(variety=True), False),
    ("fixed", S.flags(variety="fixed", variety_k=3, l2=True), False)])
def test_shards_add_up_to_the_full_batch(o64, name, f, ragged, world):
    from socialways_amd.data import shard_scenes
    B, sb = 43, scene_rows(SIZES43)
    K1 = f.variety_k - 1 if f.variety == "fixed" else 0
    obsv, pred, zv, ov, z, vn = S.make_draws(SIZES43, To, Tp, n_extra=K1)(8)[0]
    ln = _ragged_len(B) if ragged else None
    full = S.step64(o64, o64.D, obsv, pred, sb, zv, ov, z, ss=SS, obs_len=ln, variety_noise=vn, flags=f)
    d_full, g_full = full.d_run.grads(), full.g_run.grads()
    losses, ade, fde = np.zeros_like(full.losses), 0.0, 0.0
    d_sum = {k: torch.zeros_like(v) for k, v in d_full.items()}
    g_sum = {k: torch.zeros_like(v) for k, v in g_full.items()}
    owners = []
    for lo, hi in shard_scenes(sb, world):
        assert hi > lo
        r0, r1 = int(sb[lo, 0]), int(sb[hi - 1, 1])
        owners.append(r0 <= 19 < r1)
        part = S.step64(o64, o64.D, obsv[r0:r1], pred[r0:r1], sb[lo:hi] - r0, zv, ov, z[r0:r1], ss=SS,
                        obs_len=None if ln is None else ln[r0:r1],
                        variety_noise=None if vn is None else vn.view(K1, B, -1)[:, r0:r1].reshape(K1 * (r1 - r0), -1),
                        flags=f, global_B=B, global_row0=r0)
        losses, ade, fde = losses + part.losses, ade + part.ade, fde + part.fde
        for acc, run in ((d_sum, part.d_run), (g_sum, part.g_run)):
            for k, v in run.grads().items():
                acc[k] += v
        if f.variety == "fixed":
            assert torch.equal(part.kmin, full.kmin[r0:r1])
    assert sum(owners) == 1
    assert np.abs(losses - full.losses).max() <= ADD_REL * np.abs(full.losses).max()
    assert abs(ade - full.ade) <= ADD_REL * full.ade and abs(fde - full.fde) <= ADD_REL * full.fde
    for acc, ref in ((d_sum, d_full), (g_sum, g_full)):
        for k in ref:
            assert float(ref[k].abs().max()) > 0
            assert _rel(acc[k], ref[k]) <= ADD_REL, (name, world, k, _rel(acc[k], ref[k]))


def test_the_shard_that_owns_row_19_carries_the_variety_term(o64):
    """The additivity above would also hold if no shard carried the term: without it the generator gradient differs."""
    f, sb = S.flags(variety=True), scene_rows(SIZES43)
    obsv, pred, zv, ov, z, _ = S.make_draws(SIZES43, To, Tp)(8)[0]
    with_term = S.step64(o64, o64.D, obsv, pred, sb, zv, ov, z, ss=SS, flags=f).g_run.grads()
    without = S.step64(o64, o64.D, obsv, pred, sb, zv, ov, z, ss=SS, flags=S.flags()).g_run.grads()
    assert _rel(with_term["decoder.fc1.0.weight"], without["decoder.fc1.0.weight"]) > 1e-3
    # a shard that starts past row 19 has no such row
    shifted = S.step64(o64, o64.D, obsv[23:], pred[23:], sb[3:] - 23, zv, ov, z[23:], ss=SS, flags=f, global_B=43, global_row0=23)
    plain = S.step64(o64, o64.D, obsv[23:], pred[23:], sb[3:] - 23, zv, ov, z[23:], ss=SS, flags=S.flags(), global_B=43,
                     global_row0=23)
    for k, v in shifted.g_run.grads().items():
        assert torch.equal(v, plain.g_run.grads()[k]), k


def test_full_length_obs_len_is_the_dense_reference(o64):
    f, sb = S.flags(l2=True), scene_rows(SIZES43)
    obsv, pred, zv, ov, z, _ = S.make_draws(SIZES43, To, Tp)(13)[0]
    dense = S.step64(o64, o64.D, obsv, pred, sb, zv, ov, z, ss=SS, flags=f)
    full = S.step64(o64, o64.D, obsv, pred, sb, zv, ov, z, ss=SS, obs_len=np.full(43, To), flags=f)
    assert np.abs(dense.losses - full.losses).max() <= ADD_REL * np.abs(dense.losses).max()
    assert abs(dense.ade - full.ade) <= ADD_REL * dense.ade and abs(dense.fde - full.fde) <= ADD_REL * dense.fde
    for a, b in ((dense.d_run, full.d_run), (dense.g_run, full.g_run)):
        ga, gb = a.grads(), b.grads()
        for k in ga:
            assert _rel(gb[k], ga[k]) <= ADD_REL, (k, _rel(gb[k], ga[k]))
    # ... and a ragged one is not
    short = S.step64(o64, o64.D, obsv, pred, sb, zv, ov, z, ss=SS, obs_len=_ragged_len(43), flags=f)
    assert _rel(short.g_run.grads()["encoder.lstm.weight_hh_l0"], dense.g_run.grads()["encoder.lstm.weight_hh_l0"]) > 1e-3


def test_the_per_case_bounds_are_four_times_the_fp32_oracles_own_error():
    import test_gpu_step_dp_reference as DP
    bounds = {}
    for (name, epoch, batch, tensor), typed in DP.OWN_ERROR.items():
        seed, own = DP.fp32_oracle_own_error(name, epoch, batch, tensor)
        print("%s, epoch %d batch %d, seed %d, d/d%s: the fp32 oracle misses float64 by %.3e (faithful), %.3e (block-diagonal)"
              % (name, epoch, batch, seed, tensor, own["faithful"], own["blockdiag"]))
        assert abs(max(own.values()) - typed) <= 0.01 * typed, (own, typed)
        bounds.setdefault((name, epoch, batch, "G bucket"), {})[tensor] = 4 * typed
    assert bounds == DP.REL_OF
