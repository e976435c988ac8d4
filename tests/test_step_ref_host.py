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
   cases: the figures in their derivation are recomputed here.
e. the cases of test_gpu_wide_step_reference.py (the wide and the generic engine: other hidden sizes, latent-code counts and
   horizons), with the fp32 oracle of each width standing in for the trainer: the seed rule finds a seed with at most
   MAX_AMBIGUOUS kink inputs, and every loss, the ADE/FDE row and every gradient tensor of step64(dtype=float32) stay within HALF
   of the bound the GPU file uses (OUT_RT / OUT_AT, GRAD_REL of tests/_ref64.py), so the GPU file takes those bounds unchanged.
   Recomputed here (pytest -s), seed; largest gradient error as a share of a tensor's largest entry; largest relative loss error,
   none with a kink input near 0: h64-nl3 seed 2, 1.71e-6, 2.2e-7; h96 seed 1, 1.46e-6, 7.8e-8; h128 seed 1, 2.18e-6, 1.1e-7; h128-nl17 seed 2,
   3.36e-6, 1.0e-7; h128-tp25 seed 2, 6.4e-7, 6.9e-8; h128-u2-l2 seed 1, 1.10e-6, 1.1e-7; h128-variety seed 1, 1.16e-6, 1.1e-7;
   h160-tp10 seed 1, 1.38e-6, 1.3e-7; h160-tp10-noinfo seed 1, 1.55e-6, 1.3e-7; h80 seed 1, 1.67e-6, 5.4e-8; h256 seed 8, 3.66e-6,
   1.8e-7 - the largest, against half of GRAD_REL = 1e-5 and half of OUT_RT = 5e-6.
f. shard additivity in float64 (ADD_REL) at 3 and 17 latent codes, and the count read from the discriminator (2 by default).
g. after one step at the real learning rates the oracle's U = 2 and U = 0 runs share D's Linear layers (the restore of
   train.py:541-542) and neither D's LSTM nor the generator: what part e of the GPU file asserts of the two engines."""
import numpy as np
import pytest
import torch

import sw_oracle as O
import _step_ref as S
from _ref64 import GRAD_REL, MAX_AMBIGUOUS, OUT_AT, OUT_RT, close_grads_branch_consistent, scene_rows, wide_oracles

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


# ---- e - g: the wide and the generic engine's cases (tests/test_gpu_wide_step_reference.py), from the oracle alone -----------------
# id -> (H, n_latent_codes, Tp, flags): every width / code count / horizon the GPU file builds a trainer at, and the switches
# that change which terms a step differentiates
WIDE_HOST = {
    "h64-nl3": (64, 3, 12, S.flags()), "h96": (96, 2, 12, S.flags()), "h128": (128, 2, 12, S.flags()),
    "h128-u2-l2": (128, 2, 12, S.flags(U=2, l2=True)), "h128-variety": (128, 2, 12, S.flags(variety=True)),
    "h128-nl17": (128, 17, 12, S.flags()), "h128-tp25": (128, 2, 25, S.flags()), "h160-tp10": (160, 2, 10, S.flags()),
    "h160-tp10-noinfo": (160, 2, 10, S.flags(info=False)), "h80": (80, 2, 12, S.flags()), "h256": (256, 2, 12, S.flags())}


@pytest.mark.parametrize("name", sorted(WIDE_HOST))
def test_wide_cases_have_a_seed_and_the_fp32_oracle_stays_within_half_of_the_gpu_bounds(name):
    H, nl, tp, f = WIDE_HOST[name]
    sb = scene_rows(SIZES43)
    o32, o64 = wide_oracles(H, nl, tp)
    assert S.n_codes(o64.D) == nl == o64.n_latent_codes and o64.D.latent_decoder[2].out_features == nl
    seed, draws, n_amb = S.pick_draws(S.make_draws(SIZES43, To, tp, H // 2), o64, sb, f)
    assert n_amb <= MAX_AMBIGUOUS, (name, seed, n_amb)
    obsv, pred, zv, ov, z, _ = draws[0]
    assert z.shape == (43, H // 2)
    r64 = S.step64(o64, o64.D, obsv, pred, sb, zv, ov, z, ss=SS, flags=f, seed=seed)
    r32 = S.step64(o32, o32.D, obsv, pred, sb, zv, ov, z, ss=SS, flags=f, seed=seed, dtype=torch.float32)
    assert len(r64.losses) == 3 * (f.U + 1) + 3
    # outputs: half of rtol OUT_RT + atol OUT_AT * max|ref| (_close_out), element by element
    got = np.concatenate([r32.losses, [r32.ade, r32.fde]])
    want = np.concatenate([r64.losses, [r64.ade, r64.fde]])
    for lo, hi in ((0, len(r64.losses)), (len(r64.losses), len(want))):          # the MSE terms, the ADE/FDE row
        bound = 0.5 * (OUT_RT * np.abs(want[lo:hi]) + OUT_AT * np.abs(want[lo:hi]).max())
        assert (np.abs(got[lo:hi] - want[lo:hi]) <= bound).all(), (name, got[lo:hi], want[lo:hi])
    loss_err = float(np.abs(got / want - 1).max())
    # gradients: half of GRAD_REL per tensor, through the comparison the GPU file uses (with no ambiguous unit: max|err|)
    close_grads_branch_consistent({k: v.double() for k, v in r32.d_run.grads().items()}, r64.d_run, "host", name + ", D", GRAD_REL / 2)
    close_grads_branch_consistent({k: v.double() for k, v in r32.g_run.grads().items()}, r64.g_run, "host", name + ", G", GRAD_REL / 2)
    grad_err = 0.0
    for a, b in ((r32.d_run.grads(), r64.d_run.grads()), (r32.g_run.grads(), r64.g_run.grads())):
        for k, ref in b.items():
            if not f.info and k.startswith("latent_decoder."):
                assert not bool(ref.any()) and not bool(a[k].any()), k
            else:
                assert float(ref.abs().max()) > 0, k
                grad_err = max(grad_err, _rel(a[k], ref))
    print("%s: seed %d, %d kink inputs near 0; the fp32 oracle's step misses float64 by %.2e (gradients, of a tensor's largest "
          "entry), %.1e (losses, ADE/FDE, relative)" % (name, seed, n_amb, grad_err, loss_err))


@pytest.fixture(scope="module", params=[(64, 3), (128, 17)], ids=["h64-nl3", "h128-nl17"])
def o64_nl(request):
    H, nl = request.param
    return wide_oracles(H, nl, Tp)[1]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,f", [("plain", S.flags()), ("l2-variety", S.flags(l2=True, variety=True))])
def test_shards_add_up_at_other_latent_code_counts(o64_nl, name, f, world):
    from socialways_amd.data import shard_scenes
    orc, B, sb = o64_nl, 43, scene_rows(SIZES43)
    nl, H = orc.n_latent_codes, orc.encoder.hidden_size
    assert nl != 2
    obsv, pred, zv, ov, z, _ = S.make_draws(SIZES43, To, Tp, H // 2)(8)[0]
    full = S.step64(orc, orc.D, obsv, pred, sb, zv, ov, z, ss=SS, flags=f)
    d_full, g_full = full.d_run.grads(), full.g_run.grads()
    losses, ade, fde = np.zeros_like(full.losses), 0.0, 0.0
    d_sum = {k: torch.zeros_like(v) for k, v in d_full.items()}
    g_sum = {k: torch.zeros_like(v) for k, v in g_full.items()}
    owners = []
    for lo, hi in shard_scenes(sb, world):
        r0, r1 = int(sb[lo, 0]), int(sb[hi - 1, 1])
        owners.append(r0 <= 19 < r1)
        part = S.step64(orc, orc.D, obsv[r0:r1], pred[r0:r1], sb[lo:hi] - r0, zv, ov, z[r0:r1], ss=SS, flags=f, global_B=B,
                        global_row0=r0)
        losses, ade, fde = losses + part.losses, ade + part.ade, fde + part.fde
        for acc, run in ((d_sum, part.d_run), (g_sum, part.g_run)):
            for k, v in run.grads().items():
                acc[k] += v
    assert sum(owners) == 1
    assert np.abs(losses - full.losses).max() <= ADD_REL * np.abs(full.losses).max()
    assert abs(ade - full.ade) <= ADD_REL * full.ade and abs(fde - full.fde) <= ADD_REL * full.fde
    for acc, ref in ((d_sum, d_full), (g_sum, g_full)):
        for k in ref:
            assert float(ref[k].abs().max()) > 0
            assert _rel(acc[k], ref[k]) <= ADD_REL, (nl, name, world, k, _rel(acc[k], ref[k]))
    # ... and the info term does run over nl codes: with the count of the fused path it is another number
    two = ((full.d_run.grads()["latent_decoder.2.bias"]) * nl / 2)
    assert _rel(two, d_full["latent_decoder.2.bias"]) > 0.1


def test_the_latent_code_count_is_the_discriminators_and_two_by_default():
    o32 = O.SocialWaysOracle(Tp)
    assert S.n_codes(o32.D) == 2 == S.NL and S.n_codes(object()) == 2 and S.oracle_of(o32, o32.D, Tp).n_latent_codes == 2
    o5 = O.SocialWaysOracle(Tp, n_latent_codes=5)
    o64 = S.oracle_of(o5, o5.D, Tp)
    assert S.n_codes(o5.D) == 5 and o64.n_latent_codes == 5 and o64.D.latent_decoder[2].weight.dtype == torch.float64


def test_unrolling_changes_the_oracles_generator_update_and_restores_the_linear_layers_of_d():
    """What test_gpu_wide_step_reference.py (part e) compares between a U = 2 and a U = 0 trainer, on the oracle: after one
    step from the same weights D's Linear layers are equal (the restore of train.py:541-542), D's LSTM is not - and neither is
    the generator, whose update differentiates through the D of the step's last update."""
    sb = scene_rows(SIZES43)
    obsv, pred, zv, ov, z, _ = S.make_draws(SIZES43, To, Tp)(1)[0]
    after = {}
    for U in (2, 0):
        torch.manual_seed(79)
        orc = O.SocialWaysOracle(Tp, use_social=True, n_unrolling_steps=U)
        orc.train_step(obsv, pred, sb, zv, ov, z, SS)
        after[U] = orc
    for (k, a), (_, b) in zip(after[2].D.named_parameters(), after[0].D.named_parameters()):
        assert torch.equal(a, b) == ("lstm" not in k), k
    differ = [k for (k, a), (_, b) in zip(S._g_named(after[2]), S._g_named(after[0])) if not torch.equal(a, b)]
    assert len(differ) >= 20, differ
