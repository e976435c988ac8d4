"""The branch-consistent float64 comparison of tests/_ref64.py, checked on the CPU: the fp32 oracle stands in for the
kernels, the reference is the float64 oracle with the same weights (as tests/test_gpu_gen_reference.py builds it).  The
helper has to pass an honest fp32 gradient at GRAD_REL on the large shapes where no seed avoids every ReLU kink, and has
to reject a gradient that is wrong in ways a branch flip cannot explain."""
import functools

import numpy as np
import pytest
import torch

import sw_oracle as O
import _ref64 as R
from _ref64 import _report      # noqa: F401  (module fixture: the observed errors, printed with pytest -s)

TO, TP = 8, 12
CASES = {"rowblocks": [70, 5, 130, 64, 1], "big200": [200, 3], "edges": [16, 17, 32, 33, 48, 49, 64, 1], "metric": [8] * 256}
# Each shape runs twice: at the seed the seed rule picks (pick_fewest: few ambiguous units, often none of them flipped by
# the stand-in) and at a fixed seed where the fp32 oracle does take the other branch of 1-3 units (seed 1; the metric shape
# at seed 3 has 8 ambiguous units and no flip).  The rejection tests use the fixed seeds: flips are on offer there.
FIXED = {"rowblocks": 1, "big200": 1, "edges": 1, "metric": 3}


def _oracles():
    torch.manual_seed(2000 + TP)
    o32 = O.SocialWaysOracle(TP, use_social=True)
    with R._f64():
        o64 = O.SocialWaysOracle(TP, use_social=True)
    for n in R.G_NAMES:
        getattr(o64, n).double().load_state_dict({k: v.double() for k, v in getattr(o32, n).state_dict().items()})
    return o32, o64


def _stand_in(o32, obsv, z, cot, sb):
    """The fp32 oracle's gradients of <rollout, cot>."""
    for n in R.G_NAMES:
        getattr(o32, n).zero_grad()
    (o32.predict(obsv, z, TP, sb) * cot).sum().backward()
    return {k: (torch.zeros_like(p) if p.grad is None else p.grad.clone()) for k, p in R.gen_params(o32)}


@functools.lru_cache(maxsize=None)
def _case(name, fixed=False):
    sizes = CASES[name]
    B, sb = int(np.sum(sizes)), R.scene_rows(sizes)
    o32, o64 = _oracles()

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        return ((torch.randn(B, TO, 2, generator=g) * 0.1).cumsum(1), torch.rand(B, 32, generator=g),
                torch.randn(B, TP, 4, generator=g) * 0.1)

    def ambiguous_of(inp):
        return R.gen_ambiguous(o64, lambda: o64.predict(inp[0].double(), inp[1].double(), TP, sb))

    if fixed:
        seed = FIXED[name]
        obsv, z, cot = make(seed)
        n_amb = ambiguous_of((obsv, z, cot))
    else:
        seed, (obsv, z, cot), n_amb = R.pick_fewest(make, ambiguous_of)

    def fn():
        pred = o64.predict(obsv.double(), z.double(), TP, sb)
        return (pred * cot.double()).sum(), pred

    ref_run, pred64 = R.run64(R.gen_params(o64), R.gen_mods(o64), fn, seed)
    got = _stand_in(o32, obsv, z, cot, sb)
    return dict(o32=o32, sb=sb, obsv=obsv, z=z, cot=cot, got=got, ref_run=ref_run, pred64=pred64.detach(), seed=seed,
                n_amb=n_amb, tag="seed %d" % seed)


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_oracle_passes_the_branch_consistent_comparison(name, fixed):
    c = _case(name, fixed)
    name += "@%d" % c["seed"]
    with torch.no_grad():
        R._close_out(c["o32"].predict(c["obsv"], c["z"], TP, c["sb"]), c["pred64"], "rollout", name, c["tag"])
    R.close_grads_branch_consistent(c["got"], c["ref_run"], name, c["tag"])


def test_plain_comparison_fails_where_a_unit_flipped():
    """The helper is doing work: without the flip assignment the same gradients miss GRAD_REL."""
    c = _case("big200", fixed=True)
    assert c["n_amb"] > 0
    ref = c["ref_run"].grads()
    with pytest.raises(AssertionError, match="max.err"):
        for k, g in c["got"].items():
            R._close_grad(g, ref[k], k, "plain", c["tag"])
    R._observed.pop("plain", None)


def _mutated(c, k, fn):
    got = {n: g.clone() for n, g in c["got"].items()}
    got[k] = fn(got[k])
    return got


def _rejects(c, got):
    with pytest.raises(AssertionError, match=r"max\|err\| .* > |neither 0 nor 1"):
        R.close_grads_branch_consistent(got, c["ref_run"], "mutations", c["tag"])
    R._observed.pop("mutations", None)


@pytest.mark.parametrize("name", ["big200", "metric"])
def test_rejects_a_scaled_tensor(name):
    c = _case(name, fixed=True)
    for k in ("decoder.fc1.0.weight", "feature_embedder.fc.2.weight", "encoder.lstm.weight_hh_l0"):
        _rejects(c, _mutated(c, k, lambda g: g * (1 + 1e-3)))


@pytest.mark.parametrize("name", ["big200", "metric"])
def test_rejects_a_zeroed_weight_gradient_tile(name):
    c = _case(name, fixed=True)

    def zero_tile(g):
        g[16:32, 16:32] = 0
        return g
    _rejects(c, _mutated(c, "decoder.fc1.0.weight", zero_tile))


@pytest.mark.parametrize("name", ["big200", "metric"])
def test_rejects_a_missing_scene(name):
    """`got` computed with one scene's cotangent zeroed: that scene's gradient contribution is missing."""
    c = _case(name, fixed=True)
    s0, s1 = (int(v) for v in c["sb"][-1])
    cot = c["cot"].clone()
    cot[s0:s1] = 0
    _rejects(c, _stand_in(c["o32"], c["obsv"], c["z"], cot, c["sb"]))


def test_rejects_a_non_binary_flip():
    """`got` moved by half of the largest flip vector: no binary assignment explains it."""
    c = _case("big200", fixed=True)
    A = R.flip_vectors(c["ref_run"])
    names = [k for k, _ in c["ref_run"].params]
    ref = c["ref_run"].grads()
    scale = torch.cat([torch.full((ref[k].numel(),), float(ref[k].abs().max()), dtype=torch.float64) for k in names])
    size = (A.abs() / scale.clamp_min(1e-300)[:, None]).max(0).values
    u = int(size.argmax())
    assert float(size[u]) > 4 * R.GRAD_REL        # half of it is still twice the tolerance
    got, off = {}, 0
    for k in names:
        n = ref[k].numel()
        got[k] = c["got"][k].double() + 0.5 * A[off:off + n, u].view(ref[k].shape)
        off += n
    _rejects(c, got)


def test_without_ambiguous_units_it_is_the_plain_comparison():
    torch.manual_seed(5)
    lin = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.LeakyReLU(0.2), torch.nn.Linear(8, 2)).double()
    x = torch.randn(16, 4, dtype=torch.float64)
    params = list(lin.named_parameters())
    ref_run, _ = R.run64(params, [lin], lambda: (lin(x).sum(), None), 0)
    assert R.count_ambiguous(ref_run.rec) == 0
    ok = ref_run.grads()
    R.close_grads_branch_consistent(ok, ref_run, "tiny", "seed 0")
    bad = {k: v.clone() for k, v in ok.items()}
    bad["0.weight"][0, 0] += 1e-4 * float(ok["0.weight"].abs().max())
    with pytest.raises(AssertionError, match="0.weight"):
        R.close_grads_branch_consistent(bad, ref_run, "tiny", "seed 0")
    R._observed.pop("tiny", None)


@pytest.mark.parametrize("case", R.WIDE_CASES, ids=[c[0] for c in R.WIDE_CASES])
def test_wide_cases_have_a_seed_within_the_ambiguity_cap(case):
    """The seed rule of tests/test_gpu_wide_reference.py, known to hold before a GPU is involved: every row's float64
    oracle, drawn from the torch seed the GPU test uses, has a seed of SEEDS (pick_fewest) whose generator + discriminator
    forward keeps at most MAX_AMBIGUOUS kink inputs within MARGIN of 0."""
    _, H, nl, Tp, To, sizes, _, _ = case
    B, sb = int(np.sum(sizes)), R.scene_rows(sizes)
    _, o64 = R.wide_oracles(H, nl, Tp)
    seed, _, n_amb = R.wide_pick(o64, B, To, Tp, H, sb)
    print("wide case %-14s seed %3d: %d kink inputs within %.1e of 0" % (case[0], seed, n_amb, R.MARGIN))
    assert n_amb <= R.MAX_AMBIGUOUS, (case[0], seed, n_amb)
