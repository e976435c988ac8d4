"""Shared pieces of the float64 reference tests (test_gpu_disc_reference.py, test_gpu_gen_reference.py, test_ref64_host.py).

The reference is always the oracle's modules (oracle/sw_oracle.py) cast to double, loaded with the weights of the code under
test and fed the exact fp32 inputs.  Tolerances: outputs elementwise rtol OUT_RT + atol OUT_AT * max|ref|; gradients per
tensor max|err| <= GRAD_REL * max|ref|.

(Leaky)ReLU kinks.  Where a pre-activation lies within fp32 rounding (MARGIN) of 0 the fp32 code and the float64 reference
may take different branches, and one such unit moves a weight gradient by far more than fp32 summation does.  Small cases
avoid that by the choice of the seed (`_pick`: the first seed of SEEDS whose float64 forward keeps every kink input MARGIN
away from 0).  Large cases (millions of ReLU inputs) have no such seed; they use `close_grads_branch_consistent`, which
accepts a gradient iff it equals the reference gradient with SOME binary choice of branch for the few ambiguous units."""
import contextlib

import numpy as np
import pytest
import torch

from _util import assert_close

SEEDS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233)
MARGIN = 2e-7
OUT_RT, OUT_AT = 1e-5, 1e-6
GRAD_REL = 2e-5
MAX_AMBIGUOUS = 16      # a case with more ambiguous units than this fails: the seed rule is meant to keep them few
COEF_TOL = 0.1          # a fitted flip coefficient must be this close to 0 or 1

G_NAMES = ("encoder", "feature_embedder", "attention", "decoder")

_observed = {}      # group -> maxima over the group's cases: printed at the end of the module (pytest -s), then cleared


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, v in sorted(_observed.items()):
        line = "observed max error  %-12s outputs %.2e  gradients %.2e" % (group, v.get("out", 0.0), v.get("grad", 0.0))
        if "ambiguous" in v:
            line += "  (before flip assignment %.2e; ambiguous units <= %d per case, %d in all, %d assigned flipped)" % (
                v.get("grad_plain", 0.0), v["ambiguous"], v.get("ambiguous_sum", 0), v.get("flipped_sum", 0))
        print(line)
    _observed.clear()


def _note(group, kind, ratio):
    g = _observed.setdefault(group, {})
    g[kind] = max(g.get(kind, 0.0), ratio)


def _note_sum(group, kind, n):
    g = _observed.setdefault(group, {})
    g[kind] = g.get(kind, 0) + n


@contextlib.contextmanager
def _f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)     # the oracle builds its zero states with the default dtype
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _close_out(got, ref, what, group, tag, at=OUT_AT):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(float(ref.abs().max()), 1e-30)
    _note(group, "out", float((got - ref).abs().max()) / scale)
    assert_close(got.numpy(), ref.numpy(), OUT_RT, at * scale, "%s (%s)" % (what, tag))


def _close_grad(got, ref, what, group, tag, rel=GRAD_REL):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite entries (%s)" % (what, tag)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    if scale > 0:
        _note(group, "grad", err / scale)
    assert err <= rel * scale, "%s: max|err| %.3e > %.1e * max|ref| %.3e (%s)" % (what, err, rel, scale, tag)


def _is_kink(m):
    return isinstance(m, (torch.nn.LeakyReLU, torch.nn.ReLU))


@contextlib.contextmanager
def _kink_margin(*mods):
    """Yields a list that ends up holding the smallest |input| of every (Leaky)ReLU run inside the block."""
    seen, hooks = [], []
    for mod in mods:
        for m in mod.modules():
            if _is_kink(m):
                hooks.append(m.register_forward_hook(lambda m_, inp, out: seen.append(float(inp[0].detach().abs().min()))
                                                     if inp[0].numel() else None))
    box = [float("inf")]
    try:
        yield box
    finally:
        for h in hooks:
            h.remove()
        box[0] = min(seen, default=float("inf"))


def _pick(make, margin_of):
    """First seed of SEEDS whose float64 forward keeps every kink input above MARGIN: (seed, inputs, margin)."""
    best = (None, 0.0)
    for seed in SEEDS:
        inp = make(seed)
        m = margin_of(inp)
        if m > MARGIN:
            return seed, inp, m
        best = max(best, (seed, m), key=lambda t: t[1])
    raise AssertionError("no seed of %s keeps the kink inputs above %.1e (best: seed %s, %.2e)" % (SEEDS, MARGIN, *best))


# ---- branch-consistent comparison ----------------------------------------------------------------------------------------
@contextlib.contextmanager
def recording(*mods):
    """Yields a list that collects (module, input x, output y) of every (Leaky)ReLU run inside the block; y keeps its
    gradient (retain_grad) where a graph is being built."""
    rec, hooks = [], []

    def hook(m, inp, out):
        if inp[0].numel():
            if out.requires_grad:
                out.retain_grad()
            rec.append((m, inp[0], out))

    for mod in mods:
        for m in mod.modules():
            if _is_kink(m):
                hooks.append(m.register_forward_hook(hook))
    try:
        yield rec
    finally:
        for h in hooks:
            h.remove()


def count_ambiguous(rec):
    return sum(int((x.detach().abs() < MARGIN).sum()) for _, x, _ in rec)


def pick_fewest(make, ambiguous_of):
    """The seed rule of the branch-consistent cases: the first seed of SEEDS with no ambiguous unit, as `_pick`; where
    there is none, the seed of SEEDS with the fewest.  -> (seed, inputs, ambiguous units)."""
    best = None
    for seed in SEEDS:
        inp = make(seed)
        n = ambiguous_of(inp)
        if n == 0:
            return seed, inp, 0
        if best is None or n < best[2]:
            best = (seed, inp, n)
    return best


class RefRun:
    """A float64 forward + backward kept with its graph: `params` [(name, leaf)] whose .grad is the reference gradient,
    `rec` the (Leaky)ReLU records of `recording`, `seed` for the messages."""

    def __init__(self, params, rec, seed):
        self.params, self.rec, self.seed = list(params), rec, seed

    def grads(self):
        return {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in self.params}


def run64(params, mods, fn, seed):
    """Zero the gradients of `params`, run fn() -> (loss, outputs) in float64 with every kink of `mods` recorded, and
    back-propagate keeping the graph.  -> (RefRun, outputs)."""
    for _, p in params:
        p.grad = None
    with _f64(), recording(*mods) as rec:
        loss, outs = fn()
    loss.backward(retain_graph=True)
    return RefRun(params, rec, seed), outs


def flip_vectors(ref_run):
    """One vector per ambiguous unit u (|x_u| < MARGIN): what taking the other branch of u adds to the concatenated
    parameter gradient, to first order: -+(1 - slope) dL/dy_u dx_u/dtheta, minus where the reference took the positive
    branch; dx_u/dtheta is the total derivative through everything upstream.  -> (n_params_total, U) matrix."""
    plist = [p for _, p in ref_run.params]
    cols = []
    for m, x, y in ref_run.rec:
        slope = float(getattr(m, "negative_slope", 0.0))
        for i in (x.detach().abs() < MARGIN).nonzero():
            i = tuple(i.tolist())
            gy = 0.0 if y.grad is None else float(y.grad[i])
            col = torch.zeros(sum(p.numel() for p in plist), dtype=torch.float64)
            if gy != 0.0 and x.requires_grad:
                gs = torch.autograd.grad(x[i], plist, retain_graph=True, allow_unused=True)
                sign = -1.0 if float(x.detach()[i]) > 0 else 1.0
                col = torch.cat([(torch.zeros_like(p) if g is None else g).reshape(-1).double() for g, p in zip(gs, plist)])
                col = col * (sign * (1.0 - slope) * gy)
            cols.append(col)
    return torch.stack(cols, 1) if cols else None


def close_grads_branch_consistent(got, ref_run, group, tag, rel=GRAD_REL):
    """`got` {name: gradient} against the float64 run `ref_run`.  Passes iff a binary assignment s_u of the ambiguous
    units exists with, for every parameter tensor at once, max|got - ref - sum_u s_u delta_u| <= rel * max|ref| (the
    `_close_grad` criterion, finiteness included).  s comes from least squares on the concatenated gradient (every tensor
    in units of its own max|ref|) and rounding; only the rounded s is used for acceptance.  With no ambiguous unit this is
    `_close_grad` on every tensor."""
    names = [k for k, _ in ref_run.params]
    ref = ref_run.grads()
    assert set(got) == set(names), (sorted(got), names)
    A = flip_vectors(ref_run)
    U = 0 if A is None else A.shape[1]
    assert U <= MAX_AMBIGUOUS, "%d ambiguous units (|x| < %.1e) > %d (%s)" % (U, MARGIN, MAX_AMBIGUOUS, tag)
    if U == 0:
        _note(group, "ambiguous", 0)
        for k in names:
            sc = float(ref[k].abs().max())
            if sc > 0 and got[k].shape == ref[k].shape:     # the report's "before" column: nothing to assign here
                _note(group, "grad_plain", float((got[k].detach().cpu().double() - ref[k]).abs().max()) / sc)
            _close_grad(got[k], ref[k], "d/d%s" % k, group, tag, rel)
        return
    g = {}
    for k in names:
        g[k] = got[k].detach().cpu().double()
        assert g[k].shape == ref[k].shape, (k, g[k].shape, ref[k].shape)
        assert bool(torch.isfinite(g[k]).all()), "d/d%s: non-finite entries (%s)" % (k, tag)
    d = torch.cat([(g[k] - ref[k]).reshape(-1) for k in names])
    scale = torch.cat([torch.full((ref[k].numel(),), float(ref[k].abs().max()), dtype=torch.float64) for k in names])
    inv = torch.where(scale > 0, 1.0 / scale.clamp_min(1e-300), torch.zeros_like(scale))

    def worst(v):       # largest per-tensor max|v| / max|ref|; a tensor whose reference is all zeros tolerates nothing
        r = v.abs() * inv
        return float(torch.where((scale == 0) & (v != 0), torch.full_like(r, float("inf")), r).max())

    matters = torch.tensor([worst(A[:, u]) > rel for u in range(U)])
    s = torch.zeros(U, dtype=torch.float64)
    coef = torch.zeros(U, dtype=torch.float64)
    if bool(matters.any()):
        Aw = A[:, matters] * inv[:, None]
        coef[matters] = torch.linalg.lstsq(Aw, (d * inv)[:, None]).solution[:, 0]
        s = coef.round().clamp(0, 1) * matters
    before, after = worst(d), worst(d - A @ s)
    info = "%s; %d ambiguous units, %d assigned flipped (fitted %s), error before %.2e after %.2e of max|ref|" % (
        tag, U, int(s.sum()), " ".join("%.3f" % c for c in coef.tolist()), before, after)
    _note(group, "grad", after)
    _note(group, "grad_plain", before)
    _note(group, "ambiguous", U)
    _note_sum(group, "ambiguous_sum", U)
    _note_sum(group, "flipped_sum", int(s.sum()))
    off_binary = (coef - coef.round().clamp(0, 1)).abs() > COEF_TOL
    assert not bool((off_binary & matters).any()), "a fitted flip coefficient is neither 0 nor 1 (%s)" % info
    resid = d - A @ s
    off = 0
    for k in names:
        n = ref[k].numel()
        sc, err = float(ref[k].abs().max()), float(resid[off:off + n].abs().max()) if n else 0.0
        assert err <= rel * sc, "d/d%s: max|err| %.3e > %.1e * max|ref| %.3e (%s)" % (k, err, rel, sc, info)
        off += n


# ---- the generator's float64 reference -------------------------------------------------------------------------------------
def gen_params(orc):
    return [(n + "." + k, p) for n in G_NAMES for k, p in getattr(orc, n).named_parameters()]


def gen_mods(orc):
    return [getattr(orc, n) for n in G_NAMES]


def scene_rows(sizes):
    sizes = list(sizes)
    return np.stack([np.cumsum([0] + sizes[:-1]), np.cumsum(sizes)], 1).astype(np.int64)


def gen_ambiguous(orc, fn, extra_mods=()):
    """Ambiguous units of the float64 forward fn() (no graph)."""
    with torch.no_grad(), _f64(), recording(*gen_mods(orc), *extra_mods) as rec:
        fn()
    return count_ambiguous(rec)


# ---- the wide path (hidden sizes above 64): cases and float64 references of test_gpu_wide_reference.py ---------------------
W_INFO = 0.5
TARGETS = (0.03, 0.96)
_MIX = [5, 1, 9, 16, 3, 2]
# (id, H, n_latent_codes, n_next, To, scene sizes, forms the trainer must take: seq, decloop, heads, generator phases run)
WIDE_CASES = [
    ("h64-nl3", 64, 3, 12, 8, _MIX, (True, False, True), True),                 # sequence kernel <1>, per-step decode, nlp padding
    ("h96", 96, 2, 12, 8, [33, 32, 2], (False, False, True), True),             # per-step LSTM, half-filled 64-unit block, B past 64
    ("h128-ragged", 128, 2, 12, 8, _MIX, (True, True, True), True),             # sequence <2>, decode loop
    ("h128-aligned", 128, 2, 12, 8, [16, 16], (True, True, True), True),
    ("h128-nopairs", 128, 2, 12, 8, [1] * 17, (True, True, True), True),
    ("h128-amax", 128, 2, 12, 8, [64, 1], (True, True, True), True),
    ("h128-tp1", 128, 2, 1, 2, [5, 1, 9, 4, 2], (True, True, False), True),     # loop with no re-fed step; K4 = 4: GEMM heads
    ("h128-tp2", 128, 2, 2, 2, [5, 1, 9, 4, 2], (True, True, False), True),     # one re-fed step; K4 = 8
    ("h128-nl5-tp16", 128, 5, 16, 8, [33, 32, 2], (True, True, True), True),    # K4 = 64, nlp = 8
    ("h128-nl17", 128, 17, 12, 8, _MIX, (True, True, False), False),            # nl past the heads' limit: GEMM heads (b, c only)
    ("h160-tp10", 160, 2, 10, 8, _MIX, (False, False, False), True),            # nub = 3, D3 = 100, K4 = 40: GEMM heads
    ("h256", 256, 2, 12, 8, [33, 32, 2], (False, False, True), True),           # heads at WH_MAXH, wgrad batch flush
    ("h288", 288, 2, 12, 2, _MIX, (False, False, False), True),                 # past WH_MAXH
    ("h128-metric", 128, 2, 12, 8, [8] * 256, (True, True, True), True),        # the one large case
]


def wide_torch_seed(H, nl, Tp):
    return 3000 + H + 7 * nl + Tp


def wide_oracles(H, nl, Tp, use_social=True):
    """The fp32 oracle drawn from the case's torch seed (the initial weights a WideTrainer draws from the same seed: same
    construction order) and its float64 copy, D included."""
    import sw_oracle as O
    torch.manual_seed(wide_torch_seed(H, nl, Tp))
    o32 = O.SocialWaysOracle(Tp, hidden_size=H, use_social=use_social, n_latent_codes=nl)
    return o32, wide_oracle64(o32)


def wide_oracle64(src, D=None):
    """float64 oracle with the weights of `src` (an oracle or a trainer's G: anything with the four generator modules)
    and of the discriminator D (default src.D)."""
    import sw_oracle as O
    H, nl, Tp = src.encoder.hidden_size, (D or src.D).latent_decoder[2].out_features, (D or src.D).n_next
    with _f64():
        o64 = O.SocialWaysOracle(Tp, hidden_size=H, use_social=src.use_social, n_latent_codes=nl)
    for n in G_NAMES:
        getattr(o64, n).double().load_state_dict({k: v.detach().cpu().double() for k, v in getattr(src, n).state_dict().items()})
    o64.D.double().load_state_dict({k: v.detach().cpu().double() for k, v in (D or src.D).state_dict().items()})
    return o64


def wide_inputs(B, To, Tp, H):
    """seed -> (obsv (B, To, 2), real future (B, Tp, 2): one random walk, noise (B, H / 2), cotangent (B, Tp, 4))."""
    def make(seed):
        g = torch.Generator().manual_seed(seed)
        walk = (torch.randn(B, To + Tp, 2, generator=g) * 0.1).cumsum(1)
        return (walk[:, :To].contiguous(), walk[:, To:].contiguous(), torch.rand(B, H // 2, generator=g),
                torch.randn(B, Tp, 4, generator=g) * 0.1)
    return make


def wide_ambiguous(o64, inp, sb, Tp):
    """Kink inputs within MARGIN of 0 in the float64 forward of the generator and of D on the fake and the real future."""
    import sw_oracle as O
    o, real, z = inp[0].double(), inp[1].double(), inp[2].double()

    def fn():
        o4, p4 = O.get_traj_4d(o, real)
        fake = o64.predict(o, z, Tp, sb)
        o64.D(o4, fake)
        o64.D(o4, p4)
    return gen_ambiguous(o64, fn, [o64.D])


def wide_pick(o64, B, To, Tp, H, sb):
    seed, inp, n_amb = pick_fewest(wide_inputs(B, To, Tp, H), lambda inp: wide_ambiguous(o64, inp, sb, Tp))
    return seed, inp, n_amb
