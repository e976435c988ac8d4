"""The assembled training step of the two other engines - WideTrainer.step() (socialways_amd/wide.py: _step_device, _capture /
_replay) and GenericTrainer.step() (socialways_amd/generic.py: the _Mse / k = B / Bg arithmetic under torch's tape) - against
the float64 step of tests/_step_ref.py, at the bounds of tests/_ref64.py unchanged (OUT_RT / OUT_AT, GRAD_REL per tensor).
tests/test_gpu_wide_reference.py holds the wide engine's phases one by one and drives them itself; this module holds the order
and the scales step() calls them with.  test_gpu_step_reference.py is the same for the fused 64-unit trainer.

Every trainer of parts a - d has lr_g = lr_d = 0.0, so the weights stay what they were (asserted after every step with
torch.equal: gp.flat / dp.flat of the wide engine, every parameter of the generic one) and the U + 1 discriminator updates
and the generator phase of every step differentiate at the same known weights.  After EVERY step: losses_from(out) and the
ADE/FDE row (_close_out), every D and every generator gradient (close_grads_branch_consistent), finite, and zero exactly where
the reference is exactly zero (embedder / attention without a pair, latent_decoder.* without the info loss) and nowhere else.
Where the gradients are read (tests/_step_ref.py): wide - dp.gflat / gp.gflat after the step (the last D update's gradient
and G's), and on an eager step also each of the U + 1 D buckets and the G bucket as _allreduce is handed them; generic - D's
p.grad in front of every _reduce_grads(D_optimizer), G's p.grad after the step.

a. engines   one eager step, default flags, the launch forms (tr.seq, tr.decloop, tr.heads) asserted: wide 64 units with 3
             codes (sequence kernel, per-step decode, nlp padding), 96 (per-step LSTM), 128 (sequence, decode loop, fused heads:
             the lpart loss route), 128 with 17 codes (past the heads' limit: the sw_sqdiff loss route; 2 / nl of _kres and gc at
             nl = 17), 160 at Tp 10 (GEMM heads); generic 80 and 64 with 3 codes.  The loss route is asserted from the call log.
b. switches  U 0 / 2, no info loss, L2, variety as written (row 19 inside the 17-agent scene), L2 + variety, no social block,
             (To, Tp) = (3, 2), Tp 25, 17 single agents (P = 0 with the social block on): wide 128 and generic 80; U 2 and no
             info loss also at 128 / 17 codes, so both loss routes see u > 0 and wi = 0.
c. routes    wide 128, use_graph: five draws, steps 1 - 2 eager, step 3 captures and replays, 4 - 5 replay (zeros_val / ones_val
             change with every draw and travel through w["scal"]); the same with U = 2 at 17 codes; step_many of four.  The
             route is asserted as taken (tr._graphs, the optimizers' counters, no bucket handed over by a replayed step).
d. shards    the shards of shard_scenes(sb, 2) and (sb, 3) stepped one after the other on ONE trainer with global_B = 43 and
             global_row0 = r0, loss rows and gradients cloned after each shard, added in float64 and held to the full-batch
             reference: plain, L2 + variety as written (row 19 addressed globally lives on one shard), 3 codes; wide 128 eager,
             wide 128 with each shard replayed from a graph of its own (one captured key per _row0), generic 80.
e. restore   the one thing lr = 0 cannot see - lr_d = 1e-3, lr_g = 1e-4, bit for bit: a U = 2 and a U = 0 trainer from one torch
             seed, one step on one draw.  D's nn.Linear parameters are equal (both "after the first D update": the
             _d_backup / _lin_mask restore of train.py:541-542), D's LSTM parameters are not, D_optimizer.t is 3 and 1.  Wide 128
             eager, wide 128 replayed from the graph (two eager steps of the layout, weights and Adam state put back, the step
             that counts is the replay - and equals the eager trainer bit for bit, which pins the Adam indices a replayed step
             reads from w["scal"]), generic 80.  The generator is NOT equal in the two: its update differentiates through the
             thrice-updated D (the CPU oracle shows the same, tests/test_step_ref_host.py); it is held to the fp32 oracle's step
             of the same depth instead, within the rounding of one Adam update.

Shapes: SIZES43 (43 agents: single agents, a scene above one 16-row tile, a partial last tile, row 19 inside the 17-agent
scene) at To = 8, Tp = 12, SS = 0.25 unless said.  Weights: the draw of _ref64.wide_torch_seed(H, nl, Tp), the cases
tests/test_step_ref_host.py checks on the CPU first (seed rule, the fp32 oracle within half of these bounds).  Seed rule of
tests/_ref64.py over all draws of a case.

Observed on an MI355X, largest max|err| / max|ref| (outputs; gradients), pytest -s: a.engines 1.2e-7; 4.6e-6.  b.switches 7.8e-8;
4.0e-6.  c.routes 1.2e-7; 3.6e-6.  d.shards 1.2e-7; 7.2e-6.  No ambiguous unit at the picked seeds; part e is bit for bit; the 53
cases take 11 s together.  

What the module turned up: no fault of the two engines - every case passed as first written, and the product code is unchanged.
One statement of the plan behind it did not hold and is not asserted: that the generator of the U = 2 and of the U = 0 trainer
of part e are equal after the step.  The generator's update differentiates through the D of the step's last update, which
U changes; the CPU oracle's own two runs differ in at least 20 of the generator's 22 tensors
(test_step_ref_host.py::test_unrolling_changes_the_oracles_generator_update_and_restores_the_linear_layers_of_d).  Each
generator is held to the oracle's step of its own depth instead."""
import numpy as np
import pytest
import torch

import sw_oracle as O
import _step_ref as S
from _ref64 import MAX_AMBIGUOUS, _close_out, _report, close_grads_branch_consistent, scene_rows, wide_torch_seed  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES43 = [1, 5, 17, 8, 3, 9]
SINGLES = [1] * 17
SS = 0.25          # not 1: the ADE/FDE row and g_l2 carry it
LR_D, LR_G = 1e-3, 1e-4


def _engine(name):
    from socialways_amd.generic import GenericTrainer
    from socialways_amd.wide import WideTrainer
    return {"wide": WideTrainer, "generic": GenericTrainer}[name]


@pytest.fixture
def calls(monkeypatch):
    """[entry point] of every socialways_amd._lib.call made while the test runs."""
    from socialways_amd import _lib as L
    seen, real = [], L.call

    def recorded(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, "call", recorded)
    return seen


def _build(engine, H, nl, Tp, f, use_social=True, use_graph=False, lr_g=0.0, lr_d=0.0):
    cls = _engine(engine)
    torch.manual_seed(wide_torch_seed(H, nl, Tp))
    tr = cls(Tp, hidden_size=H, n_latent_codes=nl, lr_g=lr_g, lr_d=lr_d, use_social=use_social, device="cuda:0",
             use_graph=use_graph, **S.trainer_kw(f))
    assert type(tr) is cls and tr.n_latent_codes == nl and tr.n_unrolling_steps == f.U and tr.use_info_loss == f.info
    assert tr.loss_info_w == S.W_INFO and tr.loss_l2_w == S.W_L2 and tr.use_graph == (use_graph and engine == "wide")
    return tr


def _weights(tr):
    if hasattr(tr, "dp"):
        return [tr.dp.flat.clone(), tr.gp.flat.clone()]
    return [q.detach().clone() for q in list(tr.D.parameters()) + list(tr.G.parameters())]


class Case:
    """A trainer of the named engine with lr = 0, the float64 oracle with its weights, the draws the seed rule picked."""

    def __init__(self, engine, H, nl=2, f=None, sizes=SIZES43, To=8, Tp=12, n_steps=1, use_social=True, forms=None, use_graph=False):
        f = S.flags() if f is None else f
        self.tr = _build(engine, H, nl, Tp, f, use_social, use_graph)
        self.wide = engine == "wide"
        if forms is not None:
            got = (self.tr.seq, self.tr.decloop, self.tr.heads)
            assert got == forms, "launch forms of %s %d / %d codes: %s" % (engine, H, nl, got)
        self.f, self.Tp, self.sizes, self.B, self.sb = f, Tp, sizes, int(np.sum(sizes)), scene_rows(sizes)
        self.pairs = use_social and max(sizes) > 1
        self.orc = S.oracle_of(self.tr.G, self.tr.D, Tp, H, use_social)
        assert self.orc.n_latent_codes == nl == S.n_codes(self.orc.D)
        self.seed, self.draws, self.n_amb = S.pick_draws(S.make_draws(sizes, To, Tp, H // 2, n_steps), self.orc, self.sb, f)
        assert self.n_amb <= MAX_AMBIGUOUS, (self.seed, self.n_amb)
        self.tag = "%s %d units %d codes, seed %d, %d kink inputs near 0" % (engine, H, nl, self.seed, self.n_amb)
        self.w0 = _weights(self.tr)
        self.d_taps, self.g_taps = S.tap_updates(self.tr)

    def ref(self, i, **kw):
        o, p, zv, ov, z, _ = self.draws[i]
        return S.step64(self.orc, self.orc.D, o, p, self.sb, zv, ov, z, ss=SS, flags=self.f, seed=self.seed, **kw)

    def device_draw(self, i):
        o, p, zv, ov, z, _ = self.draws[i]
        return o.cuda(), p.cuda(), zv, ov, z

    def step(self, i, **kw):
        del self.d_taps[:], self.g_taps[:]
        o, p, zv, ov, z = self.device_draw(i)
        return self.tr.step(o, p, self.sb, zv, ov, z, SS, **kw)

    def premise(self):
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(_weights(self.tr), self.w0)), "lr = 0 moved a weight"

    def grads(self):
        """(D's, the generator's) gradients as the step left them."""
        if self.wide:
            return S.wide_grads(self.tr)
        return S.generic_grads(self.tr, self.d_taps[-1])

    def compare_grads(self, d_got, g_got, ref, group, tag):
        if d_got is not None:
            close_grads_branch_consistent(d_got, ref.d_run, group, tag + ", D")
        if g_got is not None:
            close_grads_branch_consistent(g_got, ref.g_run, group, tag + ", G")
        for got, want in ((d_got, ref.d_run.grads()), (g_got, ref.g_run.grads())):
            for k, g in ({} if got is None else got).items():
                zero_ok = ((not self.pairs and k.startswith(("feature_embedder.", "attention.")))
                           or (not self.f.info and k.startswith("latent_decoder.")))
                assert bool(torch.isfinite(g).all()), (k, tag)
                assert bool(want[k].any()) != zero_ok, "the reference of %s is%s all zero (%s)" % (k, "" if zero_ok else " not", tag)
                assert bool(g.any()) != zero_ok, "d/d%s is%s all zero (%s)" % (k, "" if zero_ok else " not", tag)

    def compare_out(self, out, ref, group, tag):
        assert out.shape == (self.f.U + 3, 3) and out.dtype == torch.float64
        losses = self.tr.losses_from(out, [self.B], self.Tp, SS)[0]
        _close_out(torch.from_numpy(losses), torch.from_numpy(ref.losses), "MSE terms", group, tag)
        _close_out(out[-1, :2], torch.tensor([ref.ade, ref.fde]), "ADE/FDE sums", group, tag)

    def compare_taps(self, ref, group, tag, eager=True):
        """What each update of the step was made from: U + 1 D buckets and the G bucket of an eager wide step (none of a
        replayed one), D's p.grad in front of each of the generic engine's U + 1 D updates and G's in front of its one."""
        n_d, n_g = ((self.f.U + 1, 1) if eager else (0, 0))
        assert (len(self.d_taps), len(self.g_taps)) == (n_d, n_g), (len(self.d_taps), len(self.g_taps), tag)
        for u, t in enumerate(self.d_taps):
            self.compare_grads(S.wide_grads(self.tr, d_flat=t)[0] if self.wide else t, None, ref, group, "%s, D update %d" % (tag, u + 1))
        for t in self.g_taps:
            self.compare_grads(None, S.wide_grads(self.tr, g_flat=t)[1] if self.wide else t, ref, group, tag + ", G update")

    def check(self, out, i, group, tag="", eager=True):
        """Everything a step leaves, against the float64 step of draw i."""
        self.premise()
        tag = "step %d%s, %s" % (i + 1, tag, self.tag)
        ref = self.ref(i)
        self.compare_out(out, ref, group, tag)
        self.compare_grads(*self.grads(), ref, group, tag)
        self.compare_taps(ref, group, tag, eager)
        return ref


def _row_19_is_inside_the_large_scene(c):
    assert c.sb[2, 0] <= 19 < c.sb[2, 1] and c.sizes[2] == 17


# ---- a. engines and launch forms --------------------------------------------------------------------------------------------------
# id -> (engine, H, nl, Tp, (seq, decloop, heads) the row was chosen for)
ENGINES = {
    "wide-h64-nl3": ("wide", 64, 3, 12, (True, False, True)),           # sequence kernel, per-step decode, nlp padding
    "wide-h96": ("wide", 96, 2, 12, (False, False, True)),              # per-step LSTM
    "wide-h128": ("wide", 128, 2, 12, (True, True, True)),              # sequence, decode loop, fused heads: the lpart loss route
    "wide-h128-nl17": ("wide", 128, 17, 12, (True, True, False)),       # past the heads' limit: the sw_sqdiff loss route
    "wide-h160-tp10": ("wide", 160, 2, 10, (False, False, False)),      # GEMM heads
    "generic-h80": ("generic", 80, 2, 12, None),
    "generic-h64-nl3": ("generic", 64, 3, 12, None),
}


@pytest.mark.parametrize("name", sorted(ENGINES))
def test_engines_and_launch_forms(name, calls):
    engine, H, nl, Tp, forms = ENGINES[name]
    c = Case(engine, H, nl, Tp=Tp, forms=forms)
    _row_19_is_inside_the_large_scene(c)
    del calls[:]
    out = c.step(0)
    if c.wide:          # the loss route: the fused heads write lpart[u], the other one is 3 (U + 1) + 2 sw_sqdiff calls
        assert not c.tr._graphs
        assert calls.count("sw_sqdiff") == (0 if forms[2] else 3 * (c.f.U + 1) + 2)
        assert calls.count("sw_wide_disc_heads_fwd") == (c.f.U + 2 if forms[2] else 0)
    c.check(out, 0, "a.engines", " (%s)" % name)


# ---- b. switches ------------------------------------------------------------------------------------------------------------------
# id -> (flags, Case keywords)
SWITCHES = {
    "u0": (S.flags(U=0), {}), "u2": (S.flags(U=2), {}), "noinfo": (S.flags(info=False), {}), "l2": (S.flags(l2=True), {}),
    "variety": (S.flags(variety=True), {}), "l2-variety": (S.flags(l2=True, variety=True), {}),
    "nosocial": (S.flags(), dict(use_social=False)), "to3-tp2": (S.flags(), dict(To=3, Tp=2)), "tp25": (S.flags(), dict(Tp=25)),
    "singles": (S.flags(), dict(sizes=SINGLES))}
TRAINERS = {"wide-h128": ("wide", 128, 2), "wide-h128-nl17": ("wide", 128, 17), "generic-h80": ("generic", 80, 2)}
SWITCH_CASES = ([("wide-h128", s) for s in sorted(SWITCHES)] + [("wide-h128-nl17", "u2"), ("wide-h128-nl17", "noinfo")]
                + [("generic-h80", s) for s in sorted(SWITCHES)])


@pytest.mark.parametrize("trainer,switch", SWITCH_CASES, ids=["%s-%s" % c for c in SWITCH_CASES])
def test_switches(trainer, switch):
    engine, H, nl = TRAINERS[trainer]
    f, kw = SWITCHES[switch]
    c = Case(engine, H, nl, f, **kw)
    if switch == "singles":
        assert c.B == 17 and not c.pairs and c.tr.G.use_social         # P = 0 with the social block on
    elif "sizes" not in kw:
        _row_19_is_inside_the_large_scene(c)
    if trainer == "wide-h128-nl17":
        assert not c.tr.heads
    out = c.step(0)
    c.check(out, 0, "b.switches", " (%s)" % switch)


# ---- c. routes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl,U", [(2, 1), (17, 2)])
def test_route_graph_five_steps(nl, U):
    c = Case("wide", 128, nl, S.flags(U=U), n_steps=5, use_graph=True, forms=(True, True, nl == 2))
    labels = [(d[2], d[3]) for d in c.draws]
    assert len(set(labels)) == 5                                       # zeros_val / ones_val of every step are its own
    for i in range(5):
        out = c.step(i)
        assert len(c.tr._graphs) == (1 if i >= 2 else 0)
        assert c.tr.D_optimizer.t == (U + 1) * (i + 1) and c.tr.predictor_optimizer.t == i + 1
        c.check(out, i, "c.routes", " (graph)", eager=i < 2)
    if (nl, U) == (2, 1):
        assert c.tr.D_optimizer.t == 10 and c.tr.predictor_optimizer.t == 5
    assert len(c.tr._graphs) == 1 and len(next(iter(c.tr._graphs.values()))["segments"]) == 1


def test_route_step_many_of_four():
    c = Case("wide", 128, 2, S.flags(), n_steps=4, use_graph=True)
    del c.d_taps[:], c.g_taps[:]
    outs = c.tr.step_many([c.device_draw(i) for i in range(4)], c.sb, SS)
    assert len(outs) == 4 and len(c.tr._graphs) == 1 and c.tr.D_optimizer.t == 8 and c.tr.predictor_optimizer.t == 4
    assert (len(c.d_taps), len(c.g_taps)) == (4, 2)                    # two eager steps, then the graph
    c.premise()
    for j in range(4):
        ref = c.ref(j)
        c.compare_out(outs[j], ref, "c.routes", "step_many step %d, %s" % (j + 1, c.tag))
    c.compare_grads(*c.grads(), ref, "c.routes", "step_many step 4, %s" % c.tag)      # the buffers hold the last step's


# ---- d. shards in one process -----------------------------------------------------------------------------------------------------
SHARDED = {"plain": (S.flags(), 2), "l2-variety": (S.flags(l2=True, variety=True), 2), "nl3": (S.flags(), 3)}
SHARD_ENGINES = {"wide-h128": ("wide", 128, False), "wide-h128-graph": ("wide", 128, True), "generic-h80": ("generic", 80, False)}
_full = {}        # (H, variant) -> (weights, seed, the full-batch reference): computed once, shared by the world sizes and routes


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("variant", sorted(SHARDED))
@pytest.mark.parametrize("trainer", sorted(SHARD_ENGINES))
def test_shards_add_up_to_the_full_batch_reference(trainer, variant, world):
    from socialways_amd.data import shard_scenes
    engine, H, graph = SHARD_ENGINES[trainer]
    f, nl = SHARDED[variant]
    c = Case(engine, H, nl, f, use_graph=graph)
    _row_19_is_inside_the_large_scene(c)
    if (H, variant) not in _full:
        _full[H, variant] = (c.w0, c.seed, c.ref(0))
    w0, seed, ref = _full[H, variant]
    assert seed == c.seed and all(torch.equal(a, b) for a, b in zip(w0, c.w0))
    o, p, zv, ov, z = c.device_draw(0)
    out_sum, d_sum, g_sum, owners = 0.0, None, None, []
    shards = shard_scenes(c.sb, world)
    assert len(shards) == world and all(hi > lo for lo, hi in shards)
    for lo, hi in shards:
        r0, r1 = int(c.sb[lo, 0]), int(c.sb[hi - 1, 1])
        owners.append(r0 <= 19 < r1)
        for _ in range(3 if graph else 1):        # with the graph: two eager steps of the shard's key, the third is replayed
            del c.d_taps[:], c.g_taps[:]
            out = c.tr.step(o[r0:r1], p[r0:r1], c.sb[lo:hi] - r0, zv, ov, z[r0:r1], SS, global_B=c.B, global_row0=r0)
        c.premise()
        assert not graph or (len(c.d_taps), len(c.g_taps)) == (0, 0)          # the third step of a key is replayed
        d_got, g_got = c.grads()                   # (host copies: the packed buffers are overwritten by the next shard)
        out_sum = out_sum + out.double().clone()
        d_sum = d_got if d_sum is None else {k: d_sum[k] + v for k, v in d_got.items()}
        g_sum = g_got if g_sum is None else {k: g_sum[k] + v for k, v in g_got.items()}
    assert sum(owners) == 1
    if c.wide:
        assert len(c.tr._graphs) == (world if graph else 0)            # a key of its own per _row0
        assert len({k[9] for k in c.tr._seen}) == world and {k[4] for k in c.tr._seen} == {43.0}
    tag = "%s, %s, %d shards, %s" % (trainer, variant, world, c.tag)
    c.compare_out(out_sum, ref, "d.shards", tag)
    c.compare_grads(d_sum, g_sum, ref, "d.shards", tag)


# ---- e. the restore of D's Linear layers: the one thing lr = 0 cannot see ----------------------------------------------------------
def _named_weights(tr):
    return ({k: q.detach().clone() for k, q in tr.D.named_parameters()}, {k: q.detach().clone() for k, q in S._g_named(tr)})


def _reset(tr, w0):
    """Weights and Adam state of a wide trainer back to construction (the graphs and their keys stay)."""
    tr.dp.flat.copy_(w0[0])
    tr.gp.flat.copy_(w0[1])
    for opt in (tr.D_optimizer, tr.predictor_optimizer):
        opt.m.zero_()
        opt.v.zero_()
        opt.t = 0
        opt.step_t.zero_()


_oracle_step = {}      # (H, U) -> the generator of the fp32 oracle after its step of that depth


def _oracle_generator_after_one_step(H, U, draw, sb):
    if (H, U) not in _oracle_step:
        torch.manual_seed(wide_torch_seed(H, 2, 12))
        orc = O.SocialWaysOracle(12, hidden_size=H, use_social=True, lr_g=LR_G, lr_d=LR_D, n_unrolling_steps=U)
        o, p, zv, ov, z, _ = draw
        orc.train_step(o, p, sb, zv, ov, z, SS)
        _oracle_step[H, U] = {k: q.detach().clone() for k, q in S._g_named(orc)}
    return _oracle_step[H, U]


@pytest.mark.parametrize("route", ["wide-h128-eager", "wide-h128-graph", "generic-h80"])
def test_unrolled_updates_restore_the_linear_layers_of_d_and_only_them(route):
    engine, H, graph = {"wide-h128-eager": ("wide", 128, False), "wide-h128-graph": ("wide", 128, True),
                        "generic-h80": ("generic", 80, False)}[route]
    sb = scene_rows(SIZES43)
    draw = S.make_draws(SIZES43, 8, 12, H // 2)(1)[0]
    o, p, zv, ov, z, _ = draw
    after = {}
    for U in (2, 0):
        tr = _build(engine, H, 2, 12, S.flags(U=U), use_graph=graph, lr_g=LR_G, lr_d=LR_D)
        w0 = _weights(tr)
        if U == 2:
            first, init = w0, _named_weights(tr)
        assert all(torch.equal(a, b) for a, b in zip(w0, first))       # one torch seed: the same initial weights
        if graph:       # two eager steps of the layout, then the step that counts - from construction again - is the replay
            for _ in range(2):
                tr.step(o.cuda(), p.cuda(), sb, zv, ov, z, SS)
            _reset(tr, w0)
            assert not tr._graphs
        out = tr.step(o.cuda(), p.cuda(), sb, zv, ov, z, SS)
        torch.cuda.synchronize()
        if graph:
            assert len(tr._graphs) == 1
        t_d = tr.D_optimizer.t if engine == "wide" else int(tr.D_optimizer.state[next(tr.D.parameters())]["step"])
        assert t_d == U + 1
        after[U] = _named_weights(tr) + (out.clone(),)
        if graph:       # ... and equals the eager trainer bit for bit: the Adam indices a replayed step reads from w["scal"]
            twin = _build(engine, H, 2, 12, S.flags(U=U), use_graph=False, lr_g=LR_G, lr_d=LR_D)
            out_t = twin.step(o.cuda(), p.cuda(), sb, zv, ov, z, SS)
            torch.cuda.synchronize()
            assert twin.D_optimizer.t == U + 1 and not twin._graphs
            assert torch.equal(out_t, out) and torch.equal(twin.dp.flat, tr.dp.flat) and torch.equal(twin.gp.flat, tr.gp.flat), U
    (d2, g2, _), (d0, g0, _) = after[2], after[0]
    assert sorted(k for k in d2 if "lstm" in k) == ["obsv_encoder_lstm." + n for n in ("bias_hh_l0", "bias_ih_l0", "weight_hh_l0", "weight_ih_l0")]
    for k in d2:
        assert not torch.equal(d0[k], init[0][k]), "the first update left D's %s where it was" % k
        if "lstm" in k:     # the LSTM keeps its three updates
            assert not torch.equal(d2[k], d0[k]), "D's %s after three updates equals the one after the first" % k
        else:               # every Linear layer is the one after the first update
            assert torch.equal(d2[k], d0[k]), "D's %s was not restored to the first update's" % k
    # The generator's update differentiates through the D of the step's LAST update, so it depends on U (the oracle's does too:
    # test_step_ref_host.py).  Each is held to the fp32 oracle's step of its own depth.  One Adam update moves a weight by at
    # most lr_g (|m / (sqrt(v) + eps)| <= 1 at the first step), so two correct steps differ by 2 lr_g at the most - where the
    # sign of a noise-level gradient differs - and by the rounding of the gradient elsewhere.
    assert sum(not torch.equal(g2[k], g0[k]) for k in g2) >= 20, "the generator's update did not see the D of the last update"
    for U, g in ((2, g2), (0, g0)):
        want = _oracle_generator_after_one_step(H, U, draw, sb)
        d = torch.cat([(q.cpu() - want[k]).abs().reshape(-1) for k, q in g.items()])
        assert all(not torch.equal(q, init[1][k]) for k, q in g.items()), "a generator tensor did not move (U = %d)" % U
        assert float(d.max()) <= 2.2 * LR_G and float((d <= 0.1 * LR_G).float().mean()) > 0.95, (route, U, float(d.max()))
