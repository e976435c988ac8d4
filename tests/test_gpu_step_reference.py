"""The assembled training step - SocialWaysTrainer.step() / step_many() in one process - against the float64 step of
tests/_step_ref.py, at the bound its kernels are held to one by one.

Every trainer here has lr_g = lr_d = 0.0: wg_adam_fin computes w - 0 * m / denom = w, so the weights stay what they were
(asserted after every step with torch.equal on D._flat and G._flat_all) and every gradient of every step - both D updates,
the G phase, eager or replayed from a graph - is taken at known weights.  After EVERY step: losses_from(out) and the ADE/FDE row
(_close_out), p.grad of every D and every generator parameter (close_grads_branch_consistent, GRAD_REL per tensor), finite,
and zero exactly where the reference is exactly zero (embedder / attention without a pair, the latent decoder without the
info loss) and nowhere else.  What that pins beyond the kernels: the loss scales 1 / Bg and w_info / (2 Bg) from global_B,
which D weights the generator phase sees, the L2 and variety terms on d/d(pred_hat), r = 19 - row0, obs_len and z staged by
address into a captured graph, and the shard arguments of step().

a. switches  U 0 / 1 / 2, no info loss, L2, variety as written (row 19 inside the 17-agent scene), "fixed" (k = 3, + L2, with
             last_variety against the reference's arg-min), no social block, hidden size 32 (zero-padded, z 16 wide);
             SMALL at Tp = 25 (generator phase without sw_disc_dpred) and (To, Tp) = (3, 2);
b. routes    eager; five steps through the graph (2 eager, capture, 2 replays, five draws); step_many of 4, four launches; z
             resident on the device - each asserted as taken (tr._graphs, the call log of _lib);
c. ragged    obs_len[i] = 2 + (5 i) % 7 (lengths 2 and 8 share a tile and a scene), NaN padding: default route, ragged_fused
             eager, ragged_fused through the graph with obs_len changing between replays (second rule 2 + (3 i) % 7),
             step_many(obs_len=[...]);
d. shards    the shards of shard_scenes(sb, 2) and (sb, 3) stepped one after the other on one trainer with global_B = 43 and
             global_row0 = r0; loss rows and p.grad added in float64 and held to the full-batch reference: plain, ragged,
             variety as written, "fixed".

Shapes: SIZES43 (43 agents: single agents, a scene above one 16-row tile, a partial last tile) at To = 8, Tp = 12 unless said.
Seed rule of tests/_ref64.py over all draws of a case.  Observed on an MI355X, largest max|err| / max|ref| (outputs;
gradients), pytest -s: a.switches 3.9e-7; 1.05e-5.  b.routes 3.1e-7; 2.3e-6.  c.ragged 3.4e-7; 9.1e-6.
d.shards 2.8e-7; 1.9e-6.  No ambiguous unit at the picked seeds; the 27 cases take 11 s together.  """
import numpy as np
import pytest
import torch

import _step_ref as S
from _ref64 import MAX_AMBIGUOUS, _close_out, _report, close_grads_branch_consistent, scene_rows  # noqa: F401
from test_gpu_ragged import padded
from test_gpu_ragged_train import NAN, dev_len, mixes_a_tile_and_a_scene

pytestmark = pytest.mark.gpu

SIZES43 = [1, 5, 17, 8, 3, 9]
SMALL = [5, 1, 9, 4, 2]
SS = 0.25          # not 1: the ADE/FDE row and g_l2 carry it


def rule_a(B):
    return (2 + (5 * np.arange(B)) % 7).astype(np.int32)


def rule_b(B):
    return (2 + (3 * np.arange(B)) % 7).astype(np.int32)


@pytest.fixture
def calls(monkeypatch):
    """[(entry point, args)] of every socialways_amd._lib.call made while the test runs."""
    from socialways_amd import _lib as L
    seen, real = [], L.call

    def recorded(name, *args):
        seen.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(L, "call", recorded)
    return seen


def _names(calls):
    return [n for n, _ in calls]


class Case:
    """A trainer with lr = 0, the float64 oracle with its weights, and the draws the seed rule picked."""

    def __init__(self, sizes, To, Tp, f, n_steps=1, lens=None, H=64, use_social=True, **kw):
        import socialways_amd as sw
        torch.manual_seed(4000 + Tp + H)
        self.tr = sw.SocialWaysTrainer(Tp, hidden_size=H, lr_g=0.0, lr_d=0.0, use_social=use_social, device="cuda:0",
                                       **S.trainer_kw(f), **kw)
        assert type(self.tr) is sw.SocialWaysTrainer
        self.f, self.Tp, self.sizes, self.B, self.sb = f, Tp, sizes, int(np.sum(sizes)), scene_rows(sizes)
        self.pairs = use_social and max(sizes) > 1
        self.orc = S.oracle_of(self.tr.G, self.tr.D, Tp, H, use_social)
        self.lens = lens
        make = S.make_draws(sizes, To, Tp, H // 2, n_steps, f.variety_k - 1 if f.variety == "fixed" else 0)
        self.seed, self.draws, self.n_amb = S.pick_draws(make, self.orc, self.sb, f, lens)
        assert self.n_amb <= MAX_AMBIGUOUS, (self.seed, self.n_amb)
        self.tag = "seed %d, %d kink inputs near 0" % (self.seed, self.n_amb)
        self.w0 = (self.tr.D._flat.clone(), self.tr.G._flat_all.clone())

    def ref(self, i, **kw):
        o, p, zv, ov, z, vn = self.draws[i]
        ln = None if self.lens is None else self.lens[i]
        return S.step64(self.orc, self.orc.D, o, p, self.sb, zv, ov, z, ss=SS, obs_len=ln, variety_noise=vn, flags=self.f,
                        seed=self.seed, **kw)

    def device_draw(self, i, z_on_device=False, fill=NAN):
        """(obsv, pred, zeros_val, ones_val, z) of step i as the trainer takes them; a ragged observation is NaN in front of
        every row's valid frames."""
        o, p, zv, ov, z, _ = self.draws[i]
        if self.lens is not None:
            o = padded(o, self.lens[i], fill)
        return o.cuda(), p.cuda(), zv, ov, (z.cuda() if z_on_device else z)

    def premise(self):
        torch.cuda.synchronize()
        assert torch.equal(self.tr.D._flat, self.w0[0]) and torch.equal(self.tr.G._flat_all, self.w0[1]), "lr = 0 moved a weight"

    def compare(self, out, d_got, g_got, ref, group, tag):
        tag = "%s, %s" % (tag, self.tag)
        losses = self.tr.losses_from(out, [self.B], self.Tp, SS)[0]
        _close_out(torch.from_numpy(losses), torch.from_numpy(ref.losses), "MSE terms", group, tag)
        _close_out(out[-1, :2], torch.tensor([ref.ade, ref.fde]), "ADE/FDE sums", group, tag)
        close_grads_branch_consistent(d_got, ref.d_run, group, tag + ", D")
        close_grads_branch_consistent(g_got, ref.g_run, group, tag + ", G")
        for got, want in ((d_got, ref.d_run.grads()), (g_got, ref.g_run.grads())):
            for k, g in got.items():
                zero_ok = ((not self.pairs and k.startswith(("feature_embedder.", "attention.")))
                           or (not self.f.info and k.startswith("latent_decoder.")))
                assert bool(torch.isfinite(g).all()), (k, tag)
                assert bool(want[k].any()) != zero_ok, "the reference of %s is%s all zero (%s)" % (k, "" if zero_ok else " not", tag)
                assert bool(g.any()) != zero_ok, "d/d%s is%s all zero (%s)" % (k, "" if zero_ok else " not", tag)

    def check(self, out, i, group, tag=""):
        """Everything a step leaves, against the float64 step of draw i."""
        self.premise()
        d_got, g_got = S.trainer_grads(self.tr)
        ref = self.ref(i)
        self.compare(out, d_got, g_got, ref, group, "step %d%s" % (i + 1, tag))
        return ref


def _step(c, i, **kw):
    o, p, zv, ov, z = c.device_draw(i, kw.pop("z_on_device", False))
    ln = kw.pop("obs_len", None)
    vn = c.draws[i][5]
    return c.tr.step(o, p, c.sb, zv, ov, z, SS, variety_noise=vn, obs_len=ln, **kw)


# ---- a. switches ----------------------------------------------------------------------------------------------------------------
SWITCHES = {
    "u0": (S.flags(U=0), {}), "u1": (S.flags(), {}), "u2": (S.flags(U=2), {}), "noinfo": (S.flags(info=False), {}),
    "l2": (S.flags(l2=True), {}), "variety": (S.flags(variety=True), {}),
    "fixed": (S.flags(variety="fixed", variety_k=3, l2=True), {}), "nosocial": (S.flags(), dict(use_social=False)),
    "hidden32": (S.flags(), dict(H=32))}


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_switches(name):
    f, kw = SWITCHES[name]
    c = Case(SIZES43, 8, 12, f, **kw)
    assert c.sb[2, 0] <= 19 < c.sb[2, 1] and c.sizes[2] == 17          # row 19 lies inside the 17-agent scene
    out = _step(c, 0)
    ref = c.check(out, 0, "a.switches", " (%s)" % name)
    assert out.shape == (f.U + 3, 3)
    if name == "fixed":
        l2min, kmin = c.tr.last_variety
        km, want = kmin.cpu().long(), ref.kmin
        chosen, best = ref.l2_k[km, torch.arange(c.B)], ref.l2_k.min(0).values
        # another sample than the reference's only where the two tie within the fp32 rounding of a 24-term sum of squares
        assert bool(((km == want) | (chosen <= best * (1 + 1e-6))).all()), "last_variety: another sample than the reference's arg-min"
        _close_out(l2min, best, "per-agent best-of-K error", "a.switches", c.tag)
    if name == "hidden32":      # the padding of the packed gradient buffers stays zero, and z is 16 wide
        assert c.draws[0][4].shape == (43, 16) and c.tr.D._true is not None
        for m in (c.tr.D, c.tr.G.encoder, c.tr.G.decoder, c.tr.G.feature_embedder, c.tr.G.attention):
            assert not bool((m._gflat * (1 - m.pad_mask())).any()), type(m).__name__


def test_generator_phase_without_the_one_launch_d_pass(calls):
    """Tp = 25: past the LDS of sw_disc_dpred, the generator phase forms d/d(pred_hat) with sw_disc_fwd + sw_disc_bwd_gan."""
    from socialways_amd import ops
    c = Case(SMALL, 8, 25, S.flags())
    assert c.B == 21 and not ops.disc_dpred_supported(25)
    out = _step(c, 0)
    assert "sw_disc_dpred" not in _names(calls) and "sw_disc_bwd_gan" in _names(calls)
    c.check(out, 0, "a.switches", " (Tp 25)")


def test_short_history_and_horizon():
    c = Case(SIZES43, 3, 2, S.flags())
    c.check(_step(c, 0), 0, "a.switches", " (To 3, Tp 2)")


# ---- b. routes -------------------------------------------------------------------------------------------------------------------
def test_route_eager(calls):
    c = Case(SIZES43, 8, 12, S.flags(), n_steps=2, use_graph=False)
    for i in range(2):
        out = _step(c, i)
        c.check(out, i, "b.routes", " (eager)")
    assert not c.tr._graphs and "sw_gen_images" in _names(calls)
    assert not any(n.startswith("sw_stage_step") for n in _names(calls))


@pytest.mark.parametrize("z_on_device", [False, True])
def test_route_graph_five_steps(calls, z_on_device):
    c = Case(SIZES43, 8, 12, S.flags(), n_steps=5)
    assert c.tr.use_graph
    for i in range(5):
        del calls[:]
        out = _step(c, i, z_on_device=z_on_device)
        assert len(c.tr._graphs) == 1 and [(k[-2], k[-1]) for k in c.tr._graphs] == [(False, z_on_device)]      # (ragged, z by address)
        st = next(iter(c.tr._graphs.values()))
        assert (st["graph"] is not None) == (i >= 2) and st["n"] == min(i + 1, 2)
        staged = [a for n, a in calls if n == "sw_stage_step_zdev"]
        if i < 2:        # eager, through the staging launch
            assert len(staged) == 1 and staged[0][-2] == int(z_on_device)
        elif i == 2:     # recorded twice, replayed once
            assert len(staged) == 2
        else:            # replayed: no launch of ours
            assert not calls and st["flip"] == i % 2
        c.check(out, i, "b.routes", " (graph%s)" % (", z on the device" if z_on_device else ""))


def test_route_step_many_of_four():
    c = Case(SIZES43, 8, 12, S.flags(), n_steps=16)
    for r in range(4):
        outs = c.tr.step_many([c.device_draw(i) for i in range(4 * r, 4 * r + 4)], c.sb, SS)
        torch.cuda.synchronize()
        assert len(c.tr._graphs) == 1 and [k[5] for k in c.tr._graphs] == [4]
        assert (next(iter(c.tr._graphs.values()))["graph"] is not None) == (r >= 2)
        # p.grad is the last step's; the loss rows of all four are the launch's
        c.premise()
        d_got, g_got = S.trainer_grads(c.tr)
        for j in range(4):
            ref = c.ref(4 * r + j)
            tag = "launch %d step %d, %s" % (r + 1, j + 1, c.tag)
            losses = c.tr.losses_from(outs[j], [c.B], c.Tp, SS)[0]
            _close_out(torch.from_numpy(losses), torch.from_numpy(ref.losses), "MSE terms", "b.routes", tag)
            _close_out(outs[j][-1, :2], torch.tensor([ref.ade, ref.fde]), "ADE/FDE sums", "b.routes", tag)
        c.compare(outs[3], d_got, g_got, ref, "b.routes", "launch %d step 4" % (r + 1))


# ---- c. ragged -------------------------------------------------------------------------------------------------------------------
def _lens(n, rules):
    lens = [r(43) for r in rules]
    assert len(lens) == n and all(mixes_a_tile_and_a_scene(ln, scene_rows(SIZES43), 8) for ln in lens)
    return lens


def test_ragged_default_route(calls):
    c = Case(SIZES43, 8, 12, S.flags(), lens=_lens(1, [rule_a]))
    out = _step(c, 0, obs_len=c.lens[0])
    assert not c.tr._graphs and not c.tr.ragged_fused
    assert "sw_disc_fwd_ragged" in _names(calls) and "sw_disc_update_ragged" not in _names(calls)
    c.check(out, 0, "c.ragged", " (default route)")


def test_ragged_fused_eager(calls):
    c = Case(SIZES43, 8, 12, S.flags(), lens=_lens(1, [rule_a]), ragged_fused=True, use_graph=False)
    out = _step(c, 0, obs_len=dev_len(c.lens[0]))
    assert not c.tr._graphs and "sw_disc_update_ragged" in _names(calls) and "sw_disc_fwd_ragged" not in _names(calls)
    c.check(out, 0, "c.ragged", " (fused, eager)")


def test_ragged_fused_graph_with_obs_len_changing_between_replays(calls):
    c = Case(SIZES43, 8, 12, S.flags(), n_steps=5, lens=_lens(5, [rule_a, rule_b, rule_a, rule_b, rule_a]), ragged_fused=True)
    assert c.tr.use_graph and not np.array_equal(c.lens[3], c.lens[4])
    for i in range(5):
        del calls[:]
        ln = dev_len(c.lens[i]) if i % 2 else c.lens[i]       # a device tensor travels unread, a host array is checked first
        out = _step(c, i, obs_len=ln)
        assert len(c.tr._graphs) == 1 and [(k[-2], k[-1]) for k in c.tr._graphs] == [(True, False)]
        st = next(iter(c.tr._graphs.values()))
        assert (st["graph"] is not None) == (i >= 2)
        if i >= 3:
            assert not calls and torch.equal(st["obs_len"].cpu(), torch.from_numpy(c.lens[i]))
        c.check(out, i, "c.ragged", " (fused, graph)")


def test_ragged_step_many(calls):
    c = Case(SIZES43, 8, 12, S.flags(), n_steps=12, lens=_lens(12, [rule_a, rule_b] * 6), ragged_fused=True)
    for r in range(3):
        idx = range(4 * r, 4 * r + 4)
        outs = c.tr.step_many([c.device_draw(i) for i in idx], c.sb, SS, obs_len=[c.lens[i] for i in idx])
        torch.cuda.synchronize()
        assert [(k[5], k[-2]) for k in c.tr._graphs] == [(4, True)]
        c.premise()
        d_got, g_got = S.trainer_grads(c.tr)
        for j, i in enumerate(idx):
            ref = c.ref(i)
            tag = "launch %d step %d, %s" % (r + 1, j + 1, c.tag)
            losses = c.tr.losses_from(outs[j], [c.B], c.Tp, SS)[0]
            _close_out(torch.from_numpy(losses), torch.from_numpy(ref.losses), "MSE terms", "c.ragged", tag)
            _close_out(outs[j][-1, :2], torch.tensor([ref.ade, ref.fde]), "ADE/FDE sums", "c.ragged", tag)
        c.compare(outs[3], d_got, g_got, ref, "c.ragged", "launch %d step 4 (step_many)" % (r + 1))
    assert next(iter(c.tr._graphs.values()))["graph"] is not None


# ---- d. shards in one process ---------------------------------------------------------------------------------------------------
SHARDED = {"plain": (S.flags(), False), "ragged": (S.flags(), True), "variety": (S.flags(variety=True), False),
           "fixed": (S.flags(variety="fixed", variety_k=3, l2=True), False)}
_full = {}        # variant -> (weights, seed, the full-batch reference): computed once, shared by both world sizes


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", sorted(SHARDED))
def test_shards_add_up_to_the_full_batch_reference(name, world):
    from socialways_amd.data import shard_scenes
    f, ragged = SHARDED[name]
    c = Case(SIZES43, 8, 12, f, lens=_lens(1, [rule_a]) if ragged else None)
    if name not in _full:
        _full[name] = (c.w0, c.seed, c.ref(0))
    w0, seed, ref = _full[name]
    assert seed == c.seed and torch.equal(w0[0], c.w0[0]) and torch.equal(w0[1], c.w0[1])
    o, p, zv, ov, z = c.device_draw(0)
    vn, K1, B = c.draws[0][5], f.variety_k - 1, c.B
    out_sum, d_sum, g_sum, owners = 0.0, None, None, []
    shards = shard_scenes(c.sb, world)
    assert len(shards) == world and all(hi > lo for lo, hi in shards)
    for lo, hi in shards:
        r0, r1 = int(c.sb[lo, 0]), int(c.sb[hi - 1, 1])
        owners.append(r0 <= 19 < r1)
        out = c.tr.step(o[r0:r1], p[r0:r1], c.sb[lo:hi] - r0, zv, ov, z[r0:r1], SS, global_B=B, global_row0=r0,
                        variety_noise=vn.view(K1, B, -1)[:, r0:r1].reshape(K1 * (r1 - r0), -1) if vn is not None else None,
                        obs_len=c.lens[0][r0:r1] if ragged else None)
        c.premise()
        d_got, g_got = S.trainer_grads(c.tr)
        out_sum = out_sum + out.double()
        d_sum = d_got if d_sum is None else {k: d_sum[k] + v for k, v in d_got.items()}
        g_sum = g_got if g_sum is None else {k: g_sum[k] + v for k, v in g_got.items()}
    assert sum(owners) == 1
    c.compare(out_sum, d_sum, g_sum, ref, "d.shards", "%s, %d shards" % (name, world))
