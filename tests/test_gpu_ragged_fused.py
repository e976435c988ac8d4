"""The fused ragged training step on the GPU (SocialWaysTrainer(ragged_fused=True)): sw_disc_update_ragged,
sw_stage_step_ragged and what is built on them.

a. sw_disc_update_ragged against sw_disc_fwd_ragged + sw_disc_bwd_gan_adam, bit for bit, on NaN-prefilled buffers: a tile with
   one live lane, a partial last tile, the register route (To = 8) and the saved-rows route (To = 5, 3); four length patterns;
   NaN padding against repeated-frame padding; zero rows in front of a row's start; full length against sw_disc_update;
b. the same kernel against float64 (tests/_ragged_ref.py through tests/_ref64.py, GRAD_REL) at one mixed-length case per route;
c. sw_stage_step_ragged against sw_stage_step_zdev on the same slot contents, and its clamped obs_len;
d. five steps of a fused trainer (captured on the third) against a default one (eager), bit for bit - also uncaptured, with
   two unrolling steps + the L2 term, and with z on the device - and a dense step afterwards;
e. step_many(obs_len=[...]) against the step(obs_len=) calls;
f. train_epoch_ragged on the ragged synthetic recording, fused against default, host z and DeviceNoise."""
import numpy as np
import pytest
import torch

from _ref64 import GRAD_REL, _close_grad, _close_out, _pick, _report  # noqa: F401
from test_gpu_disc_reference import TARGETS, W_INFO, _d64, _disc, _grads_of, _tile_sums
from test_gpu_ragged import disc_images, padded
from test_gpu_ragged_train import (NAN, _disc64, _disc_make, _state, bits, dev_len, dsave_parts, mixes_a_tile_and_a_scene,  # noqa: F401
                                   ragged_data, zero_bits)
from test_gpu_sample import crowd

pytestmark = pytest.mark.gpu

Tp = 12
SIZES43 = [1, 5, 17, 8, 3, 9]      # 43 agents: single agents, a scene above one 16-row tile, a partial last tile


def patterns(n, T):
    """full / all two frames / 2 .. T cycling inside every tile / the first tile all short next to the second all full."""
    cyc = ((np.arange(n) % (T - 1)) + 2).astype(np.int32)
    tiles = cyc.copy()
    tiles[:16], tiles[16:32] = 2, T
    return dict(full=np.full(n, T, dtype=np.int32), two=np.full(n, 2, dtype=np.int32), cycle=cyc, tiles=tiles)


def update_pass(D, w0, obsv, preds, z, ln, fused, img, tab):
    """One D update pass with the fused Adam on NaN-prefilled save / delta buffers, from the weights w0: the two launches
    (fused False), sw_disc_update_ragged (True) or, ln None, the dense sw_disc_update -> everything the pass leaves."""
    from socialways_amd import _lib as L, ops
    n, T = obsv.shape[0], obsv.shape[1]
    dev = obsv.device
    D._flat.copy_(w0)
    ws = ops.Workspaces(dev)
    ws.get("d.dsave", L.workspace_floats(L.WS_DSAVE, n, T, Tp, 2)).fill_(NAN)
    ws.get("d.ddelta", L.workspace_floats(L.WS_DDELTA, n, T, Tp, 2)).fill_(NAN)
    L.call("sw_disc_images", L.ptr(D._flat), L.ptr(img), L.ptr(tab), Tp, L.stream())
    try:
        assert ops.disc_update_supported(D._flat, n, T, Tp)
        g, m, v, snap = (torch.zeros_like(D._flat) for _ in range(4))
        part = torch.zeros((n + 15) // 16, 3, device=dev)
        adam = (m, v, torch.ones((), device=dev), 1e-3, 0.9, 0.999, 1e-8)
        targets = torch.tensor(TARGETS, device=dev)
        args = (targets, (0, 1), z, 1.0 / n, W_INFO / (2.0 * n), g)
        if fused:
            kw = {} if ln is None else dict(obs_len=ln)
            labels, codes = ops.disc_update(D._flat, obsv, preds, *args, ws, w_snapshot=snap, loss_part=part, adam=adam, **kw)
        else:
            labels, codes, ctx = ops.disc_forward(D._flat, obsv, preds, save=True, ws=ws, save_lstm=1, w_snapshot=snap, obs_len=ln)
            ops.disc_backward_gan(D._flat, ctx, labels, codes, *args, (), ws=ws, loss_part=part, adam=adam)
        torch.cuda.synchronize()
        sv = dsave_parts(ws.get("d.dsave", 1), n, T, Tp, 2)
        out = dict(label_fake=labels[0], label_real=labels[1], code_fake=codes[0], code_real=codes[1], loss_sums=part, gradients=g,
                   weights=D._flat.clone(), exp_avg=m, exp_avg_sq=v, snapshot=snap, images=img.clone(),
                   h_rows=sv["act"][..., 320:].clone(), x4s=sv["x4s"].clone())
        out.update({k: sv[k].clone() for k in ("o1", "both", "q1", "c1", "l1", "px")})
        return out, sv["act"].clone()
    finally:
        L.call("sw_disc_images", None, None, None, 0, None)


@pytest.mark.parametrize("n,T", [(17, 8), (40, 8), (136, 8), (17, 5), (33, 3)])
def test_update_in_one_launch_equals_the_two_ragged_launches_bit_for_bit(n, T):
    from socialways_amd import _lib as L
    dev = torch.device("cuda:0")
    D = _disc(Tp)
    w0 = D._flat.clone()
    gen = torch.Generator(device="cuda").manual_seed(100 * n + T)
    obsv = ((torch.rand(n, T, 2, device=dev, generator=gen) * 0.1 - 0.03).cumsum(1)).contiguous()
    preds = [(torch.randn(n, Tp, 4, device=dev, generator=gen) * 0.1).contiguous() for _ in range(2)]
    z = torch.rand(n, 32, device=dev, generator=gen)
    lib = L.load()
    tab_h = np.empty((D._flat.numel(), 2), dtype=np.int32)
    assert lib.sw_disc_image_table(Tp, tab_h.ctypes.data) == 0
    tab = torch.from_numpy(tab_h).to(dev)
    img = torch.zeros(lib.sw_disc_image_floats(Tp), device=dev)
    seen = {}
    for name, ln in patterns(n, T).items():
        lnd = dev_len(ln)
        two, _ = update_pass(D, w0, padded(obsv, ln, NAN), preds, z, lnd, False, img, tab)
        one, act = update_pass(D, w0, padded(obsv, ln, NAN), preds, z, lnd, True, img, tab)
        rep, _ = update_pass(D, w0, padded(obsv, ln, "repeat"), preds, z, lnd, True, img, tab)
        for k in two:
            assert bits(two[k], one[k]), "%s, %s: max |diff| %.3e" % (name, k, float((two[k] - one[k]).abs().max()))
            assert bits(one[k], rep[k]), "%s, %s: NaN padding against a repeated frame" % (name, k)
            assert not bool(torch.isnan(one[k]).any()), (name, k)
        assert float(one["gradients"].abs().max()) > 0 and not torch.equal(one["weights"], w0)
        for r in range(n):          # in front of a row's start: all-zero bits (To = 8 saves h and the input alone)
            s = T - int(ln[r])
            rows = one["h_rows"][:s, r] if T == 8 else act[:s, r]
            assert zero_bits(rows) and zero_bits(one["x4s"][:s, r]), (name, r)
            assert float(one["h_rows"][s:, r].abs().min()) > 0, (name, r)
        seen[name] = one
    dense, _ = update_pass(D, w0, obsv, preds, z, None, True, img, tab)
    for k in dense:
        assert bits(seen["full"][k], dense[k]), "full length against sw_disc_update: %s" % k
    for name in ("two", "cycle", "tiles"):
        assert not bits(seen[name]["gradients"], dense["gradients"]), name


@pytest.mark.parametrize("n,T", [(40, 8), (33, 3)])
def test_update_in_one_launch_at_mixed_lengths_against_float64(n, T):
    """Every weight gradient, the outputs and the loss sums of sw_disc_update_ragged against tests/_ragged_ref.disc_ragged in
    float64 - the bound and the seed rule of the two-launch case (GRAD_REL, tests/_ref64.py); -s prints the observed errors."""
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    ln = patterns(n, T)["cycle"]
    assert mixes_a_tile_and_a_scene(ln, [[0, n]], T)
    D = _disc(Tp)
    Dref = _d64(D)
    seed, (obsv, preds, z), margin = _pick(_disc_make(n, T, Tp, 2), lambda inp: _disc64(Dref, inp[0], ln, inp[1])[3][0])
    tag = "seed %d, kink margin %.2e" % (seed, margin)
    ws = ops.Workspaces(dev)
    targets = torch.tensor(TARGETS, device=dev)
    dflat = torch.full_like(D._flat, NAN)
    part = torch.full(((n + 15) // 16, 3), NAN, device=dev)
    with disc_images(D, True):
        labels, codes = ops.disc_update(D._flat, padded(obsv, ln, NAN).to(dev), [p.to(dev) for p in preds], targets, (0, 1), z.to(dev),
                                        1.0 / n, W_INFO / (2.0 * n), dflat, ws, loss_part=part, obs_len=dev_len(ln))
        torch.cuda.synchronize()
    rl, rc, p64, _ = _disc64(Dref, obsv, ln, preds)
    z2 = z.double()[:, :2]
    t0, t1 = (float(torch.tensor(t, dtype=torch.float32)) for t in TARGETS)
    (((rl[0] - t0) ** 2).mean() + ((rl[1] - t1) ** 2).mean() + W_INFO * ((rc[0] - z2) ** 2).mean()).backward()
    group = "ragged.disc_update"
    for k in range(2):
        _close_out(labels[k], rl[k], "label[%d]" % k, group, tag)
        _close_out(codes[k], rc[k], "code[%d]" % k, group, tag)
    got = _grads_of(D, dflat)
    for k, q in Dref.named_parameters():
        _close_grad(got[k], q.grad, "dD/d%s" % k, group, tag, GRAD_REL)
    parts64 = torch.stack([((rl[0] - t0) ** 2).sum(1), ((rc[0] - z2) ** 2).sum(1), ((rl[1] - t1) ** 2).sum(1)], 1).detach()
    for c in range(3):
        _close_out(part[:, c], _tile_sums(parts64[:, c], n), "loss_part column %d" % c, group, tag)


@pytest.mark.parametrize("zdev", [0, 1])
def test_staging_equals_the_dense_staging_and_clamps_obs_len(zdev):
    import socialways_amd as sw
    from socialways_amd import _lib as L
    dev = torch.device("cuda:0")
    n, T = 21, 8
    torch.manual_seed(7)
    G = sw.Generator(use_social=True, device=dev)
    G.unify()
    D = _disc(Tp)
    lib = L.load()
    tab_h = np.empty((D._flat.numel(), 2), dtype=np.int32)
    assert lib.sw_disc_image_table(Tp, tab_h.ctypes.data) == 0
    tab = torch.from_numpy(tab_h).to(dev)
    obsv, pred, _ = crowd([21])
    z = torch.rand(n, 32)
    zd = z.to(dev)
    ln_in = np.array([0, 1, T + 3, 2, T, -5] + [2 + i % (T - 1) for i in range(n - 6)], dtype=np.int32)
    ln = dev_len(ln_in)
    U = 2

    def run(ragged):
        hdr = 12 if ragged else 8
        slot = torch.zeros(hdr + n * 32, dtype=torch.float32).pin_memory()
        hn = slot.numpy()
        hn[:4].view(np.uint64)[:] = (obsv.data_ptr(), pred.data_ptr())
        hn[4], hn[5], hn[6], hn[7] = 0.04, 0.93, 6.0, 3.0
        if zdev:
            hn[8:10].view(np.uint64)[:] = zd.data_ptr()
        else:
            hn[hdr:] = z.numpy().ravel()
        if ragged:
            hn[10:12].view(np.uint64)[:] = ln.data_ptr()
        out = dict(obsv=torch.full((n, T, 2), NAN, device=dev), pred=torch.full((n, Tp, 2), NAN, device=dev),
                   pred4=torch.full((n, Tp, 4), NAN, device=dev), targets=torch.full((4,), NAN, device=dev),
                   z=torch.full((n, 32), NAN, device=dev), steps=torch.full((U + 1,), NAN, device=dev),
                   gimg=torch.zeros(lib.sw_gen_image_floats(), device=dev),      # padding is never written
                   dimg=torch.zeros(lib.sw_disc_image_floats(Tp), device=dev))
        ol = torch.full((n,), -7, dtype=torch.int32, device=dev)
        head = (slot.data_ptr(), n, T, Tp, L.ptr(out["obsv"]), L.ptr(out["pred"]), L.ptr(out["pred4"]), L.ptr(out["targets"]),
                L.ptr(out["z"]), L.ptr(out["steps"]), U, L.ptr(G.encoder._flat), L.ptr(G.decoder._flat),
                L.ptr(G.feature_embedder._flat), L.ptr(G.attention._flat), L.ptr(out["gimg"]), L.ptr(D._flat), L.ptr(out["dimg"]),
                L.ptr(tab), zdev)
        try:
            if ragged:
                L.call("sw_stage_step_ragged", *head, L.ptr(ol), L.stream())
            else:
                L.call("sw_stage_step_zdev", *head, L.stream())
            torch.cuda.synchronize()
        finally:
            L.call("sw_gen_images", None, None, None, None, None, None)
            L.call("sw_disc_images", None, None, None, 0, None)
        out["targets"] = out["targets"][:2]
        return out, ol
    dense, untouched = run(False)
    ragged, ol = run(True)
    assert set(dense) == set(ragged)
    for k in dense:
        assert bits(dense[k], ragged[k]), k
        assert not bool(torch.isnan(ragged[k]).any()), k
    assert torch.equal(ragged["z"], zd) and torch.equal(ragged["obsv"], obsv)
    assert torch.equal(ragged["steps"].cpu(), torch.tensor([7.0, 8.0, 4.0]))
    assert torch.equal(ol.cpu(), torch.from_numpy(np.clip(ln_in, 2, T))) and int(ol[0]) == 2 and int(ol[2]) == T
    assert bool((untouched == -7).all())


def _moments(tr):
    return [tr.D_optimizer.m, tr.D_optimizer.v, tr.predictor_optimizer.m, tr.predictor_optimizer.v]


def _same(a, b, out_a, out_b, what):
    assert torch.equal(out_a, out_b), "%s: the returned sums" % (what,)
    assert torch.equal(a.G._flat_all, b.G._flat_all) and torch.equal(a.D._flat, b.D._flat), "%s: the weights" % (what,)
    for p, q in zip(_moments(a), _moments(b)):
        assert torch.equal(p, q), "%s: the optimizers' moments" % (what,)
    assert (a.D_optimizer.t, a.predictor_optimizer.t) == (b.D_optimizer.t, b.predictor_optimizer.t)


def _ragged_steps(n, T, k, seed):
    """k steps' (lengths, z on the host, label-noise scalars): every step has other lengths and another z."""
    rs = np.random.RandomState(seed)
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i in range(k):
        ln = rs.randint(2, T + 1, size=n).astype(np.int32)
        ln[i], ln[i + 1] = 2, T
        out.append((ln, torch.rand(n, 32, generator=gen), float(rs.uniform(0, 0.1)), float(rs.uniform(0.9, 1.0))))
    return out


@pytest.mark.parametrize("case,kw_fused,kw_both,z_on_device", [
    ("graph", {}, {}, False),
    ("eager", dict(use_graph=False), {}, False),
    ("unrolled_l2", {}, dict(n_unrolling_steps=2, use_l2_loss=True), False),
    ("z_device", {}, {}, True)])
def test_fused_steps_equal_the_eager_ragged_steps_bit_for_bit(case, kw_fused, kw_both, z_on_device):
    import socialways_amd as sw

    def trainer(**kw):
        torch.manual_seed(51)
        return sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0", **kw_both, **kw)
    obsv, gt, sb = crowd(SIZES43)
    n, T = obsv.shape[0], obsv.shape[1]
    assert 37 <= n <= 50
    a, b = trainer(ragged_fused=True, **kw_fused), trainer()
    assert a.ragged_fused and not b.ragged_fused and b.use_graph
    assert torch.equal(_state(a), _state(b))
    w0 = _state(a)
    captured = a.use_graph
    for i, (ln, z, zv, ov) in enumerate(_ragged_steps(n, T, 5, 13)):
        o = padded(obsv, ln, NAN if i == 3 else "repeat")
        zz = z.cuda() if z_on_device else z
        lnd = dev_len(ln) if i % 2 else ln          # a device tensor travels unread, a host array is checked first
        oa = a.step(o, gt, sb, zv, ov, zz, 1.0, obs_len=lnd)
        ob = b.step(o, gt, sb, zv, ov, zz, 1.0, obs_len=lnd)
        torch.cuda.synchronize()
        _same(a, b, oa, ob, "%s, step %d" % (case, i + 1))
        assert bool(torch.isfinite(oa).all()) and bool(torch.isfinite(_state(a)).all())
        assert not b._graphs
        if captured:        # two eager runs, capture on the third, replays from then on: ONE ragged layout
            assert len(a._graphs) == 1 and [(k[-2], k[-1]) for k in a._graphs] == [(True, z_on_device)]     # (ragged, z by address)
            st = next(iter(a._graphs.values()))
            assert (st["graph"] is not None) == (i >= 2) and st["n"] == min(i + 1, 2)
            if i >= 2:
                assert st["flip"] == i % 2 and st["obs_len"].dtype == torch.int32
                assert torch.equal(st["obs_len"].cpu(), torch.from_numpy(ln))
        else:
            assert not a._graphs
    assert float((_state(a) != w0).float().mean()) > 0.5
    # a dense step afterwards: a graph of its own beside the ragged one, and still the dense-only trainer's step
    z = torch.rand(n, 32, generator=torch.Generator().manual_seed(3))
    for i in range(3):
        oa = a.step(obsv, gt, sb, 0.05, 0.95, z, 1.0)
        ob = b.step(obsv, gt, sb, 0.05, 0.95, z, 1.0)
        torch.cuda.synchronize()
        _same(a, b, oa, ob, "%s, dense step %d" % (case, i + 1))
    assert len(b._graphs) == 1 and len(a._graphs) == (2 if captured else 0)
    if captured:
        assert sorted(k[-2] for k in a._graphs) == [False, True] and all(s["graph"] is not None for s in a._graphs.values())


def test_step_many_with_obs_len_equals_the_single_steps():
    import socialways_amd as sw

    def trainer():
        torch.manual_seed(52)
        return sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0", ragged_fused=True)
    obsv, gt, sb = crowd(SIZES43)
    n, T = obsv.shape[0], obsv.shape[1]
    a, b = trainer(), trainer()
    steps = _ragged_steps(n, T, 9, 17)
    for r in range(3):          # the launch of three steps is captured on its third call
        chunk = steps[3 * r:3 * r + 3]
        batches = [(padded(obsv, ln, NAN), gt, zv, ov, z) for ln, z, zv, ov in chunk]
        outs = a.step_many(batches, sb, 1.0, obs_len=[ln for ln, _, _, _ in chunk])
        for j, ((o, g, zv, ov, z), (ln, _, _, _)) in enumerate(zip(batches, chunk)):
            ob = b.step(o, g, sb, zv, ov, z, 1.0, obs_len=ln)
            assert torch.equal(outs[j], ob), (r, j)
        torch.cuda.synchronize()
        _same(a, b, outs[-1], ob, "launch %d" % (r + 1))
    assert len(a._graphs) == 1 and next(iter(a._graphs.values()))["graph"] is not None
    assert [k[5] for k in a._graphs] == [3] and [k[5] for k in b._graphs] == [1]
    # without the switch: K step(obs_len=) calls, no graph
    c = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0")
    outs = c.step_many(batches, sb, 1.0, obs_len=[ln for ln, _, _, _ in chunk])
    assert len(outs) == 3 and not c._graphs and all(bool(torch.isfinite(o).all()) for o in outs)


@pytest.mark.parametrize("device_noise", [False, True])
def test_train_epoch_ragged_fused_equals_the_eager_epochs(ragged_data, device_noise):
    import socialways_amd as sw
    data = ragged_data

    def run(fused):
        torch.manual_seed(61)
        np.random.seed(12)
        tr = sw.SocialWaysTrainer(Tp, use_social=True, device="cuda:0", ragged_fused=fused)
        draws = np.random.RandomState(5)
        gen = torch.Generator().manual_seed(6)

        def draw(bs):
            return float(draws.uniform(0, 0.1)), float(draws.uniform(0.9, 1.0)), torch.rand(bs, 32, generator=gen)
        if device_noise:
            tr.noise = sw.DeviceNoise(77)
        res = [tr.train_epoch_ragged(data, 64, draw=None if device_noise else draw) for _ in range(2)]
        torch.cuda.synchronize()
        return tr, res
    a, ra = run(True)
    b, rb = run(False)
    assert len(a._graphs) > 0 and not b._graphs and a.epoch == b.epoch == 2
    for (ade, fde, losses, sizes), (ade2, fde2, losses2, sizes2) in zip(ra, rb):
        assert (ade, fde, sizes) == (ade2, fde2, sizes2) and np.array_equal(losses, losses2)
        assert np.isfinite(losses).all() and len(sizes) > 2
    assert torch.equal(_state(a), _state(b)) and bool(torch.isfinite(_state(a)).all())
    for p, q in zip(_moments(a), _moments(b)):
        assert torch.equal(p, q)
    if device_noise:
        assert a.noise.step == b.noise.step == 2 * len(ra[0][3])
