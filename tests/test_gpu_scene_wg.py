"""Scene-per-workgroup backward launch (sw_social_enc_bwd, ops.SCENE_WG): the same values in the same places as the
social-backward launch followed by the observation BPTT launch, bit for bit, on NaN-prefilled buffers - dgates rows, pair
rows, agent rows, the social weight gradients, the masked copy; nothing outside the logical shape is written.  Layouts that
do not qualify, and ragged steps, keep the two launches.  At the trainer level: three steps, eager and captured, z on the
host and in device memory, switch on against off."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TP = 12
GUARD = 64      # floats behind every buffer that must stay NaN


@contextlib.contextmanager
def _gen_images(G, on):
    from socialways_amd import _lib as L
    if not on:
        yield
        return
    img = torch.empty(L.load().sw_gen_image_floats(), device="cuda:0")
    L.call("sw_gen_images", L.ptr(G.encoder._flat), L.ptr(G.decoder._flat), L.ptr(G.feature_embedder._flat),
           L.ptr(G.attention._flat), L.ptr(img), L.stream())
    try:
        yield
    finally:
        torch.cuda.synchronize()
        L.call("sw_gen_images", None, None, None, None, None, None)


@contextlib.contextmanager
def _kernel_names():
    """Names of the kernels launched inside the block (sw_kernel_timing)."""
    from socialways_amd import _lib as L
    lib = L.load()
    names = set()
    lib.sw_kernel_timing(1)
    try:
        yield names
    finally:
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        lib.sw_kernel_timing_read(buf, len(buf))
        lib.sw_kernel_timing(0)
        names.update(line.split()[0] for line in buf.value.decode().splitlines() if line.strip())


def _sub_batches(sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return np.stack([off[:-1], off[1:]], 1)


def _nan(n, dev):
    return torch.full((n + GUARD,), float("nan"), device=dev)


def _bits(t):
    return t.view(torch.int32)


def _forward(G, obsv, scenes):
    """Encoder and social-pool launches: what the backward reads (h_T, attention rows, saved rows)."""
    from socialways_amd import _lib as L
    dev = obsv.device
    B, To = obsv.shape[0], obsv.shape[1]
    enc, emb, att = G.encoder._flat, G.feature_embedder._flat, G.attention._flat
    r = {"hT": _nan(B * 64, dev), "cT": _nan(B * 64, dev), "act": _nan(To * B * 384, dev), "x4s": _nan(To * B * 4, dev),
         "S_pool": _nan(B * 64, dev), "attn": _nan(B * L.AMAX, dev)}
    st = L.stream()
    L.call("sw_enc_lstm_fwd_aux", L.ptr(obsv), 0, L.ptr(enc), None, None, B, To, L.ptr(r["hT"]), L.ptr(r["cT"]), None,
           L.ptr(r["act"]), L.ptr(r["x4s"]), 0, None, None, 0, st)
    L.call("sw_social_pool_fwd_aux", L.ptr(obsv), To, L.ptr(r["hT"]), L.ptr(scenes.scene_off), scenes.S, B, scenes.amax,
           L.ptr(emb), L.ptr(att), L.ptr(r["S_pool"]), L.ptr(r["attn"]), None, 0, None, None, None, None, 0, st)
    torch.cuda.synchronize()
    return r


# the issue's lists, and 250 two-agent scenes: with the 8 copy workgroups of the masked copy below they exceed the CUs, so the
# scene workgroups copy (every smaller list gets copy workgroups of its own)
SIZES = ([8, 8], [1], [16], [1, 16, 2], [3, 5, 7, 1, 1, 16], [2] * 40, [2] * 250)


def _backward(G, obsv, scenes, fwd, grads, aux, fused):
    """Social backward + observation BPTT as two launches or as the one, on fresh NaN buffers."""
    from socialways_amd import _lib as L
    dev = obsv.device
    B, To = obsv.shape[0], obsv.shape[1]
    enc, emb, att = G.encoder._flat, G.feature_embedder._flat, G.attention._flat
    dS, dhT, dcT = grads
    src, mask = aux
    n_pairs = L.workspace_floats(L.WS_PAIRS, B, To, TP, 1, scenes.P)
    r = {"dgates": _nan(To * B * 256, dev), "pairs": _nan(n_pairs, dev), "d_emb": _nan(emb.numel(), dev),
         "d_att": _nan(att.numel(), dev), "aux": torch.arange(src.numel() + GUARD, device=dev, dtype=torch.float32)}
    r["aux"][-GUARD:] = float("nan")
    wgrad = torch.empty(L.workspace_floats(L.WS_WGRAD, B, To, TP), device=dev)
    dh = dhT.clone()
    hT, attn, act = fwd["hT"], fwd["attn"], fwd["act"]
    st = L.stream()
    if fused:
        L.call("sw_social_enc_bwd", L.ptr(obsv), To, L.ptr(hT), L.ptr(scenes.scene_off), L.ptr(scenes.pair_off), scenes.S, B,
               scenes.amax, scenes.P, L.ptr(emb), L.ptr(att), L.ptr(attn), L.ptr(dS), L.ptr(dh), L.ptr(dcT), L.ptr(r["d_emb"]),
               L.ptr(r["d_att"]), L.ptr(r["pairs"]), L.ptr(wgrad), L.ptr(enc), L.ptr(act), L.ptr(r["dgates"]), L.ptr(src),
               L.ptr(r["aux"]), L.ptr(mask), src.numel(), None, st)
        torch.cuda.synchronize()
        assert torch.equal(dh, dhT), "dh_T is read, not updated"
    else:
        L.call("sw_social_pool_bwd", L.ptr(obsv), To, L.ptr(hT), L.ptr(scenes.scene_off), L.ptr(scenes.pair_off), scenes.S, B,
               scenes.amax, scenes.P, L.ptr(emb), L.ptr(att), L.ptr(attn), L.ptr(dS), L.ptr(dh), L.ptr(r["d_emb"]),
               L.ptr(r["d_att"]), L.ptr(r["pairs"]), L.ptr(wgrad), None, 0, None, None, None, None, None, st)
        L.call("sw_enc_lstm_bwd_aux", L.ptr(enc), L.ptr(act), None, L.ptr(dh), L.ptr(dcT), None, B, To, 0, L.ptr(r["dgates"]),
               None, None, L.ptr(src), L.ptr(r["aux"]), L.ptr(mask), src.numel(), st)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("images", (False, True), ids=("weights", "images"))
@pytest.mark.parametrize("To", (2, 8))
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)) if len(s) < 8 else "%dx%d" % (s[0], len(s)))
def test_backward_equals_the_two_launches(sizes, To, images):
    """dgates rows, pair rows, agent rows (dWh, Wh, Q, sd), the social weight gradients and the masked copy.  [1] has no
    pair and [16] alone runs the in-register social backward: neither takes the fused launch."""
    import socialways_amd as sw
    from socialways_amd import _lib as L
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(14)
    G = sw.Generator(use_social=True, device=dev)
    G.unify()
    B = int(np.sum(sizes))
    g = torch.Generator().manual_seed(200 * B + To)
    obsv = (torch.rand(B, To, 2, generator=g).cumsum(1) * 0.3 + torch.rand(B, 1, 2, generator=g) * 4).to(dev).contiguous()
    scenes = ops.SceneIndex(_sub_batches(sizes), B, dev)
    if sizes in ([1], [16]):
        assert not ops.scene_wg(scenes, True)
        z = torch.zeros(4096, device=dev)
        rc = L.load().sw_social_enc_bwd(*([z.data_ptr(), To] + [z.data_ptr()] * 3 + [scenes.S, B, scenes.amax, scenes.P]
                                          + [z.data_ptr()] * 13 + [None, None, None, 0, None, None]))
        assert rc == -2
        return
    assert ops.scene_wg(scenes, True)
    grads = [(torch.randn(B, 64, generator=g) * 0.1).to(dev) for _ in range(3)]
    n_aux = 2000
    aux = ((torch.rand(n_aux, generator=g) + 1.0).to(dev), (torch.rand(n_aux, generator=g) - 0.5).to(dev))
    with _gen_images(G, images):
        fwd = _forward(G, obsv, scenes)
        want = _backward(G, obsv, scenes, fwd, grads, aux, fused=False)
        got = _backward(G, obsv, scenes, fwd, grads, aux, fused=True)
    for name in want:
        assert torch.equal(_bits(got[name]), _bits(want[name])), \
            "%s: %d floats differ" % (name, int((_bits(got[name]) != _bits(want[name])).sum()))
        assert torch.isnan(got[name][-GUARD:]).all(), name
    for name in ("dgates", "d_emb", "d_att"):
        assert torch.isfinite(got[name][:-GUARD]).all(), name
    assert float(got["dgates"][:-GUARD].abs().max()) > 0
    copied = got["aux"][:n_aux] != torch.arange(n_aux, device=dev)
    assert torch.equal(copied, aux[1] > 0), "the masked copy"


def _tracks(sizes, seed):
    B = int(np.sum(sizes))
    g = torch.Generator().manual_seed(seed)
    track = torch.rand(B, 8 + TP, 2, generator=g).cumsum(1) * 0.3 + torch.rand(B, 1, 2, generator=g) * 4
    return B, track[:, :8].contiguous().to("cuda:0"), track[:, 8:].contiguous().to("cuda:0"), g


@pytest.mark.parametrize("sizes", ([17], [1] * 257, [8] * 257), ids=("17", "1x257", "8x257"))
def test_layouts_that_do_not_qualify_keep_the_two_launches(sizes):
    """A scene above 16 agents, more than 256 scenes: gen_backward runs the existing launches whatever ops.SCENE_WG says, the
    entry point itself refuses the layout, and the results are those of the switch off."""
    import socialways_amd as sw
    from socialways_amd import _lib as L
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(12)
    G = sw.Generator(use_social=True, device=dev)
    G.unify()
    B, obsv, _, g = _tracks(sizes, int(np.sum(sizes)))
    noise = torch.rand(B, 32, generator=g).to(dev)
    scenes = ops.SceneIndex(_sub_batches(sizes), B, dev)
    assert not ops.scene_wg(scenes, True)
    z = torch.zeros(4096, device=dev)
    rc = L.load().sw_social_enc_bwd(*([z.data_ptr(), 8] + [z.data_ptr()] * 3 + [scenes.S, B, scenes.amax, max(scenes.P, 1)]
                                      + [z.data_ptr()] * 13 + [None, None, None, 0, None, None]))
    assert rc == -2, "SW_ESHAPE before anything is launched"
    args = (G.encoder._flat, G.feature_embedder._flat, G.attention._flat, G.decoder._flat)
    res = []
    for on in (True, False):
        old, ops.SCENE_WG = ops.SCENE_WG, on
        try:
            pred4, ctx = ops.gen_forward(*args, obsv, noise, scenes, TP, True, save=True, ws=ops.Workspaces(dev))
            d = [torch.zeros_like(w) for w in args]
            with _kernel_names() as names:
                ops.gen_backward(*args, ctx, torch.ones_like(pred4) * 0.01, *d, ws=ops.Workspaces(dev))
        finally:
            ops.SCENE_WG = old
        assert "enc_lstm_bwd_kernel" in names, names
        assert scenes.P == 0 or names & {"social_pool_bwd_rows_kernel", "social_pool_bwd_kernel"}, names
        res.append([pred4] + d)
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_a_qualifying_step_drops_the_social_backward_launch_and_a_ragged_step_keeps_it():
    """One eager trainer step on 8-agent scenes: dense, the social backward rides in the BPTT launch; with obs_len (ragged
    histories) both launches run, whatever the switch says."""
    import socialways_amd as sw
    sizes = [8] * 4
    B, obsv, pred, g = _tracks(sizes, 31)
    sb = _sub_batches(sizes)
    torch.manual_seed(0)
    tr = sw.SocialWaysTrainer(TP, use_social=True, device="cuda:0", use_graph=False)
    obs_len = torch.randint(2, 9, (B,), generator=g)
    for ol in (None, obs_len):
        z = torch.rand(B, 32, generator=g)
        tr.step(obsv, pred, sb, 0.02, 0.9, z, 1.0, obs_len=ol)           # warm-up of this form
        with _kernel_names() as names:
            out = tr.step(obsv, pred, sb, 0.02, 0.9, z, 1.0, obs_len=ol)
        assert torch.isfinite(out).all()
        assert "enc_lstm_bwd_kernel" in names, names
        assert ("social_pool_bwd_rows_kernel" in names) is (ol is not None), names


@pytest.mark.parametrize("z_on", ("host", "device"))
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "captured"))
@pytest.mark.parametrize("sizes", ([8] * 4, [1, 16, 2, 8]), ids=("8x4", "1x16x2x8"))
def test_three_trainer_steps_switch_on_against_off(sizes, graph, z_on):
    """Weights, Adam state, loss sums and ADE/FDE sums after three steps, bit for bit."""
    import socialways_amd as sw
    from socialways_amd import ops
    dev = torch.device("cuda:0")
    B, sb = int(np.sum(sizes)), _sub_batches(sizes)
    g = torch.Generator().manual_seed(21)
    track = torch.rand(B, 8 + TP, 2, generator=g).cumsum(1) * 0.3 + torch.rand(B, 1, 2, generator=g) * 4
    obsv, pred = track[:, :8].contiguous().to(dev), track[:, 8:].contiguous().to(dev)
    res = []
    for on in (True, False):
        old, ops.SCENE_WG = ops.SCENE_WG, on
        try:
            torch.manual_seed(0)
            tr = sw.SocialWaysTrainer(TP, use_social=True, device="cuda:0", use_graph=graph)
            gen = torch.Generator().manual_seed(5)
            outs = [tr.step(obsv, pred, sb, 0.01 * i, 0.9, torch.rand(B, 32, generator=gen).to(dev if z_on == "device" else "cpu"), 1.0).clone()
                    for i in range(3)]
            torch.cuda.synchronize()
            res.append(outs + [tr.D._flat.clone(), tr.D_optimizer.m.clone(), tr.D_optimizer.v.clone(), tr.G._flat_all.clone(),
                               tr.predictor_optimizer.m.clone(), tr.predictor_optimizer.v.clone()])
            tr.release_graphs()
        finally:
            ops.SCENE_WG = old
    names = ["step %d sums" % i for i in range(3)] + ["D weights", "D exp_avg", "D exp_avg_sq", "G weights", "G exp_avg",
                                                      "G exp_avg_sq"]
    for name, a, b in zip(names, *res):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), "%s: max |diff| %.3e" % (name, float((a - b).abs().max()))
    assert float(res[0][7].abs().max()) > 0, "the generator's moments moved"
