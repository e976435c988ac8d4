"""An LSTM forward that starts from the zero state peels its first step and issues only Wx x + b there: W_hh h adds exact
zeros.  Every place that does so is compared bit for bit with a path that keeps the full first step: the encoder with
explicit zero tensors as h0 / c0, the discriminator's scoring launch with the ragged launch at full history length, and the
update pass (gates in registers at To = 8) with both."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _gen_images(G, on):
    import contextlib
    from socialways_amd import _lib as L

    @contextlib.contextmanager
    def cm():
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
    return cm()


@pytest.mark.parametrize("images", (False, True), ids=("weights", "images"))
@pytest.mark.parametrize("x_mode", (0, 1))
@pytest.mark.parametrize("T", (2, 3, 8))
def test_encoder_from_no_state_equals_encoder_from_explicit_zeros(T, x_mode, images):
    """sw_enc_lstm_fwd with h0 = c0 = NULL (first step without recurrent products) against the same call with zero tensors
    (full first step): final state, saved rows and saved inputs.  With weight images and positions in, B <= 4096 runs the
    eight-wave kernel, everything else the four-wave kernel; B = 1, 16, 17, 40: one lane live, a full tile, a tile of
    replicas of the last agent, three tiles."""
    import socialways_amd as sw
    from socialways_amd import _lib as L
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    G = sw.Generator(use_social=True, device=dev)
    G.unify()
    enc = G.encoder._flat
    with _gen_images(G, images):
        for B in (1, 16, 17, 40):
            g = torch.Generator().manual_seed(1000 * T + B)
            x = (torch.rand(B, T, 2 if x_mode == 0 else 4, generator=g).cumsum(1) * 0.1).to(dev).contiguous()
            res = []
            for zeros in (False, True):
                h0 = torch.zeros(B, 64, device=dev) if zeros else None
                c0 = torch.zeros(B, 64, device=dev) if zeros else None
                hT, cT = torch.full((B, 64), float("nan"), device=dev), torch.full((B, 64), float("nan"), device=dev)
                act = torch.full((T, B, 384), float("nan"), device=dev)
                x4s = torch.full((T, B, 4), float("nan"), device=dev)
                L.call("sw_enc_lstm_fwd", L.ptr(x), x_mode, L.ptr(enc), L.ptr(h0), L.ptr(c0), B, T, L.ptr(hT), L.ptr(cT), None,
                       L.ptr(act), L.ptr(x4s), 0, L.stream())
                torch.cuda.synchronize()
                res.append((hT, cT, act, x4s))
            for name, a, b in zip(("hT", "cT", "act", "x4s"), *res):
                assert torch.isfinite(a).all(), (name, B)
                assert torch.equal(a, b), (name, B, float((a - b).abs().max()))


@pytest.mark.parametrize("images", (False, True), ids=("weights", "images"))
@pytest.mark.parametrize("x_mode,T", ((0, 2), (0, 3), (1, 1), (1, 2), (1, 3)))
def test_encoder_output_combinations_equal_the_all_outputs_call(x_mode, T, images):
    """sw_enc_lstm_fwd picks one of 16 instances of enc_lstm_fwd_kernel by x_mode and by which of y / act / x4s are asked
    for.  The other tests reach six of them: nothing saved and act + x4s for both x_modes, and through the module API
    x_mode 1 with y alone and with all three.  Here every combination of outputs runs for both x_modes (with images and
    positions, act + x4s without y is the eight-wave kernel); every requested output, pre-filled with NaN, must be finite and
    equal to the same output of the call that asks for all three.  T = 1 (x_mode 1): only the peeled step runs and the
    prefetch index is clamped to 0.  B = 1, 16, 17, 40: one live lane, a full tile, a tile of replicas, three tiles."""
    import itertools
    import socialways_amd as sw
    from socialways_amd import _lib as L
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    G = sw.Generator(use_social=True, device=dev)
    G.unify()
    enc = G.encoder._flat
    shapes = {"hT": lambda B: (B, 64), "cT": lambda B: (B, 64), "y": lambda B: (B, T, 64), "act": lambda B: (T, B, 384),
              "x4s": lambda B: (T, B, 4)}

    def run(B, x, want):
        out = {k: torch.full(shapes[k](B), float("nan"), device=dev) for k in ("hT", "cT") + want}
        p = lambda k: L.ptr(out[k]) if k in out else None
        L.call("sw_enc_lstm_fwd", L.ptr(x), x_mode, L.ptr(enc), None, None, B, T, p("hT"), p("cT"), p("y"), p("act"), p("x4s"), 0,
               L.stream())
        torch.cuda.synchronize()
        return out

    with _gen_images(G, images):
        for B in (1, 16, 17, 40):
            g = torch.Generator().manual_seed(1000 * T + B)
            x = (torch.rand(B, T, 2 if x_mode == 0 else 4, generator=g).cumsum(1) * 0.1).to(dev).contiguous()
            ref = run(B, x, ("y", "act", "x4s"))
            for k, v in ref.items():
                assert torch.isfinite(v).all(), (k, B)
            for n in range(3):
                for want in itertools.combinations(("y", "act", "x4s"), n):
                    got = run(B, x, want)
                    for k, v in got.items():
                        assert torch.isfinite(v).all(), (want, k, B)
                        assert torch.equal(v, ref[k]), (want, k, B, float((v - ref[k]).abs().max()))


def _disc_setup(B, To, x_cols=2):
    import socialways_amd as sw
    dev = torch.device("cuda:0")
    torch.manual_seed(100 * B + To)
    D = sw.Discriminator(12, 64, 2, device=dev)
    obsv = torch.randn(B, To, x_cols, device=dev).cumsum(1) * 0.1
    return D, obsv, dev


@pytest.mark.parametrize("x_cols", (2, 4), ids=("positions", "states"))
@pytest.mark.parametrize("To", (2, 8))
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("B", (1, 17))
def test_score_equals_ragged_score_at_full_length(B, K, To, x_cols):
    """sw_disc_score (peeled first step) against sw_disc_score_ragged with every history at full length (lanes may start
    at different steps there: it keeps the full products): scores and codes."""
    from socialways_amd import ops
    D, obsv, dev = _disc_setup(B, To, x_cols)
    pred4 = torch.randn(K, B, 12, 4, device=dev) * 0.1
    full = torch.full((B,), To, dtype=torch.int32, device=dev)
    s0, c0 = ops.disc_score(D._flat, obsv, pred4, K)
    s1, c1 = ops.disc_score(D._flat, obsv, pred4, K, obs_len=full)
    torch.cuda.synchronize()
    assert torch.isfinite(s0).all() and torch.isfinite(c0).all()
    assert torch.equal(s0, s1) and torch.equal(c0, c1)


@pytest.mark.parametrize("To", (2, 8))
def test_update_pass_with_and_without_precomputed_rows_and_the_ragged_score(To):
    """sw_disc_update at B = 17 with obs_pre 0 (To = 8: the unrolled loop that keeps the gates in registers, else
    lstm_obs_loop) and obs_pre 1 (rows left by a forward pass) on the same inputs: labels, codes, loss sums, gradients,
    weights and moments after the fused Adam update are equal - and the labels / codes are those of the ragged scoring
    launch at full length, which keeps the recurrent products of the first step."""
    from socialways_amd import _lib as L
    from socialways_amd import ops
    B = 17
    D, obsv, dev = _disc_setup(B, To)
    fake, real = torch.randn(B, 12, 4, device=dev) * 0.1, torch.randn(B, 12, 4, device=dev) * 0.1
    z = torch.rand(B, 32, device=dev)
    targets = torch.tensor([0.05, 0.95], device=dev)
    lib = L.load()
    n = D._flat.numel()
    tab_h = np.empty((n, 2), dtype=np.int32)
    assert lib.sw_disc_image_table(12, tab_h.ctypes.data) == 0
    tab = torch.from_numpy(tab_h).to(dev)
    img = torch.zeros(lib.sw_disc_image_floats(12), device=dev)
    w0 = D._flat.clone()
    full = torch.full((B,), To, dtype=torch.int32, device=dev)
    score, code = ops.disc_score(w0, obsv, torch.stack([fake, real]), 2, obs_len=full)
    res = []
    for obs_pre in (False, True):
        D._flat.copy_(w0)
        ws = ops.Workspaces(dev)
        L.call("sw_disc_images", L.ptr(D._flat), L.ptr(img), L.ptr(tab), 12, L.stream())
        try:
            assert ops.disc_update_supported(D._flat, B, To, 12)
            if obs_pre:
                ops.disc_forward(D._flat, obsv, [fake, real], save=True, ws=ws, save_lstm=1)
            g = torch.zeros_like(D._flat)
            m, v = torch.zeros_like(D._flat), torch.zeros_like(D._flat)
            part = torch.zeros((B + 15) // 16, 3, device=dev)
            adam = (m, v, torch.ones((), device=dev), 1e-3, 0.9, 0.999, 1e-8)
            labels, codes = ops.disc_update(D._flat, obsv, [fake, real], targets, (0, 1), z, 1.0 / B, 0.25 / B, g, ws,
                                            obs_pre=obs_pre, loss_part=part, adam=adam)
            torch.cuda.synchronize()
            res.append([t.clone() for t in labels + codes] + [part, g, D._flat.clone(), m, v])
        finally:
            L.call("sw_disc_images", None, None, None, 0, None)
    names = ["label_fake", "label_real", "code_fake", "code_real", "loss sums", "gradients", "weights", "exp_avg", "exp_avg_sq"]
    for name, a, b in zip(names, res[0], res[1]):
        assert torch.equal(a, b), "%s: max |diff| %.3e" % (name, float((a - b).abs().max()))
    assert float(res[0][5].abs().max()) > 0 and not torch.equal(res[0][6], w0)
    for k in range(2):
        assert torch.equal(res[0][k].reshape(-1), score[k]), "label %d against the ragged score" % k
        assert torch.equal(res[0][2 + k], code[k]), "code %d against the ragged score" % k
