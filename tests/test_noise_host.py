"""The counter-based device noise stream without a GPU: the numpy Philox of tests/_philox.py against the published
known-answer vectors and the layout pin, the statistics of the stream it defines, the argument checks of sw_noise_uniform
(made before any device call) and the DeviceNoise object."""
import numpy as np
import pytest
import torch

import _philox as P


def words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("counter,key,out", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answer_vectors(counter, key, out):
    """Random123's kat_vectors for philox4x32-10."""
    got = P.philox4x32_10(words(counter), words(key))
    assert [int(w) for w in got] == words(out)


def test_stream_layout_pin():
    """Seed 2019, training domain, step 0, draw 0: which counter word is the row, and which output word which column."""
    x = P.uniform(2019, 0, 2, 8)
    assert x.shape == (1, 1, 2, 8) and x.dtype == np.float32
    want0 = np.float32([0.39590013, 0.04927576, 0.6159625, 0.09173757, 0.93431014, 0.6823922, 0.6637776, 0.44013768])
    want1 = np.float32([0.78608245, 0.6699315, 0.22339916, 0.6070749])
    assert np.allclose(x[0, 0, 0], want0, rtol=0, atol=5e-8), x[0, 0, 0]
    assert np.allclose(x[0, 0, 1, :4], want1, rtol=0, atol=5e-8), x[0, 0, 1]
    # every index moves the values, and the two domains are different streams
    base = P.uniform(2019, 0, 3, 8)
    for kw in (dict(step0=1), dict(draw0=1), dict(row0=1)):
        assert not np.array_equal(P.uniform(2019, 0, 3, 8, **kw), base), kw
    assert not np.array_equal(P.uniform(2019, 1, 3, 8), base)
    assert np.array_equal(P.uniform(2019, 0, 3, 8, row0=1)[0, 0, :2], base[0, 0, 1:])
    assert not np.array_equal(P.uniform(1 << 40, 0, 3, 8), P.uniform(0, 0, 3, 8)), "the high seed word is part of the key"
    # padding columns are zero, the values are multiples of 2^-24
    pad = P.uniform(2019, 0, 3, 6, ld=12)
    assert pad.shape[-1] == 12 and not pad[..., 6:].any() and np.array_equal(pad[..., :6], base[..., :6])
    assert np.array_equal(np.float64(base) * 2 ** 24, np.round(np.float64(base) * 2 ** 24))


@pytest.mark.parametrize("domain", [0, 1])
def test_stream_statistics(domain):
    """(20 draws, 64 rows, 32 columns) of seed 2019, N = 40 960: mean, 16-bin chi-square, neighbour correlations, range."""
    x = P.uniform(2019, domain, 64, 32, n_draws=20)[0]
    assert x.shape == (20, 64, 32)
    P.assert_uniform(x, "seed 2019 domain %d" % domain)


def test_argument_checks_without_gpu():
    """Every refusal of sw_noise_uniform comes before any device call: NULL stream, no GPU, an address never touched."""
    from socialways_amd import _lib as L
    lib = L.load()
    EARG, ESHAPE = -1, -2
    good = dict(seed=7, domain=0, step0=0, n_steps=1, draw0=0, n_draws=1, row0=0, rows=4, cols=8, ld=8, out=4096)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sw_noise_uniform(a["seed"], a["domain"], a["step0"], a["n_steps"], a["draw0"], a["n_draws"], a["row0"], a["rows"],
                                    a["cols"], a["ld"], a["out"], None)
    top = (1 << 32) - 1
    for kw in (dict(domain=-1), dict(domain=2), dict(cols=0), dict(cols=-4), dict(cols=1025, ld=1028), dict(ld=4), dict(ld=10),
               dict(cols=6, ld=6), dict(out=None), dict(out=4096 + 4), dict(out=4096 + 8), dict(n_steps=0), dict(n_draws=0),
               dict(rows=0), dict(rows=-1), dict(n_steps=-3), dict(row0=top, rows=2), dict(row0=top - 2, rows=4),
               dict(draw0=top, n_draws=2), dict(step0=top, n_steps=2)):
        assert call(**kw) == EARG, kw
    # 2^31 float4s and more do not fit the kernel's index: refused as a shape, not wrapped
    for kw in (dict(rows=1 << 28, cols=32, ld=32), dict(n_steps=1 << 20, n_draws=1 << 20), dict(n_draws=1 << 30, rows=1 << 30),
               dict(n_steps=1 << 30, n_draws=1 << 30, rows=1 << 30, cols=1024, ld=1024)):
        assert call(**kw) == ESHAPE, kw


def test_device_noise_object():
    import socialways_amd as sw
    dn = sw.DeviceNoise(2019)
    assert dn.state_dict() == {"seed": 2019, "step": 0}
    dn.step = 37
    other = sw.DeviceNoise(1, step=5)
    assert other.state_dict() == {"seed": 1, "step": 5}
    other.load_state_dict(dn.state_dict())
    assert other.state_dict() == dn.state_dict() == {"seed": 2019, "step": 37}
    assert sw.DeviceNoise((1 << 64) + 5).seed == 5 and sw.DeviceNoise(-1).seed == (1 << 64) - 1        # the key is 64 bits
    sd = dn.state_dict()
    sd["step"] = 99
    assert dn.step == 37, "state_dict() is a copy"
    # no host implementation (the rule of test_no_cpu_fallback)
    with pytest.raises(sw.SocialWaysHipError):
        dn.fill(4, 8, domain=0, device="cpu")
    with pytest.raises(sw.SocialWaysHipError):
        dn.fill(4, 8, domain=0, out=torch.empty(4, 8))


def test_checkpoint_without_noise_is_the_reference_dict():
    """checkpoint() gains a 'noise' entry only when a DeviceNoise is set; load_checkpoint restores it when present."""
    import socialways_amd as sw
    torch.manual_seed(0)
    tr = sw.SocialWaysTrainer(12, device="cpu", fused_adam=False)
    assert tr.noise is None
    keys = sorted(tr.checkpoint())
    assert keys == sorted(['epoch', 'attentioner_dict', 'feature_embedder_dict', 'encoder_dict', 'decoder_dict', 'pred_optimizer',
                           'D_dict', 'D_optimizer'])
    tr.noise = sw.DeviceNoise(11, step=6)
    ck = tr.checkpoint()
    assert sorted(ck) == sorted(keys + ["noise"]) and ck["noise"] == {"seed": 11, "step": 6}
    fresh = sw.SocialWaysTrainer(12, device="cpu", fused_adam=False)
    fresh.load_checkpoint(ck)
    assert fresh.noise.state_dict() == {"seed": 11, "step": 6}
    given = sw.SocialWaysTrainer(12, device="cpu", fused_adam=False)
    given.noise = mine = sw.DeviceNoise(3)
    given.load_checkpoint(ck)
    assert given.noise is mine and mine.state_dict() == {"seed": 11, "step": 6}
    del ck["noise"]
    given.load_checkpoint(ck)
    assert mine.state_dict() == {"seed": 11, "step": 6}, "a checkpoint without the entry leaves the stream alone"
    with pytest.raises(TypeError):
        tr.evaluate(None, noise=torch.rand(3, 3))
