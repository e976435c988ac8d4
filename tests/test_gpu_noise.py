"""The counter-based device noise stream on the GPU: sw_noise_uniform against the numpy Philox of tests/_philox.py bit for
bit, and DeviceNoise through Generator.sample(), evaluate*(), train_epoch() and the checkpoint."""
import copy

import numpy as np
import pytest
import torch

import _philox as P
from _util import golden, state_from, as_checkpoint, dataset_from

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 17, 8, 3, 70, 1, 12]       # the ragged scenes of tests/test_gpu_sample.py: 117 agents
BIG_SEED = 0x9E3779B97F4A7C15


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- the kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,ld", [(1, 1, 4), (5, 6, 8), (17, 12, 32), (70, 32, 32), (3, 33, 36), (2, 1024, 1024)])
def test_kernel_equals_the_numpy_philox(rows, cols, ld):
    """Every shape with both domains, n_steps and n_draws in {1, 3}, non-zero row0 / draw0 / step0: the block, its zero
    padding and a sentinel-filled tail behind it."""
    import socialways_amd as sw
    for seed, domain, n_steps, n_draws, row0, draw0, step0 in ((2019, 0, 1, 1, 0, 0, 0), (BIG_SEED, 1, 3, 3, 1000003, 7, 123456),
                                                               (5, 0, 3, 1, 11, 0, 4000000000), (5, 1, 1, 3, 0, 4000000000, 9)):
        dn = sw.DeviceNoise(seed)
        n = n_steps * n_draws * rows * ld
        buf = torch.full((n + 64,), -7.0, device="cuda")
        got = dn.fill(rows, cols, domain=domain, step=step0, n_steps=n_steps, draw0=draw0, n_draws=n_draws, row0=row0, ld=ld,
                      out=buf[:n])
        want = P.uniform(seed, domain, rows, cols, step0, n_steps, draw0, n_draws, row0, ld)
        assert got.shape == want.shape == (n_steps, n_draws, rows, ld) and got.data_ptr() == buf.data_ptr()
        assert torch.equal(got, dev(want)), (seed, domain, n_steps, n_draws)
        assert not got[..., cols:].any(), "padding columns are exactly 0"
        assert float(got[..., :cols].max()) > 0.0
        assert torch.equal(buf[n:], torch.full((64,), -7.0, device="cuda")), "nothing is written past the block"
        fresh = dn.fill(rows, cols, domain=domain, step=step0, n_steps=n_steps, draw0=draw0, n_draws=n_draws, row0=row0, ld=ld)
        assert torch.equal(fresh, got) and fresh.data_ptr() != got.data_ptr()


def test_kernel_index_edges_and_seed_words():
    import socialways_amd as sw
    top = (1 << 32) - 3
    got = sw.DeviceNoise(2019).fill(3, 32, domain=0, row0=top)
    assert torch.equal(got, dev(P.uniform(2019, 0, 3, 32, row0=top)))
    hi, zero = sw.DeviceNoise(1 << 40).fill(5, 8, domain=1), sw.DeviceNoise(0).fill(5, 8, domain=1)
    assert torch.equal(hi, dev(P.uniform(1 << 40, 1, 5, 8))) and torch.equal(zero, dev(P.uniform(0, 1, 5, 8)))
    assert not torch.equal(hi, zero), "the high seed word is part of the key"
    # more than one workgroup, and a row count that is no multiple of anything
    big = sw.DeviceNoise(BIG_SEED).fill(1237, 32, domain=0, step=3, n_draws=2)
    assert torch.equal(big, dev(P.uniform(BIG_SEED, 0, 1237, 32, step0=3, n_draws=2)))
    # the default ld is cols rounded up to 4; the argument checks of the C ABI reach Python as errors
    assert sw.DeviceNoise(1).fill(2, 6, domain=0).shape == (1, 1, 2, 8)
    for kw in (dict(domain=2), dict(ld=6), dict(row0=(1 << 32) - 1), dict(n_draws=0)):
        with pytest.raises(sw.SocialWaysHipError):
            sw.DeviceNoise(1).fill(2, 6, **dict(dict(domain=0), **kw))


def test_kernel_tiling_is_invisible():
    """One call, row by row, draw by draw and step by step: the same block."""
    import socialways_amd as sw
    dn = sw.DeviceNoise(77)
    kw = dict(domain=1, step=5, draw0=2, row0=9, ld=16)
    S, K, R, C = 3, 4, 19, 14
    whole = dn.fill(R, C, n_steps=S, n_draws=K, **kw)
    rows = torch.cat([dn.fill(1, C, n_steps=S, n_draws=K, **dict(kw, row0=9 + i)) for i in range(R)], dim=2)
    draws = torch.cat([dn.fill(R, C, n_steps=S, n_draws=1, **dict(kw, draw0=2 + k)) for k in range(K)], dim=1)
    steps = torch.cat([dn.fill(R, C, n_steps=1, n_draws=K, **dict(kw, step=5 + t)) for t in range(S)], dim=0)
    assert torch.equal(rows, whole) and torch.equal(draws, whole) and torch.equal(steps, whole)


@pytest.mark.parametrize("domain", [0, 1])
def test_kernel_output_statistics(domain):
    """The conditions of tests/test_noise_host.py on what the kernel wrote (which equals that stream bit for bit)."""
    import socialways_amd as sw
    x = sw.DeviceNoise(2019).fill(64, 32, domain=domain, n_draws=20)[0]
    assert torch.equal(x, dev(P.uniform(2019, domain, 64, 32, n_draws=20)[0]))
    P.assert_uniform(x.cpu().numpy(), "kernel, seed 2019 domain %d" % domain)


def test_fill_is_capturable():
    """No host sync, no allocation: the launch records into a graph and replays."""
    import socialways_amd as sw
    dn = sw.DeviceNoise(3)
    out = torch.zeros(2, 1, 10, 32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dn.fill(10, 32, domain=0, step=4, n_steps=2, out=out)
    torch.cuda.current_stream().wait_stream(s)
    want = out.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dn.fill(10, 32, domain=0, step=4, n_steps=2, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(want, dev(P.uniform(3, 0, 10, 32, step0=4, n_steps=2)))


# ---- sampling ----------------------------------------------------------------------------------------------------------
def crowd(sizes, To=8, seed=3):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    B = int(np.sum(sizes))
    obsv = (torch.rand(B, To, 2, device="cuda", generator=gen) * 0.1 - 0.03).cumsum(1).contiguous()
    ends = np.cumsum(sizes)
    return obsv, np.stack([ends - np.asarray(sizes), ends], axis=1).astype(np.int64)


@pytest.mark.parametrize("hidden", [64, 24])
@pytest.mark.parametrize("social", [False, True])
def test_sample_with_device_noise_equals_sample_with_its_tensor(social, hidden):
    import socialways_amd as sw
    torch.manual_seed(0)
    G = sw.Generator(hidden, 1, use_social=social, device="cuda:0")
    obsv, sb = crowd(SIZES)
    B, Tp, nl = obsv.shape[0], 12, hidden // 2
    assert B == 117 and G.noise_len == nl
    for K in (1, 3, 20):
        dn = sw.DeviceNoise(7)
        z = dn.fill(B, nl, domain=1, n_draws=K)[0]
        assert z.shape == (K, B, nl) and torch.equal(z, dev(P.uniform(7, 1, B, nl, n_draws=K)[0]))
        got = G.sample(obsv, K, Tp, sb, noise=dn)
        assert got.shape == (K, B, Tp, 4) and float(got.abs().max()) > 0.0
        assert torch.equal(got, G.sample(obsv, K, Tp, sb, noise=z)), K
        assert torch.equal(got, sw.sample(obsv, K, Tp, sb, noise=sw.DeviceNoise(7), generator=G))
    # rows are absolute: the last scene alone, told where it starts, gets the futures it had in the batch (no social
    # block: with one, too - a scene does not see its neighbours - but the bits of the pooled state may depend on the tiling)
    a, b = int(sb[-1, 0]), int(sb[-1, 1])
    if not social:
        part = G.sample(obsv[a:b], 20, Tp, [], noise=sw.DeviceNoise(7), row0=a)
        assert torch.equal(part, got[:, a:b])
    assert not torch.equal(G.sample(obsv[a:b], 20, Tp, [], noise=sw.DeviceNoise(7)), got[:, a:b])
    with pytest.raises(ValueError):
        G.sample(obsv, 0, Tp, sb, noise=sw.DeviceNoise(7))


def test_sample_ranked_takes_a_device_noise():
    import socialways_amd as sw
    torch.manual_seed(0)
    tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0")
    obsv, sb = crowd(SIZES)
    K, M, B = 6, 2, obsv.shape[0]
    a = tr.sample_ranked(obsv, K, M, sb, noise=sw.DeviceNoise(7))
    b = tr.sample_ranked(obsv, K, M, sb, noise=sw.DeviceNoise(7).fill(B, 32, domain=1, n_draws=K)[0])
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].shape == (M, B, 12, 4)


# ---- evaluation --------------------------------------------------------------------------------------------------------
def eval_golden():
    import socialways_amd as sw
    g = golden("test_eval")
    ds = dataset_from(g)
    data = sw.SceneDataset(ds["obsvs"], ds["preds"], ds["batches"], g["ds.times"], device="cuda:0")
    tr = sw.SocialWaysTrainer(12, use_social=True, device="cuda:0")
    tr.load_checkpoint(as_checkpoint(state_from(g, "w0.")))
    return data, tr


def same_records(ca, cb):
    assert len(ca) == len(cb) > 0
    for ra, rb in zip(ca, cb):
        assert ra["timestamp"] == rb["timestamp"]
        for k in ("obsvs", "preds_our", "preds_gtt", "preds_lnr"):
            assert np.array_equal(ra[k], rb[k]), k


def test_evaluate_with_device_noise():
    import socialways_amd as sw
    data, tr = eval_golden()
    K = 20
    batches = [(int(a), int(b)) for a, b in data.test_batches]
    assert len(batches) > 1
    dn = sw.DeviceNoise(2019)
    rng = torch.get_rng_state()
    host_stream = tr.eval_noise

    def no_host_noise(*a):
        raise AssertionError("eval_noise() called on the device-noise path")
    tr.eval_noise = no_host_noise
    c0 = []
    want = tr.evaluate(data, n_gen_samples=K, collect=c0, noise=dn)
    assert tr.evaluate(data, n_gen_samples=K, noise=dn) == want, "two calls, the same numbers"
    assert tr.evaluate(data, n_gen_samples=K, noise=sw.DeviceNoise(2019)) == want
    assert tr.evaluate(data, n_gen_samples=K, noise=sw.DeviceNoise(2020)) != want
    assert torch.equal(torch.get_rng_state(), rng), "the host generator is not consumed"
    assert len(want) == 4 and all(np.isfinite(want)) and want[2] < want[0] and want[3] < want[1]
    # the folding of scenes into launches does not change a scene's draws; the float64 sums regroup
    largest = max(b - a for a, b in batches)
    for chunk in (64, K * largest):
        tr.TEST_CHUNK = chunk
        assert len(list(tr.eval_chunks(batches, K, chunk))) > 1
        cc = []
        got = tr.evaluate(data, n_gen_samples=K, collect=cc, noise=dn)
        same_records(c0, cc)
        assert np.allclose(got, want, rtol=1e-12, atol=0.0), (chunk, got, want)
    del tr.TEST_CHUNK
    # just_one: the first scene's draws are those it has in the full run
    c1 = []
    tr.evaluate(data, n_gen_samples=K, just_one=True, collect=c1, noise=dn)
    same_records(c0[:1], c1)
    # the scene and ranking forms return evaluate()'s four numbers bit for bit
    # (evaluate_scenes' argument list is pinned by tests/test_scene_host.py: it takes the stream from trainer.noise only)
    rk = tr.evaluate_ranked(data, n_gen_samples=K, top_m=5, noise=dn)
    keys = ("ade_avg", "fde_avg", "ade_min", "fde_min")
    assert tuple(rk[k] for k in keys) == want and tr.evaluate_ranked(data, n_gen_samples=K, noise=dn) == rk
    # ... and so does the diverse form, per agent and per scene; at radius 0 its picks are the ranking's
    for joint in (False, True):
        dv = tr.evaluate_diverse(data, n_gen_samples=K, top_m=5, radius=0.5, joint=joint, noise=dn)
        assert tuple(dv[k] for k in keys) == want
        assert tr.evaluate_diverse(data, n_gen_samples=K, top_m=5, radius=0.5, joint=joint, noise=dn) == dv
    d0 = tr.evaluate_diverse(data, n_gen_samples=K, top_m=5, radius=0.0, joint=False, noise=dn)
    for kd, kr in (("ade_div1", "ade_top1"), ("fde_div1", "fde_top1"), ("ade_divm", "ade_topm"), ("fde_divm", "fde_topm")):
        assert d0[kd] == rk[kr], (kd, d0[kd], rk[kr])
    assert torch.equal(torch.get_rng_state(), rng), "the host generator is not consumed"
    # trainer.noise is the default of the keyword
    tr.noise = dn
    sc = tr.evaluate_scenes(data, n_gen_samples=K)
    assert tuple(sc[k] for k in keys) == want and tr.evaluate_scenes(data, n_gen_samples=K) == sc
    assert tr.evaluate(data, n_gen_samples=K) == want and tr.evaluate_ranked(data, n_gen_samples=K, top_m=5) == rk
    tr.noise = None
    # the host-noise code path fed the same values (its own padding and copy, chunk by chunk) gives the same metrics
    calls = []

    def stream_values(chunk, K_, noise_len):
        lo, hi = chunk[0][0], chunk[-1][1]
        calls.append((lo, hi))
        return dn.fill(hi - lo, noise_len, domain=1, n_draws=K_, row0=lo)[0].cpu()
    tr.eval_noise = stream_values
    ch = []
    assert tr.evaluate(data, n_gen_samples=K, collect=ch) == want and len(calls) == 1
    same_records(c0, ch)
    # without a DeviceNoise evaluate() is still test() on the reference's host stream
    tr.eval_noise = host_stream
    torch.manual_seed(31)
    ref = tr.test(data, n_gen_samples=4)
    torch.manual_seed(31)
    assert tr.noise is None and np.allclose(tr.evaluate(data, n_gen_samples=4), ref, rtol=2e-5, atol=2e-6)
    assert not torch.equal(torch.get_rng_state(), rng)


# ---- training ----------------------------------------------------------------------------------------------------------
def toy_data():
    import socialways_amd as sw
    toy = golden("toy_768_8_3")
    return sw.SceneDataset(toy["obsvs"], toy["preds"], toy["batches"], toy["times"], device="cuda:0")


def twin_draw(seed, noise_len, variety_k=0):
    """The draws of train_epoch() with DeviceNoise(seed), made by hand for the `draw` callback: the reference's two label
    scalars from numpy's generator, z (and the extra samples' z) from fill() - through the HOST, so the twin takes the
    pinned-slot path."""
    import socialways_amd as sw
    dn, step = sw.DeviceNoise(seed), [0]

    def draw(bs):
        zv, ov = np.random.uniform(0, 0.1), np.random.uniform(0.9, 1.0)
        s = step[0]
        step[0] += 1
        z = dn.fill(bs, noise_len, domain=0, step=s)[0, 0].cpu()
        if variety_k:
            return zv, ov, z, dn.fill(bs, noise_len, domain=0, step=s, draw0=1, n_draws=variety_k - 1)[0].cpu()
        return zv, ov, z
    return draw, step


def weights(tr):
    torch.cuda.synchronize()
    return tr.G._flat_all.clone(), tr.D._flat.clone()


def test_train_epoch_with_device_noise_equals_a_draw_fed_twin():
    """Four toy epochs of 10 packed batches of 64 (eager steps, capture, replay; launches of 4, 3, 2 and 1 steps): losses and
    weights bit for bit - z by address from one fill launch per graph launch against z through the pinned slot, which
    tests/test_gpu_trainer.py shows to be bit-identical paths."""
    import socialways_amd as sw
    data = toy_data()
    n_batches = len(list(data.packed_steps(64)))
    assert n_batches == 10
    res = []
    for device_noise in (True, False):
        torch.manual_seed(5)
        tr = sw.SocialWaysTrainer(2, use_social=True, device="cuda:0")
        np.random.seed(1)
        draw, step = (None, None) if device_noise else twin_draw(5, tr.noise_len)
        if device_noise:
            tr.noise = sw.DeviceNoise(5)
        eps = [tr.train_epoch(data, 64, draw=draw) for _ in range(4)]
        if device_noise:
            assert tr.noise.step == 4 * n_batches, "one step per packed batch"
            assert len(tr._graphs) > 0 and any(st["graph"] is not None for st in tr._graphs.values()), "the graph path is taken"
            assert all(k[-1] is True for k in tr._graphs), "every captured layout reads z by address"
        else:
            assert step[0] == 4 * n_batches and not any(k[-1] for k in tr._graphs)
        res.append((eps, weights(tr)))
        tr.release_graphs()
    for (a0, f0, l0, s0), (a1, f1, l1, s1) in zip(res[0][0], res[1][0]):
        assert a0 == a1 and f0 == f1 and s0 == s1 and np.array_equal(l0, l1)
    assert torch.equal(res[0][1][0], res[1][1][0]) and torch.equal(res[0][1][1], res[1][1][1])
    assert np.isfinite(res[0][0][-1][2]).all()


def test_checkpoint_continues_the_stream():
    import socialways_amd as sw
    data = toy_data()
    torch.manual_seed(5)
    tr = sw.SocialWaysTrainer(2, use_social=True, device="cuda:0")
    tr.noise = sw.DeviceNoise(5)
    np.random.seed(1)
    tr.train_epoch(data, 64)
    ck = tr.checkpoint()
    assert ck["noise"] == {"seed": 5, "step": 10}
    ck = copy.deepcopy(ck)                # state_dict() tensors are views of the live packed buffers
    np.random.seed(2)
    want = tr.train_epoch(data, 64)
    w_want = weights(tr)
    tr.release_graphs()
    torch.manual_seed(99)
    fresh = sw.SocialWaysTrainer(2, use_social=True, device="cuda:0")
    assert fresh.noise is None
    fresh.load_checkpoint(ck)
    assert fresh.noise.state_dict() == {"seed": 5, "step": 10}
    np.random.seed(2)
    got = fresh.train_epoch(data, 64)
    assert fresh.noise.step == 20
    assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2])
    w_got = weights(fresh)
    assert torch.equal(w_got[0], w_want[0]) and torch.equal(w_got[1], w_want[1])
    fresh.release_graphs()


def test_variety_fixed_consumes_draws_1_to_k():
    import socialways_amd as sw
    data = toy_data()
    K = 3
    res = []
    for device_noise in (True, False):
        torch.manual_seed(5)
        tr = sw.SocialWaysTrainer(2, use_social=True, device="cuda:0", use_variety_loss="fixed", variety_k=K, use_l2_loss=True)
        np.random.seed(1)
        draw = None if device_noise else twin_draw(5, tr.noise_len, K)[0]
        if device_noise:
            tr.noise = sw.DeviceNoise(5)
        ep = tr.train_epoch(data, 64, draw=draw)
        l2min, kmin = tr.last_variety
        res.append((ep, l2min.clone(), kmin.clone(), weights(tr)))
        if device_noise:
            assert tr.noise.step == 10
    a, b = res
    assert a[0][0] == b[0][0] and np.array_equal(a[0][2], b[0][2])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and len(a[2].unique()) > 1, "every draw wins somewhere"
    assert torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1])


def test_shard_rule_in_a_single_process():
    """What a rank of a data-parallel job fills - rows [r0, r1) of the packed batch from row0 = r0 - is that slice of the
    single-process z, for the shards shard_scenes() gives at world 2 and 3 (verified in one process only)."""
    import socialways_amd as sw
    data = toy_data()
    dn = sw.DeviceNoise(5)
    seen = 0
    for step, (a, b, sb) in enumerate(data.packed_steps(64)):
        whole = dn.fill(b - a, 32, domain=0, step=step, n_draws=3)
        for world in (2, 3):
            cover = []
            for lo, hi in sw.shard_scenes(sb, world):
                if hi <= lo:
                    continue
                r0, r1 = int(sb[lo, 0]), int(sb[hi - 1, 1])
                assert torch.equal(dn.fill(r1 - r0, 32, domain=0, step=step, n_draws=3, row0=r0), whole[:, :, r0:r1])
                cover += list(range(r0, r1))
                seen += r0 > 0
            assert cover == list(range(b - a)), "the union over ranks is the single-process z"
    assert seen > 0


def test_wide_and_generic_trainers_refuse_a_device_noise():
    import socialways_amd as sw
    from socialways_amd.generic import GenericTrainer
    from socialways_amd.wide import WideTrainer
    obsv, sb = crowd([3, 2])
    for cls in (WideTrainer, GenericTrainer):
        torch.manual_seed(0)
        tr = cls(12, hidden_size=128, device="cuda:0")
        assert type(tr) is cls and tr.noise is None
        tr.noise = None
        with pytest.raises(sw.SocialWaysHipError, match="DeviceNoise"):
            tr.noise = sw.DeviceNoise(1)
        assert tr.noise is None
        for call in (tr.evaluate, tr.evaluate_ranked):
            with pytest.raises(sw.SocialWaysHipError, match="DeviceNoise"):
                call(None, noise=sw.DeviceNoise(1))
        with pytest.raises(sw.SocialWaysHipError, match="DeviceNoise"):
            tr.G.sample(obsv, 2, 12, sb, noise=sw.DeviceNoise(1))
