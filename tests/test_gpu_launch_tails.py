"""The second code path of the launches in csrc/sw_misc.hip that cap their grid or clamp a last partial workgroup, against
float64 numpy written from the kernels' header comments (train.py:379-385, 527-536, 587-614; calc_statistics.py:28-32):

* adam_packed_kernel (at most 512 x 256 threads) at n = 2 * 131 072 + 37: a full second trip of the grid loop and a partial
  third, three updates with the step as a device scalar, every element of w / exp_avg / exp_avg_sq against float64 Adam
  under the bound of test_gpu_kernels.test_adam_packed_kernel_equals_torch_fused_adam, no weight left at its start bits,
  and the registered discriminator images kept equal to the scattered weights;
* traj_dist_kernel (at most 2 048 x 256 threads) at 629 562 entries, t0 = 0 and a single counted frame (T - t0 = 1);
* sample_reduce_kernel / variety_grad_kernel / sample_rank_kernel at B = 259 (B % 4 = B % 256 = 3) with K = 1, 64, 130
  (variety: 1, 64, its limit), the outputs inside NaN-prefilled larger allocations whose rows [B, B + 4) keep their bits.

The inputs of the three selection kernels lie on binary grids on which their float32 sums are exact (checked without a GPU
by test_grid_inputs_sum_exactly_in_float32), so the selections, integer ranks and tie rules (the lowest k wins; constructed
ties beside the ones the grid produces) are compared exactly and the quotients / fused multiply-adds to one float32
rounding (2^-23 relative).  The ADE/FDE second trip lives with its test,
test_gpu_kernels.test_loss_and_ade_reductions_any_batch_size.

Seeded faults these cases kill (profiles/seeded_faults.txt): the doubled grid stride of adam_packed_kernel and of
traj_dist_kernel, which the covering modules let through before.  Observed on an MI355X (pytest -s): the largest error of
the Adam case is 0.26 of its bound on the weights, 0.008 on exp_avg, below 0.001 on exp_avg_sq; every other comparison of
this module is exact or one rounding.  The 14 GPU cases take 0.6 s together."""
import numpy as np
import pytest
import torch

from _util import assert_close

ADAM_N = 2 * 131072 + 37
LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-8
B_TAIL = 259
ULP = 2.0 ** -23
NAN_BITS = 0x7FC00000


# ---- inputs (host) ------------------------------------------------------------------------------------------------------------
def reduce_inputs(K, B=B_TAIL):
    """err (K, B, 2) on the grid of 1/64 in [0, 8): sums over K <= 130 draws need 17 bits.  The last agent's draws 5 and 9
    (where K allows) share the smallest ADE and FDE."""
    rng = np.random.default_rng(100 + K)
    err = rng.integers(0, 512, size=(K, B, 2)).astype(np.float32) / 64.0
    if K > 9:
        err[:, B - 1] += 0.25
        err[5, B - 1] = err[9, B - 1] = 0.125
    return err


def variety_inputs(K, B=B_TAIL, Tp=12):
    """predK (K, B, Tp, 4), gt (B, Tp, 2), dpredK (K, B, Tp, 4) on the grid of 1/8 in [-4, 4): squared differences are
    multiples of 1/64 below 64, their sum over 2 Tp terms needs 17 bits.  The last agent's copies 5 and 9 equal the truth."""
    rng = np.random.default_rng(200 + K)
    grid = lambda *s: rng.integers(-32, 32, size=s).astype(np.float32) / 8.0
    predK, gt, d = grid(K, B, Tp, 4), grid(B, Tp, 2), grid(K, B, Tp, 4)
    if K > 9:
        for b in range(3, B, 8):                       # copies 7 and 2 of every eighth agent: one grid step off the truth
            predK[7, b, :, :2] = predK[2, b, :, :2] = gt[b]
            predK[7, b, 0, 0] = predK[2, b, 0, 0] = gt[b, 0, 0] + 0.125
        predK[5, B - 1, :, :2] = predK[9, B - 1, :, :2] = gt[B - 1]
    return predK, gt, d


def rank_inputs(K, B=B_TAIL):
    """score (K, B) on the grid of 1/2 (most draws tie with others), err (K, B, 2), best (B,) = the min-ADE draw.  All draws
    of the last agent score alike."""
    rng = np.random.default_rng(300 + K)
    score = (np.round(rng.normal(size=(K, B)) * 2) / 2).astype(np.float32)
    score[:, B - 1] = 0.5
    err = rng.random(size=(K, B, 2)).astype(np.float32)
    return score, err, err[..., 0].argmin(axis=0).astype(np.int32)


def test_grid_inputs_sum_exactly_in_float32():
    """What the exact comparisons below rely on: the float32 sums the kernels form equal the float64 sums in any order, equal
    sums (ties) occur, and the constructed ties are the smallest entries of the last agent."""
    for K in (1, 64, 130):
        err = reduce_inputs(K)
        s32 = np.zeros(err.shape[1:], np.float32)
        for k in range(K):
            s32 = s32 + err[k]
        assert np.array_equal(s32.astype(np.float64), err.astype(np.float64).sum(0))
        if K > 9:
            assert err[:, -1, 0].argmin() == 5 and err[9, -1, 0] == err[5, -1, 0] and (np.delete(err[:, -1, 0], [5, 9]) > 0.125).all()
    for K in (1, 64):
        predK, gt, _ = variety_inputs(K)
        q = (predK[..., :2] - gt[None]) ** 2
        s32 = np.zeros(q.shape[:2], np.float32)
        for t in range(q.shape[2]):
            s32 = s32 + q[:, :, t, 1]
            s32 = s32 + q[:, :, t, 0]
        s64 = q.astype(np.float64).sum((2, 3))
        assert np.array_equal(s32.astype(np.float64), s64)
        if K > 9:
            assert s64[5, -1] == 0.0 and s64[9, -1] == 0.0 and (np.delete(s64[:, -1], [5, 9]) > 0).all()
            srt = np.sort(s64, axis=0)
            assert (srt[0] == srt[1]).sum() >= 1 + len(range(3, B_TAIL, 8)) and (s64[:, 3::8].argmin(0) == 2).all()
    for K in (64, 130):
        score = rank_inputs(K)[0]
        assert len(np.unique(score)) < 32 and (score[:, -1] == 0.5).all()


# ---- float64 references -------------------------------------------------------------------------------------------------------
def adam64(w, m, v, g, t):
    """One Adam update (train.py:379-385, torch.optim.Adam without weight decay / amsgrad) in float64."""
    g = g.astype(np.float64)
    m = BETA1 * m + (1 - BETA1) * g
    v = BETA2 * v + (1 - BETA2) * g * g
    w = w - LR / (1 - BETA1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - BETA2 ** t) + EPS)
    return w, m, v


def _adam_check(name, got, ref, floor):
    err = np.abs(got.astype(np.float64) - ref)
    tol = floor + 4e-6 * np.abs(ref)
    bad = err > tol
    assert not bad.any(), "%s: %d elements off, first at %d, max err %.3e" % (name, bad.sum(), int(np.argmax(bad)), err.max())
    return float((err / tol).max())


def _nan_padded(rows, cols, dtype=torch.float32):
    """(rows + 4, cols) filled with the NaN bit pattern; the kernel gets the first `rows` rows."""
    t = torch.full((rows + 4, cols), NAN_BITS, dtype=torch.int32, device="cuda")
    return t if dtype == torch.int32 else t.view(torch.float32)


def _pad_untouched(t, rows):
    return bool((t[rows:].view(torch.int32) == NAN_BITS).all())


# ---- sw_adam_packed -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_adam_packed_second_and_third_trip_against_float64():
    from socialways_amd import _lib as L
    n = ADAM_N
    assert n > 2 * 512 * 256 and n % 256 != 0
    gen = torch.Generator(device="cpu").manual_seed(3)
    w0 = torch.randn(n, generator=gen)
    w, m, v = w0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    rw, rm, rv = w0.numpy().astype(np.float64), np.zeros(n), np.zeros(n)
    gmax = 0.0
    for t in (1, 2, 3):
        g = torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=gen))
        gmax = max(gmax, float(g.abs().max()))
        step = torch.full((), float(t), device="cuda")
        gd = g.cuda()
        L.call("sw_adam_packed", L.ptr(w), L.ptr(gd), L.ptr(m), L.ptr(v), n, L.ptr(step), LR, BETA1, BETA2, EPS, 0, L.stream())
        w_prev = rw
        rw, rm, rv = adam64(rw, rm, rv, g.numpy(), t)
        if t == 1:
            # a skipped element keeps its start bits.  Every element whose float64 update exceeds one ulp of its weight has
            # to move (a gradient so small that the update rounds away is not a skipped element)
            moves = (np.abs(rw - w_prev) > np.spacing(np.abs(w0.numpy()))) & (g.numpy() != 0)
            assert moves.mean() > 0.999
            same = (w.cpu().view(torch.int32) == w0.view(torch.int32)).numpy()
            assert not (same & moves).any(), "%d weights at their start bits, first at %d" % ((same & moves).sum(),
                                                                                                  int(np.argmax(same & moves)))
    torch.cuda.synchronize()
    worst = [_adam_check("weights", w.cpu().numpy(), rw, 1e-9), _adam_check("exp_avg", m.cpu().numpy(), rm, 2e-7 * gmax),
             _adam_check("exp_avg_sq", v.cpu().numpy(), rv, 2e-7 * gmax * gmax)]
    print("adam_packed n=%d: largest err / bound for w, m, v = %.3f %.3f %.3f" % (n, *worst))


@pytest.mark.gpu
def test_adam_packed_keeps_registered_disc_images_current():
    """disc_Tp = 12 with D's images registered: after the update the image holds the new weight in both places of every
    element (sw_disc_image_table) and zero everywhere else; the weights themselves equal float64 Adam."""
    import socialways_amd as sw
    from socialways_amd import _lib as L
    torch.manual_seed(12)
    D = sw.Discriminator(12, 64, 2, device=torch.device("cuda:0"))
    lib = L.load()
    n = D._flat.numel()
    tab_h = np.empty((n, 2), dtype=np.int32)
    assert lib.sw_disc_image_table(12, tab_h.ctypes.data) == 0
    tab = torch.from_numpy(tab_h).cuda()
    img = torch.zeros(lib.sw_disc_image_floats(12), device="cuda")
    w0 = D._flat.detach().clone()
    gen = torch.Generator(device="cpu").manual_seed(4)
    g = torch.randn(n, generator=gen) * 1e-2
    m, v, step = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.ones((), device="cuda")
    L.call("sw_disc_images", L.ptr(D._flat), L.ptr(img), L.ptr(tab), 12, L.stream())
    try:
        gd = g.cuda()
        L.call("sw_adam_packed", L.ptr(D._flat), L.ptr(gd), L.ptr(m), L.ptr(v), n, L.ptr(step), LR, BETA1, BETA2, EPS, 12,
               L.stream())
        torch.cuda.synchronize()
    finally:
        L.call("sw_disc_images", None, None, None, 0, None)
    w1 = D._flat.detach().cpu().numpy()
    rw, _, _ = adam64(w0.cpu().numpy().astype(np.float64), np.zeros(n), np.zeros(n), g.numpy(), 1)
    _adam_check("weights", w1, rw, 1e-9)
    want = np.zeros(img.numel(), np.float32)
    for c in (0, 1):
        has = tab_h[:, c] >= 0
        want[tab_h[has, c]] = w1[has]
    assert (tab_h >= 0).any() and not np.array_equal(w1, w0.cpu().numpy())
    assert np.array_equal(img.cpu().numpy().view(np.int32), want.view(np.int32))


# ---- sw_traj_dist -------------------------------------------------------------------------------------------------------------
def _traj_ref(a, b, t0):
    d = a[:, None, :, t0:].astype(np.float64) - b[None, :, :, t0:].astype(np.float64)
    return np.sqrt((d ** 2).sum(-1)).mean(-1).transpose(2, 0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("Na,Nb,nPed,T,t0", [(331, 317, 6, 2, 1), (331, 317, 6, 2, 0), (9, 4, 5, 7, 0), (9, 4, 5, 7, 6)])
def test_traj_dist_grid_stride_first_frame_and_single_frame(Na, Nb, nPed, T, t0):
    import socialways_amd as sw
    if Na > 9:
        assert Na * Nb * nPed > 2048 * 256 and Na % 256 and Nb % 256
    rng = np.random.default_rng(Na + t0)
    a, b = rng.normal(size=(Na, nPed, T, 2)).astype(np.float32), rng.normal(size=(Nb, nPed, T, 2)).astype(np.float32)
    D = sw.stats.traj_dist(a, b, t0).cpu().numpy()
    assert D.shape == (nPed, Na, Nb)
    assert_close(D, _traj_ref(a, b, t0), 2e-6, 1e-7, "mean displacement matrix")
    if Na > 9:
        Dm = sw.stats.traj_dist(a, a, t0)
        assert torch.equal(Dm, Dm.transpose(1, 2)), "d(i,j) == d(j,i) bitwise"


# ---- sw_sample_reduce ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 64, 130])
def test_sample_reduce_last_partial_workgroup(K):
    from socialways_amd import _lib as L
    B = B_TAIL
    err = reduce_inputs(K)
    pa, best = _nan_padded(B, 4), _nan_padded(B, 1, torch.int32)
    e = torch.from_numpy(err).cuda()
    L.call("sw_sample_reduce", L.ptr(e), B, K, L.ptr(pa), L.ptr(best), L.stream())
    torch.cuda.synchronize()
    assert _pad_untouched(pa, B) and _pad_untouched(best, B)
    e64 = err.astype(np.float64)
    got = pa[:B].cpu().numpy().astype(np.float64)
    assert_close(got[:, :2], e64.mean(0), ULP, 0.0, "mean ADE / FDE")
    assert np.array_equal(got[:, 2:], e64.min(0)), "min ADE / FDE are selections"
    assert np.array_equal(best[:B, 0].cpu().numpy(), e64[..., 0].argmin(0)), "the lowest k among equal ADEs"
    if K > 9:
        assert int(best[B - 1, 0]) == 5


# ---- sw_variety_grad ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 64])
def test_variety_grad_last_partial_workgroup(K):
    from socialways_amd import _lib as L
    B, Tp = B_TAIL, 12
    predK, gt, d0 = variety_inputs(K, B, Tp)
    scale = float(np.float32(0.37))
    kmin, l2min = _nan_padded(B, 1, torch.int32), _nan_padded(B, 1)
    p, g, d = torch.from_numpy(predK).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(d0).cuda()
    L.call("sw_variety_grad", L.ptr(p), L.ptr(g), K, B, Tp, scale, L.ptr(d), L.ptr(kmin), L.ptr(l2min), L.stream())
    torch.cuda.synchronize()
    assert _pad_untouched(kmin, B) and _pad_untouched(l2min, B)
    diff = predK[..., :2].astype(np.float64) - gt[None].astype(np.float64)
    l2 = (diff ** 2).sum((2, 3)) / (2 * Tp)                                  # (K, B)
    km = l2.argmin(0)                                                        # first minimum: the lowest k
    assert np.array_equal(kmin[:B, 0].cpu().numpy(), km)
    assert_close(l2min[:B, 0].cpu().numpy(), l2.min(0), ULP, 0.0, "l2min")
    want = d0.astype(np.float64)
    rows = np.arange(B)
    want[km, rows, :, :2] += scale * diff[km, rows]
    got = d.cpu().numpy()
    touched = np.zeros(d0.shape, bool)
    touched[km, rows, :, :2] = True
    assert np.array_equal(got[~touched].view(np.int32), d0[~touched].view(np.int32)), "only copy kmin[b], columns 0:2, changes"
    assert_close(got[touched], want[touched], ULP, 1e-12, "dpredK")
    if K > 9:
        assert int(kmin[B - 1, 0]) == 5 and float(l2min[B - 1, 0]) == 0.0


# ---- sw_sample_rank -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 64, 130])
def test_sample_rank_last_partial_workgroup(K):
    from socialways_amd import _lib as L
    B = B_TAIL
    score, err, best = rank_inputs(K)
    s, e, bst = torch.from_numpy(score).cuda(), torch.from_numpy(err).cuda(), torch.from_numpy(best).cuda()
    full = np.argsort(-score.astype(np.float64).T, axis=1, kind="stable")        # (B, K): descending, the lowest k first
    rank_of_best = (full == best[:, None]).argmax(1)
    rows = np.arange(B)[:, None]
    for M in sorted({1, min(5, K), K}):
        order, pa = _nan_padded(B, M, torch.int32), _nan_padded(B, 5)
        L.call("sw_sample_rank", L.ptr(s), L.ptr(e), L.ptr(bst), B, K, M, L.ptr(order), L.ptr(pa), L.stream())
        torch.cuda.synchronize()
        assert _pad_untouched(order, B) and _pad_untouched(pa, B)
        assert np.array_equal(order[:B].cpu().numpy(), full[:, :M]), (K, M)
        top = err.transpose(1, 0, 2)[rows, full[:, :M]]                           # (B, M, 2)
        want = np.concatenate([top[:, 0], top.min(1), rank_of_best[:, None].astype(np.float32)], axis=1)
        assert np.array_equal(pa[:B].cpu().numpy(), want), (K, M)
        assert order[B - 1].tolist() == list(range(M)), "equal scores: ascending k"
