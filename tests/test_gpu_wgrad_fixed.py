"""The fixed part of a weight-gradient launch (csrc/sw_wgrad.hip, csrc/sw_wgrad_dev.h): how a job finds its problem (all search
keys in one fetch, compared in registers; NB, rows per slice and the wg_run instance precomputed on the host), the prefetch
in front of the accumulator setup, the 16-byte LDS rows / workspace rows of the epilogue, and the reduction's wave-uniform
lookup over per-problem padded element ranges with (n, k) by a multiply instead of a division.

Every operand is a view into a larger allocation filled with NaN with a row stride wider than the logical width, outputs are
pre-filled with NaN (accumulate: with random values).  Reference: delta.double().T @ act.double() and the column sums.
Tolerance: 2e-5 of each tensor's largest entry (the gradient bound of the float64 pin) - the bound of
tests/test_gpu_wgrad_bounds.py, whose sums are up to four times as long as the ones here.

Rows: 1, 3, 4, 5 (less than one 4-row group, one group, one group + 1 row: waves with an empty slice), 13 and 17 (one and
two groups per wave - a first trip of the four-group pipeline that is mostly padding -, the last live wave with a single row),
127 / 128 / 129 (both sides of the 32-rows-per-wave cap on the split: two whole trips per wave, then a second workgroup per
output block).  Delta widths 1, 2, 16, 32, 64, 80 (64 + 16: two
problems), 256 (four output blocks: the multiply that replaces j / NB); act widths 16 .. 64 (1 .. 4 k-tiles, b32 / b64 / b128
LDS writes), 80 and 160 (several column blocks = several problems, the ones column on the last)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-5
ROWS = (1, 3, 4, 5, 13, 17, 127, 128, 129)
NS = (1, 2, 16, 32, 64, 80, 256)
KS = (16, 32, 48, 64, 80, 160)
MAXP = 24                       # SW_WG_MAXP (csrc/sw_wgrad.h): problems of one batch
ENC_WHH = 320 + 16384           # lstm.weight_hh_l0 in the packed encoder buffer (sw_common.h)
ENC_N = 33600


def _L():
    from socialways_amd import _lib as L
    return L


def _dev():
    return torch.device("cuda:0")


def _ws(L):
    return torch.empty(L.workspace_floats(L.WS_WGRAD, 1, 2, 1), device=_dev())


def _nan_view(rows, cols, gen, front=1, back=1):
    """rows x cols random values inside a NaN allocation: NaN rows around them, 4 NaN columns in front of and at least 4
    behind every row."""
    ld = (cols + 3) // 4 * 4 + 8
    big = torch.full((front + rows + back, ld), float("nan"), device=_dev())
    view = big[front:front + rows, 4:4 + cols]
    view.copy_(torch.randn(rows, cols, generator=gen).to(_dev()))
    return big, view, ld


def _check(got, want, what):
    assert torch.isfinite(got).all(), what
    bound = TOL * max(float(want.abs().max()), 1e-30)
    err = float((got.double() - want).abs().max())
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("form", ("nodb", "db", "db-accumulate"))
@pytest.mark.parametrize("N", NS)
def test_every_row_count_and_width(N, form):
    L = _L()
    gen = torch.Generator().manual_seed(77 * N + len(form))
    ws = _ws(L)
    with_db, accumulate = form != "nodb", int(form == "db-accumulate")
    for K in KS:
        for R in ROWS:
            dbig, delta, ldd = _nan_view(R, N, gen)
            abig, act, lda = _nan_view(R, K, gen)
            if accumulate:
                dW0, db0 = torch.randn(N, K + 3, generator=gen).to(_dev()), torch.randn(N, generator=gen).to(_dev())
            else:
                dW0, db0 = torch.full((N, K + 3), float("nan"), device=_dev()), torch.full((N,), float("nan"), device=_dev())
            dW, db = dW0.clone(), db0.clone()
            L.call("sw_linear_wgrad", delta.data_ptr(), ldd, act.data_ptr(), lda, R, N, K, L.ptr(dW), K + 3,
                   L.ptr(db) if with_db else None, L.ptr(ws), accumulate, L.stream())
            want_W, want_b = delta.double().T @ act.double(), delta.double().sum(0)
            if accumulate:
                want_W, want_b = want_W + dW0[:, :K].double(), want_b + db0.double()
            _check(dW[:, :K], want_W, ("dW", R, N, K))
            pad, pad0 = dW[:, K:], dW0[:, K:]              # the row stride's 3 extra columns: untouched, bit for bit
            assert torch.equal(pad.view(torch.int32), pad0.view(torch.int32)), ("wrote outside dW", R, N, K)
            if with_db:
                _check(db, want_b, ("db", R, N, K))
            else:
                assert torch.equal(db.view(torch.int32), db0.view(torch.int32))
            assert dbig[0].isnan().all() and dbig[-1].isnan().all() and abig[0].isnan().all() and abig[-1].isnan().all()


@pytest.mark.parametrize("T,B", [(3, 1), (1, 5), (1, 13), (1, 17), (1, 127), (8, 16), (3, 43)])
def test_tail_columns_and_rows_without_an_act_operand(T, B):
    """The LSTM problem (sw_enc_lstm_wgrad): 256 delta columns against K = 64 + the 4-column tail + the ones column, rows
    below row0 = B without an act operand.  T * B = 3, 5, 13, 17, 127, 128, 129 rows."""
    L = _L()
    gen = torch.Generator().manual_seed(1000 * T + B)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(_dev())
    nan = float("nan")
    act_big = torch.full((T + 2, B, 384), nan, device=_dev())
    act = act_big[1:T + 1]
    act.copy_(rnd(T, B, 384))
    dg_big = torch.full((T + 1, B, 256), nan, device=_dev())
    dgates = dg_big[:T]
    dgates.copy_(rnd(T, B, 256))
    x4_big = torch.full((T + 1, B, 4), nan, device=_dev())
    x4s = x4_big[:T]
    x4s.copy_(rnd(T, B, 4))
    d_enc_w = torch.full((ENC_N,), nan, device=_dev())
    tmp = torch.full((2048,), nan, device=_dev())
    L.call("sw_enc_lstm_wgrad", L.ptr(rnd(ENC_N)), act.data_ptr(), x4s.data_ptr(), None, dgates.data_ptr(), B, T,
           L.ptr(d_enc_w), L.ptr(_ws(L)), L.ptr(tmp), L.stream())
    dg = dgates.double().reshape(T * B, 256)
    hprev = torch.cat([torch.zeros(1, B, 64, device=_dev()), act[:T - 1, :, 320:384]]).double()
    got_hh = d_enc_w[ENC_WHH:ENC_WHH + 16384].view(256, 64)
    if T == 1:          # every row lies below row0: no products at all
        assert torch.equal(got_hh, torch.zeros_like(got_hh))
    else:
        _check(got_hh, dg.T @ hprev.reshape(T * B, 64), ("dW_hh", T, B))
    _check(tmp[:1024].view(256, 4), dg.T @ x4s.double().reshape(T * B, 4), ("dWx", T, B))
    _check(tmp[1024:1280], dg.sum(0), ("dbx", T, B))
    assert torch.isfinite(d_enc_w).all()
    assert act_big[0].isnan().all() and act_big[-1].isnan().all() and dg_big[-1].isnan().all() and x4_big[-1].isnan().all()


def test_a_batch_of_exactly_the_most_problems():
    """SW_WG_MAXP problems in ONE launch through sw_wide_wgrad: the last search key decides, the job count is no multiple of
    the grid's padding, and the reduction's element ranges are padded to whole waves after problems of 1 x 16 .. 64 x 65
    elements.  A 25th problem would open a second batch (tests/test_gpu_wide_reference.py covers that)."""
    L = _L()
    gen = torch.Generator().manual_seed(24)
    shapes = [(ROWS[i % len(ROWS)] + 16 * (i % 5), (1, 2, 16, 32, 64)[i % 5], 4 * (1 + (7 * i) % 16), i % 3 != 0) for i in range(MAXP)]
    assert len(shapes) == MAXP and all(N <= 64 and K <= 64 for _, N, K, _ in shapes)        # one problem each
    arr = (ctypes.c_longlong * (10 * MAXP))()
    built = []
    for i, (R, N, K, bias) in enumerate(shapes):
        dbig, delta, ldd = _nan_view(R, N, gen)
        abig, act, lda = _nan_view(R, K, gen)
        dW = torch.full((N * K + 4,), float("nan"), device=_dev())
        db = torch.full((N + 4,), float("nan"), device=_dev()) if bias else None
        for j, v in enumerate((delta.data_ptr(), ldd, act.data_ptr(), lda, R, N, K, L.ptr(dW), K, L.ptr(db) if bias else 0)):
            arr[10 * i + j] = int(v)
        built.append((dbig, delta, abig, act, dW, db))
    assert L.load().sw_wide_wgrad(ctypes.cast(arr, ctypes.c_void_p), MAXP, L.ptr(_ws(L)), L.stream()) == 0
    torch.cuda.synchronize()
    for (R, N, K, bias), (dbig, delta, abig, act, dW, db) in zip(shapes, built):
        _check(dW[:N * K].view(N, K), delta.double().T @ act.double(), ("dW", R, N, K))
        assert dW[N * K:].isnan().all(), ("wrote behind dW", R, N, K)
        if bias:
            _check(db[:N], delta.double().sum(0), ("db", R, N, K))
            assert db[N:].isnan().all()
        assert dbig[0].isnan().all() and dbig[-1].isnan().all() and abig[0].isnan().all() and abig[-1].isnan().all()


def test_a_batch_with_precomputed_partials():
    """A dense scene of 17 agents: the social backward leaves per-slice partials of the embedder's three layers in the
    workspace (wg_add_pre, reduced by the generator's launch next to its GEMM problems, in the layout their producer
    writes).  Whole generator backward on NaN-prefilled gradients against float64."""
    from test_gpu_gen_reference import _check as gen_check
    gen_check("wgrad.pre", [17], 8, 12)


@pytest.mark.parametrize("lr", (0.0, 1e-3))
def test_adam_inside_the_reduction_equals_the_update_behind_it(lr):
    """A discriminator update (its LSTM problem carries db2: b_ih and b_hh receive the same sum) with Adam applied by the
    reduction, against the same call without Adam followed by sw_adam_packed: gradients, weights, both moments and the
    weight images, bit for bit.  lr = 0 leaves the weights as they were and still moves the moments."""
    import socialways_amd as sw
    from socialways_amd import ops
    L = _L()
    dev, B, To = _dev(), 17, 8
    torch.manual_seed(5)
    D = sw.Discriminator(12, 64, 2, device=dev)
    obsv = torch.randn(B, To, 2, device=dev).cumsum(1) * 0.1
    fake, real = torch.randn(B, 12, 4, device=dev) * 0.1, torch.randn(B, 12, 4, device=dev) * 0.1
    z = torch.rand(B, 32, device=dev)
    targets = torch.tensor([0.05, 0.95], device=dev)
    lib = L.load()
    n = D._flat.numel()
    tab_h = np.empty((n, 2), dtype=np.int32)
    assert lib.sw_disc_image_table(12, tab_h.ctypes.data) == 0
    tab = torch.from_numpy(tab_h).to(dev)
    img = torch.zeros(lib.sw_disc_image_floats(12), device=dev)
    w0, m0, v0 = D._flat.clone(), torch.randn(n, device=dev) * 0.01, torch.rand(n, device=dev) * 1e-4
    res = []
    for fused in (True, False):
        D._flat.copy_(w0)
        ws = ops.Workspaces(dev)
        L.call("sw_disc_images", L.ptr(D._flat), L.ptr(img), L.ptr(tab), 12, L.stream())
        try:
            assert ops.disc_update_supported(D._flat, B, To, 12)
            g = torch.full_like(D._flat, float("nan"))
            m, v, step = m0.clone(), v0.clone(), torch.full((), 3.0, device=dev)
            ops.disc_update(D._flat, obsv, [fake, real], targets, (0, 1), z, 1.0 / B, 0.25 / B, g, ws,
                            adam=(m, v, step, lr, 0.9, 0.999, 1e-8) if fused else None)
            if not fused:
                L.call("sw_adam_packed", L.ptr(D._flat), L.ptr(g), L.ptr(m), L.ptr(v), n, L.ptr(step), lr, 0.9, 0.999, 1e-8, 12,
                       L.stream())
            torch.cuda.synchronize()
            res.append((g, D._flat.clone(), m, v, img.clone()))
        finally:
            L.call("sw_disc_images", None, None, None, 0, None)
    # Parameter by parameter: the packed buffers' alignment padding belongs to no parameter - the reduction never touches it,
    # sw_adam_packed steps over it like over everything else (with the NaN the gradient buffer was pre-filled with).
    names = [k for k, _ in D.named_parameters()]
    for what, a, b in zip(("gradient", "weight", "exp_avg", "exp_avg_sq"), res[0], res[1]):
        for k, x, y in zip(names, D.split_grad(a), D.split_grad(b)):
            assert torch.isfinite(x).all(), (what, k)
            assert torch.equal(x, y), "%s of %s: max |diff| %.3e" % (what, k, float((x - y).abs().max()))
    assert torch.isfinite(res[0][4]).all() and torch.equal(res[0][4], res[1][4]), "images"
    grads = dict(zip(names, D.split_grad(res[0][0])))
    bih, bhh = [grads[k] for k in sorted(grads) if "bias_ih" in k or "bias_hh" in k]
    assert torch.equal(bih, bhh) and float(bih.abs().max()) > 0
    moved = any(not torch.equal(x, y) for x, y in zip(D.split_grad(res[0][1]), D.split_grad(w0)))
    assert moved is (lr != 0.0) and not torch.equal(res[0][2], m0)
