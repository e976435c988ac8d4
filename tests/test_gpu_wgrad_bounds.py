"""The weight-gradient GEMM reads its operands through bounded buffer loads: a wave's descriptor covers exactly the rows of
its slice, rows beyond it (prefetch overrun, the padding of the last 4-row group) and rows in front of it (the LSTM problem's
h_{t-1} at t = 0) read zero.  Here every operand is a view into a larger allocation filled with NaN, with a row stride wider
than the logical width: a descriptor that ends too late (or starts too early) lets a NaN row in, one that ends too early
loses rows and misses the float64 reference.

Reference: delta.double().T @ act.double() and the column sums.  Tolerance: 2e-5 of each tensor's largest entry (the
gradient bound of the float64 pin)."""
import pytest
import torch

TOL = 2e-5
EARG, ESHAPE = -1, -2
ROWS = (1, 2, 3, 4, 5, 7, 15, 17, 63, 65, 127, 129, 515)
NK = ((2, 80), (32, 48), (80, 160), (160, 64), (160, 32), (256, 64))
ENC_WHH = 320 + 16384           # lstm.weight_hh_l0 in the packed encoder buffer (sw_common.h)
ENC_N = 33600


def _L():
    from socialways_amd import _lib as L
    return L


def _ws(L, dev):
    return torch.empty(L.workspace_floats(L.WS_WGRAD, 1, 2, 1), device=dev)


def _up4(n):
    return (n + 3) // 4 * 4


def _nan_view(rows, cols, dev, gen, front=1, back=1):
    """rows x cols random values inside a NaN allocation: `front` / `back` NaN rows around them, 4 NaN columns in front
    and at least 4 behind every row (row stride = cols rounded up to 4, + 8)."""
    ld = _up4(cols) + 8
    big = torch.full((front + rows + back, ld), float("nan"), device=dev)
    view = big[front:front + rows, 4:4 + cols]
    view.copy_(torch.randn(rows, cols, generator=gen).to(dev))
    return big, view, ld


def _check(got, want, what):
    assert torch.isfinite(got).all(), what
    bound = TOL * max(float(want.abs().max()), 1e-30)
    err = float((got.double() - want).abs().max())
    assert err <= bound, (what, err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("with_db", (False, True), ids=("nodb", "db"))
@pytest.mark.parametrize("N,K", NK)
def test_linear_wgrad_reads_its_rows_and_nothing_else(N, K, with_db, accumulate):
    """R from fewer rows than one 4-row group over fewer groups than the pipeline holds and slices that end inside a group
    to more slices than rows; column blocks of 64 / 48 / 32 / 16 act columns, output blocks of 2 .. 64 delta columns."""
    L = _L()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1000 * N + K)
    ws = _ws(L, dev)
    for R in ROWS:
        dbig, delta, ldd = _nan_view(R, N, dev, gen)
        abig, act, lda = _nan_view(R, K, dev, gen)
        if accumulate:
            dW0, db0 = torch.randn(N, K, generator=gen).to(dev), torch.randn(N, generator=gen).to(dev)
        else:       # NaN: every element must be written
            dW0, db0 = torch.full((N, K), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)
        dW, db = dW0.clone(), db0.clone()
        L.call("sw_linear_wgrad", delta.data_ptr(), ldd, act.data_ptr(), lda, R, N, K, L.ptr(dW), K,
               L.ptr(db) if with_db else None, L.ptr(ws), accumulate, L.stream())
        want_W = delta.double().T @ act.double()
        want_b = delta.double().sum(0)
        if accumulate:
            want_W, want_b = want_W + dW0.double(), want_b + db0.double()
        _check(dW, want_W, ("dW", R, N, K))
        if with_db:
            _check(db, want_b, ("db", R, N, K))
        assert dbig[0].isnan().all() and dbig[-1].isnan().all() and abig[0].isnan().all() and abig[-1].isnan().all()


@pytest.mark.gpu
@pytest.mark.parametrize("with_h0", (False, True), ids=("zero-state", "h0"))
@pytest.mark.parametrize("B", (1, 5, 16, 17, 33))
@pytest.mark.parametrize("T", (1, 2, 3, 8))
def test_enc_lstm_wgrad_reads_its_rows_and_nothing_else(T, B, with_h0):
    """The LSTM problem takes h_{t-1} as "the act row one time step earlier": its act pointer lies one step IN FRONT of the
    buffer.  That step holds NaN here, and so does the step behind dgates / x4s.  dW_hh = sum_{t >= 1} dgates_t^T h_{t-1}
    (+ dgates_0^T h0), the composed input matrix dgates^T x4 and its bias (left in `tmp`) over all rows."""
    L = _L()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(100 * T + B)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    nan = float("nan")
    act_big = torch.full((T + 2, B, 384), nan, device=dev)
    act = act_big[1:T + 1]
    act.copy_(rnd(T, B, 384))
    dg_big = torch.full((T + 1, B, 256), nan, device=dev)
    dgates = dg_big[:T]
    dgates.copy_(rnd(T, B, 256))
    x4_big = torch.full((T + 1, B, 4), nan, device=dev)
    x4s = x4_big[:T]
    x4s.copy_(rnd(T, B, 4))
    h0 = rnd(B, 64) if with_h0 else None
    enc_w = rnd(ENC_N)
    d_enc_w = torch.full((ENC_N,), nan, device=dev)
    tmp = torch.full((2048,), nan, device=dev)
    ws = _ws(L, dev)
    L.call("sw_enc_lstm_wgrad", L.ptr(enc_w), act.data_ptr(), x4s.data_ptr(), L.ptr(h0), dgates.data_ptr(), B, T,
           L.ptr(d_enc_w), L.ptr(ws), L.ptr(tmp), L.stream())
    dg = dgates.double().reshape(T * B, 256)
    hprev = torch.cat([(h0 if with_h0 else torch.zeros(B, 64, device=dev))[None], act[:T - 1, :, 320:384]]).double()
    want_hh = dg.T @ hprev.reshape(T * B, 64)
    got_hh = d_enc_w[ENC_WHH:ENC_WHH + 16384].view(256, 64)
    if T == 1 and not with_h0:       # every row lies below row0: no products at all
        assert torch.equal(got_hh, torch.zeros_like(got_hh))
    else:
        _check(got_hh, want_hh, ("dW_hh", T, B))
    _check(tmp[:1024].view(256, 4), dg.T @ x4s.double().reshape(T * B, 4), ("dWx", T, B))
    _check(tmp[1024:1280], dg.sum(0), ("dbx", T, B))
    assert torch.isfinite(d_enc_w).all()
    assert act_big[0].isnan().all() and act_big[-1].isnan().all() and dg_big[-1].isnan().all() and x4_big[-1].isnan().all()


def test_argument_checks_return_before_any_device_call():
    """`p` is a non-NULL address nobody dereferences: every call returns from the host-side checks.  A problem whose row
    slices could span 2^31 bytes is refused (the kernel's offsets inside a slice are 32-bit byte offsets)."""
    lib = _L().load()
    p = 4096

    def lin(delta=p, ldd=64, act=p, lda=64, R=128, N=64, K=64, dW=p, ldw=64, db=p, ws=p):
        return lib.sw_linear_wgrad(delta, ldd, act, lda, R, N, K, dW, ldw, db, ws, 0, None)

    for kw in (dict(delta=None), dict(act=None), dict(dW=None), dict(ws=None), dict(R=0), dict(R=-1), dict(N=0), dict(K=0)):
        assert lin(**kw) == EARG, kw
    for kw in (dict(ldd=66), dict(lda=65), dict(N=257), dict(N=17),
               dict(R=2 ** 31 - 1, ldd=4, N=2), dict(R=2 ** 31 - 1, lda=4, K=2), dict(R=2 ** 24, ldd=128), dict(R=2 ** 23, lda=256)):
        assert lin(**kw) == ESHAPE, kw

    def enc(enc_w=p, act=p, x4s=p, dgates=p, B=8, T=8, d=p, ws=p, tmp=p):
        return lib.sw_enc_lstm_wgrad(enc_w, act, x4s, None, dgates, B, T, d, ws, tmp, None)

    for kw in (dict(enc_w=None), dict(act=None), dict(x4s=None), dict(dgates=None), dict(d=None), dict(ws=None), dict(tmp=None),
               dict(B=0), dict(T=0)):
        assert enc(**kw) == EARG, kw
    assert enc(B=2 ** 20, T=8) == ESHAPE          # 2^23 rows of 384 floats: a slice of a quarter of them spans 3 GiB
