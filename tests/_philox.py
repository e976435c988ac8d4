"""Philox4x32-10 in numpy, written from the specification of the device noise stream (include/socialways_hip.h,
sw_noise_uniform) - the reference the kernel is compared with bit for bit.

  round:   (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped after each
           of the 10 rounds by (W0, W1)
  stream:  key = (seed low 32 bits, seed high 32 bits), counter = (row, draw, step, (column >> 2) + 256 domain); the four
           output words are columns 4b .. 4b+3 of column block b; value = float(word >> 8) * 2^-24
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 broadcastable arrays of 32-bit words, key: 2 words -> 4 uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & MASK for c in counter])
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2            # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniform(seed, domain, rows, cols, step0=0, n_steps=1, draw0=0, n_draws=1, row0=0, ld=None):
    """The (n_steps, n_draws, rows, ld) float32 block sw_noise_uniform writes: zero in the columns cols .. ld-1."""
    ld = (cols + 3) // 4 * 4 if ld is None else ld
    nb = (cols + 3) // 4
    t = (step0 + np.arange(n_steps, dtype=np.uint64))[:, None, None, None]
    k = (draw0 + np.arange(n_draws, dtype=np.uint64))[None, :, None, None]
    i = (row0 + np.arange(rows, dtype=np.uint64))[None, None, :, None]
    b = (np.arange(nb, dtype=np.uint64) + np.uint64(256 * domain))[None, None, None, :]
    words = philox4x32_10((i, k, t, b), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w = np.stack(words, axis=-1).reshape(n_steps, n_draws, rows, 4 * nb)
    out = np.zeros((n_steps, n_draws, rows, ld), dtype=np.float32)
    out[..., :cols] = ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24))[..., :cols]
    return out


def stream_statistics(x):
    """x (draws, rows, columns) of the stream -> dict: |mean - 1/2| in units of sqrt(1 / (12 N)), the 16-bin chi-square
    statistic (15 degrees of freedom), the largest |Pearson correlation| between neighbours along columns, rows and draws
    in units of 1 / sqrt(N), and the extremes."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    counts = np.bincount(np.minimum((x * 16).astype(np.int64), 15).ravel(), minlength=16)
    corr = []
    for ax in (2, 1, 0):
        a, b = np.take(x, range(0, x.shape[ax] - 1), axis=ax).ravel(), np.take(x, range(1, x.shape[ax]), axis=ax).ravel()
        corr.append(abs(np.corrcoef(a, b)[0, 1]) * np.sqrt(n))
    return dict(n=n, mean_sigma=abs(x.mean() - 0.5) / np.sqrt(1.0 / (12 * n)), chi2=float(((counts - n / 16.0) ** 2 / (n / 16.0)).sum()),
                corr_sigma=max(corr), lo=float(x.min()), hi=float(x.max()))


def assert_uniform(x, what=""):
    """The acceptance conditions of the stream at N = x.size: |mean - 1/2| < 4 sqrt(1 / (12 N)); 16-bin chi-square < 37.7 (the
    99.9 % point at 15 degrees of freedom); neighbour correlations < 4 / sqrt(N); all values in [0, 1)."""
    s = stream_statistics(x)
    print("%s: N %d, mean %.2f sigma, chi2 %.1f, max neighbour correlation %.2f sigma, range [%.3g, %.8g]"
          % (what, s["n"], s["mean_sigma"], s["chi2"], s["corr_sigma"], s["lo"], s["hi"]))
    assert s["mean_sigma"] < 4.0, (what, s)
    assert s["chi2"] < 37.7, (what, s)
    assert s["corr_sigma"] < 4.0, (what, s)
    assert 0.0 <= s["lo"] and s["hi"] < 1.0, (what, s)
    return s
