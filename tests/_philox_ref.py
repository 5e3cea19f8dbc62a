"""NumPy restatement of the noise stream of `odehip_latent_sample` (include/odecgru_hip.h): Philox4x32-10 with the Random123 constants
and the documented word -> uniform -> Box-Muller mapping, in float64.  Independent of the library: nothing here loads it.

    q                = ((k * global_batch + b_global) * C + c) * 64 + pixel // 4
    (w0, w1, w2, w3) = philox4x32_10(counter = (q lo, q hi, offset lo, offset hi), key = (seed lo, seed hi))
    u(w)             = ((w >> 9) + 0.5) * 2**-23
    eps[4 pixels]    = r0 cos(2 pi u(w1)), r0 sin(2 pi u(w1)), r1 cos(2 pi u(w3)), r1 sin(2 pi u(w3)),   r_i = sqrt(-2 ln u(w_2i))
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]   # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x.astype(np.uint32) for x in c]


def word_uniform(w):
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals_of_quads(q, seed, offset):
    """q: uint64 array of global quad indices -> float64 array q.shape + (4,)."""
    q = np.asarray(q, dtype=np.uint64)
    seed, offset = int(seed), int(offset)
    w = philox4x32_10((q & np.uint64(MASK), q >> np.uint64(32), np.full(q.shape, offset & MASK), np.full(q.shape, offset >> 32)),
                      (seed & MASK, seed >> 32))
    out = np.empty(q.shape + (4,), dtype=np.float64)
    for p in range(2):
        r = np.sqrt(-2.0 * np.log(word_uniform(w[2 * p])))
        th = 2.0 * np.pi * word_uniform(w[2 * p + 1])
        out[..., 2 * p] = r * np.cos(th)
        out[..., 2 * p + 1] = r * np.sin(th)
    return out


def noise(n_samples, batch, channels, seed, offset, batch_offset=0, global_batch=None):
    """The (n_samples * batch, channels, 16, 16) float64 noise of a shard, sample-major, as `eps_out` lays it out."""
    global_batch = batch if global_batch is None else global_batch
    k = np.arange(n_samples, dtype=np.uint64)[:, None, None]
    b = np.arange(batch, dtype=np.uint64)[None, :, None] + np.uint64(batch_offset)
    j = np.arange(channels * 64, dtype=np.uint64)[None, None, :]
    q = (k * np.uint64(global_batch) + b) * np.uint64(channels * 64) + j
    return normals_of_quads(q, seed, offset).reshape(n_samples * batch, channels, 16, 16)


def moment_report(x):
    """|mean|, |var - 1|, |m4 - 3| in units of their standard errors under N(0, 1), and max |x|."""
    x = np.asarray(x, dtype=np.float64).ravel()
    n = x.size
    return {"n": n, "mean_se": abs(x.mean()) / np.sqrt(1.0 / n), "var_se": abs((x * x).mean() - x.mean() ** 2 - 1.0) / np.sqrt(2.0 / n),
            "m4_se": abs((x ** 4).mean() - 3.0) / np.sqrt(96.0 / n), "max_abs": float(np.abs(x).max())}


def check_moments(x):
    """The bounds of the stream's definition: 5 standard errors on the first three even / odd moments, |eps| < 6 (r <= 5.77)."""
    r = moment_report(x)
    assert r["mean_se"] <= 5.0 and r["var_se"] <= 5.0 and r["m4_se"] <= 5.0 and r["max_abs"] < 6.0, r
    return r
