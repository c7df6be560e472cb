"""Shared by the tests of pinn_sample_box / pinn_refine_keys (test_emulated_sample.py, test_gpu_sample.py): a Philox4x32-10 reference in numpy
and the float64 / float32 statements of the box map, the ball test and the sampling keys."""
import functools

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

# the published known-answer vectors of Philox4x32-10 (Random123 kat_vectors): counter, key, output
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two; returns the four output words as uint32 arrays.  uint64 arithmetic throughout."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def words(seed, stream, first, n, purpose):
    """[n, 4] uint32: the Philox block of the elements first .. first + n - 1 (counter = lo32 idx, hi32 idx, stream, purpose; key = seed)"""
    idx = np.uint64(first) + np.arange(n, dtype=np.uint64)
    out = philox4x32_10((idx & MASK, idx >> np.uint64(32), stream, purpose), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=1)


def unit_box(seed, stream, first, n, dim):
    """[n, dim] float32: (r_k >> 8) * 2^-24, exact"""
    return ((words(seed, stream, first, n, 0)[:, :dim] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24))


def box64(seed, stream, first, n, lo, hi):
    """[n, dim] float64: lo + u (hi - lo)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return lo + unit_box(seed, stream, first, n, lo.size).astype(np.float64) * (hi - lo)


def noise_u(seed, stream, first, n):
    """[n] float32: ((r_0 >> 9) + 0.5) * 2^-23 of the purpose-1 block, exact"""
    r0 = words(seed, stream, first, n, 1)[:, 0]
    return ((r0 >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


# ---- balls ------------------------------------------------------------------------------------------------------------------------------
def in_balls(cols, balls):
    """cols: the float32 columns x, y, (z); balls: (centre[3], radius, ndim, keep_boundary).  The fp32 statement of the test."""
    out = np.zeros(cols[0].size, dtype=bool)
    for centre, r, ndim, keep in balls:
        d2 = np.zeros(cols[0].size, dtype=np.float32)
        for k in (0, 1, 2)[:ndim]:
            d = cols[k] - np.float32(centre[k])
            d2 = d2 + d * d
        r2 = np.float32(r) * np.float32(r)
        out |= (d2 < r2) if keep else (d2 <= r2)
    return out


def boundary_margin(cols, balls):
    """min over points and balls of | |x - centre| - r | / r in float64: the ball test is not sensitive to fp32 rounding while this is >> eps32"""
    m = np.inf
    for centre, r, ndim, _ in balls:
        d2 = sum((cols[k].astype(np.float64) - centre[k]) ** 2 for k in range(ndim))
        m = min(m, float(np.abs(np.sqrt(d2) - r).min() / r))
    return m


DISC = ((0.5, 0.5, 0.0), 0.4, 2)
BALL = ((0.3, 0.6, 0.5), 0.35, 3)
MASK_SEED, MASK_STREAM = 1111, 0
SIZES = (1, 255, 256, 257, 70001, 300000)            # 300000 > 1024 * 256: the grid stride of the key kernels wraps


@functools.lru_cache(maxsize=None)
def mask_points(dim):
    """the unit-box points of the key tests, all sizes being prefixes of the largest (float32 [300000, dim])"""
    return unit_box(MASK_SEED, MASK_STREAM, 0, max(SIZES), dim)


def ball_cases(keep):
    """(name, dim, balls): a disc on (x, y, t) points without a z column; the disc and a ball on (x, y, z, t) points"""
    return (("disc", 3, (DISC + (keep,),)), ("disc+ball", 4, (DISC + (keep,), BALL + (keep,))))


# ---- sampling keys ----------------------------------------------------------------------------------------------------------------------
POWER_C = ((1.0, 0.0), (1.0, 1.0), (0.5, 1.0), (2.0, 0.1))
KEY_SEED, KEY_STREAM, KEY_FIRST = 2024, 3, 17


@functools.lru_cache(maxsize=None)
def sample_scores(n):
    """|N(0,1)|^2 in float32 with exact zeros, and -- from 16 points up -- one NaN, one negative and one +inf score"""
    rng = np.random.default_rng(600 + n)
    s = (rng.standard_normal(n) ** 2).astype(np.float32)
    s[rng.random(n) < 0.05] = 0.0
    if n >= 16:
        s[3], s[n // 2], s[n - 2] = np.nan, -1.0, np.inf
    if n == 1:
        s[0] = 1.5
    return s


def keys_reference(score, excluded, power, c, u, dtype):
    """The sampling keys in ``dtype`` arithmetic from the fp32 scores and the exact fp32 noise u: (keys, valid).  -inf where excluded (a ball,
    or a score that is not finite or is negative) or p == 0.  The mean is formed in float64 in both (the kernel does so too) and then rounded."""
    valid = ~excluded & np.isfinite(score) & (score >= 0)
    s = np.where(valid, score, 0).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = s if power == 1.0 else (np.sqrt(s) if power == 0.5 else np.power(s, dtype(power)))
        m = dtype(q[valid].astype(np.float64).mean()) if valid.any() else dtype(0)
        p = (q / m if m != 0 else np.zeros_like(q)) + dtype(c)
        key = np.log(p) - np.log(-np.log(u.astype(dtype)))
    key = np.where(valid & (p > 0), key, -np.inf)
    return key, valid


def key_errors(got, score, excluded, power, c, u):
    """(delta, delta_ref, same_inf): max |got - float64 reference| and max |float32 reference - float64 reference| over the finite keys, and
    whether the -inf set of ``got`` is the reference's"""
    k64, _ = keys_reference(score, excluded, power, c, u, np.float64)
    k32, _ = keys_reference(score, excluded, power, c, u, np.float32)
    fin = np.isfinite(k64)
    same = bool(np.array_equal(np.isneginf(got), ~fin) and np.array_equal(np.isneginf(k32), ~fin))
    if not fin.any():
        return 0.0, 0.0, same
    with np.errstate(invalid="ignore"):
        return float(np.abs(got.astype(np.float64) - k64)[fin].max()), float(np.abs(k32.astype(np.float64) - k64)[fin].max()), same
