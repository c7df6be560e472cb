"""Shared by the tests of pinn_binned_sums / pinn_causal_cdf / pinn_sample_box_cdf (test_emulated_causal.py, test_gpu_causal.py,
test_causal_host.py): the numpy statements of the bin rule, the causal weights and their CDF, and the inverse-CDF draw, on the Philox and box
references of tests/_sample_cases.py."""
import functools
import math

import numpy as np

from tests import _sample_cases as SC

MAX_BINS = 64
SUM_N = (1, 63, 64, 65, 255, 257, 70001)
SUM_BINS = (1, 7, 16, 64)
LO, HI = 0.0, 16.0                                     # powers of two: with 16 or 64 bins the interior edges are exact fp32 numbers
EPS52 = 2.0 ** -52


# ---- binned sums --------------------------------------------------------------------------------------------------------------------------
def bin_rule(coord, lo, hi, n_bins):
    """the bin of every coordinate in numpy float32, as include/pinn_hip.h states it (NaN coordinates: bin 0, to be masked by the caller)"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = coord.astype(np.float32) - np.float32(lo)
        q = d * np.float32(n_bins / (hi - lo))
        b = np.clip(np.floor(q), 0, n_bins - 1)
    return np.where(np.isnan(b), 0, b).astype(np.int64)


def counted(value, coord):
    with np.errstate(invalid="ignore"):
        return np.isfinite(value) & (value >= 0) & ~np.isnan(coord)


@functools.lru_cache(maxsize=None)
def sums_case(n):
    """(value, coord) float32 [n]: coordinates over [LO - 2, HI + 2] with both edges of the range, points outside it on both sides, a NaN and
    values exactly on interior bin edges; scores |N(0,1)|^2 with a negative, -inf, +inf and a NaN"""
    rng = np.random.default_rng(900 + n)
    coord = (LO - 2.0 + (HI - LO + 4.0) * rng.random(n)).astype(np.float32)
    value = (rng.standard_normal(n) ** 2).astype(np.float32)
    edges = [LO, HI, LO - 1.5, HI + 1.5, 0.25, 1.0, 8.0, 15.75]
    for k, e in enumerate(edges[:max(0, n - 1)]):
        coord[(7 * k + 1) % n] = e
    if n >= 63:
        value[2], value[n // 2], value[n - 2], value[n // 3] = -1.0, -np.inf, np.inf, np.nan
        coord[n // 5] = np.nan
    return value, coord


def binned_reference(value, coord, lo, hi, n_bins):
    """(sums [n_bins] by math.fsum, counts [n_bins], sum |v| per bin) over the counted points"""
    ok = counted(value, coord)
    b = bin_rule(coord, lo, hi, n_bins)[ok]
    v = value[ok].astype(np.float64)
    sums = np.array([math.fsum(v[b == k]) for k in range(n_bins)])
    return sums, np.bincount(b, minlength=n_bins).astype(np.float64), np.array([math.fsum(np.abs(v[b == k])) for k in range(n_bins)])


# ---- causal weights and their CDF ---------------------------------------------------------------------------------------------------------
def cdf_reference(binned, eps, floor):
    """the formulas of pinn_causal_cdf in numpy float64 from a host [2, B] array: (m, c, w, cdf64 [B + 1], cdf32 [B + 1] -- rounded, made
    non-decreasing, cdf32[B] = 1)"""
    s = np.asarray(binned, dtype=np.float64)
    B = s.shape[1]
    m = np.divide(s[0], s[1], out=np.zeros(B), where=s[1] > 0)
    c = np.zeros(B)
    for b in range(1, B):
        c[b] = c[b - 1] + m[b - 1]
    w = np.exp(-eps * c)
    d = np.maximum(w, min(floor, 1.0))                 # (no w exceeds 1: a floor above 1 is used as 1)
    total = 0.0
    for b in range(B):
        total += d[b]
    cdf64, acc = np.zeros(B + 1), 0.0
    for b in range(1, B + 1):
        acc += d[b - 1]
        cdf64[b] = acc / total
    cdf32 = np.maximum.accumulate(cdf64.astype(np.float32))
    cdf32[B] = 1.0
    return m, c, w, cdf64, cdf32


def w_bound(B, eps, c):
    """relative error allowed on w_b against the float64 reference: c_b carries at most B + 1 roundings and the product with eps one more, an
    argument error x delta becomes the same relative error of exp(-x), and exp itself is within a few ulp"""
    return EPS52 * (4.0 + (B + 2) * eps * c)


def profile_case(B, seed=5):
    """a [2, B] array of sums and counts with one empty bin (from 4 bins up)"""
    rng = np.random.default_rng(seed + B)
    counts = rng.integers(1, 2000, B).astype(np.float64)
    sums = counts * (0.05 + rng.random(B)) * np.linspace(0.2, 2.0, B)
    if B >= 4:
        counts[B // 2], sums[B // 2] = 0.0, 0.0
    return np.stack([sums, counts])


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------
def uniform_table(B):
    return (np.arange(B + 1, dtype=np.float64) / B).astype(np.float32)


def general_table(B=16):
    """a causal table with widths that fall by two orders of magnitude"""
    return cdf_reference(profile_case(B), 0.6, 0.01)[4]


# zero-width bins, the first and the last among them
GAP_TABLE = np.array([0.0, 0.0, 0.25, 0.25, 0.75, 1.0, 1.0], dtype=np.float32)
SHARE_SEED, SHARE_STREAM, SHARE_N = 1111, 3, 65536


def draw_reference(seed, stream, first, n, lo, hi, table):
    """The draw of pinn_sample_box_cdf in numpy: (points float32 [n, dim] with the time column by the fp32 formulas, b int64 [n], t64 float64
    [n]: the float64 evaluation of the same formulas from the same fp32 table and the same u)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    dim, B = lo.size, table.size - 1
    U = SC.unit_box(seed, stream, first, n, dim)
    lo32, span32, hi32 = lo.astype(np.float32), (hi - lo).astype(np.float32), hi.astype(np.float32)
    # fma(u, span, lo) with one rounding: the float64 product of two fp32 numbers is exact, the sum rounds once in float64 and once to fp32 --
    # a double rounding that differs from the fma in rare ties only, which is why the uniform cases compare with the BOX kernel, not with this
    P = np.minimum((U.astype(np.float64) * span32 + lo32).astype(np.float32), hi32)
    u = U[:, dim - 1]
    b = np.searchsorted(table[:B], u, side="right").astype(np.int64) - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.minimum((u - table[b]) / (table[b + 1] - table[b]), np.float32(1))
        s = (b.astype(np.float32) + f) / np.float32(B)
        t32 = np.minimum((s.astype(np.float64) * span32[-1] + lo32[-1]).astype(np.float32), hi32[-1])
        T = table.astype(np.float64)
        f64 = np.minimum((u.astype(np.float64) - T[b]) / (T[b + 1] - T[b]), 1.0)
    t64 = np.minimum(float(lo32[-1]) + (b + f64) / B * float(span32[-1]), float(hi32[-1]))
    P[:, dim - 1] = t32
    return P, b, t64


def t_bound(lo, hi):
    """four fp32 roundings in s and the fma, with slack: 8 * 2^-24 * max(span, |lo|, |hi|)"""
    return 8.0 * 2.0 ** -24 * max(hi - lo, abs(lo), abs(hi))


def share_errors(b, table):
    """(|count - n p| in binomial sigmas per bin with p > 0, the counts of the bins with p == 0)"""
    B = table.size - 1
    p = np.diff(table.astype(np.float64))
    counts = np.bincount(b, minlength=B).astype(np.float64)
    n = float(b.size)
    pos = p > 0
    return np.abs(counts[pos] - n * p[pos]) / np.sqrt(n * p[pos] * (1 - p[pos]) + 1e-300), counts[~pos]
