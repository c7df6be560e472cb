"""CPU tests of pinn_binned_sums, pinn_causal_cdf and pinn_sample_box_cdf: the kernel sources compiled for x86 against the SIMT emulator, on host
arrays framed by guard words that are checked after every call (as in test_emulated_sample.py).  The references are in tests/_causal_cases.py."""
import ctypes
import sys

import numpy as np
import pytest

from tests import _causal_cases as CC
from tests import _sample_cases as SC
from tests.test_emulated_sample import BOX_N, FIRSTS, SEEDS, STREAMS, Guarded, bits, draw, emu, put  # noqa: F401

WAVE_BOX = ((0.0, 0.0, 0.0), (30.0, 30.0, 20.0))
BOX_3D = ((-15.0, -15.0, -15.0, 2.0), (15.0, 15.0, 15.0, 14.0))


def binned(emu, value, coord, lo, hi, n_bins):
    """pinn_binned_sums on guarded copies -> float64 [2, n_bins]; guards intact, inputs unwritten"""
    n = value.size
    v, c = put(value), put(coord)
    ws, out = Guarded(emu.binned_sums_workspace_bytes(n, n_bins)), Guarded(16 * n_bins, fill=0xFF)
    emu.binned_sums(v.ptr, c.ptr, n, lo, hi, n_bins, out.ptr, ws.ptr, ws.nbytes)
    assert all(g.guards_intact() for g in (v, c, ws, out)), "a guard word was overwritten"
    assert np.array_equal(v.view(np.uint32), bits(value)) and np.array_equal(c.view(np.uint32), bits(coord)), "an input was written to"
    return out.view(np.float64).copy().reshape(2, n_bins)


def table(emu, sums, eps, floor):
    """pinn_causal_cdf on a guarded copy of the host [2, B] array -> (w float64 [B], cdf float32 [B + 1])"""
    B = sums.shape[1]
    s, w, cdf = put(np.ascontiguousarray(sums, dtype=np.float64)), Guarded(8 * B, fill=0xFF), Guarded(4 * (B + 1), fill=0xFF)
    emu.causal_cdf(s.ptr, B, eps, floor, w.ptr, cdf.ptr)
    assert all(g.guards_intact() for g in (s, w, cdf)), "a guard word was overwritten"
    assert np.array_equal(s.view(np.float64), np.asarray(sums, dtype=np.float64).reshape(-1)), "the input was written to"
    return w.view(np.float64).copy(), cdf.view(np.float32).copy()


def draw_cdf(emu, seed, stream, first, n, lo, hi, tab):
    """pinn_sample_box_cdf into guarded buffers -> float32 [n, dim]"""
    cols, t = [Guarded(4 * n, fill=0xFF) for _ in lo], put(tab)
    emu.sample_box(seed, stream, first, n, lo, hi, [c.ptr for c in cols], 0, t.ptr, tab.size - 1)
    assert all(c.guards_intact() for c in cols) and t.guards_intact(), "a guard word was overwritten"
    assert np.array_equal(t.view(np.uint32), bits(tab)), "the table was written to"
    return np.stack([c.view(np.float32).copy() for c in cols], axis=1)


# ---- binned sums --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", CC.SUM_BINS)
@pytest.mark.parametrize("n", CC.SUM_N)
def test_binned_sums_against_fsum(emu, n, n_bins):
    """counts equal the numpy float32 bin rule exactly; each sum within n_b * 2^-52 * sum|v| of math.fsum over the bin: n_b - 1 fp64 additions
    at 2^-53 each on partial sums no larger than sum|v|, with a factor 2 of slack"""
    value, coord = CC.sums_case(n)
    got = binned(emu, value, coord, CC.LO, CC.HI, n_bins)
    sums, counts, absum = CC.binned_reference(value, coord, CC.LO, CC.HI, n_bins)
    assert np.array_equal(got[1], counts), (n, n_bins)
    err = np.abs(got[0] - sums)
    print(f"n={n} bins={n_bins}: max err / bound {np.max(err / np.maximum(counts * CC.EPS52 * absum, 1e-300)):.3f}")
    assert (err <= counts * CC.EPS52 * absum).all(), (n, n_bins)
    assert np.array_equal(got, binned(emu, value, coord, CC.LO, CC.HI, n_bins))                   # two calls: identical bytes
    if n >= 63:
        assert counts.sum() == n - 5                                                          # the five skipped points of the case


def test_binned_sums_edges_clamp_and_skip(emu):
    """points exactly on interior edges go to the upper bin, both ends of the range and points outside it to the first / last bin; a negative,
    infinite or NaN value and a NaN coordinate are neither summed nor counted"""
    coord = np.array([0.0, 16.0, -3.0, 40.0, 4.0, 8.0, 7.9999995, 12.0, 1.0, 2.0, 3.0, np.nan, np.inf, -np.inf], dtype=np.float32)
    value = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, -1.0, np.inf, np.nan, 5.0, 256.0, 512.0], dtype=np.float32)
    got = binned(emu, value, coord, 0.0, 16.0, 4)
    assert np.array_equal(got, np.array([[1.0 + 4.0 + 512.0, 16.0 + 64.0, 32.0, 2.0 + 8.0 + 128.0 + 256.0], [3.0, 2.0, 1.0, 4.0]]))
    assert np.array_equal(binned(emu, value[:0], coord[:0], 0.0, 16.0, 4), np.zeros((2, 4)))          # n == 0: zeros


# ---- the causal weights and their CDF -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps,floor", [(0.6, 0.0), (0.6, 0.01), (25.0, 0.0), (1e3, 1e-3)])
@pytest.mark.parametrize("B", (1, 2, 7, 16, 63, 64))
def test_causal_cdf_against_float64(emu, B, eps, floor):
    sums = CC.profile_case(B)
    w, cdf = table(emu, sums, eps, floor)
    m, c, w64, cdf64, cdf32 = CC.cdf_reference(sums, eps, floor)
    assert cdf[0] == 0.0 and cdf[B] == 1.0 and (np.diff(cdf) >= 0).all() and w[0] == 1.0
    rel = np.abs(w - w64) / np.maximum(w64, 1e-300)
    assert (rel[w64 > 0] <= CC.w_bound(B, eps, c)[w64 > 0]).all() and (w[w64 == 0] <= 1e-300).all(), (B, eps)
    ulp = np.spacing(np.abs(cdf64).astype(np.float32)).astype(np.float64)
    assert (np.abs(cdf.astype(np.float64) - cdf64.astype(np.float32)) <= ulp).all(), (B, eps, floor)
    if B >= 4:
        assert m[B // 2] == 0.0 and w[B // 2 + 1] == w[B // 2]                                     # an empty bin counts as m = 0
    w2, cdf2 = table(emu, sums, eps, floor)
    assert np.array_equal(w, w2) and np.array_equal(bits(cdf), bits(cdf2))


def test_causal_cdf_known_answers(emu):
    for B in (1, 8, 16, 64):
        counts = np.full(B, 10.0)
        eq = np.stack([counts * 0.25, counts])                                                    # equal means m = 0.25 in every bin
        w, _ = table(emu, eq, 2.0, 0.0)
        want = np.exp(-2.0 * 0.25 * np.arange(B))
        assert (np.abs(w - want) <= CC.w_bound(B, 2.0, 0.25 * np.arange(B)) * want).all()
        uni = CC.uniform_table(B)
        # floor = 1 or eps = 0: the uniform table, exact; a floor above 1 is floor = 1 -- up to the largest double, whose 64-fold sum would
        # overflow and leave inf / inf in the table
        for eps, floor in ((2.0, 1.0), (0.0, 0.0), (2.0, 3.0), (2.0, sys.float_info.max)):
            assert np.array_equal(bits(table(emu, CC.profile_case(B), eps, floor)[1]), bits(uni)), (B, eps, floor)
        w, cdf = table(emu, np.zeros((2, B)), 3.0, 0.0)                                           # all-zero sums: w = 1, the uniform table
        assert np.array_equal(w, np.ones(B)) and np.array_equal(bits(cdf), bits(uni))


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 16, 64))
@pytest.mark.parametrize("n", BOX_N)
def test_uniform_table_gives_the_box_draw_bit_for_bit(emu, n, B):
    """(a) every step of the inverse is exact with the table b / B, B a power of two: ALL columns equal pinn_sample_box's"""
    tab = CC.uniform_table(B)
    for (lo, hi), first, seed, stream in zip((WAVE_BOX, BOX_3D), FIRSTS, SEEDS, STREAMS):
        assert np.array_equal(bits(draw_cdf(emu, seed, stream, first, n, lo, hi, tab)), bits(draw(emu, seed, stream, first, n, lo, hi))), (n, B, first)


@pytest.mark.parametrize("case", ["wave", "3d"])
def test_general_table_space_bits_bins_and_time_bound(emu, case):
    """(b) the space columns stay pinn_sample_box's bits; (c) the bin of every point is the reference's; (d) t within 8 * 2^-24 * max(span,
    |lo|, |hi|) of the float64 evaluation of the same formulas and inside [float32(lo_t), float32(hi_t)]; (g) a window is the tail.
    The call returns t, not b.  On these ranges b is read back from t through one more rounding (the fma), so (c) is held here only for
    points farther than 1e-5 of a bin from an edge -- the 7-bin table has no other check of its bins.  The exact comparison of (c), every
    point, is test_bins_of_the_unit_draw_equal_the_reference_exactly: there t is bit-identical to the reference's for B = 16 and 64."""
    (lo, hi), first, seed, stream = {"wave": (WAVE_BOX, FIRSTS[1], SEEDS[0], 2), "3d": (BOX_3D, FIRSTS[0], SEEDS[1], 7)}[case]
    n, dim = 70001, len(lo)
    for tab in (CC.general_table(16), CC.general_table(7), CC.general_table(64)):
        B = tab.size - 1
        got = draw_cdf(emu, seed, stream, first, n, lo, hi, tab)
        assert np.array_equal(bits(got[:, :dim - 1]), bits(draw(emu, seed, stream, first, n, lo, hi)[:, :dim - 1]))
        P, b, t64 = CC.draw_reference(seed, stream, first, n, lo, hi, tab)
        t = got[:, dim - 1]
        width = (hi[-1] - lo[-1]) / B
        got_b = np.minimum(np.floor((t.astype(np.float64) - lo[-1]) / width), B - 1).astype(np.int64)
        inner = np.abs((t.astype(np.float64) - lo[-1]) / width - np.round((t.astype(np.float64) - lo[-1]) / width)) > 1e-5
        assert np.array_equal(got_b[inner], b[inner])                                             # (a point ON an edge belongs to either side)
        assert (np.abs(t.astype(np.float64) - t64) <= CC.t_bound(lo[-1], hi[-1])).all()
        assert (t >= np.float32(lo[-1])).all() and (t <= np.float32(hi[-1])).all()
        assert np.array_equal(bits(draw_cdf(emu, seed, stream, first + 100, n - 100, lo, hi, tab)), bits(got[100:]))
        assert np.array_equal(bits(draw_cdf(emu, seed, stream, first, n, lo, hi, tab)), bits(got))      # two calls: identical bytes


def test_bins_of_the_unit_draw_equal_the_reference_exactly(emu):
    """(c) on the unit time range with a power-of-two bin count t = (b + f) / B, f < 1 unless rounded up: floor(t B) is the device's bin, a
    comparison of the same fp32 numbers; (e) bins of zero width, the first and the last among them, are never drawn"""
    n = 70001
    for tab in (CC.general_table(16), CC.general_table(64)):
        B = tab.size - 1
        t = draw_cdf(emu, 7, 1, 0, n, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), tab)[:, 2]
        P, b, _ = CC.draw_reference(7, 1, 0, n, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), tab)
        assert np.array_equal(bits(t), bits(P[:, 2]))                                             # the fp32 formulas, bit for bit (the fma is exact here)
        f_one = t * np.float32(B) == (b + 1).astype(np.float32)                                   # f rounded to 1: the point sits on the upper edge
        assert np.array_equal(np.floor(t * np.float32(B)).astype(np.int64) - f_one, b) and f_one.mean() < 1e-3
    t = draw_cdf(emu, 7, 1, 0, n, (0.0, 0.0, 0.0), (1.0, 1.0, 6.0), CC.GAP_TABLE)[:, 2]
    _, b, _ = CC.draw_reference(7, 1, 0, n, (0.0, 0.0, 0.0), (1.0, 1.0, 6.0), CC.GAP_TABLE)
    assert set(np.unique(b)) == {1, 3, 4} and (t >= 1.0).all() and (t <= 5.0).all() and not ((t > 2.0) & (t < 3.0)).any()
    assert np.array_equal(np.minimum(np.floor(t), 4).astype(np.int64)[t != np.floor(t)], b[t != np.floor(t)])


def test_bin_shares_follow_the_table(emu):
    """(f) 65536 points: every bin's share within 5 binomial sigma of its width -- a bar the numpy reference sampler meets alone with this
    seed and table (test_causal_host.py checks that without a library)"""
    tab = CC.general_table(16)
    lo, hi = WAVE_BOX
    t = draw_cdf(emu, CC.SHARE_SEED, CC.SHARE_STREAM, 0, CC.SHARE_N, lo, hi, tab)[:, 2]
    b = CC.bin_rule(t, lo[2], hi[2], 16)
    sig, empty = CC.share_errors(b, tab)
    print("sigmas:", np.round(sig, 2))
    assert (sig <= 5.0).all() and (empty == 0).all()


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_their_codes_and_write_nothing(emu):
    L, C = emu.lib, ctypes
    n, B = 100, 16
    nb = emu.binned_sums_workspace_bytes(n, B)
    assert nb > 0 and nb % 256 == 0 and emu.binned_sums_workspace_bytes((1 << 31) - 1, B) == nb
    assert [emu.binned_sums_workspace_bytes(*a) for a in ((-1, B), (1 << 31, B), (n, 0), (n, 65))] == [0, 0, 0, 0]
    v, c = put(np.ones(n, dtype=np.float32)), put(np.linspace(0, 1, n, dtype=np.float32))
    ws, out = Guarded(nb), Guarded(16 * B, fill=0xFF)
    sums = lambda n_=n, v_=v.ptr, c_=c.ptr, lo=0.0, hi=1.0, b=B, o=out.ptr, w=ws.ptr, wb=nb: L.pinn_binned_sums(v_, c_, n_, lo, hi, b, o, w, wb, None)
    before = out.raw.copy()
    assert sums(-1) == -5 and sums(1 << 31) == -5 and sums(b=0) == -5 and sums(b=65) == -5
    assert sums(lo=1.0, hi=1.0) == -5 and sums(lo=2.0, hi=1.0) == -5 and sums(hi=float("inf")) == -5 and sums(lo=float("nan")) == -5
    assert sums(v_=None) == -1 and sums(c_=None) == -1 and sums(o=None) == -1 and sums(w=None) == -1
    assert sums(wb=nb - 1) == -4 and sums(w=ws.ptr + 16) == -4
    assert np.array_equal(before, out.raw)
    assert sums(0, v_=None, c_=None) == 0 and np.array_equal(out.view(np.float64), np.zeros(2 * B))    # n == 0: zeros
    assert sums() == 0 and out.view(np.float64)[B:].sum() == n and all(g.guards_intact() for g in (v, c, ws, out))

    s, w, cdf = put(CC.profile_case(B)), Guarded(8 * B, fill=0xFF), Guarded(4 * (B + 1), fill=0xFF)
    tab = lambda s_=s.ptr, b=B, eps=1.0, fl=0.0, w_=w.ptr, c_=cdf.ptr: L.pinn_causal_cdf(s_, b, eps, fl, w_, c_, None)
    before = (w.raw.copy(), cdf.raw.copy())
    assert tab(b=0) == -5 and tab(b=65) == -5 and tab(eps=-1.0) == -5 and tab(fl=-0.5) == -5
    assert tab(eps=float("inf")) == -5 and tab(eps=float("nan")) == -5 and tab(fl=float("inf")) == -5 and tab(fl=float("nan")) == -5
    assert tab(s_=None) == -1 and tab(w_=None) == -1 and tab(c_=None) == -1
    assert np.array_equal(before[0], w.raw) and np.array_equal(before[1], cdf.raw)
    assert tab() == 0 and w.guards_intact() and cdf.guards_intact()

    d4 = C.c_double * 4
    lo, hi = d4(0, 0, 0, 0), d4(1, 1, 1, 1)
    cols, t = [Guarded(4 * n, fill=0xFF) for _ in range(4)], put(CC.uniform_table(B))
    box = lambda n_=n, dim=3, x=cols[0].ptr, y=cols[1].ptr, z=None, t_=cols[3].ptr, lo_=lo, hi_=hi, tab_=t.ptr, b=B: L.pinn_sample_box_cdf(
        1, 0, 0, n_, dim, lo_, hi_, tab_, b, x, y, z, t_, None)
    before = [c_.raw.copy() for c_ in cols]
    assert box(-1) == -5 and box(1 << 31) == -5 and box(b=0) == -5 and box(b=65) == -5
    assert box(dim=2) == -2 and box(dim=5) == -2
    assert box(x=None) == -1 and box(y=None) == -1 and box(t_=None) == -1 and box(dim=4) == -1 and box(lo_=None) == -1 and box(hi_=None) == -1
    assert box(tab_=None) == -1 and box(0, tab_=None) == -1
    assert box(0) == 0 and box(0, x=None, y=None, t_=None) == 0                                  # n == 0: a valid no-op
    assert all(np.array_equal(b_, c_.raw) for b_, c_ in zip(before, cols))
    assert box() == 0 and box(dim=4, z=cols[2].ptr) == 0 and all(c_.guards_intact() for c_ in cols)
