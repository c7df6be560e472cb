"""CPU tests of pinn_sample_box and pinn_refine_keys: the kernel sources compiled for x86 against the SIMT emulator, on host arrays framed by guard
words that are checked after every call (as in test_emulated_refine.py).  The references are in tests/_sample_cases.py: Philox4x32-10 in numpy
(pinned by the published known-answer vectors), the box map, the fp32 ball test and the sampling keys in float64 and float32."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _sample_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
BOX_N = (1, 63, 64, 65, 255, 257, 70001)
FIRSTS = (0, 2 ** 32 - 3)                              # the second crosses the 32-bit carry of the counter
SEEDS = (1111, 0x1234567890ABCDEF)
STREAMS = (0, 7)


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pinn_elastodynamics_amd", "csrc"), "-j", str(min(16, os.cpu_count() or 1)), "emu"],
                   check=True, stdout=subprocess.DEVNULL)
    from pinn_elastodynamics_amd.capi import PinnLib
    return PinnLib(os.path.join(ROOT, "build", "emu", "libpinn_emu.so"))


class Guarded:
    """nbytes of payload at a 256-byte aligned address, guard words in front and behind"""

    def __init__(self, nbytes, fill=0xA5):
        self.raw = np.full(nbytes + 2 * GUARD + 512, 0xA5, dtype=np.uint8)
        base = self.raw.ctypes.data
        self.off = (-(base + GUARD) % 256) + GUARD
        self.nbytes = nbytes
        self.ptr = base + self.off
        self.raw[self.off:self.off + nbytes] = fill

    def view(self, dtype):
        return self.raw[self.off:self.off + self.nbytes].view(dtype)

    def guards_intact(self):
        return bool((self.raw[:self.off] == 0xA5).all() and (self.raw[self.off + self.nbytes:] == 0xA5).all())


def put(a):
    g = Guarded(a.nbytes)
    g.view(a.dtype)[:] = a.reshape(-1)
    return g


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def draw(emu, seed, stream, first, n, lo, hi):
    """pinn_sample_box into guarded buffers -> float32 [n, dim]"""
    cols = [Guarded(4 * n, fill=0xFF) for _ in lo]
    emu.sample_box(seed, stream, first, n, lo, hi, [c.ptr for c in cols])
    assert all(c.guards_intact() for c in cols), "a guard word was overwritten"
    return np.stack([c.view(np.float32).copy() for c in cols], axis=1)


def make_keys(emu, score, cols, balls, mode, power=1.0, c=1.0, seed=0, stream=0, first=0):
    """pinn_refine_keys on guarded copies -> float32 [n]; guards intact, inputs unwritten"""
    from pinn_elastodynamics_amd.capi import Ball
    n = score.size
    sc, xs = put(score), [put(a) for a in cols]
    ws, out = Guarded(emu.refine_keys_workspace_bytes(n)), Guarded(4 * n, fill=0xFF)
    bs = [Ball((ctypes.c_double * 3)(*ce), r, nd, keep) for ce, r, nd, keep in balls]
    z = xs[2].ptr if len(xs) > 2 else None
    emu.refine_keys(sc.ptr, n, xs[0].ptr if xs else None, xs[1].ptr if xs else None, z, bs, mode, power, c, seed, stream, first, out.ptr, ws.ptr,
                    ws.nbytes)
    assert all(g.guards_intact() for g in [sc, ws, out] + xs), "a guard word was overwritten"
    assert np.array_equal(sc.view(np.uint32), bits(score)) and all(np.array_equal(g.view(np.uint32), bits(a)) for g, a in zip(xs, cols)), "an input was written to"
    return out.view(np.float32).copy()


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def test_reference_reproduces_the_published_philox_vectors():
    """pins the numpy reference (not the code under test) to the known-answer vectors of Philox4x32-10"""
    for counter, key, want in SC.KAT:
        assert tuple(int(v[0]) for v in SC.philox4x32_10(counter, key)) == want


@pytest.mark.parametrize("dim", [3, 4])
@pytest.mark.parametrize("n", BOX_N)
def test_unit_box_equals_the_reference_bit_for_bit(emu, n, dim):
    lo, hi = [0.0] * dim, [1.0] * dim
    for first in FIRSTS:
        for seed, stream in zip(SEEDS, STREAMS):
            got = draw(emu, seed, stream, first, n, lo, hi)
            assert np.array_equal(bits(got), bits(SC.unit_box(seed, stream, first, n, dim))), (n, dim, first, seed)
            assert got.min() >= 0.0 and got.max() < 1.0
            if n > 100:                              # a window of the same stream is the tail of the longer call
                assert np.array_equal(bits(draw(emu, seed, stream, first + 100, n - 100, lo, hi)), bits(got[100:]))
    a, b = draw(emu, SEEDS[0], 0, 0, n, lo, hi), draw(emu, SEEDS[0], 1, 0, n, lo, hi)
    assert not np.array_equal(a, b)                  # another stream: other points


BOXES = {"wave": ((0.0, 0.0, 0.0), (30.0, 30.0, 20.0)), "plate": ((0.0, 0.0, 0.0), (0.5, 0.5, 10.0)),
         "wave-shifted": ((-15.0, -15.0, 0.0), (15.0, 15.0, 20.0)), "plate-shifted": ((-15.0, -15.0, 0.0), (-14.5, -14.5, 10.0)),
         "3d": ((-15.0, -15.0, -15.0, 0.0), (15.0, 15.0, 15.0, 14.0))}


@pytest.mark.parametrize("box", sorted(BOXES))
def test_general_box_within_one_ulp_and_inside(emu, box):
    """each value within 1 ulp (fp32) of lo + u (hi - lo) evaluated in float64 -- the kernel's fma rounds once, the 1 ulp covers the second
    rounding of the float64 reference to fp32 -- and inside [float32(lo), float32(hi)]"""
    lo, hi = BOXES[box]
    n = 70001
    got = draw(emu, 1111, 2, 2 ** 32 - 3, n, lo, hi)
    ref = SC.box64(1111, 2, 2 ** 32 - 3, n, lo, hi)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - ref) <= ulp).all()
    assert (got >= np.asarray(lo, dtype=np.float32)).all() and (got <= np.asarray(hi, dtype=np.float32)).all()
    assert (np.abs(got.mean(axis=0) - (np.asarray(lo) + np.asarray(hi)) / 2) < 0.01 * (np.asarray(hi) - np.asarray(lo))).all()


# ---- mask mode ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("n", SC.SIZES)
def test_mask_keys_are_the_scores_outside_the_balls(emu, n, keep):
    for name, dim, balls in SC.ball_cases(keep):
        P = SC.mask_points(dim)[:n]
        cols = [np.ascontiguousarray(P[:, k]) for k in range(dim - 1)]          # x, y, (z): the time column plays no part
        assert SC.boundary_margin(cols, balls) > 1e-6, "a reference point too close to a boundary: a condition on the inputs"
        score = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        score[n // 3] = np.nan
        inside = SC.in_balls(cols, balls)
        got = make_keys(emu, score, cols, balls, "mask")
        want = np.where(inside, np.float32(-np.inf), score)
        assert np.array_equal(bits(got), bits(want)), (name, n)
        if n >= 255:
            assert 0.4 < inside.mean() < 0.65
    score = np.arange(n, dtype=np.float32)
    assert np.array_equal(bits(make_keys(emu, score, [], [], "mask")), bits(score))       # no balls: no columns needed


def test_mask_boundary_conventions_on_exact_points(emu):
    """points exactly ON a boundary (coordinates and radius exact in fp32): kept with keep_boundary = 1, excluded with 0"""
    x = np.array([0.75, 0.5, 0.5, 0.8, 0.5, 0.5], dtype=np.float32)
    y = np.array([0.5, 0.25, 0.5, 0.5, 0.5, 0.5], dtype=np.float32)
    z = np.array([0.0, 0.0, 0.0, 0.0, 0.25, 0.125], dtype=np.float32)
    score = np.arange(1, 7, dtype=np.float32)
    ninf = -np.inf
    for nd, on, inner in ((2, [0, 1], [2, 4, 5]), (3, [0, 1, 4], [2, 5])):
        for keep in (0, 1):
            got = make_keys(emu, score, [x, y, z], [((0.5, 0.5, 0.0), 0.25, nd, keep)], "mask")
            want = score.copy()
            want[inner] = ninf
            if not keep:
                want[on] = ninf
            assert np.array_equal(got, want), (nd, keep, got)


# ---- sample mode --------------------------------------------------------------------------------------------------------------------------
def sample_case(n):
    name, dim, balls = SC.ball_cases(0)[1]
    P = SC.mask_points(dim)[:n]
    cols = [np.ascontiguousarray(P[:, k]) for k in range(3)]
    return cols, balls, SC.sample_scores(n), SC.noise_u(SC.KEY_SEED, SC.KEY_STREAM, SC.KEY_FIRST, n)


@pytest.mark.parametrize("power,c", SC.POWER_C)
@pytest.mark.parametrize("n", SC.SIZES)
def test_sample_keys_against_the_float64_reference(emu, n, power, c):
    """The -inf set is exactly the reference's (balls, invalid scores, p == 0); every other key is within delta of the float64 reference formed
    from the same u and the same fp32 scores, delta <= 4 x delta_ref, delta_ref the error of the same formula in numpy float32: three chained
    library transcendentals (powf, logf, logf) at a few ulp each here, at most 1 ulp each in numpy, and the final add.  Measured ratios:
    profiles/refine_sampling.txt."""
    cols, balls, score, u = sample_case(n)
    got = make_keys(emu, score, cols, balls, "sample", power, c, SC.KEY_SEED, SC.KEY_STREAM, SC.KEY_FIRST)
    d, d_ref, same = SC.key_errors(got, score, SC.in_balls(cols, balls), power, c, u)
    print(f"n={n} power={power} c={c}: delta {d:.3e}, delta_ref {d_ref:.3e}, ratio {d / d_ref if d_ref else 0.0:.2f}")
    assert same, "the excluded set differs from the reference's"
    assert not np.isnan(got).any() and d <= 4.0 * d_ref


def test_sample_keys_of_all_zero_scores(emu):
    n = 257
    z = np.zeros(n, dtype=np.float32)
    u = SC.noise_u(5, 1, 9, n)
    assert np.isneginf(make_keys(emu, z, [], [], "sample", 1.0, 0.0, 5, 1, 9)).all()                 # c = 0: nothing can be drawn
    got = make_keys(emu, z, [], [], "sample", 1.0, 1.0, 5, 1, 9)                                       # c = 1: the Gumbel term alone
    gumbel = -np.log(-np.log(u.astype(np.float64)))
    assert np.abs(got - gumbel).max() <= 4 * np.abs((-np.log(-np.log(u))).astype(np.float64) - gumbel).max()


def test_sample_then_select_is_a_weighted_draw(emu):
    """n = 65536, K = 1024, score 1 at even and 3 at odd indices, p ~ score: pinn_select_k on the produced keys"""
    n, K = 65536, 1024
    score = np.where(np.arange(n) % 2 == 1, 3.0, 1.0).astype(np.float32)
    u = SC.noise_u(1111, 0, 0, n)
    keys = make_keys(emu, score, [], [], "sample", 1.0, 0.0, 1111, 0, 0)
    sc, ws, out = put(keys), Guarded(emu.select_workspace_bytes(n)), Guarded(4 * K, fill=0xFF)
    emu.select_k(sc.ptr, n, K, True, out.ptr, ws.ptr, ws.nbytes)
    assert sc.guards_intact() and ws.guards_intact() and out.guards_intact()
    sel = out.view(np.int32).astype(np.int64)
    assert sel.size == K and (np.diff(sel) > 0).all() and sel[0] >= 0 and sel[-1] < n
    assert np.array_equal(sel, np.sort(np.argsort(-keys, kind="stable")[:K]))
    no_ball = np.zeros(n, dtype=bool)
    k64, _ = SC.keys_reference(score, no_ball, 1.0, 0.0, u, np.float64)
    d, d_ref, same = SC.key_errors(keys, score, no_ball, 1.0, 0.0, u)
    delta = 4.0 * d_ref                                      # the bar of the key test
    assert same and d <= delta
    order = np.sort(k64)[::-1]
    thr = order[K - 1]
    chosen = np.zeros(n, dtype=bool)
    chosen[sel] = True
    assert (k64[sel] >= thr - delta).all() and chosen[k64 > thr + delta].all()
    share = float((sel % 2 == 1).mean())
    print(f"odd share {share:.3f}; reference gap K / K+1: {order[K - 1] - order[K]:.2e}; delta {delta:.2e}")
    assert abs(share - 0.75) <= 0.07                         # 5 sigma of a binomial with K = 1024


# ---- arguments, determinism ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_their_codes_and_write_nothing(emu):
    from pinn_elastodynamics_amd.capi import Ball
    L, C = emu.lib, ctypes
    n = 100
    d4 = C.c_double * 4
    lo, hi = d4(0, 0, 0, 0), d4(1, 1, 1, 1)
    cols = [Guarded(4 * n, fill=0xFF) for _ in range(4)]
    box = lambda n_=n, dim=3, x=cols[0].ptr, y=cols[1].ptr, z=None, t=cols[3].ptr, lo_=lo, hi_=hi: L.pinn_sample_box(1, 0, 0, n_, dim, lo_, hi_, x, y, z, t, None)
    before = [c.raw.copy() for c in cols]
    assert box(-1) == -5 and box(1 << 31) == -5
    assert box(dim=2) == -2 and box(dim=5) == -2
    assert box(x=None) == -1 and box(y=None) == -1 and box(t=None) == -1 and box(dim=4) == -1 and box(lo_=None) == -1 and box(hi_=None) == -1
    assert box(0) == 0 and box(0, x=None, y=None, t=None) == 0                       # n == 0: a valid no-op
    assert all(np.array_equal(b, c.raw) for b, c in zip(before, cols))
    assert box() == 0 and box(dim=4, z=cols[2].ptr) == 0 and all(c.guards_intact() for c in cols)

    nb = emu.refine_keys_workspace_bytes(n)
    assert nb > 0 and nb % 256 == 0 and emu.refine_keys_workspace_bytes(-1) == 0 and emu.refine_keys_workspace_bytes(1 << 31) == 0
    assert emu.refine_keys_workspace_bytes((1 << 31) - 1) == nb
    sc, ws, out = put(np.ones(n, dtype=np.float32)), Guarded(nb), Guarded(4 * n, fill=0xFF)
    xs = [put(np.full(n, 0.5, dtype=np.float32)) for _ in range(3)]
    disc = (Ball * 4)(*[Ball((C.c_double * 3)(0.5, 0.5, 0.5), 0.1, 2, 0)] * 4)
    ball = (Ball * 1)(Ball((C.c_double * 3)(0.5, 0.5, 0.5), 0.1, 3, 0))
    odd = (Ball * 1)(Ball((C.c_double * 3)(0.5, 0.5, 0.5), 0.1, 1, 0))
    keys = lambda n_=n, s=sc.ptr, x=xs[0].ptr, y=xs[1].ptr, z=xs[2].ptr, b=disc, nb_=1, mode=0, o=out.ptr, w=ws.ptr, wb=nb: L.pinn_refine_keys(
        s, n_, x, y, z, b, nb_, mode, 1.0, 1.0, 1, 0, 0, o, w, wb, None)
    before = out.raw.copy()
    assert keys(-1) == -5 and keys(1 << 31) == -5 and keys(nb_=-1) == -5 and keys(nb_=5) == -5 and keys(b=odd) == -5
    assert keys(mode=2) == -3 and keys(mode=-1) == -3
    assert keys(s=None) == -1 and keys(o=None) == -1 and keys(w=None) == -1 and keys(x=None) == -1 and keys(y=None) == -1
    assert keys(b=None) == -1 and keys(b=ball, z=None) == -1
    assert keys(wb=nb - 1) == -4 and keys(w=ws.ptr + 16) == -4
    for mode in (0, 1):
        assert keys(0, mode=mode) == 0 and keys(0, mode=mode, s=None, o=None, x=None, y=None, z=None) == 0          # n == 0: a valid no-op
    assert np.array_equal(before, out.raw)
    assert keys(nb_=0, x=None, y=None, z=None, b=None) == 0 and np.array_equal(out.view(np.float32), np.ones(n, dtype=np.float32))
    assert keys(z=None) == 0 and keys(nb_=4) == 0 and np.isneginf(out.view(np.float32)).all()           # a disc needs no z
    assert all(g.guards_intact() for g in [sc, ws, out] + xs)


def test_two_calls_give_identical_bytes(emu):
    n = 70001
    lo, hi = BOXES["3d"]
    a, b = draw(emu, 99, 4, 12345, n, lo, hi), draw(emu, 99, 4, 12345, n, lo, hi)
    assert np.array_equal(bits(a), bits(b))
    cols, balls, score, _ = sample_case(n)
    for mode in ("mask", "sample"):
        k1, k2 = (make_keys(emu, score, cols, balls, mode, 2.0, 0.1, 8, 2, 40) for _ in range(2))
        assert np.array_equal(bits(k1), bits(k2)), mode
