"""-m gpu: causal sampling on the device -- HipEngine.binned_sums / causal_cdf / sample_box(t_cdf=...) against the numpy references of
tests/_causal_cases.py (the bounds of the emulator tests), then DeepHPM.resample_collocation and train(causal=...) on a 4x32 net."""
import numpy as np
import pytest

from tests import _causal_cases as CC
from tests import _refine_cases as RC

pytestmark = pytest.mark.gpu
DISC = (15.0, 15.0, 2.0)                                  # the source disc of the infinite case
BOX_3D = ((-15.0, -15.0, -15.0, 2.0), (15.0, 15.0, 15.0, 14.0))


def engine():
    from tests.test_gpu_refine import engine as shared
    return shared([3, 32, 32, 7])


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host(cols):
    return np.stack([c.cpu().numpy() for c in cols], axis=1)


# ---- the three calls against the numpy references -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", (7, 64))
@pytest.mark.parametrize("n", (257, 70001))
def test_binned_sums_against_fsum(n, n_bins):
    """the bar of the emulator test of the same name: counts exact, sums within n_b * 2^-52 * sum|v| of math.fsum; two calls the same bytes"""
    import torch
    eng = engine()
    value, coord = CC.sums_case(n)
    v, c = dev(value), dev(coord)
    a, b = (eng.binned_sums(v, c, CC.LO, CC.HI, n_bins) for _ in range(2))
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    got = a.cpu().numpy()
    sums, counts, absum = CC.binned_reference(value, coord, CC.LO, CC.HI, n_bins)
    err = np.abs(got[0] - sums)
    print(f"n={n} bins={n_bins}: max err / bound {np.max(err / np.maximum(counts * CC.EPS52 * absum, 1e-300)):.3f}")
    assert np.array_equal(got[1], counts) and (err <= counts * CC.EPS52 * absum).all()
    assert np.array_equal(bits(v.cpu().numpy()), bits(value)) and np.array_equal(bits(c.cpu().numpy()), bits(coord))
    assert np.array_equal(eng.binned_sums(v[:0], c[:0], CC.LO, CC.HI, n_bins).cpu().numpy(), np.zeros((2, n_bins)))


@pytest.mark.parametrize("B", (7, 64))
def test_causal_cdf_against_float64(B):
    eng = engine()
    sums = CC.profile_case(B)
    for eps, floor in ((0.6, 0.0), (0.6, 0.01), (25.0, 0.0)):
        w, cdf = (t.cpu().numpy() for t in eng.causal_cdf(dev(sums, np.float64), eps, floor))
        m, c, w64, cdf64, cdf32 = CC.cdf_reference(sums, eps, floor)
        assert cdf[0] == 0.0 and cdf[B] == 1.0 and (np.diff(cdf) >= 0).all() and w[0] == 1.0
        rel = np.abs(w - w64) / np.maximum(w64, 1e-300)
        assert (rel[w64 > 0] <= CC.w_bound(B, eps, c)[w64 > 0]).all() and (w[w64 == 0] <= 1e-300).all(), (B, eps, rel.max())
        ulp = np.spacing(np.abs(cdf64).astype(np.float32)).astype(np.float64)
        assert (np.abs(cdf.astype(np.float64) - cdf64.astype(np.float32)) <= ulp).all()
    for eps, floor in ((2.0, 1.0), (0.0, 0.0)):
        if B == 64:                                                                               # the uniform table, exact for a power of two
            assert np.array_equal(bits(eng.causal_cdf(dev(sums, np.float64), eps, floor)[1].cpu().numpy()), bits(CC.uniform_table(B)))


@pytest.mark.parametrize("n", (257, 70001))
def test_uniform_table_gives_the_box_draw_bit_for_bit(n):
    """(a) with the table b / B, B in (1, 16, 64), all columns equal sample_box's, across the 32-bit carry of the counter too"""
    eng = engine()
    for (lo, hi), first, seed, stream in (((RC.LB, RC.UB), 0, 1111, 0), (BOX_3D, 2 ** 32 - 3, 0x1234567890ABCDEF, 7)):
        want = host(eng.sample_box(n, lo, hi, seed, stream, first))
        for B in (1, 16, 64):
            got = host(eng.sample_box(n, lo, hi, seed, stream, first, t_cdf=dev(CC.uniform_table(B))))
            assert np.array_equal(bits(got), bits(want)), (n, B, first)


@pytest.mark.parametrize("n", (257, 70001))
def test_general_table_space_bits_bins_and_time_bound(n):
    """(b) the space columns keep sample_box's bits, (c) on the unit time range the bins are the reference's exactly, (d) t within
    8 * 2^-24 * max(span, |lo|, |hi|) of the float64 evaluation and inside the box; a window is the tail of the longer call"""
    eng = engine()
    for B in (16, 7, 64):
        tab = CC.general_table(B)
        td = dev(tab)
        for (lo, hi), first, seed, stream in (((RC.LB, RC.UB), 2 ** 32 - 3, 1111, 2), (BOX_3D, 0, 0x1234567890ABCDEF, 7)):
            dim = len(lo)
            got = host(eng.sample_box(n, lo, hi, seed, stream, first, t_cdf=td))
            assert np.array_equal(bits(got[:, :dim - 1]), bits(host(eng.sample_box(n, lo, hi, seed, stream, first))[:, :dim - 1]))
            _, _, t64 = CC.draw_reference(seed, stream, first, n, lo, hi, tab)
            t = got[:, dim - 1]
            assert (np.abs(t.astype(np.float64) - t64) <= CC.t_bound(lo[-1], hi[-1])).all()
            assert (t >= np.float32(lo[-1])).all() and (t <= np.float32(hi[-1])).all()
            assert np.array_equal(bits(host(eng.sample_box(n - 100, lo, hi, seed, stream, first + 100, t_cdf=td))), bits(got[100:]))
        if B != 7:
            unit = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
            t = host(eng.sample_box(n, *unit, 7, 1, 0, t_cdf=td))[:, 2]
            P, b, _ = CC.draw_reference(7, 1, 0, n, *unit, tab)
            assert np.array_equal(bits(t), bits(P[:, 2]))
            f_one = t * np.float32(B) == (b + 1).astype(np.float32)
            assert np.array_equal(np.floor(t * np.float32(B)).astype(np.int64) - f_one, b)


def test_bin_shares_follow_the_table():
    """(f) 65536 points: every bin's share within 5 binomial sigma of its width (the numpy sampler meets the bar alone: test_causal_host.py)"""
    eng = engine()
    tab = CC.general_table(16)
    t = eng.sample_box(CC.SHARE_N, RC.LB, RC.UB, CC.SHARE_SEED, CC.SHARE_STREAM, 0, t_cdf=dev(tab))[2].cpu().numpy()
    sig, empty = CC.share_errors(CC.bin_rule(t, RC.LB[2], RC.UB[2], 16), tab)
    print("sigmas:", np.round(sig, 2))
    assert (sig <= 5.0).all() and (empty == 0).all()


def test_errors_carry_their_codes():
    from pinn_elastodynamics_amd.capi import PinnLibError
    eng = engine()
    v = dev(np.ones(10))
    with pytest.raises(PinnLibError, match="code -5"):
        eng.binned_sums(v, v, 0.0, 1.0, 65)
    with pytest.raises(PinnLibError, match="code -5"):
        eng.binned_sums(v, v, 1.0, 1.0, 4)
    with pytest.raises(PinnLibError, match="code -5"):
        eng.causal_cdf(dev(np.ones((2, 4)), np.float64), -1.0)
    with pytest.raises(PinnLibError, match="code -5"):
        eng.sample_box(10, RC.LB, RC.UB, 1, t_cdf=dev(np.linspace(0, 1, 66)))


# ---- DeepHPM ------------------------------------------------------------------------------------------------------------------------------------
def wave_model():
    from tests.test_gpu_refine import model
    return model([3] + 4 * [32] + [7], n_rows=2000)


# floor = 0.05: every bin keeps a share of at least floor / 16 = 0.3 % of the 2000 rows whatever the profile (max(w, floor) <= 1 in 16 bins), an
# expected count of 6 or more, for which 5 binomial sigma is still a tail of 1e-5; without a floor the late bins would hold about e^-15 of
# the rows and a single row there would stand 40 "sigma" out
CAUSAL = dict(bins=16, eps=1.0, candidates=8192, exclude=[DISC], seed=42, floor=0.05)


def test_resample_collocation_redraws_the_set_from_its_table():
    """fresh 4x32 net, 2000 rows, 8192 probe points, the source disc excluded: the set keeps its size, no new row lies in the disc or outside
    the box, the rows' time-bin shares are within 5 sigma of the returned table, the device rows and the host columns agree, and a second
    model built the same way returns the same bytes"""
    outs = []
    for _ in range(2):
        m, Collo = wave_model()
        out = m.resample_collocation(CAUSAL)
        assert out["redrawn"] == 2000 and out["kept"] == 0 and m._n_collo == 2000 and m._shard(0, 2000) == (0, 2000)
        got = host(m._collo)
        assert got.shape == (2000, 3) and np.array_equal(got, np.concatenate([m.x_c, m.y_c, m.t_c], axis=1).astype(np.float32))
        assert np.array_equal(got, np.stack(m._collo_host, axis=1))
        assert ((got[:, 0] - DISC[0]) ** 2 + (got[:, 1] - DISC[1]) ** 2 > DISC[2] ** 2).all()
        assert (got >= np.asarray(RC.LB, dtype=np.float32)).all() and (got <= np.asarray(RC.UB, dtype=np.float32)).all()
        cdf, w = out["cdf"], out["w"]
        assert cdf.shape == (17,) and cdf[0] == 0 and cdf[16] == 1 and (np.diff(cdf) >= 0).all() and w[0] == 1.0 and (np.diff(w) <= 0).all()
        assert out["counts"].sum() < 8192 and out["counts"].sum() > 0.97 * 8192 and (out["profile"] >= 0).all()
        _, _, w64, _, cdf32 = CC.cdf_reference(np.stack([out["profile"] * out["counts"], out["counts"]]), 1.0 / m._causal_ref, 0.05)
        assert np.abs(cdf - cdf32).max() <= 4 * 2.0 ** -24                                         # (the profile came back as means: a rounding each)
        sig, empty = CC.share_errors(CC.bin_rule(got[:, 2], RC.LB[2], RC.UB[2], 16), cdf)
        print("sigmas:", np.round(sig, 2))
        assert (sig <= 5.0).all() and (empty == 0).all()
        assert np.isfinite(m.getloss()[0])
        outs.append((out, got))
    (a, ga), (b, gb) = outs
    assert ga.tobytes() == gb.tobytes() and all(a[k].tobytes() == b[k].tobytes() for k in ("w", "cdf", "profile", "counts"))


def test_train_with_causal_gives_finite_losses_and_composes_with_refinement():
    m, _ = wave_model()
    h = m.train(4, 1e-3, 1, causal=dict(every=2, bins=16, eps=1.0, candidates=8192))
    # a fresh model, ref="first": both triggers redraw -- steps 3 and 4 train on the rows drawn behind step 2
    assert np.isfinite(h[4]).all() and len(h[4]) == 4 and m._causal_cdf.shape == (17,) and m._refine_round == 2 and m._causal_ref > 0
    h = m.train(4, 1e-3, 1, causal=dict(every=2, bins=16, eps=1.0, candidates=8192, exclude=[DISC]),
                refine=dict(every=2, candidates=2048, n_replace=100, seed=3, exclude=[DISC], causal=True))
    assert np.isfinite(h[4]).all() and m._refine_round == 6 and m._n_collo == 2000
    got = host(m._collo)
    assert np.array_equal(got, np.stack(m._collo_host, axis=1)) and (got >= np.asarray(RC.LB, dtype=np.float32)).all()


def test_train_without_causal_is_bit_identical():
    """identical train calls on two fresh models, one with causal=None and one without the keyword: the same parameters bit for bit"""
    thetas = []
    for kw in ({}, {"causal": None}):
        m, _ = wave_model()
        m.train(3, 1e-3, 2, **kw)
        thetas.append(m.theta.cpu().numpy())
    assert thetas[0].tobytes() == thetas[1].tobytes() and np.isfinite(thetas[0]).all()
