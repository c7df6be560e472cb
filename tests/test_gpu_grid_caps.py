"""-m gpu: every capped-grid kernel outside the fused training step run PAST its cap, against the references (tests/_grid_cap_cases.py: the caps
are read from the sources, the sizes derived from them).  The chain forward heads through Host::forward with a second and a third tile per wave,
the same entry points in PINN_PREC_FP32 over more than two workspace passes, and pinn_binned_sums, pinn_field_error_sums and pinn_select_k with
index ranges of two and three tiles per workgroup, workgroups with one point and with none."""
import numpy as np
import pytest
import torch

from tests import _causal_cases as CC
from tests import _grid_cap_cases as GC
from tests import _refine_cases as RC
from tests import _refine_family_cases as FC
from tests import _variant_matrix as vm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = int(vm.SENTINEL)                    # a NaN payload no arithmetic produces: fills every output and the guard words behind it
SENTINEL64 = 0x7FF5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pinn_elastodynamics_amd.capi import PinnLib
    return PinnLib()


def engine():
    from tests.test_gpu_refine import engine as shared
    return shared([3, 32, 32, 7])


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)        # (a copy: the shared cases are read-only)


def bits(t):
    return t.view(torch.int32)


def poison(eng, name):
    """fill the engine's scratch workspace `name` (allocated by an earlier call) with 0xFF bytes -- NaN records, huge counts: a record that a
    workgroup with an empty range left unwritten is then read as such, not as the zero or the right value an earlier call left there"""
    eng.__dict__[name].fill_(0xFF)


# ---- the chain forward heads ------------------------------------------------------------------------------------------------------------------
_INPUTS = {}


def inputs(row):
    """(parameters, point columns, frozen streams or None) of the row's net and set on the device; the last set only is kept"""
    key = (row.family, row.hidden, row.n)
    if key not in _INPUTS:
        _INPUTS.clear()
        X, fr = GC.points(row), GC.frozen(row)
        _INPUTS[key] = (dev(GC.net(row)), [dev(X[:, k]) for k in range(X.shape[1])], None if fr is None else dev(fr))
    return _INPUTS[key]


def workspace(lib, row):
    """(buffer, pointer, bytes): the minimum workspace of the split modes (a forward head takes no panels), the one of an engine of
    max_points = 1 << 13 in PINN_PREC_FP32"""
    from pinn_elastodynamics_amd.hip_engine import aligned_buffer
    if row.prec == "fp32":
        nbytes = lib.workspace_bytes(row.layers, GC.FP32_MAX_POINTS, "fp32")
        assert nbytes == GC.fp32_workspace_bytes(row.layers), "pinn_workspace_bytes left the formula tests/_grid_cap_cases.py derives the passes from"
    else:
        nbytes = lib.min_workspace_bytes(row.layers, row.prec)
    return aligned_buffer(nbytes, DEV) + (nbytes,)


def call(lib, head, layers, prec, th, cols, fr, ws):
    """one forward head into a fresh output filled with the sentinel, guard words behind it -> the fp32 device tensor [rows, n]"""
    n, rows = cols[0].numel(), GC.HEADS[head][3]
    assert all(c.is_contiguous() and c.numel() == n for c in cols) and (fr is None or (fr.is_contiguous() and fr.numel() == 50 * n))
    buf = torch.full((rows * n + vm.GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    p, xs, out, tail = th.data_ptr(), [c.data_ptr() for c in cols], buf.data_ptr(), (prec, ws[1], ws[2])
    if head == "wave_fields":
        lib.wave2d_fields(p, layers, *xs, n, RC.LB, RC.UB, True, out, *tail)
    elif head == "wave_score":
        lib.wave2d_residual_score(p, layers, *xs, n, RC.LB, RC.UB, True, 2.5, 0.25, 1.0, True, RC.WEIGHTS, out, *tail)
    elif head == "wave_predict":
        lib.wave2d_predict(p, layers, *xs, n, RC.LB, RC.UB, True, out, *tail)
    elif head == "net_streams":
        lib.net_streams(p, layers, *xs, n, FC.PLATE_LB, FC.PLATE_UB, False, out, *tail)
    elif head == "plate_score":
        lib.plate2d_residual_score(p, layers, *xs, n, FC.PLATE_LB, FC.PLATE_UB, False, fr.data_ptr(), 20.0, 0.25, 1.0, FC.PLATE_WEIGHTS, out, *tail)
    elif head == "plate_predict":
        lib.plate2d_predict(p, layers, *xs, n, FC.PLATE_LB, FC.PLATE_UB, False, fr.data_ptr(), out, *tail)
    elif head == "nc3d_fields":
        lib.nc3d_fields(p, layers, *xs, n, FC.NC3D_LB, FC.NC3D_UB, True, out, *tail)
    else:
        lib.nc3d_residual_score(p, layers, *xs, n, FC.NC3D_LB, FC.NC3D_UB, True, 2.5, 0.25, 1.0, FC.NC3D_WEIGHTS, out, *tail)
    torch.cuda.synchronize()
    assert bool((buf[rows * n:] == SENTINEL).all()), f"{head}: write past the end of the [{rows}, {n}] output"
    return buf[:rows * n].view(torch.float32).view(rows, n)


def part(cols, fr, lo, hi):
    """the points lo..hi as a call of their own: fresh columns, the frozen streams sliced and made contiguous"""
    return [c[lo:hi].clone() for c in cols], None if fr is None else fr[..., lo:hi].contiguous()


@pytest.mark.parametrize("row", GC.SPLIT_ROWS + GC.FP32_ROWS, ids=str)
def test_forward_head_past_the_cap(lib, row):
    """One forward head at a size whose launch gives some waves a second (and, at the larger size, a third and a ragged) tile -- in
    PINN_PREC_FP32: more than two workspace passes.
      position   the output of the big call equals, BIT FOR BIT, the same call on the points [0, cap_points) and on [cap_points, n): no per-point
                 head does arithmetic across points, so a point's result cannot depend on the tile, trip or pass it is computed in
      oracle     float64 oracle on the first 64 points, the 64 on either side of cap_points, the last 64 and 1024 random ones, with the head's
                 existing metric and bar: relative L2 below _variant_matrix.BAR[prec] (fields, streams); at most 6 x the float32 oracle's own error
                 on the same points for (s, sqrt(s)) of the scores and for the value / strain blocks of predict (f16x3 and fp32, as the files that
                 own those bars run them; the one-MFMA bf16 line is held to the primary references below, as those files hold it)
      primary    score and predict at EVERY point against the float64 formulas on the fp32 output of the fields / streams call of the same mode at
                 the same n, within the per-point rounding bound of score_from_fields / *_from_streams / *_predict_from_*
      and        guard words behind every output, no unwritten (sentinel) value, two calls the same bits, the frozen streams unwritten, and in the
                 split modes no path counter moves."""
    th, cols, fr = inputs(row)
    ws = workspace(lib, row)
    n, (cap, _) = row.n, row.cap
    assert n > cap and (row.prec != "fp32" or n > 2 * cap)
    fr0 = None if fr is None else fr.clone()
    run = lambda head, c=cols, f=fr: call(lib, head, row.layers, row.prec, th, c, f, ws)
    lib.path_counts(reset=True)
    out, again = run(row.head), run(row.head)
    if row.prec != "fp32":                                             # (a PINN_PREC_FP32 fields / streams call counts, by its row of CALLS)
        assert not any(lib.path_counts().values()), lib.path_counts()
    assert bool(torch.isfinite(out).all()), f"{row}: {int((~torch.isfinite(out)).sum())} values not finite (unwritten ones are NaN)"
    assert torch.equal(bits(out), bits(again)), f"{row}: two calls differ"
    # position independence
    for lo, hi in ((0, cap), (cap, n)):
        alone = run(row.head, *part(cols, fr, lo, hi))
        same = bits(out[:, lo:hi]) == bits(alone)
        assert bool(same.all()), (f"{row}: points [{lo}, {hi}) differ from the same call on them alone at {int((~same).sum())} places, the first at point "
                                  f"{lo + int((~same).any(0).nonzero()[0])}")
    assert fr is None or torch.equal(bits(fr), bits(fr0)), "the frozen streams were written to"
    # float64 oracle on the subset
    if row.prec in GC.ORACLE_MODES or row.head in ("wave_fields", "net_streams", "nc3d_fields"):
        idx, ref, bars = GC.oracle_case(row)
        got = GC.metrics(row, out[:, dev(idx, np.int64)].cpu().numpy(), ref)
        print(f"{row}: oracle on {idx.size} points: " + ", ".join(f"{g:.3e} ({g / b:.3f} of the bar {b:.3e})" for g, b in zip(got, bars)))
        assert all(g <= b for g, b in zip(got, bars)) and (len(bars) > 1 or got[0] < bars[0]), (str(row), got, bars)
    # primary reference at every point
    if row.head in GC.FIELDS_OF:
        F = run(GC.FIELDS_OF[row.head]).cpu().numpy().reshape(-1, GC.NOUT[row.family], n)
        ref, bound = GC.primary(row, F, None if fr is None else GC.frozen(row))
        err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = float(np.nanmax(np.where(err > 0, err / bound, 0.0)))
        print(f"{row}: primary at {n} points: max |delta| / bound = {worst:.3f}")
        assert (err <= bound).all(), (str(row), int((err > bound).sum()), np.argwhere(err > bound)[:4].tolist())


# ---- pinn_binned_sums ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planted", (False, True), ids=("plain", "planted"))
@pytest.mark.parametrize("n_bins", GC.BINNED_BINS)
@pytest.mark.parametrize("n", GC.BINNED_N)
def test_binned_sums_past_the_cap(n, n_bins, planted):
    """512 workgroups with ranges of two and three 1024-tiles (at n = 524289 workgroup 256 holds one point, 257..511 none; planted: that point is a
    skipped one): counts exact, sums within the bound of test_binned_sums_against_fsum (n_b * 2^-52 * sum|v| of math.fsum), two calls the same bits"""
    eng = engine()
    value, coord = GC.binned_case(n, planted)
    v, c = dev(value), dev(coord)
    a = eng.binned_sums(v, c, CC.LO, CC.HI, n_bins)
    poison(eng, "_bins_ws")
    b = eng.binned_sums(v, c, CC.LO, CC.HI, n_bins)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    got = a.cpu().numpy()
    sums, counts, absum = GC.binned_reference(n, planted, n_bins)
    assert counts.sum() == n - (5 if not planted else 7 if n == GC.BINNED_CAP + 1 else 9)          # the skipped points of the case
    err = np.abs(got[0] - sums)
    print(f"binned n={n} bins={n_bins} {'planted' if planted else 'plain'}: max err / bound {np.max(err / np.maximum(counts * CC.EPS52 * absum, 1e-300)):.3f}")
    assert np.array_equal(got[1], counts) and (err <= counts * CC.EPS52 * absum).all()
    assert np.array_equal(v.cpu().numpy().view(np.uint32), value.view(np.uint32)) and np.array_equal(c.cpu().numpy().view(np.uint32), coord.view(np.uint32))


# ---- pinn_field_error_sums ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_rows", GC.ERR_CASES)
def test_field_error_sums_past_the_cap(n, n_rows):
    """1024 workgroups with ranges of two and three 256-tiles (at n = 262145 workgroup 512 holds one point, the ones behind none), 16 permuted rows
    of a 20-row pred and the 1-row case: the bound of test_field_error_sums_against_numpy, guard words behind [2, n_rows], two calls the same bits"""
    eng = engine()
    rows, pred, ref, want = GC.error_case(n, n_rows)
    p, r = dev(pred), dev(ref)
    bufs = [torch.full((2 * n_rows + 32,), SENTINEL64, dtype=torch.int64, device=DEV) for _ in range(2)]
    for buf in bufs:
        eng.field_error_sums(p, rows, r, out=buf[:2 * n_rows].view(torch.float64))
        poison(eng, "_err_ws")
    torch.cuda.synchronize()
    assert all(bool((buf[2 * n_rows:] == SENTINEL64).all()) for buf in bufs), "write past the end of the [2, n_rows] sums"
    assert torch.equal(bufs[0], bufs[1])
    got = bufs[0][:2 * n_rows].view(torch.float64).cpu().numpy().reshape(2, n_rows)
    rel = np.abs(got - want) / want
    print(f"error sums n={n} rows={n_rows}: largest relative difference {rel.max():.2e} (bound {(n + 2) * 2.0 ** -52:.2e}: {rel.max() / ((n + 2) * 2.0 ** -52):.3f} of it)")
    assert (rel <= (n + 2) * 2.0 ** -52).all()


# ---- pinn_select_k ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", GC.SELECT_KINDS)
@pytest.mark.parametrize("n", GC.SELECT_N)
def test_select_k_with_ties_past_the_cap(n, kind):
    """1024 workgroups with index ranges of two (n = 262145) and three (524545) 256-tiles, tie-heavy data: select_ks(n), the k whose `need` runs out
    in the second tile of workgroup 1's range, and n - 1, both directions, exactly select_reference"""
    eng = engine()
    score = RC.select_data(kind, n)
    sc = dev(score)
    eng.select_k(sc, 1)
    for largest in (True, False):
        for k in GC.select_ks(kind, n, largest):
            poison(eng, "_select_ws")
            got = eng.select_k(sc, k, largest).cpu().numpy()
            assert got.dtype == np.int32 and np.array_equal(got, RC.select_reference(score, k, largest)), (n, k, largest, kind)
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), score.view(np.uint32))
