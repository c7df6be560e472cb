"""CPU half of the grid-cap tests (tests/_grid_cap_cases.py): the sizes are held to the caps read from the sources, the oracle subsets of the GPU
half are shown not to be degenerate, and the kernels that the SIMT emulator runs past their cap in about 20 s or less are run there, on host arrays
framed by guard words: pinn_select_k (both sizes), pinn_field_error_sums (both sizes) and pinn_binned_sums (both sizes).  The chain heads at
these sizes are the GPU half's (tests/test_gpu_grid_caps.py)."""
import numpy as np
import pytest

from tests import _causal_cases as CC
from tests import _grid_cap_cases as GC
from tests import _refine_cases as RC
from tests._predict_cases import Guarded, put
from tests.test_emulated_refine import emu  # noqa: F401


# ---- the sizes --------------------------------------------------------------------------------------------------------------------------------
def test_sizes_exceed_the_caps_read_from_the_sources():
    """Every derived size exceeds its cap, and for today's constants the sizes are the numbers of the table this file was written to.  A change of
    Host::MAX_BLOCKS, NB_PREDICT, the rule of nb(), causal::MAX_BLOCKS / TILE, validate::MAX_BLOCKS, select::MAX_BLOCKS / THREADS or of the fp32
    workspace formula lands here: look at the sizes, then at the table."""
    assert GC.HOST_MAX_BLOCKS * GC.WAVES_PER_WORKGROUP == 8192
    one, two = GC.chain_cap(1), GC.chain_cap(2)
    assert one == (131072, 16) and two == (262144, 32)
    assert GC.sizes(*one) == (131073, 262161) and GC.sizes(*two) == (262145, 524321)
    assert (GC.nb(64, 4), GC.nb(64, 5), GC.nb(128, 4), GC.nb(32, 1), GC.nb(64, 3, predict=True), GC.nb(128, 3, predict=True)) == (2, 1, 1, 2, 1, 1)
    want = {"wave_fields-w64-f16x3": 262145, "wave_score-w64-f16x3": 262145, "wave_fields-w100-f16x3": 131073, "wave_score-w100-f16x3": 131073,
            "wave_predict-w64-f16x3": 131073, "wave_predict-w100-f16x3": 131073, "net_streams-w64-f16x3": 131073, "plate_score-w64-f16x3": 131073,
            "plate_predict-w64-f16x3": 131073, "nc3d_fields-w100-f16x3": 131073, "nc3d_score-w100-f16x3": 131073, "wave_fields-w64-bf16": 262145,
            "wave_score-w64-bf16": 262145, "wave_predict-w64-bf16": 131073}
    small = {f"{r.head}-w{r.hidden}-{r.prec}": r.n for r in GC.SPLIT_ROWS if not r.big}
    assert small == want
    assert {f"{r.head}-w{r.hidden}": r.n for r in GC.SPLIT_ROWS if r.big} == {"wave_fields-w64": 524321, "wave_score-w64": 524321, "net_streams-w64": 262161}
    for r in GC.SPLIT_ROWS:
        cap, tile = r.cap
        ntiles = -(-r.n // tile)
        assert r.n > cap and ntiles > GC.HOST_MAX_BLOCKS * GC.WAVES_PER_WORKGROUP, str(r)          # a second trip of `tile += nwaves`
        assert not r.big or (ntiles > 2 * GC.HOST_MAX_BLOCKS * GC.WAVES_PER_WORKGROUP and r.n % tile == 1), str(r)      # a third, and a ragged tile
    # PINN_PREC_FP32: more than two workspace passes of an engine of max_points = 1 << 13 at n = 70001, every head
    for r in GC.FP32_ROWS:
        mmax = r.cap[0]
        assert r.n == 70001 and mmax >= GC.FP32_MAX_POINTS and r.n > 2 * mmax, (str(r), mmax)
    assert GC.Row("net_streams", 64, "fp32").cap[0] == 8192 and GC.Row("wave_fields", 64, "fp32").cap[0] == 1936 * 8192 // 1552
    # the index-range kernels
    assert (GC.BINNED_CAP, GC.FIELD_ERR_CAP, GC.SELECT_CAP) == (524288, 262144, 262144)
    assert GC.BINNED_N == (524289, 2 * 524288 + 1025) and GC.FIELD_ERR_N == (262145, 2 * 262144 + 257) and GC.SELECT_N == GC.FIELD_ERR_N
    # ... and what the table says about the ranges: at cap_points + 1 the chunk is two tiles, one workgroup holds one point, the ones behind none
    assert GC.ranges(524289, GC.CAUSAL_MAX_BLOCKS, GC.CAUSAL_TILE) == (512, 2048) and 524289 - 256 * 2048 == 1
    assert GC.ranges(262145, GC.VALIDATE_MAX_BLOCKS, GC.VALIDATE_TILE) == (1024, 512) and 262145 - 512 * 512 == 1
    assert GC.ranges(70001, GC.CAUSAL_MAX_BLOCKS, GC.CAUSAL_TILE) == (69, 1024) and GC.ranges(70001, GC.SELECT_MAX_BLOCKS, GC.SELECT_TILE) == (274, 256)
    # ... and at 2 * cap_points + tile + 1 three
    assert GC.ranges(GC.BINNED_N[1], GC.CAUSAL_MAX_BLOCKS, GC.CAUSAL_TILE) == (512, 3 * GC.CAUSAL_TILE)
    assert GC.ranges(GC.SELECT_N[1], GC.SELECT_MAX_BLOCKS, GC.SELECT_TILE) == (1024, 3 * GC.SELECT_TILE)
    assert GC.ranges(GC.FIELD_ERR_N[1], GC.VALIDATE_MAX_BLOCKS, GC.VALIDATE_TILE) == (1024, 3 * GC.VALIDATE_TILE)


@pytest.mark.parametrize("kind", GC.SELECT_KINDS)
def test_tie_k_lands_in_the_second_tile_of_a_range(kind):
    """the extra k of the selection cases, by the reference alone: the last index taken among the threshold's equals lies in the second 256-tile of
    workgroup 1's range; for "equal" k = chunk + 300"""
    for n in GC.SELECT_N:
        _, chunk = GC.ranges(n, GC.SELECT_MAX_BLOCKS, GC.SELECT_TILE)
        for largest in (True, False):
            score = RC.select_data(kind, n)
            k = GC.tie_k(score, largest, n)
            assert kind != "equal" or k == chunk + 300
            got = RC.select_reference(score, k, largest)
            key = RC.keys_of(score)
            thr = key[got].min() if largest else key[got].max()
            assert got[key[got] == thr].max() == chunk + 299 and chunk + GC.SELECT_TILE <= chunk + 299 < chunk + 2 * GC.SELECT_TILE, (kind, n, k)
            if kind != "special":                       # (nearly distinct values there: the threshold has no further equal behind)
                assert (key == thr).sum() > (key[got] == thr).sum(), (kind, n, k)


SCORE_ROWS = [r for r in GC.SPLIT_ROWS + GC.FP32_ROWS if r.head.endswith("score") and r.prec in GC.ORACLE_MODES]


@pytest.mark.parametrize("row", SCORE_ROWS, ids=str)
def test_score_subsets_are_not_degenerate(row):
    """The bar of the scores is 6 x the float32 oracle's own error on the SAME subset of indices: that error must not be zero, and no single point
    may carry most of the subset's L2 norm (the degeneracy _refine_cases.collocation_set describes).  Seed 20 of _grid_cap_cases.subset passed for
    every row at the first try; a row that fails here gets another seed, said in that docstring."""
    idx, ref, bars = GC.oracle_case(row)
    assert idx.size >= 1024 + 64 and ref.shape == (1, idx.size) and (ref > 0).all()
    assert all(b > 0 for b in bars), (str(row), bars)
    share = float((ref ** 2).max() / (ref ** 2).sum())
    print(f"{row}: {idx.size} points, bars {bars[0]:.3e} / {bars[1]:.3e}, largest share of one point in |s|^2 {share:.3f}")
    assert share < 0.5


# ---- the emulator past the caps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", GC.SELECT_KINDS)
@pytest.mark.parametrize("n", GC.SELECT_N)
def test_select_k_with_ties_past_the_cap(emu, n, kind):
    """1024 workgroups with index ranges of two (n = 262145) and three (524545) 256-tiles, tie-heavy data: the k whose `need` runs out in the
    second tile of a range, and n - 1, both directions, exactly the reference; no byte outside the buffers changes.  (A call takes the emulator
    about 3 s at either size, so the ks of select_ks(n) are left to the GPU half.)"""
    score = RC.select_data(kind, n)
    sc, ws = put(score), Guarded(emu.select_workspace_bytes(n))
    for largest in (True, False):
        for k in sorted({GC.tie_k(score, largest, n), n - 1}):
            out = Guarded(4 * k, fill=0xFF)
            emu.select_k(sc.ptr, n, k, largest, out.ptr, ws.ptr, ws.nbytes)
            assert sc.guards_intact() and ws.guards_intact() and out.guards_intact(), "a guard word was overwritten"
            assert np.array_equal(out.view(np.int32), RC.select_reference(score, k, largest)), (n, k, largest, kind)
    assert np.array_equal(sc.view(np.uint32), score.view(np.uint32)), "the scores were written to"


@pytest.mark.parametrize("n,n_rows", GC.ERR_CASES)
def test_field_error_sums_past_the_cap(emu, n, n_rows):
    """1024 workgroups with ranges of two and three 256-tiles (at n = 262145 workgroup 512 holds one point, the ones behind none), 16 permuted rows
    of a 20-row pred and the 1-row case: the bound of test_field_error_sums_against_numpy, guard words behind [2, n_rows], two calls the same bytes"""
    rows, pred, ref, want = GC.error_case(n, n_rows)
    p, r, ws = put(pred), put(ref), Guarded(emu.field_error_workspace_bytes(n, n_rows), fill=0xFF)      # (NaN records: see binned())
    outs = [Guarded(16 * n_rows, fill=0xFF) for _ in range(2)]
    for o in outs:
        emu.field_error_sums(p.ptr, GC.ERR_PRED_ROWS, rows, r.ptr, n, o.ptr, ws.ptr, ws.nbytes)
    assert all(g.guards_intact() for g in [p, r, ws] + outs), "a guard word was overwritten"
    got = outs[0].view(np.float64).reshape(2, n_rows)
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
    rel = np.abs(got - want) / want
    print(f"error sums n={n} rows={n_rows}: largest relative difference {rel.max():.2e} (bound {(n + 2) * 2.0 ** -52:.2e})")
    assert (rel <= (n + 2) * 2.0 ** -52).all()


def binned(emu, value, coord, lo, hi, n_bins):
    """pinn_binned_sums on guarded copies -> float64 [2, n_bins], as test_emulated_causal.binned -- but the workspace is filled with 0xFF bytes, NaN
    records: a record that a workgroup with an empty range left unwritten then shows in the sums (the guard byte 0xA5 makes doubles of 1e-130,
    which no bound would notice)"""
    n = value.size
    v, c = put(value), put(coord)
    ws, out = Guarded(emu.binned_sums_workspace_bytes(n, n_bins), fill=0xFF), Guarded(16 * n_bins, fill=0xFF)
    emu.binned_sums(v.ptr, c.ptr, n, lo, hi, n_bins, out.ptr, ws.ptr, ws.nbytes)
    assert all(g.guards_intact() for g in (v, c, ws, out)), "a guard word was overwritten"
    assert np.array_equal(v.view(np.uint32), value.view(np.uint32)) and np.array_equal(c.view(np.uint32), coord.view(np.uint32)), "an input was written to"
    return out.view(np.float64).copy().reshape(2, n_bins)


@pytest.mark.parametrize("planted", (False, True), ids=("plain", "planted"))
@pytest.mark.parametrize("n_bins", GC.BINNED_BINS)
@pytest.mark.parametrize("n", GC.BINNED_N)
def test_binned_sums_past_the_cap(emu, n, n_bins, planted):
    """512 workgroups with ranges of two and three 1024-tiles (at n = 524289 workgroup 256 holds one point, 257..511 none): counts exact, sums within
    the bound of test_binned_sums_against_fsum, two calls the same bytes"""
    value, coord = GC.binned_case(n, planted)
    got = binned(emu, value, coord, CC.LO, CC.HI, n_bins)
    sums, counts, absum = GC.binned_reference(n, planted, n_bins)
    assert counts.sum() == n - (5 if not planted else 7 if n == GC.BINNED_CAP + 1 else 9)          # the skipped points of the case
    assert np.array_equal(got[1], counts), (n, n_bins)
    err = np.abs(got[0] - sums)
    print(f"n={n} bins={n_bins}: max err / bound {np.max(err / np.maximum(counts * CC.EPS52 * absum, 1e-300)):.3f}")
    assert (err <= counts * CC.EPS52 * absum).all(), (n, n_bins)
    assert np.array_equal(got, binned(emu, value, coord, CC.LO, CC.HI, n_bins))
