"""-m gpu: residual-adaptive refinement on the device -- HipEngine.select_k against the numpy reference (exact), HipEngine.residual_score against the
library's own fields call (head rounding only) and against the float64 oracle, DeepHPM.refine_collocation end to end, and two data-parallel ranks
that each refine their shard.  Cases and references: tests/_refine_cases.py (the same as the emulator tests)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _refine_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
_ENGINES = {}


def engine(layers, prec="f16x3"):
    import torch
    from pinn_elastodynamics_amd.hip_engine import HipEngine
    key = (tuple(layers), prec)
    if key not in _ENGINES:
        _ENGINES[key] = HipEngine(list(layers), precision=prec, device=torch.device("cuda:0"), max_points=1 << 13)
    return _ENGINES[key]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


# ---- selection ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RC.SELECT_DATA)
@pytest.mark.parametrize("n", RC.SELECT_N)
def test_select_k_equals_the_numpy_reference(n, kind):
    """every k of {0, 1, n // 10, n - 1, n}, both directions, exact; n = 70001 runs 274 workgroups (index ranges of one tile), 5000 and 70001 the
    grid-stride loop of the histogram passes is one trip -- the 2 M case of the next test makes several"""
    eng = engine([3, 32, 32, 7])
    score = RC.select_data(kind, n)
    sc = dev(score)
    for k in RC.select_ks(n):
        for largest in (True, False):
            got = eng.select_k(sc, k, largest).cpu().numpy()
            assert got.dtype == np.int32 and np.array_equal(got, RC.select_reference(score, k, largest)), (n, k, largest, kind)
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), score.view(np.uint32))


def test_select_k_large_set_is_exact_and_reproducible():
    """2 000 003 scores of a heavy-tailed positive distribution with repeated values: 1024 workgroups, several trips of the grid-stride loop and
    several tiles per index range; two calls give the same bits"""
    import torch
    eng = engine([3, 32, 32, 7])
    rng = np.random.default_rng(12)
    score = (rng.integers(0, 1 << 20, 2_000_003).astype(np.float32) / 1024.0) ** 2
    sc = dev(score)
    for k, largest in ((200_000, True), (200_000, False), (1_999_999, True)):
        a, b = eng.select_k(sc, k, largest), eng.select_k(sc, k, largest)
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), RC.select_reference(score, k, largest))


def test_select_k_errors():
    from pinn_elastodynamics_amd.capi import PinnLibError
    eng = engine([3, 32, 32, 7])
    sc = dev(np.arange(10, dtype=np.float32))
    with pytest.raises(PinnLibError, match="code -5"):
        eng.select_k(sc, 11)
    assert eng.select_k(sc, 0).numel() == 0 and eng.select_k(sc, 3).tolist() == [7, 8, 9] and eng.select_k(sc, 3, largest=False).tolist() == [0, 1, 2]


# ---- score -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RC.PRIMARY_N)
@pytest.mark.parametrize("name,layers,prec", RC.PRIMARY_LINES, ids=[l[0] for l in RC.PRIMARY_LINES])
def test_score_equals_the_residuals_of_the_fields_call(name, layers, prec, n):
    """PRIMARY check (see the emulator test of the same name): float64 residual formulas on the fp32 output of fields in the same mode, bound
    16 eps32 sum_i w_i a_i^2 per point; the engine runs in the MINIMUM workspace."""
    import torch
    from pinn_elastodynamics_amd.hip_engine import HipEngine
    eng = HipEngine(layers, precision=prec, device=torch.device("cuda:0"), workspace_bytes=0)       # (raised to pinn_min_workspace_bytes)
    X = RC.points(n, seed=77)
    th, xs = dev(RC.fresh_net(tuple(layers))), [dev(X[:, k]) for k in range(3)]
    eng.lib.path_counts(reset=True)
    s = eng.residual_score(th, *xs, RC.LB, RC.UB, True, RC.WEIGHTS).cpu().numpy()
    assert not any(eng.lib.path_counts().values())
    F = eng.fields(th, *xs, RC.LB, RC.UB, True).cpu().numpy()
    ref, bound = RC.score_from_fields(F)
    err = np.abs(s.astype(np.float64) - ref)
    print(f"{name} n={n}: max |delta| / bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(s).all() and (err <= bound).all()


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("net", RC.SECONDARY_NETS)
def test_score_against_the_float64_oracle(net, prec):
    """SECONDARY check: relative L2 of s and sqrt(s) over 1000 collocation points against the float64 oracle, at most 6 x the float32 oracle's own"""
    layers, flat, X, ref, base = RC.secondary_case(net)
    eng = engine(layers, prec)
    s = eng.residual_score(dev(flat), *[dev(X[:, k]) for k in range(3)], RC.LB, RC.UB, True, RC.WEIGHTS).cpu().numpy()
    got = (RC.rel_l2(s, ref), RC.rel_l2(np.sqrt(s.astype(np.float64)), np.sqrt(ref)))
    print(f"{net} {prec}: s {got[0]:.3e} ({got[0] / base[0]:.2f} x fp32 oracle {base[0]:.3e}), sqrt(s) {got[1]:.3e} ({got[1] / base[1]:.2f} x {base[1]:.3e})")
    assert got[0] <= 6.0 * base[0] and got[1] <= 6.0 * base[1]


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def model(layers, n_rows=5000, flat=None, seed=9, **kw):
    from oracle import pinn_oracle as po
    from pinn_elastodynamics_amd.elastic_wave import DeepHPM, unpack_params
    Collo = RC.points(n_rows, seed=21)
    m = DeepHPM(Collo.copy(), po.ricker_source_set(n_pt=20, n_time=11), po.ic_grid(num=21), np.zeros((0, 3)), layers, RC.LB, RC.UB, case="infinite",
                engine=engine(layers), verbose=False, seed=seed, **kw)
    if flat is not None:
        m.set_weights(*unpack_params(np.asarray(flat, dtype=np.float32), layers))
    return m, Collo


def test_refine_collocation_applies_the_rule_exactly():
    """4x32 Xavier weights, 5000 rows, 5000 candidates, n_replace = 500: the rows afterwards are the rule of the issue's section 4 applied in numpy to
    the scores residual_score returns; untouched rows keep their bits, N stays, getloss and a training step run, the set's score sum did not fall"""
    layers = [3] + 4 * [32] + [7]
    m, Collo = model(layers)
    cand = RC.points(5000, seed=1111)
    s_rows = m.residual_score(m.x_c, m.y_c, m.t_c).reshape(-1)
    s_cand = m.residual_score(cand[:, 0:1], cand[:, 1:2], cand[:, 2:3]).reshape(-1)
    assert s_rows.dtype == np.float32 and s_rows.shape == (5000,)
    rows, cands = RC.refine_rule(s_rows, s_cand, 500)
    assert 0 < rows.size <= 500
    want = Collo.astype(np.float32).copy()
    want[rows] = cand[cands].astype(np.float32)
    out = m.refine_collocation(cand, 500)
    assert out["replaced"] == rows.size and np.array_equal(out["rows"], rows) and np.array_equal(out["candidate_indices"], cands)
    assert out["score_replaced_max"] == float(s_rows[rows].max()) and out["score_inserted_min"] == float(s_cand[cands].min())
    got = np.stack([a.cpu().numpy() for a in m._collo], axis=1)
    assert got.shape == (5000, 3) and m._n_collo == 5000 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    host = np.concatenate([m.x_c, m.y_c, m.t_c], axis=1)
    assert np.array_equal(host.astype(np.float32), want) and np.array_equal(np.stack(m._collo_host, axis=1), want)
    assert np.array_equal(Collo, RC.points(5000, seed=21)), "the caller's array was written to"
    after = m.residual_score(m.x_c, m.y_c, m.t_c).reshape(-1)
    assert float(after.astype(np.float64).sum()) >= float(s_rows.astype(np.float64).sum())
    assert np.isfinite(m.getloss()[0]) and np.isfinite(m.train(1, 1e-3, 1)[4]).all()
    # a second call with the same candidates finds them in the set already: whatever it replaces obeys the same rule
    s2 = m.residual_score(m.x_c, m.y_c, m.t_c).reshape(-1)
    r2, c2 = RC.refine_rule(s2, m.residual_score(cand[:, 0:1], cand[:, 1:2], cand[:, 2:3]).reshape(-1), 500)
    assert np.array_equal(m.refine_collocation(cand, 500)["rows"], r2)


@pytest.mark.parametrize("net", RC.SECONDARY_NETS)
def test_selected_candidates_against_the_oracles_own_top_500(net):
    """The device's top 500 of 5000 seed-1111 uniform candidates against the top 500 by float64 score: at most 2 % of K differ, and every index that
    differs has a float64 score within 1e-3 relative of the K-th score.  (How many candidates sit in that band by the float64 scores alone is
    printed: the issue counted 2-4 of 500 for these nets.)"""
    K = 500
    if net == "inf20s":
        layers, flat = RC.trained_net()
    else:
        layers = [3] + (4 * [32] if net == "xavier4x32" else 8 * [64]) + [7]
        flat = RC.fresh_net(tuple(layers))
    cand = RC.points(5000, seed=1111)
    w = [1.0] * 7                                   # LOSS_LAYOUT["infinite"]: what refine_collocation uses by default
    s64 = RC.oracle_score(flat, layers, cand, w=w)
    top64 = np.argsort(-s64, kind="stable")[:K]
    kth = s64[top64[-1]]
    eng = engine(layers)
    s = eng.residual_score(dev(flat), *[dev(cand[:, k]) for k in range(3)], RC.LB, RC.UB, True, w)
    got = eng.select_k(s, K).cpu().numpy()
    diff = np.setxor1d(got, top64)
    band = int((np.abs(s64 - kth) <= 1e-3 * kth).sum())
    print(f"{net}: {diff.size // 2} of {K} differ; {band} candidates within 1e-3 of the K-th float64 score")
    assert diff.size // 2 <= 0.02 * K
    assert (np.abs(s64[diff] - kth) <= 1e-3 * kth).all()


def test_two_ranks_refine_their_own_shards(tmp_path):
    """Two processes on one GPU (gloo for the collective, as test_gpu_dp.py): each rank refines its shard with its own candidates, then trains a
    step.  Parameters stay bit-identical across the ranks, a rank's replaced rows lie in its shard and obey the rule on its own scores, and the
    other rank's rows are what they were."""
    out = str(tmp_path / "dp_refine.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29541", os.path.join(ROOT, "tests", "_dp_worker_refine.py"), out], env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out)
    assert np.array_equal(z["theta0"], z["theta1"]) and np.isfinite(z["theta0"]).all()
    n = int(z["n"])
    base = RC.points(n, seed=21).astype(np.float32)
    for r_ in (0, 1):
        lo, hi = n * r_ // 2, n * (r_ + 1) // 2
        rows, host = z[f"rows{r_}"], z[f"host{r_}"]
        assert rows.size > 0 and rows.min() >= lo and rows.max() < hi
        want_rows, want_cands = RC.refine_rule(z[f"s_rows{r_}"], z[f"s_cand{r_}"], 200)
        assert np.array_equal(rows, want_rows + lo) and np.array_equal(z[f"cands{r_}"], want_cands)
        untouched = np.ones(n, dtype=bool)
        untouched[rows] = False
        assert np.array_equal(host[untouched], base[untouched])           # the other rank's rows included
        assert np.array_equal(z[f"shard{r_}"], host[lo:hi])               # what the rank holds on the device is its refined shard
