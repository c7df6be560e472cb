"""-m gpu: residual-adaptive refinement for the plate and 3-D families on the device -- HipEngine.plate_residual_score / nc3d_residual_score against
the library's own streams / fields call (head rounding only) and against the float64 oracle, the selection against the oracle's own top K,
PINN.refine_collocation and NavierCauchy3D.refine_collocation end to end, and two data-parallel ranks of a PINN that each refine their shard.
Cases and references: tests/_refine_family_cases.py (the same as the emulator tests)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _refine_cases as RC
from tests import _refine_family_cases as FC

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


def min_engine(layers, prec):
    import torch
    from pinn_elastodynamics_amd.hip_engine import HipEngine
    return HipEngine(layers, precision=prec, device=torch.device("cuda:0"), workspace_bytes=0)          # (raised to pinn_min_workspace_bytes)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def trained_frozen(X, prec="f16x3"):
    """[2,5,5,n] device tensor: the trained distance / particular nets' streams at X, by the library in the given mode (what PINN holds)"""
    import torch
    xs = [dev(X[:, k]) for k in range(3)]
    out = []
    for name in ("plate_dist", "plate_part"):
        l, f = FC.golden_net(name)
        out.append(engine(l, prec).net_streams(dev(f), *xs, FC.PLATE_LB, FC.PLATE_UB, False))
    return torch.stack(out).contiguous()


# ---- primary: head rounding only ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FC.PRIMARY_N)
@pytest.mark.parametrize("name,layers,prec", FC.PLATE_LINES, ids=[l[0] for l in FC.PLATE_LINES])
def test_plate_score_equals_the_residuals_of_the_streams_call(name, layers, prec, n):
    """PRIMARY check (see the emulator test of the same name): float64 composite and residual formulas on the fp32 output of net_streams in the same
    mode and the fp32 frozen streams passed in, bound 24 eps32 sum_i |w_i| a_i^2 per point; the engine runs in the MINIMUM workspace."""
    eng = min_engine(layers, prec)
    X, fr = FC.plate_uniform(n), FC.plate_frozen(n)
    th, xs, frd = dev(FC.fresh_net(tuple(layers))), [dev(X[:, k]) for k in range(3)], dev(fr)
    eng.lib.path_counts(reset=True)
    s = eng.plate_residual_score(th, *xs, FC.PLATE_LB, FC.PLATE_UB, False, frd, FC.PLATE_WEIGHTS).cpu().numpy()
    assert not any(eng.lib.path_counts().values())
    N = eng.net_streams(th, *xs, FC.PLATE_LB, FC.PLATE_UB, False).cpu().numpy()
    ref, bound = FC.plate_score_from_streams(N, fr)
    err = np.abs(s.astype(np.float64) - ref)
    print(f"plate {name} n={n}: max |delta| / bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(s).all() and (err <= bound).all()
    assert np.array_equal(frd.cpu().numpy(), fr), "the frozen streams were written to"


@pytest.mark.parametrize("n", FC.PRIMARY_N)
@pytest.mark.parametrize("name,layers,prec", FC.NC3D_LINES, ids=[l[0] for l in FC.NC3D_LINES])
def test_nc3d_score_equals_the_residuals_of_the_fields_call(name, layers, prec, n):
    """PRIMARY check of the 3-D head: float64 residual formulas on the fp32 output of nc3d_fields in the same mode, bound 24 eps32 sum_i |w_i| a_i^2;
    minimum workspace.  All seven lines are accepted for four inputs."""
    eng = min_engine(layers, prec)
    X = FC.nc3d_points(n)
    th, xs = dev(FC.fresh_net(tuple(layers))), [dev(X[:, k]) for k in range(4)]
    eng.lib.path_counts(reset=True)
    s = eng.nc3d_residual_score(th, *xs, FC.NC3D_LB, FC.NC3D_UB, True, FC.NC3D_WEIGHTS).cpu().numpy()
    assert not any(eng.lib.path_counts().values())
    F = eng.nc3d_fields(th, *xs, FC.NC3D_LB, FC.NC3D_UB, True).cpu().numpy()
    ref, bound = FC.nc3d_score_from_fields(F)
    err = np.abs(s.astype(np.float64) - ref)
    print(f"nc3d {name} n={n}: max |delta| / bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(s).all() and (err <= bound).all()


# ---- secondary: the float64 oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("net", FC.PLATE_SECONDARY)
def test_plate_score_against_the_float64_oracle(net, prec):
    """SECONDARY check: relative L2 of s and sqrt(s) over 1000 plate collocation points against the float64 oracle, at most 6 x the float32 oracle's
    own; D / P streams from the trained nets, evaluated by the library in the same mode"""
    layers, flat, X, ref, base = FC.plate_secondary_case(net)
    eng = engine(layers, prec)
    s = eng.plate_residual_score(dev(flat), *[dev(X[:, k]) for k in range(3)], FC.PLATE_LB, FC.PLATE_UB, False, trained_frozen(X, prec),
                                 FC.PLATE_DEFAULT_W).cpu().numpy()
    got = (FC.rel_l2(s, ref), FC.rel_l2(np.sqrt(s.astype(np.float64)), np.sqrt(ref)))
    print(f"plate {net} {prec}: s {got[0]:.3e} ({got[0] / base[0]:.2f} x fp32 oracle {base[0]:.3e}), sqrt(s) {got[1]:.3e} ({got[1] / base[1]:.2f} x {base[1]:.3e})")
    assert got[0] <= 6.0 * base[0] and got[1] <= 6.0 * base[1]


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("net", FC.NC3D_SECONDARY)
def test_nc3d_score_against_the_float64_oracle(net, prec):
    layers, flat, X, ref, base = FC.nc3d_secondary_case(net)
    eng = engine(layers, prec)
    s = eng.nc3d_residual_score(dev(flat), *[dev(X[:, k]) for k in range(4)], FC.NC3D_LB, FC.NC3D_UB, True, FC.NC3D_DEFAULT_W).cpu().numpy()
    got = (FC.rel_l2(s, ref), FC.rel_l2(np.sqrt(s.astype(np.float64)), np.sqrt(ref)))
    print(f"nc3d {net} {prec}: s {got[0]:.3e} ({got[0] / base[0]:.2f} x fp32 oracle {base[0]:.3e}), sqrt(s) {got[1]:.3e} ({got[1] / base[1]:.2f} x {base[1]:.3e})")
    assert got[0] <= 6.0 * base[0] and got[1] <= 6.0 * base[1]


# ---- selection against the oracle's own top K -------------------------------------------------------------------------------------------------------
def check_selection(tag, s_dev, s64, K, delta, eng):
    top64 = np.argsort(-s64, kind="stable")[:K]
    kth = s64[top64[-1]]
    got = eng.select_k(s_dev, K).cpu().numpy()
    diff = np.setxor1d(got, top64)
    band = int((np.abs(s64 - kth) <= delta * kth).sum())
    print(f"{tag}: {diff.size // 2} of {K} differ; {band} candidates within {delta:.2e} of the K-th float64 score")
    assert diff.size // 2 <= 0.02 * K
    assert (np.abs(s64[diff] - kth) <= delta * kth).all()


@pytest.mark.parametrize("net", ["xavier4x32", "plate70"])
def test_plate_selected_candidates_against_the_oracles_own_top_500(net):
    """The device's top 500 of 5000 plate candidates (seed 77), default weights, against the top 500 by float64 score: at most 2 % of K differ and
    every differing index has a float64 score within delta * kth of the K-th.  delta = 1e-3 for the fresh net; for the trained 8x70 net the float32
    oracle's own error is of that order, so delta = 6 x the largest relative per-point error of the float32 oracle among candidates whose float64
    score lies within a factor 2 of the K-th (computed here)."""
    K = 500
    layers, flat = FC.plate_net(net)
    cand = FC.plate_set(5000, 77)
    s64 = FC.plate_oracle_score(flat, layers, cand, FC.PLATE_DEFAULT_W)
    kth = np.sort(s64)[-K]
    delta = 1e-3
    if net == "plate70":
        s32 = FC.plate_oracle_score(flat.astype(np.float32), layers, cand.astype(np.float32), FC.PLATE_DEFAULT_W, dtype=np.float32)
        near = (s64 >= 0.5 * kth) & (s64 <= 2.0 * kth)
        delta = 6.0 * float((np.abs(s32 - s64)[near] / s64[near]).max())
    eng = engine(layers)
    s = eng.plate_residual_score(dev(flat), *[dev(cand[:, k]) for k in range(3)], FC.PLATE_LB, FC.PLATE_UB, False, trained_frozen(cand),
                                 FC.PLATE_DEFAULT_W)
    check_selection(f"plate {net}", s, s64, K, delta, eng)


def test_nc3d_selected_candidates_against_the_oracles_own_top_500():
    K = 500
    layers, flat = FC.nc3d_net("xavier3x32")
    cand = FC.nc3d_points(5000, 77)
    s64 = FC.nc3d_oracle_score(flat, layers, cand, FC.NC3D_DEFAULT_W)
    eng = engine(layers)
    s = eng.nc3d_residual_score(dev(flat), *[dev(cand[:, k]) for k in range(4)], FC.NC3D_LB, FC.NC3D_UB, True, FC.NC3D_DEFAULT_W)
    check_selection("nc3d xavier3x32", s, s64, K, 1e-3, eng)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def plate_model(n_rows=5000, seed=9):
    """uv net 4x32, small frozen nets, the smallest boundary / hole / DIST sets the constructor takes; rows from the plate's sampler"""
    from pinn_elastodynamics_amd.plate_hole import PINN
    from tests.test_plate_host import plate_sets
    sets = list(plate_sets(np.random.default_rng(3), n=8))
    Collo = np.array(FC.plate_set(n_rows, 21))
    sets[0] = Collo.copy()
    lN, lS = [3] + 4 * [32] + [5], [3] + 3 * [10] + [5]
    eng = {"uv": engine(lN), "dist": engine(lS), "part": engine(lS)}
    return PINN(*sets, lN, lS, lS, FC.PLATE_LB, FC.PLATE_UB, engines=eng, verbose=False, seed=seed), Collo


def test_plate_refine_collocation_applies_the_rule_and_moves_the_frozen_columns():
    """5000 rows, 5000 candidates, n_replace = 500: replaced rows and candidates are the rule of _refine_cases.refine_rule on the scores
    residual_score returned before the call; untouched rows of _collo AND of _frozen_collo keep their bits; replaced columns of _frozen_collo are
    the candidates' streams; refresh_frozen() afterwards changes no bit; n_collo stays, the caller's array is unwritten; one training step runs"""
    import torch
    m, Collo = plate_model()
    cand = np.array(FC.plate_set(5000, 1111))
    s_rows = m.residual_score(m.x_c, m.y_c, m.t_c).reshape(-1)
    s_cand = m.residual_score(cand[:, 0:1], cand[:, 1:2], cand[:, 2:3]).reshape(-1)
    assert s_rows.dtype == np.float32 and s_rows.shape == (5000,)
    rows, cands = RC.refine_rule(s_rows, s_cand, 500)
    assert 0 < rows.size <= 500
    frozen0 = m._frozen_collo.clone()
    frozen_cand = m._frozen_at([dev(cand[:, k]) for k in range(3)])
    want = Collo.astype(np.float32).copy()
    want[rows] = cand[cands].astype(np.float32)
    out = m.refine_collocation(cand, 500)
    assert out["replaced"] == rows.size and np.array_equal(out["rows"], rows) and np.array_equal(out["candidate_indices"], cands)
    assert out["score_replaced_max"] == float(s_rows[rows].max()) and out["score_inserted_min"] == float(s_cand[cands].min())
    got = np.stack([a.cpu().numpy() for a in m._collo], axis=1)
    assert got.shape == (5000, 3) and m.n_collo == 5000 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.concatenate([m.x_c, m.y_c, m.t_c], axis=1).astype(np.float32), want)
    assert np.array_equal(Collo, FC.plate_set(5000, 21)), "the caller's array was written to"
    untouched = np.ones(5000, dtype=bool)
    untouched[rows] = False
    ut, rt, ct = torch.from_numpy(untouched).to("cuda:0"), torch.from_numpy(rows).to("cuda:0"), torch.from_numpy(cands).to("cuda:0")
    assert m._frozen_collo.shape == (2, 5, 5, 5000) and torch.equal(m._frozen_collo[..., ut], frozen0[..., ut])
    assert torch.equal(m._frozen_collo[..., rt], frozen_cand[..., ct])
    held = m._frozen_collo.clone()
    m.refresh_frozen()
    assert torch.equal(held.view(torch.int32), m._frozen_collo.view(torch.int32)), "refresh_frozen() changed bits of the gathered frozen streams"
    h = m.train(1, 1e-3)
    assert all(np.isfinite(v).all() for v in h)


def nc3d_model(n_rows=5000):
    from pinn_elastodynamics_amd.navier_cauchy_3d import NavierCauchy3D, halfspace_case
    c = halfspace_case(n_collo=64, n_ic=40, n_top=40, n_src=(6, 5), seed=4, width=32, depth=3)
    Collo = np.array(FC.nc3d_points(n_rows, 21))
    m = NavierCauchy3D(Collo.copy(), c["SRC"], c["IC"], c["TOP"], c["uv_layers"], FC.NC3D_LB, FC.NC3D_UB, engine=engine(c["uv_layers"]), verbose=False,
                       seed=9)
    return m, Collo


def test_nc3d_refine_collocation_applies_the_rule_exactly():
    """[4]+3*[32]+[12], 5000 rows, 5000 candidates, n_replace = 500: the rule on the scores residual_score returned, untouched rows keep their bits,
    host copies follow, N stays, the caller's array is unwritten, train(1, 1e-3, batch_num=2) runs over the block boundary"""
    m, Collo = nc3d_model()
    cand = np.array(FC.nc3d_points(5000, 1111))
    cols = lambda A: [A[:, k:k + 1] for k in range(4)]
    s_rows = m.residual_score(m.x_c, m.y_c, m.z_c, m.t_c).reshape(-1)
    s_cand = m.residual_score(*cols(cand)).reshape(-1)
    assert s_rows.dtype == np.float32 and s_rows.shape == (5000,)
    rows, cands = RC.refine_rule(s_rows, s_cand, 500)
    assert 0 < rows.size <= 500
    want = Collo.astype(np.float32).copy()
    want[rows] = cand[cands].astype(np.float32)
    out = m.refine_collocation(cand, 500)
    assert out["replaced"] == rows.size and np.array_equal(out["rows"], rows) and np.array_equal(out["candidate_indices"], cands)
    assert out["score_replaced_max"] == float(s_rows[rows].max()) and out["score_inserted_min"] == float(s_cand[cands].min())
    got = np.stack([a.cpu().numpy() for a in m._rows(0, 5000)], axis=1)
    assert got.shape == (5000, 4) and m._n_collo == 5000 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    host = np.concatenate([m.x_c, m.y_c, m.z_c, m.t_c], axis=1)
    assert np.array_equal(host.astype(np.float32), want) and np.array_equal(np.stack(m._collo_host, axis=1), want)
    assert np.array_equal(Collo, FC.nc3d_points(5000, 21)), "the caller's array was written to"
    after = m.residual_score(m.x_c, m.y_c, m.z_c, m.t_c).reshape(-1)
    assert float(after.astype(np.float64).sum()) >= float(s_rows.astype(np.float64).sum())
    assert np.isfinite(m.getloss()[0]) and np.isfinite(m.train(1, 1e-3, batch_num=2)[4]).all()


def test_two_ranks_of_a_plate_model_refine_their_own_shards(tmp_path):
    """Two processes on one GPU (gloo for the collective): each rank refines its shard of a PINN with its own candidates, then trains a step.
    Parameters stay bit-identical across the ranks, a rank's replaced rows lie in its shard and obey the rule on its own scores; the worker itself
    asserts that each rank's _frozen_collo equals a fresh refresh_frozen()."""
    out = str(tmp_path / "dp_refine_plate.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29547", os.path.join(ROOT, "tests", "_dp_worker_refine_plate.py"), out], env=env, capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out)
    assert np.array_equal(z["theta0"], z["theta1"]) and np.isfinite(z["theta0"]).all()
    n = int(z["n"])
    base = FC.plate_set(n, 21).astype(np.float32)
    for r_ in (0, 1):
        lo, hi = n * r_ // 2, n * (r_ + 1) // 2
        rows = z[f"rows{r_}"]
        assert rows.size > 0 and rows.min() >= lo and rows.max() < hi
        want_rows, want_cands = RC.refine_rule(z[f"s_rows{r_}"], z[f"s_cand{r_}"], 200)
        assert np.array_equal(rows, want_rows + lo) and np.array_equal(z[f"cands{r_}"], want_cands)
        want = base[lo:hi].copy()
        want[want_rows] = z[f"cand{r_}"][want_cands]
        assert np.array_equal(z[f"shard{r_}"], want)                      # what the rank holds on the device is its refined shard
