"""-m gpu: candidates drawn on the device and selection keys -- HipEngine.sample_box / refine_keys against the numpy references of
tests/_sample_cases.py (the same as the emulator tests: exact for the coordinates and the mask keys, the 4 x delta_ref bar for the sampling
keys), then refine_collocation with an int ``candidates``, ``exclude`` and both ``select`` modes in DeepHPM, NavierCauchy3D and PINN, and two
data-parallel ranks whose streams differ without coordination."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _refine_cases as RC
from tests import _refine_family_cases as FC
from tests import _sample_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SIZES = (257, 70001, 300000)
DISC = (15.0, 15.0, 2.0)                                  # the source disc of the infinite case


def engine():
    from tests.test_gpu_refine import engine as shared
    return shared([3, 32, 32, 7])


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host(cols):
    return np.stack([c.cpu().numpy() for c in cols], axis=1)


# ---- the two calls against the numpy references ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_unit_box_equals_the_reference_bit_for_bit(n):
    eng = engine()
    for dim, first, seed, stream in ((3, 0, 1111, 0), (4, 2 ** 32 - 3, 0x1234567890ABCDEF, 7)):
        got = host(eng.sample_box(n, [0.0] * dim, [1.0] * dim, seed, stream, first))
        assert got.shape == (n, dim) and np.array_equal(bits(got), bits(SC.unit_box(seed, stream, first, n, dim)))
        tail = host(eng.sample_box(n - 100, [0.0] * dim, [1.0] * dim, seed, stream, first + 100))
        assert np.array_equal(bits(tail), bits(got[100:]))
    lo, hi = FC.NC3D_LB, FC.NC3D_UB
    got, ref = host(eng.sample_box(n, lo, hi, 5, 1)), SC.box64(5, 1, 0, n, lo, hi)
    assert (np.abs(got - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()
    assert (got >= np.asarray(lo, dtype=np.float32)).all() and (got <= np.asarray(hi, dtype=np.float32)).all()


@pytest.mark.parametrize("n", SIZES)
def test_mask_keys_are_the_scores_outside_the_balls(n):
    from pinn_elastodynamics_amd.capi import Ball
    import ctypes
    eng = engine()
    for keep in (0, 1):
        for name, dim, balls in SC.ball_cases(keep):
            P = SC.mask_points(dim)[:n]
            cols = [np.ascontiguousarray(P[:, k]) for k in range(dim)]
            assert SC.boundary_margin(cols, balls) > 1e-6, "a reference point too close to a boundary: a condition on the inputs"
            score = np.random.default_rng(n).standard_normal(n).astype(np.float32)
            score[n // 3] = np.nan
            bs = [Ball((ctypes.c_double * 3)(*ce), r, nd, kp) for ce, r, nd, kp in balls]
            sc, xs = dev(score), [dev(a) for a in cols]
            got = eng.refine_keys(sc, xs, bs, "mask").cpu().numpy()
            want = np.where(SC.in_balls(cols, balls), np.float32(-np.inf), score)
            assert np.array_equal(bits(got), bits(want)), (name, n, keep)
            assert np.array_equal(bits(sc.cpu().numpy()), bits(score)) and np.array_equal(bits(host(xs)), bits(P))


@pytest.mark.parametrize("n", SIZES)
def test_sample_keys_against_the_float64_reference(n):
    """the bar of the emulator test of the same name: the -inf set exactly the reference's, delta <= 4 x delta_ref; two calls give the same bits"""
    import torch
    from pinn_elastodynamics_amd.capi import Ball
    import ctypes
    eng = engine()
    name, dim, balls = SC.ball_cases(0)[1]
    P = SC.mask_points(dim)[:n]
    cols = [np.ascontiguousarray(P[:, k]) for k in range(dim)]
    score, u = SC.sample_scores(n), SC.noise_u(SC.KEY_SEED, SC.KEY_STREAM, SC.KEY_FIRST, n)
    bs = [Ball((ctypes.c_double * 3)(*ce), r, nd, kp) for ce, r, nd, kp in balls]
    sc, xs = dev(score), [dev(a) for a in cols]
    inside = SC.in_balls(cols, balls)
    for power, c in SC.POWER_C:
        a, b = (eng.refine_keys(sc, xs, bs, "sample", power, c, SC.KEY_SEED, SC.KEY_STREAM, SC.KEY_FIRST) for _ in range(2))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        got = a.cpu().numpy()
        d, d_ref, same = SC.key_errors(got, score, inside, power, c, u)
        print(f"n={n} power={power} c={c}: delta {d:.3e}, delta_ref {d_ref:.3e}, ratio {d / d_ref if d_ref else 0.0:.2f}")
        assert same, "the excluded set differs from the reference's"
        assert not np.isnan(got).any() and d <= 4.0 * d_ref


def test_sample_then_select_is_a_weighted_draw():
    n, K = 65536, 1024
    eng = engine()
    score = np.where(np.arange(n) % 2 == 1, 3.0, 1.0).astype(np.float32)
    u = SC.noise_u(1111, 0, 0, n)
    kd = eng.refine_keys(dev(score), [], (), "sample", 1.0, 0.0, 1111, 0, 0)
    keys, sel = kd.cpu().numpy(), eng.select_k(kd, K).cpu().numpy().astype(np.int64)
    assert sel.size == K and (np.diff(sel) > 0).all()
    assert np.array_equal(sel, np.sort(np.argsort(-keys, kind="stable")[:K]))
    none = np.zeros(n, dtype=bool)
    k64, _ = SC.keys_reference(score, none, 1.0, 0.0, u, np.float64)
    d, d_ref, same = SC.key_errors(keys, score, none, 1.0, 0.0, u)
    delta = 4.0 * d_ref
    assert same and d <= delta
    thr = np.sort(k64)[::-1][K - 1]
    chosen = np.zeros(n, dtype=bool)
    chosen[sel] = True
    assert (k64[sel] >= thr - delta).all() and chosen[k64 > thr + delta].all()
    assert abs(float((sel % 2 == 1).mean()) - 0.75) <= 0.07


# ---- DeepHPM ------------------------------------------------------------------------------------------------------------------------------------
def wave_model():
    from tests.test_gpu_refine import model
    return model([3] + 4 * [32] + [7], n_rows=4096)


def outside(P, disc):
    return (P[:, 0] - disc[0]) ** 2 + (P[:, 1] - disc[1]) ** 2 > disc[2] ** 2


@pytest.mark.parametrize("select", ["top", "sample"])
def test_wave_refine_with_device_candidates(select):
    """fresh 4x32 net, 4096 rows, 8192 candidates drawn in (lb, ub), the source disc excluded: nothing inside the disc goes in, something is
    replaced, the device rows and the host columns agree, the set's size and the shard bounds stay, and a second identical model with the same
    seed inserts identical rows"""
    outs = []
    for _ in range(2):
        m, Collo = wave_model()
        shard = m._shard(0, 4096)
        out = m.refine_collocation(8192, 500, seed=42, select=select, exclude=[DISC])
        P = out["candidates"]
        assert out["replaced"] > 0 and P.shape == (out["replaced"], 3) and outside(P, DISC).all()
        assert out["candidate_indices"].max() < 8192 and np.unique(out["candidate_indices"]).size == out["replaced"]
        got = host(m._collo)
        want = Collo.astype(np.float32)
        want[out["rows"]] = P.astype(np.float32)
        assert got.shape == (4096, 3) and np.array_equal(bits(got), bits(want))
        assert np.array_equal(np.concatenate([m.x_c, m.y_c, m.t_c], axis=1).astype(np.float32), want)
        assert m._n_collo == 4096 and m._shard(0, 4096) == shard
        assert (P >= np.asarray(RC.LB)).all() and (P <= np.asarray(RC.UB)).all()
        outs.append(out)
    a, b = outs
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["candidate_indices"], b["candidate_indices"]) and np.array_equal(a["candidates"], b["candidates"])


def test_wave_top_with_device_candidates_equals_the_host_path():
    """select="top" with device candidates and an excluded disc against the path that existed before: the same candidates copied to the host,
    the points in the disc removed, passed as an array -- the same rows give way to the same points"""
    m1, _ = wave_model()
    m2, _ = wave_model()
    out1 = m1.refine_collocation(8192, 500, seed=42, exclude=[DISC])
    C = host(m2.engine.sample_box(8192, RC.LB, RC.UB, 42, 0)).astype(np.float64)
    keep = outside(C.astype(np.float32), np.asarray(DISC, dtype=np.float32))
    assert 0 < (~keep).sum() < 400                                      # (the disc is 1.4 % of the box)
    out2 = m2.refine_collocation(C[keep], 500)
    assert "candidates" not in out2 and out1["replaced"] == out2["replaced"] > 0
    assert np.array_equal(out1["rows"], out2["rows"]) and np.array_equal(out1["candidates"], C[keep][out2["candidate_indices"]])
    assert np.array_equal(out1["candidate_indices"], np.flatnonzero(keep)[out2["candidate_indices"]])
    assert np.array_equal(bits(host(m1._collo)), bits(host(m2._collo)))
    assert (out1["score_replaced_max"], out1["score_inserted_min"]) == (out2["score_replaced_max"], out2["score_inserted_min"])
    # the next device-drawn round of the same model reads another stream
    assert not np.array_equal(m1.refine_collocation(8192, 500, seed=42, exclude=[DISC])["candidates"][:5], out1["candidates"][:5])
    h = m1.train(4, 1e-3, 1, refine=dict(every=2, candidates=2048, n_replace=100, seed=3, select="sample", exclude=[DISC]))
    assert np.isfinite(h[4]).all() and m1._refine_round == 4


# ---- the other two families ---------------------------------------------------------------------------------------------------------------------
def test_nc3d_refine_with_device_candidates():
    """3x32 net, four columns, a ball in (x, y, z) excluded; both select modes on the same model"""
    from tests.test_gpu_refine_families import nc3d_model
    m, Collo = nc3d_model(4096)
    ball = (15.0, 15.0, -15.0, 8.0)
    want = Collo.astype(np.float32)
    for select in ("top", "sample"):
        out = m.refine_collocation(8192, 500, seed=11, select=select, exclude=[ball])
        P = out["candidates"]
        assert out["replaced"] > 0 and P.shape == (out["replaced"], 4)
        assert (((P[:, :3] - np.asarray(ball[:3])) ** 2).sum(axis=1) > ball[3] ** 2).all()
        want[out["rows"]] = P.astype(np.float32)
        assert np.array_equal(bits(host(m._rows(0, 4096))), bits(want)) and np.array_equal(np.stack(m._collo_host, axis=1), want)
        assert np.array_equal(np.concatenate([m.x_c, m.y_c, m.z_c, m.t_c], axis=1).astype(np.float32), want) and m._n_collo == 4096
    assert np.isfinite(m.train(2, 1e-3, batch_num=2, refine=dict(every=2, candidates=1024, n_replace=50, exclude=[ball]))[4]).all()


def test_plate_refine_with_device_candidates_moves_the_frozen_columns():
    """4x32 uv net, the hole disc (0, 0, 0.1) excluded: the frozen D / P streams of the drawn candidates follow the rows -- refresh_frozen()
    afterwards gives the same bits"""
    import torch
    from tests.test_gpu_refine_families import plate_model
    m, Collo = plate_model(4096)
    hole = (0.0, 0.0, 0.1)
    want = Collo.astype(np.float32)
    for select in ("top", "sample"):
        out = m.refine_collocation(8192, 500, seed=13, select=select, exclude=[hole])
        P = out["candidates"]
        assert out["replaced"] > 0 and P.shape == (out["replaced"], 3) and outside(P, hole).all()
        want[out["rows"]] = P.astype(np.float32)
        assert np.array_equal(bits(host(m._collo)), bits(want)) and m.n_collo == 4096
        assert np.array_equal(np.concatenate([m.x_c, m.y_c, m.t_c], axis=1).astype(np.float32), want)
        held = m._frozen_collo.clone()
        m.refresh_frozen()
        assert torch.equal(held.view(torch.int32), m._frozen_collo.view(torch.int32)), "refresh_frozen() changed bits of the gathered frozen streams"
    assert all(np.isfinite(v).all() for v in m.train(2, 1e-3, refine=dict(every=1, candidates=1024, n_replace=50, exclude=[hole])))


# ---- two ranks ----------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_draw_from_different_streams(tmp_path):
    """Two processes on one GPU (gloo for the collective): two rounds per rank, no stream given.  Round r of rank k reads stream 2 r + k: the
    inserted points are the reference's points of that stream at the returned indices, so no point goes in twice; rows stay in the shard;
    the parameters stay bit-identical across the ranks."""
    out = str(tmp_path / "dp_sample.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29553", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29553", os.path.join(ROOT, "tests", "_dp_worker_sample.py"), out], env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out)
    assert np.array_equal(z["theta0"], z["theta1"]) and np.isfinite(z["theta0"]).all()
    n = int(z["n"])
    seen = []
    for rank in (0, 1):
        lo, hi = n * rank // 2, n * (rank + 1) // 2
        for rnd in (0, 1):
            rows, idx, pts = z[f"rows_{rnd}_{rank}"], z[f"idx_{rnd}_{rank}"], z[f"pts_{rnd}_{rank}"]
            assert rows.size > 0 and rows.min() >= lo and rows.max() < hi
            ref = SC.box64(77, 2 * rnd + rank, 0, 3000, RC.LB, RC.UB)[idx]
            assert (np.abs(pts - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()           # this stream's points, no other's
            assert outside(pts, DISC).all()
            seen.append(pts)
    allp = np.concatenate(seen)
    assert np.unique(allp, axis=0).shape[0] == allp.shape[0]
