"""CPU tests of the host side of material identification for the plate and 3-D families (material.py's family descriptions, PINN.train and
NavierCauchy3D.train with identify=...): the derivative formulas against central differences of the float64 oracle loss, the schedule's
bookkeeping on a call-recording stand-in engine, and the 2-rank data-parallel path (gloo)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import nc3d_oracle as n3
from oracle import plate_oracle as pl
from pinn_elastodynamics_amd import material
from pinn_elastodynamics_amd.navier_cauchy_3d import NavierCauchy3D, halfspace_case
from pinn_elastodynamics_amd.plate_hole import PINN
from tests import _material_family_cases as MF
from tests import _refine_family_cases as FC
from tests.test_plate_host import LB, LD, LN, LP, UB, nets, plate_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP_START = dict(E=12.0, mu=0.3, rho=1.2)
DP_IDENTIFY = dict(params=("E", "mu", "rho"), lr=1e-2)
DP_STEPS = 4


def central_differences(loss, g, E, mu, rho, tag):
    for k, name in enumerate(material.NAMES):
        c = [E, mu, rho]
        h = 1e-6 * c[k]
        hi, lo = list(c), list(c)
        hi[k] += h
        lo[k] -= h
        fd = (loss(*hi) - loss(*lo)) / (2.0 * h)
        print(f"{tag} d/d{name}: {g[name]:.9e} against {fd:.9e}, relative {abs(g[name] - fd) / abs(fd):.1e}")
        assert abs(g[name] - fd) <= 1e-6 * abs(fd), name


def test_plate_gradient_equals_central_differences_of_the_oracle_loss():
    """dL/dE, dL/dmu, dL/drho from the 12 sums (plane-stress Jacobian) against central differences, step 1e-6 relative, of
    L = sum_i w_i sum_n f_i^2 of plate_oracle.plate_residuals in float64; distinct non-zero weights; relative 1e-6.  The frozen streams are
    brought to unit scale in every stream row: with the kernel tests' scales (d2/dt2 at 0.05) dL/drho is 1e-5 of L and the DIFFERENCE QUOTIENT,
    not the formula, loses seven digits to cancellation (measured 8e-7); at unit scale it measures 5e-10."""
    layers, n = [3] + 4 * [32] + [5], 2100
    X = FC.plate_uniform(n)
    fr = FC.plate_frozen(n).astype(np.float64) / np.array([1.0, 2.0, 2.0, 0.2, 0.05])[None, :, None, None]
    F = pl.composite(pl.net_streams(np.asarray(FC.fresh_net(tuple(layers))), layers, X[:, 0], X[:, 1], X[:, 2]), fr[0], fr[1])
    E, mu, rho = MF.GENERAL
    w = np.array([1.0, 2.0, 3.0, 0.5, 1.5]) / n
    sums = MF.plate_sums_of_composite(F, E, mu, rho)
    assert sums.shape == (material.PLATE.n_sums,)
    loss = lambda E_, mu_, rho_: float(((pl.plate_residuals(F, E_, mu_, rho_) ** 2).sum(0)) @ w)
    np.testing.assert_allclose(sums[:5] @ w, loss(E, mu, rho), rtol=1e-12)
    central_differences(loss, material.gradient(sums, w, E, mu, rho, material.PLATE), E, mu, rho, "plate")


def test_nc3d_gradient_equals_central_differences_of_the_oracle_loss():
    """the same for the 24 sums of the 3-D family and nc3d_oracle.nc3d_residuals; (lambda + 2G, lambda, G) is the plane-strain hooke()"""
    layers, n = [4] + 3 * [32] + [12], 2100
    X = FC.nc3d_points(n)
    o = n3.nc3d_fields(np.asarray(FC.fresh_net(tuple(layers))), layers, X[:, 0], X[:, 1], X[:, 2], X[:, 3], FC.NC3D_LB, FC.NC3D_UB, True)
    E, mu, rho = MF.GENERAL
    w = np.array(FC.NC3D_WEIGHTS) / n + 0.1 / n
    sums = MF.nc3d_sums_of_fields(o["Y"], o["dY"], E, mu, rho)
    assert sums.shape == (material.NC3D.n_sums,) and (w > 0).all() and len(set(w)) == 12
    np.testing.assert_allclose(material.hooke(E, mu, True), n3.hooke3d(E, mu), rtol=1e-15)
    loss = lambda E_, mu_, rho_: float(((n3.nc3d_residuals(o["Y"], o["dY"], E_, mu_, rho_) ** 2).sum(0)) @ w)
    np.testing.assert_allclose(sums[:12] @ w, loss(E, mu, rho), rtol=1e-12)
    central_differences(loss, material.gradient(sums, w, E, mu, rho, material.NC3D), E, mu, rho, "nc3d")


def test_family_descriptions_and_the_wave_signature():
    """gradient() checks the family's lengths; the wave family is still reached by its plane_strain flag"""
    with pytest.raises(ValueError):
        material.gradient(np.zeros(14), np.zeros(5), 1.0, 0.3, 1.0, material.PLATE)
    with pytest.raises(ValueError):
        material.gradient(np.zeros(24), np.zeros(7), 1.0, 0.3, 1.0, material.NC3D)
    M, w = np.arange(1.0, 15.0), np.arange(1.0, 8.0)
    for ps, fam in ((True, material.WAVE), (False, material.WAVE_PLANE_STRESS)):
        assert material.gradient(M, w, 2.5, 0.25, 1.0, ps) == material.gradient(M, w, 2.5, 0.25, 1.0, fam)
    assert (material.PLATE.n_sums, material.PLATE.n_weights, material.PLATE.plane_strain) == (12, 5, False)
    assert (material.NC3D.n_sums, material.NC3D.n_weights, material.NC3D.plane_strain) == (24, 12, True)


# ---- the schedule on the stand-in engine ---------------------------------------------------------------------------------------------------------
def plate_model(seed=2, n=120, **consts):
    _, rng = nets(seed)
    eng = {"uv": MF.FamilyMaterialEngine(LN), "dist": MF.FamilyMaterialEngine(LD), "part": MF.FamilyMaterialEngine(LP)}
    m = PINN(*plate_sets(rng, n), LN, LD, LP, LB, UB, engines=eng, verbose=False, seed=seed)
    for k, v in consts.items():
        setattr(m, k, v)
    return m, eng["uv"]


def nc3d_model(n=301, **kw):
    c = halfspace_case(n_collo=n, n_ic=40, n_top=40, n_src=(6, 5), seed=4, width=16, depth=2)
    eng = MF.FamilyMaterialEngine(c["uv_layers"])
    return NavierCauchy3D(c["Collo"], c["SRC"], c["IC"], c["TOP"], c["uv_layers"], c["lb"], c["ub"], engine=eng, verbose=False, seed=9, **kw), eng


def train(m, steps, identify=None, **kw):
    return m.train(steps, 1e-3, identify=identify, **kw) if isinstance(m, PINN) else m.train(steps, 1e-3, 1, identify=identify, **kw)


@pytest.mark.parametrize("model,call", [(plate_model, "plate"), (nc3d_model, "nc3d")], ids=["plate", "nc3d"])
def test_identify_none_makes_the_calls_of_today(model, call):
    a, ea = model()
    b, eb = model()
    a.train(3, 1e-3) if call == "plate" else a.train(3, 1e-3, 2)
    b.train(3, 1e-3, identify=None) if call == "plate" else b.train(3, 1e-3, 2, identify=None)
    assert ea.calls == eb.calls and sum(c[0] == call for c in eb.calls) >= 3 and not any(c[0] == "material" for c in eb.calls)
    ta, tb = (a.theta["uv"], b.theta["uv"]) if call == "plate" else (a.theta, b.theta)
    assert np.array_equal(ta.numpy(), tb.numpy()) and not hasattr(b, "material_rec")
    assert (b.E, b.mu, b.rho) == ((20.0, 0.25, 1.0) if call == "plate" else (2.5, 0.25, 1.0))


@pytest.mark.parametrize("model,call", [(plate_model, "plate"), (nc3d_model, "nc3d")], ids=["plate", "nc3d"])
def test_identify_schedule_counts_bounds_and_names(model, call):
    m, eng = model(**DP_START)
    train(m, 7, dict(params=("E", "mu", "rho"), lr=1e-2, every=3))
    mat = [k for k, c in enumerate(eng.calls) if c[0] == "material"]
    assert len(mat) == 2 and [r[0] for r in m.material_rec] == [3, 6]
    # the sums are enqueued BEFORE the step's call: the third and sixth collocation evaluation of the loop each follow a material call
    steps = [k for k, c in enumerate(eng.calls) if c[0] == call][-7:]
    assert mat[0] == steps[2] - 1 and mat[1] == steps[5] - 1
    assert all(r[1] != DP_START["E"] and r[2] != DP_START["mu"] and r[3] != DP_START["rho"] for r in m.material_rec)
    assert (m.E, m.mu, m.rho) == tuple(m.material_rec[-1][1:]) and m.E > 0 and m.rho > 0
    # the sums are taken over the step's rows, unpacked
    n_rows = m.n_collo if call == "plate" else m._n_collo
    assert [c[1:] for c in eng.calls if c[0] == "material"] == [(n_rows, False)] * 2
    # only the named constants move; bounds clip mu; the Adam state is the model's and survives a second call with the same names
    m2, eng2 = model(mu=0.3)
    E0, rho0 = m2.E, m2.rho
    train(m2, 2, dict(params=("mu",), lr=0.5, bounds=dict(mu=(0.29, 0.31))))
    state = m2._material_adam[1]
    train(m2, 2, dict(params=("mu",), lr=0.5, bounds=dict(mu=(0.29, 0.31))))
    assert m2._material_adam[1] is state and state.t == 4
    assert sum(c[0] == "material" for c in eng2.calls) == 4 and [r[0] for r in m2.material_rec] == [1, 2, 1, 2]
    assert all(r[2] in (0.29, 0.31) for r in m2.material_rec) and (m2.E, m2.rho) == (E0, rho0)
    for bad in (dict(params=("E", "nu")), dict(params=()), dict(params=("E",), rate=1.0), dict(params=("E",), every=0), dict(params=("E", "E")),
                dict(params=("E",), bounds=dict(nu=(0, 1)))):
        with pytest.raises(ValueError):
            train(model()[0], 1, bad)


@pytest.mark.parametrize("model,call", [(plate_model, "plate"), (nc3d_model, "nc3d")], ids=["plate", "nc3d"])
def test_identify_first_step_is_the_adam_step_along_the_family_gradient(model, call):
    """one step: the constants move by the host Adam along material.gradient of the block's float64 sums with the weights of the training step
    -- [10 / n_collo] * 5 for the plate, [f_uv / n] * 6 + [f_s / n] * 6 for the 3-D class --, E and rho as logarithms"""
    from oracle import pinn_oracle as po
    m, _ = model(**DP_START)
    fam = material.PLATE if call == "plate" else material.NC3D
    n = m._material_rows()
    w = m._material_weights(n)
    assert w == ([10.0 / n] * 5 if call == "plate" else [5.0 / n] * 12) and m.material_family is fam
    sums = m.material_sums()
    assert sums.shape == (fam.n_sums,) and sums.dtype == np.float64
    ref = material.gradient(sums, w, *DP_START.values(), fam)
    g = m.material_gradient()
    assert g == ref and m.material_gradient([2.0 * v for v in w])["rho"] == pytest.approx(2.0 * ref["rho"], rel=1e-14)
    with pytest.raises(ValueError):
        m.material_gradient([1.0] * 7)
    train(m, 1, DP_IDENTIFY)
    x0 = np.array([np.log(DP_START["E"]), DP_START["mu"], np.log(DP_START["rho"])])
    gx = np.array([DP_START["E"] * ref["E"], ref["mu"], DP_START["rho"] * ref["rho"]])
    x1, _, _ = po.adam_tf1_step(x0, gx, np.zeros(3), np.zeros(3), 1, 1e-2)
    np.testing.assert_allclose([np.log(m.E), m.mu, np.log(m.rho)], x1, rtol=1e-12)
    doc = (PINN.train if call == "plate" else NavierCauchy3D.train_bfgs).__doc__
    assert "constants" in doc


@pytest.mark.parametrize("family", ["plate", "nc3d"])
def test_identify_two_ranks_match_single(tmp_path, family):
    """world_size-2 gloo run of DP_STEPS identified steps: both ranks hold identical constants, and they equal the single-process run on the
    union set to 1e-12 relative.  The net's own learning rate is 0 in both runs: the stand-in returns each rank's gradient rounded to fp32, so
    with a moving net the two runs' weights -- and with them the constants -- would agree to fp32 rounding only; with the net at rest the
    comparison is of the sums' path alone (this rank's rows, the all-reduce, the same host update on every rank), which is float64 throughout."""
    script = os.path.join(ROOT, "tests", "_dp_worker_material_families.py")
    out = str(tmp_path / "dp.npz")
    port = "29563" if family == "plate" else "29564"
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", port, script, family, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    m = dp_model(family)
    dp_train(m)
    assert z["rec"].shape == (DP_STEPS, 4) and len(m.material_rec) == DP_STEPS
    np.testing.assert_array_equal(z["c0"], z["c1"])
    print(f"{family}: two ranks {z['c0']}, one rank {[m.E, m.mu, m.rho]}, max rel dev {float(np.abs(z['c0'] / [m.E, m.mu, m.rho] - 1).max()):.1e}")
    np.testing.assert_allclose(z["c0"], [m.E, m.mu, m.rho], rtol=1e-12)
    np.testing.assert_allclose(z["rec"], np.array(m.material_rec), rtol=1e-12)
    assert all(abs(v / DP_START[k] - 1) > 1e-3 for k, v in zip(material.NAMES, (m.E, m.mu, m.rho)))


def dp_model(family):
    """the model of the two-rank test (both the worker's ranks and the single process build it): 257 rows, an odd split"""
    return (plate_model(seed=3, n=257, **DP_START) if family == "plate" else nc3d_model(n=257, **DP_START))[0]


def dp_train(m):
    return m.train(DP_STEPS, 0.0, identify=DP_IDENTIFY) if isinstance(m, PINN) else m.train(DP_STEPS // 2, 0.0, 2, identify=DP_IDENTIFY)
