"""CPU tests of the host side of material identification (pinn_elastodynamics_amd/material.py and DeepHPM.train(identify=...)): the derivative
formulas against central differences of the float64 oracle loss, the Hooke coefficients and the host Adam against the oracle's, the schedule's
bookkeeping on a call-recording stand-in engine, and the 2-rank data-parallel path (gloo)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pinn_oracle as po
from pinn_elastodynamics_amd import material
from pinn_elastodynamics_amd.elastic_wave import DeepHPM, DeepHPMConfined
from tests import _material_cases as MC
from tests.test_host_logic import LAYERS, LB, UB, small_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP_START = dict(E=3.5, mu=0.3, rho=1.2)
DP_IDENTIFY = dict(params=("E", "mu", "rho"), lr=1e-2)


@pytest.mark.parametrize("plane_strain", [True, False])
def test_gradient_equals_central_differences_of_the_oracle_loss(plane_strain):
    """dL/dE, dL/dmu, dL/drho from the 14 sums against central differences of L = sum_i w_i sumsq_i of the float64 oracle, relative 1e-6"""
    layers = [3] + 4 * [32] + [7]
    flat, X = MC.fresh_net(tuple(layers)), MC.points(2100, seed=77)
    E, mu, rho = 7.3, 0.31, 1.9
    w = np.array([1.0, 2.0, 3.0, 1.0, 0.5, 1.0, 2.0]) / X.shape[0]
    sums, _ = MC.oracle_sums(flat, layers, X, consts=(E, mu, rho, plane_strain))
    g = material.gradient(sums, w, E, mu, rho, plane_strain)

    def loss(E_, mu_, rho_):
        ss, _, _ = po.wave2d_loss_grad(flat, layers, X[:, 0], X[:, 1], X[:, 2], LB, UB, True, E_, mu_, rho_, plane_strain, want_grad=False)
        return float(ss @ w)

    np.testing.assert_allclose(sums[:7] @ w, loss(E, mu, rho), rtol=1e-12)
    for k, name in enumerate(material.NAMES):
        c = [E, mu, rho]
        h = 1e-5 * c[k]
        hi, lo = list(c), list(c)
        hi[k] += h
        lo[k] -= h
        fd = (loss(*hi) - loss(*lo)) / (2.0 * h)
        print(f"plane_strain={plane_strain} d/d{name}: {g[name]:.9e} against {fd:.9e}, relative {abs(g[name] - fd) / abs(fd):.1e}")
        assert abs(g[name] - fd) <= 1e-6 * abs(fd), name


@pytest.mark.parametrize("plane_strain", [True, False])
def test_hooke_and_its_jacobian(plane_strain):
    for E, mu in ((2.5, 0.25), (7.3, 0.31), (20.0, 0.0)):
        np.testing.assert_allclose(material.hooke(E, mu, plane_strain), po.hooke_coeffs(E, mu, plane_strain), rtol=1e-15)
        J = material.hooke_jacobian(E, mu, plane_strain)
        hE, hm = 1e-6 * E, 1e-6
        fdE = (np.array(po.hooke_coeffs(E + hE, mu, plane_strain)) - np.array(po.hooke_coeffs(E - hE, mu, plane_strain))) / (2 * hE)
        fdm = (np.array(po.hooke_coeffs(E, mu + hm, plane_strain)) - np.array(po.hooke_coeffs(E, mu - hm, plane_strain))) / (2 * hm)
        np.testing.assert_allclose(J[:, 0], fdE, rtol=1e-8)
        np.testing.assert_allclose(J[:, 1], fdm, rtol=1e-7, atol=1e-8)


def test_host_adam_is_the_tf1_rule():
    rng = np.random.default_rng(4)
    x, m, v = rng.standard_normal(3), np.zeros(3), np.zeros(3)
    adam, y = material.HostAdam(3), x.copy()
    for step in range(1, 8):
        g = rng.standard_normal(3)
        x, m, v = po.adam_tf1_step(x, g, m, v, step, 1e-2)
        y = adam.step(y, g, 1e-2)
        np.testing.assert_allclose(y, x, rtol=1e-14)


def wave_model(eng=None, n=120, cls=DeepHPM, **kw):
    Collo, SRC, IC, UP = small_sets(n=n)
    eng = MC.OracleMaterialEngine(LAYERS) if eng is None else eng
    if cls is DeepHPMConfined:
        return DeepHPMConfined(Collo, SRC, IC, UP, None, LAYERS, None, None, LB, UB, engine=eng, verbose=False, seed=5, **kw), eng
    return DeepHPM(Collo, SRC, IC, UP, LAYERS, LB, UB, engine=eng, verbose=False, seed=5, **kw), eng


def test_identify_none_makes_the_calls_of_today():
    a, ea = wave_model()
    b, eb = wave_model()
    a.train(3, 1e-3, 2)
    b.train(3, 1e-3, 2, identify=None)
    assert ea.calls == eb.calls and not any(c[0] == "material" for c in eb.calls)
    assert np.array_equal(a.theta.numpy(), b.theta.numpy()) and not hasattr(b, "material_rec")
    assert (b.E, b.mu, b.rho) == (2.5, 0.25, 1.0)


def test_identify_schedule_counts_bounds_and_names():
    m, eng = wave_model(**DP_START)
    m.train(7, 1e-3, 1, identify=dict(params=("E", "mu", "rho"), lr=1e-2, every=3))
    mat = [k for k, c in enumerate(eng.calls) if c[0] == "material"]
    assert len(mat) == 2 and [r[0] for r in m.material_rec] == [3, 6]
    # the sums are enqueued BEFORE the step's call: the third and sixth collocation evaluation each follow a material call
    waves = [k for k, c in enumerate(eng.calls) if c[0] == "wave"]
    assert mat[0] == waves[2] - 1 and mat[1] == waves[5] - 1
    assert all(r[1] != DP_START["E"] and r[2] != DP_START["mu"] and r[3] != DP_START["rho"] for r in m.material_rec)
    assert (m.E, m.mu, m.rho) == tuple(m.material_rec[-1][1:]) and m.E > 0 and m.rho > 0
    # only the named constants move; bounds clip mu; every=1 over two blocks
    m2, eng2 = wave_model(mu=0.3)
    m2.train(2, 1e-3, 2, identify=dict(params=("mu",), lr=0.5, bounds=dict(mu=(0.29, 0.31))))
    assert sum(c[0] == "material" for c in eng2.calls) == 4 and [r[0] for r in m2.material_rec] == [1, 2, 3, 4]
    assert all(r[2] in (0.29, 0.31) for r in m2.material_rec) and (m2.E, m2.rho) == (2.5, 1.0)
    # the blocks of the sums are the step's blocks
    assert [c[1] for c in eng2.calls if c[0] == "material"] == [60, 60, 60, 60]
    for bad in (dict(params=("E", "nu")), dict(params=()), dict(params=("E",), rate=1.0), dict(params=("E",), every=0), dict(params=("E", "E"))):
        with pytest.raises(ValueError):
            wave_model()[0].train(1, 1e-3, 1, identify=bad)


def test_identify_first_step_is_the_adam_step_along_the_oracle_gradient():
    """one step: the constants move by the host Adam along material.gradient of the block's float64 sums -- E and rho as logarithms"""
    m, _ = wave_model(**DP_START)
    n = m._n_collo
    g = m.material_gradient()
    w = m._material_weights(n)
    flat = m.theta.numpy().astype(np.float64)
    X = np.stack([a[:, 0] for a in (m.x_c, m.y_c, m.t_c)], 1)
    sums, _ = MC.oracle_sums(flat, LAYERS, X.astype(np.float32).astype(np.float64), consts=(3.5, 0.3, 1.2, True))
    ref = material.gradient(sums, w, 3.5, 0.3, 1.2, True)
    np.testing.assert_allclose([g[k] for k in material.NAMES], [ref[k] for k in material.NAMES], rtol=1e-9)
    np.testing.assert_allclose(m.material_sums(), sums, rtol=1e-12)
    m.train(1, 1e-3, 1, identify=dict(params=("E", "mu", "rho"), lr=1e-2))
    x0 = np.array([np.log(3.5), 0.3, np.log(1.2)])
    gx = np.array([3.5 * ref["E"], ref["mu"], 1.2 * ref["rho"]])
    x1, _, _ = po.adam_tf1_step(x0, gx, np.zeros(3), np.zeros(3), 1, 1e-2)
    np.testing.assert_allclose([np.log(m.E), m.mu, np.log(m.rho)], x1, rtol=1e-12)


def test_identify_post_record_uses_the_packed_weights_and_confined_passes_it_through():
    class Packed(MC.OracleMaterialEngine):
        def material_sums(self, *a, packed=False, **kw):
            self.calls.append(("packed", packed))
            return super().material_sums(*a, packed=packed, **kw)
    m, eng = wave_model(Packed(LAYERS))
    m.train(2, 1e-3, 1, record="post", identify=dict(params=("E",)))
    assert [c[1] for c in eng.calls if c[0] == "packed"] == [False, True]     # behind a post re-evaluation the workspace holds the current weights
    m, eng = wave_model(Packed(LAYERS))
    m.train(2, 1e-3, 1, identify=dict(params=("E",)))
    assert [c[1] for c in eng.calls if c[0] == "packed"] == [False, False]
    mc, engc = wave_model(cls=DeepHPMConfined)
    out = mc.train(2, 1e-3, 1, identify=dict(params=("rho",), every=2))
    assert len(out) == 3 and sum(c[0] == "material" for c in engc.calls) == 1 and mc.rho != 1.0
    assert "constants stay where they are" in DeepHPM.train_bfgs.__doc__


def test_identify_two_ranks_match_single(tmp_path):
    """world_size-2 gloo run of six identified steps: both ranks hold equal constants, and they equal the single-process run within the
    tolerance the two-rank wave test holds the parameters to"""
    script = os.path.join(ROOT, "tests", "_dp_worker_material.py")
    out = str(tmp_path / "dp.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29561")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29561", script, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    Collo, SRC, IC, UP = small_sets(n=257)
    m = DeepHPM(Collo, SRC, IC, UP, LAYERS, LB, UB, case="semi_infinite", engine=MC.OracleMaterialEngine(LAYERS), verbose=False, seed=9, **DP_START)
    m.train(3, 1e-3, 2, identify=DP_IDENTIFY)
    assert z["rec"].shape == (6, 4) and len(m.material_rec) == 6
    np.testing.assert_array_equal(z["c0"], z["c1"])
    np.testing.assert_allclose(z["c0"], [m.E, m.mu, m.rho], rtol=2e-5, atol=2e-7)
    assert abs(m.E - 3.5) > 1e-3 and abs(m.mu - 0.3) > 1e-3 and abs(m.rho - 1.2) > 1e-3
