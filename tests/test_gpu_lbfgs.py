"""-m gpu: the device L-BFGS (pinn_lbfgs_*, backend="hip") on an MI355X: the direction and convergence cases of tests/test_emulated_lbfgs.py
through HipEngine on device buffers, the three model classes on the fixtures of the existing L-BFGS GPU tests, and a two-process run."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import pinn_oracle as po
from tests import _lbfgs_cases as LC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LB, UB = [0.0, 0.0, 0.0], [30.0, 30.0, 20.0]
OPTS = dict(maxcor=8, maxiter=10000, maxfun=10000, maxls=50, ftol=0.0, gtol=0.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


class DevicePort:
    """tests/_lbfgs_cases.drive on device buffers through HipEngine's lbfgs_* methods"""

    def __init__(self, dev, skew=0):
        self.skew = skew               # floats: 1 puts params and grad 4 bytes off 16-byte alignment (the scalar path)
        from pinn_elastodynamics_amd.hip_engine import HipEngine
        self.eng = HipEngine([3, 32, 32, 7], device=dev, max_points=1 << 10)        # (any net: the optimizer only needs the library and the stream)
        self.dev = dev

    def start(self, x0, options, coeffs, grad_scale):
        self.state = self.eng.lbfgs_state(x0.size, int(options.get("maxcor", 10)))
        self.params = torch.zeros(x0.size + 8, dtype=torch.float32, device=self.dev)[self.skew:self.skew + x0.size]
        self.params.copy_(torch.from_numpy(x0.copy()))
        self.grad = torch.zeros(x0.size + 8, dtype=torch.float32, device=self.dev)[self.skew:self.skew + x0.size]
        self.sums = torch.zeros(len(coeffs), dtype=torch.float32, device=self.dev)
        self.eng.lbfgs_init(self.state, options, coeffs, grad_scale)

    def put(self, grad, sums):
        self.grad.copy_(torch.from_numpy(grad))
        self.sums.copy_(torch.from_numpy(sums))

    def advance(self):
        self.eng.lbfgs_advance(self.state, self.params, self.grad, self.sums)

    def status(self):
        return self.eng.lbfgs_status(self.state)

    def x(self):
        return self.params.cpu().numpy()

    def debug(self):
        return self.eng.lbfgs_debug(self.state)


@pytest.mark.parametrize("pairs", [5, 8, 24])
def test_direction_equals_two_loop_on_the_stored_history(dev, pairs):
    """As tests/test_emulated_lbfgs.py, on the device: bar 2 x the error of rounding the float64 two-loop direction to fp32 (one rounding of an
    fp64 result + the margin for the order of the fp64 sums).  Measured on an MI355X: rounding error 2.1e-8 / 2.6e-8 / 2.7e-8 at the three
    history fills, difference the same to three digits (ratio 1.00)."""
    fun, x0 = LC.smooth_convex(300, seed=3)
    port = DevicePort(dev)
    rec, trace = LC.drive(port, fun, x0, OPTS, until=lambda r: r["iterations"] >= pairs)
    assert rec["status"] == 0 and rec["iterations"] == pairs and rec["skipped"] == 0
    d, S, Y = port.debug()
    ref = LC.two_loop_direction(LC.accepted_gradient(trace), S, Y)
    diff = float(np.linalg.norm(d.astype(np.float64) - ref) / np.linalg.norm(ref))
    rounding = LC.fp32_rounding_error(ref)
    print(f"pairs {pairs}: direction vs float64 two-loop {diff:.3e}, fp32 rounding of the reference {rounding:.3e}, ratio {diff / rounding:.2f}")
    assert S.shape[0] == min(pairs, 8) and diff <= 2.0 * rounding


@pytest.mark.parametrize("skew", [0, 1])
def test_direction_with_a_gradient_scale_and_a_scalar_tail(dev, skew):
    """As tests/test_emulated_lbfgs.py: grad_scale = 1000, P = 303 (scalar tail), aligned and skewed pointers: the stored pairs are bit for bit
    the separately rounded fp32 mul and sub, the direction equals the two-loop one within 2 x fp32 rounding.  Measured on an MI355X: ratio 1.00."""
    fun, x0 = LC.smooth_convex(303, seed=7)
    port = DevicePort(dev, skew=skew)
    rec, trace = LC.drive(port, fun, x0, OPTS, until=lambda r: r["iterations"] >= 11, grad_scale=1000.0)
    assert rec["status"] == 0 and rec["pairs"] == 8 and port.params.data_ptr() % 16 == 4 * skew
    diff, rounding, same = LC.scaled_direction_check(port, trace, 1000.0)
    print(f"grad_scale 1000, skew {skew}: direction vs two-loop {diff:.3e}, rounding {rounding:.3e}, ratio {diff / rounding:.2f}")
    assert same and diff <= 2.0 * rounding


def test_large_vector_uses_many_workgroups(dev):
    """40 001 parameters (39 workgroups in the inner-product pass, a scalar tail), m = 64: converges, direction still equals the two-loop one"""
    fun, x0 = LC.quadratic(40001, 50.0, seed=4)
    port = DevicePort(dev)
    rec, trace = LC.drive(port, fun, x0, dict(OPTS, maxcor=64), until=lambda r: r["iterations"] >= 12)
    d, S, Y = port.debug()
    ref = LC.two_loop_direction(LC.accepted_gradient(trace), S, Y)
    diff = float(np.linalg.norm(d.astype(np.float64) - ref) / np.linalg.norm(ref))
    print(f"P 40001: direction vs two-loop {diff:.3e}, rounding {LC.fp32_rounding_error(ref):.3e}")
    assert S.shape[0] == 12 and diff <= 2.0 * LC.fp32_rounding_error(ref)


def test_convergence_against_scipy_counts(dev):
    """The two convergence problems of the CPU tests with the same margins over scipy's evaluation count (1.5 x + 10).  Measured on an MI355X:
    quadratic 59 evaluations (scipy 59), chained Rosenbrock 152 (scipy 153)."""
    import scipy.optimize
    for name, (fun, x0), m, gtol in (("quadratic", LC.quadratic(50, 100.0, seed=1), 10, 1e-4), ("rosenbrock", LC.chained_rosenbrock(23), 17, 1e-3)):
        x0 = x0.astype(np.float32)
        rec, _ = LC.drive(DevicePort(dev), fun, x0, dict(OPTS, maxcor=m, gtol=gtol))
        ref = scipy.optimize.minimize(fun, x0.astype(np.float64), jac=True, method="L-BFGS-B",
                                      options=dict(maxcor=m, maxiter=10000, maxfun=10000, maxls=50, ftol=0.0, gtol=gtol))
        print(f"{name}: device nfev {rec['evaluations']} nit {rec['iterations']}, scipy nfev {ref.nfev} nit {ref.nit}")
        assert rec["status_name"] == "gtol" and rec["evaluations"] <= 1.5 * ref.nfev + 10


def counted(model, name="callback"):
    seen = []
    orig = getattr(model, name)

    def cb(loss):
        seen.append(loss)
        orig(loss)
    setattr(model, name, cb)
    return seen


def test_wave_class_on_device(dev, tmp_path):
    from pinn_elastodynamics_amd.elastic_wave import DeepHPM
    rng = np.random.default_rng(6)
    layers = [3] + 4 * [32] + [7]
    Collo, SRC, IC = po.collocation_points(5000, LB, UB, rng), po.ricker_source_set(n_pt=20, n_time=30), po.ic_grid(num=15)
    m = DeepHPM(Collo, SRC, IC, np.zeros((0, 3)), layers, LB, UB, case="infinite", seed=3, verbose=False)
    l0 = m.getloss()[0]
    m.engine.lib.path_counts(reset=True)
    res = m.train_bfgs(batch_num=1, options=dict(maxiter=15, maxfun=20), backend="hip")
    cnt = m.engine.lib.path_counts(reset=True)
    l1 = m.getloss()[0]
    assert l1 < 0.7 * l0 and m.count == res.nfev == len(m.loss_rec) and 10 <= res.nfev <= 20
    assert cnt["fused-registers"] >= res.nfev and cnt["two-kernel"] == 0 and cnt["fp32"] == 0
    assert res.fun == pytest.approx(l1, rel=1e-5)
    m.save_NN(str(tmp_path / "uv.pickle"))
    m2 = DeepHPM(Collo, SRC, IC, np.zeros((0, 3)), layers, LB, UB, ExistModel=1, modelDir=str(tmp_path / "uv.pickle"), case="infinite", verbose=False)
    assert torch.equal(m.theta, m2.theta) and abs(m2.getloss()[0] - l1) < 1e-6 * max(1.0, l1)


def test_plate_class_and_pretraining_on_device(dev, tmp_path):
    from pinn_elastodynamics_amd.plate_hole import PINN
    from tests.test_plate_host import plate_sets
    rng = np.random.default_rng(11)
    sets = plate_sets(rng, n=4000)
    lN, lD, lP = [3] + 4 * [32] + [5], [3] + 4 * [20] + [5], [3] + 4 * [20] + [5]
    m = PINN(*sets, lN, lD, lP, [0.0, 0.0, 0.0], [0.5, 0.5, 10.0], verbose=False)
    lib = m.eng["uv"].lib
    l0 = m.getloss()
    lib.path_counts(reset=True)
    sd, sp = counted(m, "callback_dist"), counted(m, "callback_part")
    rd = m.train_bfgs_dist(options=dict(maxiter=20, maxfun=25), backend="hip")
    rp = m.train_bfgs_part(options=dict(maxiter=20, maxfun=25), backend="hip")
    cnt = lib.path_counts(reset=True)
    l1 = m.getloss()
    assert l1["loss_DIST"] < 0.5 * l0["loss_DIST"] and l1["loss_PART"] < l0["loss_PART"]
    assert len(sd) == rd.nfev <= 25 and len(sp) == rp.nfev <= 25 and sd[0] == pytest.approx(l0["loss_DIST"], rel=1e-4)
    assert cnt["fused-registers"] >= rd.nfev + rp.nfev        # 4 x 20 nets: the fused multi-set kernel
    lib.path_counts(reset=True)
    res = m.train_bfgs(options=dict(maxiter=15, maxfun=20), backend="hip")
    cnt = lib.path_counts(reset=True)
    l2 = m.getloss()
    assert l2["loss"] < l1["loss"] and res.nfev == m.count - rd.nfev - rp.nfev
    assert cnt["fused-registers"] >= res.nfev
    for TYPE, key in (("UV", "uv"), ("DIST", "dist"), ("PART", "part")):
        m.save_NN(str(tmp_path / f"{key}.npz"), TYPE)
    m2 = PINN(*sets, lN, lD, lP, [0.0, 0.0, 0.0], [0.5, 0.5, 10.0], partDir=str(tmp_path / "part.npz"), distDir=str(tmp_path / "dist.npz"),
              uvDir=str(tmp_path / "uv.npz"), verbose=False)
    for k in ("uv", "dist", "part"):
        assert torch.equal(m.theta[k], m2.theta[k])
    assert m2.getloss()["loss"] == pytest.approx(l2["loss"], rel=1e-6)


def test_nc3d_class_on_device(dev, tmp_path):
    from pinn_elastodynamics_amd.navier_cauchy_3d import NavierCauchy3D, halfspace_case
    c = halfspace_case(n_collo=20000, n_ic=2000, n_top=2000, n_src=(40, 20), seed=2, width=128, depth=10)
    m = NavierCauchy3D(c["Collo"], c["SRC"], c["IC"], c["TOP"], c["uv_layers"], c["lb"], c["ub"], verbose=False, seed=3)
    l0 = m.getloss()[0]
    m.engine.lib.path_counts(reset=True)
    seen = counted(m)
    res = m.train_bfgs(1, options=dict(maxiter=15, maxfun=20), backend="hip")
    cnt = m.engine.lib.path_counts(reset=True)
    l1 = m.getloss()[0]
    assert l1 < l0 and len(seen) == res.nfev <= 20
    assert cnt["fused-lds"] >= res.nfev and cnt["two-kernel"] == 0
    m.save_NN(str(tmp_path / "uv.npz"))
    m2 = NavierCauchy3D(c["Collo"], c["SRC"], c["IC"], c["TOP"], c["uv_layers"], c["lb"], c["ub"], ExistModel=1, modelDir=str(tmp_path / "uv.npz"), verbose=False)
    assert torch.equal(m.theta, m2.theta)


def test_two_ranks_on_one_gpu_stay_bit_identical(tmp_path):
    out = str(tmp_path / "dp_lbfgs.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29541", os.path.join(ROOT, "tests", "_dp_worker_lbfgs.py"), out], env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out)
    assert np.array_equal(z["theta0"], z["theta1"]) and np.isfinite(z["theta0"]).all()
    l0, l1, fun = z["loss"]
    nfev, nit, count = z["counts"]
    assert l1 < 0.7 * l0 and fun == pytest.approx(l1, rel=1e-5) and nfev == count <= 30
