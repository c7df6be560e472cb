"""CPU tests of backend="hip" in the three model classes: the shared driver (elastic_wave.lbfgs_hip) on the existing small host problems, with
the oracle-backed stand-in engine for the losses and the library's L-BFGS running through the x86 emulator build (tests/_lbfgs_engine.py)."""
import numpy as np
import pytest
import scipy.optimize

from pinn_elastodynamics_amd.elastic_wave import DeepHPM
from pinn_elastodynamics_amd.navier_cauchy_3d import NavierCauchy3D, halfspace_case
from pinn_elastodynamics_amd.plate_hole import PINN
from tests._lbfgs_engine import LbfgsOracleEngine, OverflowingEngine
from tests.test_host_logic import LAYERS, LB, UB, small_sets
from tests.test_plate_host import LB as PLB, LD, LN, LP, UB as PUB, nets, plate_sets

# backend="hip" against backend="torch" at the same maxfun.  Both are L-BFGS with a strong-Wolfe search on the same objective and history length,
# but torch's search interpolates differently and its iterates differ from the first step on; on these problems the loss falls by an order of
# magnitude within the budget, so a factor 2 in the loss reached is a few evaluations of progress.  Bar (fixed before measuring): hip <= 2 x torch.
# Measured: wave 1.00 x, plate 0.66 x, 3-D 0.99 x torch's loss.
VS_TORCH = 2.0


@pytest.fixture(autouse=True)
def no_scipy(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("backend='hip' must not call scipy.optimize.minimize")
    monkeypatch.setattr(scipy.optimize, "minimize", boom)


class Counter:
    def __init__(self, model, name="callback"):
        self.losses = []
        orig = getattr(model, name)

        def cb(loss):
            self.losses.append(loss)
            orig(loss)
        setattr(model, name, cb)


def wave_model(engine=None, seed=11):
    Collo, SRC, IC, UP = small_sets()
    return DeepHPM(Collo, SRC, IC, UP, LAYERS, LB, UB, engine=engine or LbfgsOracleEngine(LAYERS), verbose=False, seed=seed)


def plate_model(seed=6):
    (_, _, _), rng = nets(seed)
    eng = {"uv": LbfgsOracleEngine(LN), "dist": LbfgsOracleEngine(LD), "part": LbfgsOracleEngine(LP)}
    return PINN(*plate_sets(rng), LN, LD, LP, PLB, PUB, engines=eng, verbose=False, seed=seed)


def nc3d_model(engine_cls=LbfgsOracleEngine):
    c = halfspace_case(n_collo=301, n_ic=40, n_top=40, n_src=(6, 5), seed=4, width=16, depth=2)
    return NavierCauchy3D(c["Collo"], c["SRC"], c["IC"], c["TOP"], c["uv_layers"], c["lb"], c["ub"], engine=engine_cls(c["uv_layers"]), verbose=False, seed=9)


def test_wave_class(capsys):
    m = wave_model()
    l0 = m.getloss()[0]
    cnt = Counter(m)
    res = m.train_bfgs(1, options=dict(maxiter=25, maxfun=40), backend="hip")
    l1 = m.getloss()[0]
    assert l1 < 0.5 * l0 and res.nfev == len(cnt.losses) <= 40 and res.nit <= 25 and res.status in (3, 4) and res.message
    assert cnt.losses[0] == pytest.approx(l0, rel=1e-5) and res.fun == pytest.approx(l1, rel=1e-5) and min(cnt.losses) == pytest.approx(res.fun, rel=1e-5)
    t = wave_model()
    t.train_bfgs(1, options=dict(maxiter=25, maxfun=40), backend="torch")
    lt = t.getloss()[0]
    print(f"wave: hip {l1:.4e} torch {lt:.4e} ratio {l1 / lt:.2f}")
    assert l1 <= VS_TORCH * lt


def test_wave_class_blocks_and_batches():
    """two collocation blocks (INF:321-335 walks them), status read every 5 evaluations: same iterates as one status read per evaluation"""
    a, b = wave_model(), wave_model()
    ca, cb = Counter(a), Counter(b)
    ra = a.train_bfgs(2, options=dict(maxiter=10, maxfun=12, block=5), backend="hip")
    rb = b.train_bfgs(2, options=dict(maxiter=10, maxfun=12, block=1), backend="hip")
    assert np.array_equal(a.theta.numpy(), b.theta.numpy()) and ca.losses == cb.losses and len(ca.losses) == 24 and ra.nfev == rb.nfev == 12
    assert a.engine.advances >= b.engine.advances == 24          # (the calls of a block behind the stop change nothing)


def test_plate_class_and_both_pretraining_stages():
    m = plate_model()
    l0 = m.getloss()
    for stage, name, key in ((m.train_bfgs_dist, "callback_dist", "loss_DIST"), (m.train_bfgs_part, "callback_part", "loss_PART")):
        cnt = Counter(m, name)
        res = stage(options=dict(maxiter=8, maxfun=10), backend="hip")
        assert res.nfev == len(cnt.losses) <= 10
        assert cnt.losses[0] == pytest.approx(l0[key], rel=1e-5)              # the callbacks see the unscaled loss (PLATE:527-559)
        assert res.fun == pytest.approx(1000.0 * min(cnt.losses), rel=1e-5)   # the optimizer saw 1000 x (PLATE:220,230)
    l1 = m.getloss()
    assert l1["loss_DIST"] < l0["loss_DIST"] and l1["loss_PART"] < l0["loss_PART"]
    cnt = Counter(m)
    res = m.train_bfgs(options=dict(maxiter=12, maxfun=20), backend="hip")
    l2 = m.getloss()["loss"]
    assert l2 < 0.8 * l1["loss"] and res.nfev == len(cnt.losses) <= 20
    t = plate_model()
    t.train_bfgs_dist(options=dict(maxiter=8, maxfun=10), backend="hip")
    t.train_bfgs_part(options=dict(maxiter=8, maxfun=10), backend="hip")
    t.train_bfgs(options=dict(maxiter=12, maxfun=20), backend="torch")
    lt = t.getloss()["loss"]
    print(f"plate: hip {l2:.4e} torch {lt:.4e} ratio {l2 / lt:.2f}")
    assert l2 <= VS_TORCH * lt


# The pre-training stages (1000 x loss, gradient scale 1000) against backend="torch" at the same maxfun: the same bar, for the same reason.
# Measured: dist 1.01 x, part 0.92 x torch's loss.
@pytest.mark.parametrize("stage, key", [("train_bfgs_dist", "loss_DIST"), ("train_bfgs_part", "loss_PART")])
def test_pretraining_stages_against_torch(stage, key):
    reached = {}
    for backend in ("hip", "torch"):
        m = plate_model()
        l0 = m.getloss()[key]
        cnt = Counter(m, "callback_dist" if key == "loss_DIST" else "callback_part")
        getattr(m, stage)(options=dict(maxiter=25, maxfun=30), backend=backend)
        reached[backend] = m.getloss()[key]
        assert reached[backend] < 0.5 * l0 and len(cnt.losses) <= 31 and cnt.losses[0] == pytest.approx(l0, rel=1e-5)
    print(f"{stage}: hip {reached['hip']:.4e} torch {reached['torch']:.4e} ratio {reached['hip'] / reached['torch']:.2f}")
    assert reached["hip"] <= VS_TORCH * reached["torch"]


def test_pretraining_has_no_range_ladder():
    """The stream losses ignore the adjoint shift: a non-finite pre-training point raises at once, naming the net, and leaves the shift alone"""
    m = plate_model()
    m.theta["dist"].fill_(float("nan"))
    with pytest.raises(FloatingPointError, match="pre-training of the 'dist' net"):
        m.train_bfgs_dist(options=dict(maxiter=8, maxfun=10), backend="hip")
    assert m.eng["dist"].adjoint_shift == 0 and m.eng["dist"].advances == 10      # the one enqueued block of maxfun evaluations, no restart


def test_nc3d_class():
    m = nc3d_model()
    l0 = m.getloss()[0]
    cnt = Counter(m)
    res = m.train_bfgs(1, options=dict(maxiter=10, maxfun=15), backend="hip")
    l1 = m.getloss()[0]
    assert l1 < l0 and res.nfev == len(cnt.losses) <= 15
    t = nc3d_model()
    t.train_bfgs(1, options=dict(maxiter=10, maxfun=15), backend="torch")
    lt = t.getloss()[0]
    print(f"3-D: hip {l1:.4e} torch {lt:.4e} ratio {l1 / lt:.2f}")
    assert l1 <= VS_TORCH * lt


@pytest.mark.parametrize("nan_from", [0, 3])
def test_range_ladder_restarts_from_the_last_accepted_point(nan_from):
    """The engine's gradients turn NaN (sums intact) at the start point / from the 4th evaluation on, until adjoint_shift is raised: the stage
    reports it, the driver climbs the ladder (+ 4), starts again from the last accepted point with an empty history and finishes the budget."""
    eng = OverflowingEngine(LAYERS, nan_from)
    m = wave_model(engine=eng)
    l0 = m.getloss()[0]
    eng.wave_calls = 0
    cnt = Counter(m)
    res = m.train_bfgs(1, options=dict(maxiter=25, maxfun=40, block=4), backend="hip")
    assert eng.adjoint_shift == 4 and eng.poisoned >= 1
    assert res.nfev == len(cnt.losses) <= 40 and np.isfinite(m.theta.numpy()).all() and m.getloss()[0] < 0.5 * l0


@pytest.mark.parametrize("make, call", [(wave_model, lambda m: m.train_bfgs(1, backend="lbfgs")), (plate_model, lambda m: m.train_bfgs(backend="device")),
                                        (plate_model, lambda m: m.train_bfgs_dist(backend="")), (plate_model, lambda m: m.train_bfgs_part(backend="HIP")),
                                        (nc3d_model, lambda m: m.train_bfgs(1, backend="cuda"))])
def test_unknown_backend_raises(make, call):
    with pytest.raises(ValueError, match="backend"):
        call(make())
