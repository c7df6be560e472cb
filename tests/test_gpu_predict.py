"""-m gpu: the predict heads on the device -- HipEngine.wave_predict / plate_predict against the library's own fields / streams
call (head rounding only) and against the float64 reference, field_error_sums against numpy, and predict_device / validate /
train(validate=...) of DeepHPM and PINN end to end.  Cases and references: tests/_predict_cases.py (the same as the emulator tests)."""
import os

import numpy as np
import pytest

from tests import _predict_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
_ENGINES = {}


def min_engine(layers, prec):
    import torch
    from pinn_elastodynamics_amd.hip_engine import HipEngine
    key = (tuple(layers), prec)
    if key not in _ENGINES:
        _ENGINES[key] = HipEngine(list(layers), precision=prec, device=torch.device("cuda:0"), workspace_bytes=0)      # (raised to pinn_min_workspace_bytes)
    return _ENGINES[key]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32)).to("cuda:0")      # (a copy: the shared cases are read-only)


def run(family, layers, flat, X, prec, frozen=None, with_fields=False):
    """(predict output [rows, n], the fields / streams call of the same engine or None) as numpy, in the minimum workspace"""
    eng, th = min_engine(layers, prec), dev(flat)
    xs = [dev(X[:, k]) for k in range(X.shape[1])]
    if family == "wave":
        out = eng.wave_predict(th, *xs, PC.LB, PC.UB, True)
        F = eng.fields(th, *xs, PC.LB, PC.UB, True) if with_fields else None
    else:
        fr = dev(frozen)
        before = fr.clone()
        out = eng.plate_predict(th, *xs, PC.PLATE_LB, PC.PLATE_UB, False, fr)
        F = eng.net_streams(th, *xs, PC.PLATE_LB, PC.PLATE_UB, False) if with_fields else None
        import torch
        assert torch.equal(fr.view(torch.int32), before.view(torch.int32)), "the frozen streams were written to"
    return out.cpu().numpy(), None if F is None else F.cpu().numpy()


def check_primary(tag, out, ref, bound):
    err = np.abs(out.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(err > 0, err / bound, 0.0)))
    print(f"{tag}: max |delta| / bound = {worst:.3f}")
    assert np.isfinite(out).all() and (err <= bound).all()


# ---- primary ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layers,prec", PC.WAVE_LINES, ids=[l[0] for l in PC.WAVE_LINES])
def test_wave_predict_equals_the_rows_of_the_fields_call(name, layers, prec):
    """PRIMARY check on the device, n in (1, 33, 2100): bound 4 eps32 x (sum of the absolute values of the row's leaf terms), no forward slack"""
    for n in PC.PRIMARY_N:
        out, F = run("wave", layers, PC.fresh_net(tuple(layers)), PC.wave_points(n), prec, with_fields=True)
        check_primary(f"wave {name} n={n}", out, *PC.wave_predict_from_fields(F))


@pytest.mark.parametrize("name,layers,prec", PC.PLATE_LINES, ids=[l[0] for l in PC.PLATE_LINES])
def test_plate_predict_equals_the_composite_of_the_streams_call(name, layers, prec):
    """PRIMARY check of the plate head; stream rows 3 and 4 of both frozen blocks are NaN, the frozen array must come back unchanged"""
    for n in PC.PRIMARY_N:
        fr = PC.poisoned(PC.plate_frozen(n))
        out, N = run("plate", layers, PC.fresh_net(tuple(layers)), PC.plate_uniform(n), prec, frozen=fr, with_fields=True)
        check_primary(f"plate {name} n={n}", out, *PC.plate_predict_from_streams(N, fr))


# ---- secondary --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("family,net", PC.SECONDARY_CASES, ids=[f"{f}-{n}" for f, n in PC.SECONDARY_CASES])
def test_predict_against_the_float64_reference(family, net, prec):
    """SECONDARY check on the device: relative L2 over 1000 points of the value rows and of the strain rows, each as one block, at most 6 x the
    same error of the float32 run of the reference (profiles/predict_head_accuracy.txt holds the multiples)"""
    layers, flat, X, ref, base = PC.secondary_case(family, net)
    frozen = None
    if family == "plate":
        xs = [dev(X[:, k]) for k in range(3)]
        st = lambda nm: (lambda lf: min_engine(lf[0], prec).net_streams(dev(lf[1]), *xs, PC.PLATE_LB, PC.PLATE_UB, False).cpu().numpy())(PC.golden_net(nm))
        frozen = np.stack([st("plate_dist"), st("plate_part")])
    out, _ = run(family, layers, flat, X, prec, frozen=frozen)
    got = PC.block_errors(family, out, ref)
    print(f"{family} {net} {prec}: values {got[0]:.3e} ({got[0] / base[0]:.2f} x float32 reference {base[0]:.3e}), "
          f"strains {got[1]:.3e} ({got[1] / base[1]:.2f} x {base[1]:.3e})")
    assert got[0] <= 6.0 * base[0] and got[1] <= 6.0 * base[1]


# ---- error sums -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PC.ERR_N)
def test_field_error_sums_against_numpy(n):
    import torch
    pred, ref, want = PC.error_data(n)
    eng = min_engine([3, 32, 32, 7], "f16x3")
    p, r = dev(pred).reshape(PC.ERR_PRED_ROWS, n), dev(ref).reshape(len(PC.ERR_ROWS), n)
    a = eng.field_error_sums(p, PC.ERR_ROWS, r)
    b = eng.field_error_sums(p, PC.ERR_ROWS, r)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))             # two calls: identical bits
    a = a.cpu().numpy()
    if n == 0:
        assert (a == 0.0).all()
        return
    rel = np.abs(a - want) / want
    print(f"error sums n={n}: largest relative difference {rel.max():.2e} (bound {(n + 2) * 2.0 ** -52:.2e})")
    assert (rel <= (n + 2) * 2.0 ** -52).all()


# ---- the model classes ------------------------------------------------------------------------------------------------------------------------------------
def blocks_agree(family, a, b):
    for sl in (PC.VALUE_ROWS[family], PC.STRAIN_ROWS[family]):
        assert PC.rel_l2(a[sl], b[sl].astype(np.float64)) <= 1e-6


def wave_model(golden_dir=None):
    from pinn_elastodynamics_amd import pointsets as ps
    from pinn_elastodynamics_amd.elastic_wave import DeepHPM
    if golden_dir is None:
        c = ps.infinite_case(N_f=3000, N_ext=300, seed=5, width=32)
        return DeepHPM(c["Collo"], c["SRC"], c["IC"], c["UP"], c["uv_layers"], c["lb"], c["ub"], verbose=False)
    c = ps.infinite_case(N_f=3000, N_ext=300, seed=5)
    return DeepHPM(c["Collo"], c["SRC"], c["IC"], c["UP"], c["uv_layers"], c["lb"], c["ub"], ExistModel=1, modelDir=f"{golden_dir}/weights_inf20s.npz",
                   case="infinite", verbose=False)


def plate_model(golden_dir):
    from pinn_elastodynamics_amd import pointsets as ps
    from pinn_elastodynamics_amd.plate_hole import PINN
    c = ps.plate_case(seed=9, n_collo=3000, n_refine=1500)
    paths = {k: f"{golden_dir}/weights_plate_{k}.npz" for k in ("uv", "dist", "part")}
    return PINN(c["Collo"], c["HOLE"], c["IC"], c["LF"], c["RT"], c["UP"], c["LW"], c["DIST"], c["uv_layers"], c["dist_layers"], c["part_layers"],
                c["lb"], c["ub"], partDir=paths["part"], distDir=paths["dist"], uvDir=paths["uv"], verbose=False)


def test_wave_class_predict_validate_and_train(golden_dir):
    """DeepHPM at the reference's trained weights: predict_device equals predict to 1e-6 relative L2 per row block, predict_frames stacks
    predict_device per frame, validate reproduces pointsets.relative_l2 of the downloaded predict on the FEM fixture to 1e-6 relative;
    then train(iter=4, validate=dict(every=2)) on a small fresh model records steps 2 and 4"""
    from pinn_elastodynamics_amd import pointsets as ps
    m = wave_model(golden_dir)
    fem = np.load(f"{golden_dir}/fem_inf20s.npz")["fem"].astype(np.float64)
    cols = (fem[:, 0:1], fem[:, 1:2], fem[:, 2:3])
    host = np.concatenate(m.predict(*cols), axis=1).T
    blocks_agree("wave", m.predict_device(*cols).cpu().numpy(), host)
    fr = m.predict_frames(fem[:50, 0], fem[:50, 1], np.array([1.0, 7.5])).cpu().numpy()
    assert fr.shape == (2, 8, 50) and np.array_equal(fr[1], m.predict_device(fem[:50, 0], fem[:50, 1], np.full(50, 7.5)).cpu().numpy())
    ref = {k: fem[:, 3 + j] for j, k in enumerate(("u", "v", "s11", "s22", "s12"))}
    got = m.validate(*cols, ref)
    for j, k in enumerate(ref):
        assert got[k] == pytest.approx(ps.relative_l2(host[j], np.asarray(ref[k], dtype=np.float32)), rel=1e-6)
    small = wave_model()
    small.train(4, 1e-3, 1, validate=dict(every=2, points=cols, ref=ref, fields=("u", "s12")))
    assert [s for s, _ in small.val_rec] == [2, 4] and small.val_rec[1][1] == small.validate(*cols, ref, fields=("u", "s12"))
    assert all(np.isfinite(list(d.values())).all() for _, d in small.val_rec)


def test_plate_class_predict_validate_and_train(golden_dir):
    from pinn_elastodynamics_amd import pointsets as ps
    m = plate_model(golden_dir)
    fem = np.load(f"{golden_dir}/fem_plate.npz")["fem"].astype(np.float64)
    cols = (fem[:, 0:1], fem[:, 1:2], fem[:, 2:3])
    host = np.concatenate(m.predict(*cols), axis=1).T
    blocks_agree("plate", m.predict_device(*cols).cpu().numpy(), host)
    ref = {k: fem[:, 3 + j] for j, k in enumerate(("u", "v", "s11", "s22", "s12"))}
    got = m.validate(*cols, ref)
    for j, k in enumerate(ref):
        assert got[k] == pytest.approx(ps.relative_l2(host[j], np.asarray(ref[k], dtype=np.float32)), rel=1e-6)
    m.train(4, 1e-4, validate=dict(every=2, points=cols, ref=ref))
    assert [s for s, _ in m.val_rec] == [2, 4] and m.val_rec[1][1] == m.validate(*cols, ref)
