"""CPU tests of the device L-BFGS (pinn_lbfgs_* of include/pinn_hip.h, csrc/pinn_lbfgs.hpp): the same kernel sources compiled for x86 against the
SIMT emulator, on host arrays; f and g are evaluated in numpy between the advance calls.  Every buffer handed to the library is framed by guard
words that are checked after every call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _lbfgs_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                 # bytes of 0xA5 on both sides of every buffer
EPS = float(np.finfo(float).eps)


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pinn_elastodynamics_amd", "csrc"), "-j", str(min(16, os.cpu_count() or 1)), "emu"],
                   check=True, stdout=subprocess.DEVNULL)
    from pinn_elastodynamics_amd.capi import PinnLib
    return PinnLib(os.path.join(ROOT, "build", "emu", "libpinn_emu.so"))


class Guarded:
    """nbytes of payload at a 256-byte aligned address (+ `skew` bytes), guard words in front and behind"""

    def __init__(self, nbytes, skew=0):
        self.raw = np.full(nbytes + 2 * GUARD + 512 + skew, 0xA5, dtype=np.uint8)
        base = self.raw.ctypes.data
        self.off = (-(base + GUARD) % 256) + GUARD + skew
        self.nbytes = nbytes
        self.ptr = base + self.off

    def view(self, dtype):
        return self.raw[self.off:self.off + self.nbytes].view(dtype)

    def guards_intact(self):
        return bool((self.raw[:self.off] == 0xA5).all() and (self.raw[self.off + self.nbytes:] == 0xA5).all())


class HostPort:
    def __init__(self, lib, skew=0):
        self.lib, self.skew = lib, skew

    def start(self, x0, options, coeffs, grad_scale):
        P, m = x0.size, int(options.get("maxcor", 10))
        self.P, self.m = P, m
        nb = self.lib.lbfgs_state_bytes(P, m)
        assert nb > 0
        self.state, self.params, self.grad, self.sums = Guarded(nb), Guarded(4 * P, self.skew), Guarded(4 * P, self.skew), Guarded(4 * len(coeffs))
        self.params.view(np.float32)[:] = x0
        self.lib.lbfgs_init(self.state.ptr, nb, P, options, coeffs, grad_scale)
        self.check_guards()

    def buffers(self):
        return (self.state, self.params, self.grad, self.sums)

    def check_guards(self):
        assert all(b.guards_intact() for b in self.buffers()), "a guard word was overwritten"

    def put(self, grad, sums):
        self.grad.view(np.float32)[:] = grad
        self.sums.view(np.float32)[:] = sums

    def advance(self):
        self.lib.lbfgs_advance(self.state.ptr, self.params.ptr, self.grad.ptr, self.sums.ptr)
        self.check_guards()

    def status(self):
        return self.lib.lbfgs_status(self.state.ptr)

    def x(self):
        return self.params.view(np.float32).copy()

    def debug(self):
        return self.lib.lbfgs_debug_read(self.state.ptr, self.P, self.m)

    def losses(self, first, count):
        return self.lib.lbfgs_read_losses(self.state.ptr, first, count)


OPTS = dict(maxcor=8, maxiter=10000, maxfun=10000, maxls=50, ftol=0.0, gtol=0.0)


@pytest.mark.parametrize("pairs", [5, 8, 24])
def test_direction_equals_two_loop_on_the_stored_history(emu, pairs):
    """After `pairs` accepted pairs (below m = 8, equal to m, 3 m with the ring wrapped twice) the direction in the state equals a float64 two-loop
    recursion on the SAME stored fp32 history and the fp32 gradient of the last accepted point.
    Bar, fixed before the code ran: 2 x the error of merely rounding the reference direction to fp32.  The device forms the direction in fp64 from
    fp64 inner products of the stored fp32 rows and rounds it ONCE to fp32 -- that is 1 x the rounding error; the second unit is the margin for the
    different order of the fp64 sums in the compact form and the two-loop recursion (1e-16 x the conditioning of R, far below 1e-8 on this problem).
    Measured on the 300-parameter convex problem below (x86 emulator build): rounding error 2.1e-8 / 2.6e-8 / 2.7e-8 at the three history fills, difference
    the same to three digits (ratio 1.00)."""
    fun, x0 = LC.smooth_convex(300, seed=3)
    port = HostPort(emu)
    rec, trace = LC.drive(port, fun, x0, OPTS, until=lambda r: r["iterations"] >= pairs)
    assert rec["status"] == 0 and rec["iterations"] == pairs and rec["skipped"] == 0
    d, S, Y = port.debug()
    assert S.shape[0] == min(pairs, 8)
    ref = LC.two_loop_direction(LC.accepted_gradient(trace), S, Y)
    diff = float(np.linalg.norm(d.astype(np.float64) - ref) / np.linalg.norm(ref))
    rounding = LC.fp32_rounding_error(ref)
    print(f"pairs {pairs}: direction vs float64 two-loop {diff:.3e}, fp32 rounding of the reference {rounding:.3e}, ratio {diff / rounding:.2f}")
    assert diff <= 2.0 * rounding
    # the newest stored pair is the difference of the two fp32 points the evaluations saw, not alpha * d
    acc = [t for i, t in enumerate(trace) if i == 0 or t[3]["iterations"] > trace[i - 1][3]["iterations"]]
    assert np.array_equal(S[-1], acc[-1][0] - acc[-2][0]) and np.array_equal(Y[-1], acc[-1][2] - acc[-2][2])


@pytest.mark.parametrize("skew", [0, 4])
def test_direction_with_a_gradient_scale_and_a_scalar_tail(emu, skew):
    """The pre-training stages' setting: grad_scale = 1000, so gn = 1000 * g is a rounded product and y = gn - g_k a second rounding; P = 303 leaves
    a 3-element scalar tail behind the 16-byte loads, and skewed pointers put every element on the scalar path.  The stored pairs are bit for bit
    the fp32 differences of the accepted points / scaled gradients (mul and sub separately rounded, no fma), and the direction equals the two-loop
    one on them under the same bar as above (2 x fp32 rounding of the reference).  Measured: ratio 1.00 at both skews."""
    fun, x0 = LC.smooth_convex(303, seed=7)
    port = HostPort(emu, skew=skew)
    rec, trace = LC.drive(port, fun, x0, OPTS, until=lambda r: r["iterations"] >= 11, grad_scale=1000.0)
    assert rec["status"] == 0 and rec["pairs"] == 8
    diff, rounding, same = LC.scaled_direction_check(port, trace, 1000.0)
    print(f"grad_scale 1000, skew {skew}: direction vs two-loop {diff:.3e}, rounding {rounding:.3e}, ratio {diff / rounding:.2f}")
    assert same and diff <= 2.0 * rounding


@pytest.mark.parametrize("maxiter, m", [(3, 8), (11, 4)])
def test_pairs_held_after_a_stop_are_the_pairs_stored(emu, maxiter, m):
    """The step that stops a stage is not stored: `pairs` counts the rows debug_read returns, and those are the differences of the accepted points
    before it, oldest first -- below a full ring and with the ring wrapped."""
    fun, x0 = LC.smooth_convex(40, seed=9)
    port = HostPort(emu)
    rec, trace = LC.drive(port, fun, x0, dict(OPTS, maxcor=m, maxiter=maxiter))
    assert rec["status_name"] == "maxiter" and rec["iterations"] == maxiter
    d, S, Y = port.debug()
    acc = LC.accepted(trace)[:-1]                      # every accepted point but the one the stage stopped at
    held = min(m, maxiter - 1)
    assert rec["pairs"] == S.shape[0] == held
    for i in range(held):
        assert np.array_equal(S[-1 - i], acc[-1 - i][0] - acc[-2 - i][0]) and np.array_equal(Y[-1 - i], acc[-1 - i][2] - acc[-2 - i][2])


def scipy_count(fun, x0, m, gtol):
    import scipy.optimize
    res = scipy.optimize.minimize(fun, np.asarray(x0, dtype=np.float64), jac=True, method="L-BFGS-B",
                                  options=dict(maxcor=m, maxiter=10000, maxfun=10000, maxls=50, ftol=0.0, gtol=gtol))
    return res


def test_quadratic_converges_to_gtol(emu):
    """Strictly convex quadratic, 50 parameters, condition 100, m = 10, gtol 1e-4 (fp32 parameters put a floor of ~100 x 6e-8 x |x| under the
    gradient: the tolerance sits a decade above it).  Evaluation count against scipy's L-BFGS-B (float64 iterates, same m and tolerances): the
    line searches share More-Thuente's logic but the device's iterates are fp32, so the paths part after a few steps; margin 1.5 x scipy + 10.
    Measured: device 59 evaluations in 55 iterations, scipy 59 in 55."""
    fun, x0 = LC.quadratic(50, 100.0, seed=1)
    x0 = x0.astype(np.float32)
    opts = dict(OPTS, maxcor=10, gtol=1e-4)
    rec, trace = LC.drive(HostPort(emu), fun, x0, opts)
    ref = scipy_count(fun, x0, 10, 1e-4)
    print(f"quadratic: device nfev {rec['evaluations']} nit {rec['iterations']}, scipy nfev {ref.nfev} nit {ref.nit}")
    assert rec["status_name"] == "gtol" and rec["max_abs_grad"] <= 1e-4
    assert ref.success and rec["evaluations"] <= 1.5 * ref.nfev + 10
    assert abs(rec["f"] - ref.fun) <= 1e-5 * max(1.0, abs(ref.fun))


def test_chained_rosenbrock_converges_with_odd_sizes(emu):
    """Chained Rosenbrock, P = 23 (not a multiple of 4), m = 17, gtol 1e-3 (curvature up to ~1e3: fp32 parameters floor the gradient near 1e-4).
    Margin over scipy's evaluation count as above: 1.5 x + 10.  Measured: device 152 evaluations in 129 iterations, scipy 153 in 126."""
    fun, x0 = LC.chained_rosenbrock(23)
    x0 = x0.astype(np.float32)
    opts = dict(OPTS, maxcor=17, gtol=1e-3)
    rec, trace = LC.drive(HostPort(emu), fun, x0, opts)
    ref = scipy_count(fun, x0, 17, 1e-3)
    print(f"rosenbrock: device nfev {rec['evaluations']} nit {rec['iterations']} f {rec['f']:.3e}, scipy nfev {ref.nfev} nit {ref.nit} f {ref.fun:.3e}")
    assert rec["status_name"] == "gtol"
    assert ref.success and rec["evaluations"] <= 1.5 * ref.nfev + 10
    assert rec["f"] < 1e-6 and np.allclose(trace[-1][0], 1.0, atol=1e-2)


def test_unaligned_parameter_and_gradient_pointers_take_the_scalar_path(emu):
    fun, x0 = LC.quadratic(37, 30.0, seed=5)
    rec, _ = LC.drive(HostPort(emu, skew=4), fun, x0, dict(OPTS, gtol=1e-4))
    assert rec["status_name"] == "gtol"


@pytest.mark.parametrize("P", [1, 3])
def test_tiny_parameter_counts(emu, P):
    fun, x0 = LC.quadratic(P, 10.0, seed=P)
    rec, trace = LC.drive(HostPort(emu), fun, x0, dict(OPTS, gtol=1e-5))
    assert rec["status_name"] == "gtol" and rec["evaluations"] < 40


def test_stop_rules_carry_their_status(emu):
    fun, x0 = LC.chained_rosenbrock(10)
    rec, trace = LC.drive(HostPort(emu), fun, x0, dict(OPTS, maxfun=7))
    assert rec["status_name"] == "maxfun" and rec["evaluations"] == 7 and len(trace) == 7
    rec, _ = LC.drive(HostPort(emu), fun, x0, dict(OPTS, maxiter=3))
    assert rec["status_name"] == "maxiter" and rec["iterations"] == 3
    rec, trace = LC.drive(HostPort(emu), fun, x0, dict(OPTS, ftol=0.5))
    assert rec["status_name"] == "ftol" and rec["iterations"] >= 1
    fs = [t[1] for t in trace]
    port = HostPort(emu)
    rec, trace = LC.drive(port, fun, x0, dict(OPTS, maxfun=30))
    # the loss ring holds every evaluation's loss, in order
    assert port.losses(0, rec["loss_pos"]) == [t[1] for t in trace] and rec["loss_pos"] == rec["evaluations"] == 30
    assert port.losses(25, 5) == [t[1] for t in trace[25:]]
    # at a stop the parameters are the last accepted point, whose loss the record carries
    assert fun(port.x().astype(np.float64))[0] == pytest.approx(rec["f"], rel=1e-12)
    assert rec["f"] == min(t[3]["f"] for t in trace) and fs


def test_curvature_skipped_pair_is_counted(emu):
    """f = -x has no curvature: the search extrapolates to its largest step (a warning end with sufficient decrease, taken as L-BFGS-B takes it),
    y = 0 there, s.y <= 2.2e-16 y.y: the pair is skipped, counted, and not stored."""
    rec, _ = LC.drive(HostPort(emu), lambda x: (-float(x[0]), np.array([-1.0])), np.array([0.5]), dict(OPTS, maxiter=1))
    assert rec["status_name"] == "maxiter" and rec["skipped"] == 1 and rec["pairs"] == 0 and rec["step"] == 1e10


def test_nan_trial_is_cut_back_and_never_enters_the_history(emu):
    fun0, x0 = LC.quadratic(3, 4.0, seed=2)
    x0 = 3.0 * x0.astype(np.float32)
    seen = {"nan": 0}

    def fun(x):
        if np.linalg.norm(x - x0) > 0.4 and seen["nan"] < 2 or np.linalg.norm(x - x0) > 50.0:
            seen["nan"] += 1
            return float("nan"), np.full(3, np.nan)
        return fun0(x)

    port = HostPort(emu)

    def finite_state(rec):
        d, S, Y = port.debug()
        assert np.isfinite(S).all() and np.isfinite(Y).all() and np.isfinite(rec["f"])

    rec, trace = LC.drive(port, fun, x0, dict(OPTS, gtol=1e-4), after_each=finite_state)
    assert seen["nan"] == 2 and rec["status_name"] == "gtol"
    # first trial at step min(1, 1/|g|): NaN; halved: NaN again; a quarter: finite (whether it also satisfies the Wolfe conditions is the search's business)
    g0 = trace[0][2].astype(np.float64)
    a0 = min(1.0, 1.0 / np.linalg.norm(g0))
    for i, frac in ((1, 1.0), (2, 0.5), (3, 0.25)):
        assert np.allclose(trace[i][0].astype(np.float64), x0 - frac * a0 * g0, rtol=1e-6, atol=1e-6)
    assert not np.isfinite(trace[1][1]) and not np.isfinite(trace[2][1]) and np.isfinite(trace[3][1])
    assert trace[2][3]["iterations"] == 0 and trace[2][3]["pairs"] == 0
    # a NaN loss at a point whose gradient is finite is cut back the same way; only a finite, acceptable loss with a non-finite gradient is a status
    calls = {"n": 0}

    def overflowed(x):
        calls["n"] += 1
        f, g = fun0(x)
        return (f, np.full(3, np.inf)) if calls["n"] == 2 else (f, g)
    rec, _ = LC.drive(HostPort(emu), overflowed, 0.1 * x0, dict(OPTS, gtol=1e-4))
    assert rec["status_name"] == "nonfinite_grad" and rec["evaluations"] == 2


def test_start_points(emu):
    port = HostPort(emu)
    rec, _ = LC.drive(port, lambda x: (float("nan"), np.zeros(5)), np.ones(5), OPTS)
    assert rec["status_name"] == "nonfinite_start" and rec["evaluations"] == 1 and np.array_equal(port.x(), np.ones(5, dtype=np.float32))
    rec, _ = LC.drive(port, lambda x: (1.0, np.array([0.0, np.inf, 0, 0, 0])), np.ones(5), OPTS)
    assert rec["status_name"] == "nonfinite_start"
    rec, _ = LC.drive(port, lambda x: (2.0, np.zeros(5)), np.ones(5), OPTS)           # zero gradient: converged where it stands
    assert rec["status_name"] == "gtol" and rec["evaluations"] == 1 and rec["iterations"] == 0 and rec["f"] == 2.0
    assert np.array_equal(port.x(), np.ones(5, dtype=np.float32))


def test_calls_after_a_stop_change_no_byte(emu):
    fun, x0 = LC.chained_rosenbrock(9)
    for opts in (dict(OPTS, maxfun=6), dict(OPTS, maxiter=4), dict(OPTS, gtol=1e-2)):
        port = HostPort(emu)
        rec, _ = LC.drive(port, fun, x0, opts)
        assert rec["status"] != 0
        before = [b.raw.copy() for b in port.buffers()]
        for k in range(3):
            if k == 2:                     # whatever the caller hands over now
                port.put(np.full(9, 7.0, dtype=np.float32), np.array([-1e9, 0.0], dtype=np.float32))
                before = [b.raw.copy() for b in port.buffers()]
            port.advance()
            assert all(np.array_equal(a, b.raw) for a, b in zip(before, port.buffers()))
        assert port.status() == rec


def test_argument_errors_return_their_codes(emu):
    L = emu.lib
    from pinn_elastodynamics_amd.capi import LbfgsOptions, LbfgsRecord
    assert emu.lbfgs_state_bytes(100, 0) == 0 and emu.lbfgs_state_bytes(100, 65) == 0 and emu.lbfgs_state_bytes(0, 5) == 0
    nb = emu.lbfgs_state_bytes(100, 5)
    assert nb > 2 * 5 * 100 * 4 and emu.lbfgs_state_bytes(100, 6) > nb
    st = Guarded(nb)
    o = LbfgsOptions(5, 10, 10, 20, 0.0, 0.0)
    c = (ctypes.c_float * 1)(1.0)
    init = lambda state, nbytes, P, opt, co, ns: L.pinn_lbfgs_init(state, nbytes, P, ctypes.byref(opt) if opt is not None else None, co, ns, 1.0, None)
    assert init(None, nb, 100, o, c, 1) == -1 and init(st.ptr, nb, 100, None, c, 1) == -1 and init(st.ptr, nb, 100, o, None, 1) == -1
    assert init(st.ptr + 16, nb, 100, o, c, 1) == -8           # misaligned
    assert init(st.ptr, nb - 1, 100, o, c, 1) == -8            # short
    assert init(st.ptr, nb, 0, o, c, 1) == -5 and init(st.ptr, nb, 100, o, c, 0) == -5 and init(st.ptr, nb, 100, o, c, 129) == -5
    for h in (0, 65):
        assert init(st.ptr, nb, 100, LbfgsOptions(h, 10, 10, 20, 0.0, 0.0), c, 1) == -9
    assert init(st.ptr, nb, 100, o, c, 1) == 0
    buf = Guarded(400)
    assert L.pinn_lbfgs_advance(None, buf.ptr, buf.ptr, buf.ptr, None) == -1 and L.pinn_lbfgs_advance(st.ptr, None, buf.ptr, buf.ptr, None) == -1
    assert L.pinn_lbfgs_advance(st.ptr + 8, buf.ptr, buf.ptr, buf.ptr, None) == -8
    assert L.pinn_lbfgs_status(st.ptr, None, None) == -1 and L.pinn_lbfgs_status(None, ctypes.byref(LbfgsRecord()), None) == -1
    out = (ctypes.c_double * 4)()
    assert L.pinn_lbfgs_read_losses(st.ptr, 0, 1025, out, None) == -5 and L.pinn_lbfgs_read_losses(st.ptr, -1, 1, out, None) == -5
    n = ctypes.c_int(0)
    assert L.pinn_lbfgs_debug_read(st.ptr, 100, 65, None, None, None, 0, ctypes.byref(n), None) == -9
    assert L.pinn_lbfgs_debug_read(st.ptr, 101, 5, None, None, None, 0, ctypes.byref(n), None) == -8      # not the sizes it was initialised for
    assert st.guards_intact() and b"L-BFGS" in L.pinn_error_string(-8) and b"history" in L.pinn_error_string(-9)
