"""Shared by tests/test_emulated_lbfgs.py (host arrays through the x86 emulator build) and tests/test_gpu_lbfgs.py (device buffers through
HipEngine): the test problems, the float64 two-loop reference and a driver that evaluates f and g in numpy between pinn_lbfgs_advance calls.

A `port` is the thin adapter the two files give the driver:
    port.start(x0, options, coeffs, grad_scale)   allocate state / params / grad / sums and call pinn_lbfgs_init
    port.put(grad, sums)                          hand one evaluation over
    port.advance()  port.status() -> dict  port.x() -> fp32 numpy copy of params  port.debug() -> (d, S, Y)  port.losses(first, count)
"""
import numpy as np


def two_loop_direction(g, S, Y):
    """-H g by the two-loop recursion in float64 on the stored pairs (oldest first), H0 = (s.y / y.y of the newest pair) I"""
    g = np.asarray(g, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    q = g.copy()
    k = S.shape[0]
    rho = [1.0 / float(Y[i] @ S[i]) for i in range(k)]
    al = [0.0] * k
    for i in reversed(range(k)):
        al[i] = rho[i] * float(S[i] @ q)
        q -= al[i] * Y[i]
    if k:
        q *= float(S[-1] @ Y[-1]) / float(Y[-1] @ Y[-1])
    for i in range(k):
        be = rho[i] * float(Y[i] @ q)
        q += (al[i] - be) * S[i]
    return -q


def fp32_rounding_error(v):
    """relative L2 error of merely rounding a float64 vector to fp32"""
    v = np.asarray(v, dtype=np.float64)
    return float(np.linalg.norm(v.astype(np.float32).astype(np.float64) - v) / np.linalg.norm(v))


def quadratic(P, cond, seed):
    rng = np.random.default_rng(seed)
    a = np.logspace(0.0, np.log10(cond), P)
    b = rng.standard_normal(P)

    def fun(x):
        return 0.5 * float(x @ (a * x)) - float(b @ x), a * x - b
    return fun, rng.standard_normal(P)


def smooth_convex(P, seed):
    """a strictly convex non-quadratic: the curvature changes along the run, so every pair matters"""
    rng = np.random.default_rng(seed)
    a = np.logspace(0.0, 2.0, P)
    c = rng.standard_normal(P)

    def fun(x):
        z = x - c
        return 0.5 * float(z @ (a * z)) + 0.25 * float(np.sum(z ** 4)), a * z + z ** 3
    return fun, rng.standard_normal(P)


def chained_rosenbrock(P):
    def fun(x):
        a, b = x[:-1], x[1:]
        f = float(np.sum(100.0 * (b - a * a) ** 2 + (1.0 - a) ** 2))
        g = np.zeros_like(x)
        g[:-1] += -400.0 * a * (b - a * a) - 2.0 * (1.0 - a)
        g[1:] += 200.0 * (b - a * a)
        return f, g
    return fun, np.full(P, -1.2) * (1.0 + 0.05 * np.arange(P) / P)


def drive(port, fun, x0, options, max_calls=20000, until=None, after_each=None, grad_scale=1.0):
    """Evaluate fun at the port's parameters (as float64 of the fp32 values), advance, read the status; the loss travels as two fp32 sums with
    coefficients (1, 1); stops at a non-running status, when
    `until(record)` says so, or after max_calls.  ``grad_scale`` = k: the optimizer minimises k * fun (coefficients (k, k), gradient scale k), as
    the plate's pre-training stages do with k = 1000; f and g of the trace stay fun's own.  Returns (record, trace): trace[i] = (x32, f, g32, record after the advance)."""
    port.start(np.asarray(x0, dtype=np.float32), options, [float(grad_scale)] * 2, float(grad_scale))
    trace = []
    rec = None
    for _ in range(max_calls):
        x = port.x()
        f, g = fun(x.astype(np.float64))
        g32 = np.asarray(g, dtype=np.float32)
        hi = np.float32(f)                 # the loss as two fp32 sums (high part + remainder): the device adds them in fp64
        port.put(g32, np.array([hi, np.float32(f - float(hi))], dtype=np.float32))
        port.advance()
        rec = port.status()
        trace.append((x, float(hi) + float(np.float32(f - float(hi))), g32, rec))
        if after_each is not None:
            after_each(rec)
        if rec["status"] != 0 or (until is not None and until(rec)):
            break
    return rec, trace


def accepted(trace):
    """the trace entries of the accepted points, in order: the first evaluation and every one after which `iterations` went up"""
    return [t for i, t in enumerate(trace) if i == 0 or t[3]["iterations"] > trace[i - 1][3]["iterations"]]


def scaled_direction_check(port, trace, grad_scale):
    """(difference to the float64 two-loop direction, fp32 rounding error of that reference, stored pairs == fp32 differences of the accepted
    points) with the optimizer's gradient gn = fl32(grad_scale * g) and y = fl32(gn_new - gn_old) as two separately rounded fp32 operations"""
    gs = np.float32(grad_scale)
    d, S, Y = port.debug()
    acc = accepted(trace)
    gn = [gs * t[2] for t in acc]                         # fp32 products
    ref = two_loop_direction(gn[-1], S, Y)
    diff = float(np.linalg.norm(d.astype(np.float64) - ref) / np.linalg.norm(ref))
    k = S.shape[0]
    same = all(np.array_equal(S[-1 - i], acc[-1 - i][0] - acc[-2 - i][0]) and np.array_equal(Y[-1 - i], gn[-1 - i] - gn[-2 - i]) for i in range(k))
    return diff, fp32_rounding_error(ref), same


def accepted_gradient(trace):
    """fp32 gradient at the last accepted point: the evaluation after which `iterations` last went up (or the first evaluation)"""
    it, g = 0, trace[0][2]
    for _, _, g32, rec in trace:
        if rec["iterations"] > it:
            it, g = rec["iterations"], g32
    return g
