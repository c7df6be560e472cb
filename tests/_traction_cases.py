"""Shared by tests/test_emulated_traction.py, tests/test_traction_host.py and tests/test_gpu_traction.py: the float64 reference of the wave
family's traction boundary term (pinn_wave2d_traction_loss_grad, INF:267-276) and the inputs the tests feed it.

The reference is built from oracle.pinn_oracle.mlp_forward_tangent / mlp_backward (the oracle's own forward and reverse pass; nothing under
oracle/ changes for it); tests/test_traction_host.py holds it to torch float64 autograd once.

Inputs everywhere: Xavier weights with 0.3 N(0,1) biases (as the data-head tests), random unit normals, N(0,1) targets -- residuals of
order one, no term trivially small --, and two unequal weights."""
import numpy as np

from oracle import pinn_oracle as po

LB, UB = [0.0, 0.0, 0.0], [30.0, 30.0, 20.0]
S11, S22, S12 = 4, 5, 6      # the stress outputs of the wave net (u, v, ut, vt, s11, s22, s12)


def traction_reference(params, layers, x, y, t, lb, ub, normalize, aux, weights):
    """(sums [2] = sum r_x^2, sum r_y^2; grad_flat of weights[0] sums[0] + weights[1] sums[1]; r [n, 2]) in float64.
    aux [4, n] = nx, ny, tx, ty;  r_x = s11 nx + s12 ny - tx,  r_y = s12 nx + s22 ny - ty."""
    params = np.asarray(params, dtype=np.float64)
    Ws, bs = po.unpack_params(params, layers)
    X = np.stack([np.asarray(v, dtype=np.float64).reshape(-1) for v in (x, y, t)], 1)
    Y, _, cache = po.mlp_forward_tangent(X, Ws, bs, lb, ub, normalize, n_tangent=0)
    nx, ny, tx, ty = (np.asarray(a, dtype=np.float64) for a in aux)
    rx = Y[:, S11] * nx + Y[:, S12] * ny - tx
    ry = Y[:, S12] * nx + Y[:, S22] * ny - ty
    gx, gy = 2.0 * weights[0] * rx, 2.0 * weights[1] * ry
    Ybar = np.zeros_like(Y)
    Ybar[:, S11], Ybar[:, S22], Ybar[:, S12] = gx * nx, gy * ny, gx * ny + gy * nx
    Wbar, bbar = po.mlp_backward(Ybar, [], Ws, cache)
    return np.array([(rx * rx).sum(), (ry * ry).sum()]), po.pack_params(Wbar, bbar), np.stack([rx, ry], 1)


def make_net(layers, rng):
    """flat float64 parameters: Xavier weights, 0.3 N(0,1) biases"""
    Ws, bs = po.xavier_init(layers, rng)
    return po.pack_params(Ws, [0.3 * rng.standard_normal(b.shape) for b in bs])


def make_set(n, rng, lb=LB, ub=UB):
    """(X [n, 3] in the box, aux [4, n] float32: random unit normals, N(0,1) targets)"""
    X = np.asarray(lb) + (np.asarray(ub) - np.asarray(lb)) * rng.random((n, 3))
    th = 2.0 * np.pi * rng.random(n)
    aux = np.stack([np.cos(th), np.sin(th), rng.standard_normal(n), rng.standard_normal(n)]).astype(np.float32)
    return X, np.ascontiguousarray(aux)


def weights_for(n):
    """two unequal weights of the size a mean over the set gives"""
    return [1.0 / n, 2.5 / n]


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
