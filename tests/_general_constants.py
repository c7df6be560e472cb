"""Material constants and domains at which no two quantities of the physics heads coincide (shared by the tests that use them).

At the reference's E = 2.5, nu = 0.25, rho = 1 the plane-strain coefficients are c1 = 3, c2 = 1, G = 1: c2, G and rho are the same
float, and a head that reads one for another computes the same numbers.  Likewise every 2-D domain of the older tests has equal x and
y spans and offsets.  Here c1, c2, G and rho are pairwise distinct and none is 1, and every input has its own span and offset."""
import numpy as np

from oracle import pinn_oracle as po

# (E, nu, rho)
CONSTS = {
    "A": (7.3, 0.31, 1.7),        # plane strain / 3-D: c1 10.12, c2 4.55, G 2.79; plane stress: c1 8.08, c2 2.50
    "B": (40.0, 0.42, 0.35),      # stiff and light: c1 102, c2 74, G 14 -- adjoint seeds ~30x the reference's
}

# 2-D (x, y, t): spans 30 / 8 / 17, non-zero offsets
LB2, UB2 = [-4.0, 3.0, 0.5], [26.0, 11.0, 17.5]
# 3-D (x, y, z, t): spans 30 / 12 / 17 / 9
LB3, UB3 = [-3.0, 2.0, -17.0, 0.25], [27.0, 14.0, 0.0, 9.25]


def distinct(E, mu, rho, plane_strain=True):
    """c1, c2, G, rho pairwise distinct and none equal to 1 (the property the sets are chosen for)"""
    v = list(po.hooke_coeffs(E, mu, plane_strain)) + [rho]
    return all(abs(a - 1.0) > 0.1 for a in v) and all(abs(v[i] - v[j]) > 0.1 for i in range(4) for j in range(i))


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def one_hot_weights(tw):
    """one weight vector per residual term, with only that term's weight"""
    tw = np.asarray(tw, np.float64)
    out = []
    for i in range(tw.size):
        w = np.zeros_like(tw)
        w[i] = tw[i]
        out.append(w)
    return out


def check_terms(call, oracle, tw, tol_loss, tol_grad, per_term=True, tol_sum=1e-5):
    """call(weights) -> (loss sums, gradient) of the kernel under test; oracle(weights) -> (sums, gradient) of the float64 oracle.
    The full-weight call against the oracle at the path's bars; with ``per_term`` also one call per residual term (one-hot weights): its
    gradient against the oracle's gradient of that term alone, relative to that term's own norm -- a wrong coefficient in one adjoint
    entry is an O(1) error there, where it is diluted in the norm of the whole gradient -- and the per-term gradients add up to the full
    one.  A single term's gradient can be a sum with more cancellation than the whole (the momentum terms: ~1.1x the path's error at
    the full weights, measured), so the per-term gradient bar is 3x the path's: still ~1e4 below what a wrong coefficient gives."""
    ss, g = oracle(tw)
    loss, grad = call(tw)
    errs = [("all", rel(loss, ss), rel(grad, g))]
    gsum = None
    if per_term:
        gsum = np.zeros(g.size)
        for i, w in enumerate(one_hot_weights(tw)):
            l_i, g_i = call(w)
            errs.append((i, rel(l_i, ss), rel(g_i, oracle(w)[1])))
            gsum += g_i
    bad = [e for e in errs if not (e[1] < tol_loss and e[2] < (tol_grad if e[0] == "all" else 3 * tol_grad))]
    assert not bad, f"(term, loss err, grad err) over the bars {tol_loss:g} / {tol_grad:g}: {bad}"
    if gsum is not None:
        assert rel(gsum, grad.astype(np.float64)) < tol_sum, rel(gsum, grad.astype(np.float64))
    return errs
