"""Shared pieces of the stream-target-set tests (pinn_stream_loss_grad_multi): the set shapes of the plate's pre-training losses
(pinn_elastodynamics_amd/plate_hole.py, PLATE:194-215) on random points, and the float64 oracle summed over the sets."""
import numpy as np

from oracle import plate_oracle as pl
from oracle import pinn_oracle as po

LBP, UBP = [0.0, 0.0, 0.0], [0.5, 0.5, 10.0]
NOUT = 5


def fresh_net(layers, rng, bias=0.2):
    W, b = po.xavier_init(layers, rng)
    return po.pack_params(W, [bias * rng.standard_normal(x.shape) for x in b])


def points(n, rng):
    return np.stack([rng.random(n) * 0.5, rng.random(n) * 0.5, rng.random(n) * 10.0], 1)


def _w(pairs):
    w = np.zeros((5, NOUT))
    for s, o in pairs:
        w[s, o] = 1.0
    return w


# weight patterns (stream, output) of plate_hole.py: which of the 25 pairs of a set count
DIST_PATTERNS = [
    ("DIST", _w([(0, o) for o in range(5)]), True),                 # value targets of all five outputs
    ("IC", _w([(3, 0), (3, 1)]), False),                            # (dD_u/dt)^2 + (dD_v/dt)^2, no targets
]
PART_PATTERNS = [
    ("IC", _w([(0, o) for o in range(5)] + [(3, 0), (3, 1)]), False),
    ("LF", _w([(0, 0), (0, 4)]), False),
    ("RT", _w([(0, 2), (0, 4)]), True),                             # s11 = traction target, s12 = 0
    ("LW", _w([(0, 1), (0, 4)]), False),
    ("UP", _w([(0, 3), (0, 4)]), False),
]


def make_sets(patterns, sizes, rng, poison=False, target_scale=1.0):
    """[(X [n,3] float64, targets [5, NOUT, n] float64 or None, weights [5, NOUT] = pattern / n)], as PINN builds them (mean squares: 1 / n).
    ``poison``: the copy handed to the library (see device_targets) carries NaN in every row whose weight is 0."""
    sets = []
    for (name, w, has_t), n in zip(patterns, sizes):
        X = points(n, rng)
        tg = None
        if has_t:
            tg = np.zeros((5, NOUT, n))
            for s, o in zip(*np.nonzero(w)):
                tg[s, o] = target_scale * rng.standard_normal(n)
        sets.append((X, tg, w / max(n, 1)))
    return sets


def device_targets(tg, w, poison):
    """float32 copy for the library; rows of weight 0 hold NaN when ``poison`` (the head must not read them into the result)"""
    if tg is None:
        return None
    out = np.ascontiguousarray(tg.astype(np.float32))
    if poison:
        out[w == 0] = np.nan
    return out


def oracle_sets(flat, layers, sets):
    """(per-set reported sums [m, NOUT] under the call's ONE normalisation, gradient of the unnormalised loss, loss) in float64"""
    wmax = max((float(np.abs(w).max()) for _, _, w in sets), default=0.0)
    sums = np.zeros((len(sets), NOUT))
    grad = np.zeros(flat.size)
    for k, (X, tg, w) in enumerate(sets):
        if X.shape[0] == 0:
            continue
        ss, g = pl.stream_loss_grad(flat, layers, X[:, 0], X[:, 1], X[:, 2], tg, w)
        sums[k] = ((w / wmax) * ss).sum(0)
        grad += g
    return sums, grad, wmax * sums.sum()


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def case_sets(c, kind, n=None, rng=None):
    """The sets PINN builds from a pointsets.plate_case() dict for loss_DIST (``kind`` = 'dist') or loss_PART ('part'), as
    (X, targets or None, weights); ``n``: a random subsample of that many points per set."""
    def sub(A):
        A = np.asarray(A, dtype=np.float64)
        if n is None or A.shape[0] <= n:
            return A
        return A[np.sort(rng.choice(A.shape[0], n, replace=False))]

    out = []
    if kind == "dist":
        D, IC = sub(c["DIST"]), sub(c["IC"])
        tg = np.zeros((5, NOUT, D.shape[0]))
        tg[0] = D[:, 3:8].T
        out.append((D[:, 0:3], tg, DIST_PATTERNS[0][1] / D.shape[0]))
        out.append((IC[:, 0:3], None, DIST_PATTERNS[1][1] / IC.shape[0]))
        return out
    IC = sub(c["IC"])
    out.append((IC[:, 0:3], None, PART_PATTERNS[0][1] / IC.shape[0]))
    for name, pat in (("LF", PART_PATTERNS[1][1]), ("RT", PART_PATTERNS[2][1]), ("LW", PART_PATTERNS[3][1]), ("UP", PART_PATTERNS[4][1])):
        A = sub(c[name])
        tg = None
        if name == "RT":
            tg = np.zeros((5, NOUT, A.shape[0]))
            tg[0, 2] = A[:, 3]
        out.append((A[:, 0:3], tg, pat / A.shape[0]))
    return out


def golden_net(golden_dir, key):
    w = np.load(f"{golden_dir}/weights_plate_{key}.npz")
    layers = [int(v) for v in w["layers"]]
    L = len(layers) - 1
    return layers, po.pack_params([w[f"W{i}"] for i in range(L)], [w[f"b{i}"] for i in range(L)])


def device_call(eng, flat, sets, dev, poison=False):
    """HipEngine.stream_loss_grad_multi on float64 host sets -> (sums [m, NOUT], grad) float64"""
    import torch

    def td(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    loss = torch.full((len(sets), 8), float("nan"), dtype=torch.float32, device=dev)
    rows = []
    for k, (X, tg, w) in enumerate(sets):
        t32 = device_targets(tg, w, poison)
        rows.append((td(X[:, 0]), td(X[:, 1]), td(X[:, 2]), None if t32 is None else td(t32), w.tolist(), loss[k]))
    grad = eng.stream_loss_grad_multi(td(flat), rows, LBP, UBP, False)
    torch.cuda.synchronize()
    return loss[:, :NOUT].cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)


def three_way(layers, flat, sets, dev, max_points=1 << 14):
    """Errors against the float64 oracle of (a) the fused call, (b) the same call under PINN_FLAG_TWO_KERNEL, (c) the fp32 mode, at the
    same points: dict name -> (loss error, gradient error); asserts with the path counters that each ran where it was meant to."""
    from pinn_elastodynamics_amd.hip_engine import HipEngine
    sums, g, _ = oracle_sets(flat, layers, sets)
    nonempty = sum(1 for X, _, _ in sets if X.shape[0])
    out = {}
    for name, prec, two, path, count in (("fused", "f16x3", False, "fused-registers", 1), ("two-kernel", "f16x3", True, "two-kernel", nonempty),
                                         ("fp32", "fp32", False, "fp32", nonempty)):
        eng = HipEngine(layers, precision=prec, device=dev, max_points=max_points)
        eng.two_kernel = two
        assert eng.path("stream_sets") == path, (name, eng.path("stream_sets"))
        eng.lib.path_counts(reset=True)
        s, gr = device_call(eng, flat, sets, dev, poison=(name == "fused"))
        cnt = eng.lib.path_counts(reset=True)
        assert cnt[path] == count and sum(cnt.values()) == count, (name, cnt)
        out[name] = (rel(s, sums), rel(gr, g))
    return out
