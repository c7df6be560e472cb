"""What the three model classes use and is not a model class: the flat parameter layout (pack_params / unpack_params), Xavier initialisation,
host columns to device tensors, the range ladder around an evaluation (evaluate_with_finite_gradient / relax_adjoint_shift), the step's one
collective (all_reduce_sum) and the L-BFGS stage: lbfgs_stage runs one stage on any of the three backends -- scipy's L-BFGS-B on the host,
torch.optim.LBFGS on the device (lbfgs_on_device), the library's own optimizer (lbfgs_hip).
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch



def _col(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))


def device_array(a, device):
    """a numpy array of any shape -> contiguous fp32 device tensor of that shape"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def device_column(a, device):
    """a numpy column ([N,1] or [N]) or a device tensor -> contiguous fp32 device tensor [N]"""
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    return device_array(_col(a), device)


def truncated_normal(rng: np.random.Generator, shape, stddev: float) -> np.ndarray:
    """tf.truncated_normal (INF:156): normal draws, redrawn while |z| > 2 standard deviations"""
    W = rng.standard_normal(shape)
    bad = np.abs(W) > 2.0
    while bad.any():
        W[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(W) > 2.0
    return (W * stddev).astype(np.float32)


def xavier_init(layers: Sequence[int], rng: np.random.Generator):
    """initialize_NN / xavier_init (INF:141-156) as one function of a layer list and a generator: truncated normal (|z| <= 2) times
    sqrt(2/(in+out)), zero biases of shape [1, out].  The build's own seeded stream (TF1's is
    not reproducible).  The model classes also carry the reference's two METHODS (net_api.NetApi)."""
    Ws, bs = [], []
    for i in range(len(layers) - 1):
        n_in, n_out = layers[i], layers[i + 1]
        Ws.append(truncated_normal(rng, (n_in, n_out), float(np.sqrt(2.0 / (n_in + n_out)))))
        bs.append(np.zeros((1, n_out), dtype=np.float32))
    return Ws, bs


def pack_params(weights, biases) -> np.ndarray:
    """[W_list, b_list] -> flat fp32 vector W0,b0,W1,b1,... (the C-ABI layout)."""
    parts = []
    for W, b in zip(weights, biases):
        parts += [np.asarray(W, dtype=np.float32).reshape(-1), np.asarray(b, dtype=np.float32).reshape(-1)]
    return np.concatenate(parts)


def unpack_params(flat, layers):
    Ws, bs, o = [], [], 0
    flat = np.asarray(flat)
    for i in range(len(layers) - 1):
        n_in, n_out = layers[i], layers[i + 1]
        Ws.append(flat[o:o + n_in * n_out].reshape(n_in, n_out).copy())
        o += n_in * n_out
        bs.append(flat[o:o + n_out].reshape(1, n_out).copy())
        o += n_out
    assert o == flat.size
    return Ws, bs


def evaluate_with_finite_gradient(engine, evaluate, n_params, state, device_check=0, check=None):
    """Run ``evaluate()`` (it fills and returns the device buffer [grad | sums]) and bring the result to the host.  The 16-bit
    reverse pass can overflow when residuals are orders of magnitude above their trained size (include/pinn_hip.h,
    PINN_ADJOINT_SHIFT); the sums of squares are still right then, only the gradient is non-finite.  In that case the adjoint
    shift of the engine is raised by 4 (x1/16) and the evaluation repeated; once the loss has fallen 256-fold below where the shift
    was raised, it is lowered again.  ``state`` is a dict the caller keeps between evaluations.  ``device_check=P``: test the first P
    entries on the device and return only the sums behind them.  Deterministic in every rank of a
    data-parallel job (all ranks see the same reduced buffer).  ``check``: called behind the host synchronisation of every evaluation,
    BEFORE the result is looked at -- the model classes pass the status check of their collective (a failed P2P all-reduce leaves NaN in the
    buffer: that must raise as a collective failure, not climb this ladder)."""
    for _ in range(7):
        buf = evaluate().detach()
        if device_check:         # gradient stays on the device: check it there, bring only the loss sums back
            finite = bool(torch.isfinite(buf[:device_check]).all())
            if check is not None:
                check()
            if finite:
                return buf[device_check:].cpu().numpy()
        else:
            host = buf.cpu().numpy()
            if check is not None:
                check()
            if np.isfinite(host[:n_params]).all():
                return host
        # a weight beyond the fused kernels' format (|w| <= 2047) poisons the whole result with NaN: leave the fused path and repeat
        leave = getattr(engine, "leave_fused_path_if_weights_out_of_range", None)
        if leave is not None and state.get("theta") is not None and leave(state["theta"]):
            continue
        if engine.adjoint_shift >= 24:
            break
        engine.adjoint_shift = min(engine.adjoint_shift + 4, 24)
        state["raised_at"] = None                    # filled with the loss of the next successful evaluation
    raise FloatingPointError("non-finite gradient even with the reverse pass scaled by 2^-24")


def relax_adjoint_shift(engine, loss, state):
    """Companion of evaluate_with_finite_gradient: call with the loss of every successful evaluation."""
    if engine.adjoint_shift == 0:
        return
    if state.get("raised_at") is None:
        state["raised_at"] = loss
    elif loss < state["raised_at"] / 256.0:
        engine.adjoint_shift -= 4
        state["raised_at"] = loss


def all_reduce_sum(buf, group, events=None, p2p=None, adam=None, n_params=0):
    """The step's one collective: all-reduce(sum) of the fused buffer [gradient | loss sums], enqueued in stream order behind the kernels that
    filled it.  Default: torch.distributed.all_reduce (RCCL under the "nccl" backend).  ``p2p`` (a p2p.P2PAllReduce): the library's one-shot
    kernel over IPC-mapped peer buffers instead; with ``adam = (params, m, v, lr, step)`` it also applies the Adam update to the first
    ``n_params`` entries of the sum -- returns True then.  ``events``: a list that receives one (start, end) pair of timing events per call,
    recorded on the current stream around the collective (with RCCL the stream waits for the communicator's own stream, so the pair brackets
    it) -- bench.py's ``allreduce_ms``; None (default): nothing is recorded."""
    if events is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    folded = False
    if p2p is not None:
        p2p.all_reduce(buf, adam=adam, n_params=n_params)
        folded = adam is not None
    else:
        torch.distributed.all_reduce(buf, op=torch.distributed.ReduceOp.SUM, group=group)
    if events is not None:
        ev[1].record()
        events.append(ev)
    return folded


def lbfgs_on_device(theta, loss_and_grad, options, callback=None):
    """The L-BFGS stage without the host in the loop: ``torch.optim.LBFGS`` (two-loop recursion with ``maxcor`` correction pairs and a
    strong-Wolfe line search, all vector work on the GPU in fp32) drives the same kernels.  ``loss_and_grad()`` evaluates at the current
    ``theta`` and returns (loss as float, gradient device tensor).  scipy's L-BFGS-B -- what the reference uses through
    ScipyOptimizerInterface -- spends ~35 ms per iteration on a 35 k-parameter net with 50 pairs, ten times the kernels' time; this is
    the opt-in alternative (``train_bfgs(..., backend="torch")``).  The iterates differ from scipy's (another line search), the
    objective and its gradient do not."""
    p = theta.detach().clone().requires_grad_(True)
    opt = torch.optim.LBFGS([p], lr=1.0, max_iter=int(options.get("maxiter", 1000)), max_eval=int(options.get("maxfun", 1250)),
                            history_size=int(options.get("maxcor", 50)), tolerance_grad=float(options.get("gtol", 1e-10)),
                            tolerance_change=float(options.get("tolerance_change", 1e-14)), line_search_fn="strong_wolfe")
    stats = {"nfev": 0, "fun": None}

    def closure():
        theta.copy_(p.detach())
        loss, grad = loss_and_grad()
        p.grad = grad.detach().clone()
        stats["nfev"] += 1
        stats["fun"] = loss
        if callback is not None:
            callback(loss)
        return torch.tensor(loss, dtype=torch.float32, device=theta.device)

    opt.step(closure)
    theta.copy_(p.detach())
    final = loss_and_grad()[0]                       # the optimizer's last point is not necessarily its last evaluation
    stats["fun"] = final
    stats["nit"] = opt.state[p].get("n_iter", 0)
    return stats


BFGS_BACKENDS = ("scipy", "torch", "hip")


def check_backend(backend):
    if backend not in BFGS_BACKENDS:
        raise ValueError(f"backend must be one of {BFGS_BACKENDS}, not {backend!r}")


class LbfgsResult(dict):
    """What a device L-BFGS stage returns: fun, nit, nfev, status, message, success -- the fields of scipy's OptimizeResult a caller of
    train_bfgs looks at (the parameters stay on the device, in the model's theta)."""
    __getattr__ = dict.get


_LBFGS_MESSAGES = {1: "CONVERGENCE: max|g| <= gtol", 2: "CONVERGENCE: relative reduction of f <= ftol", 3: "STOP: total no. of iterations reached limit",
                   4: "STOP: total no. of f and g evaluations reached limit", 5: "ABNORMAL: line search failed",
                   6: "ABNORMAL: loss or gradient not finite at the start point", 7: "ABNORMAL: gradient not finite at an acceptable point"}


def lbfgs_hip(engine, theta, evaluate, n_params, loss_coeffs, options, callback=None, grad_scale=1.0, loss_scale=1.0, block=16, check=None,
              shift_state=None, ladder=True, what="this stage"):
    """The L-BFGS stage as a stream of kernels (``backend="hip"``): the library's own optimizer (pinn_lbfgs_*, include/pinn_hip.h: compact-form
    direction, strong-Wolfe line search and scipy's stop rules, all on the device) behind the same loss kernels.  ``evaluate()`` enqueues the
    loss + gradient kernels at ``theta`` and returns the device buffer [grad (n_params) | sums]; the loss the optimizer sees is
    ``sum_j loss_coeffs[j] * sums[j]`` and its gradient ``grad_scale * grad``.  Nothing synchronises per evaluation: *evaluate -> advance* is
    enqueued in blocks of ``block`` evaluations (``options["block"]`` overrides), the status is read ONCE per block, and the block's losses come
    out of the device's loss ring -- so ``callback(loss / loss_scale)`` still fires once per evaluation, in order, but in BATCHES of up to
    ``block`` calls, after the block has run.  When the status says stop, nothing more is enqueued (the calls of a block that were already behind
    the stop change nothing); ``theta`` then holds the last accepted point, which is the best one.  ``check``: called at every status read (the
    model classes pass their collective's status check).  A stop with a non-finite gradient climbs the range ladder of
    evaluate_with_finite_gradient (leave the fused path for an out-of-range weight, else adjoint shift + 4) and starts again from the last
    accepted point with an empty history and what is left of maxiter / maxfun; with ``shift_state`` (the model's bookkeeping dict) the shift is
    lowered again as the loss falls (relax_adjoint_shift, at every status read -- once per block instead of once per evaluation).
    ``ladder=False``: the evaluation has no range ladder (the plate's pre-training losses ignore the adjoint shift): a non-finite loss or gradient
    raises FloatingPointError at once, naming ``what``.  Returns an LbfgsResult (fun, nit, nfev, status, message)."""
    opts = dict(options)
    block = max(1, min(int(opts.pop("block", block)), 1024))
    maxfun, maxiter = int(opts.get("maxfun", 15000)), int(opts.get("maxiter", 15000))
    opts.setdefault("gtol", 1e-5)                        # scipy's default pgtol (the reference does not set it)
    state = engine.lbfgs_state(n_params, int(opts.get("maxcor", 10)))
    nfev = nit = 0
    while True:
        engine.lbfgs_init(state, dict(opts, maxfun=max(1, maxfun - nfev), maxiter=max(0, maxiter - nit)), loss_coeffs, grad_scale)
        seen = 0
        while True:
            for _ in range(max(1, min(block, maxfun - nfev - seen))):
                buf = evaluate()
                engine.lbfgs_advance(state, theta, buf[:n_params], buf[n_params:])
            rec = engine.lbfgs_status(state)
            if check is not None:
                check()
            if callback is not None:
                for f in engine.lbfgs_losses(state, seen, rec["loss_pos"] - seen):
                    callback(f / loss_scale)
            seen = rec["loss_pos"]
            if shift_state is not None and np.isfinite(rec["f"]):
                relax_adjoint_shift(engine, rec["f"] / loss_scale, shift_state)
            if rec["status"] != 0:
                break
        nfev += rec["evaluations"]
        nit += rec["iterations"]
        if rec["status"] in (6, 7) and not ladder:
            raise FloatingPointError(f"{what} produced a non-finite loss or gradient (loss = {rec['f'] / loss_scale}); "
                                     f"restart from other weights or use precision='bf16x3'")
        if rec["status"] in (6, 7):
            leave = getattr(engine, "leave_fused_path_if_weights_out_of_range", None)
            if leave is not None and leave(theta):
                pass
            elif engine.adjoint_shift < 24:
                engine.adjoint_shift = min(engine.adjoint_shift + 4, 24)
                if shift_state is not None:
                    shift_state["raised_at"] = None
            else:
                raise FloatingPointError("non-finite loss or gradient even with the reverse pass scaled by 2^-24")
            if nfev < maxfun:
                continue
        break
    return LbfgsResult(fun=rec["f"], nit=nit, nfev=nfev, status=rec["status"], message=_LBFGS_MESSAGES.get(rec["status"], "?"),
                       success=rec["status"] in (1, 2), max_abs_grad=rec["max_abs_grad"], pairs=rec["pairs"], skipped=rec["skipped"])


def lbfgs_stage(backend, engine, theta, evaluate, loss_of_sums, loss_coeffs, options, callback, check, shift_state):
    """One L-BFGS stage over the flat parameter tensor ``theta`` (updated in place) on ``backend``: "scipy" = L-BFGS-B on the host over a
    float64 copy, loss and gradient from the device; "torch" = lbfgs_on_device; "hip" = lbfgs_hip.  ``evaluate()`` enqueues the loss + gradient
    kernels at ``theta`` and returns the device buffer [grad (theta.numel()) | sums]; ``loss_of_sums(host sums)`` is the loss, and
    ``loss_coeffs`` the same loss as a coefficient vector over the sums (what "hip" hands to the library).  Every evaluation the host looks at
    runs the range ladder (evaluate_with_finite_gradient with ``check`` and ``shift_state``, then relax_adjoint_shift); ``callback(loss)`` fires
    once per evaluation.  Returns scipy's OptimizeResult, lbfgs_on_device's dict or an LbfgsResult."""
    P = theta.numel()
    if backend == "hip":
        return lbfgs_hip(engine, theta, evaluate, P, loss_coeffs, options, callback, check=check, shift_state=shift_state)
    if backend == "torch":
        last = []

        def evaluate_and_keep():
            last[:] = [evaluate()]
            return last[0]

        def loss_and_grad():
            sums = evaluate_with_finite_gradient(engine, evaluate_and_keep, 0, shift_state, device_check=P, check=check)
            loss = loss_of_sums(sums)
            relax_adjoint_shift(engine, loss, shift_state)
            return loss, last[0][:P]
        return lbfgs_on_device(theta, loss_and_grad, options, callback)

    def fun(theta64):
        theta.copy_(torch.from_numpy(theta64.astype(np.float32)).to(theta.device))
        host = evaluate_with_finite_gradient(engine, evaluate, P, shift_state, check=check)
        loss = loss_of_sums(host[P:])
        relax_adjoint_shift(engine, loss, shift_state)
        callback(loss)
        return loss, host[:P].astype(np.float64)

    import scipy.optimize
    x0 = theta.detach().cpu().numpy().astype(np.float64)
    result = scipy.optimize.minimize(fun, x0, jac=True, method='L-BFGS-B', options=options)
    theta.copy_(torch.from_numpy(result.x.astype(np.float32)).to(theta.device))
    return result
