"""Device engine: PyTorch owns HBM buffers and streams, libpinn_hip.so does the work.

This is the only place the product touches the GPU kernels.  There is NO CPU fallback: without a
GPU or without the built shared library, construction raises.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from .capi import DEFAULT_LIB, FLAG_STATE_FP16, FLAG_TWO_KERNEL, FLAG_WEIGHTS_PACKED, MATERIAL_SUMS, MATERIAL_SUMS_NC3D, MATERIAL_SUMS_PLATE, MAX_TIME_BINS, PREC, PinnLib, PinnLibError, adjoint_shift


def param_count(layers: Sequence[int]) -> int:
    return sum(layers[i] * layers[i + 1] + layers[i + 1] for i in range(len(layers) - 1))


def aligned_buffer(nbytes: int, device):
    """(byte tensor, pointer): ``nbytes`` behind a 256-byte aligned pointer, what every workspace and state argument of include/pinn_hip.h asks for"""
    buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
    return buf, (buf.data_ptr() + 255) // 256 * 256


class LbfgsState:
    """The caller-owned state buffer of pinn_lbfgs_* (include/pinn_hip.h): a byte tensor and its 256-byte aligned window"""

    def __init__(self, lib, device, n_params: int, history: int):
        self.n_params, self.history = int(n_params), int(history)
        self.nbytes = lib.lbfgs_state_bytes(n_params, history)
        if self.nbytes == 0:
            raise PinnLibError(f"no L-BFGS state for n_params={n_params}, history={history} (history must be 1..64)")
        self.buf, self.ptr = aligned_buffer(self.nbytes, device)


class LbfgsMixin:
    """pinn_lbfgs_* on tensors of ``self.device`` through ``self.lib`` (a capi.PinnLib), enqueued on ``self._stream()``.  HipEngine is the product's
    user; the only synchronising methods are lbfgs_status / lbfgs_losses / lbfgs_debug."""

    def lbfgs_state(self, n_params: int, history: int) -> LbfgsState:
        return LbfgsState(self.lib, self.device, n_params, history)

    def lbfgs_init(self, state: LbfgsState, options: dict, loss_coeffs, grad_scale: float = 1.0):
        """options: scipy's names (maxcor = state.history, maxiter, maxfun, maxls, ftol, gtol); loss = sum_j loss_coeffs[j] * sums[j]"""
        self.lib.lbfgs_init(state.ptr, state.nbytes, state.n_params, dict(options, maxcor=state.history), loss_coeffs, grad_scale, self._stream())

    def lbfgs_advance(self, state: LbfgsState, params: torch.Tensor, grad: torch.Tensor, sums: torch.Tensor):
        """Consumes the evaluation at ``params`` (grad, sums) and writes the next point to evaluate into ``params``.  Asynchronous."""
        for a in (params, grad):
            assert a.dtype == torch.float32 and a.is_contiguous() and a.numel() == state.n_params and a.device.type == self.device.type
        assert sums.dtype == torch.float32 and sums.is_contiguous()
        self.lib.lbfgs_advance(state.ptr, params.data_ptr(), grad.data_ptr(), sums.data_ptr(), self._stream())

    def lbfgs_status(self, state: LbfgsState) -> dict:
        return self.lib.lbfgs_status(state.ptr, self._stream())

    def lbfgs_losses(self, state: LbfgsState, first: int, count: int):
        return self.lib.lbfgs_read_losses(state.ptr, first, count, self._stream())

    def lbfgs_debug(self, state: LbfgsState):
        return self.lib.lbfgs_debug_read(state.ptr, state.n_params, state.history, self._stream())


class HipEngine(LbfgsMixin):
    """loss/gradient, fields and Adam on one GPU, on flat fp32 parameter vectors.

    All tensors are fp32 CUDA(HIP) tensors; points are SoA (x, y, t).  Methods enqueue on the
    current torch stream and return device tensors without synchronising.
    """

    def __init__(self, layers: Sequence[int], precision: str = "f16x3", device: Optional[torch.device] = None,
                 max_points: int = 1 << 18, lib_path: str = DEFAULT_LIB, workspace_bytes: Optional[int] = None,
                 workspace_cap_bytes: int = 8 << 30, fast_state: bool = False):
        if not torch.cuda.is_available():
            raise PinnLibError("HipEngine needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.lib = PinnLib(lib_path)
        self.layers = [int(v) for v in layers]
        self.precision = precision
        # fast_state: PINN_FLAG_STATE_FP16 -- the fused 8-layer collocation kernel parks its states as fp16 only: 17 % faster, but the
        # gradient at trained weights loses accuracy by cancellation (DESIGN_HISTORY.md section 6).  Off by default.
        self.fast_state = bool(fast_state)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.n_params = param_count(self.layers)
        self.adjoint_shift = 0
        self.two_kernel = False               # PINN_FLAG_TWO_KERNEL on every call (set by leave_fused_path_if_weights_out_of_range)
        self.needs_finite_probe = True        # 16-bit reverse pass: the model classes check the first gradient (PINN_ADJOINT_SHIFT)
        if self.lib.supported_width(self.layers[1]) == 0:
            raise PinnLibError(f"hidden width {self.layers[1]} is not supported by the compiled kernels")
        want = workspace_bytes if workspace_bytes is not None else self.lib.workspace_bytes(self.layers, max_points, precision)
        if workspace_bytes is None:
            # larger point sets are walked in several passes; the default cap of 8 GiB already amortises the launches
            # (``workspace_cap_bytes`` raises or lowers it, ``workspace_bytes`` fixes the size outright)
            want = min(want, int(workspace_cap_bytes))
        want = max(want, self.lib.min_workspace_bytes(self.layers, precision))
        if want == 0:
            raise PinnLibError(f"no kernel variant for layers={self.layers} precision={precision}")
        self.ws_bytes = int(want)
        self.ws, self._ws_ptr = aligned_buffer(self.ws_bytes, self.device)
        self._lib_path = lib_path

    def for_layers(self, layers: Sequence[int]) -> "HipEngine":
        """A sibling engine for a net of other layer sizes (same precision mode, device and library): neural_net(X, weights, biases) of
        the model classes on weights that are not the model's own net (INF:188-199 takes any weight list)."""
        return HipEngine(layers, precision=self.precision, device=self.device, max_points=1 << 16, lib_path=self._lib_path, fast_state=self.fast_state)

    # ------------------------------------------------------------------------------------------
    def _mode(self, packed: bool) -> int:
        """precision_mode argument of the loss / gradient calls: the precision, PINN_FLAG_WEIGHTS_PACKED when the previous call of this
        engine used the same parameter values (skip the repack launch), and the current adjoint shift (``self.adjoint_shift``, see
        PINN_ADJOINT_SHIFT in include/pinn_hip.h; the model classes adapt it when a gradient comes back non-finite)."""
        return (self._forward_mode(packed) | (FLAG_STATE_FP16 if self.fast_state else 0)
                | (FLAG_TWO_KERNEL if self.two_kernel else 0) | adjoint_shift(self.adjoint_shift))

    def _forward_mode(self, packed: bool) -> int:
        """precision_mode argument of the forward-only score and predict calls: the precision and PINN_FLAG_WEIGHTS_PACKED, no other flag"""
        return PREC[self.precision] | (FLAG_WEIGHTS_PACKED if packed else 0)

    def leave_fused_path_if_weights_out_of_range(self, params: torch.Tensor) -> bool:
        """The fused kernels' weight format holds |w| <= 2047 (include/pinn_hip.h); beyond it a call returns NaN throughout.  Called by the
        model classes when a result comes back non-finite: if a weight is out of range, this engine's calls switch to the two-kernel path
        (PINN_FLAG_TWO_KERNEL) for good and True is returned -- the caller repeats its evaluation.  Synchronises (one reduction)."""
        if self.two_kernel or self.precision != "f16x3":      # (bf16x3: the fused format has fp32's range, nothing to leave for)
            return False
        if float(params.detach().abs().max()) <= self.lib.fused_weight_limit():
            return False
        self.two_kernel = True
        return True

    def path(self, head: str = "wave") -> str:
        """Which kernel path this engine's loss + gradient calls of family ``head`` take ('fused-registers', 'fused-lds', 'two-kernel',
        'fp32'): pinn_path_for with this engine's layer list, precision mode word and workspace size (include/pinn_hip.h)."""
        return self.lib.path_for(self.layers, self._mode(False), head, self.ws_bytes)

    def warn_if_slow_path(self, head: str = "wave") -> None:
        """One warning per engine and family when the calls land on the two-kernel path (2.3-5x slower than the fused kernel): the fused
        kernel is compiled for the depths the reference's scripts use, any other layer list still WORKS, just not at the published speed."""
        seen = self.__dict__.setdefault("_slow_path_warned", set())
        if head in seen:
            return
        if self.path(head) == "two-kernel" and not self.two_kernel:
            import warnings
            seen.add(head)
            warnings.warn(f"layers {self.layers} ({self.precision}, '{head}' calls) run on the two-kernel path (chain_kernel + wgrad_kernel): "
                          f"2.3-5x slower than the fused persistent kernel, which is compiled for 4 or 8 hidden layers of width <= 64 (the "
                          f"'stream_sets' calls of the plate's pre-training: 4), 8 of width <= 128, 6 of width <= 160 and the 10 x 128 3-D net -- or the workspace is too small for its scratch images "
                          f"(pinn_path_for, include/pinn_hip.h)", RuntimeWarning, stacklevel=3)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- argument marshalling shared by the methods below -------------------------------------------------------------
    @staticmethod
    def _chk(t: torch.Tensor, n: Optional[int] = None):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "expect contiguous fp32 device tensors"
        if n is not None:
            assert t.numel() == n, f"expected {n} elements, got {t.numel()}"

    def _check(self, params, cols) -> int:
        """The checks of every method that takes point columns (x, y, t) or (x, y, z, t): contiguous fp32 device tensors of one length, and
        ``params`` one of n_params elements.  Returns the number of points."""
        n = cols[0].numel()
        for v in cols:
            self._chk(v, n)
        self._chk(params, self.n_params)
        return n

    def _optional(self, t: Optional[torch.Tensor], numel: int) -> int:
        """pointer of an optional tensor of ``numel`` elements (targets), 0 for None"""
        if t is None:
            return 0
        self._chk(t, numel)
        return t.data_ptr()

    def _net(self, params, cols, n, lb, ub, normalize):
        """the leading arguments of a capi.PinnLib per-point call"""
        return (params.data_ptr(), self.layers, *[v.data_ptr() for v in cols], n, lb, ub, normalize)

    def _ws_tail(self):
        return self._ws_ptr, self.ws_bytes, self._stream()

    def _grad(self, grad_out, accumulate):
        if grad_out is None:
            return torch.empty(self.n_params, dtype=torch.float32, device=self.device), False
        return grad_out, accumulate

    def _outs(self, grad_out, accumulate, loss_out, n_loss: int = 8):
        grad_out, accumulate = self._grad(grad_out, accumulate)
        if loss_out is None:
            loss_out = torch.empty(n_loss, dtype=torch.float32, device=self.device)
        return grad_out, accumulate, loss_out

    def _new_or_checked(self, out, shape):
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._chk(out, math.prod(shape))
        return out

    def _set_rows(self, sets, per_point: int, min_loss: int = 0):
        """side sets (x, y, t, targets [per_point * n] or None, weights, loss_out) -> the rows capi.PinnLib takes; ``min_loss``: the
        loss_out tensors are checked to hold that many floats"""
        rows = []
        for x, y, t, tg, w, lo in sets:
            n = x.numel()
            for v in (x, y, t):
                self._chk(v, n)
            if min_loss:
                assert lo.is_cuda and lo.dtype == torch.float32 and lo.is_contiguous() and lo.numel() >= min_loss
            rows.append((x.data_ptr(), y.data_ptr(), t.data_ptr(), n, self._optional(tg, per_point * n), w, lo.data_ptr()))
        return rows

    def _adam(self, adam):
        """adam = (m, v, lr, step[, beta1, beta2, eps]) or None -> the (m, v, lr, beta1, beta2, eps, step) of capi.PinnLib or None"""
        if adam is None:
            return None
        m, v, lr, step = adam[:4]
        b1, b2, eps = (list(adam[4:]) + [0.9, 0.999, 1e-8][len(adam) - 4:])[:3]
        for a in (m, v):
            self._chk(a, self.n_params)
        return m.data_ptr(), v.data_ptr(), lr, b1, b2, eps, step

    def _scratch(self, name: str, nbytes_of):
        """(pointer, bytes) of the scratch buffer ``name`` of a call family whose size does not depend on n: allocated at its first use, one per engine"""
        if name not in self.__dict__:
            nbytes = nbytes_of()
            buf, ptr = aligned_buffer(nbytes, self.device)
            self.__dict__.update({name: buf, name + "_ptr": ptr, name + "_bytes": nbytes})
        return self.__dict__[name + "_ptr"], self.__dict__[name + "_bytes"]

    # ---- wave family (4 streams: value, d/dx, d/dy, d/dt) ---------------------------------------------------------------
    def wave_loss_grad(self, params, x, y, t, lb, ub, normalize, term_weights, E=2.5, mu=0.25, rho=1.0, plane_strain=True,
                       grad_out: Optional[torch.Tensor] = None, accumulate: bool = False, loss_out: Optional[torch.Tensor] = None, packed: bool = False):
        """Returns (sumsq[7] device tensor, grad_flat).  grad = d/dparams sum_i term_weights[i]*sumsq[i]."""
        n = self._check(params, (x, y, t))
        grad_out, accumulate, loss_out = self._outs(grad_out, accumulate, loss_out)
        self.lib.wave2d_loss_grad(*self._net(params, (x, y, t), n, lb, ub, normalize), E, mu, rho, plane_strain, term_weights,
                                  loss_out.data_ptr(), grad_out.data_ptr(), accumulate, self._mode(packed), *self._ws_tail())
        return loss_out[:7], grad_out

    def wave_loss_grad_profile(self, params, x, y, t, lb, ub, normalize, term_weights, E=2.5, mu=0.25, rho=1.0, plane_strain=True):
        """Synchronous variant returning HIP-event kernel times in ms: dict(repack, chain, wgrad, reduce)."""
        n = self._check(params, (x, y, t))
        grad, _, loss = self._outs(None, False, None)
        ms = self.lib.wave2d_loss_grad_profile(*self._net(params, (x, y, t), n, lb, ub, normalize), E, mu, rho, plane_strain, term_weights,
                                               loss.data_ptr(), grad.data_ptr(), False, self.precision, *self._ws_tail())
        return dict(zip(("repack", "chain", "wgrad", "reduce"), ms))

    def data_loss_grad(self, params, x, y, t, lb, ub, normalize, targets, out_weights,
                       grad_out: Optional[torch.Tensor] = None, accumulate: bool = False, loss_out: Optional[torch.Tensor] = None, packed: bool = False):
        """Value-only terms.  targets: [n_out, n] device tensor or None.  Returns (sumsq[n_out], grad)."""
        n, nout = self._check(params, (x, y, t)), self.layers[-1]
        tptr = self._optional(targets, nout * n)
        grad_out, accumulate, loss_out = self._outs(grad_out, accumulate, loss_out)
        self.lib.data_loss_grad(*self._net(params, (x, y, t), n, lb, ub, normalize), tptr, out_weights, loss_out.data_ptr(), grad_out.data_ptr(),
                                accumulate, self._mode(packed), *self._ws_tail())
        return loss_out[:nout], grad_out

    def data_loss_grad_multi(self, params, sets, lb, ub, normalize, grad_out, accumulate=False, packed=False):
        """Several value-only sets in one call.  sets: list of (x, y, t, targets_or_None, out_weights, loss_out[>=n_out]); the sums of
        set k land in its loss_out, the gradients are summed into grad_out."""
        self._chk(params, self.n_params)
        rows = self._set_rows(sets, self.layers[-1])
        self.lib.data_loss_grad_multi(params.data_ptr(), self.layers, rows, lb, ub, normalize, grad_out.data_ptr(), accumulate, self._mode(packed),
                                      *self._ws_tail())
        return grad_out

    def wave_traction_loss_grad(self, params, x, y, t, lb, ub, normalize, aux, weights, grad_out=None, accumulate=False, loss_out=None, packed=False):
        """Traction boundary term of the wave family (pinn_wave2d_traction_loss_grad, INF:267-276).  aux: [4, n] = nx, ny, tx, ty per point,
        the normals used as given; r_x = s11 nx + s12 ny - tx, r_y = s12 nx + s22 ny - ty.  Returns ((sum r_x^2, sum r_y^2), grad) with
        grad (+)= d/dparams (weights[0] sum r_x^2 + weights[1] sum r_y^2)."""
        n = self._check(params, (x, y, t))
        self._chk(aux, 4 * n)
        grad_out, accumulate, loss_out = self._outs(grad_out, accumulate, loss_out)
        self.lib.wave2d_traction_loss_grad(*self._net(params, (x, y, t), n, lb, ub, normalize), aux.data_ptr(), weights, loss_out.data_ptr(),
                                           grad_out.data_ptr(), accumulate, self._mode(packed), *self._ws_tail())
        return loss_out[:2], grad_out

    def wave_step(self, params, x, y, t, lb, ub, normalize, term_weights, sets, grad_out, loss_out, E=2.5, mu=0.25, rho=1.0, plane_strain=True,
                  accumulate: bool = False, adam=None, traction=None):
        """One training step's evaluation in one library call (pinn_wave2d_step): the collocation batch (x, y, t) with its seven term weights, the
        value-only ``sets`` (as data_loss_grad_multi: (x, y, t, targets_or_None, out_weights, loss_out)), the gradient of everything into
        ``grad_out`` and -- with ``adam = (m, v, lr, step[, beta1, beta2, eps])`` -- the TF1 Adam update of ``params`` behind it.  For the nets of
        the register-state fused kernel that is repack | one persistent launch | one reduction (+ Adam); for every other net the library makes
        the separate calls inside: the same bits either way.
        ``traction = (x, y, t, aux[4, n], weights[2], loss_out[>= 2])``: a traction boundary set as well (pinn_wave2d_step_traction): it joins
        the value-only sets' table as set kind 2 -- at most three ``sets`` then --, same launch, same reduction (+ Adam); None: the call above."""
        n = self._check(params, (x, y, t))
        self._chk(grad_out, self.n_params)
        rows = self._set_rows(sets, self.layers[-1])
        if traction is not None:
            tx, ty, tt, taux, tw, tlo = traction
            tn = self._check(params, (tx, ty, tt))
            self._chk(taux, 4 * tn)
            assert tlo.is_cuda and tlo.dtype == torch.float32 and tlo.is_contiguous() and tlo.numel() >= 2
            self.lib.wave2d_step_traction(*self._net(params, (x, y, t), n, lb, ub, normalize), E, mu, rho, plane_strain, term_weights, loss_out.data_ptr(),
                                          rows, tx.data_ptr(), ty.data_ptr(), tt.data_ptr(), tn, taux.data_ptr(), tw, tlo.data_ptr(), grad_out.data_ptr(),
                                          accumulate, self._adam(adam), self._mode(False), *self._ws_tail())
            return grad_out
        self.lib.wave2d_step(*self._net(params, (x, y, t), n, lb, ub, normalize), E, mu, rho, plane_strain, term_weights, loss_out.data_ptr(), rows,
                             grad_out.data_ptr(), accumulate, self._adam(adam), self._mode(False), *self._ws_tail())
        return grad_out

    def fields(self, params, x, y, t, lb, ub, normalize):
        """Returns [4, n_out, n]: Y and its derivatives w.r.t. x, y, t."""
        n = self._check(params, (x, y, t))
        out = torch.empty((4, self.layers[-1], n), dtype=torch.float32, device=self.device)
        self.lib.wave2d_fields(*self._net(params, (x, y, t), n, lb, ub, normalize), out.data_ptr(), self.precision, *self._ws_tail())
        return out

    # ---- residual-adaptive refinement: per-point score and selection ------------------------------------------------
    def residual_score(self, params, x, y, t, lb, ub, normalize, term_weights, E=2.5, mu=0.25, rho=1.0, plane_strain=True,
                       out: Optional[torch.Tensor] = None, packed: bool = False):
        """Returns the device tensor [n] of  sum_i term_weights[i] * f_i(n)^2  (pinn_wave2d_residual_score): the wave residuals of
        net_f_sig per point, formed in the kernel -- nothing but the score leaves it."""
        n = self._check(params, (x, y, t))
        out = self._new_or_checked(out, (n,))
        self.lib.wave2d_residual_score(*self._net(params, (x, y, t), n, lb, ub, normalize), E, mu, rho, plane_strain, term_weights, out.data_ptr(),
                                       self._forward_mode(packed), *self._ws_tail())
        return out

    def plate_residual_score(self, params, x, y, t, lb, ub, normalize, frozen, term_weights, E=20.0, mu=0.25, rho=1.0,
                             out: Optional[torch.Tensor] = None, packed: bool = False):
        """The same for the plate family (pinn_plate2d_residual_score): ``frozen`` is the [2, 5, 5, n] tensor of plate_loss_grad at these points,
        the five residuals are those of the composite P + D*N.  Returns the device tensor [n]."""
        n = self._check(params, (x, y, t))
        self._chk(frozen, 50 * n)
        out = self._new_or_checked(out, (n,))
        self.lib.plate2d_residual_score(*self._net(params, (x, y, t), n, lb, ub, normalize), frozen.data_ptr(), E, mu, rho, term_weights, out.data_ptr(),
                                        self._forward_mode(packed), *self._ws_tail())
        return out

    def nc3d_residual_score(self, params, x, y, z, t, lb, ub, normalize, term_weights, E=2.5, mu=0.25, rho=1.0,
                            out: Optional[torch.Tensor] = None, packed: bool = False):
        """The same for the 4-input family (pinn_nc3d_residual_score): the twelve residuals of nc3d_loss_grad.  Returns the device tensor [n]."""
        n = self._check(params, (x, y, z, t))
        out = self._new_or_checked(out, (n,))
        self.lib.nc3d_residual_score(*self._net(params, (x, y, z, t), n, lb, ub, normalize), E, mu, rho, term_weights, out.data_ptr(),
                                     self._forward_mode(packed), *self._ws_tail())
        return out

    # ---- material identification: fp64 residual and moment sums over a point set ------------------------------------
    def material_sums(self, params, x, y, t, lb, ub, normalize, E=2.5, mu=0.25, rho=1.0, plane_strain=True,
                      out: Optional[torch.Tensor] = None, packed: bool = False):
        """Returns the device float64 tensor [14] of pinn_wave2d_material_sums: the sums of squares of the seven wave residuals, then the
        seven moment sums their derivatives by (c1, c2, G, rho) are made of (material.gradient turns them into dL/dE, dL/dmu, dL/drho).
        Forward only, fixed summation order, no synchronisation."""
        n = self._check(params, (x, y, t))
        ws, ws_bytes = self._scratch("_material_ws", self.lib.material_sums_workspace_bytes)
        if out is None:
            out = torch.empty(MATERIAL_SUMS, dtype=torch.float64, device=self.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == MATERIAL_SUMS
        self.lib.wave2d_material_sums(*self._net(params, (x, y, t), n, lb, ub, normalize), E, mu, rho, plane_strain, out.data_ptr(),
                                      self._forward_mode(packed), self._ws_ptr, self.ws_bytes, ws, ws_bytes, self._stream())
        return out

    def _sums_out(self, out, n_sums):
        """the float64 device tensor [n_sums] a material call writes: ``out`` checked, or a new one"""
        if out is None:
            out = torch.empty(n_sums, dtype=torch.float64, device=self.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == n_sums
        return out

    def plate_material_sums(self, params, x, y, t, lb, ub, normalize, frozen, E, mu, rho, out: Optional[torch.Tensor] = None, packed: bool = False):
        """The same for the plate family (pinn_plate2d_material_sums): ``frozen`` is the [2, 5, 5, n] tensor of plate_loss_grad at these points.
        Returns the device float64 tensor [12]: the sums of squares of the five plane-stress residuals, then the seven moment sums
        (material.gradient with material.PLATE)."""
        n = self._check(params, (x, y, t))
        self._chk(frozen, 50 * n)
        ws, ws_bytes = self._scratch("_material_ws", self.lib.material_sums_workspace_bytes)
        out = self._sums_out(out, MATERIAL_SUMS_PLATE)
        self.lib.plate2d_material_sums(*self._net(params, (x, y, t), n, lb, ub, normalize), frozen.data_ptr(), E, mu, rho, out.data_ptr(),
                                       self._forward_mode(packed), self._ws_ptr, self.ws_bytes, ws, ws_bytes, self._stream())
        return out

    def nc3d_material_sums(self, params, x, y, z, t, lb, ub, normalize, E, mu, rho, out: Optional[torch.Tensor] = None, packed: bool = False):
        """The same for the 4-input family (pinn_nc3d_material_sums).  Returns the device float64 tensor [24]: the sums of squares of the twelve
        residuals of nc3d_loss_grad, then the twelve moment sums (material.gradient with material.NC3D)."""
        n = self._check(params, (x, y, z, t))
        ws, ws_bytes = self._scratch("_material_ws", self.lib.material_sums_workspace_bytes)
        out = self._sums_out(out, MATERIAL_SUMS_NC3D)
        self.lib.nc3d_material_sums(*self._net(params, (x, y, z, t), n, lb, ub, normalize), E, mu, rho, out.data_ptr(),
                                    self._forward_mode(packed), self._ws_ptr, self.ws_bytes, ws, ws_bytes, self._stream())
        return out

    # ---- predict heads: value + space tangents only, and the per-field error sums behind them ------------------------
    def wave_predict(self, params, x, y, t, lb, ub, normalize, out: Optional[torch.Tensor] = None, packed: bool = False):
        """Returns the device tensor [8, n] = u, v, s11, s22, s12, e11, e22, e12 (pinn_wave2d_predict): the forward of ``fields`` with the
        streams value, d/dx, d/dy only -- no time tangent."""
        n = self._check(params, (x, y, t))
        out = self._new_or_checked(out, (8, n))
        self.lib.wave2d_predict(*self._net(params, (x, y, t), n, lb, ub, normalize), out.data_ptr(), self._forward_mode(packed), *self._ws_tail())
        return out

    def plate_predict(self, params, x, y, t, lb, ub, normalize, frozen, out: Optional[torch.Tensor] = None, packed: bool = False):
        """The same for the plate family (pinn_plate2d_predict): ``frozen`` is the [2, 5, 5, n] tensor of plate_loss_grad at these points (its
        stream rows 0..2 are read), the eight rows are those of the composite P + D*N."""
        n = self._check(params, (x, y, t))
        self._chk(frozen, 50 * n)
        out = self._new_or_checked(out, (8, n))
        self.lib.plate2d_predict(*self._net(params, (x, y, t), n, lb, ub, normalize), frozen.data_ptr(), out.data_ptr(), self._forward_mode(packed),
                                 *self._ws_tail())
        return out

    def field_error_sums(self, pred, rows, ref, out: Optional[torch.Tensor] = None):
        """Per-field error sums of the device tensor ``pred`` [pred_rows, n] against ``ref`` [len(rows), n] (pinn_field_error_sums): the device
        float64 tensor [2, len(rows)] = sum (pred[rows[j]] - ref[j])^2, then sum ref[j]^2, formed in fp64 in a fixed order.  No synchronisation."""
        self._chk(pred)
        rows = [int(r) for r in rows]
        n = pred.shape[-1]
        self._chk(ref, len(rows) * n)
        # (the size depends on the row count only: one buffer for the 16 rows a call may have)
        ws, ws_bytes = self._scratch("_err_ws", lambda: self.lib.field_error_workspace_bytes(0, 16))
        if out is None:
            out = torch.empty((2, len(rows)), dtype=torch.float64, device=self.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == 2 * len(rows)
        self.lib.field_error_sums(pred.data_ptr(), pred.numel() // n if n else max(rows) + 1, rows, ref.data_ptr(), n, out.data_ptr(),
                                  ws, ws_bytes, self._stream())
        return out

    def select_k(self, score, k: int, largest: bool = True):
        """The k largest (or smallest) entries of the device tensor ``score`` as a device int32 [k] of ASCENDING indices (pinn_select_k):
        ties go to the lowest index, a NaN ranks above +inf, the result is exactly reproducible.  No synchronisation."""
        self._chk(score)
        ws, ws_bytes = self._scratch("_select_ws", lambda: self.lib.select_workspace_bytes(0))
        out = torch.empty(int(k), dtype=torch.int32, device=self.device)
        self.lib.select_k(score.data_ptr(), score.numel(), k, largest, out.data_ptr(), ws, ws_bytes, self._stream())
        return out

    def sample_box(self, n: int, lo, hi, seed: int, stream: int = 0, first: int = 0, t_cdf: Optional[torch.Tensor] = None):
        """n points uniform in the box [lo, hi] (3 bounds: columns x, y, t; 4: x, y, z, t) as a tuple of device columns (pinn_sample_box):
        Philox4x32-10 keyed by ``seed``, point i a function of (seed, stream, first + i) alone.  No synchronisation.
        ``t_cdf``: a device float32 [bins + 1] table (causal_cdf) -- the time column then follows its piecewise-constant density over the bins
        of [lo_t, hi_t] (pinn_sample_box_cdf), the space columns keep their bits.  None: exactly the call above."""
        dim = len(lo)
        cols = tuple(torch.empty(int(n), dtype=torch.float32, device=self.device) for _ in range(dim))
        if t_cdf is None:
            self.lib.sample_box(seed, stream, first, n, lo, hi, [c.data_ptr() for c in cols], self._stream())
        else:
            self._chk(t_cdf)
            self.lib.sample_box(seed, stream, first, n, lo, hi, [c.data_ptr() for c in cols], self._stream(), t_cdf.data_ptr(), t_cdf.numel() - 1)
        return cols

    # ---- causal sampling: per-time-bin score sums, the causal weights and their CDF ---------------------------------
    def binned_sums(self, value, coord, lo: float, hi: float, n_bins: int, out: Optional[torch.Tensor] = None):
        """Per-bin sums of the device tensor ``value`` over ``n_bins`` equal bins of [lo, hi] of the device tensor ``coord``
        (pinn_binned_sums): the device float64 tensor [2, n_bins] = the sums, then the counts; a value that is negative or not finite (the
        -inf keys of refine_keys' mask mode) is skipped.  fp64, fixed order, no synchronisation."""
        self._chk(value)
        self._chk(coord, value.numel())
        # (the size depends on the bin count only: one buffer for the 64 bins a call may have)
        ws, ws_bytes = self._scratch("_bins_ws", lambda: self.lib.binned_sums_workspace_bytes(0, MAX_TIME_BINS))
        if out is None:
            out = torch.empty((2, int(n_bins)), dtype=torch.float64, device=self.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == 2 * int(n_bins)
        self.lib.binned_sums(value.data_ptr(), coord.data_ptr(), value.numel(), lo, hi, n_bins, out.data_ptr(), ws, ws_bytes, self._stream())
        return out

    def causal_cdf(self, binned, eps: float, floor: float = 0.0):
        """(w, cdf) of pinn_causal_cdf from the [2, bins] output of binned_sums: the device float64 tensor [bins] of the causal weights
        w_b = exp(-eps * sum of the earlier bins' mean values) and the device float32 tensor [bins + 1] of the CDF of max(w, floor) that
        sample_box(t_cdf=...) reads.  One small launch, no synchronisation."""
        assert binned.is_cuda and binned.dtype == torch.float64 and binned.is_contiguous() and binned.dim() == 2 and binned.shape[0] == 2
        n_bins = int(binned.shape[1])
        w = torch.empty(n_bins, dtype=torch.float64, device=self.device)
        cdf = torch.empty(n_bins + 1, dtype=torch.float32, device=self.device)
        self.lib.causal_cdf(binned.data_ptr(), n_bins, eps, floor, w.data_ptr(), cdf.data_ptr(), self._stream())
        return w, cdf

    def refine_keys(self, score, cols, balls=(), mode: str = "mask", power: float = 1.0, c: float = 1.0, seed: int = 0, stream: int = 0, first: int = 0):
        """Selection keys of the device scores ``score`` at the device columns ``cols`` (x, y, t) or (x, y, z, t) (pinn_refine_keys): -inf
        inside the ``balls`` -- (xc, yc, r) discs, (xc, yc, zc, r) balls --; otherwise the score (mode 'mask') or log p + Gumbel noise with
        p = score^power / mean + c (mode 'sample'), so that select_k(keys, k) draws k points without replacement, P ~ p.  No synchronisation."""
        self._chk(score)
        n = score.numel()
        for v in cols:
            self._chk(v, n)
        ws, ws_bytes = self._scratch("_keys_ws", lambda: self.lib.refine_keys_workspace_bytes(0))
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        x, y = (cols[0].data_ptr(), cols[1].data_ptr()) if len(cols) >= 2 else (None, None)      # (no columns: fine without balls)
        z = cols[2].data_ptr() if len(cols) == 4 else None
        self.lib.refine_keys(score.data_ptr(), n, x, y, z, list(balls), mode, power, c, seed, stream, first, out.data_ptr(), ws, ws_bytes, self._stream())
        return out

    # ---- plate family (5 streams: value, d/dx, d/dy, d/dt, d2/dt2) --------------------------------------------------
    def net_streams(self, params, x, y, t, lb, ub, normalize):
        """Returns [5, n_out, n]: the net's outputs, their first derivatives and the second time derivative."""
        n = self._check(params, (x, y, t))
        out = torch.empty((5, self.layers[-1], n), dtype=torch.float32, device=self.device)
        self.lib.net_streams(*self._net(params, (x, y, t), n, lb, ub, normalize), out.data_ptr(), self.precision, *self._ws_tail())
        return out

    def plate_loss_grad(self, params, x, y, t, lb, ub, normalize, frozen, term_weights, E=20.0, mu=0.25, rho=1.0,
                        grad_out=None, accumulate=False, loss_out=None):
        """frozen: [2, 5, 5, n] streams of the distance and particular nets.  Returns (sumsq[5], grad wrt this net)."""
        n = self._check(params, (x, y, t))
        self._chk(frozen, 50 * n)
        grad_out, accumulate, loss_out = self._outs(grad_out, accumulate, loss_out)
        self.lib.plate2d_loss_grad(*self._net(params, (x, y, t), n, lb, ub, normalize), frozen.data_ptr(), E, mu, rho, term_weights,
                                   loss_out.data_ptr(), grad_out.data_ptr(), accumulate, self._mode(False), *self._ws_tail())
        return loss_out[:5], grad_out

    def plate_step(self, params, x, y, t, lb, ub, normalize, frozen, term_weights, hole, grad_out, loss_out, hole_loss_out, E=20.0, mu=0.25, rho=1.0,
                   accumulate: bool = False, adam=None):
        """The plate's step in one library call (pinn_plate2d_step): collocation set (frozen: [2, 5, 5, n]) + hole-traction set
        ``hole = (x, y, t, aux[12, n], weights[2])`` -> gradient in ``grad_out``, sums in ``loss_out`` / ``hole_loss_out``, and with
        ``adam = (m, v, lr, step[, beta1, beta2, eps])`` the TF1 Adam update of ``params`` in the same final launch."""
        n = self._check(params, (x, y, t))
        self._chk(frozen, 50 * n)
        self._chk(grad_out, self.n_params)
        hx, hy, ht, haux, hw = hole
        hn = self._check(params, (hx, hy, ht))
        self._chk(haux, 12 * hn)
        self.lib.plate2d_step(*self._net(params, (x, y, t), n, lb, ub, normalize), frozen.data_ptr(), E, mu, rho, term_weights, loss_out.data_ptr(),
                              hx.data_ptr(), hy.data_ptr(), ht.data_ptr(), hn, haux.data_ptr(), hw, hole_loss_out.data_ptr(), grad_out.data_ptr(),
                              accumulate, self._adam(adam), self._mode(False), *self._ws_tail())
        return grad_out

    def traction_loss_grad(self, params, x, y, t, lb, ub, normalize, aux, weights, grad_out=None, accumulate=False, loss_out=None, packed=False):
        """aux: [12, n] = D values, P values, nx, ny.  Returns ((sum tx^2, sum ty^2), grad)."""
        n = self._check(params, (x, y, t))
        self._chk(aux, 12 * n)
        grad_out, accumulate, loss_out = self._outs(grad_out, accumulate, loss_out)
        self.lib.plate2d_traction_loss_grad(*self._net(params, (x, y, t), n, lb, ub, normalize), aux.data_ptr(), weights, loss_out.data_ptr(),
                                            grad_out.data_ptr(), accumulate, self._mode(packed), *self._ws_tail())
        return loss_out[:2], grad_out

    def stream_loss_grad(self, params, x, y, t, lb, ub, normalize, targets, weights, grad_out=None, accumulate=False, loss_out=None):
        """targets: [5, n_out, n] or None; weights: 5 x n_out nested list.  Returns (per-output normalised sums, grad)."""
        n, nout = self._check(params, (x, y, t)), self.layers[-1]
        tptr = self._optional(targets, 5 * nout * n)
        grad_out, accumulate, loss_out = self._outs(grad_out, accumulate, loss_out)
        self.lib.stream_loss_grad(*self._net(params, (x, y, t), n, lb, ub, normalize), tptr, weights, loss_out.data_ptr(), grad_out.data_ptr(),
                                  accumulate, self.precision, *self._ws_tail())
        return loss_out[:nout], grad_out

    def stream_loss_grad_multi(self, params, sets, lb, ub, normalize, grad_out=None, accumulate=False):
        """All stream-target sets of a pre-training loss in one library call (pinn_stream_loss_grad_multi).  sets: list of
        (x, y, t, targets [5, n_out, n] or None, weights 5 x n_out, loss_out[>= n_out]).  The sums of set k land in its loss_out, normalised
        by the largest |weight| of ALL sets; the gradient of the unnormalised loss goes to grad_out.  Returns grad_out."""
        self._chk(params, self.n_params)
        nout = self.layers[-1]
        rows = self._set_rows(sets, 5 * nout, min_loss=nout)
        grad_out, accumulate = self._grad(grad_out, accumulate)
        self._chk(grad_out, self.n_params)
        self.lib.stream_loss_grad_multi(params.data_ptr(), self.layers, rows, lb, ub, normalize, grad_out.data_ptr(), accumulate, self._mode(False),
                                        *self._ws_tail())
        return grad_out

    # ---- 3-D Navier-Cauchy extension (layers [4, H, ..., H, 12]; inputs x, y, z, t) -------------------------------------
    def nc3d_loss_grad(self, params, x, y, z, t, lb, ub, normalize, term_weights, E=2.5, mu=0.25, rho=1.0,
                       grad_out=None, accumulate=False, loss_out=None, packed=False):
        """Returns (sumsq[12], grad): residuals (f_u,f_v,f_w,f_ut,f_vt,f_wt,f_s11,f_s22,f_s33,f_s12,f_s13,f_s23), see include/pinn_hip.h."""
        n = self._check(params, (x, y, z, t))
        grad_out, accumulate, loss_out = self._outs(grad_out, accumulate, loss_out, 16)
        self.lib.nc3d_loss_grad(*self._net(params, (x, y, z, t), n, lb, ub, normalize), E, mu, rho, term_weights, loss_out.data_ptr(),
                                grad_out.data_ptr(), accumulate, self._mode(packed), *self._ws_tail())
        return loss_out[:12], grad_out

    def nc3d_data_loss_grad(self, params, x, y, z, t, lb, ub, normalize, targets, out_weights,
                            grad_out=None, accumulate=False, loss_out=None, packed=False):
        """Value-only terms of the 4-input net.  targets: [n_out, n] device tensor or None.  Returns (sumsq[n_out], grad)."""
        n, nout = self._check(params, (x, y, z, t)), self.layers[-1]
        tptr = self._optional(targets, nout * n)
        grad_out, accumulate, loss_out = self._outs(grad_out, accumulate, loss_out, 16)
        self.lib.nc3d_data_loss_grad(*self._net(params, (x, y, z, t), n, lb, ub, normalize), tptr, out_weights, loss_out.data_ptr(),
                                     grad_out.data_ptr(), accumulate, self._mode(packed), *self._ws_tail())
        return loss_out[:nout], grad_out

    def nc3d_fields(self, params, x, y, z, t, lb, ub, normalize):
        """Returns [5, n_out, n]: the outputs and their derivatives w.r.t. x, y, z, t."""
        n = self._check(params, (x, y, z, t))
        out = torch.empty((5, self.layers[-1], n), dtype=torch.float32, device=self.device)
        self.lib.nc3d_fields(*self._net(params, (x, y, z, t), n, lb, ub, normalize), out.data_ptr(), self.precision, *self._ws_tail())
        return out

    def adam_step(self, params, m, v, grad, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
        for a in (params, m, v, grad):
            self._chk(a, self.n_params)
        self.lib.adam_step(params.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), self.n_params, lr, step, beta1, beta2, eps,
                           self._stream())
