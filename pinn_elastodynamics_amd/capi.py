"""ctypes binding of the C-ABI declared in include/pinn_hip.h (libpinn_hip.so).

Pointer arguments are passed as plain integers (``tensor.data_ptr()`` for device memory), so the
binding itself has no torch dependency; PyTorch is only the owner of device buffers and streams.
"""
from __future__ import annotations

import ctypes as C
import os

PREC = {"bf16": 0, "f16x3": 1, "f16": 2, "bf16x3": 3, "fp32": 4}
HEADS = {"wave": 0, "data": 1, "plate": 2, "nc3d": 3, "nc3d_data": 4, "streams": 5, "stream_sets": 6}      # PINN_HEAD_*
PATHS = {1: "fused-registers", 2: "fused-lds", 3: "two-kernel", 4: "fp32"}                  # PINN_PATH_*
FLAG_WEIGHTS_PACKED = 0x100
FLAG_TWO_KERNEL = 0x400            # PINN_FLAG_TWO_KERNEL: keep the call off the fused kernel (weights beyond its |w| <= 2047 format)
FLAG_STATE_FP16 = 0x200            # PINN_FLAG_STATE_FP16: fused 8-layer collocation kernel parks fp16 states only (faster, not parity-grade)
def adjoint_shift(k: int) -> int:
    """PINN_ADJOINT_SHIFT(k) of include/pinn_hip.h"""
    return (int(k) & 0x1f) << 16


def mode_bits(prec) -> int:
    """precision name (optionally "+packed") or ready-made integer -> the precision_mode argument"""
    return PREC[prec] if isinstance(prec, str) else int(prec)


PREC["f16x3+fp16state"] = PREC["f16x3"] | FLAG_STATE_FP16       # the opt-in fp16-state variant of the fused 8-layer collocation kernel
for _k in list(PREC):                      # "<mode>+packed": the workspace still holds this call's packed weights (PINN_FLAG_WEIGHTS_PACKED)
    PREC[_k + "+packed"] = PREC[_k] | FLAG_WEIGHTS_PACKED

_HERE = os.path.dirname(os.path.abspath(__file__))
# (PINN_HIP_LIB: another build of the same library -- the A / B experiments of tools/ run the product's own bench against build/exp/NAME/libpinn_hip.so)
DEFAULT_LIB = os.environ.get("PINN_HIP_LIB") or os.path.join(_HERE, "lib", "libpinn_hip.so")


class PointSet(C.Structure):
    """pinn_point_set of include/pinn_hip.h"""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("t", C.c_void_p), ("n", C.c_int64), ("targets", C.c_void_p),
                ("out_weights", C.c_float * 8), ("loss_terms_out", C.c_void_p)]


MAX_STREAM_SETS = 8                # PINN_MAX_STREAM_SETS


class StreamSet(C.Structure):
    """pinn_stream_set of include/pinn_hip.h"""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("t", C.c_void_p), ("n", C.c_int64), ("targets", C.c_void_p),
                ("weights", (C.c_float * 8) * 5), ("loss_terms_out", C.c_void_p)]


MAX_BALLS = 4                      # PINN_MAX_BALLS
MAX_TIME_BINS = 64                 # PINN_MAX_TIME_BINS
MATERIAL_SUMS = 14                 # PINN_MATERIAL_SUMS
MATERIAL_SUMS_PLATE = 12           # PINN_MATERIAL_SUMS_PLATE
MATERIAL_SUMS_NC3D = 24            # PINN_MATERIAL_SUMS_NC3D
KEYS_MODE = {"mask": 0, "sample": 1}             # PINN_KEYS_*


class Ball(C.Structure):
    """pinn_ball of include/pinn_hip.h"""
    _fields_ = [("centre", C.c_double * 3), ("radius", C.c_double), ("ndim", C.c_int), ("keep_boundary", C.c_int)]


def ball_array(balls):
    """(xc, yc, r) discs and (xc, yc, zc, r) balls as a pinn_ball array, the boundary excluded with the inside (keep_boundary = 0); a Ball
    structure is taken as it is"""
    out = (Ball * max(len(balls), 1))()
    for k, b in enumerate(balls):
        if isinstance(b, Ball):
            out[k] = b
            continue
        v = [float(a) for a in b]
        if len(v) not in (3, 4):
            raise ValueError("an excluded region is (xc, yc, r) or (xc, yc, zc, r)")
        centre = v[:-1] + [0.0] * (4 - len(v))
        out[k] = Ball((C.c_double * 3)(*centre), v[-1], len(v) - 1, 0)
    return out


class AdamState(C.Structure):
    """pinn_adam_state of include/pinn_hip.h"""
    _fields_ = [("m", C.c_void_p), ("v", C.c_void_p), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("step", C.c_int64)]


class RangeState(C.Structure):
    """pinn_range_state of include/pinn_hip.h: what the finite-gradient ladder of pinn_wave2d_loss_grad_checked carries between calls"""
    _fields_ = [("adjoint_shift", C.c_int32), ("two_kernel", C.c_int32), ("attempts", C.c_int32), ("reserved", C.c_int32)]


LBFGS_STATUS = {0: "running", 1: "gtol", 2: "ftol", 3: "maxiter", 4: "maxfun", 5: "linesearch", 6: "nonfinite_start", 7: "nonfinite_grad"}      # PINN_LBFGS_*
LBFGS_MAX_HISTORY, LBFGS_MAX_SUMS, LBFGS_LOSS_RING = 64, 128, 1024


class LbfgsOptions(C.Structure):
    """pinn_lbfgs_options of include/pinn_hip.h"""
    _fields_ = [("history", C.c_int), ("maxiter", C.c_int), ("maxfun", C.c_int), ("maxls", C.c_int), ("ftol", C.c_double), ("gtol", C.c_double)]


class LbfgsRecord(C.Structure):
    """pinn_lbfgs_record of include/pinn_hip.h"""
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("evaluations", C.c_int), ("pairs", C.c_int), ("skipped", C.c_int), ("trials", C.c_int),
                ("loss_pos", C.c_int64), ("f", C.c_double), ("max_abs_grad", C.c_double), ("step", C.c_double)]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["status_name"] = LBFGS_STATUS.get(self.status, "?")
        return d


class PinnLibError(RuntimeError):
    pass


# ---- prototypes: symbol -> (restype, argtypes) of EVERY function include/pinn_hip.h declares, a row per declaration in the header's order and
# spelling.  Module-level data: tests/test_capi_header.py holds it to the header without loading a library; PinnLib.__init__ applies it.
_vp, _i32, _i64, _f64, _sz, _u32, _u64 = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_size_t, C.c_uint32, C.c_uint64
_pi32, _pf64, _pf32, _psz = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_size_t)
_NET = [_vp, _pi32, _i32]                          # params_flat, layers, n_layers
_BOX = [_pf64, _pf64, _i32]                        # lb, ub, normalize
_PTS3 = [_vp, _vp, _vp, _i64] + _BOX               # x, y, t, n + box
_PTS4 = [_vp, _vp, _vp, _vp, _i64] + _BOX          # x, y, z, t, n + box
_MAT = [_f64, _f64, _f64]                          # E, mu, rho
_WAVE = _MAT + [_i32, _pf32]                       # + plane_strain, term_weights[7]
_OUT = [_vp, _vp, _i32]                            # loss_terms_out, grad_flat_out, accumulate
_TAIL = [_i32, _vp, _sz, _vp]                      # precision_mode, workspace, ws_bytes, stream
_SUMS = [_vp] + _TAIL[:3] + [_vp, _sz, _vp]        # sums_out, precision_mode, workspace, ws_bytes, sums_workspace, sums_ws_bytes, stream
_ADAM = C.POINTER(AdamState)
PROTOTYPES = {
    "pinn_supported_width": (_i32, [_i32]),
    "pinn_fused_weight_limit": (C.c_float, []),
    "pinn_path_for": (_i32, [_pi32, _i32, _i32, _i32, _sz]),
    "pinn_debug_path_counts": (None, [_vp, _i32]),
    "pinn_workspace_bytes": (_sz, [_pi32, _i32, _i64, _i32]),
    "pinn_min_workspace_bytes": (_sz, [_pi32, _i32, _i32]),
    "pinn_wave2d_loss_grad": (_i32, _NET + _PTS3 + _WAVE + _OUT + _TAIL),
    "pinn_wave2d_loss_grad_profile": (_i32, _NET + _PTS3 + _WAVE + _OUT + _TAIL + [_pf32]),
    "pinn_data_loss_grad": (_i32, _NET + _PTS3 + [_vp, _pf32] + _OUT + _TAIL),
    "pinn_wave2d_fields": (_i32, _NET + _PTS3 + [_vp] + _TAIL),
    "pinn_wave2d_residual_score": (_i32, _NET + _PTS3 + _WAVE + [_vp] + _TAIL),
    "pinn_wave2d_predict": (_i32, _NET + _PTS3 + [_vp] + _TAIL),
    "pinn_material_sums_workspace_bytes": (_sz, []),
    "pinn_wave2d_material_sums": (_i32, _NET + _PTS3 + _MAT + [_i32] + _SUMS),
    "pinn_field_error_workspace_bytes": (_sz, [_i64, _i32]),
    "pinn_field_error_sums": (_i32, [_vp, _i64, _pi32, _i32, _vp, _i64, _vp, _vp, _sz, _vp]),
    "pinn_select_workspace_bytes": (_sz, [_i64]),
    "pinn_select_k": (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, _sz, _vp]),
    "pinn_sample_box": (_i32, [_u64, _u32, _u64, _i64, _i32, _pf64, _pf64, _vp, _vp, _vp, _vp, _vp]),
    "pinn_refine_keys_workspace_bytes": (_sz, [_i64]),
    "pinn_refine_keys": (_i32, [_vp, _i64, _vp, _vp, _vp, C.POINTER(Ball), _i32, _i32, _f64, _f64, _u64, _u32, _u64, _vp, _vp, _sz, _vp]),
    "pinn_binned_sums_workspace_bytes": (_sz, [_i64, _i32]),
    "pinn_binned_sums": (_i32, [_vp, _vp, _i64, _f64, _f64, _i32, _vp, _vp, _sz, _vp]),
    "pinn_causal_cdf": (_i32, [_vp, _i32, _f64, _f64, _vp, _vp, _vp]),
    "pinn_sample_box_cdf": (_i32, [_u64, _u32, _u64, _i64, _i32, _pf64, _pf64, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "pinn_net_streams": (_i32, _NET + _PTS3 + [_vp] + _TAIL),
    "pinn_plate2d_loss_grad": (_i32, _NET + _PTS3 + [_vp] + _MAT + [_pf32] + _OUT + _TAIL),
    "pinn_plate2d_residual_score": (_i32, _NET + _PTS3 + [_vp] + _MAT + [_pf32, _vp] + _TAIL),
    "pinn_plate2d_material_sums": (_i32, _NET + _PTS3 + [_vp] + _MAT + _SUMS),
    "pinn_plate2d_predict": (_i32, _NET + _PTS3 + [_vp, _vp] + _TAIL),
    "pinn_plate2d_traction_loss_grad": (_i32, _NET + _PTS3 + [_vp, _pf32] + _OUT + _TAIL),
    "pinn_stream_loss_grad": (_i32, _NET + _PTS3 + [_vp, _pf32] + _OUT + _TAIL),
    "pinn_stream_loss_grad_multi": (_i32, _NET + [C.POINTER(StreamSet), _i32] + _BOX + [_vp, _i32] + _TAIL),
    "pinn_probe_ranges": (_i32, [_vp, _vp, _i64, _vp, _sz, _vp, _pi32, _pf32]),
    # (no `accumulate` argument, a pinn_range_state at the end)
    "pinn_wave2d_loss_grad_checked": (_i32, _NET + _PTS3 + _WAVE + [_vp, _vp] + _TAIL + [C.POINTER(RangeState)]),
    "pinn_data_loss_grad_multi": (_i32, _NET + [C.POINTER(PointSet), _i32] + _BOX + [_vp, _i32] + _TAIL),
    "pinn_wave2d_step": (_i32, _NET + _PTS3 + _WAVE + [_vp, C.POINTER(PointSet), _i32, _vp, _i32, _ADAM] + _TAIL),
    "pinn_plate2d_step": (_i32, _NET + _PTS3 + [_vp] + _MAT + [_pf32, _vp, _vp, _vp, _vp, _i64, _vp, _pf32, _vp, _vp, _i32, _ADAM] + _TAIL),
    "pinn_wave2d_traction_loss_grad": (_i32, _NET + _PTS3 + [_vp, _pf32] + _OUT + _TAIL),
    "pinn_wave2d_step_traction": (_i32, _NET + _PTS3 + _WAVE + [_vp, C.POINTER(PointSet), _i32, _vp, _vp, _vp, _i64, _vp, _pf32, _vp, _vp, _i32, _ADAM] + _TAIL),
    "pinn_nc3d_loss_grad": (_i32, _NET + _PTS4 + _MAT + [_pf32] + _OUT + _TAIL),
    "pinn_nc3d_data_loss_grad": (_i32, _NET + _PTS4 + [_vp, _pf32] + _OUT + _TAIL),
    "pinn_nc3d_fields": (_i32, _NET + _PTS4 + [_vp] + _TAIL),
    "pinn_nc3d_residual_score": (_i32, _NET + _PTS4 + _MAT + [_pf32, _vp] + _TAIL),
    "pinn_nc3d_material_sums": (_i32, _NET + _PTS4 + _MAT + _SUMS),
    "pinn_adam_step": (_i32, [_vp, _vp, _vp, _vp, _i64, _f64, _f64, _f64, _f64, _i64, _vp]),
    "pinn_lbfgs_state_bytes": (_sz, [_i64, _i32]),
    "pinn_lbfgs_init": (_i32, [_vp, _sz, _i64, C.POINTER(LbfgsOptions), _pf32, _i32, _f64, _vp]),
    "pinn_lbfgs_advance": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "pinn_lbfgs_status": (_i32, [_vp, C.POINTER(LbfgsRecord), _vp]),
    "pinn_lbfgs_read_losses": (_i32, [_vp, _i64, _i64, _pf64, _vp]),
    "pinn_lbfgs_debug_read": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _i32, _pi32, _vp]),
    "pinn_p2p_create": (_i32, [_i32, _i32, _i64, C.POINTER(_vp), _vp]),
    "pinn_p2p_connect": (_i32, [_vp, _vp]),
    "pinn_p2p_set_timeout_ms": (_i32, [_vp, _f64]),
    "pinn_p2p_allreduce": (_i32, [_vp, _vp, _i64, _vp, _ADAM, _i64, _vp]),
    "pinn_p2p_status": (_i32, [_vp, _pi32]),
    "pinn_p2p_peek_status": (_i32, [_vp]),
    "pinn_p2p_destroy": (_i32, [_vp]),
    "pinn_p2p_debug_force_coarse": (_i32, [_i32]),
    "pinn_debug_set_fused": (_i32, [_i32]),
    "pinn_debug_set_step_launch": (_i32, [_i32]),
    "pinn_debug_set_xcd_bonus": (_i32, [_i32]),
    "pinn_debug_set_fused_grid_cap": (_i32, [_i32]),
    "pinn_debug_cache_policy": (_i32, [_pi32, _i32, _i32, _psz, _psz]),
    "pinn_debug_set_stamp_buffer": (None, [_vp]),
    "pinn_debug_wall_clock_khz": (_i32, []),
    "pinn_debug_set_profile_buffer": (None, [_vp]),
    "pinn_debug_profile_ring_arm": (_i32, [_i32]),
    "pinn_debug_profile_ring_stride": (None, [_i32]),
    "pinn_debug_profile_ring_read": (_i32, [_vp, _vp, _i32]),
    "pinn_error_string": (C.c_char_p, [_i32]),
    "pinn_abi_version": (_i32, []),
}

# The profiling hook of the library is process-wide and keeps a raw host pointer: the buffer it writes to is owned HERE, at module
# level, for as long as the hook is on -- never by a PinnLib instance that may be collected while another engine still launches.
_PROFILE_BUFFER = None
_F8 = C.c_float * 8


class PinnLib:
    """Thin, checked wrapper over the shared library's entry points."""

    def __init__(self, path: str = DEFAULT_LIB):
        if not os.path.exists(path):
            raise PinnLibError(
                f"{path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C pinn_elastodynamics_amd/csrc hip`). There is no CPU fallback.")
        self.path = path
        self.lib = C.CDLL(path)
        # every entry of the table the library exports (one-variant experiment builds of older trees lack the newest ones; the product library is held
        # to the full set by tests/test_capi_symbols.py)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(self.lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes

    # -- helpers -------------------------------------------------------------------------------
    @staticmethod
    def _ints(v):
        return (C.c_int * len(v))(*[int(x) for x in v])

    @staticmethod
    def _floats(v, n):
        v = list(v) + [0.0] * (n - len(v))
        return (C.c_float * n)(*[float(x) for x in v])

    @staticmethod
    def _box(lb, ub, normalize, dim=3):
        """lb[dim], ub[dim], normalize"""
        arr = C.c_double * dim
        return arr(*[float(x) for x in lb]), arr(*[float(x) for x in ub]), int(bool(normalize))

    def _net_points(self, params, layers, cols, n, lb, ub, normalize):
        """the leading arguments of every per-point entry point: net, the 3 (x, y, t) or 4 (x, y, z, t) columns, n, box"""
        return (params, self._ints(layers), len(layers), *cols, int(n), *self._box(lb, ub, normalize, len(cols)))

    def _wave_head(self, E, mu, rho, plane_strain, term_weights):
        return float(E), float(mu), float(rho), int(bool(plane_strain)), self._floats(term_weights, 7)

    @staticmethod
    def _tail(prec, ws, ws_bytes, stream):
        """precision_mode, workspace, ws_bytes, stream"""
        return mode_bits(prec), ws, int(ws_bytes), stream

    @staticmethod
    def _set_array(struct, sets):
        """rows (x, y, t, n, targets_or_0, weights, loss_out) as a PointSet (weights: out_weights[<= 8]) or StreamSet (weights[5][<= 8]) array"""
        arr = (struct * max(1, len(sets)))()
        for a, (x, y, t, n, tg, w, lo) in zip(arr, sets):
            a.x, a.y, a.t, a.n, a.targets, a.loss_terms_out = x or None, y or None, t or None, int(n), tg or None, lo
            if struct is PointSet:
                a.out_weights = _F8(*[float(v) for v in w[:8]])
            else:
                a.weights = (_F8 * 5)(*[_F8(*[float(v) for v in row]) for row in w])
        return arr

    @staticmethod
    def adam_state(adam):
        """None or (m, v, lr, beta1, beta2, eps, step) -> the `const pinn_adam_state*` argument"""
        if adam is None:
            return None
        return C.byref(AdamState(adam[0], adam[1], float(adam[2]), float(adam[3]), float(adam[4]), float(adam[5]), int(adam[6])))

    def check(self, rc: int, what: str):
        if rc != 0:
            raise PinnLibError(f"{what} failed: {self.error_string(rc)}")

    def call(self, name: str, *args, accept=()) -> int:
        """Calls the library's ``name``; a return code other than 0 or one of ``accept`` raises PinnLibError under that name"""
        rc = getattr(self.lib, name)(*args)
        if rc not in accept:
            self.check(rc, name)
        return rc

    def error_string(self, rc: int) -> str:
        return f"{self.lib.pinn_error_string(rc).decode()} (code {rc})"

    # -- entry points --------------------------------------------------------------------------
    def abi_version(self) -> int:
        return self.lib.pinn_abi_version()

    def set_profile_buffer(self, enable: bool):
        """Process-wide profiling hook: while on, every loss+gradient call writes its kernel milliseconds {repack, chain or whole
        fused kernel, weight gradient, reductions} into the returned float32[4] (and synchronises the stream)."""
        global _PROFILE_BUFFER
        if enable:
            if _PROFILE_BUFFER is None:
                _PROFILE_BUFFER = (C.c_float * 4)()
            self.lib.pinn_debug_set_profile_buffer(C.cast(_PROFILE_BUFFER, C.c_void_p))
            import numpy as _np
            return _np.ctypeslib.as_array(_PROFILE_BUFFER)
        self.lib.pinn_debug_set_profile_buffer(None)      # (the module-level buffer stays allocated: a launch in flight may still write to it)
        return None

    def profile_ring_arm(self, max_launches: int, every: int = 1) -> int:
        """Start recording the next launches of the fused kernel with HIP events in stream order, nothing synchronises (include/pinn_hip.h);
        ``every`` > 1: the launches of every ``every``-th step only"""
        self.lib.pinn_debug_profile_ring_stride(int(every))
        return int(self.lib.pinn_debug_profile_ring_arm(int(max_launches)))

    def set_stamp_buffer(self, device_ptr) -> None:
        """128 x uint64 device buffer for the fused kernel's shader-clock stamps of workgroup 0 (None: off)"""
        self.lib.pinn_debug_set_stamp_buffer(None if device_ptr is None else C.c_void_p(int(device_ptr)))

    def path_for(self, layers, precision, head: str = "wave", ws_bytes: int = 0) -> str:
        """pinn_path_for: 'fused-registers' | 'fused-lds' | 'two-kernel' | 'fp32' for a loss + gradient call of family ``head``
        ('wave', 'data', 'plate', 'nc3d', 'nc3d_data', 'streams', 'stream_sets'); ``precision`` is a mode name or the full precision_mode word"""
        rc = int(self.lib.pinn_path_for(self._ints(layers), len(layers), mode_bits(precision), HEADS[head], int(ws_bytes)))
        if rc <= 0:
            raise PinnLibError(f"pinn_path_for failed: {self.error_string(rc)}")
        return PATHS[rc]

    def cache_policy(self, layers, head: str = "wave") -> dict:
        """pinn_debug_cache_policy: per-workgroup bytes of the fused collocation kernel's two memory classes and which of them (if any) the
        instantiation marks non-temporal -- {'policy': 'none' | 'sums' | 'images', 'images_bytes', 'sums_bytes', 'grid_bytes' (256 workgroups)}"""
        im, su = C.c_size_t(0), C.c_size_t(0)
        rc = int(self.lib.pinn_debug_cache_policy(self._ints(layers), len(layers), HEADS[head], C.byref(im), C.byref(su)))
        if rc < 0:
            raise PinnLibError(f"pinn_debug_cache_policy failed: {self.error_string(rc)}")
        return {"policy": ("none", "sums", "images")[rc], "images_bytes": int(im.value), "sums_bytes": int(su.value), "grid_bytes": 256 * (int(im.value) + int(su.value))}

    def path_counts(self, reset: bool = False) -> dict:
        """calls per path since the last reset (pinn_debug_path_counts)"""
        buf = (C.c_int64 * 5)()
        self.lib.pinn_debug_path_counts(C.cast(buf, C.c_void_p), int(bool(reset)))
        return {PATHS[i]: int(buf[i]) for i in range(1, 5)}

    def profile_ring_read(self):
        """Stop the recording and return (milliseconds, streams) of the recorded launches, in launch order"""
        import numpy as _np
        cap = 4096
        ms = (C.c_float * cap)()
        tags = (C.c_int * cap)()
        m = int(self.lib.pinn_debug_profile_ring_read(C.cast(ms, C.c_void_p), C.cast(tags, C.c_void_p), cap))
        return _np.array(ms[:m], dtype=_np.float64), _np.array(tags[:m], dtype=_np.int64)

    def profiling(self):
        """Context manager around set_profile_buffer: the hook is always reset, whatever the body raises."""
        lib = self

        class _Ctx:
            def __enter__(self_inner):
                return lib.set_profile_buffer(True)

            def __exit__(self_inner, *exc):
                lib.set_profile_buffer(False)
                return False
        return _Ctx()

    def set_fused(self, enable) -> int:
        """0: two-kernel path, 1: fused kernel where it applies (default)"""
        return int(self.lib.pinn_debug_set_fused(int(bool(enable))))

    def set_step_launch(self, enable) -> int:
        """0: the step entry points make their separate calls inside, 1: the one launch where it applies (default)"""
        return int(self.lib.pinn_debug_set_step_launch(int(bool(enable))))

    def fused_weight_limit(self) -> float:
        return float(self.lib.pinn_fused_weight_limit())

    def supported_width(self, h: int) -> int:
        return self.lib.pinn_supported_width(int(h))

    def workspace_bytes(self, layers, n, prec) -> int:
        return int(self.lib.pinn_workspace_bytes(self._ints(layers), len(layers), int(n), mode_bits(prec)))

    def min_workspace_bytes(self, layers, prec) -> int:
        return int(self.lib.pinn_min_workspace_bytes(self._ints(layers), len(layers), mode_bits(prec)))

    def wave2d_loss_grad(self, params, layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, term_weights,
                         loss_out, grad_out, accumulate, prec, ws, ws_bytes, stream=0):
        self.call("pinn_wave2d_loss_grad", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize),
                  *self._wave_head(E, mu, rho, plane_strain, term_weights), loss_out, grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream))

    def wave2d_loss_grad_checked(self, params, layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, term_weights,
                                 loss_out, grad_out, prec, ws, ws_bytes, state: "RangeState", stream=0) -> int:
        """pinn_wave2d_loss_grad_checked: the call + the finite-gradient ladder, synchronous; ``state`` is kept by the caller.  Returns the rc
        (PINN_ERR_RANGE = -7 is a result a caller may want to handle, everything else raises)."""
        return self.call("pinn_wave2d_loss_grad_checked", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize),
                         *self._wave_head(E, mu, rho, plane_strain, term_weights), loss_out, grad_out, *self._tail(prec, ws, ws_bytes, stream),
                         C.byref(state), accept=(-7,))

    def probe_ranges(self, params, grad, n_params, ws, ws_bytes, stream=0):
        """(gradient finite?, max |w|) -- one small reduction and a stream synchronisation"""
        fin, wmax = C.c_int32(0), C.c_float(0.0)
        self.call("pinn_probe_ranges", params or None, grad or None, int(n_params), ws, int(ws_bytes), stream, C.byref(fin), C.byref(wmax))
        return bool(fin.value), float(wmax.value)

    def wave2d_loss_grad_profile(self, params, layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, term_weights,
                                 loss_out, grad_out, accumulate, prec, ws, ws_bytes, stream=0):
        """Synchronous; returns [repack, chain, wgrad, reductions] kernel milliseconds (HIP events)."""
        ms = (C.c_float * 4)()
        self.call("pinn_wave2d_loss_grad_profile", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize),
                  *self._wave_head(E, mu, rho, plane_strain, term_weights), loss_out, grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream), ms)
        return [float(v) for v in ms]

    def data_loss_grad(self, params, layers, x, y, t, n, lb, ub, normalize, targets, out_weights, loss_out, grad_out,
                       accumulate, prec, ws, ws_bytes, stream=0):
        self.call("pinn_data_loss_grad", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), targets, self._floats(out_weights, 8),
                  loss_out, grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream))

    def data_loss_grad_multi(self, params, layers, sets, lb, ub, normalize, grad_out, accumulate, prec, ws, ws_bytes, stream=0):
        """sets: list of (x, y, t, n, targets_or_0, out_weights, loss_out) with device pointers as integers."""
        self.call("pinn_data_loss_grad_multi", params, self._ints(layers), len(layers), self._set_array(PointSet, sets), len(sets),
                  *self._box(lb, ub, normalize), grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream))

    def wave2d_step(self, params, layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, term_weights, loss_out, sets, grad_out,
                    accumulate, adam, prec, ws, ws_bytes, stream=0):
        """pinn_wave2d_step.  sets: as data_loss_grad_multi; adam: None or (m, v, lr, beta1, beta2, eps, step)."""
        self.call("pinn_wave2d_step", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize),
                  *self._wave_head(E, mu, rho, plane_strain, term_weights), loss_out, self._set_array(PointSet, sets), len(sets), grad_out,
                  int(bool(accumulate)), self.adam_state(adam), *self._tail(prec, ws, ws_bytes, stream))

    def plate2d_step(self, params, layers, x, y, t, n, lb, ub, normalize, frozen, E, mu, rho, term_weights, loss_out, hx, hy, ht, hn, haux, hweights,
                     hloss_out, grad_out, accumulate, adam, prec, ws, ws_bytes, stream=0):
        """pinn_plate2d_step.  adam: None or (m, v, lr, beta1, beta2, eps, step)."""
        self.call("pinn_plate2d_step", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), frozen, float(E), float(mu), float(rho),
                  self._floats(term_weights, 5), loss_out, hx, hy, ht, int(hn), haux, self._floats(hweights, 2), hloss_out, grad_out,
                  int(bool(accumulate)), self.adam_state(adam), *self._tail(prec, ws, ws_bytes, stream))

    def wave2d_traction_loss_grad(self, params, layers, x, y, t, n, lb, ub, normalize, aux, weights, loss_out, grad_out, accumulate,
                                  prec, ws, ws_bytes, stream=0):
        """pinn_wave2d_traction_loss_grad.  aux: device [4][n] = nx, ny, tx, ty; loss_out: 2 floats (sum r_x^2, sum r_y^2)"""
        self.call("pinn_wave2d_traction_loss_grad", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), aux, self._floats(weights, 2),
                  loss_out, grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream))

    def wave2d_step_traction(self, params, layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, term_weights, loss_out, sets, tx, ty, tt, tn,
                             taux, tweights, tloss_out, grad_out, accumulate, adam, prec, ws, ws_bytes, stream=0):
        """pinn_wave2d_step_traction.  sets / adam: as wave2d_step; (tx, ty, tt, tn, taux, tweights, tloss_out): the traction set."""
        self.call("pinn_wave2d_step_traction", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize),
                  *self._wave_head(E, mu, rho, plane_strain, term_weights), loss_out, self._set_array(PointSet, sets), len(sets),
                  tx or None, ty or None, tt or None, int(tn), taux or None, self._floats(tweights, 2), tloss_out or None, grad_out,
                  int(bool(accumulate)), self.adam_state(adam), *self._tail(prec, ws, ws_bytes, stream))

    def wave2d_fields(self, params, layers, x, y, t, n, lb, ub, normalize, fields_out, prec, ws, ws_bytes, stream=0):
        self.call("pinn_wave2d_fields", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), fields_out, *self._tail(prec, ws, ws_bytes, stream))

    def wave2d_residual_score(self, params, layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, term_weights, score_out, prec, ws,
                              ws_bytes, stream=0):
        self.call("pinn_wave2d_residual_score", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize),
                  *self._wave_head(E, mu, rho, plane_strain, term_weights), score_out, *self._tail(prec, ws, ws_bytes, stream))

    def wave2d_predict(self, params, layers, x, y, t, n, lb, ub, normalize, out, prec, ws, ws_bytes, stream=0):
        """pinn_wave2d_predict: out [8][n] = u, v, s11, s22, s12, e11, e22, e12"""
        self.call("pinn_wave2d_predict", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), out, *self._tail(prec, ws, ws_bytes, stream))

    def plate2d_predict(self, params, layers, x, y, t, n, lb, ub, normalize, frozen, out, prec, ws, ws_bytes, stream=0):
        """pinn_plate2d_predict: frozen [2][5][5][n] (stream rows 0..2 read), out [8][n] in the order of wave2d_predict"""
        self.call("pinn_plate2d_predict", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), frozen, out, *self._tail(prec, ws, ws_bytes, stream))

    def material_sums_workspace_bytes(self) -> int:
        return int(self.lib.pinn_material_sums_workspace_bytes())

    def wave2d_material_sums(self, params, layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, sums_out, prec, ws, ws_bytes,
                             sums_ws, sums_ws_bytes, stream=0):
        """pinn_wave2d_material_sums: sums_out (device, MATERIAL_SUMS doubles) = the seven sums of squared wave residuals, then the seven
        moment sums of include/pinn_hip.h; sums_ws: material_sums_workspace_bytes() of scratch"""
        self.call("pinn_wave2d_material_sums", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), float(E), float(mu), float(rho),
                  int(bool(plane_strain)), sums_out, *self._tail(prec, ws, ws_bytes, stream)[:3], sums_ws, int(sums_ws_bytes), stream)

    def field_error_workspace_bytes(self, n, n_rows) -> int:
        return int(self.lib.pinn_field_error_workspace_bytes(int(n), int(n_rows)))

    def field_error_sums(self, pred, pred_rows, rows, ref, n, sums_out, ws, ws_bytes, stream=0):
        """pinn_field_error_sums: sums_out (device, 2 * len(rows) doubles) = sum (pred[rows[j]] - ref[j])^2, then sum ref[j]^2"""
        rows = [int(r) for r in rows]
        self.call("pinn_field_error_sums", pred, int(pred_rows), (C.c_int * max(1, len(rows)))(*rows), len(rows), ref, int(n), sums_out, ws,
                  int(ws_bytes), stream)

    def select_workspace_bytes(self, n) -> int:
        return int(self.lib.pinn_select_workspace_bytes(int(n)))

    def select_k(self, score, n, k, largest, idx_out, ws, ws_bytes, stream=0):
        self.call("pinn_select_k", score, int(n), int(k), int(bool(largest)), idx_out, ws, int(ws_bytes), stream)

    def sample_box(self, seed, stream_id, first, n, lo, hi, cols, stream=0, t_cdf=None, n_bins=0):
        """pinn_sample_box.  cols: the 3 (x, y, t) or 4 (x, y, z, t) device pointers; lo / hi: as many bounds.  With ``t_cdf`` (a device
        pointer to n_bins + 1 floats): pinn_sample_box_cdf, the time column drawn from that table."""
        dim = len(cols)
        x, y, z, t = (cols[0], cols[1], None, cols[2]) if dim == 3 else (tuple(cols) + (None,) * 4)[:4]
        d4 = lambda v: (C.c_double * 4)(*([float(a) for a in v] + [0.0] * 4)[:4])
        if t_cdf is None:
            self.call("pinn_sample_box", int(seed), int(stream_id), int(first), int(n), dim, d4(lo), d4(hi), x, y, z, t, stream)
        else:
            self.call("pinn_sample_box_cdf", int(seed), int(stream_id), int(first), int(n), dim, d4(lo), d4(hi), t_cdf, int(n_bins), x, y, z, t, stream)

    def binned_sums_workspace_bytes(self, n, n_bins) -> int:
        return int(self.lib.pinn_binned_sums_workspace_bytes(int(n), int(n_bins)))

    def binned_sums(self, value, coord, n, lo, hi, n_bins, sums_out, ws, ws_bytes, stream=0):
        """pinn_binned_sums: sums_out (device, 2 * n_bins doubles) = per bin of [lo, hi] the sum of value, then the count"""
        self.call("pinn_binned_sums", value, coord, int(n), float(lo), float(hi), int(n_bins), sums_out, ws, int(ws_bytes), stream)

    def causal_cdf(self, binned, n_bins, eps, floor, w_out, cdf_out, stream=0):
        """pinn_causal_cdf: w_out (device, n_bins doubles), cdf_out (device, n_bins + 1 floats) from the output of binned_sums"""
        self.call("pinn_causal_cdf", binned, int(n_bins), float(eps), float(floor), w_out, cdf_out, stream)

    def refine_keys_workspace_bytes(self, n) -> int:
        return int(self.lib.pinn_refine_keys_workspace_bytes(int(n)))

    def refine_keys(self, score, n, x, y, z, balls, mode, power, c, seed, stream_id, first, key_out, ws, ws_bytes, stream=0):
        """pinn_refine_keys.  balls: see ball_array; mode: 'mask' | 'sample'."""
        self.call("pinn_refine_keys", score, int(n), x, y, z, ball_array(balls), len(balls), KEYS_MODE[mode], float(power), float(c), int(seed),
                  int(stream_id), int(first), key_out, ws, int(ws_bytes), stream)

    def net_streams(self, params, layers, x, y, t, n, lb, ub, normalize, streams_out, prec, ws, ws_bytes, stream=0):
        self.call("pinn_net_streams", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), streams_out, *self._tail(prec, ws, ws_bytes, stream))

    def plate2d_loss_grad(self, params, layers, x, y, t, n, lb, ub, normalize, frozen, E, mu, rho, term_weights, loss_out, grad_out,
                          accumulate, prec, ws, ws_bytes, stream=0):
        self.call("pinn_plate2d_loss_grad", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), frozen, float(E), float(mu), float(rho),
                  self._floats(term_weights, 5), loss_out, grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream))

    def plate2d_residual_score(self, params, layers, x, y, t, n, lb, ub, normalize, frozen, E, mu, rho, term_weights, score_out, prec, ws, ws_bytes,
                               stream=0):
        self.call("pinn_plate2d_residual_score", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), frozen, float(E), float(mu),
                  float(rho), self._floats(term_weights, 5), score_out, *self._tail(prec, ws, ws_bytes, stream))

    def nc3d_residual_score(self, params, layers, x, y, z, t, n, lb, ub, normalize, E, mu, rho, term_weights, score_out, prec, ws, ws_bytes,
                            stream=0):
        self.call("pinn_nc3d_residual_score", *self._net_points(params, layers, (x, y, z, t), n, lb, ub, normalize), float(E), float(mu), float(rho),
                  self._floats(term_weights, 12), score_out, *self._tail(prec, ws, ws_bytes, stream))

    def plate2d_material_sums(self, params, layers, x, y, t, n, lb, ub, normalize, frozen, E, mu, rho, sums_out, prec, ws, ws_bytes, sums_ws,
                              sums_ws_bytes, stream=0):
        """pinn_plate2d_material_sums: sums_out (device, MATERIAL_SUMS_PLATE doubles) = the five sums of squared plate residuals, then the
        seven moment sums of include/pinn_hip.h; frozen [2][5][5][n]; sums_ws: material_sums_workspace_bytes() of scratch"""
        self.call("pinn_plate2d_material_sums", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), frozen, float(E), float(mu),
                  float(rho), sums_out, *self._tail(prec, ws, ws_bytes, stream)[:3], sums_ws, int(sums_ws_bytes), stream)

    def nc3d_material_sums(self, params, layers, x, y, z, t, n, lb, ub, normalize, E, mu, rho, sums_out, prec, ws, ws_bytes, sums_ws,
                           sums_ws_bytes, stream=0):
        """pinn_nc3d_material_sums: sums_out (device, MATERIAL_SUMS_NC3D doubles) = the twelve sums of squared 3-D residuals, then the twelve
        moment sums of include/pinn_hip.h"""
        self.call("pinn_nc3d_material_sums", *self._net_points(params, layers, (x, y, z, t), n, lb, ub, normalize), float(E), float(mu),
                  float(rho), sums_out, *self._tail(prec, ws, ws_bytes, stream)[:3], sums_ws, int(sums_ws_bytes), stream)

    def plate2d_traction_loss_grad(self, params, layers, x, y, t, n, lb, ub, normalize, aux, weights, loss_out, grad_out, accumulate,
                                   prec, ws, ws_bytes, stream=0):
        self.call("pinn_plate2d_traction_loss_grad", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), aux, self._floats(weights, 2),
                  loss_out, grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream))

    def stream_loss_grad(self, params, layers, x, y, t, n, lb, ub, normalize, targets, weights, loss_out, grad_out, accumulate, prec,
                         ws, ws_bytes, stream=0):
        w = [float(v) for row in weights for v in row]
        self.call("pinn_stream_loss_grad", *self._net_points(params, layers, (x, y, t), n, lb, ub, normalize), targets, (C.c_float * len(w))(*w),
                  loss_out, grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream))

    def stream_loss_grad_multi(self, params, layers, sets, lb, ub, normalize, grad_out, accumulate, prec, ws, ws_bytes, stream=0):
        """pinn_stream_loss_grad_multi.  sets: list of (x, y, t, n, targets_or_0, weights[5][<=8], loss_out) with device pointers as
        integers; the reported sums of every set are normalised by the largest |weight| of the whole call."""
        self.call("pinn_stream_loss_grad_multi", params, self._ints(layers), len(layers), self._set_array(StreamSet, sets), len(sets),
                  *self._box(lb, ub, normalize), grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream))

    # -- 3-D Navier-Cauchy extension (4 inputs x, y, z, t; 12 outputs) ---------------------------------------------
    def nc3d_loss_grad(self, params, layers, x, y, z, t, n, lb, ub, normalize, E, mu, rho, term_weights, loss_out, grad_out, accumulate,
                       prec, ws, ws_bytes, stream=0):
        self.call("pinn_nc3d_loss_grad", *self._net_points(params, layers, (x, y, z, t), n, lb, ub, normalize), float(E), float(mu), float(rho),
                  self._floats(term_weights, 12), loss_out, grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream))

    def nc3d_data_loss_grad(self, params, layers, x, y, z, t, n, lb, ub, normalize, targets, out_weights, loss_out, grad_out, accumulate,
                            prec, ws, ws_bytes, stream=0):
        self.call("pinn_nc3d_data_loss_grad", *self._net_points(params, layers, (x, y, z, t), n, lb, ub, normalize), targets,
                  self._floats(out_weights, 16), loss_out, grad_out, int(bool(accumulate)), *self._tail(prec, ws, ws_bytes, stream))

    def nc3d_fields(self, params, layers, x, y, z, t, n, lb, ub, normalize, fields_out, prec, ws, ws_bytes, stream=0):
        self.call("pinn_nc3d_fields", *self._net_points(params, layers, (x, y, z, t), n, lb, ub, normalize), fields_out, *self._tail(prec, ws, ws_bytes, stream))

    def adam_step(self, params, m, v, grad, n_params, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, stream=0):
        self.call("pinn_adam_step", params, m, v, grad, int(n_params), float(lr), float(beta1), float(beta2), float(eps), int(step), stream)

    # -- L-BFGS on the device (pinn_lbfgs_*) ---------------------------------------------------------------------------
    def lbfgs_state_bytes(self, n_params: int, history: int) -> int:
        return int(self.lib.pinn_lbfgs_state_bytes(int(n_params), int(history)))

    def lbfgs_init(self, state, state_bytes, n_params, options: dict, loss_coeffs, grad_scale=1.0, stream=0):
        """pinn_lbfgs_init.  options: scipy's names (maxcor, maxiter, maxfun, maxls, ftol, gtol); loss = sum_j loss_coeffs[j] * sums[j]."""
        o = LbfgsOptions(int(options.get("maxcor", 10)), int(options.get("maxiter", 15000)), int(options.get("maxfun", 15000)), int(options.get("maxls", 20)),
                         float(options.get("ftol", 2.220446049250313e-09)), float(options.get("gtol", 1e-5)))
        c = [float(v) for v in loss_coeffs]
        self.call("pinn_lbfgs_init", state or None, int(state_bytes), int(n_params), C.byref(o), (C.c_float * max(1, len(c)))(*c), len(c),
                  float(grad_scale), stream)

    def lbfgs_advance(self, state, params, grad, sums, stream=0):
        self.call("pinn_lbfgs_advance", state or None, params or None, grad or None, sums or None, stream)

    def lbfgs_status(self, state, stream=0) -> dict:
        """pinn_lbfgs_status (synchronises the stream): the record as a dict, with 'status_name' from LBFGS_STATUS"""
        r = LbfgsRecord()
        self.call("pinn_lbfgs_status", state or None, C.byref(r), stream)
        return r.as_dict()

    def lbfgs_read_losses(self, state, first: int, count: int, stream=0):
        """losses of the evaluations [first, first + count) as a list of floats (synchronises)"""
        out = (C.c_double * max(1, int(count)))()
        self.call("pinn_lbfgs_read_losses", state or None, int(first), int(count), out, stream)
        return [float(v) for v in out[:int(count)]]

    def lbfgs_debug_read(self, state, n_params: int, history: int, stream=0):
        """(direction [P], S [pairs, P], Y [pairs, P]) as numpy arrays, pairs oldest first (pinn_lbfgs_debug_read; tests)"""
        import numpy as _np
        d = _np.zeros(int(n_params), dtype=_np.float32)
        S = _np.zeros((int(history), int(n_params)), dtype=_np.float32)
        Y = _np.zeros_like(S)
        n = C.c_int(0)
        self.call("pinn_lbfgs_debug_read", state or None, int(n_params), int(history), d.ctypes.data, S.ctypes.data, Y.ctypes.data, int(history),
                  C.byref(n), stream)
        return d, S[:n.value].copy(), Y[:n.value].copy()
