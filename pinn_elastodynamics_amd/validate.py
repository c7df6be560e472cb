"""The output side of a training run on the device: what the model classes share for predict_device / predict_frames / validate and for
train(validate=...) (elastic_wave.DeepHPM, plate_hole.PINN).  The fields come from the predict head of the
class's family (engine.wave_predict / plate_predict: value and space tangents only), the comparison with reference data from
engine.field_error_sums: per field  sum (pred - ref)^2  and  sum ref^2  in fp64 on the device; only the 2 x fields doubles come to the host.
"""
from __future__ import annotations

import numpy as np
import torch

from .optim import device_column


def tile_frames(space_cols, times, device):
    """The same spatial points at every time of ``times``, tiled on the device: frame k holds rows k*n .. (k+1)*n - 1.  Returns
    (tiled space columns, tiled time column, T, n)."""
    cols = [device_column(a, device) for a in space_cols]
    tt = device_column(times, device)
    T, n = int(tt.numel()), int(cols[0].numel())
    return [c.repeat(T) for c in cols], tt.repeat_interleave(n), T, n


def field_rows(names, fields):
    """rows of the predict output for the field names ``fields`` (``names``: the order of the class's predict tuple)"""
    rows = []
    for f in fields:
        if f not in names:
            raise ValueError(f"unknown field {f!r}: predict returns {tuple(names)}")
        rows.append(names.index(f))
    if not 1 <= len(rows) <= 16:
        raise ValueError("fields: 1 to 16 names")
    return rows


def reference_rows(ref, fields, n, device):
    """the reference columns ref[name] (numpy [N,1] / [N] or device tensors) of ``fields`` as one fp32 device tensor [len(fields), n]"""
    rows = []
    for f in fields:
        if f not in ref:
            raise ValueError(f"ref has no column {f!r}")
        c = device_column(ref[f], device)
        if c.numel() != n:
            raise ValueError(f"ref[{f!r}] has {c.numel()} rows, the points {n}")
        rows.append(c)
    return torch.stack(rows).contiguous()


def relative_l2(sums, fields):
    """host [2, k] sums -> dict name -> sqrt(sum (pred - ref)^2 / sum ref^2)"""
    s = np.asarray(sums, dtype=np.float64).reshape(2, len(fields))
    with np.errstate(divide="ignore", invalid="ignore"):
        return {f: float(np.sqrt(s[0, j] / s[1, j])) for j, f in enumerate(fields)}


def error_sums(model, cols, ref_rows, rows, aux=None):
    """one predict call at the device columns ``cols`` (``aux``: what model._predict_aux(cols) returned, or None), one error-sums call: the
    device tensor [2, len(rows)] of doubles"""
    pred = model._predict_cols(cols) if aux is None else model._predict_cols(cols, aux)
    return model._predict_engine().field_error_sums(pred, rows, ref_rows)


def validate(model, cols, ref, fields):
    """model.validate: one predict call, one error-sums call, one download of 2 * len(fields) doubles"""
    fields = tuple(fields)
    rows = field_rows(list(model.PREDICT_FIELDS), fields)
    cols = [device_column(a, model.device) for a in cols]
    ref_rows = reference_rows(ref, fields, int(cols[0].numel()), model.device)
    return relative_l2(error_sums(model, cols, ref_rows, rows).cpu().numpy(), fields)


class ValidateSchedule:
    """train(..., validate=dict(every=E, points=(x, y, [z,] t), ref={name: column}, fields=(...))): the relative L2 of ``fields`` against
    ``ref`` at ``points`` behind every E-th step of the call.  Points and reference are uploaded once, here; ``after_step(j)`` (j = 1, 2, ...
    counted over the whole train call) enqueues a predict and an error-sums call and keeps the sums on the device; ``flush()`` -- called at
    the block's existing host synchronisation -- downloads them and appends (step, dict) to ``model.val_rec``.  Data parallel: every rank
    evaluates the same points with the same parameters and gets the same numbers; no collective."""

    def __init__(self, model, validate):
        kw = dict(validate)
        try:
            self.every, points, ref = int(kw.pop("every")), kw.pop("points"), kw.pop("ref")
        except KeyError as e:
            raise ValueError(f"validate: missing {e.args[0]!r} (need every, points, ref)") from None
        self.fields = tuple(kw.pop("fields", model.VALIDATE_FIELDS))
        if kw:
            raise ValueError(f"validate: unknown entries {sorted(kw)}")
        if self.every < 1:
            raise ValueError("validate: every >= 1")
        if len(points) != len(model.PREDICT_INPUTS):
            raise ValueError(f"validate: points = {model.PREDICT_INPUTS}")
        self.model = model
        self.rows = field_rows(list(model.PREDICT_FIELDS), self.fields)
        self.cols = [device_column(a, model.device) for a in points]
        self.ref_rows = reference_rows(ref, self.fields, int(self.cols[0].numel()), model.device)
        self.aux = model._predict_aux(self.cols)      # what does not change while the net trains (the plate's frozen D / P streams), once
        self.pending = []
        if not hasattr(model, "val_rec"):
            model.val_rec = []

    def after_step(self, step):
        if step % self.every == 0:
            self.pending.append((step, error_sums(self.model, self.cols, self.ref_rows, self.rows, self.aux)))

    def flush(self):
        if self.pending:
            host = torch.stack([s for _, s in self.pending]).cpu().numpy()
            for (step, _), s in zip(self.pending, host):
                self.model.val_rec.append((step, relative_l2(s, self.fields)))
            self.pending = []


def schedule(model, validate):
    """the ValidateSchedule of train(validate=...), or None for validate=None"""
    return None if validate is None else ValidateSchedule(model, validate)


class PredictMixin:
    """predict_device / predict_frames / validate of a model class.  The class supplies PREDICT_FIELDS (the names of predict's tuple, in
    order), PREDICT_INPUTS (the coordinate names), VALIDATE_FIELDS (the default fields of validate: what FEM frames carry), ``device``,
    ``_predict_cols(device columns[, aux]) -> device tensor [rows, n]`` and ``_predict_engine()``; ``_predict_aux(device columns)`` may return what
    a repeated evaluation at the same points can reuse (None: nothing)."""

    def _predict_aux(self, xs):
        return None

    def predict_device(self, *cols):
        """predict's fields at the points (numpy columns or device tensors), formed by the family's predict head: the device tensor
        [len(PREDICT_FIELDS), N], rows in the order of predict's tuple.  No host synchronisation."""
        if len(cols) != len(self.PREDICT_INPUTS):
            raise ValueError(f"predict_device{self.PREDICT_INPUTS}")
        return self._predict_cols([device_column(a, self.device) for a in cols])

    def predict_frames(self, *cols):
        """predict_device of the same spatial points at every time of the last argument ``times``: the coordinates are tiled on the device
        (no host meshgrid, no upload per frame), ONE predict call; returns the device tensor [T, rows, n_xy] (a view of the call's output)."""
        if len(cols) != len(self.PREDICT_INPUTS):
            raise ValueError(f"predict_frames{self.PREDICT_INPUTS[:-1] + ('times',)}")
        space, tt, T, n = tile_frames(cols[:-1], cols[-1], self.device)
        out = self._predict_cols(space + [tt])
        return out.reshape(out.shape[0], T, n).permute(1, 0, 2)

    def validate(self, *args, fields=None):
        """validate(x, y, [z,] t, ref, fields=(...)): relative L2 = sqrt(sum (pred - ref)^2 / sum ref^2) of the named fields of predict
        against the columns ``ref[name]`` (e.g. pointsets.preprocess) at the points -- one predict call, one error-sums call, one download of
        2 * len(fields) doubles.  Returns dict name -> float.  An unknown field name raises ValueError."""
        if len(args) != len(self.PREDICT_INPUTS) + 1:
            raise ValueError(f"validate{self.PREDICT_INPUTS + ('ref',)}")
        return validate(self, args[:-1], args[-1], self.VALIDATE_FIELDS if fields is None else fields)
