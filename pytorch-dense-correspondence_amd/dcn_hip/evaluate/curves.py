"""The curves of an evaluation table (csrc/curve_kernels.hip): make_cdf_plot and compute_area_above_curve
(evaluation.py:2658-2674, :2844-2863)."""
import collections
import os

import numpy as np
import torch

from .. import _lib
from ._chain import COLUMNS, EvalTable, _rows
from .across_objects import AcrossObjectTable

CURVE_FIELDS = ("pixel_match_error_l2", "pixel_match_error_l2_masked", "norm_diff_pred_3d", "norm_diff_pred_3d_masked",
                "norm_diff_descriptor_ground_truth", "fraction_pixels_closer_than_ground_truth",
                "fraction_pixels_closer_than_ground_truth_masked", "average_l2_distance_for_false_positives",
                "average_l2_distance_for_false_positives_masked")     # the nine columns the reference plots
CURVE_DROP_NAN = ("norm_diff_pred_3d", "norm_diff_pred_3d_masked")    # the two it dropna()s (make_descriptor_accuracy_plot)
CURVE_EMPTY, CURVE_NAN, CURVE_NONFINITE = 1, 2, 4                     # DCN_CURVE_*
CURVE_SUMMARY = ("count", "dropped", "min", "max", "lowerlimit", "binsize", "area_above_curve", "flags")
MAX_CURVES, MAX_CURVE_BINS = 64, 4096


class EvalCurves(collections.namedtuple("EvalCurves", "fields cumcount cdf summary status num_bins")):
    """``fields``: the curves' names, C of them; device tensors cumcount int64 [C, num_bins], cdf float64 [C, num_bins],
    summary float64 [C, 8] in the order of CURVE_SUMMARY, status int32 [1] (the OR of the curves' flags)."""


def cumulative_frequencies(values, row_pair=None, num_bins=100, drop_nan=False, out_summary=None, fields=None):
    """``scipy.stats.cumfreq(values[k], num_bins)`` times ``1.0 / len(values[k])`` and the area above it, for every row k of
    ``values`` (float64 [C, R] or [R]; C <= 64) in one launch (csrc/curve_kernels.hip, include/dcn_hip.h section 14).
    ``row_pair`` int32 [R]: rows with a negative entry do not belong to the table.  ``drop_nan``: a bool or one per curve
    (``dropna()``).  ``out_summary``: the contiguous float64 [C, 8] device tensor the kernel writes its summary to (a view
    into a larger tensor will do).  ``fields``: names for EvalCurves.fields (default 0 .. C - 1).  Nothing is read back."""
    if not torch.is_tensor(values) or values.dtype != torch.float64:
        raise TypeError("values must be a float64 tensor, got %s" % (values.dtype if torch.is_tensor(values) else
                                                                     type(values).__name__))
    if values.dim() == 1:
        values = values.view(1, -1)
    if values.dim() != 2:
        raise ValueError("values must be [C, R] or [R], got %s" % (tuple(values.shape),))
    C, R = int(values.shape[0]), int(values.shape[1])
    nb = int(num_bins)
    if not 1 <= C <= MAX_CURVES:
        raise ValueError("1 .. %d curves per call, got %d" % (MAX_CURVES, C))
    if not 2 <= nb <= MAX_CURVE_BINS:
        raise ValueError("num_bins must be 2 .. %d, got %d" % (MAX_CURVE_BINS, nb))
    if R > 0 and (values.stride(1) != 1 or (C > 1 and values.stride(0) < R)):
        values = values.contiguous()
    ld = int(values.stride(0)) if C > 1 and R > 0 else R
    dev = values.device
    if row_pair is not None:
        row_pair = _rows(row_pair, torch.int32, "row_pair", R)
        if row_pair.device != dev:
            raise ValueError("row_pair is on %s, values on %s" % (row_pair.device, dev))
    drops = [bool(drop_nan)] * C if isinstance(drop_nan, (bool, int, np.bool_)) else [bool(d) for d in drop_nan]
    if len(drops) != C:
        raise ValueError("drop_nan: one per curve (%d), got %d" % (C, len(drops)))
    names = tuple(range(C)) if fields is None else tuple(fields)
    if len(names) != C:
        raise ValueError("fields: one per curve (%d), got %d" % (C, len(names)))
    if out_summary is None:
        out_summary = torch.empty((C, len(CURVE_SUMMARY)), dtype=torch.float64, device=dev)
    elif out_summary.dtype != torch.float64 or tuple(out_summary.shape) != (C, len(CURVE_SUMMARY)) \
            or not out_summary.is_contiguous() or out_summary.device != dev:
        raise ValueError("out_summary must be a contiguous float64 [%d, %d] tensor on %s" % (C, len(CURVE_SUMMARY), dev))
    _lib.require_device(values, row_pair, out_summary)
    # (a bool tensor filled from the host: stream-ordered, no read)
    drop = torch.tensor(drops, dtype=torch.uint8).to(dev, non_blocking=True)
    cumcount = torch.empty((C, nb), dtype=torch.int64, device=dev)
    cdf = torch.empty((C, nb), dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    rc = _lib.get().dcn_eval_curves(C, R, ld, p(values) if R > 0 else None, p(row_pair), p(drop), nb, p(cumcount), p(cdf),
                                    p(out_summary), p(status), _lib.stream_ptr())
    _lib.check(rc, "dcn_eval_curves")
    return EvalCurves(names, cumcount, cdf, out_summary, status, nb)


def evaluation_curves(table, fields=None, num_bins=100, *, drop_nan=None, out_summary=None):
    """The curves of an evaluation table on the device.  ``table``: an EvalTable (same-scene, cross-scene, cross-instance or
    keypoints: the rows of ``columns`` named by ``fields``, default CURVE_FIELDS, NaNs dropped for the fields of
    CURVE_DROP_NAN) or an AcrossObjectTable (``norm_diff_descriptor_best_match``, converted to float64 on the device, no
    NaN dropped); ``row_pair`` selects the rows.  ``drop_nan`` overrides the per-field rule (``area_above_curve`` passes
    True).  ValueError for a field the table does not have.  -> EvalCurves; nothing is read back."""
    if isinstance(table, AcrossObjectTable):
        have = ("norm_diff_descriptor_best_match",)
        fields = have if fields is None else tuple(fields)
        rows = {have[0]: table.norm_diff_descriptor_best_match}
    elif isinstance(table, EvalTable):
        have = COLUMNS
        fields = CURVE_FIELDS if fields is None else tuple(fields)
        rows = None
    else:
        raise TypeError("table must be an EvalTable or an AcrossObjectTable, got %s" % type(table).__name__)
    unknown = [f for f in fields if f not in have]
    if unknown or not fields:
        raise ValueError("unknown field(s) %s: this table has %s" % (unknown, ", ".join(have)))
    if rows is None:
        values = torch.stack([table.columns[COLUMNS.index(f)] for f in fields])
        drops = [f in CURVE_DROP_NAN for f in fields]
    else:
        values = torch.stack([rows[f].double() for f in fields])
        drops = [False] * len(fields)
    if drop_nan is not None:
        drops = [bool(drop_nan)] * len(fields)
    return cumulative_frequencies(values, table.row_pair, num_bins, drops, out_summary, fields)


def _refused_range(mn, mx, num_bins):
    """numpy's message for the range scipy.stats.cumfreq derives from a minimum and a maximum that are not finite"""
    with np.errstate(all="ignore"):
        s = (np.float64(mx) - np.float64(mn)) / (2. * (num_bins - 1.))
        return "supplied range of [{}, {}] is not finite".format(np.float64(mn) - s, np.float64(mx) + s)


def curves_to_host(curves):
    """ONE copy to the host.  -> {field: {"x_axis": lowerlimit + binsize * arange(num_bins) (``make_cdf_plot``'s, before its
    cosmetic scale factor), "cdf", "cumcount", "count", "area_above_curve"}}.  Raises what the reference's call on that
    column would have raised: ValueError in numpy's words for a curve with a NaN (not dropped) or a value that is not finite,
    ZeroDivisionError for one without values."""
    C, nb = len(curves.fields), int(curves.num_bins)
    block = torch.cat([curves.cumcount.double().view(-1), curves.cdf.reshape(-1), curves.summary.reshape(-1)]).cpu().numpy()
    cumcount = block[:C * nb].reshape(C, nb).astype(np.int64)      # (counts below 2^53 are exact in float64)
    cdf = block[C * nb:2 * C * nb].reshape(C, nb)
    summary = block[2 * C * nb:].reshape(C, len(CURVE_SUMMARY))
    out = {}
    for k, field in enumerate(curves.fields):
        n, _, mn, mx, lowerlimit, binsize, area, flags = summary[k]
        flags = int(flags)
        if flags & CURVE_NAN:
            raise ValueError("%s: %s" % (field, _refused_range(np.nan, np.nan, nb)))
        if flags & CURVE_NONFINITE:
            raise ValueError("%s: %s" % (field, _refused_range(mn, mx, nb)))
        if flags & CURVE_EMPTY:
            raise ZeroDivisionError("%s: float division by zero (no value in this column)" % (field,))
        out[field] = {"x_axis": lowerlimit + binsize * np.arange(0, nb), "cdf": cdf[k].copy(), "cumcount": cumcount[k].copy(),
                      "count": int(n), "area_above_curve": float(area)}
    return out


def area_above_curve(table, field, num_bins=100):
    """``DenseCorrespondenceEvaluationPlotter.compute_area_above_curve(df, field, num_bins)`` (evaluation.py:2844-2863) on a
    device table: NaNs dropped whatever the field, as there.  One launch, one copy.  -> float."""
    return curves_to_host(evaluation_curves(table, (field,), num_bins, drop_nan=True))[field]["area_above_curve"]


def write_stats_yaml(table, output_dir):
    """What ``run_on_single_dataframe`` saves (evaluation.py:2953-2975): ``<output_dir>/stats.yaml`` with the one key
    ``norm_diff_3d_area_above_curve``.  -> the dict written."""
    import dense_correspondence_manipulation.utils.utils as utils
    d = {"norm_diff_3d_area_above_curve": float(area_above_curve(table, "norm_diff_pred_3d"))}
    os.makedirs(output_dir, exist_ok=True)
    utils.saveToYaml(d, os.path.join(output_dir, "stats.yaml"))
    return d
