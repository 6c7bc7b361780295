"""Shared checks of the evaluation curves (dcn_hip.evaluate.cumulative_frequencies and what is built on it; csrc/curve_kernels.hip),
taking a device: "cpu" drives the host-emulation build, "cuda" the gfx950 library.  Not a test module.

The oracle is ``scipy.stats.cumfreq`` with the reference's two lines on top of it (``cumhist *= 1.0 / len(data)`` and ``b *
np.sum(1 - cumhist)``, evaluation.py:2671-2672, :2858-2862).  The fixtures tests/golden/curves_ref_*.npz hold the cases' inputs,
what the reference's own ``make_cdf_plot`` and ``compute_area_above_curve`` gave for them, and the emulation build's outputs."""
import collections
import glob
import os

import numpy as np
import torch

from helpers import ROOT                     # (first: puts the package on sys.path)
from dcn_hip import evaluate  # noqa: E402

GOLDENS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "curves_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("curves_ref_"):-len(".npz")] for p in GOLDENS]
EMPTY, NAN, NONFINITE = 1, 2, 4
SUMMARY_BITS = ("n", "dropped", "mn", "mx", "lowerlimit", "binsize")       # compared bit for bit
EDGE_COUNTS = [4, 5, 3, 5, 7, 8, 10, 7, 4, 6]                              # the on_edges case: 50 values and the 9 interior edges in 10 bins


def area_bound(num_bins, oracle):
    """|area - oracle| <= 4 * num_bins * 2^-53 * |oracle|: the terms 1 - cdf[i] lie in [0, 1], so any order of summing
    num_bins of them is within (num_bins - 1) * 2^-53 of the exact sum relative to it, numpy's pairwise order and the kernel's
    both; twice that between the two, and the product with binsize adds one rounding each."""
    return 4.0 * num_bins * 2.0 ** -53 * abs(oracle)


def _case(values, num_bins=100, row_pair=None, drop_nan=False):
    values = np.atleast_2d(np.asarray(values, np.float64))
    C = values.shape[0]
    drops = [bool(drop_nan)] * C if isinstance(drop_nan, bool) else [bool(d) for d in drop_nan]
    return dict(values=values, num_bins=int(num_bins), row_pair=None if row_pair is None else np.asarray(row_pair, np.int32),
                drop_nan=drops)


def edges_of(x, num_bins):
    """numpy's bin edges for scipy's range of ``x``"""
    s = (x.max() - x.min()) / (2. * (num_bins - 1.))
    return np.histogram(x, bins=num_bins, range=(x.min() - s, x.max() + s))[1]


def build_cases():
    """name -> case, the smallest at which the kernel can go wrong (a workgroup has 1024 work-items with four rows each in
    flight: 5 000 rows are more than one trip of its loop)"""
    rng = np.random.RandomState(20)
    cases = collections.OrderedDict()
    for R in (1, 2, 63, 64, 65, 257, 5000):
        cases["r%d" % R] = _case(rng.rand(R) * 7.0)
    cases["bins2"] = _case(rng.rand(257) * 3.0 - 1.0, num_bins=2)
    cases["bins4096"] = _case(rng.randn(257), num_bins=4096)
    cases["all_equal"] = _case(np.full(65, 3.5))
    cases["single"] = _case([3.5])
    cases["two_values"] = _case([0.25, 11.0])
    cases["integers"] = _case(np.arange(100.0))
    x = np.random.RandomState(0).rand(50) * 7.0
    e = edges_of(x, 10)
    cases["on_edges"] = _case(np.concatenate([x, e[1:-1]]), num_bins=10)
    cases["mixed_magnitude"] = _case([-1e-3, 5e2, 7.0])
    # rows that do not belong: interleaved and at the end, carrying NaN, with drop_nan OFF (they must not flag the curve)
    R = 130
    v = rng.rand(R) * 40.0
    pair = np.repeat(np.arange(13), 10).astype(np.int32)
    out = np.zeros(R, bool)
    out[[0, 5, 6, 64, 77]] = True
    out[118:] = True
    v[out], pair[out] = np.nan, -1
    cases["row_pair"] = _case(v, row_pair=pair)
    v = rng.rand(257) * 2.0
    v[rng.rand(257) < 0.2] = np.nan
    cases["nan_dropped"] = _case(v, drop_nan=True)
    cases["nan_not_dropped"] = _case(v, drop_nan=False)
    v = rng.rand(65)
    v[17] = np.inf
    cases["inf"] = _case(v)
    cases["no_rows"] = _case(np.zeros((1, 0)))
    cases["all_nan_dropped"] = _case(np.full(65, np.nan), drop_nan=True)
    # nine curves in one launch, drop_nan per curve: flagged curves beside clean ones, some rows not in the table
    R = 257
    v = rng.rand(9, R) * np.array([1, 10, 0.1, 640, 5, 1, 1, 300, 2])[:, None]
    pair = np.arange(R, dtype=np.int32) // 20
    pair[[3, 100, 101, 256]] = -1
    v[:, pair < 0] = np.nan
    v[1, 50:60] = np.nan            # dropped
    v[2, 7] = np.nan                # not dropped: NAN
    v[4, 200] = -np.inf             # NONFINITE
    v[5, pair >= 0] = np.nan        # every value dropped: EMPTY
    v[6, 9] = np.nan                # dropped
    v[8, :] = np.where(pair >= 0, 2.0, np.nan)   # all equal
    cases["nine_curves"] = _case(v, row_pair=pair, drop_nan=[False, True, False, False, False, True, True, False, False])
    return cases


def oracle(case):
    """scipy on the host, curve by curve -> dict of arrays (flags, n, dropped, mn, mx, lowerlimit, binsize, area [C];
    cumcount, cdf [C, num_bins])"""
    import warnings
    import scipy.stats as ss
    nb, C = case["num_bins"], case["values"].shape[0]
    out = dict(flags=np.zeros(C, np.int64), n=np.zeros(C), dropped=np.zeros(C), cumcount=np.zeros((C, nb), np.int64),
               cdf=np.full((C, nb), np.nan))
    for key in ("mn", "mx", "lowerlimit", "binsize", "area"):
        out[key] = np.full(C, np.nan)
    for k in range(C):
        data = case["values"][k]
        if case["row_pair"] is not None:
            data = data[case["row_pair"] >= 0]
        if case["drop_nan"][k]:
            out["dropped"][k] = np.isnan(data).sum()
            data = data[~np.isnan(data)]
        out["n"][k] = (~np.isnan(data)).sum()
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                cumhist, l, b, _ = ss.cumfreq(data, nb)
            out["cumcount"][k] = cumhist.astype(np.int64)
            cumhist *= 1.0 / len(data)
            out["area"][k] = b * np.sum((1 - cumhist))
            out["cdf"][k], out["lowerlimit"][k], out["binsize"][k] = cumhist, l, b
            out["mn"][k], out["mx"][k] = data.min(), data.max()
        except ValueError as err:
            assert "is not finite" in str(err), err
            out["flags"][k] = NAN if np.isnan(data).any() else NONFINITE
            out["cumcount"][k] = 0
            if out["flags"][k] == NONFINITE:
                out["mn"][k], out["mx"][k] = data.min(), data.max()
        except ZeroDivisionError:
            out["flags"][k] = EMPTY
            out["cumcount"][k] = 0
    return out


def run(case, device, **kw):
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device)
    return evaluate.cumulative_frequencies(t(case["values"], torch.float64), t(case["row_pair"], torch.int32),
                                           case["num_bins"], case["drop_nan"], **kw)


def to_numpy(curves):
    s = curves.summary.cpu().numpy()
    out = dict(cumcount=curves.cumcount.cpu().numpy(), cdf=curves.cdf.cpu().numpy(), status=int(curves.status.cpu()[0]),
               flags=s[:, 7].astype(np.int64), area=s[:, 6].copy())
    for i, key in enumerate(SUMMARY_BITS):
        out[key] = s[:, i].copy()
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and (np.array_equal(a.view(np.int64), b.view(np.int64))
                                   or bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)))))


def check_against(got, want, num_bins, what):
    """``got``: to_numpy of a launch; ``want``: the oracle's dict (or a golden's)"""
    assert np.array_equal(got["flags"], want["flags"]), (what, got["flags"], want["flags"])
    assert got["status"] == int(np.bitwise_or.reduce(want["flags"])), (what, got["status"])
    assert np.array_equal(got["cumcount"], want["cumcount"]), what
    for key in SUMMARY_BITS + ("cdf",):
        assert same_bits(got[key], want[key]), (what, key, got[key], want[key])
    for k, flag in enumerate(want["flags"]):
        if flag:
            assert np.isnan(got["area"][k]), (what, k)
        else:
            err, bound = abs(got["area"][k] - want["area"][k]), area_bound(num_bins, want["area"][k])
            print("%s curve %d: area %.17g oracle %.17g |diff| %.3g bound %.3g" % (what, k, got["area"][k], want["area"][k],
                                                                                 err, bound))
            assert err <= bound, (what, k, got["area"][k], want["area"][k])
            assert got["cumcount"][k, -1] == want["n"][k], (what, k)        # the maximum itself: the last bin is closed


def check_case(name, case, device, want=None):
    want = oracle(case) if want is None else want
    first = to_numpy(run(case, device))
    check_against(first, want, case["num_bins"], name)
    again = to_numpy(run(case, device))
    for key in first:
        assert same_bits(np.asarray(first[key], np.float64), np.asarray(again[key], np.float64)), (name, key, "run to run")
    return first


def golden_case(z):
    rp = z["row_pair"]
    return dict(values=z["values"], num_bins=int(z["num_bins"]), row_pair=rp if int(z["has_row_pair"]) else None,
                drop_nan=[bool(d) for d in z["drop_nan"]])


def golden_want(z, prefix):
    return {k: z[prefix + k] for k in ("flags", "cumcount", "cdf", "area") + SUMMARY_BITS}


def check_golden(z, device):
    """the launch against what the reference's own functions gave, and against the emulation build's stored outputs"""
    case, nb = golden_case(z), int(z["num_bins"])
    got = check_case("golden", case, device, golden_want(z, "ref_"))
    emu = golden_want(z, "emu_")
    assert np.array_equal(got["cumcount"], emu["cumcount"]) and np.array_equal(got["flags"], emu["flags"])
    for key in SUMMARY_BITS + ("cdf", "area"):                            # the same text compiled twice: the area too
        assert same_bits(got[key], emu[key]), key
    # curves_to_host's x axis is make_cdf_plot's
    if not np.any(z["ref_flags"]):
        host = evaluate.curves_to_host(run(case, device))
        for k in range(case["values"].shape[0]):
            assert same_bits(host[k]["x_axis"], z["ref_x_axis"][k]) and same_bits(host[k]["cdf"], z["ref_cdf"][k])
            assert host[k]["count"] == int(z["ref_n"][k]) and np.array_equal(host[k]["cumcount"], z["ref_cumcount"][k])
    return got


def check_host_rules(device):
    """the argument checks, pinned"""
    import pytest
    v = torch.zeros((1, 8), dtype=torch.float64, device=device)
    for nb in (1, 4097):
        with pytest.raises(ValueError, match="num_bins"):
            evaluate.cumulative_frequencies(v, num_bins=nb)
    for C in (0, 65):
        with pytest.raises(ValueError, match="curves per call"):
            evaluate.cumulative_frequencies(torch.zeros((C, 8), dtype=torch.float64, device=device))
    with pytest.raises(TypeError, match="float64"):
        evaluate.cumulative_frequencies(v.float())
    with pytest.raises(ValueError, match="row_pair"):
        evaluate.cumulative_frequencies(v, row_pair=torch.zeros(7, dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match="drop_nan"):
        evaluate.cumulative_frequencies(v, drop_nan=[True, False])
    with pytest.raises(ValueError, match="out_summary"):
        evaluate.cumulative_frequencies(v, out_summary=torch.zeros((1, 8), dtype=torch.float32, device=device))
    # the limits themselves are legal
    c = evaluate.cumulative_frequencies(torch.arange(64.0 * 8, dtype=torch.float64, device=device).view(64, 8), num_bins=4096)
    assert int(c.status.cpu()[0]) == 0 and tuple(c.cdf.shape) == (64, 4096)
    assert int(evaluate.cumulative_frequencies(v, num_bins=2).cumcount.cpu()[0, -1]) == 8


def check_raw_entry_rejects(lib, device):
    """the C entry's own checks: DCN_E_INVALID, nothing launched"""
    import ctypes
    v = torch.zeros((1, 8), dtype=torch.float64, device=device)
    drop = torch.zeros(64, dtype=torch.uint8, device=device)
    cc = torch.zeros((1, 4096), dtype=torch.int64, device=device)
    cd = torch.zeros((1, 4096), dtype=torch.float64, device=device)
    s = torch.zeros((1, 8), dtype=torch.float64, device=device)
    st = torch.zeros(1, dtype=torch.int32, device=device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda c, rows, ld, nb: lib.get().dcn_eval_curves(c, rows, ld, p(v), None, p(drop), nb, p(cc), p(cd), p(s), p(st),
                                                             lib.stream_ptr())
    for args in ((0, 8, 8, 100), (65, 8, 8, 100), (1, 8, 8, 1), (1, 8, 8, 4097), (1, -1, 8, 100), (1, 8, 7, 100)):
        assert call(*args) == -1, args
    assert call(1, 8, 8, 100) == 0


def scipy_check_table(curves, columns, row_pair, drops, num_bins=100):
    """``curves`` (EvalCurves of a device table) against scipy on the table copied to the host, field by field: counts exact,
    area within the bound, count + dropped == rows in the table.  ``columns``: {field: numpy column}"""
    got = to_numpy(curves)
    rows = int((row_pair >= 0).sum())
    for k, field in enumerate(curves.fields):
        case = _case(np.asarray(columns[field], np.float64), num_bins, row_pair, bool(drops[k]))
        want = oracle(case)
        one = {key: (val[k:k + 1] if isinstance(val, np.ndarray) else int(want["flags"][0])) for key, val in got.items()}
        check_against(one, want, num_bins, field)
        if not case["drop_nan"][0] and want["flags"][0] == NAN:
            continue
        assert got["n"][k] + got["dropped"][k] == rows, (field, got["n"][k], got["dropped"][k], rows)
    return got


def check_curves_to_host_errors(cases, device):
    import pytest
    with pytest.raises(ValueError, match=r"supplied range of \[nan, nan\] is not finite"):
        evaluate.curves_to_host(run(cases["nan_not_dropped"], device))
    with pytest.raises(ValueError, match=r"supplied range of \[-inf, inf\] is not finite"):
        evaluate.curves_to_host(run(cases["inf"], device))
    for name in ("no_rows", "all_nan_dropped"):
        with pytest.raises(ZeroDivisionError):
            evaluate.curves_to_host(run(cases[name], device))
    with pytest.raises(ValueError, match="is not finite"):                  # a flagged curve beside clean ones
        evaluate.curves_to_host(run(cases["nine_curves"], device))
    host = evaluate.curves_to_host(run(cases["integers"], device))[0]
    assert host["count"] == 100 and host["x_axis"].tolist() == [k - 0.5 for k in range(100)]
    assert host["cumcount"].tolist() == list(range(1, 101)) and set(host) == {"x_axis", "cdf", "cumcount", "count",
                                                                               "area_above_curve"}


def check_table(t, device, fields, drops, columns, tmp_path=None):
    """evaluation_curves / area_above_curve / write_stats_yaml of a device table against scipy on its copy"""
    import pytest
    import yaml
    row_pair = t.row_pair.cpu().numpy()
    curves = evaluate.evaluation_curves(t)
    assert curves.fields == tuple(fields) and curves.num_bins == 100
    got = scipy_check_table(curves, columns, row_pair, drops)
    with pytest.raises(ValueError, match="unknown field"):
        evaluate.evaluation_curves(t, ("no_such_column",))
    clean = [f for k, f in enumerate(fields) if got["flags"][k] == 0]
    assert clean, got["flags"]
    host = evaluate.curves_to_host(evaluate.evaluation_curves(t, clean))
    for f in clean:
        k = fields.index(f)
        assert host[f]["count"] == got["n"][k] and same_bits(host[f]["area_above_curve"], got["area"][k])
        assert same_bits(host[f]["cdf"], got["cdf"][k]) and np.array_equal(host[f]["cumcount"], got["cumcount"][k])
        # compute_area_above_curve drops NaNs whatever the field
        want = oracle(_case(np.asarray(columns[f], np.float64), 100, row_pair, True))
        a = evaluate.area_above_curve(t, f)
        assert isinstance(a, float) and abs(a - want["area"][0]) <= area_bound(100, want["area"][0]), (f, a, want["area"][0])
    if tmp_path is not None:
        d = evaluate.write_stats_yaml(t, str(tmp_path))
        with open(str(tmp_path / "stats.yaml")) as f:
            assert yaml.safe_load(f) == d
        assert list(d) == ["norm_diff_3d_area_above_curve"]
        assert d["norm_diff_3d_area_above_curve"] == evaluate.area_above_curve(t, "norm_diff_pred_3d")
    return got


def _eval_table_columns(t):
    cols = t.columns.cpu().numpy()
    return {f: cols[evaluate.COLUMNS.index(f)] for f in evaluate.CURVE_FIELDS}


def check_same_scene_table(device, h, w, make_dcn, tmp_path):
    import evaluate_common as ec
    store = ec.synthetic_store(device, h, w)
    dcn = make_dcn(h, w)
    dcn.train()
    chosen = evaluate.choose_pairs(store, 10, np.random.RandomState(0))
    t = evaluate.evaluate_frame_pairs(dcn, store, chosen, 100, generator=torch.Generator(device).manual_seed(0))
    assert dcn.training and int(t.status.cpu()[0]) == 0
    rows = int((t.row_pair >= 0).sum())
    assert 0 < rows < int(t.row_pair.numel())                                # rows past the end, marked -1
    drops = [f in evaluate.CURVE_DROP_NAN for f in evaluate.CURVE_FIELDS]
    assert sum(drops) == 2 and len(evaluate.CURVE_FIELDS) == 9
    check_table(t, device, evaluate.CURVE_FIELDS, drops, _eval_table_columns(t), tmp_path)


def check_across_object_table(device, h, w):
    import acrossobj_common as ac
    store = ac.three_object_store(device, h, w)
    chosen = evaluate.choose_object_pairs(store, 6, np.random.RandomState(3))
    net = ac.StubNetwork().to(device)
    t = evaluate.evaluate_object_pairs(net, store, chosen, 50, generator=torch.Generator(device).manual_seed(3), batch_pairs=2)
    assert int(t.status.cpu()[0]) == 0 and t.norm_diff_descriptor_best_match.dtype == torch.float32
    field = "norm_diff_descriptor_best_match"
    columns = {field: t.norm_diff_descriptor_best_match.cpu().numpy().astype(np.float64)}
    got = check_table(t, device, (field,), [False], columns)
    assert got["n"][0] == int((t.row_pair >= 0).sum()) > 0 and got["flags"][0] == 0


def check_cross_scene_table(device):
    """a cross-scene table (the 48 x 64 golden's scenes, labels and views): rows without a result in the middle of the table"""
    import crossscene_common as cc
    z = np.load([p for p in cc.GOLDENS if p.endswith("48x64_d3.npz")][0])
    store, net = cc.golden_store(z, device)
    labels = evaluate.cross_scene_labels(store, cc.golden_annotations(z))
    t = evaluate.evaluate_cross_scene_rows(net, store, labels, cc.golden_views(z))
    rp = t.row_pair.cpu().numpy()
    has = np.nonzero(rp >= 0)[0]
    assert int(t.status.cpu()[0]) == 0 and 0 < len(has) < len(rp) and (rp[:has[-1]] < 0).any()   # interior rows left out
    drops = [f in evaluate.CURVE_DROP_NAN for f in evaluate.CURVE_FIELDS]
    check_table(t, device, evaluate.CURVE_FIELDS, drops, _eval_table_columns(t))
