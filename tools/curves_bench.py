#!/usr/bin/env python3
"""Times the evaluation curves on the device (csrc/curve_kernels.hip, dcn_hip.evaluate.evaluation_curves) and validation while
training (dcn_hip.train.Validation).

Part ``curves``: the nine curves of a same-scene table of 2 500 and of 250 000 rows (the reference's 25 pairs x 100 matches,
and a hundred times that; 2 % of the 3D columns NaN, 1 % of the rows past the end) by ``evaluation_curves`` -- no read-back --
against what there was before for the same numbers: the table's ``.cpu()`` copy, ``scipy.stats.cumfreq`` per field and the
reference's two lines, the synchronisation included because it is the point.  The two interleaved window by window.

Part ``trainer``: a ``StoreTrainer`` iteration with ``validation`` configured, on iterations WITHOUT a validation pass, against
the iteration of a trainer without the option (the code of the commit before: the option adds nothing to an iteration), on the
same draws, B = 1 and 4 as in profiles/train_bench.json, interleaved window by window.  Accepted when the difference of the
medians lies within the max - min spread of the plain trainer's own windows.

Part ``pass``: one validation pass, 25 pairs x 100 matches at 640 x 480 with Resnet34_8s, nine fields, 100 bins.

Device events around windows of back-to-back calls and the wall clock around the same windows (ending in a synchronize); 5
windows each, medians and max - min spreads.  Each part runs in a fresh child process.

    python tools/curves_bench.py [--out profiles/curves_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from train_bench import CFG, H, W, D, WINDOWS, build_dcn, summary, window          # noqa: E402

CURVE_CALLS, HOST_CALLS, TRAIN_CALLS, PASS_CALLS = 50, 5, 5, 2


def synthetic_table(rows, device, seed=0):
    """An EvalTable with the columns' magnitudes (pixels, metres, descriptor norms, fractions), NaNs and rows past the end"""
    import torch
    from dcn_hip import evaluate
    rng = np.random.RandomState(seed)
    R = rows + rows // 100
    scale = {"pixel_match_error_l2": 80.0, "pixel_match_error_l2_masked": 40.0, "pixel_match_error_l1": 100.0,
             "norm_diff_pred_3d": 0.1, "norm_diff_pred_3d_masked": 0.05, "norm_diff_ground_truth_3d": 0.01}
    cols = np.stack([np.abs(rng.randn(R)) * scale.get(f, 1.0) for f in evaluate.COLUMNS])
    for f in ("norm_diff_pred_3d", "norm_diff_pred_3d_masked"):
        cols[evaluate.COLUMNS.index(f), rng.rand(R) < 0.02] = np.nan
    pair = (np.arange(R) // 100).astype(np.int32)
    cols[:, rows:], pair[rows:] = np.nan, -1
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    z = torch.zeros(1, dtype=torch.int32, device=device)
    return evaluate.EvalTable(c(cols), None, None, None, c(pair), None, None, z, None, None, None, None)


def host_curves(t):
    """The numbers of evaluation_curves the way there was before: one copy of the table, scipy per field"""
    import scipy.stats as ss
    import torch
    from dcn_hip import evaluate
    R = int(t.row_pair.numel())
    block = torch.cat([t.columns, t.row_pair.double().view(1, R)]).cpu().numpy()
    keep = block[-1] >= 0
    out = {}
    for f in evaluate.CURVE_FIELDS:
        data = block[evaluate.COLUMNS.index(f)][keep]
        if f in evaluate.CURVE_DROP_NAN:
            data = data[~np.isnan(data)]
        cumhist, l, b, _ = ss.cumfreq(data, 100)
        cumhist *= 1.0 / len(data)
        out[f] = (cumhist, l, b, b * np.sum(1 - cumhist))
    return out


def part_curves():
    import torch
    from dcn_hip import evaluate
    runs = []
    for rows in (2500, 250000):
        t = synthetic_table(rows, "cuda")
        device = lambda: evaluate.evaluation_curves(t)
        host = lambda: host_curves(t)
        # the same numbers first
        got, want = evaluate.curves_to_host(device()), host()
        worst = max(abs(got[f]["area_above_curve"] - want[f][3]) / want[f][3] for f in evaluate.CURVE_FIELDS)
        assert all(np.array_equal(got[f]["cdf"], want[f][0]) for f in evaluate.CURVE_FIELDS) and worst < 4 * 100 * 2.0 ** -53
        for _ in range(5):
            device(), host()
        samples = {"evaluation_curves": [], "cpu_copy_and_scipy": []}
        for _ in range(WINDOWS):
            samples["evaluation_curves"].append(window(device, CURVE_CALLS))
            samples["cpu_copy_and_scipy"].append(window(host, HOST_CALLS))
        res = {"rows": rows, "fields": len(evaluate.CURVE_FIELDS), "num_bins": 100, "cdf_bits_equal": True,
               "area_worst_relative_difference": float(worst)}
        for k, v in samples.items():
            res[k] = summary(v)
        res["wall_ratio_host_over_device"] = round(res["cpu_copy_and_scipy"]["wall_us"] / res["evaluation_curves"]["wall_us"], 1)
        # what the kernel has to read: two passes over the nine columns and the row selector
        R = int(t.row_pair.numel())
        res["bytes_read"] = 2 * 9 * R * (8 + 4)
        runs.append(res)
    return {"shape": "same-scene table, 9 fields, 100 bins; medians of %d windows of %d (device) / %d (host) calls, interleaved"
                     % (WINDOWS, CURVE_CALLS, HOST_CALLS), "runs": runs}


def _pcl():
    from bench import LOSS_CONFIG
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    return PixelwiseContrastiveLoss(image_shape=[H, W], config=LOSS_CONFIG)


def _validation(store, rate):
    import torch
    from dcn_hip.train import Validation
    return Validation(store, rate, generator=torch.Generator(device=store.device).manual_seed(5),
                      host_rng=np.random.RandomState(5))


def part_trainer():
    import torch
    from dcn_hip.train import StoreTrainer
    from synthetic_bench import make_store
    store = make_store(torch.device("cuda", 0))
    runs = []
    for B in (1, 4):
        def make(validation):
            tr = StoreTrainer(build_dcn(), _pcl(), store, CFG, generator=torch.Generator(device=store.device).manual_seed(3),
                              host_rng=np.random.RandomState(3), batch_size=B, validation=validation)
            it = [0]

            def step():
                it[0] += 1
                tr.iteration(it[0])
                if tr.validation is not None and tr.validation.due(it[0]):
                    tr.validate(it[0])
            return tr, step
        plain, with_v = make(None), make(_validation(store, 10 ** 9))          # (rate: no pass in the timed iterations)
        for _, fn in (plain, with_v):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {"plain": [], "validation_configured": []}
        for _ in range(WINDOWS):
            samples["plain"].append(window(plain[1], TRAIN_CALLS))
            samples["validation_configured"].append(window(with_v[1], TRAIN_CALLS))
        res = {"B": B, "iterations_timed_per_loop": WINDOWS * TRAIN_CALLS, "validation_passes": with_v[0].validation.rows}
        for k, v in samples.items():
            res[k] = summary(v)
        for clock in ("device", "wall"):
            diff = res["validation_configured"][clock + "_us"] - res["plain"][clock + "_us"]
            res["difference_%s_us" % clock] = round(diff, 1)
            res["accepted_%s" % clock] = bool(abs(diff) <= res["plain"][clock + "_spread_us"])
        runs.append(res)
        del plain, with_v
        torch.cuda.empty_cache()
    return {"shape": "%dx%d, Resnet34_8s, D = %d, the store and data types of train_bench; medians of %d windows of %d "
                     "iterations, the two trainers interleaved" % (W, H, D, WINDOWS, TRAIN_CALLS), "runs": runs}


def part_pass():
    import torch
    from dcn_hip.train import StoreTrainer
    from synthetic_bench import make_store
    store = make_store(torch.device("cuda", 0))
    val = _validation(store, 1)
    tr = StoreTrainer(build_dcn(), _pcl(), store, CFG, generator=torch.Generator(device=store.device).manual_seed(3),
                      host_rng=np.random.RandomState(3), batch_size=1, validation=val)
    tr.dcn.train()
    tr.iteration(1)
    it = [1]

    def one():
        it[0] += 1
        tr.validate(it[0])
    for _ in range(2):
        one()
    samples = [window(one, PASS_CALLS) for _ in range(WINDOWS)]
    tr.read_log()
    rows = tr.validation_history
    res = summary(samples)
    res.update(shape="%d pairs x %d matches at %dx%d, Resnet34_8s, %d fields, %d bins; medians of %d windows of %d passes"
               % (val.num_image_pairs, val.num_matches, W, H, len(val.fields), val.num_bins, WINDOWS, PASS_CALLS),
               rows_per_pass=float(np.median(rows[:, 4])), passes=int(val.rows))
    return res


PARTS = {"curves": part_curves, "trainer": part_trainer, "pass": part_pass}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=("all",) + tuple(PARTS), default="all")
    a = ap.parse_args()
    if a.part == "all":      # each part in a fresh child process of its own
        res = {}
        for part in PARTS:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part], stdout=subprocess.PIPE, check=True)
            res[part] = json.loads(out.stdout.decode().strip().split("\n")[-1])
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("curves_bench: no GPU (a time measured anywhere else says nothing about the MI355X)")
        from dcn_hip import _lib
        _lib.load()
        res = PARTS[a.part]()
        res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
