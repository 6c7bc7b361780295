#!/usr/bin/env python3
"""Times the across-object search (csrc/acrossobj_kernels.hip, dcn_hip/evaluate/across_objects.py) for 25 pairs x 100 queries of 640 x 480
descriptor images at D = 3 and D = 16, on random masks and descriptors:

  1. the whole call: ``evaluate.across_object_queries`` + ``evaluate.best_match_pairs`` (device time between two events);
  2. the search launch alone (device time of ``pair_search_kernel`` from the profiler's kernel records), against its traffic
     model P * HW * D * 4 bytes of res_b read once, at the 6.3 TB/s achievable HBM bandwidth;
  3. the baseline: the same queries through the public piece that existed before, ``match.find_best_matches`` called pair by
     pair on the same tensors, in the same process.

The two paths' results are compared first (equal pixels, distances equal bit for bit).  Warm-up runs first; every figure is
the median of ``--repeats`` timed windows of ``--iters`` calls; the machine is named in the output.

    python tools/acrossobj_bench.py [--repeats 5] [--iters 20] [--out profiles/acrossobj_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch  # noqa: E402

from augment_bench import ACHIEVABLE, PEAK  # noqa: E402
from frames_bench import event_us, kernel_us  # noqa: E402

H, W, P, Q = 480, 640, 25, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dims", type=int, nargs="+", default=[3, 16])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib, evaluate, match
    _lib.load()
    dev = torch.device("cuda", 0)
    res = {"machine": torch.cuda.get_device_name(0), "library": _lib.library_info()["version"],
           "shape": "%d pairs x %d queries, %dx%d" % (P, Q, W, H), "repeats": a.repeats, "iters": a.iters,
           "achievable_bps": ACHIEVABLE, "peak_bps": PEAK, "runs": []}
    for D in a.dims:
        g = torch.Generator(device=dev).manual_seed(D)
        mask = (torch.rand((P, H, W), device=dev, generator=g) < 0.3).to(torch.uint8)
        res_a = torch.randn((P, H, W, D), device=dev, generator=g)
        res_b = torch.randn((P, H, W, D), device=dev, generator=g)
        seeds = torch.arange(P, device=dev)
        q = evaluate.across_object_queries(mask, res_a, Q, order_seeds=seeds)

        def whole():
            x = evaluate.across_object_queries(mask, res_a, Q, order_seeds=seeds)
            return evaluate.best_match_pairs(res_b, x.queries, x.offsets, max_pair_rows=Q)

        def search():
            return evaluate.best_match_pairs(res_b, q.queries, q.offsets, max_pair_rows=Q)

        def base():
            return [match.find_best_matches(res_b[p], q.queries[p * Q:(p + 1) * Q]) for p in range(P)]
        m, ref = whole(), base()
        assert int(q.status.cpu()[0]) == 0 and int(m.status.cpu()[0]) == 0
        idx = torch.cat([r[0] for r in ref])
        dist = torch.cat([r[1] for r in ref])
        same_pixels = bool(torch.equal(m.best_uv[1].long() * W + m.best_uv[0].long(), idx))
        same_bits = bool(torch.equal(m.norm_diff_descriptor_best_match.view(torch.int32), dist.view(torch.int32)))
        t = {k: [] for k in ("whole", "search", "base")}
        for _ in range(a.repeats):                             # the three alternate inside every repeat
            for k, fn in (("whole", whole), ("search", search), ("base", base)):
                t[k].append(event_us(fn, a.iters))
        us_kernel = kernel_us(search, "pair_search_kernel", reps=max(5, a.iters))
        us_pick = kernel_us(whole, "across_pick_kernel", reps=max(5, a.iters))
        nbytes = P * H * W * D * 4
        med = {k: float(np.median(v)) for k, v in t.items()}
        res["runs"].append({
            "D": D, "same_pixels_as_baseline": same_pixels, "same_distance_bits_as_baseline": same_bits,
            "whole_call_us": round(med["whole"], 1), "whole_call_us_all": [round(x, 1) for x in t["whole"]],
            "search_call_us": round(med["search"], 1), "search_call_us_all": [round(x, 1) for x in t["search"]],
            "pair_search_kernel_us": round(us_kernel, 2), "across_pick_kernel_us": round(us_pick, 2),
            "pair_search_model_bytes": nbytes, "pair_search_GB_per_s": round(nbytes / (us_kernel * 1e-6) / 1e9, 1),
            "pair_search_fraction_of_achievable": round(nbytes / (us_kernel * 1e-6) / ACHIEVABLE, 4),
            "pair_search_GFLOP_per_s": round(3.0 * P * Q * H * W * D / (us_kernel * 1e-6) / 1e9, 1),
            "baseline_per_pair_find_best_matches_us": round(med["base"], 1),
            "baseline_us_all": [round(x, 1) for x in t["base"]],
            "search_speedup_vs_baseline": round(med["base"] / med["search"], 2)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
