#!/usr/bin/env python3
"""Times the qualitative evaluation's arithmetic (csrc/picture_kernels.hip, dcn_hip/evaluate/pictures.py) at 640 x 480 on one
MI355X:

  1. ``evaluate.descriptor_pictures`` for P = 8 pairs, D = 3 (the four pictures of plot_descriptor_colormaps per pair);
  2. ``evaluate.heat_maps`` for 8 pairs x 100 rows, D = 3 and D = 16, as a plane and through a colour table;

each against (a) the reference's formulation in the same process on the same tensors -- the ``.cpu()`` copy plus the numpy
text (tests/pictures_common.py states it; for the heat maps ONE pair of 100 rows is run and the figure is scaled by 8: the
full 800 rows take tens of seconds) -- and (b) a device formulation in torch ops.  The variants are interleaved: window k of
every variant runs before window k + 1 of any.  Call times are device events around back-to-back calls, medians of
``--repeats`` windows with their spread; kernel times come from the profiler's kernel records in a pass of their own.  The
ranges and normalise kernels' read rates and the heat kernel's store rate are given as a share of the 6.3 TB/s achievable
HBM rate, from byte counts computed here from the shapes.

    python tools/pictures_bench.py [--repeats 5] [--out profiles/pictures_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools"),
           os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch  # noqa: E402

import pictures_common as pc  # noqa: E402
from augment_bench import ACHIEVABLE, PEAK  # noqa: E402
from frames_bench import event_us, kernel_us  # noqa: E402

H, W, P, ROWS = 480, 640, 8, 100


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(variants, repeats):
    """{name: (fn, kind)} with kind "events" (device events over 10 back-to-back calls, microseconds -> ms) or "wall" -> {name:
    {"median_ms", "all_ms"}}; window k of every variant before window k + 1 of any"""
    for fn, _ in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, (fn, kind) in variants.items():
            times[k].append(event_us(fn, 10) * 1e-3 if kind == "events" else wall_ms(fn))
    return {k: {"median_ms": round(float(np.median(t)), 4), "all_ms": [round(x, 4) for x in t]} for k, t in times.items()}


def torch_pictures(ra, rb, ma, mb):
    """The pair and masked-pair pictures in torch ops on the device (masks 0 / 1; a zero under the mask counts, unlike the
    reference -- a formulation to time, not to pin)"""
    out = []
    lo = torch.minimum(ra.amin((1, 2)), rb.amin((1, 2)))[:, None, None]
    hi = torch.maximum(ra.amax((1, 2)), rb.amax((1, 2)))[:, None, None]
    inf = float("inf")
    on_a, on_b = ma[..., None] != 0, mb[..., None] != 0
    mlo = torch.minimum(torch.where(on_a, ra, inf).amin((1, 2)), torch.where(on_b, rb, inf).amin((1, 2)))[:, None, None]
    mhi = torch.maximum(torch.where(on_a, ra, -inf).amax((1, 2)), torch.where(on_b, rb, -inf).amax((1, 2)))[:, None, None]
    for x, on in ((ra, on_a), (rb, on_b)):
        out.append((255 * ((x - lo) / (hi - lo)).clamp(0, 1)).to(torch.uint8))
        out.append((255 * (((x - mlo) / (mhi - mlo)) * on).clamp(0, 1)).to(torch.uint8))
    return torch.stack([torch.stack([out[0], out[2]], 1), torch.stack([out[1], out[3]], 1)], 1)


def numpy_pictures(ra, rb, ma, mb):
    """The reference's formulation: the copy to the host, then the numpy text"""
    a, b, m1, m2 = (t.cpu().numpy() for t in (ra, rb, ma, mb))
    _, pair, _, _ = pc.np_ranges(a, b, m1, m2)
    ch = (0, 1, 2)
    return [pc.np_picture(x, ch) for x in (pc.np_pair(a, pair), pc.np_pair(b, pair), pc.np_masked(a, m1, pair),
                                            pc.np_masked(b, m2, pair))]


def torch_heat(res_b, queries, variance, table):
    out = []
    for p in range(res_b.shape[0]):
        q = queries[p * ROWS:(p + 1) * ROWS]
        nd = (res_b[p][None] - q[:, None, None, :]).square().sum(-1).sqrt()
        plane = (torch.exp(-nd / variance) * 255).to(torch.uint8)
        out.append(plane if table is None else table[plane.long()])
    return torch.cat(out)


def numpy_heat_one_pair(res_b, queries, variance, table):
    r, q = res_b[0].cpu().numpy(), queries[:ROWS].cpu().numpy()
    out = []
    for d in q:
        plane = pc.np_heat_reference(np.sqrt(np.sum(np.square(r - d), axis=2)), variance)
        out.append(plane if table is None else table[plane])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib, evaluate as ev
    _lib.load()
    dev = torch.device("cuda", 0)
    res = {"machine": torch.cuda.get_device_name(0), "library": _lib.library_info()["version"], "repeats": a.repeats,
           "achievable_bps": ACHIEVABLE, "peak_bps": PEAK, "shape": "%dx%d, %d pairs" % (W, H, P)}
    g = torch.Generator(device=dev).manual_seed(0)
    ys, xs = torch.arange(H, device=dev).view(H, 1), torch.arange(W, device=dev).view(1, W)
    mask = torch.stack([torch.stack([((xs - 300 - 5 * i - 20 * s) ** 2 + (ys - 240) ** 2 < (120 + 4 * i) ** 2) for i in range(P)])
                        for s in range(2)]).to(torch.uint8)
    # ---- 1. descriptor_pictures, D = 3
    D = 3
    ra, rb = (torch.randn((P, H, W, D), device=dev, generator=g) for _ in range(2))
    ours = lambda: ev.descriptor_pictures(ra, rb, mask[0], mask[1])
    got = ours().pictures
    want = numpy_pictures(ra, rb, mask[0], mask[1])
    equal = all(np.array_equal(got[:, i, s].cpu().numpy(), want[2 * i + s]) for i in range(2) for s in range(2))
    timing = interleaved({"descriptor_pictures": (ours, "events"),
                          "torch_ops_on_device": (lambda: torch_pictures(ra, rb, mask[0], mask[1]), "events"),
                          "cpu_copy_and_numpy": (lambda: numpy_pictures(ra, rb, mask[0], mask[1]), "wall")}, a.repeats)
    read = 2 * P * H * W * (4 * D + 1)
    written = 4 * P * H * W * 3
    k = {n: kernel_us(ours, n) for n in ("range_partial_kernel", "range_finish_kernel", "norm_kernel")}
    res["descriptor_pictures"] = {
        "D": D, "equal_numpy_statement": bool(equal), "timing": timing, "kernel_us": {n: round(v, 2) for n, v in k.items()},
        "model_bytes_read_per_launch": read, "model_bytes_written_normalise": written,
        "range_partial_read_fraction_of_achievable": round(read / (k["range_partial_kernel"] * 1e-6) / ACHIEVABLE, 4),
        "norm_kernel_read_fraction_of_achievable": round(read / (k["norm_kernel"] * 1e-6) / ACHIEVABLE, 4),
        "norm_kernel_read_plus_write_fraction_of_achievable": round((read + written) / (k["norm_kernel"] * 1e-6) / ACHIEVABLE, 4)}
    del ra, rb
    # ---- 2. heat_maps, 8 pairs x 100 rows
    table = ev.colour_table().to(dev)
    table_host = ev.colour_table().numpy()
    offsets = torch.arange(0, (P + 1) * ROWS, ROWS, device=dev, dtype=torch.int64)
    res["heat_maps"] = []
    for D in (3, 16):
        res_b = torch.randn((P, H, W, D), device=dev, generator=g) * (0.35 / np.sqrt(D))
        pick = torch.randint(0, H * W, (P * ROWS,), device=dev, generator=g)
        queries = torch.stack([res_b[r // ROWS].view(-1, D)[pick[r]] for r in range(P * ROWS)]).contiguous()
        for name, t, t_host in (("plane", None, None), ("coloured", table, table_host)):
            ours = lambda: ev.heat_maps(res_b, queries, offsets, 0.25, t)
            got = ours().maps
            base = torch_heat(res_b, queries, 0.25, t)
            differing = int((got != base).sum())
            largest = int((got.int() - base.int()).abs().max())
            del base
            timing = interleaved({"heat_maps": (ours, "events"),
                                  "torch_ops_on_device": (lambda: torch_heat(res_b, queries, 0.25, t), "events"),
                                  "cpu_copy_and_numpy_one_pair": (lambda: numpy_heat_one_pair(res_b, queries, 0.25, t_host),
                                                                  "wall")}, a.repeats)
            timing["cpu_copy_and_numpy_scaled_to_%d_pairs_ms" % P] = round(
                timing["cpu_copy_and_numpy_one_pair"]["median_ms"] * P, 2)
            stored = P * ROWS * H * W * (3 if t is not None else 1)
            us = kernel_us(ours, "heat_kernel", reps=5)
            res["heat_maps"].append({
                "D": D, "output": name, "rows": P * ROWS, "timing": timing, "heat_kernel_us": round(us, 2),
                "model_bytes_read": P * H * W * D * 4, "model_bytes_stored": stored,
                "bytes_differing_from_torch_ops": differing, "largest_difference_levels": largest,
                "store_GB_per_s": round(stored / (us * 1e-6) / 1e9, 1),
                "store_fraction_of_achievable": round(stored / (us * 1e-6) / ACHIEVABLE, 4)})
            del got
        del res_b, queries
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
