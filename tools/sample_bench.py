#!/usr/bin/env python3
"""Times the device sample builder (csrc/sample_kernels.hip) at B = 4 pairs of 640 x 480 with training.yaml counts
(10 000 matching attempts, 75 masked + 75 background non-matches per match, masks and blind set on), on synthetic depth
surfaces like bench.py's pairgen scene: the whole within-scene build (dcn_within_scene_samples, drawn seeds, no images) with
device events around back-to-back builds, and the writer launch alone (device time of ``write_kernel`` from the profiler's
kernel records).  The writer's bytes are its two int64 outputs over the whole capacity (16 B per entry, the -1 tail
included) plus the reads of its useful entries (8 B each: the list / match it draws from); reported against the 6.3 TB/s
achievable HBM bandwidth.  For comparison it times the per-pair mirror path (correspondence_finder.py's device functions:
find, two non-match draws, the blind set, host concatenation into PairLists).

    python tools/sample_bench.py [--iters 50] [--out profiles/sample_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch  # noqa: E402

from augment_bench import ACHIEVABLE, PEAK  # noqa: E402

B, H, W, A, K1, K2 = 4, 480, 640, 10000, 75, 75


def scene(dev):
    rng = np.random.RandomState(0)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    depth, masks = np.zeros((2, B, H, W), np.uint16), np.zeros((2, B, H, W), np.uint8)
    for k in range(2):
        for p in range(B):
            d = 900 + 150 * np.sin(xs / (60 + 40 * rng.rand())) + 120 * np.cos(ys / (50 + 30 * rng.rand())) + 40 * rng.rand()
            d[rng.rand(H, W) < 0.02] = 0
            depth[k, p] = d.astype(np.uint16)
            masks[k, p, 120:360, 100 + 20 * p:380 + 20 * k] = 1
    pa = np.stack([np.eye(4)] * B)
    pb = []
    for p in range(B):
        ry = 0.01 * p
        T = np.eye(4)
        T[:3, :3] = [[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]]
        T[:3, 3] = [0.02, -0.01, 0.01]
        pb.append(T)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return c(depth[0].view(np.int16)), c(depth[1].view(np.int16)), c(masks[0]), c(masks[1]), pa, np.stack(pb)


def mirror_batch(d0, d1, m0, m1, pa, pb):
    """The per-pair path through the product-root mirror functions, then host concatenation."""
    from dcn_hip.loss import PairLists
    from dense_correspondence.correspondence_tools import correspondence_finder as cf
    tuples = []
    for p in range(B):
        uv_a, uv_b = cf.batch_find_pixel_correspondences(d0[p], pa[p], d1[p], pb[p], num_attempts=A, img_a_mask=m0[p].float())
        mb = m1[p].float()
        nm = cf.create_non_correspondences(uv_b, (H, W), K1, img_b_mask=mb)
        bg = cf.create_non_correspondences(uv_b, (H, W), K2, img_b_mask=1 - mb)
        ma = uv_a[1] * W + uv_a[0]
        matched = torch.zeros(H * W, dtype=torch.int64, device=d0.device)
        matched[ma] = 1
        blind_a = (m0[p].reshape(-1).long() - matched).nonzero().squeeze(1)
        bu, bv = cf.random_sample_from_masked_image_torch(mb, int(blind_a.numel()))
        rep = lambda k: ma.view(-1, 1).expand(-1, k).reshape(-1)
        tuples.append((ma, uv_b[1].long() * W + uv_b[0].long(), rep(K1), (nm[1].long() * W + nm[0].long()).reshape(-1),
                       rep(K2), (bg[1].long() * W + bg[0].long()).reshape(-1), blind_a, bv * W + bu))
    return PairLists.from_lists(tuples, d0.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--mirror-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib, samples
    _lib.load()
    dev = torch.device("cuda", 0)
    d0, d1, m0, m1, pa, pb = scene(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    kw = dict(num_matching_attempts=A, sample_matches_only_off_mask=True, num_masked_non_matches_per_match=K1,
              num_background_non_matches_per_match=K2, use_image_b_mask_inv=True)
    r = samples.build_within_scene_samples(d0, d1, m0, m1, pa, pb, generator=g, **kw)
    params, seeds = r.aug_params, r.seeds
    build = lambda: samples.build_within_scene_samples(d0, d1, m0, m1, pa, pb, aug_params=params, seeds=seeds, **kw)
    for _ in range(3):
        build()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        r = build()
    e1.record()
    torch.cuda.synchronize()
    us_build = e0.elapsed_time(e1) * 1e3 / a.iters
    off = r.offsets.cpu().numpy()
    cap = int(r.idx_a.numel())
    useful = int(off[-1])
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(10):
            build()
        torch.cuda.synchronize()
    wr = [e.device_time for e in prof.events() if "write_kernel" in e.name and e.device_time > 0]
    us_writer = float(np.mean(wr)) if wr else float("nan")
    wbytes = 16 * cap + 8 * useful
    per_pair = [[int(off[4 * p + t + 1] - off[4 * p + t]) for t in range(4)] for p in range(B)]
    res = {"shape": "B=%d pairs %dx%d, %d attempts, %d + %d non-matches per match, blind on" % (B, W, H, A, K1, K2),
           "lists_per_pair": per_pair, "capacity_entries": cap, "useful_entries": useful,
           "build_us_per_batch": round(us_build, 2), "writer_us": round(us_writer, 2), "writer_bytes": wbytes,
           "writer_GB_per_s": round(wbytes / (us_writer * 1e-6) / 1e9, 1),
           "writer_fraction_of_achievable": round(wbytes / (us_writer * 1e-6) / ACHIEVABLE, 3),
           "achievable_bps": ACHIEVABLE, "peak_bps": PEAK}
    print("build  %8.2f us/batch; writer %8.2f us, %d bytes, %.3f of 6.3 TB/s" % (us_build, us_writer, wbytes,
                                                                                res["writer_fraction_of_achievable"]), flush=True)
    times = []
    for it in range(a.mirror_iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mirror_batch(d0, d1, m0, m1, pa, pb)
        torch.cuda.synchronize()
        if it >= 1:
            times.append(time.perf_counter() - t0)
    res["mirror_ms_per_batch"] = round(1e3 * float(np.mean(times)), 3)
    res["speedup_vs_mirror"] = round(res["mirror_ms_per_batch"] * 1e3 / us_build, 1)
    print("mirror per-pair path: %.3f ms per batch (%.1fx)" % (res["mirror_ms_per_batch"], res["speedup_vs_mirror"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
