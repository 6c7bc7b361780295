#!/usr/bin/env python3
"""Times the synthetic multi-object merge (csrc/merge_kernels.hip) at B = 4 samples of 640 x 480 with 5 000 matches per
object and sample: the fused merge launch (dcn_merge_images, 2 frames: uint8 RGB + mask of both objects in, float network
input + float merged mask out = 24 bytes per pixel-frame) and the prune + concatenation (dcn_merge_prune, two launches).  The
merge launches rotate over more than 256 MiB of distinct input / output buffers so that the Infinity Cache cannot serve
repeats; the host is held behind a device-side sleep while it queues launches, so device events bracket back-to-back kernels
only.  Reports microseconds per batch, algorithmic bytes, GB/s and the fraction of the 6.3 TB/s achievable / 8 TB/s peak HBM
bandwidth.  For comparison it also times the mirror path (correspondence_augmentation.merge_images_with_occlusions: one frame
per call, one host read of the kept count).

    python tools/merge_bench.py [--iters 200] [--out profiles/merge_bench.json]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch  # noqa: E402

from augment_bench import ACHIEVABLE, PEAK, time_launches  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--mirror-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib, merge
    _lib.load()
    lib = _lib.get()
    B, H, W, NM = 4, 480, 640, 5000
    dev = torch.device("cuda", 0)
    per_set = 2 * B * H * W * (2 * 3 + 2 * 1 + 12 + 4)            # per pixel-frame: two RGB + two masks in, input + mask out
    nsets = (256 << 20) // per_set + 2
    g = torch.Generator(device=dev).manual_seed(0)
    sets = []
    for _ in range(nsets):
        rgb = torch.randint(0, 256, (4, B, H, W, 3), dtype=torch.uint8, device=dev, generator=g)     # a1, a2, b1, b2
        mask = (torch.rand(4, B, H, W, device=dev, generator=g) > 0.5).to(torch.uint8)
        sets.append(dict(rgb=rgb, mask=mask, net=torch.empty(2, B, 3, H, W, device=dev), mout=torch.empty(2, B, H, W, device=dev)))
    fg = merge.draw_foreground(B, dev, generator=g)
    mean = np.asarray(merge.DEFAULT_IMAGE_MEAN, np.float32)
    std = np.asarray(merge.DEFAULT_IMAGE_STD_DEV, np.float32)
    hp = lambda x: x.ctypes.data_as(_lib.c_void_p)
    p = _lib.ptr
    res = {"shape": "B=%d samples x 2 frames %dx%d, %d matches per object and sample" % (B, W, H, NM),
           "distinct_bytes_rotated": per_set * nsets, "algorithmic_bytes_per_batch": per_set, "achievable_bps": ACHIEVABLE,
           "peak_bps": PEAK, "foreground": fg.cpu().tolist()}

    def launch_merge(k):
        s = sets[k]
        r, m = s["rgb"], s["mask"]
        rc = lib.dcn_merge_images(B, 2, H, W, p(fg), p(r[0]), p(r[2]), p(r[1]), p(r[3]), p(m[0]), p(m[2]), p(m[1]), p(m[3]),
                                  hp(mean), hp(std), p(s["net"][0]), p(s["net"][1]), p(s["mout"][0]), p(s["mout"][1]), None,
                                  None, _lib.stream_ptr())
        _lib.check(rc, "dcn_merge_images")
    us = time_launches(launch_merge, nsets, a.iters)
    bps = per_set / (us * 1e-6)
    res["merge"] = {"us_per_batch": round(us, 3), "GB_per_s": round(bps / 1e9, 1),
                    "fraction_of_achievable": round(bps / ACHIEVABLE, 3), "fraction_of_peak": round(bps / PEAK, 3)}
    print("merge   %8.2f us/batch  %7.1f GB/s  %.3f of 6.3 TB/s  %.3f of 8 TB/s" % (us, bps / 1e9, bps / ACHIEVABLE,
                                                                                   bps / PEAK), flush=True)
    # prune + concatenation: 2 objects x B lists of NM entries, (u, v) in both frames
    n = B * NM
    lists = [torch.stack([torch.randint(0, W, (n,), device=dev, generator=g), torch.randint(0, H, (n,), device=dev, generator=g),
                          torch.randint(0, W, (n,), device=dev, generator=g), torch.randint(0, H, (n,), device=dev, generator=g)])
             for _ in range(2)]
    off = torch.arange(0, n + 1, NM, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.dcn_merge_prune_workspace(B, n, n)), dtype=torch.uint8, device=dev)
    out = torch.empty(4, 2 * n, dtype=torch.int64, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    empty = torch.empty(B, dtype=torch.bool, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)

    def launch_prune(k):
        m = sets[k]["mask"]
        la, lb = lists
        rc = lib.dcn_merge_prune(B, H, W, p(fg), p(m[0]), p(m[2]), p(m[1]), p(m[3]), p(la[0]), p(la[1]), p(la[2]), p(la[3]),
                                 p(off), n, p(lb[0]), p(lb[1]), p(lb[2]), p(lb[3]), p(off), n, merge.DROP_EMPTY, p(out[0]),
                                 p(out[1]), p(out[2]), p(out[3]), p(offsets), p(empty), p(status), p(ws), _lib.stream_ptr())
        _lib.check(rc, "dcn_merge_prune")
    us = time_launches(launch_prune, nsets, a.iters)
    kept = int(offsets[-1])
    pbytes = 2 * n * (4 * 8) + kept * 4 * 8                          # every entry's four coordinates in, kept ones out
    res["prune"] = {"us_per_batch": round(us, 3), "entries_in": 2 * n, "entries_kept": kept,
                    "algorithmic_bytes_per_batch": pbytes, "GB_per_s": round(pbytes / (us * 1e-6) / 1e9, 1)}
    print("prune   %8.2f us/batch  (%d entries in, %d kept, %d algorithmic bytes)" % (us, 2 * n, kept, pbytes), flush=True)
    # the drop-in mirror: one frame per call, one host read of the kept count
    from dense_correspondence.correspondence_tools import correspondence_augmentation as ca
    s = sets[0]
    pa = ((lists[0][0][:NM], lists[0][1][:NM]), (lists[0][2][:NM], lists[0][3][:NM]))
    pb = ((lists[1][0][:NM], lists[1][1][:NM]), (lists[1][2][:NM], lists[1][3][:NM]))
    random.seed(0)
    times = []
    for it in range(a.mirror_iters + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ca.merge_images_with_occlusions(s["rgb"][0, 0], s["rgb"][2, 0], s["mask"][0, 0], s["mask"][2, 0], pa, pb)
        torch.cuda.synchronize()
        if it >= 2:
            times.append(time.perf_counter() - t0)
    res["mirror_ms_per_frame"] = round(1e3 * float(np.mean(times)), 3)
    print("mirror merge_images_with_occlusions ms per frame:", res["mirror_ms_per_frame"], flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
