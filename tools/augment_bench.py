#!/usr/bin/env python3
"""Times the fused augmentation launch (csrc/augment_kernels.hip, dcn_augment_images) at B = 4 image pairs (8 images) of
640 x 480: uint8 RGB + uint8 mask in, float network input + float mask out = 20 bytes per pixel.  The launches rotate over
more than 256 MiB of distinct input / output buffers so that the Infinity Cache cannot serve repeats; the host is held behind
a device-side sleep while it queues them, so device events bracket back-to-back kernels only.  Reports microseconds per batch,
algorithmic bytes, GB/s and the fraction of the 6.3 TB/s achievable / 8 TB/s peak HBM bandwidth, for drawn records (the
training mix) and for the heaviest record (every image randomized with a gradient, hash noise and rotation).  For comparison
it also times the mirror path (correspondence_augmentation.py: host-drawn noise planes, one image per call).

    python tools/augment_bench.py [--iters 200] [--out profiles/augment_bench.json]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch  # noqa: E402

ACHIEVABLE, PEAK = 6.3e12, 8.0e12


def time_launches(launch, nsets, iters):
    """Mean device time of one launch: a device sleep keeps the GPU busy while the host queues `iters` launches."""
    for k in range(3 * nsets):                                   # warm-up
        launch(k % nsets)
    torch.cuda.synchronize()
    before, start, end = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    before.record()
    torch.cuda._sleep(int(1e8))                                    # (cycles) covers the host-side queueing below
    start.record()
    t0 = time.perf_counter()
    for k in range(iters):
        launch(k % nsets)
    queued_ms = 1e3 * (time.perf_counter() - t0)
    end.record()
    torch.cuda.synchronize()
    if before.elapsed_time(start) < queued_ms:
        print("warning: the device sleep (%.2f ms) ended before the host had queued the launches (%.2f ms): the time "
              "includes host gaps" % (before.elapsed_time(start), queued_ms), flush=True)
    return 1e3 * start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--mirror-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib, augment
    _lib.load()
    B, H, W = 4, 480, 640
    dev = torch.device("cuda", 0)
    per_set = 2 * B * H * W * (3 + 1 + 12 + 4)
    nsets = (256 << 20) // per_set + 2
    g = torch.Generator(device=dev).manual_seed(0)
    sets = []
    for _ in range(nsets):
        rgb = torch.randint(0, 256, (2 * B, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
        mask = (torch.rand(2 * B, H, W, device=dev, generator=g) > 0.3).to(torch.uint8)
        sets.append(dict(rgb=rgb, mask=mask, net=torch.empty(2 * B, 3, H, W, device=dev),
                         mout=torch.empty(2 * B, H, W, device=dev)))
    lib = _lib.get()
    mean = np.asarray(augment.DEFAULT_IMAGE_MEAN, np.float32)
    std = np.asarray(augment.DEFAULT_IMAGE_STD_DEV, np.float32)
    hp = lambda x: x.ctypes.data_as(_lib.c_void_p)
    heavy = augment.draw_params(2 * B, dev, generator=g)
    heavy[:, 0] = augment.RANDOMIZE | augment.GRADIENT | augment.NOISE | augment.FLIP_V | augment.FLIP_H
    heavy[::2, 0] |= augment.VERTICAL
    records = {"drawn": augment.draw_params(2 * B, dev, generator=g), "heaviest": heavy,
               "plain (no randomization, no rotation)": torch.zeros(2 * B, augment.PARAM_WORDS, dtype=torch.int32, device=dev)}
    p = lambda t: _lib.ptr(t)
    res = {"shape": "B=%d pairs (%d images) %dx%d" % (B, 2 * B, W, H), "distinct_bytes_rotated": per_set * nsets,
           "algorithmic_bytes_per_batch": per_set, "achievable_bps": ACHIEVABLE, "peak_bps": PEAK, "fused": {}}
    for name, prm in records.items():
        def launch(k, prm=prm):
            s = sets[k]
            rc = lib.dcn_augment_images(B, H, W, p(s["rgb"][:B]), p(s["rgb"][B:]), p(s["mask"][:B]), p(s["mask"][B:]), p(prm),
                                        None, hp(mean), hp(std), p(s["net"][:B]), p(s["net"][B:]), None, None,
                                        p(s["mout"][:B]), p(s["mout"][B:]), _lib.stream_ptr())
            _lib.check(rc, "dcn_augment_images")
        us = time_launches(launch, nsets, a.iters)
        bps = per_set / (us * 1e-6)
        res["fused"][name] = {"us_per_batch": round(us, 3), "GB_per_s": round(bps / 1e9, 1),
                              "fraction_of_achievable": round(bps / ACHIEVABLE, 3), "fraction_of_peak": round(bps / PEAK, 3)}
        print("fused %-40s %8.2f us/batch  %7.1f GB/s  %.3f of 6.3 TB/s  %.3f of 8 TB/s"
              % (name, us, bps / 1e9, bps / ACHIEVABLE, bps / PEAK), flush=True)
    # the drop-in mirror: one image per call, noise planes drawn by numpy on the host
    from dense_correspondence.correspondence_tools import correspondence_augmentation as ca
    rgb, mask = sets[0]["rgb"][0], sets[0]["mask"][0]
    uv = (torch.randint(0, W, (5000,), device=dev), torch.randint(0, H, (5000,), device=dev))
    random.seed(0)
    np.random.seed(0)
    times = {"domain_randomize_background (noise in about half the calls)": [], "random_image_and_indices_mutation": []}
    for it in range(a.mirror_iters + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ca.domain_randomize_background(rgb, mask)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ca.random_image_and_indices_mutation([rgb, mask], uv)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if it >= 2:
            times["domain_randomize_background (noise in about half the calls)"].append(t1 - t0)
            times["random_image_and_indices_mutation"].append(t2 - t1)
    res["mirror_ms_per_image"] = {k: round(1e3 * float(np.mean(v)), 3) for k, v in times.items()}
    print("mirror (host noise) ms per image:", res["mirror_ms_per_image"], flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
