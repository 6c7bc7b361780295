#!/usr/bin/env python3
"""Times the loss on device-built batches (loss_composer.get_loss_mixed over SampleBatch.device_lists()) against the
host-offsets path it stands next to (SampleBatch.pair_lists() + get_loss_batched), forward + backward, warm, on one device:

  * ``config2``: BASELINE config-2 list sizes (B = 4, 5000 / 2500 / 2500 pairs, D = 3, 640 x 480) as exactly filled lists
    (the bounds are the true lengths);
  * ``training_yaml``: the lists build_within_scene_samples makes with training.yaml counts (10 000 attempts, 75 + 75
    non-matches per match, tools/sample_bench.py's scene), where the bounds are the builder's (750 000 per list: the grid
    covers that for all four lists of a pair, the match and blind lists fill a few percent of it).

Per case and path: device time per call between device events over back-to-back calls; the step-visible cost -- wall time per
step and the host time until the step is enqueued, with a queue of matrix products (standing in for the backbone) in front of
every loss call so that the parent path's read of the offsets really waits -- five repetitions each, mean and spread; and the
forward kernel's device time from the profiler's kernel records.  Then samples.concat_sample_batches for a 2 + 2 split.

    python tools/loss_mixed_bench.py [--reps 5] [--steps 20] [--out profiles/loss_mixed_bench.json]"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch  # noqa: E402

import sample_bench  # noqa: E402

B, H, W, D = 4, 480, 640, 3
LOSS_CONFIG = {"M_masked": 0.5, "M_background": 0.5, "M_pixel": 50, "match_loss_weight": 1.0, "non_match_loss_weight": 1.0,
               "use_l2_pixel_loss_on_masked_non_matches": False, "use_l2_pixel_loss_on_background_non_matches": False,
               "scale_by_hard_negatives": True, "scale_by_hard_negatives_DIFFERENT_OBJECT": True, "alpha_triplet": 0.1}


def config2_batch(dev):
    """config-2 lists as a SampleBatch: exactly filled (bounds = lengths), a -1 tail of one list's length."""
    from dcn_hip import samples
    g = torch.Generator(device=dev).manual_seed(3)
    lens = (5000, 2500, 2500, 0)
    r = lambda n: torch.randint(0, H * W, (n,), generator=g, device=dev)
    ia = torch.cat([r(n) for _ in range(B) for n in lens] + [torch.full((5000,), -1, dtype=torch.int64, device=dev)])
    ib = torch.cat([r(n) for _ in range(B) for n in lens] + [torch.full((5000,), -1, dtype=torch.int64, device=dev)])
    off = torch.tensor(np.cumsum([0] + list(lens) * B), dtype=torch.int64).to(dev)
    return samples.SampleBatch(None, None, ia, ib, off, torch.zeros(B, dtype=torch.bool, device=dev),
                               torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                               None, None, None, None, max(lens), sum(lens))


def training_yaml_batches(dev):
    from dcn_hip import samples
    d0, d1, m0, m1, pa, pb = sample_bench.scene(dev)
    kw = dict(num_matching_attempts=sample_bench.A, sample_matches_only_off_mask=True,
              num_masked_non_matches_per_match=sample_bench.K1, num_background_non_matches_per_match=sample_bench.K2,
              use_image_b_mask_inv=True)
    g = torch.Generator(device=dev).manual_seed(0)
    whole = samples.build_within_scene_samples(d0, d1, m0, m1, pa, pb, generator=g, **kw)
    halves = [samples.build_within_scene_samples(d0[s], d1[s], m0[s], m1[s], pa[s], pb[s], generator=g, **kw)
              for s in (slice(0, 2), slice(2, 4))]
    return whole, halves


def spread(xs):
    return {"mean": round(float(np.mean(xs)), 2), "min": round(float(np.min(xs)), 2), "max": round(float(np.max(xs)), 2)}


def measure(name, sb, dev, reps, steps):
    from dense_correspondence.loss_functions import loss_composer
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    pcl = PixelwiseContrastiveLoss(image_shape=[H, W], config=LOSS_CONFIG)
    g = torch.Generator(device=dev).manual_seed(4)
    da = ((torch.rand(B, H * W, D, device=dev, generator=g) * 2 - 1) * 0.3).requires_grad_(True)
    db = ((torch.rand(B, H * W, D, device=dev, generator=g) * 2 - 1) * 0.3).requires_grad_(True)
    x = torch.rand(4096, 4096, device=dev)

    def backbone():                               # a few milliseconds of queued device work in front of the loss
        y = x
        for _ in range(6):
            y = y @ x
        return y

    def parent():
        l = loss_composer.get_loss_batched(pcl, 0, da, db, sb.pair_lists())[0]
        return torch.autograd.grad(l, [da, db])

    def mixed():
        l = loss_composer.get_loss_mixed(pcl, da, db, sb.device_lists())[0]
        return torch.autograd.grad(l, [da, db])
    off = sb.offsets.cpu().numpy()
    res = {"lists_per_pair": [[int(off[4 * p + t + 1] - off[4 * p + t]) for t in range(4)] for p in range(B)],
           "capacity": int(sb.idx_a.numel()), "max_list_len_bound": int(sb.max_list_len)}
    from torch.profiler import ProfilerActivity, profile
    for label, call in (("parent", parent), ("mixed", mixed)):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        dev_us, wall_us, host_us = [], [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                call()
            e1.record()
            torch.cuda.synchronize()
            dev_us.append(e0.elapsed_time(e1) * 1e3 / steps)
            t0 = time.perf_counter()
            for _ in range(steps):
                backbone()
                call()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host_us.append((t1 - t0) * 1e6 / steps)
            wall_us.append((t2 - t0) * 1e6 / steps)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                call()
            torch.cuda.synchronize()
        kern = {}
        for e in prof.events():
            m = re.search(r"loss_\w+_kernel", e.name)
            if e.device_time > 0 and m:
                kern.setdefault(m.group(0), []).append(e.device_time)
        res[label] = {"call_us_back_to_back": spread(dev_us), "step_wall_us_behind_queued_work": spread(wall_us),
                      "step_host_us_behind_queued_work": spread(host_us),
                      "kernel_us": {k: round(float(np.mean(v)), 2) for k, v in sorted(kern.items())}}
        print("%-14s %-7s call %8.1f us  step wall %9.1f us (min %9.1f max %9.1f)  host %9.1f us" % (
            name, label, res[label]["call_us_back_to_back"]["mean"], res[label]["step_wall_us_behind_queued_work"]["mean"],
            res[label]["step_wall_us_behind_queued_work"]["min"], res[label]["step_wall_us_behind_queued_work"]["max"],
            res[label]["step_host_us_behind_queued_work"]["mean"]), flush=True)
        print("    kernels: %s" % res[label]["kernel_us"], flush=True)
    for _ in range(steps):                        # the queued work alone, for scale
        backbone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        backbone()
    torch.cuda.synchronize()
    res["queued_work_us"] = round((time.perf_counter() - t0) * 1e6 / steps, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib, samples
    _lib.load()
    dev = torch.device("cuda", 0)
    res = {"shape": "B=%d pairs %dx%d, D=%d, forward + backward" % (B, W, H, D), "reps": a.reps, "steps_per_rep": a.steps}
    res["config2"] = measure("config2", config2_batch(dev), dev, a.reps, a.steps)
    whole, halves = training_yaml_batches(dev)
    res["training_yaml"] = measure("training_yaml", whole, dev, a.reps, a.steps)
    for _ in range(3):
        samples.concat_sample_batches(halves)
    torch.cuda.synchronize()
    us = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            samples.concat_sample_batches(halves)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / a.steps)
    res["concat_2_plus_2"] = {"us": spread(us), "capacity": int(sum(h.idx_a.numel() for h in halves))}
    print("concat 2 + 2: %.1f us (capacity %d entries)" % (res["concat_2_plus_2"]["us"]["mean"],
                                                           res["concat_2_plus_2"]["capacity"]), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
