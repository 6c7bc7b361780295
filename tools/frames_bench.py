#!/usr/bin/env python3
"""Times the frame store (csrc/frame_kernels.hip, dcn_hip/frames.py) at B = 4 pairs of 640 x 480 with training.yaml counts
(10 000 matching attempts, 75 masked + 75 background non-matches per match), from a store of 8 scenes x 250 frames (4 objects
of 2 scenes; 3.7 GB): the selection launch and the gather launch alone (device times of ``select_kernel`` / ``gather_kernel``
from the profiler's kernel records), the whole ``draw_training_batch`` (SINGLE_OBJECT_WITHIN_SCENE; device events around
back-to-back batches) next to the sample build alone on the same frames (with and without the augmentation of the images),
and, for comparison, today's host path: the reference's frame choice in Python, ``torch.stack`` of pinned host frames, the
host-to-device copy, and the same build.  The gather's bytes are the 2B frames' planes read and written (2 x 29.5 MB / 2)
plus the camera rows; reported against the 6.3 TB/s achievable HBM bandwidth.

    python tools/frames_bench.py [--iters 50] [--out profiles/frames_bench.json]"""
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

from augment_bench import ACHIEVABLE, PEAK  # noqa: E402

B, H, W, SCENES, PER_SCENE, OBJECTS = 4, 480, 640, 8, 250, 4
CFG = {"training": {"num_matching_attempts": 10000, "sample_matches_only_off_mask": True, "num_non_matches_per_match": 150,
                    "fraction_masked_non_matches": 0.5, "fraction_background_non_matches": 0.5,
                    "cross_scene_num_samples": 10000, "use_image_b_mask_inv": True, "domain_randomize": False,
                    "data_type_probabilities": {"SINGLE_OBJECT_WITHIN_SCENE": 1.0, "SINGLE_OBJECT_ACROSS_SCENE": 0.0,
                                                "DIFFERENT_OBJECT": 0.0, "MULTI_OBJECT": 0.0,
                                                "SYNTHETIC_MULTI_OBJECT": 0.0}}}


def make_store(dev):
    """Frames: random RGB, a depth surface per scene (no-return holes), a rectangular mask; camera positions spread over
    about 0.3 m per axis, so that most image b draws pass the 0.2 m test at once."""
    from dcn_hip import frames
    F = SCENES * PER_SCENE
    g = torch.Generator(device=dev).manual_seed(0)
    rgb = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    ys = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1)
    xs = torch.arange(W, device=dev, dtype=torch.float32).view(1, W)
    depth = torch.empty((F, H, W), dtype=torch.int16, device=dev)
    for s in range(SCENES):
        d = 900 + 150 * torch.sin(xs / (60 + 7 * s)) + 120 * torch.cos(ys / (50 + 5 * s))
        d = d * (torch.rand((H, W), device=dev, generator=g) >= 0.02)
        depth[s * PER_SCENE:(s + 1) * PER_SCENE] = d.to(torch.int16)
    mask = torch.zeros((F, H, W), dtype=torch.uint8, device=dev)
    mask[:, 120:360, 100:540] = 1
    rng = np.random.RandomState(1)
    poses = np.stack([np.eye(4)] * F)
    poses[:, :3, 3] = rng.uniform(-0.15, 0.15, (F, 3))
    first = [s * PER_SCENE for s in range(SCENES + 1)]
    sobj = [s // (SCENES // OBJECTS) for s in range(SCENES)]
    return frames.FrameStore.from_tensors(rgb, depth, mask, poses, first, sobj), poses, first, sobj


def kernel_us(fn, name, reps=20):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    t = [e.device_time for e in prof.events() if name in e.name and e.device_time > 0]
    return float(np.mean(t)) if t else float("nan")


def event_us(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def host_choice(poses, first, sobj, rnd):
    """The reference's SINGLE_OBJECT_WITHIN_SCENE choice in Python: object, scene, image a (two random.choice calls), image b
    by get_img_idx_with_different_pose (50 attempts, 0.2 m).  -> (frame a, frame b or None)"""
    objects = sorted(set(sobj))
    o = rnd.choice(objects)
    s = rnd.choice([i for i, x in enumerate(sobj) if x == o])
    idxs = list(range(first[s + 1] - first[s]))
    rnd.choice(idxs)
    a = first[s] + rnd.choice(idxs)
    for _ in range(50):
        rnd.choice(idxs)
        b = first[s] + rnd.choice(idxs)
        if np.linalg.norm(poses[a][0:3, 3] - poses[b][0:3, 3]) > 0.2:
            return a, b
    return a, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib, frames, samples
    _lib.load()
    dev = torch.device("cuda", 0)
    store, poses, first, sobj = make_store(dev)
    torch.cuda.synchronize()
    g = torch.Generator(device=dev).manual_seed(2)
    host = np.random.RandomState(2)
    sel = lambda: frames.select_frames(store, B, frames.SINGLE_OBJECT_WITHIN_SCENE, generator=g)
    sel_only = lambda: frames.select_frames(store, B, frames.SINGLE_OBJECT_WITHIN_SCENE, generator=g, gather=False)
    us_select = kernel_us(sel_only, "select_kernel")
    us_gather = kernel_us(sel, "gather_kernel")
    us_select_call = event_us(sel_only, a.iters)
    us_select_gather_call = event_us(sel, a.iters)
    gbytes = 2 * (2 * B) * H * W * 6 + B * 50 * 4
    draw = lambda: frames.draw_training_batch(store, B, CFG, generator=g, host_rng=host)
    us_draw = event_us(draw, a.iters)
    fb = sel()
    o = samples.options_from_config(CFG)
    kw = dict(num_matching_attempts=o.num_matching_attempts, sample_matches_only_off_mask=True,
              num_masked_non_matches_per_match=o.num_masked_non_matches_per_match,
              num_background_non_matches_per_match=o.num_background_non_matches_per_match, use_image_b_mask_inv=True,
              generator=g, cameras=fb.cams[0])
    build_plain = lambda: samples.build_within_scene_samples(fb.depth[0], fb.depth[1], fb.mask[0], fb.mask[1], None, None,
                                                             None, **kw)
    build_rgb = lambda: samples.build_within_scene_samples(fb.depth[0], fb.depth[1], fb.mask[0], fb.mask[1], None, None, None,
                                                           fb.rgb[0], fb.rgb[1], **kw)
    us_build = event_us(build_plain, a.iters)
    us_build_rgb = event_us(build_rgb, a.iters)
    # today's host path: Python choice, stack of pinned host frames, H2D, build (frames of the first scene on the host)
    hs = slice(0, PER_SCENE)
    h_rgb, h_depth, h_mask = (t[hs].cpu().pin_memory() for t in (store.rgb, store.depth, store.mask))
    h_first, h_sobj = [0, PER_SCENE // 2, PER_SCENE], [0, 0]
    h_poses = poses[hs]
    rnd = random.Random(3)
    times = []
    for it in range(a.host_iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ch = [host_choice(h_poses, h_first, h_sobj, rnd) for _ in range(B)]
        ia = [c[0] for c in ch]
        ib = [c[1] if c[1] is not None else c[0] for c in ch]
        st = lambda t, idx: torch.stack([t[i] for i in idx]).pin_memory().to(dev, non_blocking=True)
        ra, rb, da, db, ma, mb = st(h_rgb, ia), st(h_rgb, ib), st(h_depth, ia), st(h_depth, ib), st(h_mask, ia), st(h_mask, ib)
        samples.build_within_scene_samples(da, db, ma, mb, h_poses[ia], h_poses[ib], None, ra, rb,
                                           **dict(kw, cameras=None))
        torch.cuda.synchronize()
        if it >= 1:
            times.append(time.perf_counter() - t0)
    us_host = 1e6 * float(np.mean(times))
    res = {"shape": "B=%d pairs %dx%d, store %d scenes x %d frames (%.2f GB), %d attempts, %d + %d non-matches per match"
                    % (B, W, H, SCENES, PER_SCENE, store.nbytes / 1e9, o.num_matching_attempts,
                       o.num_masked_non_matches_per_match, o.num_background_non_matches_per_match),
           "select_kernel_us": round(us_select, 2), "gather_kernel_us": round(us_gather, 2),
           "select_call_us": round(us_select_call, 2), "select_and_gather_call_us": round(us_select_gather_call, 2),
           "gather_bytes": gbytes, "gather_GB_per_s": round(gbytes / (us_gather * 1e-6) / 1e9, 1),
           "gather_fraction_of_achievable": round(gbytes / (us_gather * 1e-6) / ACHIEVABLE, 3),
           "draw_training_batch_us": round(us_draw, 2), "build_alone_us": round(us_build, 2),
           "build_with_images_us": round(us_build_rgb, 2), "host_path_us": round(us_host, 1),
           "speedup_vs_host_path": round(us_host / us_draw, 1), "achievable_bps": ACHIEVABLE, "peak_bps": PEAK}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
