#!/usr/bin/env python3
"""Times the SYNTHETIC_MULTI_OBJECT path (csrc/synthetic_kernels.hip, samples.build_synthetic_multi_object_samples) at B = 4 and
B = 8 samples of 640 x 480 with training.yaml counts (10 000 matching attempts, 75 masked + 75 background non-matches per
match) on frames gathered from a synthetic store (4 objects x 2 scenes x 30 frames):

  (a) the fused builder alone;
  (b) the whole ``draw_training_batch(..., synthetic_multi_object=True)`` call (frame choice, gather, builder);
  (c) the composition of the entry points that existed before it on the same frames: two ``build_within_scene_samples``
      calls (whose non-matches and blind sets are dropped), the match lists unflattened on the device,
      ``merge.merge_synthetic_samples`` and ``samples.complete_samples``.

Device events around windows of 5 back-to-back calls, 5 windows each, (a) and (c) interleaved window by window in one process;
medians, and the spread (max - min) of (c)'s windows.  Accepted when (a) is not slower than (c) by more than that spread.
Launch counts: the device kernels one call enqueues (profiler records).

    python tools/synthetic_bench.py [--out profiles/synthetic_bench.json]"""
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

H, W, SCENES, PER_SCENE, OBJECTS = 480, 640, 8, 30, 4
WINDOWS, CALLS = 5, 5
CFG = {"training": {"num_matching_attempts": 10000, "sample_matches_only_off_mask": True, "num_non_matches_per_match": 150,
                    "fraction_masked_non_matches": 0.5, "fraction_background_non_matches": 0.5,
                    "cross_scene_num_samples": 10000, "use_image_b_mask_inv": True, "domain_randomize": False,
                    "data_type_probabilities": {"SINGLE_OBJECT_WITHIN_SCENE": 0.0, "SINGLE_OBJECT_ACROSS_SCENE": 0.0,
                                                "DIFFERENT_OBJECT": 0.0, "MULTI_OBJECT": 0.0,
                                                "SYNTHETIC_MULTI_OBJECT": 1.0}}}


def make_store(dev):
    """frames_bench's recipe with fewer frames, and a mask rectangle per object (left / right, overlapping in the middle) so
    that neither object hides the other completely"""
    from dcn_hip import frames
    F = SCENES * PER_SCENE
    g = torch.Generator(device=dev).manual_seed(0)
    rgb = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    ys = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1)
    xs = torch.arange(W, device=dev, dtype=torch.float32).view(1, W)
    depth = torch.empty((F, H, W), dtype=torch.int16, device=dev)
    mask = torch.zeros((F, H, W), dtype=torch.uint8, device=dev)
    sobj = [s // (SCENES // OBJECTS) for s in range(SCENES)]
    for s in range(SCENES):
        d = 900 + 150 * torch.sin(xs / (60 + 7 * s)) + 120 * torch.cos(ys / (50 + 5 * s))
        d = d * (torch.rand((H, W), device=dev, generator=g) >= 0.02)
        depth[s * PER_SCENE:(s + 1) * PER_SCENE] = d.to(torch.int16)
        x0 = 60 + 60 * sobj[s]
        mask[s * PER_SCENE:(s + 1) * PER_SCENE, 120:360, x0:x0 + 340] = 1
    rng = np.random.RandomState(1)
    poses = np.stack([np.eye(4)] * F)
    poses[:, :3, 3] = rng.uniform(-0.15, 0.15, (F, 3))
    first = [s * PER_SCENE for s in range(SCENES + 1)]
    return frames.FrameStore.from_tensors(rgb, depth, mask, poses, first, sobj)


def window_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_time > 0)


def composition(fb, o, fg, g):
    """What the existing entry points compose to, all on the device (no host read)"""
    from dcn_hip import merge, samples
    n, w = int(fb.mask.shape[1]), int(fb.mask.shape[3])
    A = o.num_matching_attempts
    uv, offs = [], []
    slot = torch.arange(A, device=fb.mask.device).view(1, A)
    for k in range(2):
        r = samples.build_within_scene_samples(
            fb.depth[2 * k], fb.depth[2 * k + 1], fb.mask[2 * k], fb.mask[2 * k + 1], None, None, None,
            num_matching_attempts=A, sample_matches_only_off_mask=o.sample_matches_only_off_mask,
            num_masked_non_matches_per_match=o.num_masked_non_matches_per_match,
            num_background_non_matches_per_match=o.num_background_non_matches_per_match,
            use_image_b_mask_inv=o.use_image_b_mask_inv, flip=False, generator=g, cameras=fb.cams[k])
        # the match lists (list 0 of every pair) as padded (u, v) lists of A slots per pair and their offsets
        start = r.offsets[0:4 * n:4]
        count = r.offsets[1:4 * n + 1:4] - start
        idx = (start.view(n, 1) + slot).clamp_(max=r.idx_a.numel() - 1)
        live = slot < count.view(n, 1)
        ia = torch.where(live, r.idx_a[idx], torch.zeros_like(idx))
        ib = torch.where(live, r.idx_b[idx], torch.zeros_like(idx))
        # compacted per pair: entries past a pair's count are moved behind every pair's live entries by a stable sort
        order = torch.sort((~live).view(-1).to(torch.int8), stable=True).indices
        ia, ib = ia.view(-1)[order], ib.view(-1)[order]
        total_offsets = torch.cat([count.new_zeros(1), torch.cumsum(count, 0)])
        uv.append(((ia % w, ia // w), (ib % w, ib // w)))
        offs.append(total_offsets)
    # merge_synthetic_samples takes lists of exactly offsets[-1] entries; the padded tail stays in as entries of no sample
    m = merge.merge_synthetic_samples(fb.rgb[0], fb.rgb[1], fb.rgb[2], fb.rgb[3], fb.mask[0], fb.mask[1], fb.mask[2], fb.mask[3],
                                      uv[0][0], uv[0][1], uv[1][0], uv[1][1], offs[0], offs[1], foreground=fg)
    return samples.complete_samples(m.uv_1, m.uv_2, m.offsets, fb.mask[1] | fb.mask[3], fb.mask[1] | fb.mask[3],
                                    num_masked_non_matches_per_match=o.num_masked_non_matches_per_match,
                                    num_background_non_matches_per_match=o.num_background_non_matches_per_match,
                                    use_image_b_mask_inv=o.use_image_b_mask_inv, generator=g)


def measure(store, B, dev):
    from dcn_hip import frames, merge, samples
    o = samples.options_from_config(CFG)
    g = torch.Generator(device=dev).manual_seed(2)
    host = np.random.RandomState(2)
    fb = frames.select_frames(store, B, frames.SYNTHETIC_MULTI_OBJECT, generator=g)
    fg = merge.draw_foreground(B, dev, generator=g)
    kw = dict(num_matching_attempts=o.num_matching_attempts, sample_matches_only_off_mask=o.sample_matches_only_off_mask,
              num_masked_non_matches_per_match=o.num_masked_non_matches_per_match,
              num_background_non_matches_per_match=o.num_background_non_matches_per_match,
              use_image_b_mask_inv=o.use_image_b_mask_inv)
    fused = lambda: samples.build_synthetic_multi_object_samples(fb.depth, fb.mask, fb.cams, fb.rgb, generator=g, foreground=fg,
                                                                 empty=fb.empty, **kw)
    draw = lambda: frames.draw_training_batch(store, B, CFG, generator=g, host_rng=host, synthetic_multi_object=True)
    comp = lambda: composition(fb, o, fg, g)
    sb = fused()[0]
    cb = comp()
    torch.cuda.synchronize()
    matches = int((sb.offsets[1::4] - sb.offsets[0:-1:4]).sum())
    matches_comp = int((cb.offsets[1::4] - cb.offsets[0:-1:4]).sum())
    for fn in (fused, draw, comp):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {"fused": [], "draw": [], "composition": []}
    for _ in range(WINDOWS):
        t["fused"].append(window_us(fused))
        t["composition"].append(window_us(comp))
        t["draw"].append(window_us(draw))
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = float(max(t["composition"]) - min(t["composition"]))
    return {"B": B, "fused_builder_us": round(med["fused"], 1), "draw_training_batch_us": round(med["draw"], 1),
            "composition_us": round(med["composition"], 1), "composition_spread_us": round(spread, 1),
            "fused_windows_us": [round(x, 1) for x in t["fused"]], "composition_windows_us": [round(x, 1) for x in t["composition"]],
            "draw_windows_us": [round(x, 1) for x in t["draw"]],
            "accepted": bool(med["fused"] <= med["composition"] + spread),
            "speedup_vs_composition": round(med["composition"] / med["fused"], 2),
            "launches_fused": launches(fused), "launches_draw_training_batch": launches(draw),
            "launches_composition": launches(comp), "matches_fused": matches, "matches_composition": matches_comp,
            "empty_samples": int(sb.empty.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    store = make_store(dev)
    torch.cuda.synchronize()
    res = {"shape": "samples of %dx%d, store %d scenes x %d frames of %d objects, 10000 attempts, 75 + 75 non-matches per "
                    "match; medians of %d windows of %d calls" % (W, H, SCENES, PER_SCENE, OBJECTS, WINDOWS, CALLS),
           "runs": [measure(store, B, dev) for B in (4, 8)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
