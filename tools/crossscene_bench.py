#!/usr/bin/env python3
"""Times the cross-scene evaluation (csrc/crossscene_kernels.hip, dcn_hip/evaluate/cross_scene.py) for 5 annotated pairs x 8 labels x
(10 + 10) views of 640 x 480 at D = 3 and D = 16, on a synthetic frame store (ten scenes of twelve frames, the cameras turned
about the point the labelled image's central pixel sees, a pointwise stand-in network):

  1. the whole ``evaluate.evaluate_cross_scene_rows`` call (device time between two events; gathers and the stand-in's forward
     passes included);
  2. the reprojection and statistics launches alone: the ``reproject_pixels`` and ``match_statistics_groups`` calls of one
     chain run replayed on the tensors they were given, and the device time of ``group_stats_kernel`` from the profiler's
     kernel records against its traffic model, the searched images read once each (G * HW * D * 4 bytes);
  3. the baseline, in the same process: the same rows one by one through the pair-wise entry that existed before,
     ``match_statistics_pairs`` with P = 1 on the same descriptor images (computed beforehand, outside the timed window) --
     the reference's structure, one full-image search per row.

The two paths' results are compared first (every column bit for bit).  Warm-up runs first; every figure is the median of
``--repeats`` timed windows of ``--iters`` calls; the machine is named in the output.

    python tools/crossscene_bench.py [--repeats 5] [--iters 5] [--out profiles/crossscene_bench.json]"""
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
from frames_bench import event_us  # noqa: E402

H, W, PAIRS, LABELS, VIEWS, FRAMES = 480, 640, 5, 8, 10, 12


def rotation(axis, angle):
    n = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    X = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(angle) * X + (1 - np.cos(angle)) * X.dot(X)


def make_store(dev, seed=0):
    from dcn_hip import _args, frames
    rng = np.random.RandomState(seed)
    Kd = _args.camera_k_rows(None, 1)[0][0]
    pivot = 0.9 * np.linalg.inv(Kd).dot([0.5 * W, 0.5 * H, 1.0])
    S = 2 * PAIRS
    poses = []
    for _s in range(S):
        poses.append(np.eye(4))
        for _f in range(FRAMES - 1):                          # 13 .. 16 degrees about the pivot: more than 0.2 m away
            R = rotation([rng.randn(), rng.randn(), 0.0], np.deg2rad(rng.uniform(13, 16)))
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R, pivot - R.dot(pivot)
            poses.append(T)
    F = S * FRAMES
    g = torch.Generator(device=dev).manual_seed(seed)
    rgb = torch.randint(0, 256, (F, H, W, 3), device=dev, generator=g, dtype=torch.uint8)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    phase = torch.rand((F, 1, 1), device=dev, generator=g) * 6.28
    depth = (900 + 8 * torch.sin(xs[None] / 60.0 + phase) + 6 * torch.cos(ys[None] / 45.0 - phase)).to(torch.int16)
    depth[torch.rand((F, H, W), device=dev, generator=g) < 0.03] = 0
    mask = torch.zeros((F, H, W), dtype=torch.uint8, device=dev)
    mask[:, H // 5:4 * H // 5, W // 6:5 * W // 6] = 1
    store = frames.FrameStore.from_tensors(rgb, depth, mask, np.stack(poses), [FRAMES * s for s in range(S + 1)],
                                           list(range(S)), Kd)
    ann = []
    for p in range(PAIRS):
        px = lambda: [{"u": float(rng.uniform(0.3 * W, 0.7 * W)), "v": float(rng.uniform(0.3 * H, 0.7 * H))}
                      for _ in range(LABELS)]
        ann.append({"image_a": {"scene_name": "scene_%d" % (2 * p), "image_idx": 0, "pixels": px()},
                    "image_b": {"scene_name": "scene_%d" % (2 * p + 1), "image_idx": 0, "pixels": px()}})
    return store, ann


class PointwiseNetwork(torch.nn.Module):
    """D descriptors that are a fixed pointwise function of the normalized image (no batch-shape dependence)"""

    def __init__(self, D, dev):
        super().__init__()
        self.mix = torch.randn((3, D), device=dev, generator=torch.Generator(device=dev).manual_seed(D))

    def forward_image_tensors(self, x):
        return torch.tanh(x.permute(0, 2, 3, 1) @ self.mix).contiguous()


def kernel_total_us(fn, name, reps):
    """Device time of every kernel whose name holds ``name``, per call of ``fn``"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    return float(sum(e.device_time for e in prof.events() if name in e.name and e.device_time > 0)) / reps


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[3, 16])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib, evaluate
    _lib.load()
    dev = torch.device("cuda", 0)
    run(a, dev, _lib, evaluate)


def run(a, dev, _lib, evaluate):
    store, ann = make_store(dev)
    labels = evaluate.cross_scene_labels(store, ann)
    views = evaluate.choose_cross_scene_views(store, labels, VIEWS, VIEWS, np.random.RandomState(1))
    res = {"machine": torch.cuda.get_device_name(0) if dev.type == "cuda" else str(dev), "library": _lib.library_info()["version"],
           "shape": "%d annotated pairs x %d labels x (%d + %d) views, %dx%d" % (PAIRS, LABELS, VIEWS, VIEWS, W, H),
           "table_rows": int(views.shape[0]), "views_drawn": int(((views[:, 2] > 0) & (views[:, 3:5].min(1) >= 0)).sum()),
           "repeats": a.repeats, "iters": a.iters, "achievable_bps": ACHIEVABLE, "peak_bps": PEAK, "runs": []}
    for D in a.dims:
        net = PointwiseNetwork(D, dev)
        calls = {"groups": [], "reproject": []}
        chain = evaluate.cross_scene                           # (the module whose globals the chain looks the two up in)
        real = chain.match_statistics_groups, chain.reproject_pixels
        chain.match_statistics_groups = lambda *x, **k: (calls["groups"].append((x, k)), real[0](*x, **k))[1]
        chain.reproject_pixels = lambda *x, **k: (calls["reproject"].append((x, k)), real[1](*x, **k))[1]
        try:
            t = evaluate.evaluate_cross_scene_rows(net, store, labels, views)
        finally:
            chain.match_statistics_groups, chain.reproject_pixels = real
        assert int(t.status.cpu()[0]) == 0
        rows = torch.nonzero(t.row_pair >= 0)[:, 0]
        n = int(rows.numel())
        fr = views[rows.cpu().numpy(), 3:5]
        cams = torch.cat([evaluate._gather_host_frames(store, fr[lo:lo + 16384], ("cams",))[3][0] for lo in range(0, n, 16384)])
        # the baseline's descriptor images, one per distinct frame, computed outside the timed window
        used = np.unique(fr)
        slot = {int(f): i for i, f in enumerate(used)}
        desc = []
        for lo in range(0, len(used), 16):
            rgb, _, mask, _ = evaluate._gather_frame_list(store, used[lo:lo + 16], ("rgb", "mask"))
            evaluate._forward_in_eval_mode(net, rgb, mask, None, None, 16, evaluate._aug.DEFAULT_IMAGE_MEAN,
                                           evaluate._aug.DEFAULT_IMAGE_STD_DEV, lambda l, k, y: desc.append(y))
        desc = torch.cat(desc)
        one = torch.tensor([0, 1], device=dev)
        sa, sb = [slot[int(f)] for f in fr[:, 0]], [slot[int(f)] for f in fr[:, 1]]
        fa, fb = fr[:, 0].tolist(), fr[:, 1].tolist()
        ua, va, ub, vb = t.u_a[rows], t.v_a[rows], t.u_b[rows], t.v_b[rows]

        def base():
            return [evaluate.match_statistics_pairs(desc[sa[i]:sa[i] + 1], desc[sb[i]:sb[i] + 1], store.mask[fb[i]:fb[i] + 1],
                                                    store.depth[fa[i]:fa[i] + 1], store.depth[fb[i]:fb[i] + 1], cams[i:i + 1],
                                                    ua[i:i + 1], va[i:i + 1], ub[i:i + 1], vb[i:i + 1], one) for i in range(n)]

        def whole():
            return evaluate.evaluate_cross_scene_rows(net, store, labels, views)

        def launches():
            for x, k in calls["reproject"]:
                evaluate.reproject_pixels(*x, **k)
            return [evaluate.match_statistics_groups(*x, **k) for x, k in calls["groups"]]
        ref = base()
        same = all(bool(torch.equal(bits(getattr(t, k)[:, rows]), bits(torch.cat([getattr(r, k) for r in ref], dim=1))))
                   for k in ("columns", "is_valid", "pred_uv", "closer"))
        tm = {k: [] for k in ("whole", "launches", "base")}
        for _ in range(a.repeats):                             # the three alternate inside every repeat
            for k, fn, it in (("whole", whole, a.iters), ("launches", launches, a.iters), ("base", base, max(1, a.iters // 2))):
                tm[k].append(event_us(fn, it))
        us_stats = kernel_total_us(launches, "group_stats_kernel", max(3, a.iters))
        us_rows = kernel_total_us(launches, "group_rows_kernel", max(3, a.iters))
        us_reproject = kernel_total_us(launches, "reproject_kernel", max(3, a.iters))
        images = sum(int(x[0].shape[0]) for x, _ in calls["groups"])
        nbytes = images * H * W * D * 4
        med = {k: float(np.median(v)) for k, v in tm.items()}
        res["runs"].append({
            "D": D, "rows_with_a_result": n, "searched_images": images, "statistics_calls": len(calls["groups"]),
            "same_bits_as_baseline": bool(same),
            "whole_call_us": round(med["whole"], 1), "whole_call_us_all": [round(x, 1) for x in tm["whole"]],
            "launches_us": round(med["launches"], 1), "launches_us_all": [round(x, 1) for x in tm["launches"]],
            "group_stats_kernel_us": round(us_stats, 2), "group_rows_kernel_us": round(us_rows, 2),
            "reproject_kernel_us": round(us_reproject, 2), "group_stats_model_bytes": nbytes,
            "group_stats_GB_per_s": round(nbytes / (us_stats * 1e-6) / 1e9, 1),
            "group_stats_fraction_of_achievable": round(nbytes / (us_stats * 1e-6) / ACHIEVABLE, 4),
            "baseline_row_by_row_pairs_us": round(med["base"], 1), "baseline_us_all": [round(x, 1) for x in tm["base"]],
            "launches_speedup_vs_baseline": round(med["base"] / med["launches"], 2),
            "whole_call_over_baseline": round(med["whole"] / med["base"], 3)})
        del desc, ref, t
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
