#!/usr/bin/env python3
"""Times painting mesh vertices from their views (csrc/paint_kernels.hip, dcn_hip.paint) on one MI355X: the box on a table of
tests/render_common.py, rendered at 640 x 480 from 16 poses on an arc and fused into a 0.75 m cube of 256^3 voxels; the fused
mesh's vertices are painted from F = 1, 16, 64 views of 640 x 480 (the depth images are the fused mesh's own, rendered on the
device; the views hold random values) -- uint8 views of c = 3 and float views of c = 3, 16, 32.

Per (view type, c, F): windows of back-to-back calls, device events and the wall clock around the same windows, 5 windows,
medians and max - min spreads, the variants INTERLEAVED window by window in one process:
  hip        MeshPaint.add (every launch of the call)
  torch      the same rule (include/dcn_hip.h 18a) written in torch float64 operations on the device, one frame after the other
             over all vertices; its count, sum and sumsq must EQUAL the kernel's (asserted once per case)
Rates of the hip variant: (vertex, view) pairs per second; gathered view bytes per second (c values per pair that passes rule 6)
against the achievable HBM rate; float64 operations per second (28 per pair that reaches the projection, 3 per channel of a
pair that passes) against the float64 vector peak.

    python tools/paint_bench.py [--out profiles/paint_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import render_common as rc                                                           # noqa: E402
from fusion_bench import EXTENT, FP64_VECTOR_PEAK, H, HBM_ACHIEVABLE, K, ORIGIN, W    # noqa: E402
from render_bench import arc_poses                                                   # noqa: E402
from train_bench import WINDOWS, summary, window                                     # noqa: E402

SIZE = 256
MARGIN_MM = 10.0
CASES = (("uint8", 3), ("float", 3), ("float", 16), ("float", 32))
HIP_CALLS = {1: 100, 16: 20, 64: 10}
TORCH_CALLS = {1: 10, 16: 2, 64: 1}
FP64_OPS_PROJECTION, FP64_OPS_PER_CHANNEL = 28, 3


def torch_paint(torch, count, total, squares, vertices, images, depth, cams, margin):
    """Rule 18a in torch float64 operations (each one correctly rounded operation per element, no contraction across
    operations), frame after frame over all vertices.  cams: float64 [F, 3, 4] (rule 16(a), made on the host).  A pair that
    does not pass adds +0.0, which leaves a sum as it is."""
    fx, fy, cx, cy = K
    F, h, w = depth.shape
    wx, wy, wz = (vertices[:, k].to(torch.float64) for k in range(3))
    zero = torch.zeros((), dtype=torch.float64, device=vertices.device)
    for f in range(F):
        a = cams[f]
        x, y, z = (((a[r][0] * wx + a[r][1] * wy) + a[r][2] * wz) + a[r][3] for r in range(3))
        ok = z > 0
        pu = torch.floor(((fx * x) / z + cx) + 0.0)
        pv = torch.floor(((fy * y) / z + cy) + 0.0)
        ok = ok & (pu >= 0) & (pu < w) & (pv >= 0) & (pv < h)
        iu, iv = torch.where(ok, pu, zero).to(torch.int64), torch.where(ok, pv, zero).to(torch.int64)
        mm = (depth[f].to(torch.int32) & 0xffff)[iv, iu]
        ok = ok & (mm != 0)
        e = z * 1000.0 - mm.to(torch.float64)
        ok = ok & (e >= -margin) & (e <= margin)
        values = torch.where(ok[:, None], images[f][iv, iu].to(torch.float64), zero)
        count += ok.to(torch.int32)
        total += values
        squares += values * values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("paint_bench: no GPU (a time measured anywhere else says nothing about the MI355X)")
    from dcn_hip import _lib, fusion, paint, render
    _lib.load()
    dev = torch.device("cuda", 0)
    (_, _), (full_v, full_t) = rc.box_over_plane()
    scene = render.Mesh(full_v, full_t, device=dev)
    fuse_poses = arc_poses(16)
    vol = fusion.TsdfVolume(ORIGIN, EXTENT / SIZE, (SIZE, SIZE, SIZE), device=dev)
    vol.integrate(render.render_depth(scene, fuse_poses, K, (H, W))[0], torch.from_numpy(fuse_poses).to(dev), K, pixel_offset=0.0)
    mesh = fusion.extract_mesh(vol, trim=True)                                        # (set-up: the one read-back)
    del vol
    V = mesh.num_vertices
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "windows": WINDOWS, "volume": SIZE, "vertices": V,
           "triangles": mesh.num_triangles, "margin_mm": MARGIN_MM, "runs": []}
    g = torch.Generator(device=dev).manual_seed(1)
    for F in (1, 16, 64):
        poses = arc_poses(F)
        p_dev = torch.from_numpy(poses).to(dev)
        cams = [rc.np_camera(p).tolist() for p in poses]
        depth = render.render_depth(mesh, p_dev, K, (H, W))[0]
        for kind, c in CASES:
            if kind == "uint8":
                views = torch.randint(0, 256, (F, H, W, c), dtype=torch.uint8, device=dev, generator=g)
            else:
                views = torch.randn((F, H, W, c), dtype=torch.float32, device=dev, generator=g)
            dtype = views.dtype
            paints = {"hip": paint.MeshPaint(mesh, c, dtype)}
            fns = {"hip": lambda: paints["hip"].add(views, depth, p_dev, K, margin_mm=MARGIN_MM)}
            ref = paint.MeshPaint(mesh, c, dtype)
            fns["torch"] = lambda: torch_paint(torch, ref.count, ref.sum, ref.sumsq, mesh.vertices, views, depth, cams, MARGIN_MM)
            for fn in fns.values():                                                   # warm-up, and the equality: one call each
                fn()
            for name, p in paints.items():
                equal = bool(torch.equal(p.count, ref.count) and torch.equal(p.sum, ref.sum) and torch.equal(p.sumsq, ref.sumsq))
                assert equal, "the torch formulation and %s disagree at %s c = %d, F = %d" % (name, kind, c, F)
            passed = int(ref.count.sum())
            samples = {name: [] for name in fns}
            for _ in range(WINDOWS):                                                  # interleaved; each adds into its own state
                for name, fn in fns.items():
                    samples[name].append(window(fn, TORCH_CALLS[F] if name == "torch" else HIP_CALLS[F]))
            rows = {name: summary(s) for name, s in samples.items()}
            for name, r in rows.items():
                r.update(what="paint", variant=name + (" float64 ops" if name == "torch" else ""), views=kind, c=c, F=F,
                         calls_per_window=TORCH_CALLS[F] if name == "torch" else HIP_CALLS[F])
                if name == "torch":
                    continue
                sec = r["device_us"] * 1e-6
                ops = FP64_OPS_PROJECTION * V * F + FP64_OPS_PER_CHANNEL * c * passed
                view_bytes = passed * c * views.element_size()
                r.update(equal_to_torch=True, pairs_passing=passed, pairs_per_s=round(V * F / sec, 0),
                         view_bytes_per_s=round(view_bytes / sec, 0),
                         view_share_of_achievable_hbm=round(view_bytes / sec / HBM_ACHIEVABLE, 4),
                         fp64_ops_per_s=round(ops / sec, 0), fp64_share_of_vector_peak=round(ops / sec / FP64_VECTOR_PEAK, 4),
                         torch_over_hip=round(rows["torch"]["device_us"] / r["device_us"], 1),
                         beats_torch_by_more_than_both_spreads=bool(
                             rows["torch"]["device_us"] - r["device_us"] > max(rows["torch"]["device_spread_us"], r["device_spread_us"])))
                print(json.dumps(r), flush=True)
            res["runs"] += [rows[name] for name in fns]
            del views, paints, ref, fns
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
