#!/usr/bin/env python3
"""Times TSDF fusion, surface extraction and the box crop (csrc/fusion_kernels.hip, dcn_hip.fusion) on one MI355X: the box on a
table of tests/render_common.py, rendered at 640 x 480 from F poses on an arc, fused into a 0.75 m cube of 256^3 and 512^3
voxels.

``integrate`` for F = 1, 16, 64 at both sizes: windows of back-to-back calls, device events and the wall clock around the same
windows, 5 windows, medians and max - min spreads, the variants INTERLEAVED window by window in one process:
  hip     TsdfVolume.integrate (every launch of the call)
  torch   the same rule (include/dcn_hip.h 17a) written in torch float64 operations on the device, one frame after the other
          over the whole volume; its sum and weight must EQUAL the kernel's (asserted once per size and F)
and, once, the numpy statement of tests/fusion_common.py on the host at 256^3, F = 1 (wall clock; equal state asserted).
Rates of the hip variant: voxel-frames per second; state traffic (16 bytes per voxel and launch) per second against the
achievable HBM rate; float64 operations per second (32 per voxel-frame that reaches step 8, four of them divisions) against
the float64 vector peak.

Then ``extract_mesh(trim=False)`` and ``crop_to_box(trim=False)`` on the 256^3 volume fused from 16 frames, and the whole
``fuse_scene`` (16 frames, 256^3).

    python tools/fusion_bench.py [--out profiles/fusion_bench.json] [--sizes 256 512]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fusion_common as fc                                                           # noqa: E402
import render_common as rc                                                           # noqa: E402
from render_bench import arc_poses                                                   # noqa: E402
from train_bench import WINDOWS, summary, window                                     # noqa: E402

H, W = 480, 640
K = (540.0, 540.0, 320.0, 240.0)
EXTENT = 0.75
ORIGIN = (-0.25, -0.25, 0.625)
HIP_CALLS = {(256, 1): 200, (256, 16): 40, (256, 64): 10, (512, 1): 40, (512, 16): 6, (512, 64): 2}
TORCH_CALLS = {(256, 1): 4, (256, 16): 1, (256, 64): 1, (512, 1): 1, (512, 16): 1, (512, 64): 1}
HBM_ACHIEVABLE = 6.3e12
FP64_VECTOR_PEAK = 78.6e12          # the MI355X's published float64 vector rate (half its 157.3 TFLOPS fp32 vector rate)
FP64_OPS_PER_VOXEL_FRAME = 32
FRAMES_PER_LAUNCH = 32


def torch_integrate(torch, total, weight, status, depth, cams, origin, s, mu, o, max_mm):
    """Rule 17a in torch float64 operations (each one correctly rounded operation per element, no contraction across
    operations), frame after frame over the whole volume.  cams: float64 [F, 3, 4] (rule 16(a), made on the host)."""
    nz, ny, nx = total.shape
    dev = total.device
    f64 = dict(dtype=torch.float64, device=dev)
    wx = (origin[0] + s * torch.arange(nx, **f64))[None, None, :]
    wy = (origin[1] + s * torch.arange(ny, **f64))[None, :, None]
    wz = (origin[2] + s * torch.arange(nz, **f64))[:, None, None]
    F, h, w = depth.shape
    fx, fy, cx, cy = K
    for f in range(F):
        a = cams[f]
        x, y, z = (((a[r][0] * wx + a[r][1] * wy) + a[r][2] * wz) + a[r][3] for r in range(3))
        ok = z > 0
        pu = torch.floor(((fx * x) / z + cx) + o)
        pv = torch.floor(((fy * y) / z + cy) + o)
        ok = ok & (pu >= 0) & (pu < w) & (pv >= 0) & (pv < h)
        zero = torch.zeros((), **f64)
        iu, iv = torch.where(ok, pu, zero).to(torch.int64), torch.where(ok, pv, zero).to(torch.int64)
        mm = (depth[f].to(torch.int32) & 0xffff)[iv, iu]
        ok = ok & (mm != 0) & (mm <= max_mm)
        diff = mm.to(torch.float64) / 1000.0 - z
        ok = ok & (diff > -mu)
        q = torch.round(torch.clamp(diff / mu, max=1.0) * 32768.0)
        full = ok & (weight >= fc.MAX_WEIGHT)
        take = ok & ~full
        total += torch.where(take, q, zero).to(torch.int32)
        weight += take.to(torch.int32)
        status += full.sum().to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fusion_bench: no GPU (a time measured anywhere else says nothing about the MI355X)")
    from dcn_hip import _lib, fusion, render
    _lib.load()
    dev = torch.device("cuda", 0)
    (_, _), (full_v, full_t) = rc.box_over_plane()
    scene = render.Mesh(full_v, full_t, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "windows": WINDOWS, "runs": []}
    images, poses = {}, {}
    for F in (1, 16, 64):
        poses[F] = arc_poses(F)
        images[F] = render.render_depth(scene, poses[F], K, (H, W))[0]
    for n in a.sizes:
        s = EXTENT / n
        mu = 5.0 * s
        for F in (1, 16, 64):
            depth, p_dev = images[F], torch.from_numpy(poses[F]).to(dev)
            cams = [rc.np_camera(p).tolist() for p in poses[F]]
            hip = fusion.TsdfVolume(ORIGIN, s, (n, n, n), device=dev)
            hip.integrate(depth, p_dev, K, pixel_offset=0.0)
            ref = fusion.TsdfVolume(ORIGIN, s, (n, n, n), device=dev)
            torch_integrate(torch, ref.sum, ref.weight, ref.status, depth, cams, ORIGIN, s, mu, 0.0, fusion.DEFAULT_MAX_DEPTH_MM)
            equal = bool(torch.equal(hip.sum, ref.sum) and torch.equal(hip.weight, ref.weight))
            assert equal, "the torch formulation and the kernel disagree at %d^3, F = %d" % (n, F)
            reached = int(hip.weight.sum())
            if n == a.sizes[0] and F == 1:
                t0 = time.perf_counter()
                host = fc.np_integrate(fc.empty_state((n, n, n)), depth.cpu().numpy(), poses[F], K, ORIGIN, s, mu, 0.0)
                host_s = time.perf_counter() - t0
                assert np.array_equal(host[0], hip.sum.cpu().numpy()) and np.array_equal(host[1], hip.weight.cpu().numpy())
                res["numpy_statement"] = {"size": n, "F": 1, "wall_s": round(host_s, 2), "runs": 1, "equal": True}
            fn_hip = lambda: hip.integrate(depth, p_dev, K, pixel_offset=0.0)
            fn_torch = lambda: torch_integrate(torch, ref.sum, ref.weight, ref.status, depth, cams, ORIGIN, s, mu, 0.0,
                                               fusion.DEFAULT_MAX_DEPTH_MM)
            samples = {"hip": [], "torch": []}
            for _ in range(WINDOWS):                             # interleaved; both accumulate into their own volume
                samples["hip"].append(window(fn_hip, HIP_CALLS.get((n, F), 20)))
                samples["torch"].append(window(fn_torch, TORCH_CALLS.get((n, F), 1)))
            r_hip, r_torch = summary(samples["hip"]), summary(samples["torch"])
            sec = r_hip["device_us"] * 1e-6
            launches = -(-F // FRAMES_PER_LAUNCH)
            r_hip.update(what="integrate", variant="hip", size=n, F=F, calls_per_window=HIP_CALLS.get((n, F), 20), equal_to_torch=equal,
                         voxel_frames_per_s=round(n ** 3 * F / sec, 0), voxel_frames_reaching_step_8=reached,
                         state_bytes_per_s=round(16.0 * n ** 3 * launches / sec, 0),
                         state_share_of_achievable_hbm=round(16.0 * n ** 3 * launches / sec / HBM_ACHIEVABLE, 4),
                         fp64_ops_per_s=round(FP64_OPS_PER_VOXEL_FRAME * n ** 3 * F / sec, 0),
                         fp64_share_of_vector_peak=round(FP64_OPS_PER_VOXEL_FRAME * n ** 3 * F / sec / FP64_VECTOR_PEAK, 4))
            r_torch.update(what="integrate", variant="torch float64 ops", size=n, F=F, calls_per_window=TORCH_CALLS.get((n, F), 1))
            r_hip["torch_over_hip"] = round(r_torch["device_us"] / r_hip["device_us"], 1)
            r_hip["beats_torch_by_more_than_its_spread"] = bool(r_torch["device_us"] - r_hip["device_us"] > r_torch["device_spread_us"])
            res["runs"] += [r_hip, r_torch]
            print(json.dumps(r_hip), flush=True)
            del hip, ref
            torch.cuda.empty_cache()
    n = 256
    spec = dict(origin=ORIGIN, voxel_size=EXTENT / n, shape=(n, n, n))
    crop = fc.SCENE_CROP
    vol = fusion.TsdfVolume(device=dev, **spec).integrate(images[16], torch.from_numpy(poses[16]).to(dev), K, pixel_offset=0.0)
    mesh, counts = fusion.extract_mesh(vol, trim=False)
    fg, fg_counts = fusion.crop_to_box(mesh, crop["transform"], crop["dimensions"], trim=False)
    sizes = dict(vertices=int(counts[0]), triangles=int(counts[1]), capacity=[int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])],
                 foreground_vertices=int(fg_counts[0]), foreground_triangles=int(fg_counts[1]))
    for what, fn, calls in (("extract_mesh(trim=False)", lambda: fusion.extract_mesh(vol, trim=False), 20),
                            ("crop_to_box(trim=False)", lambda: fusion.crop_to_box(mesh, crop["transform"], crop["dimensions"], trim=False), 50),
                            ("fuse_scene", lambda: fusion.fuse_scene(images[16], torch.from_numpy(poses[16]).to(dev), K, spec, crop,
                                                                     pixel_offset=0.0), 5)):
        fn()
        r = summary([window(fn, calls) for _ in range(WINDOWS)])
        r.update(what=what, size=n, F=16, calls_per_window=calls, **sizes)
        res["runs"].append(r)
        print(json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
