#!/usr/bin/env python3
"""Times the depth renderer (csrc/render_kernels.hip, dcn_hip.render) on a scene the size of the reference's: a synthetic fused
mesh of 2 000 000 small triangles (a bumpy height field over the field of view, 1000 x 1000 cells) plus a table of 2 triangles
behind it, 640 x 480, F = 1 / 16 / 64 poses on an arc.

Per F: ``render_depth`` (every launch of the call: fills, both raster kernels, the pack) in windows of back-to-back calls,
device events and the wall clock around the same windows (ending in a synchronize); 5 windows, medians and max - min spreads.
The same for ``render_scene`` (both meshes and the masks) at F = 16.

Against: the numpy statement of tests/render_common.py (what the tests hold the kernels to) on the F = 1 frame, the triangles
split over 16 processes and the partial images joined by the minimum -- run ONCE (it takes seconds: most triangles of such a mesh cover no pixel centre and leave the loop early), wall clock; its
image must equal the device's, and it counts the fragments (triangle, covered pixel centre), which is the number of atomics the
small-triangle path issues.  Rates of the F = 1 call: atomics per second, and the bytes of its triangle reads (12 bytes of
indices + 36 bytes of gathered vertices per triangle and frame) per second against the achievable HBM rate (6.3 TB/s).

    python tools/render_bench.py [--out profiles/render_bench.json] [--cells 1000] [--host-processes 16]"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import render_common as rc                                                           # noqa: E402
from train_bench import WINDOWS, summary, window                                     # noqa: E402

H, W = 480, 640
K = (540.0, 540.0, 320.0, 240.0)
CALLS = {1: 1000, 16: 100, 64: 25}           # windows of some 50 ms
HBM_ACHIEVABLE = 6.3e12


def fused_mesh(cells):
    """A height field of cells x cells quads (two triangles each) that fills the view at about 1 m, with bumps of a few
    centimetres: triangles of a fraction of a pixel to a few pixels, as a fused scan has them"""
    n = cells + 1
    x = np.linspace(-0.62, 0.62, n)
    y = np.linspace(-0.47, 0.47, n)
    xx, yy = np.meshgrid(x, y)
    zz = 1.0 + 0.04 * np.sin(9.0 * xx) * np.cos(7.0 * yy) + 0.01 * np.sin(61.0 * xx + 3.0 * yy)
    verts = np.stack([xx, yy, zz], axis=-1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(cells)[:, None] * n + np.arange(cells)[None, :]).reshape(-1)
    tris = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i, i + n + 1, i + n], 1)]).astype(np.int32)
    return verts, tris


def table_mesh():
    verts = np.array([[-3, -3, 1.3], [3, -3, 1.3], [3, 3, 1.3], [-3, 3, 1.3]], np.float32)
    return verts, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def arc_poses(F):
    out = []
    for k in range(F):
        a = 0.3 * (k / max(F - 1, 1) - 0.5) if F > 1 else 0.0
        c, s = np.cos(a), np.sin(a)
        p = np.eye(4)
        p[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]                 # about the camera's y, looking at the scene's middle
        p[:3, 3] = [-np.sin(a) * 1.0, 0.01 * k / max(F, 1), 1.0 - np.cos(a) * 1.0]
        out.append(p)
    return np.stack(out).astype(np.float32)


def _host_part(args):
    verts, tris, pose = args
    counts = {}
    depth, status = rc.np_render(verts, tris, pose[None], K, H, W, counts=counts)
    return depth[0], status[0], counts.get("fragments", 0)


def host_statement(verts, tris, pose, processes):
    """-> (depth uint16 [H, W], status [2], fragments, wall seconds): the triangles in ``processes`` parts, joined by the minimum"""
    parts = [(verts, tris[k::processes], pose) for k in range(processes)]
    t0 = time.perf_counter()
    with multiprocessing.get_context("fork").Pool(processes) as pool:
        res = pool.map(_host_part, parts)
    z = np.stack([np.where(d == 0, 65536, d.astype(np.int64)) for d, _, _ in res]).min(axis=0)
    depth = np.where(z == 65536, 0, z).astype(np.uint16)
    return depth, sum(s for _, s, _ in res), sum(n for _, _, n in res), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cells", type=int, default=1000)
    ap.add_argument("--host-processes", type=int, default=16)
    a = ap.parse_args()
    fv, ft = fused_mesh(a.cells)
    tv, tt = table_mesh()
    verts = np.concatenate([fv, tv])
    tris = np.concatenate([ft, tt + len(fv)])
    # the host's run first, before this process opens the GPU (its workers are forked)
    pose1 = arc_poses(1)
    host_depth, host_status, fragments, host_s = host_statement(verts, tris, pose1[0], a.host_processes)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("render_bench: no GPU (a time measured anywhere else says nothing about the MI355X)")
    from dcn_hip import _lib, render
    _lib.load()
    dev = torch.device("cuda", 0)
    full = render.Mesh(verts, tris, device=dev)
    fg = render.Mesh(fv, ft, device=dev)
    T = full.num_triangles
    res = {"device": torch.cuda.get_device_name(0), "triangles": T, "vertices": full.num_vertices, "shape": [H, W],
           "windows": WINDOWS, "runs": []}
    depth, status = render.render_depth(full, torch.from_numpy(pose1).to(dev), K, (H, W))
    res["equals_numpy_statement"] = bool(np.array_equal(depth[0].cpu().numpy().view(np.uint16), host_depth)
                                         and np.array_equal(status[0].cpu().numpy(), host_status))
    res["pixels_with_surface"] = int((host_depth > 0).sum())
    for F in (1, 16, 64):
        poses = torch.from_numpy(arc_poses(F)).to(dev)
        fn = lambda: render.render_depth(full, poses, K, (H, W))
        for _ in range(2):
            fn()
        r = summary([window(fn, CALLS[F]) for _ in range(WINDOWS)])
        r.update(F=F, calls_per_window=CALLS[F], what="render_depth",
                 device_us_per_frame=round(r["device_us"] / F, 1),
                 triangle_read_bytes_per_s=round(F * T * 48 / (r["device_us"] * 1e-6), 0),
                 triangle_read_share_of_achievable_hbm=round(F * T * 48 / (r["device_us"] * 1e-6) / HBM_ACHIEVABLE, 4))
        if F == 1:
            r.update(fragments=int(fragments), atomics_per_s=round(fragments / (r["device_us"] * 1e-6), 0))
        res["runs"].append(r)
    poses = torch.from_numpy(arc_poses(16)).to(dev)
    fn = lambda: render.render_scene(fg, full, poses, K, (H, W))
    for _ in range(2):
        fn()
    r = summary([window(fn, 50) for _ in range(WINDOWS)])
    r.update(F=16, calls_per_window=50, what="render_scene (both meshes, masks)")
    res["runs"].append(r)
    res["numpy_statement"] = {"F": 1, "processes": a.host_processes, "wall_s": round(host_s, 2), "runs": 1,
                              "wall_ratio_over_device_call": round(host_s * 1e6 / res["runs"][0]["wall_us"], 0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
