#!/usr/bin/env python3
"""Times the evaluation on frame-store image pairs (csrc/evaluate_kernels.hip, dcn_hip/evaluate/pairs.py) for 25 and 100 image pairs
of 640 x 480, D = 3, on a synthetic store (4 scenes x 60 frames), real Resnet34_8s:

  1. the whole ``evaluate.evaluate_network`` call (wall clock around the call, which ends in its one copy to the host);
  2. the batched statistics launch alone (device time of ``pair_stats_kernel`` from the profiler's kernel records), against
     its traffic model P * HW * D * 4 bytes of res_b once plus the P * HW mask bytes, at the 6.3 TB/s achievable HBM bandwidth;
  3. the baseline: the same work with the public pieces that existed before -- per pair ``forward_single_image_tensor`` twice,
     candidates from mask a on the host, ``pairgen.find_correspondences``, ``DenseCorrespondenceNetwork.
     compute_match_statistics``, a copy to the host and the 3D half in numpy -- on the same pairs, in the same process.

Warm-up runs first; every figure is the median of ``--repeats`` runs; the machine is named in the output.

    python tools/evaluate_bench.py [--repeats 5] [--out profiles/evaluate_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools"),
           os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch  # noqa: E402

from augment_bench import ACHIEVABLE, PEAK  # noqa: E402
from evaluate_common import numpy_3d_from_poses  # noqa: E402  (the float64 restatement the tests use)
from frames_bench import kernel_us  # noqa: E402

H, W, D, SCENES, PER_SCENE = 480, 640, 3, 4, 60


def make_store(dev):
    from dcn_hip import frames
    F = SCENES * PER_SCENE
    g = torch.Generator(device=dev).manual_seed(0)
    rgb = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    ys = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1)
    xs = torch.arange(W, device=dev, dtype=torch.float32).view(1, W)
    depth = torch.empty((F, H, W), dtype=torch.int16, device=dev)
    for s in range(SCENES):
        d = 900 + 60 * torch.sin(xs / (60 + 7 * s)) + 50 * torch.cos(ys / (50 + 5 * s))
        d = d * (torch.rand((H, W), device=dev, generator=g) >= 0.02)
        depth[s * PER_SCENE:(s + 1) * PER_SCENE] = d.to(torch.int16)
    mask = torch.zeros((F, H, W), dtype=torch.uint8, device=dev)
    mask[:, 120:360, 100:540] = 1
    rng = np.random.RandomState(1)
    poses = np.stack([np.eye(4)] * F)
    poses[:, :2, 3] = rng.uniform(-0.06, 0.06, (F, 2))           # (views overlap: most candidates have a match)
    first = [s * PER_SCENE for s in range(SCENES + 1)]
    return frames.FrameStore.from_tensors(rgb, depth, mask, poses, first, [0, 0, 1, 1])


def baseline(dcn, store, chosen, host, num_matches, rng):
    """One ``evaluate_network`` worth of work, pair by pair, with the pieces that existed before the batched path"""
    from dcn_hip import augment, pairgen
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork as DCN
    dev = store.device
    mean = torch.tensor(augment.DEFAULT_IMAGE_MEAN, device=dev).view(3, 1, 1)
    std = torch.tensor(augment.DEFAULT_IMAGE_STD_DEV, device=dev).view(3, 1, 1)
    was = dcn.training
    dcn.eval()
    rows = 0
    for s, a, b in chosen:
        with torch.no_grad():
            res = [dcn.forward_single_image_tensor((store.rgb[f].permute(2, 0, 1).float().div(255) - mean) / std)
                   for f in (int(a), int(b))]
        on = np.flatnonzero(host["mask"][a].reshape(-1))
        pick = on[np.floor(rng.rand(20) * len(on)).astype(np.int64)]
        ua, va, ub, vb = pairgen.find_correspondences(store.depth[a], store.depth[b], store.K[s], host["poses"][a],
                                                      host["poses"][b], torch.from_numpy(pick % W).to(dev),
                                                      torch.from_numpy(pick // W).to(dev))
        n = int(ua.numel())
        if n == 0:
            continue
        sel = torch.from_numpy(rng.permutation(n)[:min(n, num_matches)]).to(dev)
        ua, va, ub, vb = ua[sel], va[sel], ub[sel], vb[sel]
        gu = torch.clamp(torch.floor(ub + 0.5).long(), max=W - 1)
        gv = torch.clamp(torch.floor(vb + 0.5).long(), max=H - 1)
        st = DCN.compute_match_statistics(torch.stack([ua, va], 1), torch.stack([gu, gv], 1), res[0], res[1], store.mask[b])
        hostd = {k: v.cpu().numpy() for k, v in st.items()}
        uv_a, gt = torch.stack([ua, va], 1).cpu().numpy(), torch.stack([gu, gv], 1).cpu().numpy()
        for i in range(len(uv_a)):
            numpy_3d_from_poses(store.K[s], host["poses"][a], host["poses"][b], host["depth"][a], host["depth"][b], uv_a[i], gt[i],
                                hostd["uv_b_pred"][i], hostd["uv_b_pred_masked"][i])
        rows += len(uv_a)
    dcn.train(was)
    return rows


def median_wall(fn, repeats):
    fn()                                                         # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, nargs="+", default=[25, 100])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib, evaluate
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    _lib.load()
    dev = torch.device("cuda", 0)
    store = make_store(dev)
    dcn = DenseCorrespondenceNetwork.from_config({"descriptor_dimension": D, "image_width": W, "image_height": H},
                                                 load_stored_params=False)
    dcn.eval()
    host = {"mask": store.mask.cpu().numpy(), "depth": store.depth.cpu().numpy().view(np.uint16),
            "poses": store.poses.cpu().numpy().reshape(-1, 4, 4)}
    torch.cuda.synchronize()
    res = {"machine": torch.cuda.get_device_name(0), "library": _lib.library_info()["version"],
           "shape": "%dx%d, D=%d, Resnet34_8s, store %d scenes x %d frames (%.2f GB), 100 matches per pair asked, 20 attempts"
                    % (W, H, D, SCENES, PER_SCENE, store.nbytes / 1e9), "repeats": a.repeats,
           "achievable_bps": ACHIEVABLE, "peak_bps": PEAK, "runs": []}
    for P in a.pairs:
        g = torch.Generator(device=dev).manual_seed(2)
        whole = lambda: evaluate.evaluate_network(dcn, store, P, 100, host_rng=np.random.RandomState(3), generator=g)
        table, _ = whole()
        rows = len(table["is_valid"])
        t_whole, all_whole = median_wall(whole, a.repeats)
        chosen = evaluate.choose_pairs(store, P, np.random.RandomState(3))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dev_ms = []
        for _ in range(a.repeats):                              # device time of the chain alone (HIP events, no final copy)
            e0.record()
            evaluate.evaluate_frame_pairs(dcn, store, chosen, 100, generator=g)
            e1.record()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
        us_stats = kernel_us(lambda: evaluate.evaluate_frame_pairs(dcn, store, chosen, 100, generator=g), "pair_stats_kernel",
                             reps=max(2, a.repeats))
        us_rows = kernel_us(lambda: evaluate.evaluate_frame_pairs(dcn, store, chosen, 100, generator=g), "pair_rows_kernel",
                            reps=max(2, a.repeats))
        nbytes = len(chosen) * H * W * (D * 4 + 1)
        rng = np.random.RandomState(4)
        base_rows = [0]

        def base():
            base_rows[0] = baseline(dcn, store, chosen, host, 100, rng)
        t_base, all_base = median_wall(base, a.repeats)
        res["runs"].append({
            "pairs_asked": P, "pairs": int(len(chosen)), "rows": rows, "baseline_rows": base_rows[0],
            "evaluate_network_ms": round(t_whole * 1e3, 2), "evaluate_network_ms_all": [round(t * 1e3, 2) for t in all_whole],
            "evaluate_frame_pairs_device_ms": round(float(np.median(dev_ms)), 2),
            "pair_stats_kernel_us": round(us_stats, 2), "pair_rows_kernel_us": round(us_rows, 2),
            "pair_stats_model_bytes": nbytes, "pair_stats_GB_per_s": round(nbytes / (us_stats * 1e-6) / 1e9, 1),
            "pair_stats_fraction_of_achievable": round(nbytes / (us_stats * 1e-6) / ACHIEVABLE, 4),
            "baseline_ms": round(t_base * 1e3, 2), "baseline_ms_all": [round(t * 1e3, 2) for t in all_base],
            "speedup_vs_baseline": round(t_base / t_whole, 2)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
