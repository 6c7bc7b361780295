#!/usr/bin/env python3
"""Times the descriptor statistics of a dataset (csrc/descstats_kernels.hip, dcn_hip/evaluate/descstats.py) at 640 x 480:

  1. the whole ``evaluate.compute_descriptor_statistics_on_dataset`` call for 100 frames of a synthetic store (4 scenes x 60
     frames), D = 3, real Resnet34_8s, 16 images per forward (wall clock around the call, which ends in its one copy to the
     host; the forward pass dominates it);
  2. the statistics launch alone on 16 descriptor images, D = 3 and D = 16, and on one image, D = 3:
     ``descriptor_statistics`` by device events around back-to-back calls, and the device times of ``stats_partial_kernel`` / ``stats_finish_kernel`` from the profiler's kernel
     records, against the traffic model n * H * W * (4 D + 1) bytes at the 6.3 TB/s achievable HBM bandwidth;
  3. the baseline, in the same process on the same images: the reference's per-image torch formulation
     (evaluation.py:2177-2292: ``mean/min/max`` over the image, ``torch.nonzero`` of the mask, ``index_select``, ``mean/min/max``
     again, the running update, ``tolist`` at the end), wall clock to the final lists.

Warm-up runs first; every wall-clock figure is the median of ``--repeats`` runs; the machine is named in the output.

    python tools/descstats_bench.py [--repeats 5] [--out profiles/descstats_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools"),
           os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch  # noqa: E402

from augment_bench import ACHIEVABLE, PEAK  # noqa: E402
from evaluate_bench import H, W, SCENES, PER_SCENE, make_store, median_wall  # noqa: E402
from frames_bench import event_us, kernel_us  # noqa: E402

N = 16


def baseline(res, mask):
    """The reference's formulation, image by image, on device tensors: -> its dict of lists"""
    stats = {k: {"min": None, "max": None, "mean": None} for k in ("entire_image", "mask_image")}
    for i in range(res.shape[0]):
        flat = res[i].contiguous().view(-1, res.shape[3])
        whole = (flat.min(0)[0], flat.max(0)[0], flat.mean(0))
        idx = torch.nonzero(mask[i].view(-1, 1).squeeze(1))
        if len(idx) == 0:
            continue
        sel = flat.index_select(0, idx.squeeze(1))
        for key, (lo, hi, mean) in (("entire_image", whole), ("mask_image", (sel.min(0)[0], sel.max(0)[0], sel.mean(0)))):
            s = stats[key]
            s["min"] = lo if s["min"] is None else torch.min(s["min"], lo)
            s["max"] = hi if s["max"] is None else torch.max(s["max"], hi)
            s["mean"] = mean if s["mean"] is None else s["mean"] + mean
    for val in stats.values():
        val["mean"] = 1.0 / res.shape[0] * val["mean"]
        for f in val:
            val[f] = val[f].tolist()
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dcn_hip import _lib, evaluate
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    _lib.load()
    dev = torch.device("cuda", 0)
    res = {"machine": torch.cuda.get_device_name(0), "library": _lib.library_info()["version"], "repeats": a.repeats,
           "achievable_bps": ACHIEVABLE, "peak_bps": PEAK, "launch": []}
    g = torch.Generator(device=dev).manual_seed(0)
    ys = torch.arange(H, device=dev).view(H, 1)
    xs = torch.arange(W, device=dev).view(1, W)
    mask = torch.stack([((xs - 300 - 5 * i) ** 2 + (ys - 240) ** 2 < (120 + 4 * i) ** 2) for i in range(N)]).to(torch.uint8)
    masks = mask
    for n, D in ((N, 3), (N, 16), (1, 3)):
        mask = masks[:n]
        x = torch.randn((n, H, W, D), device=dev, generator=g)
        call = lambda: evaluate.descriptor_statistics(x, mask)
        per, pix = call()
        stats, _ = evaluate.combine_descriptor_statistics(per, pix)
        us_call = event_us(call, a.iters)
        us_partial = kernel_us(call, "stats_partial_kernel")
        us_finish = kernel_us(call, "stats_finish_kernel")
        base = lambda: baseline(x, mask)
        want = base()
        t_base, all_base = median_wall(base, a.repeats)

        def ours():
            p, m = evaluate.descriptor_statistics(x, mask)
            return evaluate.combine_descriptor_statistics(p, m)[0].cpu()
        t_ours, all_ours = median_wall(ours, a.repeats)
        got = stats.cpu().numpy()
        ref = np.array([[want[k][f] for f in ("min", "max", "mean")] for k in ("entire_image", "mask_image")])
        nbytes = n * H * W * (4 * D + 1)
        res["launch"].append({
            "shape": "%d images %dx%d, D=%d" % (n, W, H, D), "model_bytes": nbytes,
            "descriptor_statistics_call_us": round(us_call, 2), "stats_partial_kernel_us": round(us_partial, 2),
            "stats_finish_kernel_us": round(us_finish, 2),
            "partial_kernel_GB_per_s": round(nbytes / (us_partial * 1e-6) / 1e9, 1),
            "partial_kernel_fraction_of_achievable": round(nbytes / (us_partial * 1e-6) / ACHIEVABLE, 4),
            "partial_kernel_fraction_of_peak": round(nbytes / (us_partial * 1e-6) / PEAK, 4),
            "statistics_and_combine_to_host_ms": round(t_ours * 1e3, 3),
            "statistics_and_combine_to_host_ms_all": [round(t * 1e3, 3) for t in all_ours],
            "baseline_torch_per_image_ms": round(t_base * 1e3, 3),
            "baseline_torch_per_image_ms_all": [round(t * 1e3, 3) for t in all_base],
            "baseline_over_ours": round(t_base / t_ours, 2),
            "min_max_equal_baseline": bool(np.array_equal(got[:, :2], ref[:, :2].astype(np.float32))),
            "largest_mean_difference_to_baseline": float(np.abs(got[:, 2] - ref[:, 2]).max())})
        del x
    store = make_store(dev)
    dcn = DenseCorrespondenceNetwork.from_config({"descriptor_dimension": 3, "image_width": W, "image_height": H},
                                                 load_stored_params=False)
    dcn.eval()
    whole = lambda: evaluate.compute_descriptor_statistics_on_dataset(dcn, store, a.images, save_to_file=False,
                                                                      host_rng=np.random.RandomState(3), batch_images=N)
    t_whole, all_whole = median_wall(whole, a.repeats)
    res["whole_call"] = {"shape": "%d frames %dx%d, D=3, Resnet34_8s, %d images per forward, store %d scenes x %d frames"
                                  % (a.images, W, H, N, SCENES, PER_SCENE),
                         "compute_descriptor_statistics_on_dataset_ms": round(t_whole * 1e3, 2),
                         "compute_descriptor_statistics_on_dataset_ms_all": [round(t * 1e3, 2) for t in all_whole]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
