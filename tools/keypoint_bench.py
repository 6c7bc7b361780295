#!/usr/bin/env python3
"""Times the class-consistent keypoint table (dcn_hip/evaluate/keypoints.py, the wide statistics kernel of csrc/crossscene_kernels.hip)
at 640 x 480, D = 3 and D = 16, for K = 8, 24 and 64 labelled images x 8 keypoints: every labelled image is searched by
(K - 1) * 8 = 56, 184 and 504 rows.

  1. ``match_statistics_groups_wide`` (one row per lane) and ``match_statistics_groups`` (one pixel per lane, six wave
     reductions per query) on the same rows in one process, the two interleaved inside every repeat; their tables are compared
     first (every output bit for bit, asserted);
  2. the whole ``evaluate.evaluate_keypoint_rows`` call on a synthetic frame store with a pointwise stand-in network (gathers
     and the K forward passes included), with ``search`` = "wide", "groups" and None.

Every figure is the median of ``--repeats`` timed windows of ``--iters`` calls between two device events, after warm-up calls;
the machine is named in the output.  The parent process starts no GPU work itself: every (D, part) step is a process of its
own under ``timeout -k 10``, and the first step that fails ends the run.

    python tools/keypoint_bench.py [--repeats 5] [--iters 5] [--out profiles/keypoint_bench.json]
    python tools/keypoint_bench.py --images 8 --keypoints 2 --parts statistics      (fewer rows per image: the crossover)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

H, W, KEYPOINTS, IMAGES = 480, 640, 8, (8, 24, 64)
STEP_SECONDS = 240


def make_rows(K, D, dev, seed):
    """The rows of the keypoint table as the statistics entries take them: K searched images, (K - 1) * KEYPOINTS rows each"""
    import torch
    from dcn_hip import _args
    g = torch.Generator(device=dev).manual_seed(seed)
    per = (K - 1) * KEYPOINTS
    R = K * per
    res_b = torch.tanh(torch.randn((K, H, W, D), device=dev, generator=g))
    mask_b = torch.zeros((K, H, W), dtype=torch.uint8, device=dev)
    mask_b[:, H // 5:4 * H // 5, W // 6:5 * W // 6] = 1
    depth_b = torch.full((K, H, W), 900, dtype=torch.int16, device=dev)
    u_a = torch.randint(0, W, (R,), device=dev, generator=g)
    v_a = torch.randint(0, H, (R,), device=dev, generator=g)
    # a query resembles its ground truth, as a trained network's would: few pixels are closer than the ground truth
    u_b = torch.randint(W // 6, 5 * W // 6, (R,), device=dev, generator=g)
    v_b = torch.randint(H // 5, 4 * H // 5, (R,), device=dev, generator=g)
    group = torch.arange(R, device=dev) // per
    queries = (res_b[group, v_b, u_b] + 0.05 * torch.randn((R, D), device=dev, generator=g)).contiguous()
    cams = torch.zeros((R, 50), device=dev)
    Kd = torch.from_numpy(np.asarray(_args.camera_k_rows(None, 1)[1][0], np.float32)).to(dev)
    cams[:, :18] = Kd
    for c in (18, 34):
        cams[:, c:c + 16] = torch.eye(4, device=dev).reshape(16)
    return dict(res_b=res_b, mask_b=mask_b, depth_b=depth_b, queries=queries, u_a=u_a, v_a=v_a,
                depth_q=torch.full((R,), 900, dtype=torch.int16, device=dev), u_b=u_b.float(), v_b=v_b.float(), cams=cams,
                keep=torch.ones(R, dtype=torch.uint8, device=dev),
                offsets=torch.arange(K + 1, device=dev, dtype=torch.int64) * per), per


def make_store(K, dev, seed=0):
    import torch
    from dcn_hip import frames
    rng = np.random.RandomState(seed)
    g = torch.Generator(device=dev).manual_seed(seed)
    rgb = torch.randint(0, 256, (K, H, W, 3), device=dev, generator=g, dtype=torch.uint8)
    depth = torch.full((K, H, W), 900, dtype=torch.int16, device=dev)
    depth[torch.rand((K, H, W), device=dev, generator=g) < 0.03] = 0
    mask = torch.zeros((K, H, W), dtype=torch.uint8, device=dev)
    mask[:, H // 5:4 * H // 5, W // 6:5 * W // 6] = 1
    store = frames.FrameStore.from_tensors(rgb, depth, mask, np.stack([np.eye(4)] * K), list(range(K + 1)), list(range(K)),
                                           scene_names=["scene_%d" % s for s in range(K)], frame_ids=[[0]] * K)
    ann = [{"scene_name": "scene_%d" % s, "image_idx": 0, "object_id": "object_%d" % s,
            "keypoints": {"kp_%d" % k: {"u": float(rng.uniform(0.2 * W, 0.8 * W)), "v": float(rng.uniform(0.25 * H, 0.75 * H))}
                          for k in range(KEYPOINTS)}} for s in range(K)]
    return store, ann


def bits(t):
    import torch
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def same(a, b):
    import torch
    return all(bool(torch.equal(bits(getattr(a, k)), bits(getattr(b, k))))
               for k in ("columns", "is_valid", "pred_uv", "closer", "row_pair", "mask_pixels", "status"))


def step(a):
    """One (D, part) step, in a process of its own: prints one JSON line"""
    import torch
    from crossscene_bench import PointwiseNetwork
    from dcn_hip import _lib, evaluate
    from frames_bench import event_us
    _lib.load()
    dev = torch.device("cuda", 0)
    D = a.dim
    out = {"D": D, "part": a.step, "machine": torch.cuda.get_device_name(0), "library": _lib.library_info()["version"], "sizes": []}
    for K in IMAGES:
        if a.step == "statistics":
            rows, per = make_rows(K, D, dev, seed=K + D)
            wide = lambda: evaluate.match_statistics_groups_wide(max_group_rows=per, **rows)
            groups = lambda: evaluate.match_statistics_groups(max_group_rows=per, **rows)
            tw, tg = wide(), groups()
            assert int(tw.status.cpu()[0]) == 0 and same(tw, tg), "the wide and the grouped entry differ"
            closer = float(tw.column("fraction_pixels_closer_than_ground_truth").mean())
            del tw, tg
            tm = {"wide": [], "groups": []}
            for _ in range(a.repeats):                         # the two alternate inside every repeat
                for k, fn in (("wide", wide), ("groups", groups)):
                    tm[k].append(event_us(fn, a.iters))
            med = {k: float(np.median(v)) for k, v in tm.items()}
            out["sizes"].append({"labelled_images": K, "rows_per_searched_image": per, "rows": K * per, "same_bits": True,
                                 "mean_fraction_closer_than_ground_truth": round(closer, 5),
                                 "wide_us": round(med["wide"], 1), "wide_us_all": [round(x, 1) for x in tm["wide"]],
                                 "groups_us": round(med["groups"], 1), "groups_us_all": [round(x, 1) for x in tm["groups"]],
                                 "groups_over_wide": round(med["groups"] / med["wide"], 2)})
            del rows
        else:
            store, ann = make_store(K, dev)
            net = PointwiseNetwork(D, dev)
            labels = evaluate.keypoint_labels(store, ann)
            table = evaluate.keypoint_rows(labels)
            run = lambda search: (lambda: evaluate.evaluate_keypoint_rows(net, store, labels, table, search=search))
            tw, tg = run("wide")(), run("groups")()
            assert int(tw.status.cpu()[0]) == 0 and same(tw, tg), "the chain's two searches differ"
            del tw, tg
            tm = {"wide": [], "groups": [], "default": []}
            for _ in range(a.repeats):
                for k, s in (("wide", "wide"), ("groups", "groups"), ("default", None)):
                    tm[k].append(event_us(run(s), max(1, a.iters // 2)))
            med = {k: float(np.median(v)) for k, v in tm.items()}
            out["sizes"].append({"labelled_images": K, "rows": int(table.shape[0]), "same_bits": True,
                                 "default_search": "wide" if table.shape[0] >= evaluate.WIDE_GROUP_MIN_ROWS * K else "groups",
                                 "chain_wide_us": round(med["wide"], 1), "chain_groups_us": round(med["groups"], 1),
                                 "chain_default_us": round(med["default"], 1),
                                 "chain_us_all": {k: [round(x, 1) for x in v] for k, v in tm.items()}})
            del store, net
        torch.cuda.empty_cache()
    print("KEYPOINT_BENCH " + json.dumps(out), flush=True)


def main():
    global IMAGES, KEYPOINTS
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[3, 16])
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, nargs="+", default=list(IMAGES), help="numbers of labelled images")
    ap.add_argument("--keypoints", type=int, default=KEYPOINTS, help="keypoints per image (fewer: the crossover sweep)")
    ap.add_argument("--parts", nargs="+", choices=("statistics", "chain"), default=["statistics", "chain"])
    ap.add_argument("--step", choices=("statistics", "chain"), default=None, help="(internal) run one step in this process")
    ap.add_argument("--dim", type=int, default=3)
    a = ap.parse_args()
    IMAGES, KEYPOINTS = tuple(a.images), a.keypoints
    if a.step:
        return step(a)
    res = {"shape": "%dx%d, K = %s labelled images x %d keypoints" % (W, H, list(IMAGES), KEYPOINTS), "repeats": a.repeats,
           "iters": a.iters, "steps": []}
    for D in a.dims:
        for part in a.parts:
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", part, "--dim",
                   str(D), "--repeats", str(a.repeats), "--iters", str(a.iters), "--keypoints", str(KEYPOINTS), "--images"] \
                + [str(k) for k in IMAGES]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            lines = [l for l in p.stdout.decode().splitlines() if l.startswith("KEYPOINT_BENCH ")]
            if p.returncode != 0 or not lines:                 # nothing more is started on the GPU after a failed step
                sys.stderr.write(p.stderr.decode()[-4000:])
                raise SystemExit("step %s D = %d failed (exit status %d)" % (part, D, p.returncode))
            res["steps"].append(json.loads(lines[-1][len("KEYPOINT_BENCH "):]))
    res["machine"], res["library"] = res["steps"][0]["machine"], res["steps"][0]["library"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
