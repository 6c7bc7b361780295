#!/usr/bin/env python3
"""Times a whole training iteration fed from a frame store -- data, step, schedule and logging together -- and the guarded
Adam kernel (csrc/train_kernels.hip) against dcn_adam_step.

Fixed settings: a synthetic store at 640 x 480 (synthetic_bench's recipe: 4 objects x 2 scenes x 30 frames), Resnet34_8s,
D = 3, B = 1 and B = 4, within-scene / across-scene / different-object pairs 2 : 1 : 1 with training.yaml's counts.

Part ``loops``: three loops on the same draws (same seeds), interleaved window by window in one process:

  (1) trainer     ``dcn_hip.train.StoreTrainer.iteration``: the skip decision, the schedule and the log on the device;
  (2) unguarded   the loop INTEGRATION.md prints under "Drawing batches from a frame store" (dcn_hip.optim.Adam, no guard);
  (3) host_reads  that loop made reference-faithful the only way there was: ``if int(num_valid) == 0: continue`` and the
                  reference's five ``.item()`` logging reads (training.py:353-413).

Part ``adam``: dcn_adam_step_guarded against dcn_adam_step on the model's own tensors, alone in its process, the two kernels
interleaved window by window.  Accepted when the guarded kernel's median exceeds dcn_adam_step's by no more than the
max - min spread of dcn_adam_step's own windows.

Device events around windows of back-to-back calls and the wall clock around the same windows (ending in a synchronize); 5
windows each, medians and max - min spreads.  Each part runs in a fresh child process.

    python tools/train_bench.py [--out profiles/train_bench.json]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

H, W, D = 480, 640, 3
WINDOWS, CALLS, ADAM_CALLS = 5, 5, 20
CFG = {"training": {"num_matching_attempts": 10000, "sample_matches_only_off_mask": True, "num_non_matches_per_match": 150,
                    "fraction_masked_non_matches": 0.5, "fraction_background_non_matches": 0.5,
                    "cross_scene_num_samples": 10000, "use_image_b_mask_inv": True, "domain_randomize": False,
                    "data_type_probabilities": {"SINGLE_OBJECT_WITHIN_SCENE": 2.0, "SINGLE_OBJECT_ACROSS_SCENE": 1.0,
                                                "DIFFERENT_OBJECT": 1.0, "MULTI_OBJECT": 0.0, "SYNTHETIC_MULTI_OBJECT": 0.0},
                    "learning_rate": 1.0e-4, "learning_rate_decay": 0.9, "steps_between_learning_rate_decay": 250,
                    "weight_decay": 1.0e-4, "num_iterations": 3500, "batch_size": 1, "logging_rate": 100, "save_rate": 500}}


def build_dcn():
    import torch
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    torch.manual_seed(0)
    cfg = {"descriptor_dimension": D, "image_width": W, "image_height": H,
           "backbone": {"model_class": "Resnet", "resnet_name": "Resnet34_8s"}}
    return DenseCorrespondenceNetwork.from_config(cfg, load_stored_params=False)


def window(fn, calls):
    """-> (device microseconds, wall-clock microseconds) per call of one window"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls, (time.perf_counter() - t0) * 1e6 / calls


def summary(samples):
    dev, wall = [s[0] for s in samples], [s[1] for s in samples]
    r = lambda v: round(float(v), 1)
    return {"device_us": r(np.median(dev)), "device_spread_us": r(max(dev) - min(dev)), "device_windows_us": [r(x) for x in dev],
            "wall_us": r(np.median(wall)), "wall_spread_us": r(max(wall) - min(wall)), "wall_windows_us": [r(x) for x in wall]}


# ------------------------------------------------------------------------------------------------ the three loops
def make_loops(store, B):
    import torch
    from dcn_hip import frames
    from dcn_hip.optim import Adam
    from dcn_hip.train import StoreTrainer
    from dense_correspondence.loss_functions import loss_composer
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    dev = store.device
    t = CFG["training"]
    rngs = lambda: (torch.Generator(device=dev).manual_seed(3), np.random.RandomState(3))
    from bench import LOSS_CONFIG                      # (training.yaml's loss_function section, as bench.py keeps it)
    pcl = lambda: PixelwiseContrastiveLoss(image_shape=[H, W], config=LOSS_CONFIG)
    g1, h1 = rngs()
    trainer = StoreTrainer(build_dcn(), pcl(), store, CFG, generator=g1, host_rng=h1, batch_size=B)
    it1 = [0]

    def loop_trainer():
        it1[0] += 1
        trainer.iteration(it1[0])

    def plain(host_reads):
        dcn, p = build_dcn(), pcl()
        opt = Adam(dcn.parameters(), lr=t["learning_rate"], weight_decay=t["weight_decay"])
        g, host = rngs()
        skipped = [0]

        def step():
            s, _, _ = frames.draw_training_batch(store, B, CFG, generator=g, host_rng=host, per_pair_types=True)
            ya, yb = dcn.forward_pair(s.input_a, s.input_b)
            loss, terms, _, num_valid = loss_composer.get_loss_mixed(p, dcn.process_network_output(ya, B),
                                                                     dcn.process_network_output(yb, B), s.device_lists())
            if host_reads and int(num_valid) == 0:
                skipped[0] += 1
                return
            opt.zero_grad()
            loss.backward()
            opt.step()
            if host_reads:   # update_plots: loss, match, masked, background and blind non-match loss, one .item() each
                mean = terms.mean(0)
                return [loss.item()] + [mean[k].item() for k in (1, 2, 3, 4)]
        return step, skipped
    loop_unguarded, _ = plain(False)
    loop_host, skipped = plain(True)
    return trainer, {"trainer": loop_trainer, "unguarded": loop_unguarded, "host_reads": loop_host}, skipped


def part_loops():
    import torch
    from synthetic_bench import make_store
    dev = torch.device("cuda", 0)
    store = make_store(dev)
    runs = []
    for B in (1, 4):
        trainer, loops, skipped = make_loops(store, B)
        for fn in loops.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in loops}
        for _ in range(WINDOWS):
            for k, fn in loops.items():
                samples[k].append(window(fn, CALLS))
        snap = trainer.state.read()
        res = {"B": B, "iterations_timed_per_loop": WINDOWS * CALLS, "trainer_active": snap.num_active,
               "trainer_skipped": snap.num_skipped, "host_reads_skipped": skipped[0]}
        for k in loops:
            res[k] = summary(samples[k])
        res["trainer_minus_unguarded_device_us"] = round(res["trainer"]["device_us"] - res["unguarded"]["device_us"], 1)
        res["trainer_minus_unguarded_wall_us"] = round(res["trainer"]["wall_us"] - res["unguarded"]["wall_us"], 1)
        res["host_reads_minus_trainer_wall_us"] = round(res["host_reads"]["wall_us"] - res["trainer"]["wall_us"], 1)
        runs.append(res)
        del trainer, loops
        torch.cuda.empty_cache()
    return {"shape": "%dx%d, Resnet34_8s, D = %d, synthetic store (8 scenes x 30 frames, 4 objects), within : across : "
                     "different = 2 : 1 : 1, medians of %d windows of %d iterations, loops interleaved" % (W, H, D, WINDOWS, CALLS),
            "runs": runs}


# ------------------------------------------------------------------------------------------------ the Adam kernels
def part_adam():
    import torch
    from dcn_hip import _lib
    from dcn_hip.train import TrainState
    lib = _lib.get()
    dcn = build_dcn()
    ps = [p for p in dcn.parameters()]
    g = torch.Generator(device="cuda").manual_seed(1)
    mk = lambda p, scale: torch.empty_like(p, memory_format=torch.preserve_format).copy_(
        torch.randn(p.shape, device="cuda", generator=g) * scale)
    cols = [ps, [mk(p, 1e-2) for p in ps], [mk(p, 1e-3) for p in ps], [mk(p, 1e-3).abs_() for p in ps]]
    n = len(ps)
    tabs = [(ctypes.c_void_p * n)(*[x.data_ptr() for x in col]) for col in cols]
    numel = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
    state = TrainState("cuda", 1.0e-4, 250, 0.9)
    active, empty = (torch.tensor([v], dtype=torch.int32, device="cuda") for v in (0, -1))
    state.advance(active, 1)
    sp = ctypes.c_void_p(state.state_ptr())
    st = _lib.stream_ptr()

    def plain():
        _lib.check(lib.dcn_adam_step(n, tabs[0], tabs[1], tabs[2], tabs[3], numel, 1.0e-4, 0.9, 0.999, 1e-8, 1.0e-4, 1, st), "adam")

    def guarded():
        _lib.check(lib.dcn_adam_step_guarded(n, tabs[0], tabs[1], tabs[2], tabs[3], numel, 1e-8, 1.0e-4, 0.9, 0.999, sp, st),
                   "guarded")
    for fn in (plain, guarded):
        for _ in range(10):
            fn()
    samples = {"dcn_adam_step": [], "dcn_adam_step_guarded": []}
    for _ in range(WINDOWS):
        samples["dcn_adam_step"].append(window(plain, ADAM_CALLS))
        samples["dcn_adam_step_guarded"].append(window(guarded, ADAM_CALLS))
    state.advance(empty, 2)
    inactive = [window(guarded, ADAM_CALLS) for _ in range(WINDOWS)]
    res = {k: summary(v) for k, v in samples.items()}
    res["dcn_adam_step_guarded_inactive"] = summary(inactive)
    elements = sum(p.numel() for p in ps)
    res["elements"], res["bytes_per_call"] = elements, 28 * elements
    res["dcn_adam_step_GBps"] = round(28 * elements / res["dcn_adam_step"]["device_us"] * 1e-3, 1)
    res["dcn_adam_step_guarded_GBps"] = round(28 * elements / res["dcn_adam_step_guarded"]["device_us"] * 1e-3, 1)
    res["accepted"] = bool(res["dcn_adam_step_guarded"]["device_us"] - res["dcn_adam_step"]["device_us"]
                           <= res["dcn_adam_step"]["device_spread_us"])
    res["shape"] = "Resnet34_8s D = %d: %d tensors, medians of %d windows of %d calls, kernels interleaved" % (D, n, WINDOWS, ADAM_CALLS)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=("all", "adam", "loops"), default="all")
    a = ap.parse_args()
    if a.part == "all":      # each part in a fresh child process of its own
        res = {}
        for part in ("adam", "loops"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part], stdout=subprocess.PIPE, check=True)
            res[part] = json.loads(out.stdout.decode().strip().split("\n")[-1])
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("train_bench: no GPU (a time measured anywhere else says nothing about the MI355X)")
        from dcn_hip import _lib
        _lib.load()
        res = part_adam() if a.part == "adam" else part_loops()
        res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
