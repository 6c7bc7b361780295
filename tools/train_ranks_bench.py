#!/usr/bin/env python3
"""What the data-parallel ``StoreTrainer`` (``gradients=``) adds to an iteration on ONE MI355X: the two small gathers, the
multiply of the loss with the rank's weight, and the flat gradient buffer with its bucketed reduction on the communication
stream -- over a one-rank ``nccl`` group with ``single_rank_collectives=True``, so that every collective is really issued.

train_bench.py's settings (synthetic store at 640 x 480, Resnet34_8s, D = 3, B = 1 and B = 4, within : across : different =
2 : 1 : 1).  Two loops on the same draws (same seeds), interleaved window by window in one process:

  (1) plain   ``StoreTrainer.iteration`` as on one GPU;
  (2) ranks   ``StoreTrainer(gradients=FlatGradients(dcn, reduce="sum", bucketed=True, single_rank_collectives=True))``.

Device events and the wall clock around windows of back-to-back iterations; medians of 5 windows of 5 iterations and the
max - min of each loop's windows.  A number for several GPUs cannot come from one device: RCCL refuses two ranks on it.

    python tools/train_ranks_bench.py [--out profiles/train_ranks_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from train_bench import CALLS, CFG, D, H, W, WINDOWS, build_dcn, summary, window  # noqa: E402


def make_loops(store, B):
    import torch
    from bench import LOSS_CONFIG
    from dcn_hip.distributed import FlatGradients
    from dcn_hip.optim import GuardedAdam
    from dcn_hip.train import StoreTrainer
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    dev = store.device
    t = CFG["training"]
    rngs = lambda: (torch.Generator(device=dev).manual_seed(3), np.random.RandomState(3))
    pcl = lambda: PixelwiseContrastiveLoss(image_shape=[H, W], config=LOSS_CONFIG)
    g1, h1 = rngs()
    plain = StoreTrainer(build_dcn(), pcl(), store, CFG, generator=g1, host_rng=h1, batch_size=B)
    g2, h2 = rngs()
    dcn = build_dcn()
    grads = FlatGradients(dcn, reduce="sum", bucketed=True, single_rank_collectives=True)
    opt = grads.attach(GuardedAdam(dcn.parameters(), lr=t["learning_rate"], weight_decay=t["weight_decay"]))
    ranks = StoreTrainer(dcn, pcl(), store, CFG, optimizer=opt, gradients=grads, generator=g2, host_rng=h2, batch_size=B)
    its = {"plain": 0, "ranks": 0}

    def loop(name, trainer):
        def fn():
            its[name] += 1
            trainer.iteration(its[name])
        return fn
    return {"plain": plain, "ranks": ranks}, {"plain": loop("plain", plain), "ranks": loop("ranks", ranks)}


def run():
    import torch
    import torch.distributed as dist
    from synthetic_bench import make_store
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29513")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    store = make_store(dev)
    runs = []
    for B in (1, 4):
        trainers, loops = make_loops(store, B)
        for fn in loops.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in loops}
        for _ in range(WINDOWS):
            for k, fn in loops.items():
                samples[k].append(window(fn, CALLS))
        res = {"B": B, "iterations_timed_per_loop": WINDOWS * CALLS}
        for k in loops:
            snap = trainers[k].state.read()
            res[k] = summary(samples[k])
            res[k + "_active"], res[k + "_skipped"] = snap.num_active, snap.num_skipped
        res["ranks_minus_plain_device_us"] = round(res["ranks"]["device_us"] - res["plain"]["device_us"], 1)
        res["ranks_minus_plain_wall_us"] = round(res["ranks"]["wall_us"] - res["plain"]["wall_us"], 1)
        res["collectives"] = dict(trainers["ranks"].gradients.stats)
        runs.append(res)
        del trainers, loops
        torch.cuda.empty_cache()
    dist.destroy_process_group()
    return {"shape": "%dx%d, Resnet34_8s, D = %d, synthetic store (8 scenes x 30 frames, 4 objects), within : across : different "
                     "= 2 : 1 : 1, one-rank nccl group with single_rank_collectives, medians of %d windows of %d iterations, "
                     "loops interleaved" % (W, H, D, WINDOWS, CALLS),
            "per_iteration": "2 all_gather (types: 4 B bytes, log row: 4 + 20 B bytes), 1 all_reduce per gradient bucket; "
                             "launches besides the plain trainer's: 1 multiply, 1 concatenation, the buckets' adds",
            "runs": runs, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_ranks_bench: no GPU (a time measured anywhere else says nothing about the MI355X)")
    from dcn_hip import _lib
    _lib.load()
    line = json.dumps(run())
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
