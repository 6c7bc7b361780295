"""The data-parallel ``StoreTrainer`` (dcn_train_advance_ranks, dcn_train_log_ranks, ``FlatGradients(reduce="sum")``,
``gather_ranks``, ``StoreTrainer(gradients=...)``) through the C ABI with the kernels compiled for the host (tests/hostemu),
the ranks spawned as processes over gloo.  CPU only; the same checks (tests/train_ranks_common.py) run on the gfx950 build in
test_gpu_train_ranks.py.

The whole-loop tests use test_emu_train.py's 16 x 24 store, narrow Resnet18_8s and configuration, with the order-independent
loss backward: trainer and oracle must agree bit for bit."""
import numpy as np
import pytest
import torch

import train_common as tc
import train_ranks_common as rc
from helpers import use_emulation_library

H, W = 16, 24
N_ITERATIONS = 8
WORKER_LIMIT = 420               # seconds per spawned rank


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.fixture(autouse=True)
def exact(monkeypatch):
    from dcn_hip import loss as K
    monkeypatch.setattr(K, "EXACT_BACKWARD", True)


def make_store():
    """test_emu_train.store's recipe: object 0 has the scene ``moving`` and the scene ``still`` (every pair drawn there is
    empty), object 1 two moving scenes."""
    from dcn_hip import frames
    from test_emu_train import _pose
    rng = np.random.RandomState(0)
    moving = [_pose(t) for t in ([0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [0.25, 0.25, 0])]
    poses = moving + [_pose([0.1, 0, 0])] * 4 + moving + moving
    F = len(poses)
    depth = np.full((F, H, W), 900, np.uint16)
    depth[rng.rand(F, H, W) < 0.02] = 0
    mask = np.zeros((F, H, W), np.uint8)
    mask[:, H // 4:3 * H // 4, W // 6:5 * W // 6] = 1
    rgb = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    K = np.array([[10.0, 0.0, W / 2.0], [0.0, 10.0, H / 2.0], [0.0, 0.0, 1.0]])
    return frames.FrameStore.from_tensors(rgb, torch.from_numpy(depth.view(np.int16)), torch.from_numpy(mask), np.stack(poses),
                                          [0, 4, 8, 12, 16], [0, 0, 1, 1], K)


@pytest.fixture(scope="module")
def store(_lib):
    return make_store()


def _cfg():
    from test_emu_train import _cfg as cfg
    return cfg(True)                 # within-scene only, decay period 2


# ------------------------------------------------------------------------------------------------ T1, T2
def test_advance_ranks_equals_advance_on_the_flattened_types_and_numpy_weights():
    rc.check_advance_ranks("cpu")


def test_log_ranks_equals_log_on_the_flattened_batch():
    rc.check_log_ranks("cpu")


def test_rank_entries_refuse_bad_arguments():
    rc.check_advance_ranks_refusals("cpu")


def test_gather_ranks_without_a_group_is_a_copy():
    rc.check_gather_ranks_without_group("cpu")


# ------------------------------------------------------------------------------------------------ T3 - T5: spawned ranks
def _worker(rank, world, port, q, part, B, seeds, n, schedules, folder=None):
    import os
    os.environ["HIPEMU_THREADS"] = "2"
    torch.set_num_threads(2)
    rc.init_worker(rank, world, port, "gloo")
    use_emulation_library()
    from dcn_hip import loss as K
    K.EXACT_BACKWARD = True
    import torch.distributed as dist
    from test_emu_train import _make_dcn, _pcl
    st = make_store()
    if part == "loop":
        res = [rc.whole_loop_on_rank(_make_dcn, _pcl(), st, _cfg(), B, seeds[rank], n, t_b, o_b) for t_b, o_b in schedules]
    elif part == "run":
        import os
        res = rc.run_on_rank(_make_dcn, _pcl(), st, _cfg(), B, seeds[rank], rank, os.path.join(folder, "rank%d" % rank))
    else:
        res = rc.idle_rank_on_rank(_make_dcn, _pcl(), st, tc.still_store("cpu", H, W), _cfg(), _cfg(), B, seeds[0], n, rank)
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_equal_the_host_reading_loop_on_both_schedules(store):
    """Two ranks, B = 2, within scene only, 8 iterations, decay period 2: an all-empty iteration on a decay boundary, one rank
    empty, weights 1/3 and 2/3, full iterations.  Bit for bit with trainer and oracle both bucketed, and with both monolithic.

    Trainer bucketed against oracle MONOLITHIC is not compared here: at 16 x 24 the grouped ``forward_pair`` is unavailable
    (a group's rows are no multiple of the tile), the step has two backward calls, and the bucketed schedule then adds
    (b0 + b1) + (a0 + a1) where the monolithic one adds (b0 + a0) + (b1 + a1) -- another association of four summands, as
    test_gpu_ddp.py notes for ``two_calls_rel``; measured here, parameters, moments and batch-norm buffers of such a pairing
    differ in the last bits from the first iteration on while the ranks stay bit-equal to each other.  With ONE backward call
    per step a + b is commutative: that pairing is asserted bit for bit in test_gpu_train_ranks.py, where ``forward_pair`` is
    grouped."""
    B = 2
    seeds = rc.find_seeds(store, _cfg(), B, 2, N_ITERATIONS, lambda c: rc.pattern_two_ranks(c, B), first=(2, 3))
    both = rc.run_workers(_worker, 2, ("loop", B, seeds, N_ITERATIONS, ((True, True), (False, False))), WORKER_LIMIT)
    results = {rank: r[0] for rank, r in both.items()}
    counts = [list(c) for c in zip(*results[0]["counts"])]           # the oracle's own types: [rank][iteration]
    assert rc.pattern_two_ranks(counts, B), counts
    assert results[0]["counts"] == results[1]["counts"]
    weights = set(w for r in results.values() for w in r["weights"])
    assert float(np.float32(1.0 / 3.0)) in weights and float(np.float32(2.0 / 3.0)) in weights and 0.0 in weights, weights
    rc.assert_whole_loop(results, N_ITERATIONS, expect_bucketed=(True, True))
    assert results[0]["loss_column"] == results[1]["loss_column"]
    rc.assert_whole_loop({rank: r[1] for rank, r in both.items()}, N_ITERATIONS, expect_bucketed=(False, False))


@pytest.mark.timeout(900)
def test_three_ranks_equal_the_host_reading_loop(store):
    """Three ranks, B = 1: totals of 1, 2 and 3 non-empty pairs -- weights 1, 1/2 and 1/3.  Trainer and oracle both on the
    default schedule (bucketed: with three summands the association must be the same on both sides)."""
    seeds = rc.find_seeds(store, _cfg(), 1, 3, N_ITERATIONS, rc.pattern_three_ranks, first=(15, 16, 17))
    results = rc.run_workers(_worker, 3, ("loop", 1, seeds, N_ITERATIONS, ((None, None),)), WORKER_LIMIT)
    results = {rank: r[0] for rank, r in results.items()}
    counts = [list(c) for c in zip(*results[0]["counts"])]
    assert rc.pattern_three_ranks(counts), counts
    weights = set(w for r in results.values() for w in r["weights"])
    assert {1.0, 0.5, float(np.float32(1.0 / 3.0))} <= weights, weights
    rc.assert_whole_loop(results, N_ITERATIONS, expect_bucketed=(True, True))


@pytest.mark.timeout(900)
def test_an_idle_rank_changes_nothing(store):
    n = 4
    seed = tc.find_seed(store, _cfg(), 1, n, 2)
    results = rc.run_workers(_worker, 2, ("idle", 1, (seed, seed), n, ()), WORKER_LIMIT)
    rc.assert_idle_rank(results, n)


@pytest.mark.timeout(900)
def test_run_on_two_ranks_stops_together_and_only_the_save_rank_writes(store, tmp_path):
    results = rc.run_workers(_worker, 2, ("run", 1, (2, 3), 0, (), str(tmp_path)), WORKER_LIMIT)
    rc.assert_run(results)


# ------------------------------------------------------------------------------------------------ T6
def test_gradients_argument_refusals(store):
    from test_emu_train import _make_dcn, _pcl
    rc.check_refusals(_make_dcn, _pcl(), store, _cfg())


def test_without_a_process_group_the_gradients_trainer_is_the_plain_one(store, monkeypatch):
    from test_emu_train import _make_dcn, _pcl
    rc.check_no_process_group_equals_plain(_make_dcn, _pcl(), store, _cfg(), 1, 4, monkeypatch)
