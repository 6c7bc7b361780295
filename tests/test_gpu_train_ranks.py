"""The data-parallel ``StoreTrainer`` (dcn_train_advance_ranks, dcn_train_log_ranks, ``FlatGradients(reduce="sum")``,
``gather_ranks``, ``StoreTrainer(gradients=...)``) on the MI355X: the checks of tests/train_ranks_common.py on the gfx950
build; the whole loop with the real Resnet34_8s at 64 x 128 on two ranks that share the one device over gloo (RCCL refuses two
ranks on one device), trainer bucketed against a host-reading monolithic oracle, bit for bit; an idle rank; and whole
iterations over a one-rank RCCL group with no host read.

As in test_gpu_train.py, at 64 x 128 a within-scene pair of ``training_store`` is empty and the other two types count."""
import warnings

import numpy as np
import pytest
import torch

import train_common as tc
import train_ranks_common as rc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu

H, W, D = 64, 128, 3
N_ITERATIONS = 8
WORKER_LIMIT = 240               # seconds per spawned rank


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


# ------------------------------------------------------------------------------------------------ T1, T2 in process
def test_advance_ranks_equals_advance_on_the_flattened_types_and_numpy_weights():
    rc.check_advance_ranks("cuda")


def test_log_ranks_equals_log_on_the_flattened_batch():
    rc.check_log_ranks("cuda")


def test_rank_entries_refuse_bad_arguments():
    rc.check_advance_ranks_refusals("cuda")


def test_gather_ranks_without_a_group_is_a_copy():
    rc.check_gather_ranks_without_group("cuda")


# ------------------------------------------------------------------------------------------------ spawned ranks
def _cfg():
    return tc.training_config(within_only=False)


def _start(rank, world, port, backend):
    """What every spawned rank does first: the device, the process group, the gfx950 library, the exact loss backward, and the
    grouped ``forward_pair`` or an error."""
    torch.cuda.set_device(0)
    if backend == "nccl":
        rc.init_worker(rank, world, port, backend, device_id=torch.device("cuda", 0))
    else:
        rc.init_worker(rank, world, port, backend)
    use_gfx950_library()
    from dcn_hip import loss as K
    K.EXACT_BACKWARD = True
    warnings.filterwarnings("error", message="forward_pair: grouped launch unavailable")


def _two_rank_worker(rank, world, port, q, B, seeds, idle_seed, idle_n):
    import torch.distributed as dist
    _start(rank, world, port, "gloo")
    from test_gpu_frames import training_store
    from test_gpu_train import _make_dcn, _pcl
    store = training_store(h=H, w=W)
    loop = rc.whole_loop_on_rank(_make_dcn, _pcl(), store, _cfg(), B, seeds[rank], N_ITERATIONS, True, False)
    idle = rc.idle_rank_on_rank(_make_dcn, _pcl(), store, tc.still_store("cuda", H, W), _cfg(),
                                tc.training_config(within_only=True), 1, idle_seed, idle_n, rank)
    torch.cuda.synchronize()
    q.put((rank, {"loop": loop, "idle": idle}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_on_one_device_equal_the_host_reading_loop_and_an_idle_rank_changes_nothing():
    """Two ranks, B = 2, all three single-object types, 8 iterations, decay period 2.  Seeds searched by drawing only: an
    all-empty iteration on a decay boundary and an active one on another, one rank empty, unequal counts, a full iteration.
    The trainer reduces bucket by bucket, the oracle with one all-reduce: one backward call per step (the grouped
    ``forward_pair``) and two ranks, so every sum has two summands and the bits must agree.  Then, in the same processes,
    rank 1 draws from a store that is always empty: rank 0 is the single-process trainer on its draws."""
    from test_gpu_frames import training_store
    B, idle_n = 2, 4
    store = training_store(h=H, w=W)
    seeds = rc.find_seeds(store, _cfg(), B, 2, N_ITERATIONS, lambda c: rc.pattern_two_ranks(c, B), first=(2, 3))
    idle_seed = tc.find_seed(store, _cfg(), 1, idle_n, 2)
    del store
    results = rc.run_workers(_two_rank_worker, 2, (B, seeds, idle_seed, idle_n), WORKER_LIMIT)
    loop = {rank: r["loop"] for rank, r in results.items()}
    counts = [list(c) for c in zip(*loop[0]["counts"])]
    assert rc.pattern_two_ranks(counts, B), counts
    assert loop[0]["counts"] == loop[1]["counts"]
    rc.assert_whole_loop(loop, N_ITERATIONS, expect_bucketed=(True, False))
    for r in loop.values():          # one backward call per active iteration: the grouped forward_pair
        assert r["trainer_stats"]["bucketed_steps"] == N_ITERATIONS, r["trainer_stats"]
    assert loop[0]["loss_column"] == loop[1]["loss_column"]
    rc.assert_idle_rank({rank: r["idle"] for rank, r in results.items()}, idle_n)


# ------------------------------------------------------------------------------------------------ no synchronisation
def _sync_mode_honoured():
    try:
        torch.zeros(1, device="cuda").item()
        return False
    except RuntimeError:
        return True


def _one_rank_rccl_worker(rank, world, port, q):
    import torch.distributed as dist
    _start(rank, world, port, "nccl")
    from dcn_hip import frames
    from test_gpu_frames import _d2h_copies, training_store
    from test_gpu_train import _make_dcn, _pcl
    store, still = training_store(h=H, w=W), tc.still_store("cuda", H, W)
    cfg, within = _cfg(), tc.training_config(within_only=True)
    issued = {"gathers": 0}
    inner = dist.all_gather_into_tensor

    def counted(*a, **k):
        issued["gathers"] += 1
        return inner(*a, **k)
    dist.all_gather_into_tensor = counted
    tr = rc.make_ranks_trainer(_make_dcn(), _pcl(), store, cfg, 1, 11, True, single_rank_collectives=True)
    g, host = tr.generator, tr.host_rng
    it = [0]

    def empty_iteration():
        sb = frames.draw_training_batch(still, 1, within, generator=g, host_rng=host, per_pair_types=True)[0]
        it[0] += 1
        tr.step_on_batch(sb, it[0])

    def three():
        for k in range(3):
            if k == 1:
                empty_iteration()
            else:
                it[0] += 1
                tr.iteration(it[0])
    tr.iteration(1)
    it[0] = 1
    empty_iteration()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = _sync_mode_honoured()
        if honoured:
            three()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    d2h = []
    if not honoured:
        d2h = _d2h_copies(three)
    torch.cuda.synchronize()
    snap = tr.read_log()
    q.put((rank, {"honoured": honoured, "d2h": d2h, "rows": [[float(x) for x in r] for r in snap.history],
                  "num_active": snap.num_active, "num_skipped": snap.num_skipped, "t": snap.t, "gathers": issued["gathers"],
                  "stats": dict(tr.gradients.stats), "finite": bool(torch.isfinite(tr.last[0])), "world": tr.world}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_trainer_iterations_over_a_one_rank_rccl_group_never_synchronize():
    """In a child process with a one-rank ``nccl`` group and ``single_rank_collectives=True`` (every collective is issued):
    two warm-up iterations, then three whole trainer iterations -- the middle one on a batch known to be empty -- under torch's
    sync debug mode, or with no device-to-host copy in the profile where the runtime does not honour it."""
    r = rc.run_workers(_one_rank_rccl_worker, 1, (), WORKER_LIMIT)[0]
    assert r["d2h"] == [], r
    rows = {int(x[0]): x for x in r["rows"]}
    assert sorted(rows) == [1, 2, 3, 4, 5] and rows[2][1] == 0 and rows[4][1] == 0, r
    assert r["num_skipped"] >= 2 and r["num_active"] + r["num_skipped"] == 5 and r["t"] == r["num_active"], r
    assert r["finite"] and r["world"] == 1
    assert r["gathers"] == 2 * 5, r                    # the types and the log row of every iteration, empty or not
    assert r["stats"]["bucketed_steps"] == 5 and r["stats"]["bucket_collectives"] > 0 and r["stats"]["monolithic_steps"] == 0, r
