"""Training from a frame store with the decisions on the device (csrc/train_kernels.hip, dcn_hip.optim.GuardedAdam,
dcn_hip.train) on the MI355X: the checks of tests/train_common.py on the gfx950 build, the whole loop with the real
Resnet34_8s against a loop that reads the types on the host, no host read over whole trainer iterations, and the save point.

The whole-loop tests draw from ``test_gpu_frames.training_store(h=64, w=128)`` (B = 1 at 64 x 128 gives 128 output rows: the
grouped ``forward_pair``, not its fallback) with within-scene, across-scene and different-object pairs.  At that size the
store's default camera matrix moves a point by more than the image between two views of a moving scene, so a within-scene pair
is empty whether it is drawn from ``still`` or not: the empty iterations are the within-scene draws, the active ones the other
two types.  Within-scene pairs that count run through the save-point test, at 640 x 480."""
import warnings

import numpy as np
import pytest
import torch

import train_common as tc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu

H, W, D = 64, 128, 3


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.fixture(autouse=True)
def exact(monkeypatch):
    """The order-independent loss backward: two runs of the same step give the same bits."""
    from dcn_hip import loss as K
    monkeypatch.setattr(K, "EXACT_BACKWARD", True)


@pytest.fixture(autouse=True)
def grouped_forward_pair():
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="forward_pair: grouped launch unavailable")
        yield


# ------------------------------------------------------------------------------------------------ T1 - T3, the log kernel
def test_guarded_adam_equals_adam_bit_for_bit_over_three_steps():
    tc.check_guarded_adam_three_steps("cuda")


def test_guarded_adam_inactive_step_changes_nothing():
    tc.check_guarded_adam_inactive_step("cuda")


def test_guarded_adam_state_dict_round_trips_through_torch_adam():
    tc.check_guarded_adam_state_dict_round_trip("cuda")


def test_guarded_copy_copies_with_the_matching_flag_only():
    tc.check_guarded_copy("cuda")


def test_advance_schedule_step_count_and_bias_corrections():
    tc.check_advance("cuda")


def test_log_rows_follow_the_pair_types():
    tc.check_log_rows("cuda")


# ------------------------------------------------------------------------------------------------ T4
@pytest.fixture(scope="module")
def store(_lib):
    from test_gpu_frames import training_store
    return training_store(h=H, w=W)


def _make_dcn(h=H, w=W):
    import parity_common as pc
    return pc.build_dcn("Resnet34_8s", D, h, w)[0]


def _pcl(h=H, w=W):
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    from oracle import synth
    return PixelwiseContrastiveLoss(image_shape=[h, w], config=synth.LOSS_CONFIG)


@pytest.mark.parametrize("B", [1, 2])
def test_whole_loop_equals_the_host_reading_loop(store, B):
    tc.check_whole_loop(_make_dcn, _pcl(), store, tc.training_config(within_only=False), B, mixed=True)


# ------------------------------------------------------------------------------------------------ T5
def _sync_mode_honoured():
    try:
        torch.zeros(1, device="cuda").item()
        return False
    except RuntimeError:
        return True


def test_trainer_iterations_never_synchronize(store):
    """Two warm-up iterations, then three whole trainer iterations -- the middle one on a batch drawn from a store whose every
    scene is ``still``: known to be empty -- under torch's sync debug mode (or, where the runtime does not honour it, with no
    device-to-host copy in the profile)."""
    from dcn_hip import frames
    from dcn_hip.train import StoreTrainer
    from test_gpu_frames import _d2h_copies
    still = tc.still_store("cuda", H, W)
    cfg, within = tc.training_config(within_only=False), tc.training_config(within_only=True)
    g = torch.Generator(device="cuda").manual_seed(11)
    host = np.random.RandomState(11)
    tr = StoreTrainer(_make_dcn(), _pcl(), store, cfg, generator=g, host_rng=host, batch_size=1)
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
    if not honoured:
        assert _d2h_copies(three) == []
    torch.cuda.synchronize()
    snap = tr.read_log()
    rows = {int(r[0]): r for r in snap.history}
    assert sorted(rows) == [1, 2, 3, 4, 5] and rows[2][1] == 0 and rows[4][1] == 0
    assert snap.num_skipped >= 2 and snap.num_active + snap.num_skipped == 5 and snap.t == snap.num_active
    assert bool(torch.isfinite(tr.last[0]))


# ------------------------------------------------------------------------------------------------ T6
def test_save_point_files_and_restart(tmp_path):
    """At 640 x 480 with within-scene pairs only: the pairs of the moving scenes count, those of ``still`` are empty."""
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    from test_gpu_frames import training_store
    h, w = 480, 640
    tc.check_save_point(lambda: _make_dcn(h, w), _pcl(h, w), training_store(), tc.training_config(within_only=True), 1, tmp_path,
                        DenseCorrespondenceNetwork.from_model_folder, expect_match_loss=True)
