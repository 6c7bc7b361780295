"""Training from a frame store with the decisions on the device (csrc/train_kernels.hip, dcn_hip.optim.GuardedAdam,
dcn_hip.train) through the C ABI -- kernels compiled for the host (tests/hostemu).  CPU only; the same checks
(tests/train_common.py) run on the gfx950 build in test_gpu_train.py.

The whole-loop tests use a narrow Resnet18_8s (base width 8) at 16 x 24 -- two 8 x 8 cells by three, the smallest size at
which the network's /8 map still has more than one row and column; the emulated backbone is thousands of times slower than the
device -- and a store of that size whose camera matrix is scaled with it, so that within-scene pairs of its moving scenes keep
matches and only the scene ``still`` gives empty pairs."""
import numpy as np
import pytest
import torch

import train_common as tc
from helpers import use_emulation_library

H, W = 16, 24


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.fixture(autouse=True)
def exact(monkeypatch):
    """The order-independent loss backward: two runs of the same step give the same bits."""
    from dcn_hip import loss as K
    monkeypatch.setattr(K, "EXACT_BACKWARD", True)


# ------------------------------------------------------------------------------------------------ T1 - T3, the log kernel
def test_guarded_adam_equals_adam_bit_for_bit_over_three_steps():
    tc.check_guarded_adam_three_steps("cpu")


def test_guarded_adam_inactive_step_changes_nothing():
    tc.check_guarded_adam_inactive_step("cpu")


def test_guarded_adam_state_dict_round_trips_through_torch_adam():
    tc.check_guarded_adam_state_dict_round_trip("cpu")


def test_guarded_copy_copies_with_the_matching_flag_only():
    tc.check_guarded_copy("cpu")


def test_advance_schedule_step_count_and_bias_corrections():
    tc.check_advance("cpu")


def test_log_rows_follow_the_pair_types():
    tc.check_log_rows("cpu")


# ------------------------------------------------------------------------------------------------ T4, T6
def _pose(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


@pytest.fixture(scope="module")
def store(_lib):
    """test_gpu_frames.training_store's recipe on the CPU at 16 x 24: object 0 has the scene ``moving`` and the scene ``still``
    (equal poses: every pair drawn there is empty), object 1 two moving scenes; a wall at 0.9 m, cameras 0.25 m apart in its
    plane, focal length 10 pixels (a shift of 2.8 pixels between two views)."""
    from dcn_hip import frames
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


def _make_dcn():
    from test_emu_step import FC_SCALE, _make
    dcn, o = _make(H=H, W=W)
    with torch.no_grad():   # (untrained descriptors are tiny: scaled so that both sides of the hinge occur)
        dcn.fcn.resnet18_8s.fc.weight.mul_(FC_SCALE)
    return dcn


def _pcl():
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    from oracle import synth
    return PixelwiseContrastiveLoss(image_shape=[H, W], config=synth.LOSS_CONFIG)


def _cfg(within_only):
    return tc.training_config(within_only=within_only, attempts=200, non_matches=4, cross=40)


def test_whole_loop_equals_the_host_reading_loop_batch_of_one(store):
    tr, o = tc.check_whole_loop(_make_dcn, _pcl(), store, _cfg(True), 1)
    assert len(o["log"]["train"]["match_loss"]) == len(o["log"]["train"]["learning_rate"]) > 0


def test_whole_loop_equals_the_host_reading_loop_mixed_batch_of_two(store):
    tc.check_whole_loop(_make_dcn, _pcl(), store, _cfg(False), 2, mixed=True)


def test_save_point_files_and_restart(store, tmp_path):
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    tc.check_save_point(_make_dcn, _pcl(), store, _cfg(True), 1, tmp_path, DenseCorrespondenceNetwork.from_model_folder,
                        expect_match_loss=True)


# ------------------------------------------------------------------------------------------------ T7
def test_guarded_adam_refuses_more_than_one_parameter_group():
    from dcn_hip.optim import GuardedAdam
    a, b = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="one parameter group"):
        GuardedAdam([{"params": [a]}, {"params": [b]}])
    o = GuardedAdam([a])
    with pytest.raises(ValueError, match="one parameter group"):
        o.add_param_group({"params": [b]})


def test_guarded_adam_refuses_loaded_steps_that_differ():
    from dcn_hip.optim import Adam, GuardedAdam
    ps = [torch.nn.Parameter(torch.ones(5)), torch.nn.Parameter(torch.ones(3))]
    src = Adam(ps, lr=1e-3)
    for p in ps:
        p.grad = torch.ones_like(p)
    src.step()
    ps[1].grad = None
    src.step()                                   # steps 2 and 1
    with pytest.raises(ValueError, match="steps differ"):
        GuardedAdam(ps, lr=1e-3).load_state_dict(src.state_dict())
    ps[1].grad = torch.ones(3)
    ps[0].grad = None
    src.step()                                   # 2 and 2
    o = GuardedAdam(ps, lr=1e-3)
    o.load_state_dict(src.state_dict())
    state = tc.make_state("cpu", lr=5.0)
    o.bind(state)
    assert state.read_step_and_lr() == (2, 1e-3)


def test_guarded_adam_step_needs_a_state_and_every_gradient():
    from dcn_hip.optim import GuardedAdam
    ps = [torch.nn.Parameter(torch.ones(5)), torch.nn.Parameter(torch.ones(3))]
    o = GuardedAdam(ps, lr=1e-3)
    with pytest.raises(TypeError):
        o.step()
    ps[0].grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="no gradient"):
        o.step(tc.make_state("cpu"))
    with pytest.raises(ValueError, match="betas"):
        GuardedAdam(ps, lr=1e-3, betas=(0.8, 0.999)).bind(tc.make_state("cpu"))


def test_trainer_refuses_attached_distributed_gradients(store):
    from dcn_hip.distributed import FlatGradients
    from dcn_hip.optim import GuardedAdam
    from dcn_hip.train import StoreTrainer
    dcn = _make_dcn()
    opt = FlatGradients(dcn).attach(GuardedAdam(dcn.parameters(), lr=1e-4))
    with pytest.raises(NotImplementedError, match="distributed"):
        StoreTrainer(dcn, _pcl(), store, _cfg(True), optimizer=opt)
    with pytest.raises(TypeError, match="GuardedAdam"):
        StoreTrainer(_make_dcn(), _pcl(), store, _cfg(True), optimizer=torch.optim.Adam(_make_dcn().parameters()))


def test_types_of_the_wrong_dtype_or_device_are_refused():
    state = tc.make_state("cpu")
    with pytest.raises(TypeError, match="int32"):
        state.advance(torch.zeros(2, dtype=torch.int64), 1)
    with pytest.raises(ValueError, match="is on"):
        state.advance(torch.zeros(2, dtype=torch.int32, device="meta"), 1)
    with pytest.raises(TypeError, match="int32"):
        state.log(1, torch.zeros(1), torch.zeros(2, 5), [0, 0])
    with pytest.raises(ValueError):
        state.log(1, torch.zeros(1), torch.zeros(3, 5), torch.zeros(2, dtype=torch.int32))
    assert state.rows == 0 and state.read().num_active == 0
