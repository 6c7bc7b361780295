"""Validation while training from a frame store (dcn_hip.train.Validation) on the MI355X: ``test_gpu_frames.training_store(h=64,
w=128)`` for training as in test_gpu_train.py (within-scene pairs are empty at that size, the other two types count), a second
synthetic store for validation, the real Resnet34_8s, the order-independent loss backward.  V1 - V6 of
tests/validation_common.py, and no host read over trainer iterations with a validation pass among them."""
import warnings

import numpy as np
import pytest
import torch

import evaluate_common as ec
import train_common as tc
import validation_common as vc
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


@pytest.fixture(scope="module")
def store(_lib):
    from test_gpu_frames import training_store
    return training_store(h=H, w=W)


@pytest.fixture(scope="module")
def vstore(_lib):
    return ec.synthetic_store("cuda", H, W, seed=5)


def _make_dcn(h=H, w=W):
    import parity_common as pc
    return pc.build_dcn("Resnet34_8s", D, h, w)[0]


def _pcl(h=H, w=W):
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    from oracle import synth
    return PixelwiseContrastiveLoss(image_shape=[h, w], config=synth.LOSS_CONFIG)


def _cfg(within_only=False):
    return tc.training_config(within_only=within_only)


def test_training_with_validation_is_the_same_run(store, vstore):
    vc.check_training_is_the_same_run(_make_dcn, _pcl(), store, vstore, _cfg(), 1, True)


def test_validation_row_equals_the_pass_run_by_hand(store, vstore):
    vc.check_row_equals_the_pass_by_hand(_make_dcn, _pcl(), store, vstore, _cfg(), 1, True)


def test_iterations_with_a_validation_pass_never_synchronize(store, vstore):
    """V3: a warm-up iteration and pass, then three trainer iterations, the middle one followed by a validation pass, under
    torch's sync debug mode (or, where the runtime does not honour it, with no device-to-host copy in the profile)."""
    from test_gpu_frames import _d2h_copies
    from test_gpu_train import _sync_mode_honoured
    val = vc.make_validation(vstore, 4, rate=1, after=0)
    tr = vc.trainer(_make_dcn, _pcl(), store, _cfg(), 1, 11, validation=val)
    tr.dcn.train()
    it = [0]

    def three():
        for k in range(3):
            it[0] += 1
            tr.iteration(it[0])
            if k == 1:
                tr.validate(it[0])
    tr.iteration(1)
    tr.validate(1)
    it[0] = 1
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
    tr.read_log()
    assert tr.validation_history[:, 0].tolist() == [1, 3] and tr.dcn.training
    assert np.isfinite(tr.validation_history[:, vc.VALIDATION_HEAD + 6]).all()


def test_inactive_iteration_is_validated_and_left_out_of_the_log(store, vstore):
    vc.check_inactive_iteration(_make_dcn, _pcl(), store, vstore, _cfg(), _cfg(True), 1, H, W, True)


def test_save_point_carries_the_validation_key(store, vstore, tmp_path):
    vc.check_save_point(_make_dcn, _pcl(), store, vstore, _cfg(), 1, tmp_path)


def test_schedule_and_arguments(store, vstore):
    vc.check_schedule_and_arguments(_make_dcn, _pcl(), store, vstore, ec.synthetic_store("cuda", 32, 128), _cfg())
