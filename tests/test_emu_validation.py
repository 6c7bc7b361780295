"""Validation while training from a frame store (dcn_hip.train.Validation) through the host-emulation build: the narrow
Resnet18_8s and the 16 x 24 store of test_emu_train.py for training, a second synthetic store of that size for validation.
The checks (tests/validation_common.py) run on the gfx950 build in test_gpu_validation.py, where the no-host-read test is."""
import pytest

import evaluate_common as ec
import train_common as tc
import validation_common as vc
from helpers import use_emulation_library
from test_emu_train import H, W, _cfg, _make_dcn, _pcl, store  # noqa: F401  (store: the module's fixture)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.fixture(autouse=True)
def exact(monkeypatch):
    from dcn_hip import loss as K
    monkeypatch.setattr(K, "EXACT_BACKWARD", True)


@pytest.fixture(scope="module")
def vstore(_lib):
    return ec.synthetic_store("cpu", H, W, seed=5)


def test_training_with_validation_is_the_same_run(store, vstore):
    vc.check_training_is_the_same_run(_make_dcn, _pcl(), store, vstore, _cfg(True), 1, False)


def test_validation_row_equals_the_pass_run_by_hand(store, vstore):
    vc.check_row_equals_the_pass_by_hand(_make_dcn, _pcl(), store, vstore, _cfg(True), 1, False)


def test_inactive_iteration_is_validated_and_left_out_of_the_log(store, vstore):
    vc.check_inactive_iteration(_make_dcn, _pcl(), store, vstore, _cfg(True), _cfg(True), 1, H, W, False)


def test_save_point_carries_the_validation_key(store, vstore, tmp_path):
    vc.check_save_point(_make_dcn, _pcl(), store, vstore, _cfg(True), 1, tmp_path)


def test_schedule_and_arguments(store, vstore):
    vc.check_schedule_and_arguments(_make_dcn, _pcl(), store, vstore, ec.synthetic_store("cpu", 8, 24), _cfg(True))
