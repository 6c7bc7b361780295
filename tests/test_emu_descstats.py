"""Descriptor statistics of a dataset (csrc/descstats_kernels.hip, dcn_hip/evaluate/descstats.py) through the host-emulation build: the
reference's own compute_descriptor_statistics / update_stats loop replayed (descstats goldens), every channel-count path
with several workgroups per image against a float64 numpy statement, NaN, the argument errors, the frame choice, and the whole
compute_descriptor_statistics_on_dataset call on a small store with a tiny network (16 x 24 images: the emulated forwards
take a few seconds).  The checks are in tests/descstats_common.py."""
import numpy as np
import pytest
import torch

import descstats_common as dc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


def test_golden_set():
    assert dc.GOLDEN_IDS == dc.EXPECTED_IDS


@pytest.mark.parametrize("path", dc.GOLDENS, ids=dc.GOLDEN_IDS)
def test_golden_per_image(path):
    dc.check_golden_per_image(path, "cpu")


@pytest.mark.parametrize("path", dc.GOLDENS, ids=dc.GOLDEN_IDS)
def test_golden_combine(path):
    dc.check_golden_combine(path, "cpu")


def test_no_image_used_leaves_nan():
    dc.check_no_image_used("cpu")


@pytest.mark.parametrize("D", dc.CHANNELS)
def test_channel_counts_and_several_workgroups_per_image(D):
    dc.check_channels(D, "cpu")


@pytest.mark.parametrize("case", dc.NAN_CASES)
def test_nan_follows_torch(case):
    dc.check_nan("cpu", case)


def test_argument_errors():
    dc.check_argument_errors("cpu", on_emulation=True)


def test_choose_frames():
    dc.check_choose_frames("cpu")


def test_whole_call_on_a_small_store(tmp_path):
    import pytorch_segmentation_detection.models.resnet_dilated as rd
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    h, w = 16, 24
    torch.manual_seed(0)
    dcn = DenseCorrespondenceNetwork(rd.Resnet18_8s(num_classes=3, base_width=8), 3, image_width=w, image_height=h)
    dc.check_whole_call("cpu", h, w, dcn, tmp_path)
