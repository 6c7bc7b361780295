"""Descriptor statistics of a dataset (csrc/descstats_kernels.hip, dcn_hip/evaluate/descstats.py) on the MI355X: the checks of
tests/descstats_common.py -- the descstats goldens (the reference's own per-image statistics and update_stats loop), every
channel-count path at 240 x 320 against a float64 numpy statement with two bit-identical runs, NaN, the argument errors
(CPU tensors included), the frame choice, and the whole compute_descriptor_statistics_on_dataset call with the real Resnet34_8s
at 64 x 96.  Reads tests/golden only."""
import pytest
import torch

import descstats_common as dc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("path", dc.GOLDENS, ids=dc.GOLDEN_IDS)
def test_golden_per_image(path):
    dc.check_golden_per_image(path, "cuda")


@pytest.mark.parametrize("path", dc.GOLDENS, ids=dc.GOLDEN_IDS)
def test_golden_combine(path):
    dc.check_golden_combine(path, "cuda")


def test_no_image_used_leaves_nan():
    dc.check_no_image_used("cuda")


@pytest.mark.parametrize("D", dc.CHANNELS)
def test_channel_counts_and_several_workgroups_per_image(D):
    dc.check_channels(D, "cuda")


@pytest.mark.parametrize("case", dc.NAN_CASES)
def test_nan_follows_torch(case):
    dc.check_nan("cuda", case)


def test_argument_errors():
    dc.check_argument_errors("cuda", on_emulation=False)


def test_choose_frames():
    dc.check_choose_frames("cuda")


def test_whole_call_on_a_small_store(tmp_path):
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    h, w = 64, 96
    torch.manual_seed(0)
    dcn = DenseCorrespondenceNetwork.from_config({"descriptor_dimension": 3, "image_width": w, "image_height": h},
                                                 load_stored_params=False)
    dc.check_whole_call("cuda", h, w, dcn, tmp_path)
