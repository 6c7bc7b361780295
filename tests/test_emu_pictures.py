"""Qualitative evaluation (csrc/picture_kernels.hip, dcn_hip/evaluate/pictures.py) through the host-emulation build: the
reference's three normalisations and matplotlib's bytes (pictures goldens), the ranges and normalisations at 240 x 320 against
the numpy statement, the heat maps on every path against the reference formula, EMPTY_RANGE, the argument errors, the pair
choice, and the whole evaluate_network_qualitative call on a small store with a tiny network (16 x 24 images).  The checks are
in tests/pictures_common.py."""
import pytest
import torch

import pictures_common as pc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


def test_golden_set():
    assert pc.GOLDEN_IDS == pc.EXPECTED_IDS


@pytest.mark.parametrize("name", pc.NORM_IDS)
def test_golden_normalisations_and_pictures(name):
    pc.check_golden(name, "cpu")


@pytest.mark.parametrize("D", pc.CHANNELS)
def test_channel_counts_and_several_workgroups_per_image(D):
    pc.check_statement(D, "cpu")


@pytest.mark.parametrize("name", pc.HEAT_IDS)
def test_golden_heat_maps(name):
    pc.check_heat_golden(name, "cpu")


@pytest.mark.parametrize("case", sorted(pc.HEAT_CASES))
def test_heat_maps(case):
    pc.check_heat(case, "cpu")


def test_colour_table_is_matplotlibs():
    pc.check_colour_table()


def test_empty_range_flags_its_pair_only():
    pc.check_empty_range("cpu")


def test_argument_errors():
    pc.check_argument_errors("cpu", on_emulation=True)


def test_choose_qualitative_pairs():
    pc.check_choose_pairs("cpu")


def test_whole_call_on_a_small_store(tmp_path):
    import pytorch_segmentation_detection.models.resnet_dilated as rd
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    h, w = 16, 24
    torch.manual_seed(0)
    dcn = DenseCorrespondenceNetwork(rd.Resnet18_8s(num_classes=3, base_width=8), 3, image_width=w, image_height=h)
    pc.check_whole_call("cpu", h, w, dcn, tmp_path)
