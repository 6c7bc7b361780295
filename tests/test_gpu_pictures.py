"""Qualitative evaluation (csrc/picture_kernels.hip, dcn_hip/evaluate/pictures.py) on the MI355X: the checks of
tests/pictures_common.py -- the pictures goldens (the reference's three normalisations bit for bit, matplotlib's bytes), the
ranges and normalisations at 240 x 320 against the numpy statement with two bit-identical runs, the heat maps on every path
against the reference formula, EMPTY_RANGE, the argument errors (CPU tensors included), the pair choice, and the whole
evaluate_network_qualitative call with the real Resnet34_8s at 64 x 96.  Reads tests/golden only."""
import pytest
import torch

import pictures_common as pc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("name", pc.NORM_IDS)
def test_golden_normalisations_and_pictures(name):
    pc.check_golden(name, "cuda")


@pytest.mark.parametrize("D", pc.CHANNELS)
def test_channel_counts_and_several_workgroups_per_image(D):
    pc.check_statement(D, "cuda")


@pytest.mark.parametrize("name", pc.HEAT_IDS)
def test_golden_heat_maps(name):
    pc.check_heat_golden(name, "cuda")


@pytest.mark.parametrize("case", sorted(pc.HEAT_CASES))
def test_heat_maps(case):
    pc.check_heat(case, "cuda")


def test_empty_range_flags_its_pair_only():
    pc.check_empty_range("cuda")


def test_argument_errors():
    pc.check_argument_errors("cuda", on_emulation=False)


def test_choose_qualitative_pairs():
    pc.check_choose_pairs("cuda")


def test_whole_call_on_a_small_store(tmp_path):
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    h, w = 64, 96
    torch.manual_seed(0)
    dcn = DenseCorrespondenceNetwork.from_config({"descriptor_dimension": 3, "image_width": w, "image_height": h},
                                                 load_stored_params=False)
    pc.check_whole_call("cuda", h, w, dcn, tmp_path)
