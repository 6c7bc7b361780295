"""tests/test_emu_datapath.py's checks on the MI355X (bodies in tests/datapath_common.py): the refusals of the sample entry
points with device buffers, the Python argument errors (and a host tensor where the library takes device memory), and the call
sites the other files do not reach."""
import pytest

import datapath_common as dc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("entry", dc.ENTRIES)
def test_refusals_return_invalid_and_launch_nothing(entry):
    dc.check_refusals(entry, "cuda")


def test_concat_refusals_return_invalid_and_launch_nothing():
    dc.check_concat_refusals("cuda")


def test_workspace_sizes_of_refused_arguments_are_zero():
    dc.check_workspace_refusals()


def test_sample_builders_argument_errors():
    dc.check_sample_argument_errors("cuda")


def test_evaluate_argument_errors():
    dc.check_evaluate_argument_errors("cuda")


def test_frame_store_and_select_frames_argument_errors():
    dc.check_frames_argument_errors("cuda")


def test_merge_augment_pairgen_argument_errors():
    dc.check_merge_augment_pairgen_argument_errors("cuda")


def test_uniform_candidates_with_more_attempts_than_pixels():
    dc.check_uniform_candidates_more_attempts_than_pixels("cuda")


def test_complete_samples_without_a_single_match():
    dc.check_complete_samples_without_matches("cuda")


@pytest.mark.parametrize("replay", [True, False], ids=["replay", "seeded"])
def test_eval_matches_with_more_attempts_than_pixels(replay):
    dc.check_eval_matches_more_attempts_than_pixels("cuda", replay)


@pytest.mark.parametrize("h,w", [(7, 9), (20, 28)])
def test_concat_of_one_batch_and_of_within_with_across(h, w):
    dc.check_concat_of_one_and_of_two("cuda", h, w)
