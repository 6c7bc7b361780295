"""The host side of the device data path (samples, frames, evaluate, merge, augment, pairgen and the host half of
csrc/sample_kernels.hip) through the host-emulation build: the refusals of the sample entry points, the Python argument errors,
and the call sites the other files do not reach.  The bodies are in tests/datapath_common.py; tests/test_gpu_datapath.py runs
the same on the MI355X."""
import pytest

import datapath_common as dc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.mark.parametrize("entry", dc.ENTRIES)
def test_refusals_return_invalid_and_launch_nothing(entry):
    dc.check_refusals(entry, "cpu")


def test_concat_refusals_return_invalid_and_launch_nothing():
    dc.check_concat_refusals("cpu")


def test_workspace_sizes_of_refused_arguments_are_zero():
    dc.check_workspace_refusals()


def test_sample_builders_argument_errors():
    dc.check_sample_argument_errors("cpu")


def test_evaluate_argument_errors():
    dc.check_evaluate_argument_errors("cpu")


def test_frame_store_and_select_frames_argument_errors():
    dc.check_frames_argument_errors("cpu")


def test_merge_augment_pairgen_argument_errors():
    dc.check_merge_augment_pairgen_argument_errors("cpu")


def test_uniform_candidates_with_more_attempts_than_pixels():
    dc.check_uniform_candidates_more_attempts_than_pixels("cpu")


def test_complete_samples_without_a_single_match():
    dc.check_complete_samples_without_matches("cpu")


@pytest.mark.parametrize("replay", [True, False], ids=["replay", "seeded"])
def test_eval_matches_with_more_attempts_than_pixels(replay):
    dc.check_eval_matches_more_attempts_than_pixels("cpu", replay)


@pytest.mark.parametrize("h,w", [(7, 9), (20, 28)])
def test_concat_of_one_batch_and_of_within_with_across(h, w):
    dc.check_concat_of_one_and_of_two("cpu", h, w)
