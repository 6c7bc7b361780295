"""The best-match and match-statistics searches (csrc/match_kernels.hip, acrossobj_kernels.hip, evaluate_kernels.hip) on the
MI355X: exact-arithmetic inputs against numpy float32 bit for bit, random inputs against float64 (tests/match_common.py)."""
import pytest

import match_common as mc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("name", mc.TIER1_IDS)
def test_find_best_matches_bit_for_bit(name):
    mc.check_find_best_matches(mc.BY_NAME[name], DEVICE)


@pytest.mark.parametrize("name", mc.TIER1_IDS)
def test_match_statistics_bit_for_bit(name):
    mc.check_match_statistics(mc.BY_NAME[name], DEVICE)


@pytest.mark.parametrize("name", mc.TIER1_IDS)
def test_best_match_pairs_bit_for_bit(name):
    mc.check_best_match_pairs(mc.BY_NAME[name], DEVICE)


@pytest.mark.parametrize("name", mc.TIER1_IDS)
def test_match_statistics_pairs_bit_for_bit(name):
    mc.check_match_statistics_pairs(mc.BY_NAME[name], DEVICE)


@pytest.mark.parametrize("name", ["lattice_d3_hw2072_2^30_pm4", "lattice_d32_hw2072_2^30_pm1", "lattice_d5_hw713_2^-30_pm4",
                                  "equalnorm_d3_last_groups_pair2"])
def test_four_entry_points_agree(name):
    mc.check_four_entry_points_agree(mc.BY_NAME[name], DEVICE)


@pytest.mark.parametrize("name", ["lattice_d32_hw2072_2^30_pm1", "lattice_d3_hw713_mixed_pm4", "equalnorm_d2_first_wave_pair0"])
def test_two_consecutive_calls_are_identical(name):
    mc.check_run_to_run(mc.BY_NAME[name], DEVICE)


@pytest.mark.parametrize("name", [c.name for c in mc.TIER1 if c.kind == "equalnorm"])
def test_equal_norm_image_across_kernels(name):
    mc.check_equal_norm_across_kernels(mc.BY_NAME[name], DEVICE)


def test_reference_shaped_wrappers():
    mc.check_reference_shaped_wrappers(mc.BY_NAME["lattice_d3_hw713_2^-30_pm4"], DEVICE)


@pytest.mark.parametrize("d,n", mc.TIER2, ids=mc.TIER2_IDS)
def test_random_data_single_image_kernels_vs_float64(d, n):
    mc.check_tier2_single_image(d, n, DEVICE)


@pytest.mark.parametrize("d,n", mc.TIER2, ids=mc.TIER2_IDS)
def test_random_data_pair_kernels_vs_float64(d, n):
    mc.check_tier2_pairs(d, n, DEVICE)
