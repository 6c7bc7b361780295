"""The best-match and match-statistics searches (csrc/match_kernels.hip, acrossobj_kernels.hip, evaluate_kernels.hip) through
the host-emulation build: exact-arithmetic inputs against numpy float32 bit for bit, random inputs against float64
(tests/match_common.py)."""
import pytest

import match_common as mc
from helpers import use_emulation_library

DEVICE = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


def test_the_cases_cover_every_width_size_and_placement():
    lattice = [c for c in mc.TIER1 if c.kind.startswith("lattice")]
    for d in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64):
        assert len({c.res.shape[:2] for c in lattice if c.res.shape[2] == d}) >= 2, d
    assert {c.res.shape[0] * c.res.shape[1] for c in lattice} == set(mc.SHAPES)
    assert {c.q1 for c in mc.TIER1} == {1, 31, 32, 33, 65} and {c.q2 for c in mc.TIER1} == {63, 64, 65, 129}
    assert {c.kind for c in lattice} == {"lattice_1", "lattice_2^-30", "lattice_2^30", "lattice_mixed", "lattice_huge"}
    equal = [c for c in mc.TIER1 if c.kind == "equalnorm"]
    assert {c.pair_pixels for c in equal} == set(mc.PLACEMENTS.values())
    assert {(c.pair_pixels, c.name[-1]) for c in equal} >= {(p, str(k)) for p in mc.PLACEMENTS.values() for k in range(3)}


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
