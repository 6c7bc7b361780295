"""Class-consistent keypoint evaluation on the MI355X (dcn_hip/evaluate/keypoints.py, the wide statistics kernel of
csrc/crossscene_kernels.hip): the reference goldens through the chain with the wide entry, the grouped entry and the two-sweep
path, the wide entry against the grouped one bit for bit, and run-to-run bit identity with a tie planted across strips."""
import numpy as np
import pytest

import keypoints_common as kc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("path", kc.GOLDENS, ids=kc.GOLDEN_IDS)
def test_golden_through_the_chain(path):
    kc.check_golden_every_way(np.load(path), "cuda")


@pytest.mark.parametrize("case", kc.WIDE_CASES, ids=kc.WIDE_IDS)
def test_wide_equals_groups_bit_for_bit(case):
    kc.check_wide_against_groups(*case, device="cuda")


def test_wide_equals_groups_on_a_grid_of_many_strips():
    """48 x 64 with the automatic strip (512 pixels: six strips) and with strips of 100 pixels, no multiple of the tile; a
    group of 300 rows, one of 70 and an empty one"""
    from dcn_hip import evaluate
    import crossscene_common as cc
    groups, _, _ = cc.random_groups((300, 0, 70), 48, 64, 8, seed=5, device="cuda")
    a = evaluate.match_statistics_groups(**groups)
    assert int(a.status.cpu()[0]) == 0
    for strip in (0, 100):
        cc.same_tables(a, evaluate.match_statistics_groups_wide(strip_pixels=strip, **groups))


def test_two_runs_are_bit_identical_with_a_planted_tie_across_strips():
    kc.check_planted_tie("cuda")
