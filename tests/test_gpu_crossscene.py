"""Cross-scene evaluation on the MI355X (csrc/crossscene_kernels.hip, dcn_hip/evaluate/cross_scene.py): the reference goldens on the device,
the chain against the pair-wise statistics kernels called row by row on the same descriptors, the grouped entry against the
pair-wise one, and run-to-run bit identity with a planted exact tie."""
import numpy as np
import pytest
import torch

import crossscene_common as cc
from helpers import use_gfx950_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gfx950_library()


@pytest.mark.parametrize("path", cc.GOLDENS, ids=cc.GOLDEN_IDS)
def test_golden_through_the_chain(path):
    cc.check_golden(np.load(path), "cuda", batch_frames=4)


def test_chain_equals_the_pair_kernels_row_by_row():
    """evaluate_cross_scene_rows at 48 x 64: every row that exists, fed to match_statistics_pairs as a pair of its own with the
    same descriptor images, comes out with equal integers and bit-equal float columns (one arithmetic, eval_stats.h); a second
    run with other batch and chunk sizes gives the same bits."""
    from dcn_hip import evaluate
    z = np.load([p for p, i in zip(cc.GOLDENS, cc.GOLDEN_IDS) if i == "48x64_d3"][0])
    store, net, labels, views, t = cc.check_golden(z, "cuda")
    rows = torch.nonzero(t.row_pair >= 0)[:, 0]
    fr = views[rows.cpu().numpy(), 3:5]
    n = len(fr)
    assert n >= 10
    cams = evaluate._gather_host_frames(store, fr, ("cams",))[3][0]
    fa, fb = torch.from_numpy(fr[:, 0]).cuda(), torch.from_numpy(fr[:, 1]).cuda()
    for one_by_one in (False, True):
        for lo in (range(n) if one_by_one else [0]):
            at = slice(lo, lo + 1) if one_by_one else slice(0, n)
            k = rows[at]
            tp = evaluate.match_statistics_pairs(net.table[fa[at]].contiguous(), net.table[fb[at]].contiguous(),
                                                 store.mask[fb[at]], store.depth[fa[at]], store.depth[fb[at]], cams[at], t.u_a[k],
                                                 t.v_a[k], t.u_b[k], t.v_b[k], torch.arange(len(k) + 1, device="cuda"))
            assert int(tp.status.cpu()[0]) == 0
            for name in ("columns", "is_valid", "pred_uv", "closer"):
                assert torch.equal(cc.bits(getattr(t, name)[:, k]), cc.bits(getattr(tp, name))), (name, lo)
            assert torch.equal(t.mask_pixels[k], tp.mask_pixels)
    store2, net2 = cc.golden_store(z, "cuda")
    cc.same_tables(t, evaluate.evaluate_cross_scene_rows(net2, store2, labels, views, batch_frames=3, max_search_bytes=1))


@pytest.mark.parametrize("d", [3, 7, 16])
def test_groups_equal_pairs_bit_for_bit(d):
    """Groups of 33, 70 and 1 rows (and an empty one) over 48 x 64 images -- twelve workgroups per image -- against the pair-wise
    entry fed the same rows one pair each"""
    groups, pairs, group = cc.random_groups((33, 0, 70, 1), 48, 64, d, seed=d, device="cuda")
    cc.check_groups_against_pairs(groups, pairs, group)


def test_two_runs_are_bit_identical_with_a_planted_tie():
    """Two pixels of the searched image, in different workgroups, both EQUAL to a query: the distance 0 ties exactly and the
    smaller flat index wins, in the image and under the mask, every time"""
    from dcn_hip import evaluate
    h, w = 48, 64
    groups, _, _ = cc.random_groups((33, 70, 1), h, w, 3, seed=11, device="cuda", keep_fraction=1.0)
    r, g = 40, 1                                            # a row of the second group
    lo, hi = 5 * w + 9, 40 * w + 50                         # flat indices 329 and 2610: workgroups 1 and 10
    for flat in (lo, hi):
        groups["res_b"][g].view(h * w, 3)[flat] = groups["queries"][r]
        groups["mask_b"][g].view(h * w)[flat] = 1
    a = evaluate.match_statistics_groups(**groups)
    assert int(a.status.cpu()[0]) == 0
    assert a.pred_uv[:, r].tolist() == [lo % w, lo // w, lo % w, lo // w]
    assert float(a.column("norm_diff_descriptor")[r]) == 0.0 and float(a.column("norm_diff_descriptor_masked")[r]) == 0.0
    groups["mask_b"][g].view(h * w)[lo] = 0                  # off the mask, the first one is a million away
    b = evaluate.match_statistics_groups(**groups)
    assert b.pred_uv[:, r].tolist() == [lo % w, lo // w, hi % w, hi // w]
    for _ in range(3):
        cc.same_tables(b, evaluate.match_statistics_groups(**groups))
