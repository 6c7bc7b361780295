"""Synthetic multi-object merge (csrc/merge_kernels.hip) through the host-emulation build: the mirror module against the
reference's golden outputs, the batched path against a numpy restatement, against two chained merges of the mirror in the
reference's order and against torch's normalization, the empty-sample rule, index checks, and record draw / replay."""
import numpy as np
import pytest
import torch

import merge_common as mc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.mark.parametrize("path", mc.GOLDENS, ids=mc.GOLDEN_IDS)
def test_mirror_replays_reference_golden(path):
    mc.replay_golden(path, "cpu")


def test_golden_set_is_complete():
    ids = set(mc.GOLDEN_IDS)
    for need in mc.REQUIRED_GOLDENS:
        assert need in ids, need


@pytest.mark.parametrize("h,w", [(24, 36), (13, 17), (1, 8), (9, 1), (1, 1)])
def test_batched_path_matches_restatement(h, w):
    n = 5
    counts_a, counts_b = [7, 0, 30, 1, 12], [5, 9, 0, 3, 40]
    rgb, masks, lists = mc.example_batch(n, h, w, counts_a, counts_b, seed=h * 100 + w)
    fg = np.array([[0, 1], [1, 0], [1, 1], [0, 0], [1, 0]], dtype=np.int32)
    r = mc.run_batched(rgb, masks, lists, fg, "cpu")
    assert r.input_1.shape == (n, 3, h, w) and r.input_1.dtype == torch.float32 and r.mask_2.shape == (n, h, w)
    assert r.empty.dtype == torch.bool and r.foreground.dtype == torch.int32
    mc.check_batched_against_restatement(r, rgb, masks, lists, fg)


def test_batched_path_equals_two_chained_mirror_merges():
    """spartan_dataset_masked.py:930-953 through the single-merge mirror (pinned to the reference by the goldens), with the same
    foreground decisions: merged images, masks and the concatenated lists agree sample by sample, empty samples included."""
    n, h, w = 8, 20, 28
    rgb, masks, lists = mc.example_batch(n, h, w, [40, 25, 60, 8, 33, 50, 12, 20], [30, 44, 9, 25, 61, 14, 27, 5], seed=4)
    masks[2, 5] = 1                                              # sample 5: b covers a's frame 1 -> empty when b is in front
    masks[1, 6] = 1                                              # sample 6: only frame 2 occludes everything of b
    fg = np.array([[0, 1], [1, 0], [1, 1], [0, 0], [1, 0], [1, 0], [1, 0], [0, 1]], dtype=np.int32)
    r = mc.run_batched(rgb, masks, lists, fg, "cpu")
    off = r.offsets.numpy()
    assert bool(r.empty[5]) and bool(r.empty[6])
    for s in range(n):
        exp = mc.chained_mirror_sample(rgb, masks, lists, s, fg, "cpu")
        assert bool(r.empty[s]) == (exp is None), s
        m1, mm1, m2, mm2 = (torch.from_numpy(mc.restated_merge(rgb[f, s], rgb[2 + f, s], masks[f, s], masks[2 + f, s],
                                                               fg[s, f] == 1)[k]) for f in (0, 1) for k in (0, 1))
        if exp is not None:
            m1, mm1, m2, mm2 = exp[:4]
            sl = slice(int(off[s]), int(off[s + 1]))
            for got, want in ((r.uv_1, exp[4]), (r.uv_2, exp[5])):
                assert torch.equal(got[0][sl], want[0]) and torch.equal(got[1][sl], want[1]), s
        else:
            assert off[s + 1] == off[s]
        assert torch.equal(r.rgb_1[s], m1) and torch.equal(r.rgb_2[s], m2), s
        assert torch.equal(r.mask_1[s], mm1.float()) and torch.equal(r.mask_2[s], mm2.float()), s


def test_network_inputs_are_torchs_normalization_of_the_merged_image():
    from dcn_hip import merge
    n, h, w = 3, 12, 16
    rgb, masks, lists = mc.example_batch(n, h, w, [4, 5, 6], [3, 2, 1], seed=9)
    fg = np.array([[1, 0], [0, 1], [1, 1]], dtype=np.int32)
    mean, std = [0.1, 0.7, 0.33], [0.2, 0.31, 0.45]
    t = torch.from_numpy
    (ua1, va1, ua2, va2, offa), (ub1, vb1, ub2, vb2, offb) = lists
    r = merge.merge_synthetic_samples(*(t(x) for x in rgb), *(t(x) for x in masks), (t(ua1), t(va1)), (t(ua2), t(va2)),
                                      (t(ub1), t(vb1)), (t(ub2), t(vb2)), offa, offb, foreground=fg, mean=mean, std=std,
                                      return_rgb=True)
    assert torch.equal(r.input_1, mc.normalize_torch(r.rgb_1.numpy(), mean, std))
    assert torch.equal(r.input_2, mc.normalize_torch(r.rgb_2.numpy(), mean, std))


def test_out_of_range_entries_set_status_and_are_dropped():
    n, h, w = 2, 10, 12
    rgb, masks, lists = mc.example_batch(n, h, w, [6, 6], [6, 6], seed=2)
    ua1 = lists[0][0].copy()
    ua1[1], ua1[7] = w, -1                                       # sample 0 frame 1, sample 1 frame 1
    vb2 = lists[1][3].copy()
    vb2[3] = h + 5                                               # sample 0 frame 2
    lists = [(ua1,) + lists[0][1:], lists[1][:3] + (vb2, lists[1][4])]
    fg = np.array([[0, 0], [1, 1]], dtype=np.int32)
    r = mc.run_batched(rgb, masks, lists, fg, "cpu")
    assert int(r.status[0]) & 1
    mc.check_batched_against_restatement(r, rgb, masks, lists, fg)
    kept_u1 = r.uv_1[0][:int(r.offsets[-1])]
    assert bool((kept_u1 >= 0).all() and (kept_u1 < w).all())


def test_mirror_raises_index_error_for_out_of_range_entries():
    from dense_correspondence.correspondence_tools import correspondence_augmentation as ca
    mask = torch.zeros(6, 7, dtype=torch.uint8)
    ok = (torch.tensor([0, 6]), torch.tensor([5, 0]))
    for u, v in (([0, 7], [0, 0]), ([0, 1], [6, 0]), ([-1, 0], [0, 0])):
        with pytest.raises(IndexError):
            ca.prune_matches_if_occluded(mask, ((torch.tensor(u), torch.tensor(v)), ok))
    first, second = ca.prune_matches_if_occluded(mask, (ok, ok))
    assert torch.equal(first[0], ok[0]) and torch.equal(second[1], ok[1])


def test_malformed_offsets_empty_every_sample():
    from dcn_hip import merge
    n, h, w = 3, 8, 8
    rgb, masks, lists = mc.example_batch(n, h, w, [4, 4, 4], [4, 4, 4], seed=3)
    t = torch.from_numpy
    (ua1, va1, ua2, va2, _), (ub1, vb1, ub2, vb2, offb) = lists
    r = merge.merge_synthetic_samples(*(t(x) for x in rgb), *(t(x) for x in masks), (t(ua1), t(va1)), (t(ua2), t(va2)),
                                      (t(ub1), t(vb1)), (t(ub2), t(vb2)), [0, 8, 4, 12], offb, foreground=np.zeros((n, 2)))
    assert int(r.status[0]) & merge.BAD_OFFSETS
    assert bool(r.empty.all()) and bool((r.offsets == 0).all()) and bool((r.uv_1[0] == -1).all())


def test_foreground_draw_and_replay():
    from dcn_hip import merge
    n, h, w = 64, 6, 8
    rgb, masks, lists = mc.example_batch(n, h, w, [3] * n, [2] * n, seed=5)
    g = lambda: torch.Generator().manual_seed(11)
    t = torch.from_numpy
    (ua1, va1, ua2, va2, offa), (ub1, vb1, ub2, vb2, offb) = lists
    call = lambda **kw: merge.merge_synthetic_samples(*(t(x) for x in rgb), *(t(x) for x in masks), (t(ua1), t(va1)),
                                                      (t(ua2), t(va2)), (t(ub1), t(vb1)), (t(ub2), t(vb2)), offa, offb, **kw)
    r1, r2 = call(generator=g()), call(generator=g())
    fg = r1.foreground
    assert fg.dtype == torch.int32 and fg.shape == (n, 2) and bool(((fg == 0) | (fg == 1)).all())
    assert 0 < int(fg.sum()) < 2 * n and torch.equal(fg, r2.foreground)
    assert torch.equal(fg, merge.draw_foreground(n, "cpu", generator=g()))
    r3 = call(foreground=fg.numpy())
    for k in ("input_1", "input_2", "mask_1", "mask_2", "offsets", "empty"):
        assert torch.equal(getattr(r1, k), getattr(r3, k)), k
    assert torch.equal(r1.uv_1[0], r3.uv_1[0]) and torch.equal(r1.uv_2[1], r3.uv_2[1])
    mc.check_batched_against_restatement(call(foreground=fg, return_rgb=True), rgb, masks, lists, fg.numpy())


def test_bad_arguments_raise():
    from dcn_hip import merge
    n, h, w = 2, 8, 8
    rgb, masks, lists = mc.example_batch(n, h, w, [2, 2], [2, 2], seed=6)
    t = torch.from_numpy
    (ua1, va1, ua2, va2, offa), (ub1, vb1, ub2, vb2, offb) = lists
    ims = [t(x) for x in rgb]
    mks = [t(x) for x in masks]
    uv = [(t(ua1), t(va1)), (t(ua2), t(va2)), (t(ub1), t(vb1)), (t(ub2), t(vb2))]
    fg = np.zeros((n, 2), np.int32)
    with pytest.raises(ValueError):   # float image
        merge.merge_synthetic_samples(ims[0].float(), *ims[1:], *mks, *uv, offa, offb, foreground=fg)
    with pytest.raises(ValueError):   # mask of another size
        merge.merge_synthetic_samples(*ims, mks[0][:, :4], *mks[1:], *uv, offa, offb, foreground=fg)
    with pytest.raises(ValueError):   # offsets of the wrong length
        merge.merge_synthetic_samples(*ims, *mks, *uv, offa[:2], offb, foreground=fg)
    with pytest.raises(ValueError):   # foreground records of the wrong shape
        merge.merge_synthetic_samples(*ims, *mks, *uv, offa, offb, foreground=np.zeros((n + 1, 2)))
    with pytest.raises(ValueError):   # int32 match lists
        merge.merge_synthetic_samples(*ims, *mks, (uv[0][0].int(), uv[0][1].int()), *uv[1:], offa, offb, foreground=fg)
    with pytest.raises(ValueError):   # the pair's two lists differ in length
        merge.merge_synthetic_samples(*ims, *mks, uv[0], (uv[1][0][:3], uv[1][1][:3]), *uv[2:], offa, offb, foreground=fg)
