"""Shared by tests/test_emu_merge.py and tests/test_gpu_merge.py (not a test module): a numpy restatement of the synthetic
multi-object merge (include/dcn_hip.h section 8, after dense_correspondence/correspondence_tools/correspondence_augmentation.py
:217-345 and spartan_dataset_masked.py:890-960), the golden-fixture replay through the mirror module, and the reference's
two chained merges of one sample through that mirror."""
import glob
import os
import random

import numpy as np
import torch

GOLDENS = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("merge_ref_"):-4] for p in GOLDENS]
REQUIRED_GOLDENS = ("partial_front_b", "partial_front_a", "partial_front_b_37x53", "partial_front_a_37x53",
                    "no_occlusion_front_b_37x53", "full_occlusion_front_b_37x53", "full_occlusion_front_a_1x64",
                    "partial_front_b_1x64", "partial_front_a_48x1", "prune_partial_37x53", "prune_none_kept_37x53",
                    "prune_all_kept_1x64", "merge_matches")

FG_A, FG_B = 0, 1


def restated_merge(rgb_a, rgb_b, mask_a, mask_b, front_b):
    """One frame of one sample -> (merged uint8 [h, w, 3], merged mask uint8 [h, w]) in the reference's uint8 arithmetic."""
    fg, bg, m = (rgb_b, rgb_a, mask_b) if front_b else (rgb_a, rgb_b, mask_a)
    m3 = np.repeat(m[:, :, None], 3, axis=2).astype(np.uint8)
    merged = fg * m3 + (np.ones_like(m3) - m3) * bg
    return merged.astype(np.uint8), (mask_a + mask_b).clip(0, 1).astype(np.uint8)


def restated_prune(fg, masks, lists, h, w, drop_empty=True):
    """fg: [B, 2] records; masks: {(frame, obj): uint8 [B, h, w]} (obj 0 = a, 1 = b); lists: per object (u1, v1, u2, v2,
    offsets) numpy int64.  -> (u1, v1, u2, v2 of the kept entries, offsets [B + 1], empty [B], status)."""
    n = fg.shape[0]
    out = [[], [], [], []]
    offsets, empty, status = [0], [], 0
    for s in range(n):
        kept = []
        for o in range(2):
            u1, v1, u2, v2, off = lists[o]
            sel = []
            for i in range(int(off[s]), int(off[s + 1])):
                ok = True
                for f, (u, v) in enumerate(((u1[i], v1[i]), (u2[i], v2[i]))):
                    m = masks.get((f + 1, 1 - o))
                    if m is None:
                        continue
                    if not (0 <= u < w and 0 <= v < h):
                        status |= 1
                        ok = False
                    elif (fg[s, f] == FG_B) == (o == 0) and m[s, v, u] != 0:
                        ok = False
                if ok:
                    sel.append(i)
            kept.append((o, sel))
        is_empty = any(len(sel) == 0 for _, sel in kept)
        empty.append(is_empty)
        if not (drop_empty and is_empty):
            for o, sel in kept:
                for k, arr in enumerate(lists[o][:4]):
                    out[k].extend(arr[sel].tolist())
        offsets.append(len(out[0]))
    return [np.array(x, dtype=np.int64) for x in out], np.array(offsets), np.array(empty), status


def example_batch(n, h, w, counts_a, counts_b, seed=0):
    """n samples: random images, 0/1 blob masks (some empty / full), match lists of the given lengths inside the image."""
    rng = np.random.RandomState(seed)
    rgb = rng.randint(0, 256, size=(4, n, h, w, 3)).astype(np.uint8)          # a1, a2, b1, b2
    y, x = np.mgrid[0:h, 0:w]
    masks = np.zeros((4, n, h, w), np.uint8)
    for k in range(4):
        for s in range(n):
            cy, cx, r = rng.rand() * h, rng.rand() * w, 0.2 + 0.5 * rng.rand()
            masks[k, s] = ((y - cy) / (r * h + 1)) ** 2 + ((x - cx) / (r * w + 1)) ** 2 <= 1.0
    lists = []
    for counts in (counts_a, counts_b):
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        m = int(off[-1])
        lists.append((rng.randint(0, w, m), rng.randint(0, h, m), rng.randint(0, w, m), rng.randint(0, h, m), off))
    return rgb, masks, lists


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def replay_golden(path, device):
    """Runs the mirror module on ``device`` tensors with the recorded seed; asserts equality with the reference's outputs
    (uint8 image and mask, the pruned lists or None) and the same state of ``random`` afterwards."""
    from dense_correspondence.correspondence_tools import correspondence_augmentation as ca
    z = np.load(path)
    fn = str(z["fn"])
    pair = lambda k1, k2: ((_t(z["u_" + k1], device), _t(z["v_" + k1], device)),
                           (_t(z["u_" + k2], device), _t(z["v_" + k2], device)))
    if fn == "merge_matches":
        u, v = ca.merge_matches((_t(z["u_1"], device), _t(z["v_1"], device)), (_t(z["u_2"], device), _t(z["v_2"], device)))
        assert u.dtype == torch.int64 and np.array_equal(u.cpu().numpy(), z["out_u"])
        assert np.array_equal(v.cpu().numpy(), z["out_v"])
        return
    if fn == "prune_matches_if_occluded":
        first, second = ca.prune_matches_if_occluded(_t(z["mask"], device), pair("1", "2"))
        if bool(z["none"]):
            assert first is None and second is None
            return
        for got, k in ((first, "1"), (second, "2")):
            assert got[0].dtype == torch.int64
            assert np.array_equal(got[0].cpu().numpy(), z["out_u_" + k]) and np.array_equal(got[1].cpu().numpy(), z["out_v_" + k])
        return
    random.seed(int(z["seed"]))
    out = ca.merge_images_with_occlusions(_t(z["rgb_a"], device), _t(z["rgb_b"], device), _t(z["mask_a"], device),
                                          _t(z["mask_b"], device), pair("a1", "a2"), pair("b1", "b2"))
    assert random.random() == float(z["after_random"][0])
    assert out[0].dtype == torch.uint8 and np.array_equal(out[0].cpu().numpy(), z["out_rgb"])
    assert out[1].dtype == torch.uint8 and np.array_equal(out[1].cpu().numpy(), z["out_mask"])
    for got, k in zip(out[2:], ("a1", "a2", "b1", "b2")):
        if bool(z["none_" + k]):
            assert got is None, k
        else:
            assert np.array_equal(got[0].cpu().numpy(), z["out_u_" + k]), k
            assert np.array_equal(got[1].cpu().numpy(), z["out_v_" + k]), k


def chained_mirror_sample(rgb, masks, lists, s, fg, device):
    """Sample s the way spartan_dataset_masked.py:930-953 builds it from the mirror's single merges, with the foreground
    decisions of fg[s] replayed through ``random.random()``: -> None (empty sample) or (merged_1, mask_1, merged_2, mask_2,
    uv_1 = merge_matches(uv_a1, uv_b1), uv_2 = merge_matches(uv_a2, uv_b2))."""
    from dense_correspondence.correspondence_tools import correspondence_augmentation as ca
    t = lambda a: _t(a, device)
    sel = lambda o: slice(int(lists[o][4][s]), int(lists[o][4][s + 1]))
    uv = lambda o, f: (t(lists[o][2 * f][sel(o)]), t(lists[o][2 * f + 1][sel(o)]))
    uv_a1, uv_a2, uv_b1, uv_b2 = uv(0, 0), uv(0, 1), uv(1, 0), uv(1, 1)
    draws = [0.25 if fg[s, f] == FG_B else 0.75 for f in range(2)]
    saved = random.random
    random.random = lambda: draws.pop(0)
    try:
        m1, mm1, uv_a1, uv_a2, uv_b1, uv_b2 = ca.merge_images_with_occlusions(
            t(rgb[0, s]), t(rgb[2, s]), t(masks[0, s]), t(masks[2, s]), (uv_a1, uv_a2), (uv_b1, uv_b2))
        if any(x is None for x in (uv_a1, uv_a2, uv_b1, uv_b2)):
            return None
        m2, mm2, uv_a2, uv_a1, uv_b2, uv_b1 = ca.merge_images_with_occlusions(
            t(rgb[1, s]), t(rgb[3, s]), t(masks[1, s]), t(masks[3, s]), (uv_a2, uv_a1), (uv_b2, uv_b1))
        if any(x is None for x in (uv_a1, uv_a2, uv_b1, uv_b2)):
            return None
    finally:
        random.random = saved
    return m1, mm1, m2, mm2, ca.merge_matches(uv_a1, uv_b1), ca.merge_matches(uv_a2, uv_b2)


def normalize_torch(rgb_nhwc, mean, std):
    """torchvision ToTensor + Normalize (spartan_dataset_masked.py:297-304) on the host: float(x) / 255, - mean, / std."""
    t = torch.from_numpy(np.ascontiguousarray(rgb_nhwc)).permute(0, 3, 1, 2).float().div(255)
    return t.sub(torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)).div(torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1))


def run_batched(rgb, masks, lists, fg, device, return_rgb=True):
    from dcn_hip import merge
    t = lambda a: _t(a, device)
    (ua1, va1, ua2, va2, offa), (ub1, vb1, ub2, vb2, offb) = lists
    return merge.merge_synthetic_samples(t(rgb[0]), t(rgb[1]), t(rgb[2]), t(rgb[3]), t(masks[0]), t(masks[1]), t(masks[2]),
                                         t(masks[3]), (t(ua1), t(va1)), (t(ua2), t(va2)), (t(ub1), t(vb1)), (t(ub2), t(vb2)),
                                         t(offa), t(offb), foreground=t(fg), return_rgb=return_rgb)


def check_batched_against_restatement(r, rgb, masks, lists, fg):
    """Every output of merge_synthetic_samples against the numpy restatement."""
    from dcn_hip import merge
    n = fg.shape[0]
    h, w = masks.shape[2], masks.shape[3]
    for s in range(n):
        for f in range(2):
            exp_rgb, exp_mask = restated_merge(rgb[f, s], rgb[2 + f, s], masks[f, s], masks[2 + f, s], fg[s, f] == FG_B)
            assert np.array_equal((r.rgb_2 if f else r.rgb_1)[s].cpu().numpy(), exp_rgb), (s, f)
            assert np.array_equal((r.mask_2 if f else r.mask_1)[s].cpu().numpy(), exp_mask.astype(np.float32)), (s, f)
            exp_in = normalize_torch(exp_rgb[None], merge.DEFAULT_IMAGE_MEAN, merge.DEFAULT_IMAGE_STD_DEV)
            assert torch.equal((r.input_2 if f else r.input_1)[s:s + 1].cpu(), exp_in), (s, f)
    mk = {(f + 1, o): masks[2 * o + f] for f in range(2) for o in range(2)}
    (u1, v1, u2, v2), off, empty, status = restated_prune(fg, mk, lists, h, w)
    assert np.array_equal(r.offsets.cpu().numpy(), off)
    assert np.array_equal(r.empty.cpu().numpy(), empty)
    assert int(r.status.cpu()[0]) == status
    k = int(off[-1])
    for got, exp in ((r.uv_1[0], u1), (r.uv_1[1], v1), (r.uv_2[0], u2), (r.uv_2[1], v2)):
        g = got.cpu().numpy()
        assert got.dtype == torch.int64 and np.array_equal(g[:k], exp) and bool((g[k:] == -1).all())
