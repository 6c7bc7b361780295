"""Shared by tests/test_emu_synthetic.py and tests/test_gpu_synthetic.py (not a test module): a numpy restatement of the
SYNTHETIC_MULTI_OBJECT sample (include/dcn_hip.h section 9a, after spartan_dataset_masked.py:890-1053) built from
samples_common and merge_common, the composition of the existing entry points that the fused chain must equal, the golden
replay (tests/golden/synthetic_ref_*.npz) and the example batches."""
import glob
import os

import numpy as np
import torch

import merge_common as mc
import samples_common as sc

GOLDENS = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthetic_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("synthetic_ref_"):-4] for p in GOLDENS]
REQUIRED_GOLDENS = ("fg_aa_48x64", "fg_ab_48x64", "fg_ba_37x53", "fg_bb_37x53", "row_1x64", "column_48x1",
                    "uniform_candidates_37x53", "no_mask_inv_48x64", "a_finds_nothing_37x53", "b_finds_nothing_37x53",
                    "occluded_frame_1_48x64", "occluded_frame_2_only_37x53")
SITES = ("cand_a", "cand_b", "masked", "background")
SHAPES = ((24, 36), (13, 17), (1, 8), (9, 1), (1, 1))
FG_A, FG_B = mc.FG_A, mc.FG_B
SMALL_K = np.array([[20.0, 0, 4.2], [0, 20.0, 3.1], [0, 0, 1]])


def K_for(h, w):
    return sc.default_K() if min(h, w) > 20 else SMALL_K


def example_batch(n, h, w, seed=0, specials=True):
    """n samples of four frames (a1, a2, b1, b2): smooth depth with holes seen by two cameras a few millimetres apart (so that
    the searches find matches), blob masks, random images, foreground records covering all four combinations.  With
    ``specials`` (n >= 5): sample 1 has an empty mask a1, sample 2's object b is fully occluded in frame 2 only (a in front
    there with a full mask a2, b in front in frame 1), sample 3 is marked empty on input.
    -> dict(depth uint16 [4, n, h, w], mask uint8, rgb uint8 [4, n, h, w, 3], cams float32 [2, n, 50], fg int32 [n, 2],
    empty bool [n])"""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    depth, mask = np.zeros((4, n, h, w), np.uint16), np.zeros((4, n, h, w), np.uint8)
    for o in range(2):
        for s in range(n):
            d = 900 + 60 * np.sin(xs / (6 + 4 * rng.rand())) + 50 * np.cos(ys / (5 + 3 * rng.rand()))
            for f in range(2):
                df = d.copy()
                df[rng.rand(h, w) < 0.05] = 0
                depth[2 * o + f, s] = df.astype(np.uint16)
                cy, cx = rng.rand() * h, rng.rand() * w
                mask[2 * o + f, s] = (((ys - cy) / (0.3 * h + 0.6)) ** 2 + ((xs - cx) / (0.3 * w + 0.6)) ** 2) <= 1.0
    rgb = rng.randint(0, 256, size=(4, n, h, w, 3)).astype(np.uint8)
    K = K_for(h, w)
    scale = 1.0 if K is SMALL_K else 0.05           # a shift of about 0.1 pixel in either case
    cams = np.zeros((2, n, 50), np.float32)
    for o in range(2):
        for s in range(n):
            pb = np.eye(4)
            pb[:3, 3] = [-0.004 * scale * (1 + o), -0.003 * scale * (1 + 0.1 * s), 0.0]
            cams[o, s] = sc.cams_of(K, np.eye(4), pb)
    fg = np.array([[FG_A, FG_A], [FG_A, FG_B], [FG_B, FG_A], [FG_B, FG_B]] * ((n + 3) // 4), np.int32)[:n]
    empty = np.zeros(n, bool)
    if specials and n >= 5:
        mask[0, 1] = 0
        fg[2] = [FG_B, FG_A]
        mask[1, 2] = 1
        empty[3] = True
    return dict(depth=depth, mask=mask, rgb=rgb, cams=cams, fg=fg, empty=empty)


def example_draws(n, A, k1, k2, seed=0):
    """Generous replay streams per site and sample, on torch.rand's grid"""
    rng = np.random.RandomState(seed + 100)
    u = lambda m: (rng.randint(0, 1 << 24, size=m).astype(np.float32) / np.float32(1 << 24))
    return {"cand_a": [u(2 * A) for _ in range(n)], "cand_b": [u(2 * A) for _ in range(n)],
            "masked": [u(2 * k1 * 2 * A) for _ in range(n)], "background": [u(2 * k2 * 2 * A) for _ in range(n)]}


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def run_fused(ex, device, A, only_off, k1, k2, inv, draws=None, generator=None, seeds=None, with_rgb=True, with_empty=True):
    from dcn_hip import samples
    return samples.build_synthetic_multi_object_samples(
        _t(ex["depth"].view(np.int16), device), _t(ex["mask"], device), _t(ex["cams"], device),
        _t(ex["rgb"], device) if with_rgb else None, num_matching_attempts=A, sample_matches_only_off_mask=only_off,
        num_masked_non_matches_per_match=k1, num_background_non_matches_per_match=k2, use_image_b_mask_inv=inv, draws=draws,
        generator=generator, seeds=seeds, foreground=_t(ex["fg"], device),
        empty=_t(ex["empty"], device) if with_empty else None)


def fused_draws(ex, draws, only_off):
    """The streams the fused path is given: none at all for a sample marked empty, no ``cand_b`` where object a's search
    finds nothing because mask a1 is empty (candidates off the mask)"""
    out = {k: list(v) for k, v in draws.items()}
    for s in range(ex["empty"].size):
        if ex["empty"][s]:
            for k in out:
                out[k][s] = None
        elif only_off and not ex["mask"][0, s].any():
            out["cand_b"][s] = None
    return out


def training_store(device, h, w, K=None, still_scene=True):
    """Two objects with two scenes of four frames each: a flat wall at 0.9 m (with no-return holes) seen by cameras
    translated in its plane, 0.25 m apart -- except, with ``still_scene``, object 0's second scene, whose four poses are
    equal, so that no image b is found there and the sample arrives empty.  Object 0's mask is a rectangle on the left,
    object 1's one on the right, overlapping in the middle: neither object hides the other completely."""
    from dcn_hip import frames
    rng = np.random.RandomState(0)

    def pose(t):
        T = np.eye(4)
        T[:3, 3] = t
        return T
    moving = [pose(t) for t in ([0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [0.25, 0.25, 0])]
    poses = moving + ([pose([0.1, 0, 0])] * 4 if still_scene else moving) + moving + moving
    F = len(poses)
    depth = np.full((F, h, w), 900, np.uint16)
    depth[rng.rand(F, h, w) < 0.02] = 0
    mask = np.zeros((F, h, w), np.uint8)
    mask[:8, h // 4:3 * h // 4, w // 8:5 * w // 8] = 1
    mask[8:, h // 4:3 * h // 4, 3 * w // 8:7 * w // 8] = 1
    rgb = rng.randint(0, 256, (F, h, w, 3)).astype(np.uint8)
    return frames.FrameStore.from_tensors(_t(rgb, device), _t(depth.view(np.int16), device), _t(mask, device), np.stack(poses),
                                          [0, 4, 8, 12, 16], [0, 0, 1, 1], K)


def training_config(probs, A, non_matches=4):
    p = dict.fromkeys(("SINGLE_OBJECT_WITHIN_SCENE", "SINGLE_OBJECT_ACROSS_SCENE", "DIFFERENT_OBJECT", "MULTI_OBJECT",
                       "SYNTHETIC_MULTI_OBJECT"), 0.0)
    p.update(probs)
    return {"training": dict(num_matching_attempts=A, sample_matches_only_off_mask=True, num_non_matches_per_match=non_matches,
                             fraction_masked_non_matches=0.5, fraction_background_non_matches=0.5, cross_scene_num_samples=20,
                             use_image_b_mask_inv=True, domain_randomize=False, data_type_probabilities=p)}


def run_composition(ex, device, A, only_off, k1, k2, inv, draws):
    """What the existing entry points compose to: build_within_scene_samples per object (the same candidate stream, no
    rotation) -> the match lists unflattened -> merge_synthetic_samples -> complete_samples.  A sample marked empty has
    zero depth, as gather_frames leaves it.  -> (MergedSamples, SampleBatch)"""
    from dcn_hip import merge, samples
    n, h, w = ex["mask"].shape[1:]
    depth = ex["depth"].copy()
    depth[:, ex["empty"]] = 0
    zero = np.zeros((2 * n, 16), np.int32)
    uv, offs = [], []
    for o in range(2):
        r = samples.build_within_scene_samples(
            _t(depth[2 * o].view(np.int16), device), _t(depth[2 * o + 1].view(np.int16), device), _t(ex["mask"][2 * o], device),
            _t(ex["mask"][2 * o + 1], device), None, None, num_matching_attempts=A, sample_matches_only_off_mask=only_off,
            num_masked_non_matches_per_match=1, num_background_non_matches_per_match=1, use_image_b_mask_inv=inv,
            draws={"cand": draws["cand_a" if o == 0 else "cand_b"]}, aug_params=zero, cameras=_t(ex["cams"][o], device))
        off = r.offsets.cpu().numpy()
        ia, ib = r.idx_a.cpu().numpy(), r.idx_b.cpu().numpy()
        la = [ia[off[4 * p]:off[4 * p + 1]] for p in range(n)]
        lb = [ib[off[4 * p]:off[4 * p + 1]] for p in range(n)]
        a, b = np.concatenate(la), np.concatenate(lb)
        uv.append(((_t(a % w, device), _t(a // w, device)), (_t(b % w, device), _t(b // w, device))))
        offs.append(np.concatenate([[0], np.cumsum([len(x) for x in la])]).astype(np.int64))
    m = ex["mask"]
    merged = merge.merge_synthetic_samples(
        _t(ex["rgb"][0], device), _t(ex["rgb"][1], device), _t(ex["rgb"][2], device), _t(ex["rgb"][3], device),
        _t(m[0], device), _t(m[1], device), _t(m[2], device), _t(m[3], device), uv[0][0], uv[0][1], uv[1][0], uv[1][1],
        _t(offs[0], device), _t(offs[1], device), foreground=_t(ex["fg"], device))
    done = samples.complete_samples(merged.uv_1, merged.uv_2, merged.offsets, merged.mask_1.to(torch.uint8),
                                    merged.mask_2.to(torch.uint8), num_masked_non_matches_per_match=k1,
                                    num_background_non_matches_per_match=k2, use_image_b_mask_inv=inv,
                                    draws={"masked": draws["masked"], "background": draws["background"]})
    return merged, done


def check_equals_composition(sb, merged, done):
    n = sb.empty.numel()
    for p in range(n):
        got, want = sc.batch_lists(sb, p), sc.batch_lists(done, p)
        for t in range(6):
            assert np.array_equal(got[t], want[t]), (p, sc.KEYS[t], got[t][:8], want[t][:8], len(got[t]), len(want[t]))
        assert got[6].size == 0 and got[7].size == 0, p                           # no blind list
    off, woff = sb.offsets.cpu().numpy(), done.offsets.cpu().numpy()
    for p in range(n):                                                           # the offsets restricted to lists 0 - 2
        assert np.array_equal(np.diff(off[4 * p:4 * p + 4]), np.diff(woff[4 * p:4 * p + 4])), p
        assert off[4 * p + 4] == off[4 * p + 3]
    assert torch.equal(sb.empty.cpu(), done.empty.cpu()) and torch.equal(sb.type.cpu(), done.type.cpu())
    assert torch.equal(sb.input_a.cpu(), merged.input_1.cpu()) and torch.equal(sb.input_b.cpu(), merged.input_2.cpu())
    assert torch.equal(sb.mask_a.cpu(), merged.mask_1.cpu()) and torch.equal(sb.mask_b.cpu(), merged.mask_2.cpu())


# ---- numpy restatement -------------------------------------------------------------------------------------------------

def _search(depth_1, depth_2, mask_1, cam, A, only_off, U, site):
    """One object's match search -> list of (u, v, int(u2), int(v2)) in candidate order, or None when mask 1 is empty"""
    h, w = mask_1.shape
    if only_off:
        la = np.flatnonzero(mask_1.reshape(-1))
        if la.size == 0:
            return None
        px = [sc._pick(la, U(site, i)) for i in range(A)]
        cand = [(p % w, p // w) for p in px]
    else:
        cand = [(int(np.floor(U(site, i) * np.float32(w))), int(np.floor(U(site, A + i) * np.float32(h)))) for i in range(A)]
    out = []
    for u, v in cand:
        pr = sc._project(depth_1, depth_2, cam, u, v)
        if pr is not None:
            out.append((u, v, int(pr[0]), int(pr[1])))
    return out


def restated_sample(ex, s, A, only_off, k1, k2, inv, U):
    """Sample s -> (the 8 lists, type 4 / -1, kept entries of a, of b as (u1, v1, u2, v2) rows).  U(site, k): the uniform
    numbers of the four sites."""
    depth, mask, cams, fg = ex["depth"], ex["mask"], ex["cams"], ex["fg"]
    h, w = mask.shape[2:]
    z = np.zeros(0, np.int64)
    none = [z] * 8, -1, [], []
    if ex["empty"][s]:
        return none
    kept = []
    for o in range(2):
        found = _search(depth[2 * o, s], depth[2 * o + 1, s], mask[2 * o, s], cams[o, s], A, only_off, U, o)
        if not found:
            return none
        keep = []
        for u1, v1, u2, v2 in found:
            hit = False
            for f, (u, v) in enumerate(((u1, v1), (u2, v2))):
                if (fg[s, f] == FG_B) == (o == 0) and mask[2 * (1 - o) + f, s, v, u] != 0:
                    hit = True
            if not hit:
                keep.append((u1, v1, u2, v2))
        kept.append(keep)
    if not kept[0] or not kept[1]:
        return [z] * 8, -1, kept[0], kept[1]
    rows = np.array(kept[0] + kept[1], np.int64)
    ma, mb = rows[:, 1] * w + rows[:, 0], rows[:, 3] * w + rows[:, 2]
    M = len(ma)
    merged = ((mask[1, s].astype(np.int64) + mask[3, s]).clip(0, 1)).reshape(-1)
    lb, linv = np.flatnonzero(merged), np.flatnonzero(merged == 0)

    def nonmatch(k, site, lst):
        n = M * k
        if lst is not None and lst.size:
            b = [sc._pick(lst, U(site, e)) for e in range(n)]
        else:
            b = [int(np.floor(U(site, n + e) * np.float32(h))) * w + int(np.floor(U(site, e) * np.float32(w))) for e in range(n)]
        return np.repeat(ma, k), np.array(b, np.int64)
    m1a, m1b = nonmatch(k1, 2, lb)
    m2a, m2b = nonmatch(k2, 3, linv if inv else None)
    return [ma, mb, m1a, m1b, m2a, m2b, z, z], 4, kept[0], kept[1]


# ---- golden replay -----------------------------------------------------------------------------------------------------

def golden_example(z):
    d = lambda k: z[k].astype(np.uint16)
    return dict(depth=np.stack([d("depth_" + k) for k in ("a1", "a2", "b1", "b2")])[:, None],
                mask=np.stack([z["mask_" + k] for k in ("a1", "a2", "b1", "b2")])[:, None].astype(np.uint8),
                rgb=np.stack([z["rgb_" + k] for k in ("a1", "a2", "b1", "b2")])[:, None].astype(np.uint8),
                cams=np.stack([sc.cams_of(z["K"], z["pose_a1"], z["pose_a2"]),
                               sc.cams_of(z["K"], z["pose_b1"], z["pose_b2"])])[:, None].astype(np.float32),
                fg=z["foreground"].reshape(1, 2).astype(np.int32), empty=np.zeros(1, bool))


def replay_golden(z, device):
    ex = golden_example(z)
    draws = {k: [z["rand_" + k] if z["rand_" + k].size else None] for k in SITES}
    sb, _ = run_fused(ex, device, int(z["A"]), bool(z["only_off_mask"]), int(z["k1"]), int(z["k2"]), bool(z["inv"]),
                      draws=draws, with_empty=False)
    return sb


def check_golden(sb, z):
    sc.check_golden(sb, 0, z)
    sc.check_layout(sb)
    if int(z["type"]) == -1:
        return
    assert np.array_equal(sb.mask_a[0].cpu().numpy(), z["out_mask_a"].astype(np.float32))
    assert np.array_equal(sb.mask_b[0].cpu().numpy(), z["out_mask_b"].astype(np.float32))
    # the normalized images: EQUAL to the reference's ToTensor + Normalize tensors -- the merge goldens' inputs are checked
    # with torch.equal against that arithmetic too (merge_common.normalize_torch): no tolerance
    for got, k in ((sb.input_a, "out_image_a"), (sb.input_b, "out_image_b")):
        assert torch.equal(got[0].cpu(), torch.from_numpy(z[k])), k
