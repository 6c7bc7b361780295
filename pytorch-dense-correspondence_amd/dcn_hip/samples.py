"""Host side of the sample kernels (csrc/sample_kernels.hip): the training samples of the reference's loader
(dense_correspondence/dataset/spartan_dataset_masked.py get_within_scene_data :577-839, get_across_scene_data :1056-1141) for a
batch of device-resident frames, as the loss's concatenated pair lists.

Within-scene (SINGLE_OBJECT_WITHIN_SCENE, MULTI_OBJECT), per pair: ``num_matching_attempts`` candidates (from mask a, or
uniform), the reprojection test of ``batch_find_pixel_correspondences`` on the unaugmented frames, then the augmentation
(``augment.augment_image_pairs``' records: background randomization of the images, 180-degree rotation of images, masks and
matches), then on the rotated masks the masked / background non-matches (``create_non_correspondences`` +
``create_non_matches``) and the blind non-matches.  A pair whose mask a is empty (with ``sample_matches_only_off_mask``) or
where no match survives is empty: type -1 and no entries, as ``return_empty_data``.  Across-scene (SINGLE_OBJECT_ACROSS_SCENE,
DIFFERENT_OBJECT): ``cross_scene_num_samples`` pixels of each mask, rotated, in the blind slot.  SYNTHETIC_MULTI_OBJECT
(get_synthetic_multi_object_within_scene_data :890-1053, csrc/synthetic_kernels.hip): ``build_synthetic_multi_object_samples``
runs both objects' match searches, the occlusion prune, the non-matches on the merged frame-2 mask and the image merge as one
chain; this type has no augmentation and its blind list is empty.

Masks are 0/1 (uint8, or anything ``.to(uint8)`` maps onto 0/1); other values are outside the contract (include/dcn_hip.h
section 9).  Random numbers are drawn with the caller's generator into per-pair 64-bit seeds (the kernels hash them), or the
reference's own ``torch.rand`` streams are replayed (``draws``).  Nothing here waits for the device, except
``SampleBatch.pair_lists()`` (one read of the offsets; ``SampleBatch.device_lists()`` has none).
"""
import collections

import numpy as np
import torch

from . import _args, _lib
from . import augment as _aug
from .pairgen import invert_rigid

ONLY_OFF_MASK, MASK_INV = 1, 2
BAD_INDEX, BAD_DRAWS, BAD_OFFSETS = 1, 2, 4
CONCAT_MAX_GROUPS = 8
SITES = ("cand", "masked", "background", "blind", "across_a", "across_b")
SYNTHETIC_SITES = ("cand_a", "cand_b", "masked", "background")      # build_synthetic_multi_object_samples' own streams
CAM_FLOATS = _args.CAM_FLOATS
SINGLE_OBJECT_WITHIN_SCENE, SINGLE_OBJECT_ACROSS_SCENE, DIFFERENT_OBJECT, MULTI_OBJECT, SYNTHETIC_MULTI_OBJECT = 0, 1, 2, 3, 4

SampleOptions = collections.namedtuple(
    "SampleOptions", "num_matching_attempts sample_matches_only_off_mask num_masked_non_matches_per_match "
                     "num_background_non_matches_per_match use_image_b_mask_inv cross_scene_num_samples domain_randomize")


class SampleBatch(collections.namedtuple(
        "SampleBatch", "input_a input_b idx_a idx_b offsets empty type status seeds aug_params mask_a mask_b max_list_len "
                       "max_pair_len", defaults=(None, None))):
    """input_a / input_b: float [B, 3, H, W] network inputs (None without RGB); idx_a / idx_b: int64 [capacity] device lists,
    pair p's list t (match, masked, background, blind) at ``offsets[4p+t]:offsets[4p+t+1]``, -1 after ``offsets[4B]``;
    offsets int64 [4B + 1]; empty bool [B]; type int32 [B] (data type, -1 for an empty pair); status int32 [1] (BAD_* bits);
    seeds int64 [B] (None when replayed); aug_params int32 [2B, 16]; mask_a / mask_b: the rotated masks, float 0/1
    [B, H, W] (None without RGB); max_list_len / max_pair_len: host ints, what no list / no pair's four lists can exceed by
    the way the batch was built (None: unknown, the capacity ``idx_a.numel()`` is the bound)."""

    def device_lists(self):
        """A ``dcn_hip.loss.DeviceLists`` over ``idx_a`` / ``idx_b`` / ``offsets`` / ``type`` (no copy) for
        ``loss_composer.get_loss_mixed``: the offsets stay on the device, the launches are shaped by the builders' bounds.
        No host synchronization."""
        from .loss import DeviceLists
        cap = int(self.idx_a.numel())
        return DeviceLists(self.idx_a, self.idx_b, self.offsets, self.type,
                           cap if self.max_list_len is None else self.max_list_len,
                           cap if self.max_pair_len is None else self.max_pair_len)

    def pair_lists(self):
        """A ``dcn_hip.loss.PairLists`` over ``idx_a`` / ``idx_b`` (no copy of the lists).  The loss API takes host offsets:
        this reads the 4B + 1 offsets once, the only host synchronization of the sample path."""
        from .loss import PairLists
        return PairLists(self.idx_a, self.idx_b, self.offsets.cpu().tolist())


def options_from_config(training_config):
    """The sample settings of a training.yaml dict (its ``training`` section, or the whole config), with the reference's
    ``int(fraction * n)`` rounding (dense_correspondence_dataset_masked.py:537-549)."""
    t = training_config.get("training", training_config)
    n = t["num_non_matches_per_match"]
    return SampleOptions(int(t["num_matching_attempts"]), bool(t["sample_matches_only_off_mask"]),
                         int(t["fraction_masked_non_matches"] * n), int(t["fraction_background_non_matches"] * n),
                         bool(t["use_image_b_mask_inv"]), int(t["cross_scene_num_samples"]), bool(t["domain_randomize"]))


def _cameras(K, pose_a, pose_b, n, dev):
    """[n, CAM_FLOATS] fp32 (K, K^-1, pose a, pose b^-1) on ``dev`` in one copy, as pairgen.find_correspondences builds them."""
    rows = torch.from_numpy(_args.camera_k_rows(K, n)[1])
    poses = []
    for p, what in ((pose_a, "pose_a"), (pose_b, "pose_b")):
        if tuple(p.shape) != (n, 4, 4):
            raise ValueError("%s must be [%d, 4, 4], got %s" % (what, n, tuple(p.shape)))
        poses.append(p)
    if all(not torch.is_tensor(p) or p.device.type == "cpu" for p in poses):
        pa = np.asarray(poses[0].numpy() if torch.is_tensor(poses[0]) else poses[0], dtype=np.float64)
        pb = np.asarray(poses[1].numpy() if torch.is_tensor(poses[1]) else poses[1], dtype=np.float64)
        t = np.concatenate([rows.numpy(), _args.f32(pa).reshape(n, 16), np.stack([_args.f32(invert_rigid(x)).reshape(16) for x in pb])],
                           axis=1)
        host = torch.from_numpy(np.ascontiguousarray(t))
        if dev.type == "cuda":
            host = host.pin_memory()
        return host.to(dev, non_blocking=True)
    # device poses: the rigid inverse in float64 on the device (no host round trip)
    pa = torch.as_tensor(poses[0], device=dev).double()
    pb = torch.as_tensor(poses[1], device=dev).double()
    R = pb[:, :3, :3].transpose(1, 2)
    inv = torch.zeros_like(pb)
    inv[:, :3, :3] = R
    inv[:, :3, 3] = -(R @ pb[:, :3, 3:4]).squeeze(2)
    inv[:, 3, 3] = 1.0
    k = rows.to(dev, non_blocking=True)
    return torch.cat([k, pa.float().reshape(n, 16), inv.float().reshape(n, 16)], dim=1).contiguous()


def draw_seeds(num_pairs, device, generator=None):
    """[num_pairs] int64 seeds on ``device`` (two int32 draws each), no host sync."""
    return torch.randint(-2 ** 31, 2 ** 31, (num_pairs, 2), device=device, generator=generator,
                         dtype=torch.int32).view(torch.int64).view(-1)


def pack_draws(draws, n, dev, sites=SITES):
    """``draws``: {site: sequence of B 1-D float arrays / tensors (None = no values)} -> (rand float32, rand_offsets int64
    [sites][B + 1]) on ``dev``: the replay layout of include/dcn_hip.h section 9 (``sites=SYNTHETIC_SITES``: of section 9a,
    see pack_synthetic_draws)."""
    vals, offs, pos = [], [], 0
    for site in sites:
        per = draws.get(site) or [None] * n
        if len(per) != n:
            raise ValueError("draws[%r] needs one entry per pair (%d), got %d" % (site, n, len(per)))
        row = [pos]
        for x in per:
            a = np.zeros(0, np.float32) if x is None else np.asarray(x.cpu() if torch.is_tensor(x) else x,
                                                                      dtype=np.float32).reshape(-1)
            vals.append(a)
            pos += a.size
            row.append(pos)
        offs.append(row)
    unknown = set(draws) - set(sites)
    if unknown:
        raise ValueError("unknown draw sites %s (sites: %s)" % (sorted(unknown), sites))
    rand = torch.from_numpy(np.concatenate(vals + [np.zeros(1, np.float32)]))
    return rand.to(dev), torch.tensor(offs, dtype=torch.int64).to(dev)


def pack_synthetic_draws(draws, n, dev):
    """pack_draws for the four streams of build_synthetic_multi_object_samples: ``cand_a`` / ``cand_b`` (the reference's
    torch.rand calls of object a's and object b's match search; ``cand_b`` may be None for a sample whose object a search
    finds nothing), ``masked``, ``background`` -> (rand, rand_offsets int64 [4][B + 1]), include/dcn_hip.h section 9a."""
    return pack_draws(draws, n, dev, SYNTHETIC_SITES)


def random_source(n, dev, generator, draws, seeds, sites=SITES):
    """-> (seeds, rand, rand_offsets): the replay streams of ``draws`` (pack_draws) and no seeds, or per-pair seeds (the
    caller's, or drawn with ``generator``) and no streams."""
    if draws is not None:
        rand, roff = pack_draws(draws, n, dev, sites)
        return None, rand, roff
    return _args.seeds_for(n, dev, generator, seeds), None, None


def _params(aug_params, n, dev, generator, domain_randomize, flip):
    if aug_params is None:
        return _aug.draw_params(2 * n, dev, generator=generator, domain_randomize=domain_randomize, flip=flip)
    p = torch.as_tensor(aug_params).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(p.shape) != (2 * n, _aug.PARAM_WORDS):
        raise ValueError("aug_params must be int32 [%d, %d], got %s" % (2 * n, _aug.PARAM_WORDS, tuple(p.shape)))
    return p


def _open(mask_a, mask_b):
    """What every builder starts from: the batch's sizes and device (mask a's) and both masks as the kernels take them."""
    n, h, w = int(mask_a.shape[0]), int(mask_a.shape[1]), int(mask_a.shape[2])
    return n, h, w, mask_a.device, _args.mask(mask_a, n, h, w, "mask_a"), _args.mask(mask_b, n, h, w, "mask_b")


def _outputs(n, cap, dev, workspace_bytes):
    """idx_a, idx_b [cap], offsets [4n + 1], empty [n], type [n], status [1] and the workspace"""
    return (torch.empty(max(cap, 1), dtype=torch.int64, device=dev)[:cap], torch.empty(max(cap, 1), dtype=torch.int64,
                                                                                       device=dev)[:cap],
            torch.empty(4 * n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.bool, device=dev),
            torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev),
            torch.empty(int(workspace_bytes), dtype=torch.uint8, device=dev))


def _batch(outs, sd, params, max_list_len, max_pair_len, rgb_a=None, rgb_b=None, mask_a=None, mask_b=None, mean=None, std=None):
    """The SampleBatch of a builder's outputs and, with RGB, the augmentation launch that writes the network's inputs."""
    ia = ib = mka = mkb = None
    if (rgb_a is None) != (rgb_b is None):
        raise ValueError("rgb_a and rgb_b go together")
    if rgb_a is not None:
        out = _aug.augment_images(rgb_a, mask_a, params, rgb_b=rgb_b, mask_b=mask_b, mean=mean, std=std)
        ia, ib, mka, mkb = out["input_a"], out["input_b"], out["mask_a"], out["mask_b"]
    return SampleBatch(ia, ib, *outs[:6], sd, params, mka, mkb, max_list_len, max_pair_len)


def build_within_scene_samples(depth_a, depth_b, mask_a, mask_b, pose_a, pose_b, K=None, rgb_a=None, rgb_b=None, *,
                               num_matching_attempts, sample_matches_only_off_mask, num_masked_non_matches_per_match,
                               num_background_non_matches_per_match, use_image_b_mask_inv, domain_randomize=False, flip=True,
                               mean=_aug.DEFAULT_IMAGE_MEAN, std=_aug.DEFAULT_IMAGE_STD_DEV, generator=None, draws=None,
                               aug_params=None, seeds=None, data_type=SINGLE_OBJECT_WITHIN_SCENE, cameras=None):
    """B within-scene samples on the device (get_within_scene_data).

    depth_a, depth_b: 16-bit [B, H, W] millimetres (int16 / uint16, same bits); mask_a, mask_b: 0/1 [B, H, W]; pose_a, pose_b:
    [B, 4, 4] camera-to-world (host or device); K: [3, 3] or [B, 3, 3] on the host (None: the reference's default K);
    rgb_a, rgb_b: optional uint8 [B, H, W, 3] -> normalized network inputs of the augmented images.  ``aug_params``: [2B, 16]
    augmentation records (augment.draw_params layout) to replay, otherwise drawn with ``generator`` (``domain_randomize``,
    ``flip``).  ``draws``: the reference's torch.rand streams per site and pair (replay; see pack_draws), otherwise per-pair
    ``seeds`` (drawn with ``generator`` when None).  ``cameras``: the camera rows [B, 50] fp32 on the device (K, K^-1, pose a,
    pose b^-1, e.g. frames.FrameBatch.cams[0]) in place of K / pose_a / pose_b, which are then not read.

    -> SampleBatch.  Launches: the sample chain (about ten small kernels) and, with RGB, one augmentation launch; no host
    synchronization."""
    lib = _lib.get()
    n, h, w, dev, ma, mb = _open(mask_a, mask_b)
    da, db = _args.depth(depth_a, n, h, w, "depth_a"), _args.depth(depth_b, n, h, w, "depth_b")
    A, k1, k2 = int(num_matching_attempts), int(num_masked_non_matches_per_match), int(num_background_non_matches_per_match)
    if A < 1 or k1 < 1 or k2 < 1:
        raise ValueError("num_matching_attempts and the non-matches per match must be >= 1")
    params = _params(aug_params, n, dev, generator, domain_randomize, flip)
    sd, rand, roff = random_source(n, dev, generator, draws, seeds)
    cams = _cameras(K, pose_a, pose_b, n, dev) if cameras is None else _args.camera_rows(cameras, n, "cameras", as_given=True)
    _lib.require_device(da, db, ma, mb, cams, params, sd, rand, roff)
    cap = n * (A * (1 + k1 + k2) + h * w)
    outs = _outputs(n, cap, dev, lib.dcn_sample_workspace(n, h, w, A, A))
    idx_a, idx_b, offsets, empty, typ, status, ws = outs
    flags = (ONLY_OFF_MASK if sample_matches_only_off_mask else 0) | (MASK_INV if use_image_b_mask_inv else 0)
    P = _lib.ptr
    rc = lib.dcn_within_scene_samples(n, h, w, P(da), P(db), P(ma), P(mb), P(cams), A, k1, k2, flags, P(params), P(sd),
                                      P(rand), P(roff), int(data_type), P(idx_a), P(idx_b), cap, P(offsets), P(empty),
                                      P(typ), P(status), P(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_within_scene_samples")
    return _batch(outs, sd, params, max(A, A * k1, A * k2, h * w), cap // n, rgb_a, rgb_b, ma, mb, mean, std)


def build_across_scene_samples(mask_a, mask_b, rgb_a=None, rgb_b=None, *, num_samples, domain_randomize=False, flip=True,
                               mean=_aug.DEFAULT_IMAGE_MEAN, std=_aug.DEFAULT_IMAGE_STD_DEV, generator=None, draws=None,
                               aug_params=None, seeds=None, data_type=SINGLE_OBJECT_ACROSS_SCENE):
    """B across-scene / different-object samples on the device (get_across_scene_data): ``num_samples`` pixels of each mask,
    rotated by the pair's records, as the blind lists; a pair with an empty mask is empty.  Arguments as
    build_within_scene_samples; -> SampleBatch."""
    lib = _lib.get()
    n, h, w, dev, ma, mb = _open(mask_a, mask_b)
    ns = int(num_samples)
    if ns < 1:
        raise ValueError("num_samples must be >= 1")
    params = _params(aug_params, n, dev, generator, domain_randomize, flip)
    sd, rand, roff = random_source(n, dev, generator, draws, seeds)
    _lib.require_device(ma, mb, params, sd, rand, roff)
    cap = n * ns
    outs = _outputs(n, cap, dev, lib.dcn_sample_workspace(n, h, w, 0, 0))
    idx_a, idx_b, offsets, empty, typ, status, ws = outs
    P = _lib.ptr
    rc = lib.dcn_across_scene_samples(n, h, w, P(ma), P(mb), ns, P(params), P(sd), P(rand), P(roff), int(data_type), P(idx_a),
                                      P(idx_b), cap, P(offsets), P(empty), P(typ), P(status), P(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_across_scene_samples")
    return _batch(outs, sd, params, ns, ns, rgb_a, rgb_b, ma, mb, mean, std)


def complete_samples(uv_a, uv_b, offsets, mask_a, mask_b, *, num_masked_non_matches_per_match,
                     num_background_non_matches_per_match, use_image_b_mask_inv, generator=None, draws=None, seeds=None,
                     aug_params=None, data_type=SYNTHETIC_MULTI_OBJECT):
    """Non-matches and blind non-matches for match lists found elsewhere, e.g. merge.merge_synthetic_samples' uv_1 / uv_2
    and merged masks: uv_a (int64) / uv_b (int64 or float32) ``(u, v)`` lists, pair p at ``offsets[p]:offsets[p+1]``
    ([B + 1] tensor or sequence; a -1 capacity tail after offsets[B] is ignored); mask_a, mask_b: 0/1 [B, H, W] of the
    frames the lists index.  ``aug_params`` (optional): rotation records to apply to lists and masks first.  A pair without
    matches is empty.  -> SampleBatch (no images)."""
    lib = _lib.get()
    n, h, w, dev, ma, mb = _open(mask_a, mask_b)
    ua, va = uv_a[0].contiguous(), uv_a[1].contiguous()
    ub, vb = uv_b[0].contiguous(), uv_b[1].contiguous()
    if ua.dtype != torch.int64 or va.dtype != torch.int64 or ub.dtype != vb.dtype or len({int(x.numel()) for x in
                                                                                          (ua, va, ub, vb)}) != 1:
        raise ValueError("uv_a must be int64, uv_b int64 or float32, all four lists of one length")
    uv_b_dtype = _args.uv_dtype(ub)
    off = _args.offsets(offsets, n, dev)
    k1, k2 = int(num_masked_non_matches_per_match), int(num_background_non_matches_per_match)
    if k1 < 1 or k2 < 1:
        raise ValueError("the non-matches per match must be >= 1")
    params = None if aug_params is None else _params(aug_params, n, dev, None, False, True)
    sd, rand, roff = random_source(n, dev, generator, draws, seeds)
    _lib.require_device(ua, va, ub, vb, off, ma, mb, params, sd, rand, roff)
    count = int(ua.numel())
    cap = count * (1 + k1 + k2) + n * h * w
    outs = _outputs(n, cap, dev, lib.dcn_sample_workspace(n, h, w, 0, count))
    idx_a, idx_b, offsets_out, empty, typ, status, ws = outs
    P = _lib.ptr
    rc = lib.dcn_complete_samples(n, h, w, P(ua), P(va), P(ub), P(vb), uv_b_dtype, P(off), count, P(ma), P(mb), k1, k2,
                                  MASK_INV if use_image_b_mask_inv else 0, P(params), P(sd), P(rand), P(roff), int(data_type),
                                  P(idx_a), P(idx_b), cap, P(offsets_out), P(empty), P(typ), P(status), P(ws),
                                  _lib.stream_ptr())
    _lib.check(rc, "dcn_complete_samples")
    return _batch(outs, sd, params, max(count, count * k1, count * k2, h * w), count * (1 + k1 + k2) + h * w)


def build_synthetic_multi_object_samples(depth, mask, cameras, rgb=None, *, num_matching_attempts,
                                         sample_matches_only_off_mask, num_masked_non_matches_per_match,
                                         num_background_non_matches_per_match, use_image_b_mask_inv, generator=None, draws=None,
                                         seeds=None, foreground=None, empty=None, mean=_aug.DEFAULT_IMAGE_MEAN,
                                         std=_aug.DEFAULT_IMAGE_STD_DEV):
    """B SYNTHETIC_MULTI_OBJECT samples on the device (get_synthetic_multi_object_within_scene_data,
    spartan_dataset_masked.py:890-1053) in one chain: the within-scene match search for object a (frames a1 -> a2) and for
    object b (b1 -> b2) on the unaugmented frames, the occlusion prune and concatenation of merge.merge_synthetic_samples
    (a's kept matches, then b's), the masked / background non-matches on the merged frame-2 mask, and the merged images.
    The per-object non-matches that a composition of build_within_scene_samples would build and drop are never made.

    depth 16-bit [4, B, H, W], mask 0/1 [4, B, H, W], rgb uint8 [4, B, H, W, 3] (optional) in the slot order a1, a2, b1, b2
    and cameras fp32 [2, B, 50] (row 0: a1 -> a2, row 1: b1 -> b2), as frames.select_frames(...,
    SYNTHETIC_MULTI_OBJECT) returns them.  ``foreground``: [B, 2] records (merge.FG_A / FG_B per frame) to replay, otherwise
    merge.draw_foreground(B, device, generator).  ``empty``: bool [B] (FrameBatch.empty), samples that come out empty without
    reading a random number.  ``draws``: replay streams per site of SYNTHETIC_SITES (pack_synthetic_draws), otherwise
    per-sample ``seeds`` (drawn with ``generator`` when None).

    -> (SampleBatch, foreground).  input_a / input_b: the merged normalized images of frame 1 / frame 2 and mask_a / mask_b
    the merged masks as float 0/1 (None without ``rgb``); type 4 or -1; the BLIND list of every sample is EMPTY, as the
    reference returns empty tensors for it; aug_params None (this type is not augmented); max_list_len / max_pair_len
    from the capacity B * 2A * (1 + k_masked + k_background).  Twelve launches with images and candidates off the mask; no
    host synchronization."""
    from . import merge as _merge
    lib = _lib.get()
    if mask is None or mask.dim() != 4 or int(mask.shape[0]) != 4:
        raise ValueError("mask must be [4, B, H, W] (a1, a2, b1, b2), got %s" % (None if mask is None else tuple(mask.shape),))
    n, h, w, dev = int(mask.shape[1]), int(mask.shape[2]), int(mask.shape[3]), mask.device
    if n < 1 or n > 1024:
        raise ValueError("1 <= B <= 1024 samples per call, got %d" % n)
    mk = _args.mask(mask.reshape(4 * n, h, w), 4 * n, h, w, "mask")
    if tuple(depth.shape) != (4, n, h, w):
        raise ValueError("depth must be 16-bit integer [4, %d, %d, %d], got %s" % (n, h, w, tuple(depth.shape)))
    dp = _args.depth(depth.reshape(4 * n, h, w), 4 * n, h, w, "depth")
    if tuple(cameras.shape) != (2, n, CAM_FLOATS):
        raise ValueError("cameras must be float32 [2, %d, %d], got %s" % (n, CAM_FLOATS, tuple(cameras.shape)))
    cams = _args.camera_rows(cameras.reshape(2 * n, CAM_FLOATS), 2 * n, "cameras")
    img = None
    if rgb is not None:
        if tuple(rgb.shape) != (4, n, h, w, 3):
            raise ValueError("rgb must be uint8 [4, %d, %d, %d, 3], got %s" % (n, h, w, tuple(rgb.shape)))
        img = _args.image(rgb.reshape(4 * n, h, w, 3), 4 * n, h, w, "rgb")
    A, k1, k2 = int(num_matching_attempts), int(num_masked_non_matches_per_match), int(num_background_non_matches_per_match)
    if A < 1 or k1 < 1 or k2 < 1:
        raise ValueError("num_matching_attempts and the non-matches per match must be >= 1")
    fg = _merge.draw_foreground(n, dev, generator=generator) if foreground is None else _merge._foreground(foreground, n, dev)
    em = None
    if empty is not None:
        if tuple(empty.shape) != (n,):
            raise ValueError("empty must be [%d], got %s" % (n, tuple(empty.shape)))
        em = empty.to(torch.bool).contiguous()
    sd, rand, roff = random_source(n, dev, generator, draws, seeds, SYNTHETIC_SITES)
    _lib.require_device(dp, mk, img, cams, fg, em, sd, rand, roff)
    cap = n * 2 * A * (1 + k1 + k2)
    outs = _outputs(n, cap, dev, lib.dcn_synthetic_workspace(n, h, w, A))
    idx_a, idx_b, offsets, empty_out, typ, status, ws = outs
    net = msk = (None, None)
    m = s = None
    if img is not None:
        net = tuple(torch.empty(n, 3, h, w, dtype=torch.float32, device=dev) for _ in range(2))
        msk = tuple(torch.empty(n, h, w, dtype=torch.float32, device=dev) for _ in range(2))
        m, s = _args.mean_std(mean), _args.mean_std(std)
    flags = (ONLY_OFF_MASK if sample_matches_only_off_mask else 0) | (MASK_INV if use_image_b_mask_inv else 0)
    P = _lib.ptr
    rc = lib.dcn_synthetic_samples(n, h, w, P(dp), P(mk), P(img), P(cams), A, k1, k2, flags, P(fg), P(em), P(sd), P(rand),
                                   P(roff), None if m is None else _lib.host_ptr(m), None if s is None else _lib.host_ptr(s),
                                   P(net[0]), P(net[1]), P(msk[0]), P(msk[1]), P(idx_a), P(idx_b), cap, P(offsets),
                                   P(empty_out), P(typ), P(status), P(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_synthetic_samples")
    return SampleBatch(net[0], net[1], *outs[:6], sd, None, msk[0], msk[1], 2 * A * max(1, k1, k2), cap // n), fg


def _cat(parts):
    return None if any(x is None for x in parts) else torch.cat(parts)


def concat_sample_batches(batches):
    """SampleBatches of one image size -- e.g. one per data type -- as ONE SampleBatch of B = sum of their sizes, pairs in
    the order given: ``idx_a`` / ``idx_b`` compacted (pair p's four lists at ``offsets[4p+t]``, -1 after ``offsets[4B]``),
    ``type`` / ``empty`` / ``seeds`` / ``aug_params`` / inputs / masks concatenated (None when a batch has none), ``status``
    OR-ed (| BAD_OFFSETS for a batch whose offsets are not the builders' layout; its pairs then have empty lists), the bounds the
    largest of the batches'.  Two launches and the concatenations; no host synchronization."""
    batches = list(batches)
    if not batches:
        raise ValueError("concat_sample_batches needs at least one SampleBatch")
    lib = _lib.get()
    G = len(batches)
    if G > CONCAT_MAX_GROUPS:
        raise ValueError("at most %d batches are joined in one call, got %d" % (CONCAT_MAX_GROUPS, G))
    dev = batches[0].idx_a.device
    ns = [int(b.type.numel()) for b in batches]
    caps = [int(b.idx_a.numel()) for b in batches]
    if len({tuple(x.shape[-2:]) for b in batches for x in (b.input_a, b.mask_a) if x is not None}) > 1:
        raise ValueError("concat_sample_batches: the batches' images differ in size")
    src_a = [b.idx_a.contiguous() for b in batches]
    src_b = [b.idx_b.contiguous() for b in batches]
    src_o = [b.offsets.contiguous() for b in batches]
    src_s = [b.status for b in batches]
    _lib.require_device(*(src_a + src_b + src_o + src_s))
    n, cap = sum(ns), sum(caps)
    idx_a = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)[:cap]
    idx_b = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)[:cap]
    offsets = torch.empty(4 * n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    arr = lambda ts: (_lib.c_void_p * G)(*[None if t is None else t.data_ptr() for t in ts])
    rc = lib.dcn_concat_samples(G, (_lib.c_int * G)(*ns), arr(src_a), arr(src_b), arr(src_o), (_lib.c_int64 * G)(*caps),
                                arr(src_s), _lib.ptr(idx_a), _lib.ptr(idx_b), cap, _lib.ptr(offsets), _lib.ptr(status),
                                _lib.stream_ptr())
    _lib.check(rc, "dcn_concat_samples")
    params = None
    if all(b.aug_params is not None for b in batches):      # [2B, 16]: a's records first, then b's
        params = torch.cat([b.aug_params[:k] for b, k in zip(batches, ns)] + [b.aug_params[k:] for b, k in zip(batches, ns)])
    bound = lambda k: None if any(getattr(b, k) is None for b in batches) else max(getattr(b, k) for b in batches)
    return SampleBatch(_cat([b.input_a for b in batches]), _cat([b.input_b for b in batches]), idx_a, idx_b, offsets,
                       torch.cat([b.empty for b in batches]), torch.cat([b.type for b in batches]), status,
                       _cat([b.seeds for b in batches]), params, _cat([b.mask_a for b in batches]),
                       _cat([b.mask_b for b in batches]), bound("max_list_len"), bound("max_pair_len"))
