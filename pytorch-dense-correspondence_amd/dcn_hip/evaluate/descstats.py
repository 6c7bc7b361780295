"""The descriptor statistics of a dataset (csrc/descstats_kernels.hip): ``compute_descriptor_statistics_on_dataset``
(evaluation.py:2157-2304)."""
import os

import numpy as np
import torch

from .. import _args, _lib
from .. import augment as _aug
from ._chain import (_below, _descriptor_images, _forward_in_eval_mode, _gather_frame_list, _lots, _on_device,
                     _random_scene)

def descriptor_statistics(res, mask):
    """``compute_descriptor_statistics`` (evaluation.py:2177-2219) for n descriptor images in ONE pass over ``res`` and ``mask``.

    res: float32 [n, H, W, D] descriptor images, channel last, as ``forward_image_tensors`` returns them (D = 1 .. 64); mask:
    uint8 or bool [n, H, W] (non-zero = on the object).
    -> (per_image float32 [n, 2, 3, D]: axis 1 entire image, mask; axis 2 min, max, mean; mask_pixels int32 [n]).  Sums in
    float64, the mean rounded to float32 once; bit-identical from run to run; NaN as in torch (a NaN in a channel makes its
    min, max and mean NaN; for the mask rows only a NaN under the mask); an empty mask gives mask_pixels 0 and NaN mask rows.
    No host synchronization."""
    lib = _lib.get()
    if not torch.is_tensor(res) or not torch.is_tensor(mask):
        raise ValueError("res and mask must be tensors")
    if res.dim() != 4:
        raise ValueError("res must be [n, H, W, D], got %s" % (tuple(res.shape),))
    r, n, h, w, d = _descriptor_images(res, "res", max_images=65535)
    if mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError("mask must be uint8 (or bool), got %s" % mask.dtype)
    m = _args.mask(mask, n, h, w, "mask")
    _on_device(r, m)
    if r.device != m.device:
        raise ValueError("res and mask must be on one device, got %s and %s" % (r.device, m.device))
    dev = r.device
    per_image = torch.empty((n, 2, 3, d), dtype=torch.float32, device=dev)
    mask_pixels = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(max(1, int(lib.dcn_descriptor_statistics_workspace(n, h, w, d))), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = lib.dcn_descriptor_statistics(n, h, w, d, p(r), p(m), p(per_image), p(mask_pixels), p(ws), _lib.stream_ptr())
    _lib.check(rc, "dcn_descriptor_statistics")
    return per_image, mask_pixels


def combine_descriptor_statistics(per_image, mask_pixels, num_images=None):
    """The reference's ``update_stats`` loop and final scaling (evaluation.py:2237-2292) over ``descriptor_statistics``'
    outputs (per_image float32 [N, 2, 3, D], mask_pixels int32 [N]) in one launch: images with an empty mask are skipped for
    both sets of statistics, min / max over the images used, mean = the float32 sum of their means in image order times
    float32(1.0 / num_images) -- ``num_images`` (default N), not the number used, as in the reference.
    -> (stats float32 [2, 3, D], used int32 [1]); ``stats`` is NaN when no image was used.  No host synchronization."""
    lib = _lib.get()
    if not torch.is_tensor(per_image) or per_image.dim() != 4 or tuple(per_image.shape[1:3]) != (2, 3) \
            or per_image.dtype != torch.float32:
        raise ValueError("per_image must be float32 [N, 2, 3, D]")
    N, d = int(per_image.shape[0]), int(per_image.shape[3])
    if N < 1 or d < 1 or d > 64:
        raise ValueError("per_image must hold N >= 1 images of 1 .. 64 channels, got %s" % (tuple(per_image.shape),))
    if not torch.is_tensor(mask_pixels) or mask_pixels.dtype != torch.int32 or tuple(mask_pixels.shape) != (N,):
        raise ValueError("mask_pixels must be int32 [%d]" % N)
    num = N if num_images is None else int(num_images)
    if num < 1:
        raise ValueError("num_images must be >= 1, got %d" % num)
    pi, mp = per_image.contiguous(), mask_pixels.contiguous()
    _on_device(pi, mp)
    dev = pi.device
    stats = torch.empty((2, 3, d), dtype=torch.float32, device=dev)
    used = torch.empty(1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    rc = lib.dcn_descriptor_statistics_combine(N, d, p(pi), p(mp), num, p(stats), p(used), _lib.stream_ptr())
    _lib.check(rc, "dcn_descriptor_statistics_combine")
    return stats, used


def choose_frames(store, num_images, host_rng=None):
    """``num_images`` times the rule of ``get_random_rgbd_mask_pose`` (spartan_dataset_masked.py:410-421), on the host: a scene
    by ``get_random_scene_name`` (as ``choose_pairs``), then a frame uniform over that scene's frames.  As in ``choose_pairs``
    the rule is replayed, not the reference's random stream (it draws the scene and the image twice, :418-419).
    ``host_rng``: a numpy RandomState / Generator (default ``np.random``).
    -> int64 array [num_images, 2] of (scene, frame), frames as store indices."""
    rng = host_rng if host_rng is not None else np.random
    first = store.scene_first_frame_host
    lots = _lots(store)
    out = []
    for _ in range(int(num_images)):
        s = _random_scene(store, rng, lots)
        out.append((s, first[s] + _below(rng, first[s + 1] - first[s])))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


STAT_SETS, STAT_FIELDS = ("entire_image", "mask_image"), ("min", "max", "mean")


def compute_descriptor_statistics_on_dataset(dcn, store, num_images=100, save_to_file=True, filename=None, host_rng=None,
                                             batch_images=16):
    """``DenseCorrespondenceEvaluation.compute_descriptor_statistics_on_dataset`` (evaluation.py:2157-2304) on a frame store:
    1. choose_frames, 2. ONE ``dcn_gather_frames`` of their images and masks, 3. ToTensor + Normalize by the augmentation kernel
    with every augmentation switched off (the dataset's mean and standard deviation, as ``evaluate_frame_pairs``), 4. ``dcn.forward_image_tensors`` in eval mode,
    ``batch_images`` images at a time, 5. descriptor_statistics per batch into slices of one [num_images, 2, 3, D] tensor,
    6. one combine_descriptor_statistics launch, 7. ONE copy to the host.
    -> the reference's dict {'entire_image': {'min': [...], 'max': [...], 'mean': [...]}, 'mask_image': {...}} of lists of
    Python floats, written with ``utils.saveToYaml`` when ``save_to_file`` -- to ``filename``, by default
    ``<dcn's network params folder>/descriptor_statistics.yaml``, the file ``dcn.descriptor_image_stats`` reads.  ValueError
    when every chosen frame's mask was empty (the reference fails on ``None.tolist()``).  ``dcn.training`` is left as found."""
    n = int(num_images)
    step = int(batch_images)
    if n < 1 or n > 65534:
        raise ValueError("num_images must be 1 .. 65534, got %d" % n)
    if step < 1:
        raise ValueError("batch_images must be >= 1")
    if save_to_file and filename is None:                   # (before any work: a network without the folder cannot save)
        import dense_correspondence_manipulation.utils.utils as utils
        filename = os.path.join(utils.convert_to_absolute_path(dcn.path_to_network_params_folder),
                                "descriptor_statistics.yaml")
    chosen = choose_frames(store, n, host_rng)
    dev = store.device
    rgb, _, mask, bad_frame = _gather_frame_list(store, chosen[:, 1], ("rgb", "mask"))
    out = []

    def statistics(lo, k, res):
        if not out:
            out.extend([torch.empty((n, 2, 3, int(res.shape[3])), dtype=torch.float32, device=dev),
                        torch.empty(n, dtype=torch.int32, device=dev)])
        out[0][lo:lo + k], out[1][lo:lo + k] = descriptor_statistics(res, mask[lo:lo + k])
    _forward_in_eval_mode(dcn, rgb, mask, None, None, step, _aug.DEFAULT_IMAGE_MEAN, _aug.DEFAULT_IMAGE_STD_DEV, statistics)
    stats, used = combine_descriptor_statistics(out[0], out[1], n)
    # one transfer: the statistics, the number of images used and the gather's status word in one float64 block
    block = torch.cat([stats.double().view(-1), used.double(), bad_frame.double()]).cpu().numpy()
    if int(block[-1]) != 0:
        raise RuntimeError("dcn_hip: the frame gather rejected a frame index (status %d)" % int(block[-1]))
    if int(block[-2]) == 0:
        raise ValueError("every one of the %d chosen frames has an empty mask: no descriptor statistics" % n)
    table = block[:-2].reshape(2, 3, -1)
    out = {s: {f: [float(v) for v in table[i, j]] for j, f in enumerate(STAT_FIELDS)} for i, s in enumerate(STAT_SETS)}
    if save_to_file:
        import dense_correspondence_manipulation.utils.utils as utils
        utils.saveToYaml(out, filename)
    return out
