"""Host side of the frame-store kernels (csrc/frame_kernels.hip): a training set's frames kept in device memory, the
reference loader's frame choice for a batch of pairs (dense_correspondence/dataset/spartan_dataset_masked.py: the type wrappers
:543-575, :860-905 and their helpers :408-502; dense_correspondence_dataset_masked.py get_img_idx_with_different_pose
:260-287), the gather of the chosen frames into batch tensors, and a whole training batch drawn from the store.

A ``FrameStore`` is built once (``from_dataset`` reads every frame through the dataset's own ``get_rgbd_mask_pose``).  From
then on ``select_frames`` chooses and gathers a batch in two launches, and ``draw_training_batch`` feeds the result to the
sample builders of ``samples``: no decode, no host-to-device copy and no host synchronization per batch.  Random numbers are
drawn with the caller's generator into per-pair 64-bit seeds (the kernel hashes them), or the reference's own draws are
replayed (``draws``: the positions its ``random.choice`` / ``np.random.choice`` calls returned, include/dcn_hip.h section 10).
"""
import collections
import ctypes

import numpy as np
import torch

from . import _args, _lib
from .samples import (CAM_FLOATS, DIFFERENT_OBJECT, MULTI_OBJECT, SINGLE_OBJECT_ACROSS_SCENE, SINGLE_OBJECT_WITHIN_SCENE,
                      SYNTHETIC_MULTI_OBJECT, build_across_scene_samples, build_synthetic_multi_object_samples,
                      build_within_scene_samples, concat_sample_batches, options_from_config)

BAD_INDEX, BAD_DRAWS, NO_CANDIDATES = 1, 2, 4
SLOTS = 4
DRAW_WORDS = ("object_a", "object_b", "scene_a", "scene_b", "scene_b2", "frame_a", "frame_b")
DRAW_HEADER = 8
TYPE_NAMES = ("SINGLE_OBJECT_WITHIN_SCENE", "SINGLE_OBJECT_ACROSS_SCENE", "DIFFERENT_OBJECT", "MULTI_OBJECT",
              "SYNTHETIC_MULTI_OBJECT")


class FrameBatch(collections.namedtuple(
        "FrameBatch", "data_type frames empty scenes objects status seeds rgb depth mask cams")):
    """frames int32 [B, 4] store frame indices (a, b, -1, -1; a1, a2, b1, b2 for SYNTHETIC_MULTI_OBJECT); empty bool [B] (no
    image b with a different enough pose: frame b is frame a); scenes / objects int32 [B, 2] (of a / a1 and of b / b1; object
    -1 for a multi-object scene); status int32 [1] (BAD_INDEX | BAD_DRAWS | NO_CANDIDATES); seeds int64 [B] (None when
    replayed).  Gathered (None with ``gather=False``): rgb uint8 [k, B, H, W, 3], depth int16 [k, B, H, W] (millimetres,
    uint16 bits; zero for an empty pair), mask uint8 [k, B, H, W] with k = 2 (a, b) or 4 (a1, a2, b1, b2); cams fp32
    [k / 2, B, 50], the camera rows of samples.build_within_scene_samples (K, K^-1, pose a, pose b^-1)."""


def _host_ints(x, what):
    a = np.asarray(x.cpu() if torch.is_tensor(x) else x)
    if a.ndim != 1 or not (a.size == 0 or np.issubdtype(a.dtype, np.integer)):
        raise ValueError("%s must be a 1-D integer sequence" % what)
    return [int(v) for v in a]


class FrameStore(object):
    """The frames and tables of one mode's scenes on one device (include/dcn_hip.h section 10).  Build it with
    ``from_tensors`` or ``from_dataset``.  ``K``: float64 [S, 3, 3] on the host.  Scenes are numbered in the reference's order: every object's scene list in turn,
    then the multi-object scenes.  ``frame_ids[s]`` are scene s's image indices (its pose_data keys), in store order."""

    def __init__(self, rgb, depth, mask, poses, scene_first_frame, scene_object, K=None, scene_names=None, object_ids=None,
                 frame_ids=None, data_types=None):
        first = _host_ints(scene_first_frame, "scene_first_frame")
        sobj = _host_ints(scene_object, "scene_object")
        S = len(sobj)
        if S < 1 or len(first) != S + 1 or first[0] != 0 or any(b <= a for a, b in zip(first, first[1:])):
            raise ValueError("scene_first_frame must be [S + 1] increasing from 0, every scene with >= 1 frame")
        F = first[-1]
        rgb = _args.image(rgb, F, None, None, "rgb")
        h, w = int(rgb.shape[1]), int(rgb.shape[2])
        depth, mask = _args.depth(depth, F, h, w, "depth"), _args.mask(mask, F, h, w, "mask")
        if tuple(poses.shape) != (F, 4, 4):
            raise ValueError("poses must be [%d, 4, 4]" % F)
        O = max(sobj) + 1 if sobj else 0
        if any(o < -1 for o in sobj):
            raise ValueError("scene_object entries must be an object number >= 0 or -1 (multi-object scene)")
        object_scenes = [[s for s in range(S) if sobj[s] == o] for o in range(O)]
        if any(not l for l in object_scenes):
            raise ValueError("objects must be numbered 0 .. O - 1, each with at least one scene")
        self.device = rgb.device
        dev = self.device
        self.rgb, self.mask = rgb, mask
        self.depth = depth if depth.dtype == torch.int16 else depth.view(torch.int16)
        self.poses = torch.as_tensor(poses, dtype=torch.float64).to(dev).reshape(F, 16).contiguous()
        # host copy of the frame translations, float64 [F, 3] (evaluate.choose_pairs)
        self.poses_host = self.poses.view(F, 4, 4).cpu().numpy().copy()     # float64 [F, 4, 4] (evaluate.choose_cross_scene_views)
        self.translations_host = self.poses_host[:, :3, 3].copy()
        Ks, cams = _args.camera_k_rows(K, S)                 # (K | K^-1 per scene: the first 18 floats of a camera row)
        self.K = np.array(Ks, dtype=np.float64)
        self.scene_cams = torch.from_numpy(np.ascontiguousarray(cams, dtype=np.float32)).to(dev)
        i32 = lambda l: torch.tensor(l if l else [0], dtype=torch.int32).to(dev)
        self.scene_first_frame_host, self.scene_object_host = first, sobj
        self.object_scenes_host = object_scenes
        self.multi_scenes_host = [s for s in range(S) if sobj[s] == -1]
        offs = np.cumsum([0] + [len(l) for l in object_scenes]).tolist()
        self._tables = [i32(first), i32(sobj), i32(offs), i32(sum(object_scenes, [])), i32(self.multi_scenes_host)]
        self.num_frames, self.num_scenes, self.num_objects, self.h, self.w = F, S, O, h, w
        self.scene_names = list(scene_names) if scene_names is not None else ["scene_%d" % s for s in range(S)]
        self.object_ids = list(object_ids) if object_ids is not None else ["object_%d" % o for o in range(O)]
        self.frame_ids = ([list(f) for f in frame_ids] if frame_ids is not None
                          else [list(range(first[s + 1] - first[s])) for s in range(S)])
        _lib.require_device(self.rgb, self.depth, self.mask, self.poses, self.scene_cams, *self._tables)
        P = lambda t: t.data_ptr()
        tb = dict(zip(("scene_first_frame", "scene_object", "object_scene_offsets", "object_scenes", "multi_scenes"),
                      [P(x) for x in self._tables]))
        self.desc = _lib.FrameStoreDesc(num_frames=F, num_scenes=S, num_objects=O, num_multi=len(self.multi_scenes_host), h=h,
                                        w=w, rgb=P(self.rgb), depth=P(self.depth), mask=P(self.mask),
                                        scene_cams=P(self.scene_cams), poses=P(self.poses), **tb)
        for t in data_types or ():
            self.check_type(t)

    @classmethod
    def from_tensors(cls, rgb, depth, mask, poses, scene_first_frame, scene_object, K=None, **kw):
        """rgb uint8 [F, H, W, 3], depth 16-bit [F, H, W] millimetres, mask 0/1 [F, H, W], all on the target device; poses
        [F, 4, 4] camera-to-world (host or device); scene_first_frame [S + 1]; scene_object [S] (object number, -1 for a
        multi-object scene); K [3, 3] or [S, 3, 3] on the host (None: the reference's default K).  Keywords: scene_names,
        object_ids, frame_ids, data_types (each checked with ``check_type``)."""
        return cls(rgb, depth, mask, poses, scene_first_frame, scene_object, K, **kw)

    @classmethod
    def from_dataset(cls, dataset, mode="train", device=None, data_types=None):
        """Every frame of ``dataset``'s ``mode`` scenes (a SpartanDataset), read once through its ``get_rgbd_mask_pose``
        (masks as 0/1) and uploaded frame by frame; K per scene from ``get_camera_intrinsics``."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        objects = list(dataset.get_list_of_objects())
        scenes, sobj = [], []
        for o, oid in enumerate(objects):
            for s in dataset.get_scene_list_for_object(oid, mode=mode):
                scenes.append(s)
                sobj.append(o)
        for s in dataset._multi_object_scene_dict[mode]:
            scenes.append(s)
            sobj.append(-1)
        frame_ids = [list(dataset.get_pose_data(s).keys()) for s in scenes]
        first = np.cumsum([0] + [len(f) for f in frame_ids]).tolist()
        F = first[-1]
        rgb = depth = mask = None
        poses = np.zeros((F, 4, 4), np.float64)
        Ks = []
        for si, s in enumerate(scenes):
            cam = dataset.get_camera_intrinsics(s)
            Ks.append(np.asarray(cam.get_camera_matrix() if hasattr(cam, "get_camera_matrix") else cam, np.float64))
            for j, idx in enumerate(frame_ids[si]):
                r, d, m, pose = dataset.get_rgbd_mask_pose(s, idx)
                r, d, m = np.asarray(r), np.asarray(d), np.asarray(m)
                if rgb is None:
                    h, w = int(r.shape[0]), int(r.shape[1])
                    rgb = torch.empty((F, h, w, 3), dtype=torch.uint8, device=dev)
                    depth = torch.empty((F, h, w), dtype=torch.int16, device=dev)
                    mask = torch.empty((F, h, w), dtype=torch.uint8, device=dev)
                f = first[si] + j
                rgb[f].copy_(torch.from_numpy(np.ascontiguousarray(r, dtype=np.uint8)))
                depth[f].copy_(torch.from_numpy(np.ascontiguousarray(d.astype(np.uint16).view(np.int16))))
                mask[f].copy_(torch.from_numpy(np.ascontiguousarray(m != 0, dtype=np.uint8)))
                poses[f] = np.asarray(pose, np.float64)
        if rgb is None:
            raise ValueError("the dataset has no frames in mode %r" % mode)
        return cls(rgb, depth, mask, poses, first, sobj, np.stack(Ks), scene_names=scenes, object_ids=objects,
                   frame_ids=frame_ids, data_types=data_types)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in [self.rgb, self.depth, self.mask, self.poses, self.scene_cams]
                   + self._tables)

    def check_type(self, data_type):
        """ValueError for a data type this store cannot serve, as the reference's loader raises when it is drawn."""
        t = int(data_type)
        if t not in range(5):
            raise ValueError("unknown data type %r" % (data_type,))
        if t == MULTI_OBJECT:
            if not self.multi_scenes_host:
                raise ValueError("There are no multi object scenes in this dataset")
            return
        if self.num_objects == 0:
            raise ValueError("There are no single object scenes in this dataset")
        if t == SINGLE_OBJECT_ACROSS_SCENE:
            for o, l in enumerate(self.object_scenes_host):
                if len(l) < 2:
                    raise ValueError("There is only one scene of object %s, can't sample a different one (%s)"
                                     % (self.object_ids[o], TYPE_NAMES[t]))
        if t in (DIFFERENT_OBJECT, SYNTHETIC_MULTI_OBJECT) and self.num_objects < 2:
            raise ValueError("There is only one object, can't sample a different one (%s)" % TYPE_NAMES[t])

    @property
    def supported_types(self):
        ok = []
        for t in range(5):
            try:
                self.check_type(t)
                ok.append(t)
            except ValueError:
                pass
        return ok


def draw_words(num_attempts):
    return DRAW_HEADER + 2 * int(num_attempts)


def pack_draws(pairs, num_attempts):
    """``pairs``: one dict per pair with any of DRAW_WORDS and ``attempts_a`` / ``attempts_b`` (the image b candidates of
    scene a, and of scene b for SYNTHETIC_MULTI_OBJECT), each the position the reference's draw returned; missing words are 0.
    -> int32 [B, draw_words(num_attempts)], the replay layout of include/dcn_hip.h section 10."""
    A = int(num_attempts)
    out = np.zeros((len(pairs), draw_words(A)), np.int32)
    for p, d in enumerate(pairs):
        unknown = set(d) - set(DRAW_WORDS) - {"attempts_a", "attempts_b"}
        if unknown:
            raise ValueError("unknown draw words %s" % sorted(unknown))
        for k, name in enumerate(DRAW_WORDS):
            out[p, k] = int(d.get(name, 0))
        for base, name in ((DRAW_HEADER, "attempts_a"), (DRAW_HEADER + A, "attempts_b")):
            a = np.asarray(d.get(name, []), np.int64).reshape(-1)
            if a.size > A:
                raise ValueError("%s has %d entries, more than num_attempts = %d" % (name, a.size, A))
            out[p, base:base + a.size] = a
    return out


def select_frames(store, batch_size, data_type, *, generator=None, seeds=None, draws=None, num_attempts=50, threshold=0.2,
                  angle_threshold=20, gather=True):
    """Frames for ``batch_size`` pairs of ``data_type`` (the reference's rules; image b by get_img_idx_with_different_pose
    with ``threshold``, ``angle_threshold`` -- radians, as the reference compares them -- and ``num_attempts``), gathered
    from ``store``.  ``draws``: int [B, draw_words(num_attempts)] positions to replay (pack_draws), otherwise per-pair
    ``seeds`` (drawn with ``generator`` when None).  -> FrameBatch.  Two launches, no host synchronization."""
    store.check_type(data_type)
    n, t, A = int(batch_size), int(data_type), int(num_attempts)
    if n < 1 or A < 1:
        raise ValueError("batch_size and num_attempts must be >= 1")
    dev = store.device
    lib = _lib.get()
    dr = None if draws is None else _args.replay_table(draws, (n, draw_words(A)), "draws", dev)
    sd = None if draws is not None else _args.seeds_for(n, dev, generator, seeds)
    frames = torch.empty((n, SLOTS), dtype=torch.int32, device=dev)
    empty = torch.empty(n, dtype=torch.bool, device=dev)
    scenes = torch.empty((n, 2), dtype=torch.int32, device=dev)
    objects = torch.empty((n, 2), dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.require_device(sd, dr)
    P = _lib.ptr
    desc = ctypes.byref(store.desc)
    rc = lib.dcn_select_frames(n, t, desc, A, float(threshold), float(angle_threshold), P(sd), P(dr), P(frames), P(empty),
                               P(scenes), P(objects), P(status), _lib.stream_ptr())
    _lib.check(rc, "dcn_select_frames")
    rgb = depth = mask = cams = None
    if gather:
        rgb, depth, mask, cams = gather_frames(store, frames, empty, status, 4 if t == SYNTHETIC_MULTI_OBJECT else 2)
    return FrameBatch(t, frames, empty, scenes, objects, status, sd, rgb, depth, mask, cams)


def gather_frames(store, frames, empty, status, k=2, want=("rgb", "depth", "mask", "cams")):
    """One ``dcn_gather_frames`` launch: slots 0 .. k - 1 of ``frames`` (int32 [n, 4] store frame indices on the device) into
    new batch tensors rgb uint8 [k, n, H, W, 3], depth int16 [k, n, H, W], mask uint8 [k, n, H, W] and cams fp32 [k / 2, n, 50]
    (None for what is not in ``want``).  ``empty`` (bool [n] or None): pairs whose depth is zeroed; ``status`` (int32 [1]):
    BAD_INDEX is OR-ed into it for a frame index outside the store.  -> (rgb, depth, mask, cams)."""
    n, H, W, dev = int(frames.shape[0]), store.h, store.w, store.device
    new = lambda name, shape, dtype: torch.empty(shape, dtype=dtype, device=dev) if name in want else None
    rgb = new("rgb", (k, n, H, W, 3), torch.uint8)
    depth = new("depth", (k, n, H, W), torch.int16)
    mask = new("mask", (k, n, H, W), torch.uint8)
    cams = new("cams", (k // 2, n, CAM_FLOATS), torch.float32)
    P = _lib.ptr
    rc = _lib.get().dcn_gather_frames(n, k, ctypes.byref(store.desc), P(frames), P(empty), P(rgb), P(depth), P(mask), P(cams),
                                      P(status), _lib.stream_ptr())
    _lib.check(rc, "dcn_gather_frames")
    return rgb, depth, mask, cams


def data_type_distribution(training_config):
    """(types, probabilities) of training.yaml's ``data_type_probabilities``: the types with p > 0 in the reference's order,
    normalized (set_parameters_from_training_config, dense_correspondence_dataset_masked.py:558-589)."""
    t = training_config.get("training", training_config)
    probs = t["data_type_probabilities"]
    types, ps = [], []
    for i, name in enumerate(TYPE_NAMES):
        p = probs.get(name, 0)
        if p > 0:
            types.append(i)
            ps.append(p)
    if not types:
        raise ValueError("data_type_probabilities gives no data type a probability > 0")
    ps = np.array(ps, dtype=np.float64)
    ps /= np.sum(ps)
    return types, ps


def _build_samples(fb, dt, o, generator):
    if dt == SYNTHETIC_MULTI_OBJECT:
        return build_synthetic_multi_object_samples(
            fb.depth, fb.mask, fb.cams, fb.rgb, num_matching_attempts=o.num_matching_attempts,
            sample_matches_only_off_mask=o.sample_matches_only_off_mask,
            num_masked_non_matches_per_match=o.num_masked_non_matches_per_match,
            num_background_non_matches_per_match=o.num_background_non_matches_per_match,
            use_image_b_mask_inv=o.use_image_b_mask_inv, generator=generator, empty=fb.empty)[0]
    if dt in (SINGLE_OBJECT_WITHIN_SCENE, MULTI_OBJECT):
        return build_within_scene_samples(fb.depth[0], fb.depth[1], fb.mask[0], fb.mask[1], None, None, None, fb.rgb[0],
                                          fb.rgb[1], num_matching_attempts=o.num_matching_attempts,
                                          sample_matches_only_off_mask=o.sample_matches_only_off_mask,
                                          num_masked_non_matches_per_match=o.num_masked_non_matches_per_match,
                                          num_background_non_matches_per_match=o.num_background_non_matches_per_match,
                                          use_image_b_mask_inv=o.use_image_b_mask_inv, domain_randomize=o.domain_randomize,
                                          generator=generator, data_type=dt, cameras=fb.cams[0])
    return build_across_scene_samples(fb.mask[0], fb.mask[1], fb.rgb[0], fb.rgb[1], num_samples=o.cross_scene_num_samples,
                                      domain_randomize=o.domain_randomize, generator=generator, data_type=dt)


def draw_training_batch(store, batch_size, training_config, *, generator=None, host_rng=None, per_pair_types=False,
                        synthetic_multi_object=False):
    """One training batch from the store: the data type drawn on the host (``host_rng``: a numpy RandomState / Generator,
    default ``np.random``) from training.yaml's probabilities -- one type per batch, since the loss composes per call --
    then select_frames and build_within_scene_samples / build_across_scene_samples with options_from_config, all with
    ``generator``.  -> (SampleBatch, data_type, FrameBatch).  No host synchronization (SampleBatch.pair_lists() is the one
    read).

    ``synthetic_multi_object``: False (the default) keeps SYNTHETIC_MULTI_OBJECT out of this function: a probability > 0 for
    it raises NotImplementedError.  True draws it like any other type: select_frames gathers its four frames (a1, a2, b1, b2)
    and samples.build_synthetic_multi_object_samples builds the samples, with ``FrameBatch.empty`` passed on; the
    SampleBatch's inputs are the merged images, its BLIND lists are empty (the reference returns none for this type) and its
    ``aug_params`` is None (the type is not augmented; joined with other types, the joined batch's ``aug_params`` is None too).

    ``per_pair_types=True``: one type per PAIR, as the reference's loader draws one per sample -- ``batch_size`` draws of
    ``host_rng.choice`` in pair order; the pairs of each drawn type go through select_frames and their builder as one group
    and the groups are joined (samples.concat_sample_batches) in ascending type order, so pair i of the batch has type
    ``sorted(types_host)[i]`` (or -1 on the device when it came out empty).  -> (SampleBatch, types_host int array
    [batch_size] in draw order, [FrameBatch per group]) for ``loss_composer.get_loss_mixed(..., sb.device_lists())``; no host
    synchronization."""
    types, ps = data_type_distribution(training_config)
    if SYNTHETIC_MULTI_OBJECT in types and not synthetic_multi_object:
        raise NotImplementedError("draw_training_batch does not build SYNTHETIC_MULTI_OBJECT samples: select its four frames "
                                  "with select_frames and merge them with merge.merge_synthetic_samples, or pass "
                                  "synthetic_multi_object=True")
    for t in types:
        store.check_type(t)
    rng = host_rng if host_rng is not None else np.random
    o = options_from_config(training_config)
    if per_pair_types:
        drawn = np.array([int(types[int(rng.choice(len(types), p=ps))]) for _ in range(int(batch_size))], dtype=np.int64)
        groups, fbs = [], []
        for dt in sorted(set(drawn.tolist())):
            fb = select_frames(store, int(np.sum(drawn == dt)), dt, generator=generator)
            fbs.append(fb)
            groups.append(_build_samples(fb, dt, o, generator))
        return concat_sample_batches(groups), drawn, fbs
    dt = int(types[int(rng.choice(len(types), p=ps))])
    fb = select_frames(store, batch_size, dt, generator=generator)
    return _build_samples(fb, dt, o, generator), dt, fb
