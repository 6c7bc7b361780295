"""Pins the device frame choice (csrc/frame_kernels.hip, dcn_hip/frames.py): runs the REFERENCE's own selection code --
``get_random_image_index``, ``get_img_idx_with_different_pose``, ``get_different_scene_for_object``,
``get_two_different_object_ids`` and the five type wrappers (dense_correspondence/dataset/spartan_dataset_masked.py, imported
from the reference tree at run time through tests/reference_py3.py, never copied) -- on a ``SpartanDataset`` subclass with
in-memory pose tables, and stores the tables, every draw and the chosen frames as tests/golden/frame_ref_<type>.npz.

The subclass serves poses from memory (``get_pose_from_scene_name_and_idx``) and frames as placeholders; the wrappers run up to
the point where the frames are loaded: the last ``get_rgbd_mask_pose`` of a pair (2, or 4 for SYNTHETIC_MULTI_OBJECT) ends the
call, and the correspondence search in between (SYNTHETIC_MULTI_OBJECT's first scene) returns a placeholder.  ``random.choice``
is wrapped to record the POSITION it chose (it calls the original on ``range(len(seq))``: the same ``_randbelow`` draw) and
``np.random.choice`` to record its result; each record is labelled by the helper it came from.

Scenes (object 0: ``thresh``, ``rot``; object 1: ``same``, ``single``; object 2: ``mixed``, ``single2``; multi-object:
``multi``, ``multi_same``): translations 0.2 m -/+ 1e-6 apart (``thresh``), a pure 90-degree rotation with zero translation
next to a 0.5 m translation (``rot``; the rotation must be REJECTED -- the reference's angle is in radians, compared against
20), scenes where every pose is the same (no image b: an empty pair) and single-frame scenes.  Positions in the scene
lists are frame offsets (the pose tables' keys are 0 .. n-1 in order).  Chosen frames: -1 for None, -2 where the reference
stopped before choosing.  The reference's SYNTHETIC_MULTI_OBJECT wrapper fails to unpack the 12-tuple of
``return_empty_data`` when its first scene has no image b (spartan_dataset_masked.py:907-910): recorded as an empty pair.
Archives are written with fixed zip timestamps, so running this again regenerates the files byte for byte.

    python tests/golden/make_frame_goldens_from_reference.py
"""
import collections
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_augmentation_goldens_from_reference import write_npz        # noqa: E402
from make_sample_goldens_from_reference import setup                    # noqa: E402

A = 50                                    # get_within_scene_data's num_attempts
HEADER = 8
WORD = dict(object_a=0, object_b=1, scene_a=2, scene_b=3, scene_b2=4, frame_a=5, frame_b=6)
TYPES = ("SINGLE_OBJECT_WITHIN_SCENE", "SINGLE_OBJECT_ACROSS_SCENE", "DIFFERENT_OBJECT", "MULTI_OBJECT",
         "SYNTHETIC_MULTI_OBJECT")
PAIRS = 24


def pose(rz=0.0, t=(0.0, 0.0, 0.0), rx=0.0):
    cz, sz, cx, sx = np.cos(rz), np.sin(rz), np.cos(rx), np.sin(rx)
    T = np.eye(4)
    T[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]).dot(np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    T[:3, 3] = t
    return T


def scenes():
    rng = np.random.RandomState(7)
    base = pose(0.3, (0.1, -0.2, 0.4), 0.2)
    thresh = []
    for x in (0.0, 0.2 - 1e-6, 0.2 + 1e-6):            # pairwise 0.199999 (below), 0.200001 (above), 2e-6 (below)
        T = base.copy()
        T[0, 3] += x
        thresh.append(T)
    rot = [pose(0.0, (0.3, 0.1, 0.0)), pose(np.pi / 2, (0.3, 0.1, 0.0)), pose(0.0, (0.8, 0.1, 0.0))]
    same = [pose(0.1, (0.2, 0.2, 0.2))] * 4
    mixed = [pose(rng.uniform(-1, 1), rng.normal(0, 0.12, 3), rng.uniform(-1, 1)) for _ in range(6)]
    multi = [pose(rng.uniform(-1, 1), rng.normal(0, 0.15, 3)) for _ in range(5)]
    multi_same = [pose(0.4, (0.0, 0.1, 0.0))] * 3
    objects = collections.OrderedDict([("obj_a", ["thresh", "rot"]), ("obj_b", ["same", "single"]),
                                       ("obj_c", ["mixed", "single2"])])
    poses = dict(thresh=thresh, rot=rot, same=same, single=[pose(0.2, (0.5, 0.0, 0.0))], mixed=mixed,
                 single2=[pose(-0.3, (0.0, 0.5, 0.0))], multi=multi, multi_same=multi_same)
    return objects, ["multi", "multi_same"], poses


class Stop(Exception):
    pass


def make_dataset(sdm):
    SD = sdm.SpartanDataset
    objects, multi, poses = scenes()

    class PoseDataset(SD):
        def __init__(self):                    # (no scene files: pose tables in memory)
            self.debug, self.mode = False, "train"
            self._single_object_scene_dict = collections.OrderedDict((o, {"train": list(s), "test": []})
                                                                     for o, s in objects.items())
            self._multi_object_scene_dict = {"train": list(multi), "test": [], "evaluation_labeled_data_path": []}
            self._pose_data = {s: collections.OrderedDict((i, None) for i in range(len(p))) for s, p in poses.items()}
            self.sample_matches_only_off_mask = True
            self.num_matching_attempts = 10
            self.loads, self.stop_after, self.log = [], 2, []

        def get_pose_from_scene_name_and_idx(self, scene_name, idx):
            return poses[scene_name][int(idx)]

        def get_rgbd_mask_pose(self, scene_name, idx):
            self.loads.append((scene_name, int(idx)))
            if len(self.loads) == self.stop_after:
                raise Stop()
            return None, None, None, self.get_pose_from_scene_name_and_idx(scene_name, idx)

        def rgb_image_to_tensor(self, img):
            return img

        def return_empty_data(self, image_a_rgb, image_b_rgb, metadata=None):
            return ("EMPTY",) * 12

    return PoseDataset(), objects, multi, poses


class Recorder(object):
    """Labels every random.choice / np.random.choice with the innermost selection helper that made it; the image b search
    (get_img_idx_with_different_pose) is bracketed by ("enter", -1) / ("exit", -1) records."""

    def __init__(self, ds, sdm):
        self.ds, self.sdm, self.stack, self.events = ds, sdm, [], []

    def __enter__(self):
        rec = self
        self.orig_choice, self.orig_np_choice = random.choice, np.random.choice
        oc, onc = self.orig_choice, self.orig_np_choice

        def choice(seq):
            i = oc(range(len(seq)))
            rec.events.append((rec.stack[-1] if rec.stack else "?", int(i)))
            return seq[i]

        def np_choice(a, *args, **kw):
            r = onc(a, *args, **kw)
            for v in np.asarray(r).reshape(-1):
                rec.events.append((rec.stack[-1] if rec.stack else "?", int(v)))
            return r
        random.choice, np.random.choice = choice, np_choice
        self.saved = []
        for name in ("get_random_object_id", "get_random_single_object_scene_name", "get_random_multi_object_scene_name",
                     "get_different_scene_for_object", "get_two_different_object_ids", "get_random_image_index",
                     "get_img_idx_with_different_pose"):
            f = getattr(self.ds, name)

            def g(*a, _f=f, _name=name, **k):
                rec.stack.append(_name)
                bracket = _name == "get_img_idx_with_different_pose"
                if bracket:
                    rec.events.append(("enter", -1))
                try:
                    return _f(*a, **k)
                finally:
                    rec.stack.pop()
                    if bracket:
                        rec.events.append(("exit", -1))
            setattr(self.ds, name, g)
            self.saved.append(name)
        cf = self.sdm.correspondence_finder
        self.saved_find = cf.batch_find_pixel_correspondences
        cf.batch_find_pixel_correspondences = lambda *a, **k: ("uv", "uv")
        return self

    def __exit__(self, *exc):
        random.choice, np.random.choice = self.orig_choice, self.orig_np_choice
        for name in self.saved:
            delattr(self.ds, name)
        self.sdm.correspondence_finder.batch_find_pixel_correspondences = self.saved_find


def pack(type_name, ev):
    """The recorded draws of one pair -> the replay words of include/dcn_hip.h section 10 (words never drawn stay 0)."""
    words = np.zeros(HEADER + 2 * A, np.int32)
    pos = [0]

    def more():
        return pos[0] < len(ev)

    def take(label):
        assert ev[pos[0]][0] == label, (type_name, pos[0], ev[pos[0]], label, ev)
        pos[0] += 1
        return ev[pos[0] - 1][1]

    def image_index():
        take("get_random_image_index")
        return take("get_random_image_index")      # the second random.choice is the one kept

    def attempts(base):
        take("enter")
        k = 0
        while ev[pos[0]][0] != "exit":
            words[base + k] = image_index()
            k += 1
        take("exit")

    if type_name in ("SINGLE_OBJECT_WITHIN_SCENE", "MULTI_OBJECT"):
        if type_name == "SINGLE_OBJECT_WITHIN_SCENE":
            words[WORD["object_a"]] = take("get_random_object_id")
            words[WORD["scene_a"]] = take("get_random_single_object_scene_name")
        else:
            words[WORD["scene_a"]] = take("get_random_multi_object_scene_name")
        words[WORD["frame_a"]] = image_index()
        attempts(HEADER)
    elif type_name == "SINGLE_OBJECT_ACROSS_SCENE":
        words[WORD["object_a"]] = take("get_random_object_id")
        words[WORD["scene_a"]] = take("get_random_single_object_scene_name")
        words[WORD["scene_b"]] = take("get_different_scene_for_object")
        words[WORD["scene_b2"]] = take("get_different_scene_for_object")
        words[WORD["frame_a"]] = image_index()
        words[WORD["frame_b"]] = image_index()
    else:
        words[WORD["object_a"]] = take("get_two_different_object_ids")
        words[WORD["object_b"]] = take("get_two_different_object_ids")
        words[WORD["scene_a"]] = take("get_random_single_object_scene_name")
        words[WORD["scene_b"]] = take("get_random_single_object_scene_name")
        words[WORD["frame_a"]] = image_index()
        if type_name == "SYNTHETIC_MULTI_OBJECT":
            attempts(HEADER)
            if more():
                words[WORD["frame_b"]] = image_index()
                attempts(HEADER + A)
        else:
            words[WORD["frame_b"]] = image_index()
    assert not more(), (type_name, pos[0], ev)
    return words


def run_pair(ds, sdm, type_name):
    """-> ("frames" | "empty", the (scene, index) loads in order, the draw records)"""
    DT = sdm.SpartanDatasetDataType
    wrapper = {"SINGLE_OBJECT_WITHIN_SCENE": "get_single_object_within_scene_data",
               "SINGLE_OBJECT_ACROSS_SCENE": "get_single_object_across_scene_data",
               "DIFFERENT_OBJECT": "get_different_object_data", "MULTI_OBJECT": "get_multi_object_within_scene_data",
               "SYNTHETIC_MULTI_OBJECT": "get_synthetic_multi_object_within_scene_data"}
    assert int(getattr(DT, type_name)) == TYPES.index(type_name)
    ds.loads = []
    ds.stop_after = 4 if type_name == "SYNTHETIC_MULTI_OBJECT" else 2
    result = "frames"
    with Recorder(ds, sdm) as rec:
        try:
            out = getattr(ds, wrapper[type_name])()
            assert out[0] == "EMPTY", out
            result = "empty"
        except Stop:
            pass
        except ValueError as e:                       # (SYNTHETIC: return_empty_data's 12-tuple into 8 names)
            assert type_name == "SYNTHETIC_MULTI_OBJECT" and "unpack" in str(e), e
            result = "empty"
    return result, list(ds.loads), rec.events


def main():
    sdm, _cf = setup()
    ds, objects, multi, poses = make_dataset(sdm)
    order = [s for o in objects for s in objects[o]] + list(multi)
    first = np.cumsum([0] + [len(poses[s]) for s in order])
    sobj = [i for i, o in enumerate(objects) for _ in objects[o]] + [-1] * len(multi)
    P = np.concatenate([np.stack(poses[s]) for s in order])
    for ti, type_name in enumerate(TYPES):
        random.seed(100 + ti)
        np.random.seed(100 + ti)
        rows = collections.defaultdict(list)
        for p in range(PAIRS):
            result, loads, events = run_pair(ds, sdm, type_name)
            frame = lambda k: int(first[order.index(loads[k][0])] + loads[k][1]) if k < len(loads) else -2
            f = [frame(k) for k in range(4 if type_name == "SYNTHETIC_MULTI_OBJECT" else 2)] + \
                ([] if type_name == "SYNTHETIC_MULTI_OBJECT" else [-2, -2])
            empty = result == "empty"
            if empty:                                 # the image b that was searched for and not found
                k = 1 if len(loads) == 1 else 3
                f[k] = -1
            sa = order.index(loads[0][0])
            if type_name in ("SINGLE_OBJECT_WITHIN_SCENE", "MULTI_OBJECT"):
                sc = [sa, sa]
            elif type_name == "SYNTHETIC_MULTI_OBJECT":
                sc = [sa, order.index(loads[2][0]) if len(loads) > 2 else -2]
            else:
                sc = [sa, order.index(loads[1][0])]
            rows["draws"].append(pack(type_name, events))
            rows["ref_frames"].append(f)
            rows["ref_empty"].append(empty)
            rows["ref_scenes"].append(sc)
            rows["ref_objects"].append([sobj[s] if s >= 0 else -2 for s in sc])
        out = dict(type=np.array(ti), num_attempts=np.array(A), scene_first_frame=first.astype(np.int32),
                   scene_object=np.array(sobj, np.int32), poses=P, draws=np.stack(rows["draws"]).astype(np.int32),
                   ref_frames=np.array(rows["ref_frames"], np.int32), ref_empty=np.array(rows["ref_empty"], bool),
                   ref_scenes=np.array(rows["ref_scenes"], np.int32), ref_objects=np.array(rows["ref_objects"], np.int32))
        write_npz(os.path.join(HERE, "frame_ref_%s.npz" % type_name.lower()), out)
        print(type_name, "empty", int(np.sum(rows["ref_empty"])), "of", PAIRS, "scenes a",
              sorted(set(order[s[0]] for s in rows["ref_scenes"])))


if __name__ == "__main__":
    main()
