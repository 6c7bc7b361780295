"""Pins the device builder of SYNTHETIC_MULTI_OBJECT samples (csrc/synthetic_kernels.hip,
dcn_hip/samples.py build_synthetic_multi_object_samples): runs the REFERENCE's own
``SpartanDataset.get_synthetic_multi_object_within_scene_data`` (dense_correspondence/dataset/spartan_dataset_masked.py
:890-1053, imported from the reference tree at run time through tests/reference_py3.py, never copied) on a ``SpartanDataset``
subclass that serves four small in-memory frames (object a's a1, a2 and object b's b1, b2), and stores the inputs, every
``torch.rand`` call with its site (cand_a / cand_b / masked / background), the ``random.random()`` foreground decisions, the
merged masks that ``merge_images_with_occlusions`` returned, the 8 lists, the type and the two image tensors as
tests/golden/synthetic_ref_*.npz.

The semantic patches, the frames and the pose helper are those of make_sample_goldens_from_reference.py; ``first_seed`` and
``write_npz`` those of make_augmentation_goldens_from_reference.py.  Seeds are the first ones (from 0 up) that take the wanted
foreground decisions; archives are written with fixed zip timestamps, so running this again regenerates the files byte for
byte.

The reference cannot reach "no image b with a different enough pose": its wrapper fails to unpack the empty sample there
(make_frame_goldens_from_reference.py).  The device rule for it, an empty sample, is tested directly.

    python tests/golden/make_synthetic_goldens_from_reference.py
"""
import os
import random
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_sample_goldens_from_reference as ms                                      # noqa: E402
from make_augmentation_goldens_from_reference import first_seed, write_npz          # noqa: E402

SITES = ("cand_a", "cand_b", "masked", "background")
KEYS = ("matches_a", "matches_b", "masked_a", "masked_b", "background_a", "background_b", "blind_a", "blind_b")
FRAMES = ("a1", "a2", "b1", "b2")


def four_frames(h, w, seed, small_shift):
    """Object a's two views are make_sample_goldens' frames; object b's are the same recipe with another seed, masks moved
    to the right and another image.  ``small_shift``: second poses a fifth of a millimetre away, so that the projections of a
    one-row / one-column image stay inside it."""
    fa, fb = ms.frames(h, w, seed), ms.frames(h, w, seed + 10)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    ell = lambda cy, cx: ((((ys - cy * h) / (0.3 * h + 0.5)) ** 2 + ((xs - cx * w) / (0.3 * w + 0.5)) ** 2) <= 1.0).astype(np.uint8)
    fr = {}
    for o, f, (c1, c2) in (("a", fa, ((0.5, 0.4), (0.55, 0.45))), ("b", fb, ((0.45, 0.6), (0.5, 0.65)))):
        fr["depth_%s1" % o], fr["depth_%s2" % o] = f["depth_a"], f["depth_b"]
        fr["mask_%s1" % o], fr["mask_%s2" % o] = ell(*c1), ell(*c2)
        fr["pose_%s1" % o] = f["pose_a"]
        fr["pose_%s2" % o] = ms.pose(0.0, 0.0, [-0.0002, -0.0002, 0.0]) if small_shift else f["pose_b"]
        for k in (1, 2):                       # images of 8 x 8 blocks (they compress), another phase per frame
            bx, by = xs.astype(np.int64) // 8 + 2 * k + (5 if o == "b" else 0), ys.astype(np.int64) // 8
            fr["rgb_%s%d" % (o, k)] = np.stack([(17 * bx + 29 * by) % 256, (37 * bx + 39 * by + 11) % 256,
                                                (57 * bx + 49 * by + 101) % 256], axis=-1).astype(np.uint8)
    return fr


class Recorder(object):
    """torch.rand calls with their site, random.random() calls, and merge_images_with_occlusions' merged masks"""

    def __init__(self, cf, ca):
        self.cf, self.ca, self.site, self.calls, self.decisions, self.masks, self.saved = cf, ca, [], [], [], [], {}

    def __enter__(self):
        rec = self
        orig_rand, orig_random = torch.rand, random.random
        self.saved_globals = (orig_rand, orig_random)

        def rand(*a, **k):
            t = orig_rand(*a, **k)
            rec.calls.append((rec.site[0] if rec.site else "?", t.clone().reshape(-1).numpy()))
            return t

        def rnd():
            r = orig_random()
            rec.decisions.append(r)
            return r
        torch.rand, random.random = rand, rnd

        def at(mod, name, sites):
            f = getattr(mod, name)
            self.saved[(mod, name)] = f
            n = [0]

            def g(*a, **k):
                top = not rec.site
                if top:
                    rec.site.append(sites[n[0]])
                    n[0] += 1
                try:
                    return f(*a, **k)
                finally:
                    if top:
                        rec.site.pop()
            setattr(mod, name, g)
        at(self.cf, "batch_find_pixel_correspondences", ("cand_a", "cand_b"))
        at(self.cf, "create_non_correspondences", ("masked", "background"))
        merge = self.ca.merge_images_with_occlusions
        self.saved[(self.ca, "merge_images_with_occlusions")] = merge

        def merge_and_keep(*a, **k):
            out = merge(*a, **k)
            rec.masks.append(np.asarray(out[1]).copy())
            return out
        self.ca.merge_images_with_occlusions = merge_and_keep
        return self

    def __exit__(self, *exc):
        torch.rand, random.random = self.saved_globals
        for (mod, name), f in self.saved.items():
            setattr(mod, name, f)


def make_dataset(sdm, fr, cfg):
    class FourFrames(sdm.SpartanDataset):
        def __init__(self):                    # (no scene files)
            self.debug, self.mode = False, "train"
            self._domain_randomize = False
            self.num_matching_attempts = cfg["A"]
            self.sample_matches_only_off_mask = cfg["only_off_mask"]
            self.num_masked_non_matches_per_match = cfg["k1"]
            self.num_background_non_matches_per_match = cfg["k2"]
            self._use_image_b_mask_inv = cfg["inv"]
            self._initialize_rgb_image_to_tensor()

        def get_two_different_object_ids(self):
            return "a", "b"

        def get_random_single_object_scene_name(self, object_id):
            return object_id

        def get_random_image_index(self, scene_name):
            return 1

        def get_img_idx_with_different_pose(self, scene_name, pose, num_attempts=50):
            return 2

        def get_rgbd_mask_pose(self, scene_name, idx):
            s = "%s%d" % (scene_name, idx)
            return (Image.fromarray(fr["rgb_" + s]), fr["depth_" + s], Image.fromarray(fr["mask_" + s]), fr["pose_" + s])
    return FourFrames()


def case(sdm, cf, ca, name, h, w, fg, A=150, only_off_mask=True, k1=2, k2=2, inv=True, edit=None, seed=1, small_shift=False):
    """fg: the wanted foreground records (1 = object b in front) of frame 1 and frame 2"""
    fr = four_frames(h, w, seed, small_shift)
    if edit:
        edit(fr)
    cfg = dict(A=A, only_off_mask=only_off_mask, k1=k1, k2=k2, inv=inv)
    ds = make_dataset(sdm, fr, cfg)

    def decisions(s):
        random.seed(s)
        return (int(random.random() < 0.5), int(random.random() < 0.5))
    s = first_seed(lambda s: decisions(s) == tuple(fg))
    random.seed(s)
    torch.manual_seed(s)
    rec = Recorder(cf, ca)
    with rec:
        out = ds.get_synthetic_multi_object_within_scene_data()
    typ = int(out[0])
    drawn = [int(r < 0.5) for r in rec.decisions]
    assert drawn == list(fg)[:len(drawn)] and len(drawn) == len(rec.masks), (name, drawn)
    from dense_correspondence_manipulation.utils import constants
    o = dict(type=np.array(typ), seed=np.array(s), h=np.array(h), w=np.array(w), A=np.array(A),
             only_off_mask=np.array(only_off_mask), k1=np.array(k1), k2=np.array(k2), inv=np.array(inv),
             foreground=np.array((drawn + [0, 0])[:2], np.int32), n_decisions=np.array(len(drawn)),
             K=np.asarray(cf.get_default_K_matrix(), np.float64), mean=np.array(constants.DEFAULT_IMAGE_MEAN, np.float64),
             std=np.array(constants.DEFAULT_IMAGE_STD_DEV, np.float64))
    for k in FRAMES:
        for what in ("depth_", "mask_", "rgb_", "pose_"):
            o[what + k] = fr[what + k]
    for k, t in zip(KEYS, out[3:11]):
        o[k] = t.reshape(-1).long().numpy()
    full = typ != -1
    o["out_image_a"] = out[1].numpy() if full else np.zeros(0, np.float32)
    o["out_image_b"] = out[2].numpy() if full else np.zeros(0, np.float32)
    o["out_mask_a"] = rec.masks[0].astype(np.uint8) if full else np.zeros(0, np.uint8)
    o["out_mask_b"] = rec.masks[1].astype(np.uint8) if full else np.zeros(0, np.uint8)
    for site in SITES:
        got = [v for s2, v in rec.calls if s2 == site]
        if site.startswith("cand") and len(got) == 2:
            # batch_find_pixel_correspondences draws pytorch_rand_select_pixel's torch.rand(2, A) first (correspondence_finder
            # .py:459) and, with a mask, replaces those pixels by mask samples (:470): the second draw is the one used
            got = got[1:]
        if site in ("masked", "background"):
            # the second torch.rand of create_non_correspondences feeds its inert perturbation (:361, multiplied by zeros)
            got = got[:1]
        assert len(got) <= 1, (name, site, len(got))
        o["rand_" + site] = got[0].astype(np.float32) if got else np.zeros(0, np.float32)
    assert not [s2 for s2, _ in rec.calls if s2 not in SITES]
    path = os.path.join(HERE, "synthetic_ref_%s.npz" % name)
    write_npz(path, o)
    print(name, "type", typ, "foreground", drawn, "lists", [len(o[k]) for k in KEYS], "draws",
          {k: len(o["rand_" + k]) for k in SITES}, os.path.getsize(path), "bytes")
    return o


def main():
    sdm, cf = ms.setup()
    import dense_correspondence.correspondence_tools.correspondence_augmentation as ca

    def fill(key, value):
        def f(fr):
            fr[key] = np.full_like(fr[key], value)
        return f
    c = lambda *a, **k: case(sdm, cf, ca, *a, **k)
    kept = lambda o: int(o["type"]) == 4
    assert kept(c("fg_aa_48x64", 48, 64, (0, 0)))
    assert kept(c("fg_ab_48x64", 48, 64, (0, 1)))
    assert kept(c("fg_ba_37x53", 37, 53, (1, 0), seed=2))
    assert kept(c("fg_bb_37x53", 37, 53, (1, 1), seed=2))
    assert kept(c("row_1x64", 1, 64, (0, 1), seed=3, small_shift=True))

    def halves(fr):                            # one column: object a in the lower rows, object b in the upper ones
        for k in "12":
            fr["mask_a" + k][:] = 0
            fr["mask_a" + k][28:] = 1
            fr["mask_b" + k][:] = 0
            fr["mask_b" + k][:30] = 1
    assert kept(c("column_48x1", 48, 1, (1, 0), seed=3, small_shift=True, edit=halves))
    assert kept(c("uniform_candidates_37x53", 37, 53, (1, 0), only_off_mask=False, seed=2))
    assert kept(c("no_mask_inv_48x64", 48, 64, (0, 1), inv=False, seed=5))
    o = c("a_finds_nothing_37x53", 37, 53, (0, 0), edit=fill("depth_a2", 0))
    assert not kept(o) and o["rand_cand_b"].size == 0 and int(o["n_decisions"]) == 0     # b's scene is never searched
    o = c("b_finds_nothing_37x53", 37, 53, (0, 0), edit=fill("depth_b2", 0))
    assert not kept(o) and o["rand_cand_b"].size > 0 and int(o["n_decisions"]) == 0
    o = c("occluded_frame_1_48x64", 48, 64, (1, 0), edit=fill("mask_b1", 1))             # b in front of all of a in frame 1
    assert not kept(o) and int(o["n_decisions"]) == 1
    o = c("occluded_frame_2_only_37x53", 37, 53, (1, 0), edit=fill("mask_a2", 1), seed=2)  # a in front of all of b in frame 2
    assert not kept(o) and int(o["n_decisions"]) == 2


if __name__ == "__main__":
    main()
