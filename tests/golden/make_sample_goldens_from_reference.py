"""Pins the device sample builder (csrc/sample_kernels.hip, dcn_hip/samples.py): runs the REFERENCE's own
``SpartanDataset.get_within_scene_data`` and ``get_across_scene_data`` (dense_correspondence/dataset/spartan_dataset_masked.py
:577-839, :1056-1141, imported from the reference tree at run time through tests/reference_py3.py, never copied) on small
in-memory frames and stores inputs, every random draw and the 8 lists + type as tests/golden/sample_ref_*.npz.

A ``SpartanDataset`` subclass (the pattern of tests/reference_loop_runner.py) serves the frames; ``debug`` and
``domain_randomize`` are off (background randomization is pinned by the augmentation goldens), flips stay on.  ``torch.rand``
is wrapped to record each call together with its draw site (cand / masked / background / blind / across_a / across_b), and
``random.random`` to record the two flip decisions.

In-memory patches (py2 / torch-0.4 semantics under py3 / torch 2, added to reference_py3.SEMANTIC_PATCHES for this process):
LongTensor ``/ image_width`` is integer division (correspondence_finder.py:325, utils.py:323); an all-zero ``torch.nonzero``
is caught by ``.numel() == 0`` where torch <= 0.3 made ``.dim() == 0`` true (so "no match survives" returns (None, None),
:498-607, as the reference intends); ``diffs_k.view(-1,1)`` ->
``.reshape`` (torch 2 keeps transposed strides); flip_vertical / flip_horizontal read ``images[-1]`` where py2 leaked the list
comprehension's ``image``.

Seeds are the first ones (from 0 up) that take the wanted flips; archives are written with fixed zip timestamps, so running
this again regenerates the files byte for byte.

    python tests/golden/make_sample_goldens_from_reference.py
"""
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import reference_py3 as rp                                                           # noqa: E402
from make_augmentation_goldens_from_reference import first_seed, write_npz          # noqa: E402

PATCHES = {
    "dense_correspondence/correspondence_tools/correspondence_finder.py": [
        (r"randomized_mask_b_indices_flat/image_width", "randomized_mask_b_indices_flat//image_width",
         "torch-0.4 LongTensor '/' is integer division"),
        (r"(\w+_indices)\.dim\(\) == 0", r"\1.numel() == 0",
         "torch <= 0.3: torch.nonzero of an all-zero tensor is a 0-dim empty tensor (torch 2: shape [0, 1])"),
        (r"diffs_0\.view\(-1,1\)", "diffs_0.reshape(-1,1)", "torch 2 keeps transposed strides"),
        (r"diffs_1\.view\(-1,1\)", "diffs_1.reshape(-1,1)", "torch 2 keeps transposed strides"),
    ],
    "modules/dense_correspondence_manipulation/utils/utils.py": [
        (r"flat_pixel_locations/image_width", "flat_pixel_locations//image_width",
         "torch-0.4 LongTensor '/' is integer division"),
    ],
    "dense_correspondence/correspondence_tools/correspondence_augmentation.py": [
        (r"\(image\.height-1\) - v_pixel_positions", "(images[-1].height-1) - v_pixel_positions", "py2 leaks comprehension vars"),
        (r"\(image\.width-1\) - u_pixel_positions", "(images[-1].width-1) - u_pixel_positions", "py2 leaks comprehension vars"),
    ],
}

SITES = ("cand", "masked", "background", "blind", "across_a", "across_b")


def setup():
    for k, v in PATCHES.items():
        rp.SEMANTIC_PATCHES.setdefault(k, []).extend(v)
    rp.install()
    rp.install_third_party_stubs()
    os.environ["DC_SOURCE_DIR"] = rp.REF
    psd = types.ModuleType("pytorch_segmentation_detection")
    psd.__path__ = []
    tr = types.ModuleType("pytorch_segmentation_detection.transforms")
    tr.ComposeJoint = type("ComposeJoint", (object,), {})
    psd.transforms = tr
    sys.modules.update({psd.__name__: psd, tr.__name__: tr})
    sys.path.extend([rp.REF, os.path.join(rp.REF, "modules")])
    import dense_correspondence.dataset.spartan_dataset_masked as sdm
    import dense_correspondence.correspondence_tools.correspondence_finder as cf
    return sdm, cf


def pose(rx, ry, t):
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]).dot(np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def frames(h, w, seed):
    """Two views: smooth depth surfaces in millimetres (with no-return holes), elliptical 0/1 object masks, nearby poses
    (the default K puts the principal point far right of a small image: poses shift the view so that matches land inside)."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)

    def surf():
        d = 900 + 60 * np.sin(xs / (6 + 4 * rng.rand())) + 50 * np.cos(ys / (5 + 3 * rng.rand())) + 20 * rng.rand()
        d[rng.rand(h, w) < 0.05] = 0
        return d.astype(np.uint16)

    def mask(cy, cx):
        return ((((ys - cy * h) / (0.3 * h)) ** 2 + ((xs - cx * w) / (0.3 * w)) ** 2) <= 1.0).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    rgb = np.stack([(7 * x) % 256, (11 * y) % 256, (x + y) % 256], axis=-1).astype(np.uint8)
    return dict(depth_a=surf(), depth_b=surf(), mask_a=mask(0.5, 0.45), mask_b=mask(0.55, 0.5), rgb=rgb,
                pose_a=pose(0.0, 0.0, [0.0, 0.0, 0.0]), pose_b=pose(0.002, -0.003, [0.004, 0.002, 0.001]))


class Recorder(object):
    def __init__(self, cf):
        self.cf, self.site, self.calls, self.flips = cf, [], [], []
        self.saved = {}

    def __enter__(self):
        rec = self
        self.saved["rand"] = torch.rand
        self.saved["random"] = random.random
        orig_rand, orig_random = torch.rand, random.random

        def rand(*a, **k):
            t = orig_rand(*a, **k)
            rec.calls.append((rec.site[0] if rec.site else "?", t.clone().reshape(-1).numpy()))
            return t

        def rnd():
            r = orig_random()
            rec.flips.append(r)
            return r
        torch.rand, random.random = rand, rnd
        n_nonmatch = [0]

        def at(name, site_fn):
            f = getattr(self.cf, name)
            self.saved[name] = f

            def g(*a, **k):
                top = not rec.site
                if top:
                    rec.site.append(site_fn())
                try:
                    return f(*a, **k)
                finally:
                    if top:
                        rec.site.pop()
            setattr(self.cf, name, g)
        at("batch_find_pixel_correspondences", lambda: "cand")

        def nonmatch_site():
            n_nonmatch[0] += 1
            return "masked" if n_nonmatch[0] == 1 else "background"
        at("create_non_correspondences", nonmatch_site)
        n_across = [0]

        def blind_site():
            n_across[0] += 1
            return {0: "blind", 1: "across_a", 2: "across_b"}[n_across[0] if self.across else 0]
        at("random_sample_from_masked_image_torch", blind_site)
        return self

    def __exit__(self, *exc):
        torch.rand, random.random = self.saved.pop("rand"), self.saved.pop("random")
        for k, f in self.saved.items():
            setattr(self.cf, k, f)


def make_dataset(sdm, fr, cfg):
    SD = sdm.SpartanDataset

    class TinyDataset(SD):
        def __init__(self):                    # (no scene files)
            self.debug, self.mode = False, "train"
            self._domain_randomize = False
            self.num_matching_attempts = cfg["A"]
            self.sample_matches_only_off_mask = cfg["only_off_mask"]
            self.num_masked_non_matches_per_match = cfg["k1"]
            self.num_background_non_matches_per_match = cfg["k2"]
            self._use_image_b_mask_inv = cfg["inv"]
            self.cross_scene_num_samples = cfg["n_across"]
            self._rgb_image_to_tensor = lambda img: torch.from_numpy(np.array(img)).permute(2, 0, 1).float().div(255)

        def get_random_image_index(self, scene_name):
            return 0 if scene_name in ("scene", "scene_a") else 1

        def get_img_idx_with_different_pose(self, scene_name, pose, num_attempts=50):
            return 1

        def get_number_of_unique_single_objects(self):
            return 1

        def get_rgbd_mask_pose(self, scene_name, idx):
            s = "ab"[idx]
            return (Image.fromarray(fr["rgb"]), fr["depth_" + s], Image.fromarray(fr["mask_" + s]), fr["pose_" + s])
    return TinyDataset()


def case(sdm, cf, name, h, w, flips, across=False, A=300, only_off_mask=True, k1=3, k2=3, inv=True, n_across=40, edit=None,
         seed=1):
    fr = frames(h, w, seed)
    if edit:
        edit(fr)
    cfg = dict(A=A, only_off_mask=only_off_mask, k1=k1, k2=k2, inv=inv, n_across=n_across)
    ds = make_dataset(sdm, fr, cfg)

    def flips_of(s):
        random.seed(s)
        return (random.random() >= 0.5, random.random() >= 0.5)
    s = first_seed(lambda s: flips_of(s) == tuple(flips))
    random.seed(s)
    torch.manual_seed(s)
    rec = Recorder(cf)
    rec.across = across
    with rec:
        if across:
            out = ds.get_across_scene_data("scene_a", "scene_b", {"type": sdm.SpartanDatasetDataType.SINGLE_OBJECT_ACROSS_SCENE})
        else:
            out = ds.get_within_scene_data("scene", {"type": sdm.SpartanDatasetDataType.SINGLE_OBJECT_WITHIN_SCENE})
    keys = ("matches_a", "matches_b", "masked_a", "masked_b", "background_a", "background_b", "blind_a", "blind_b")
    rec_out = dict(across=np.array(across), type=np.array(int(out[0])), seed=np.array(s), h=np.array(h), w=np.array(w),
                   A=np.array(A), only_off_mask=np.array(only_off_mask), k1=np.array(k1), k2=np.array(k2), inv=np.array(inv),
                   n_across=np.array(n_across), flips=np.array([r >= 0.5 for r in rec.flips], dtype=bool),
                   pose_a=fr["pose_a"], pose_b=fr["pose_b"], depth_a=fr["depth_a"], depth_b=fr["depth_b"],
                   mask_a=fr["mask_a"], mask_b=fr["mask_b"])
    for k, t in zip(keys, out[3:11]):
        rec_out[k] = t.reshape(-1).long().numpy()
    for site in SITES:
        got = [v for s2, v in rec.calls if s2 == site]
        if site == "cand" and len(got) == 2:
            # batch_find_pixel_correspondences draws pytorch_rand_select_pixel's torch.rand(2, A) first (correspondence_finder
            # .py:459) and, with a mask, replaces those pixels by mask samples (:470): the second draw is the one used
            got = got[1:]
        if site in ("masked", "background"):
            # the second torch.rand of create_non_correspondences feeds its inert perturbation (:361, multiplied by zeros)
            got = got[:1]
        assert len(got) <= 1, (name, site, len(got))
        rec_out["rand_" + site] = got[0].astype(np.float32) if got else np.zeros(0, np.float32)
    assert not [s2 for s2, _ in rec.calls if s2 not in SITES]
    write_npz(os.path.join(HERE, "sample_ref_%s.npz" % name), rec_out)
    print(name, "type", int(out[0]), "flips", rec_out["flips"].tolist(), "lists",
          [len(rec_out[k]) for k in keys], "draws", {k: len(rec_out["rand_" + k]) for k in SITES})


def main():
    sdm, cf = setup()

    def zero(key):
        def f(fr):
            fr[key] = np.zeros_like(fr[key])
        return f
    case(sdm, cf, "normal_48x64", 48, 64, (False, False))
    case(sdm, cf, "flip_a_48x64", 48, 64, (True, False))
    case(sdm, cf, "flip_b_48x64", 48, 64, (False, True))
    case(sdm, cf, "flip_ab_37x53", 37, 53, (True, True), seed=2)
    case(sdm, cf, "off_mask_matches_37x53", 37, 53, (True, False), only_off_mask=False, seed=3)
    case(sdm, cf, "empty_mask_a_37x53", 37, 53, (False, False), edit=zero("mask_a"))
    case(sdm, cf, "no_match_37x53", 37, 53, (False, False), edit=zero("depth_b"))
    case(sdm, cf, "empty_mask_b_48x64", 48, 64, (False, True), edit=zero("mask_b"), seed=4)
    case(sdm, cf, "no_mask_inv_48x64", 48, 64, (True, True), inv=False, seed=5)
    case(sdm, cf, "across_48x64", 48, 64, (True, False), across=True)
    case(sdm, cf, "across_empty_b_37x53", 37, 53, (False, False), across=True, edit=zero("mask_b"))


if __name__ == "__main__":
    main()
