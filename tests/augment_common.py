"""Shared by tests/test_emu_augment.py and tests/test_gpu_augment.py (not a test module): a numpy restatement of the augmentation
rules (include/dcn_hip.h section 7, after dense_correspondence/correspondence_tools/correspondence_augmentation.py) and the
golden-fixture replay through the mirror module."""
import glob
import os
import random

import numpy as np
import torch

GOLDENS = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("augment_ref_"):-4] for p in GOLDENS]

FLIP_V, FLIP_H, RANDOMIZE, GRADIENT, VERTICAL, NOISE = 1, 2, 4, 8, 16, 32
M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def noise_plane(seed_lo, seed_hi, image, h, w):
    """(n1 - n2) mod 256, uint8 [h, w, 3], of the counter-based generator for one image record."""
    img = (np.uint64(image) * np.uint64(0x9E3779B9) + np.uint64(0x7F4A7C15)) & M32
    k0 = mix32(np.uint64(seed_lo & 0xFFFFFFFF) ^ mix32(img))
    k1 = mix32(np.uint64(seed_hi & 0xFFFFFFFF) ^ k0)
    e = np.arange(h * w * 3, dtype=np.uint64)
    r = mix32(mix32(e ^ k0) ^ k1)
    n1 = ((r >> np.uint64(16)) * np.uint64(50)) >> np.uint64(16)
    n2 = ((r & np.uint64(0xFFFF)) * np.uint64(50)) >> np.uint64(16)
    return ((n1 - n2) & np.uint64(0xFF)).astype(np.uint8).reshape(h, w, 3)


def restated_augment(rgb, mask, rec, image):
    """One image: uint8 [h, w, 3], 0/1 uint8 [h, w], int32 record, its index in the launch -> (rgb, mask) uint8."""
    h, w = mask.shape
    f = int(rec[0])
    out = rgb.copy()
    if f & RANDOMIZE:
        c1 = rec[1:4].astype(np.float64)
        c2 = rec[4:7].astype(np.float64)
        if f & GRADIENT:
            vertical = bool(f & VERTICAL)
            p = np.linspace(0, 1, h if vertical else w)
            p = np.tile(p[:, None], (1, w)) if vertical else np.tile(p, (h, 1))
            bg = np.stack([(c2[c] * p + c1[c] * (1.0 - p)) for c in range(3)], axis=-1).astype(np.uint8)
        else:
            bg = np.broadcast_to(rec[1:4].astype(np.uint8), (h, w, 3)).copy()
        if f & NOISE:
            bg = bg + noise_plane(int(rec[8]), int(rec[9]), image, h, w)        # uint8: wraps
        m = mask[:, :, None]
        out = (rgb * m + (1 - m) * bg).astype(np.uint8)
    mask = mask.copy()
    if f & FLIP_V:
        out, mask = out[::-1], mask[::-1]
    if f & FLIP_H:
        out, mask = out[:, ::-1], mask[:, ::-1]
    return np.ascontiguousarray(out), np.ascontiguousarray(mask)


def restated_uv(u, v, rec, h, w):
    f = int(rec[0])
    u2 = ((w - 1) - u) if f & FLIP_H else u.copy()
    v2 = ((h - 1) - v) if f & FLIP_V else v.copy()
    return u2, v2


def example_params(n_images, seed=0):
    """Explicit records that cover every branch: image i takes flag pattern i % 10 (plus flips from the rng)."""
    rng = np.random.RandomState(seed)
    patterns = [0, RANDOMIZE, RANDOMIZE | NOISE, RANDOMIZE | GRADIENT, RANDOMIZE | GRADIENT | VERTICAL,
                RANDOMIZE | GRADIENT | NOISE, RANDOMIZE | GRADIENT | VERTICAL | NOISE, FLIP_V | FLIP_H,
                FLIP_V | FLIP_H | RANDOMIZE | GRADIENT | VERTICAL | NOISE, FLIP_V | FLIP_H | RANDOMIZE | NOISE]
    rec = np.zeros((n_images, 16), dtype=np.int32)
    for i in range(n_images):
        rec[i, 0] = patterns[i % len(patterns)] | (int(rng.randint(0, 2)) * (FLIP_V | FLIP_H))
        rec[i, 1:7] = rng.randint(0, 255, size=6)
        rec[i, 8:10] = rng.randint(-2 ** 31, 2 ** 31 - 1, size=2, dtype=np.int64)
    return rec


def scene(n, h, w, seed=0):
    """n uint8 images with every value present and 0/1 masks with a blob each."""
    rng = np.random.RandomState(seed)
    rgb = rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    mask = np.stack([(((y - rng.rand() * h) / (0.4 * h + 1)) ** 2 + ((x - rng.rand() * w) / (0.4 * w + 1)) ** 2 <= 1.0)
                     for _ in range(n)]).astype(np.uint8)
    return rgb, mask


def normalize_torch(rgb_nhwc, mean, std):
    """torchvision ToTensor + Normalize (spartan_dataset_masked.py:297-304) on the host: float(x) / 255, - mean, / std."""
    t = torch.from_numpy(np.ascontiguousarray(rgb_nhwc)).permute(0, 3, 1, 2).float().div(255)
    return t.sub(torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)).div(torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1))


def _depth_tensor(a):
    return torch.from_numpy(a.astype(np.uint16).view(np.int16))


def replay_golden(path, device):
    """Runs the mirror module on ``device`` tensors with the recorded seed; asserts byte equality with the reference's output and
    the same state of both random streams afterwards."""
    from dense_correspondence.correspondence_tools import correspondence_augmentation as ca
    z = np.load(path)
    fn = str(z["fn"])
    rgb = torch.from_numpy(z["rgb"]).to(device)
    mask = torch.from_numpy(z["mask"]).to(device)
    random.seed(int(z["seed"]))
    np.random.seed(int(z["seed"]))
    if fn == "random_domain_randomize_background":
        out = ca.random_domain_randomize_background(rgb, mask)
        assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), z["out_rgb"])
    else:
        images = [rgb] + ([_depth_tensor(z["depth"]).to(device)] if "depth" in z.files else []) + [mask]
        uv = (torch.from_numpy(z["u"]).to(device), torch.from_numpy(z["v"]).to(device))
        out, (u, v) = getattr(ca, fn)(images, uv)
        assert np.array_equal(out[0].cpu().numpy(), z["out_rgb"])
        assert np.array_equal(out[-1].cpu().numpy(), z["out_mask"]) and out[-1].dtype == torch.uint8
        if "depth" in z.files:
            assert out[1].dtype == torch.int16
            assert np.array_equal(out[1].cpu().numpy().view(np.uint16), z["out_depth"])
        assert u.dtype == uv[0].dtype and np.array_equal(u.cpu().numpy(), z["out_u"])
        assert v.dtype == uv[1].dtype and np.array_equal(v.cpu().numpy(), z["out_v"])
    assert random.random() == float(z["after_random"][0])
    assert np.random.uniform() == float(z["after_numpy"][0])
