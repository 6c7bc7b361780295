"""Device augmentation (csrc/augment_kernels.hip) through the host-emulation build: the mirror module against the reference's
golden outputs, the batched path against a numpy restatement of the rules and torch's normalization, the flip kernels, and the
drop-in behaviour for PIL inputs (against the reference's own module, when /root/reference is there)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_common as ac
from helpers import PKG, ROOT, use_emulation_library

REFERENCE = "/root/reference"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.mark.parametrize("path", ac.GOLDENS, ids=ac.GOLDEN_IDS)
def test_mirror_replays_reference_golden(path):
    ac.replay_golden(path, "cpu")


def test_golden_set_is_complete():
    ids = set(ac.GOLDEN_IDS)
    for need in ("bg_solid", "bg_solid_noise", "bg_gradient_vertical", "bg_gradient_vertical_noise", "bg_gradient_horizontal",
                 "bg_gradient_horizontal_noise", "bg_kept_37x53", "mutation_rgb_mask_int64_rotated",
                 "mutation_rgb_mask_int64_kept", "mutation_rgb_depth_mask_float32_rotated", "flip_vertical_37x53",
                 "flip_horizontal_37x53", "bg_gradient_vertical_1x64", "bg_gradient_horizontal_48x1"):
        assert need in ids, need


@pytest.mark.parametrize("h,w", [(24, 36), (13, 17), (1, 8), (9, 1)])
def test_batched_path_with_explicit_params_matches_restatement(h, w):
    from dcn_hip import augment
    B = 5
    rgb, mask = ac.scene(2 * B, h, w, seed=h * 100 + w)
    rec = ac.example_params(2 * B, seed=w)
    n_uv = [3, 0, 5, 1, 2]
    off = np.concatenate([[0], np.cumsum(n_uv)])
    rng = np.random.RandomState(1)
    ua = rng.randint(0, w, size=off[-1]).astype(np.int64)
    va = rng.randint(0, h, size=off[-1]).astype(np.int64)
    ub = (rng.randint(0, w, size=off[-1]) + rng.rand(off[-1])).astype(np.float32)
    vb = (rng.randint(0, h, size=off[-1]) + rng.rand(off[-1])).astype(np.float32)
    t = torch.from_numpy
    r = augment.augment_image_pairs(t(rgb[:B]), t(rgb[B:]), t(mask[:B]), t(mask[B:]), (t(ua), t(va)), (t(ub), t(vb)),
                                    offsets=off, params=t(rec), return_rgb=True)
    assert r.input_a.shape == (B, 3, h, w) and r.input_a.dtype == torch.float32
    for k in range(2 * B):
        side, i = divmod(k, B)
        exp_rgb, exp_mask = ac.restated_augment(rgb[k], mask[k], rec[k], k)
        got_rgb = (r.rgb_b if side else r.rgb_a)[i].numpy()
        got_mask = (r.mask_b if side else r.mask_a)[i].numpy()
        assert np.array_equal(got_rgb, exp_rgb), (k, rec[k])
        assert np.array_equal(got_mask, exp_mask.astype(np.float32)), k
        got_in = (r.input_b if side else r.input_a)[i:i + 1]
        exp_in = ac.normalize_torch(exp_rgb[None], augment.DEFAULT_IMAGE_MEAN, augment.DEFAULT_IMAGE_STD_DEV)
        assert torch.equal(got_in, exp_in), k
    for b in range(B):
        s = slice(off[b], off[b + 1])
        eu, ev = ac.restated_uv(ua[s], va[s], rec[b], h, w)
        assert np.array_equal(r.uv_a[0][s].numpy(), eu) and np.array_equal(r.uv_a[1][s].numpy(), ev)
        eu, ev = ac.restated_uv(ub[s], vb[s], rec[B + b], h, w)
        assert r.uv_b[0].dtype == torch.float32
        assert np.array_equal(r.uv_b[0][s].numpy(), eu) and np.array_equal(r.uv_b[1][s].numpy(), ev)
    assert torch.equal(r.params, t(rec))


def test_float_uv_flip_is_torchs_rsub():
    """(W-1) - t in float32 is one rounding; the kernel's result equals torch's bit for bit, fractional values included."""
    from dcn_hip import augment
    u = torch.tensor([0.0, 0.1, 639.0, 638.99997, 1e-8, 319.5, -0.0], dtype=torch.float32)
    v = torch.tensor([0.3, 479.0, 1e-7, 12.625, 0.0, 478.99997, 5.0], dtype=torch.float32)
    fu, fv = augment.flip_uv((u, v), 480, 640)
    assert torch.equal(fu, (640 - 1) - u) and torch.equal(fv, (480 - 1) - v)


@pytest.mark.parametrize("shape,dtype", [((5, 7, 3), torch.uint8), ((5, 7), torch.uint8), ((6, 9), torch.int16),
                                         ((4, 6, 1), torch.float32), ((3, 8, 3), torch.float32), ((2, 3, 5, 2), torch.uint8),
                                         ((1, 11, 3), torch.uint8), ((10, 1), torch.int16)])
def test_flip_planes_any_pixel_size(shape, dtype):
    from dcn_hip import augment
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(shape, generator=g) * 1000).to(dtype)
    pixel_dims = len(shape) - 2 if len(shape) == 3 else 0
    hd = len(shape) - pixel_dims - 2
    for fv, fh in ((1, 0), (0, 1), (1, 1)):
        dims = ([hd] if fv else []) + ([hd + 1] if fh else [])
        y = augment.flip_planes(x, fv, fh, pixel_dims=pixel_dims)
        assert y.dtype == x.dtype and torch.equal(y, torch.flip(x, dims)), (fv, fh)


def test_draw_params_layout_and_replay():
    from dcn_hip import augment
    p = augment.draw_params(64, "cpu", generator=torch.Generator().manual_seed(7))
    assert p.dtype == torch.int32 and p.shape == (64, augment.PARAM_WORDS)
    f = p[:, 0]
    assert bool(((f & ~63) == 0).all()) and bool((((f & 1) != 0) == ((f & 2) != 0)).all())   # rotation = both flips
    assert bool(((f & (8 | 16 | 32)) == 0)[(f & 4) == 0].all())                             # nothing without randomize
    assert bool((p[:, 1:7] >= 0).all() and (p[:, 1:7] <= 254).all()) and bool((p[:, 7] == 0).all())
    assert bool((p[:, 10:] == 0).all())
    q = augment.draw_params(64, "cpu", generator=torch.Generator().manual_seed(7))
    assert torch.equal(p, q)
    none = augment.draw_params(64, "cpu", generator=torch.Generator().manual_seed(7), domain_randomize=False, flip=False)
    assert bool((none[:, 0] == 0).all())


def test_bad_arguments_raise():
    from dcn_hip import augment
    rgb = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    mask = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError):
        augment.augment_image_pairs(rgb.float(), rgb, mask, mask)
    with pytest.raises(ValueError):
        augment.augment_image_pairs(rgb, rgb, mask[:, :4], mask)
    with pytest.raises(ValueError):   # two images need offsets to split the lists
        augment.augment_image_pairs(rgb, rgb, mask, mask, uv_a=(torch.zeros(3).long(), torch.zeros(3).long()))
    with pytest.raises(TypeError):
        augment.flip_uv((torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)), 8, 8)


def test_mirror_without_reference_refuses_pil_inputs_with_reason():
    """Without the reference's module behind this root, a PIL / numpy input is an error that says why (no quiet fallback)."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from dense_correspondence.correspondence_tools import correspondence_augmentation as ca
try:
    ca.random_domain_randomize_background(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8))
except TypeError as e:
    assert "reference" in str(e), e
    print("refused")
""" % (ROOT, PKG)
    env = dict(os.environ, PYTHONPATH="", DCN_QUIET_SHIMS="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd="/", stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         timeout=120)
    assert out.returncode == 0 and b"refused" in out.stdout, out.stdout.decode()


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference source tree")
def test_dropin_pil_inputs_go_to_the_reference_module():
    """With the reference's root behind this one, PIL inputs through this root's module give exactly what the reference's own
    module gives (same outputs, same random-stream consumption; the reference's flips raise the same NameError under Python 3)."""
    code = r"""
import random, sys, importlib.util
sys.path[:0] = [%r, %r]
sys.path.append(%r)
import numpy as np
from PIL import Image
from dense_correspondence.correspondence_tools import correspondence_augmentation as ca
assert ca.__file__.startswith(%r), ca.__file__
spec = importlib.util.spec_from_file_location("ref_aug", %r)
ref = importlib.util.module_from_spec(spec); spec.loader.exec_module(ref)
assert ca._ref.get() is not None
rng = np.random.RandomState(0)
rgb = Image.fromarray(rng.randint(0, 256, (31, 45, 3)).astype(np.uint8))
mask = Image.fromarray((rng.rand(31, 45) > 0.4).astype(np.uint8))
import torch
uv = (torch.arange(5), torch.arange(5) * 2)
def run(mod, s, what):
    random.seed(s); np.random.seed(s)
    try:
        if what == "bg":
            out = np.asarray(mod.random_domain_randomize_background(rgb, mask))
        else:
            imgs, (u, v) = mod.random_image_and_indices_mutation([rgb, mask], uv)
            out = np.concatenate([np.asarray(imgs[0]).ravel(), np.asarray(imgs[1]).ravel(), u.numpy(), v.numpy()])
    except Exception as e:
        out = type(e).__name__
    return out, random.random(), np.random.uniform()
for s in range(24):
    for what in ("bg", "mut"):
        a, b = run(ca, s, what), run(ref, s, what)
        assert (a[0] == b[0] if isinstance(a[0], str) else np.array_equal(a[0], b[0])) and a[1:] == b[1:], (s, what)
print("dropin-ok")
""" % (ROOT, PKG, REFERENCE, PKG, os.path.join(REFERENCE, "dense_correspondence", "correspondence_tools",
                                              "correspondence_augmentation.py"))
    env = dict(os.environ, PYTHONPATH="", DCN_QUIET_SHIMS="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd="/", stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         timeout=300)
    assert out.returncode == 0 and b"dropin-ok" in out.stdout, out.stdout.decode()
