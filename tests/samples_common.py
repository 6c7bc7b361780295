"""Shared by tests/test_emu_samples.py and tests/test_gpu_samples.py (not a test module): golden replay of the reference's own
get_within_scene_data / get_across_scene_data (tests/golden/sample_ref_*.npz) through dcn_hip.samples, and a numpy
restatement of the sample recipe (include/dcn_hip.h section 9, after spartan_dataset_masked.py:577-858, :1056-1141 and
correspondence_finder.py) including the counter-based hash of drawn mode."""
import glob
import os

import numpy as np
import torch

GOLDENS = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("sample_ref_"):-4] for p in GOLDENS]
REQUIRED_GOLDENS = ("normal_48x64", "off_mask_matches_37x53", "empty_mask_a_37x53", "no_match_37x53", "empty_mask_b_48x64",
                    "no_mask_inv_48x64", "flip_a_48x64", "flip_b_48x64", "flip_ab_37x53", "across_48x64",
                    "across_empty_b_37x53")
SITES = ("cand", "masked", "background", "blind", "across_a", "across_b")
KEYS = ("matches_a", "matches_b", "masked_a", "masked_b", "background_a", "background_b", "blind_a", "blind_b")
FLIPS = 3                                                   # augment.FLIP_V | FLIP_H


def default_K():
    K = np.zeros((3, 3))
    K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[2, 2] = 533.6422696034836, 534.7824445233571, 319.4091030774892, 236.4374299691866, 1.0
    return K


def params_from_flips(flips_a, flips_b):
    """[2B, 16] int32 records with only the rotation bits (domain randomization off)."""
    p = np.zeros((2 * len(flips_a), 16), np.int32)
    p[:len(flips_a), 0] = [FLIPS if f else 0 for f in flips_a]
    p[len(flips_a):, 0] = [FLIPS if f else 0 for f in flips_b]
    return p


def golden_lists(z):
    """The reference's 8 lists with its [-1] sentinels dropped (PairLists.from_lists skips them)."""
    out = []
    for k in KEYS:
        a = z[k]
        out.append(np.zeros(0, np.int64) if (a.size == 1 and a[0] == -1) else a)
    return out


def golden_inputs(z):
    flips = list(z["flips"]) + [False, False]
    d16 = lambda a: torch.from_numpy(a.astype(np.uint16).view(np.int16))
    return dict(flips=(bool(flips[0]), bool(flips[1])), depth_a=d16(z["depth_a"]), depth_b=d16(z["depth_b"]),
                mask_a=torch.from_numpy(z["mask_a"]), mask_b=torch.from_numpy(z["mask_b"]))


def run_golden_batch(zs, device):
    """One batched call over the goldens ``zs`` (all within-scene or all across-scene, one image size) with their recorded
    draws and flips."""
    from dcn_hip import samples
    ins = [golden_inputs(z) for z in zs]
    st = lambda k: torch.stack([x[k] for x in ins]).to(device)
    params = torch.from_numpy(params_from_flips([x["flips"][0] for x in ins], [x["flips"][1] for x in ins]))
    draws = {s: [z["rand_" + s] for z in zs] for s in SITES}
    z0 = zs[0]
    if bool(z0["across"]):
        return samples.build_across_scene_samples(st("mask_a"), st("mask_b"), num_samples=int(z0["n_across"]), draws=draws,
                                                  aug_params=params)
    return samples.build_within_scene_samples(
        st("depth_a"), st("depth_b"), st("mask_a"), st("mask_b"), np.stack([z["pose_a"] for z in zs]),
        np.stack([z["pose_b"] for z in zs]), num_matching_attempts=int(z0["A"]),
        sample_matches_only_off_mask=bool(z0["only_off_mask"]), num_masked_non_matches_per_match=int(z0["k1"]),
        num_background_non_matches_per_match=int(z0["k2"]), use_image_b_mask_inv=bool(z0["inv"]), draws=draws,
        aug_params=params)


def batch_lists(r, p):
    """Pair p's 8 lists (a, b per type) from a SampleBatch."""
    off = r.offsets.cpu().numpy()
    ia, ib = r.idx_a.cpu().numpy(), r.idx_b.cpu().numpy()
    out = []
    for t in range(4):
        sl = slice(int(off[4 * p + t]), int(off[4 * p + t + 1]))
        out += [ia[sl], ib[sl]]
    return out


def check_golden(r, p, z):
    got = batch_lists(r, p)
    for k, g, e in zip(KEYS, got, golden_lists(z)):
        assert np.array_equal(g, e), (k, g[:8], e[:8], len(g), len(e))
    assert int(r.type.cpu()[p]) == int(z["type"])
    assert bool(r.empty.cpu()[p]) == (int(z["type"]) == -1)


# ---- numpy restatement -------------------------------------------------------------------------------------------------

def _mix32(x):
    x = np.uint32(x)
    x ^= x >> np.uint32(16)
    x = np.uint32((int(x) * 0x7feb352d) & 0xffffffff)
    x ^= x >> np.uint32(15)
    x = np.uint32((int(x) * 0x846ca68b) & 0xffffffff)
    x ^= x >> np.uint32(16)
    return int(x)


def hash_uniform(seed, site, idx):
    """The kernels' drawn-mode uniform (sample_kernels.hip ``uniform``)."""
    s = int(seed) & 0xffffffffffffffff
    k0 = _mix32((s & 0xffffffff) ^ _mix32((site * 0x9E3779B9 + 0x7F4A7C15) & 0xffffffff))
    k1 = _mix32((s >> 32) ^ k0)
    r = _mix32(_mix32((idx & 0xffffffff) ^ k0) ^ ((k1 + (idx >> 32)) & 0xffffffff))
    return np.float32(r >> 8) * np.float32(1.0 / 16777216.0)


def replay_uniform(streams):
    """U(site, k) from the reference's recorded streams {site: array}."""
    return lambda site, k: np.float32(streams[SITES[site]][k])


def _pick(lst, r):
    j = int(np.floor(np.float32(r) * np.float32(len(lst))))
    return int(lst[min(max(j, 0), len(lst) - 1)])


def _project(depth_a, depth_b, cam, u, v):
    f = np.float32
    h, w = depth_a.shape
    K, Ki, Ta, Tb = cam[0:9], cam[9:18], cam[18:34], cam[34:50]
    r3 = lambda m, x, y, z: m[0] * x + m[1] * y + m[2] * z
    r4 = lambda m, x, y, z: m[0] * x + m[1] * y + m[2] * z + m[3] * f(1)
    d = f(depth_a[v, u]) * f(1) / f(1000)
    if d == 0:
        return None
    fx, fy, fz = f(u) * d, f(v) * d, d
    c = [r3(Ki[3 * i:], fx, fy, fz) for i in range(3)]
    wv = [r4(Ta[4 * i:], *c) for i in range(3)]
    b = [r4(Tb[4 * i:], *wv) for i in range(3)]
    p = [r3(K[3 * i:], *b) for i in range(3)]
    u2, v2 = p[0] / p[2], p[1] / p[2]
    if not (u2 > 0 and u2 <= f(w) * f(1) - f(1e-3) and v2 > 0 and v2 <= f(h) * f(1) - f(1e-3)):
        return None
    d2 = f(depth_b[int(v2), int(u2)]) * f(1) / f(1000)
    return (u2, v2) if (d2 > 0 and not d2 < p[2] - f(0.003)) else None


def cams_of(K, pose_a, pose_b):
    from dcn_hip.pairgen import invert_rigid
    f = lambda a: np.asarray(a, np.float64).astype(np.float32).reshape(-1)
    return np.concatenate([f(K), f(np.linalg.inv(K)), f(pose_a), f(invert_rigid(pose_b))])


def restated_within(depth_a, depth_b, mask_a, mask_b, cam, flip_a, flip_b, A, only_off, k1, k2, inv, U):
    """One pair -> (8 lists, type 0 / -1).  U(site, k): the uniform numbers."""
    h, w = mask_a.shape
    empty = [np.zeros(0, np.int64)] * 8, -1
    if only_off:
        la = np.flatnonzero(mask_a.reshape(-1))
        if la.size == 0:
            return empty
        cand = [(_pick(la, U(0, i)) % w, _pick(la, U(0, i)) // w) for i in range(A)]
    else:
        cand = [(int(np.floor(U(0, i) * np.float32(w))), int(np.floor(U(0, A + i) * np.float32(h)))) for i in range(A)]
    matches = []
    for u, v in cand:
        pr = _project(depth_a.astype(np.uint16), depth_b.astype(np.uint16), cam, u, v)
        if pr is not None:
            matches.append((u, v, pr[0], pr[1]))
    if not matches:
        return empty
    ma, mb = [], []
    for u, v, u2, v2 in matches:
        if flip_a:
            u, v = w - 1 - u, h - 1 - v
        if flip_b:
            u2, v2 = np.float32(w - 1) - u2, np.float32(h - 1) - v2
        ma.append(v * w + u)
        mb.append(int(v2) * w + int(u2))
    ma, mb = np.array(ma, np.int64), np.array(mb, np.int64)
    M = len(ma)
    rot = lambda m, f: m[::-1, ::-1] if f else m
    ra, rb = rot(mask_a, flip_a).reshape(-1), rot(mask_b, flip_b).reshape(-1)
    lb, linv = np.flatnonzero(rb), np.flatnonzero(rb == 0)

    def nonmatch(k, site, lst):
        n = M * k
        if lst is not None and lst.size:
            b = [_pick(lst, U(site, e)) for e in range(n)]
        else:
            b = [int(np.floor(U(site, n + e) * np.float32(h))) * w + int(np.floor(U(site, e) * np.float32(w)))
                 for e in range(n)]
        return np.repeat(ma, k), np.array(b, np.int64)
    m1a, m1b = nonmatch(k1, 1, lb)
    m2a, m2b = nonmatch(k2, 2, linv if inv else None)
    matched = np.zeros(h * w, np.int64)
    matched[ma] = 1
    blind_a = np.flatnonzero((ra != 0).astype(np.int64) - matched)
    if blind_a.size and lb.size:
        blind_b = np.array([_pick(lb, U(3, e)) for e in range(blind_a.size)], np.int64)
    else:
        blind_a = blind_b = np.zeros(0, np.int64)
    return [ma, mb, m1a, m1b, m2a, m2b, blind_a, blind_b], 0


def restated_across(mask_a, mask_b, flip_a, flip_b, n, U):
    h, w = mask_a.shape
    la, lb = np.flatnonzero(mask_a.reshape(-1)), np.flatnonzero(mask_b.reshape(-1))
    z = np.zeros(0, np.int64)
    if la.size == 0 or lb.size == 0:
        return [z] * 8, -1

    def draw(lst, site, f):
        out = []
        for e in range(n):
            p = _pick(lst, U(site, e))
            u, v = p % w, p // w
            if f:
                u, v = w - 1 - u, h - 1 - v
            out.append(v * w + u)
        return np.array(out, np.int64)
    return [z] * 6 + [draw(la, 4, flip_a), draw(lb, 5, flip_b)], 1


def check_against_restatement(r, p, lists, typ):
    got = batch_lists(r, p)
    for t, (g, e) in enumerate(zip(got, lists)):
        assert np.array_equal(g, e), (p, KEYS[t], g[:8], e[:8], len(g), len(e))
    assert int(r.type.cpu()[p]) == typ


def check_layout(r):
    """offsets increasing from 0, tail -1, empty pairs with no entries, status 0."""
    off = r.offsets.cpu().numpy()
    n = r.empty.numel()
    assert off[0] == 0 and bool((np.diff(off) >= 0).all()) and off.size == 4 * n + 1
    tail = r.idx_a.cpu().numpy()[off[-1]:]
    assert bool((tail == -1).all()) and bool((r.idx_b.cpu().numpy()[off[-1]:] == -1).all())
    for p in range(n):
        if bool(r.empty[p]):
            assert off[4 * p + 4] == off[4 * p] and int(r.type[p]) == -1
    assert int(r.status.cpu()[0]) == 0
