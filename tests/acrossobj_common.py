"""Shared by tests/test_emu_acrossobj.py and tests/test_gpu_acrossobj.py: the acrossobj goldens (the reference's own
``random_sample_from_masked_image`` and ``compute_descriptor_match_statistics_no_ground_truth`` on synthetic pairs,
tests/golden/make_acrossobj_goldens_from_reference.py) replayed through dcn_hip.evaluate, a three-object frame store and a
stand-in network whose descriptors are a fixed function of the image."""
import glob
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "acrossobj_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("acrossobj_ref_"):-4] for p in GOLDENS]


def golden_inputs(z, device):
    return {k: torch.from_numpy(np.ascontiguousarray(z[k])).to(device) for k in ("mask_a", "res_a", "res_b")}


def replay_order(z):
    """``rand_inds`` as a replay table: a pair with an empty mask has no ranks in the golden (-1); the kernel never reads its
    row, so any value does"""
    return np.maximum(z["rand_inds"], 0)


def check_queries(q, z):
    """Exact: the sampled pixels, the offsets, the mask's pixel counts; the query descriptors are res_a at those pixels"""
    assert int(q.status.cpu()[0]) == 0
    off = q.offsets.cpu().numpy()
    assert np.array_equal(off, z["offsets"])
    R = int(off[-1])
    ua, va = q.u_a.cpu().numpy(), q.v_a.cpu().numpy()
    assert np.array_equal(ua[:R], z["u_a"]) and np.array_equal(va[:R], z["v_a"])
    assert np.array_equal(q.mask_pixels.cpu().numpy(), (z["mask_a"] != 0).reshape(z["mask_a"].shape[0], -1).sum(1))
    want = z["res_a"][z["row_pair"], z["v_a"], z["u_a"]]
    assert np.array_equal(q.queries.cpu().numpy()[:R], want)
    assert (ua[R:] == -1).all() and (va[R:] == -1).all() and (q.queries.cpu().numpy()[R:] == 0).all()


def check_matches(m, z, rows=None):
    """Exact best pixel and pair of EVERY row (the generator keeps the best and second-best distances 1e-4 apart, and records
    the first of two equal minima); the distance at rtol 1e-5, the tolerance tests/evaluate_common.py applies to the
    descriptor-distance columns against the reference."""
    R = len(z["row_pair"]) if rows is None else rows
    assert int(m.status.cpu()[0]) == 0
    uv = m.best_uv.cpu().numpy()
    assert np.array_equal(uv[0, :R], z["u_b"]) and np.array_equal(uv[1, :R], z["v_b"])
    assert np.array_equal(m.row_pair.cpu().numpy()[:R], z["row_pair"])
    norm = m.norm_diff_descriptor_best_match.cpu().numpy()
    np.testing.assert_allclose(norm[:R], z["best_match_diff"], rtol=1e-5)
    assert np.isnan(norm[R:]).all() and (uv[:, R:] == -1).all() and (m.row_pair.cpu().numpy()[R:] == -1).all()


def check_golden(z, device):
    from dcn_hip import evaluate
    d = golden_inputs(z, device)
    q = evaluate.across_object_queries(d["mask_a"], d["res_a"], int(z["num_samples"]), sample_order=replay_order(z))
    check_queries(q, z)
    m = evaluate.best_match_pairs(d["res_b"], q.queries, q.offsets)
    check_matches(m, z)
    # the fixtures hold what they are named for
    w = z["res_b"].shape[2]
    flat = z["v_b"] * w + z["u_b"]
    assert (flat == 0).any() and (flat == z["res_b"].shape[1] * w - 1).any()
    return q, m


def three_object_store(device, h, w, seed=0, small_mask_object=None):
    """Three objects with 2, 1 and 2 scenes of 3, 2, 4, 2 and 3 frames; rectangular masks of at least a third of the image
    (object ``small_mask_object``: 5 pixels, fewer than any sample the tests ask for); random RGB."""
    from dcn_hip import frames
    rng = np.random.RandomState(seed)
    first, sobj = [0, 3, 5, 9, 11, 14], [0, 0, 1, 2, 2]
    F = first[-1]
    rgb = rng.randint(0, 256, (F, h, w, 3)).astype(np.uint8)
    depth = np.full((F, h, w), 900, np.uint16)
    mask = np.zeros((F, h, w), np.uint8)
    for s, o in enumerate(sobj):
        for f in range(first[s], first[s + 1]):
            if o == small_mask_object:
                mask[f, h // 2, 1:6] = 1
            else:
                mask[f, h // 6 + f % 3:5 * h // 6, w // 8 + f % 2:7 * w // 8] = 1
    poses = np.stack([np.eye(4)] * F)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return frames.FrameStore.from_tensors(c(rgb), c(depth.view(np.int16)), c(mask), poses, first, sobj,
                                          scene_names=["scene_%s" % n for n in "abcde"], object_ids=["mug", "shoe", "hat"],
                                          frame_ids=[list(range(10 * s, 10 * s + first[s + 1] - first[s])) for s in range(5)])


class StubNetwork(torch.nn.Module):
    """A ``dcn`` for the chain tests: D = 3 descriptors that are a fixed pointwise function of the normalized image, so that
    batched and per-image calls agree bit for bit (no convolution, no batch-shape dependence)."""

    def __init__(self):
        super().__init__()
        self.outputs = []                                   # per call: the descriptors of a's images, then of b's

    def forward_image_tensors(self, x):
        assert not self.training
        y = x.permute(0, 2, 3, 1).contiguous()
        out = torch.stack([y[..., 0] + 0.5 * y[..., 1], y[..., 1] * y[..., 2], y[..., 2] - 0.25 * y[..., 0]], dim=3).contiguous()
        self.outputs.append(out)
        return out

    def descriptors(self):
        """(res_a, res_b) of everything forwarded so far, in pair order"""
        half = [int(o.shape[0]) // 2 for o in self.outputs]
        return (torch.cat([o[:n] for o, n in zip(self.outputs, half)]), torch.cat([o[n:] for o, n in zip(self.outputs, half)]))
