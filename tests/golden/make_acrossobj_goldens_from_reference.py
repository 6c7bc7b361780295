"""Pins the across-object evaluation (csrc/acrossobj_kernels.hip, dcn_hip/evaluate/across_objects.py): executes the REFERENCE's own functions
-- read from the reference tree at run time through tests/reference_py3.py, never copied --
  correspondence_finder.random_sample_from_masked_image (correspondence_finder.py:68-90), with ``random.sample`` wrapped so
  that its ``rand_inds`` are recorded
  evaluation.py compute_descriptor_match_statistics_no_ground_truth (:977-1003) on a recording stand-in for
  DCNEvaluationPandaTemplateAcrossObject (whose ``columns`` are read from the reference's class and stored)
  dense_correspondence_network.py find_best_match (as make_evalpairs_goldens_from_reference.py loads it)
on seeded synthetic masks and descriptor images, the way single_across_object_image_pair_quantitative_analysis (:784-859)
chains them: sample ``num_samples`` pixels of mask a, then the best match over the whole of image b for each.

Stores per case in tests/golden/acrossobj_ref_*.npz: mask_a uint8 [P, H, W], res_a / res_b float32 [P, H, W, D], rand_inds
int32 [P, Q] (-1 for a pair with an empty mask), offsets int64 [P + 1], row_pair, u_a, v_a, u_b, v_b (int64 per row),
best_match_diff float32 per row, tie_rows (rows whose minimum is shared by two bit-identical pixels of res_b), columns.

Planted matches: in every case res_b's FIRST pixel is a copy of one query's descriptor and its LAST pixel a copy of another's
(best matches at flat index 0 and at the last pixel, distance 0); the 48x64 case also has two pixels that are copies of a
third query's descriptor, so the reference's first-minimum rule is recorded.  For every other row the generator ASSERTS that
the reference's best and second-best distances differ by more than 1e-4 relative, and moves to the next seed until that
holds: a test may demand the exact best pixel of every row.

    python tests/golden/make_acrossobj_goldens_from_reference.py
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_evalpairs_goldens_from_reference as me                                    # noqa: E402
from make_augmentation_goldens_from_reference import write_npz                       # noqa: E402

GAP = 1e-4


class Template(object):
    """what compute_descriptor_match_statistics_no_ground_truth fills"""

    def __init__(self):
        self.values = {}

    def set_value(self, key, value):
        self.values[key] = value


def load_reference():
    cf, _dce, _block, env, _read = me.load_reference()
    ev = open(me.EVAL).read().split("\n")
    ns = {"PandaDataFrameWrapper": type("PandaDataFrameWrapper", (object,), {"__init__": lambda self, columns: None})}
    exec(compile(me.class_source(ev, "DCNEvaluationPandaTemplateAcrossObject"), me.EVAL, "exec"), ns)
    columns = list(ns["DCNEvaluationPandaTemplateAcrossObject"].columns)
    fns = {"np": np, "DenseCorrespondenceNetwork": env["DenseCorrespondenceNetwork"],
           "DenseCorrespondenceEvaluation": env["DenseCorrespondenceEvaluation"],
           "DCNEvaluationPandaTemplateAcrossObject": Template}
    exec(compile(me.method_source(ev, "compute_descriptor_match_statistics_no_ground_truth"), me.EVAL, "exec"), fns)
    return cf, fns["compute_descriptor_match_statistics_no_ground_truth"], env["DenseCorrespondenceNetwork"].find_best_match, \
        columns


def sample(cf, mask, q, seed):
    """random_sample_from_masked_image with its rand_inds"""
    got = []
    real = random.sample

    def recording(population, k):
        out = real(population, k)
        got.append(list(out))
        return out
    random.seed(seed)
    random.sample = recording
    try:
        idx = cf.random_sample_from_masked_image(mask, q)
    finally:
        random.sample = real
    if len(idx) == 0:
        assert not got
        return None, None
    assert len(got) == 1 and len(got[0]) == q
    return idx, np.asarray(got[0], np.int32)


def build(cf, stats, fbm, shape, d, q, masks, seed, tie):
    """One attempt at a case -> dict, or None when a row's best and second-best distances are too close"""
    P = len(masks)
    h, w = shape
    rng = np.random.RandomState(seed)
    res_a = rng.randn(P, h, w, d).astype(np.float32)
    res_b = (res_a[:, ::-1, ::-1] + 0.7 * rng.randn(P, h, w, d)).astype(np.float32)   # (another object: no pixel-wise relation)
    z = dict(mask_a=np.stack(masks).astype(np.uint8), rand_inds=np.full((P, q), -1, np.int32), offsets=[0], row_pair=[],
             u_a=[], v_a=[], u_b=[], v_b=[], best_match_diff=[], tie_rows=[])
    for p in range(P):
        idx, inds = sample(cf, masks[p], q, 1000 * seed + p)
        if idx is None:
            z["offsets"].append(z["offsets"][-1])
            continue
        z["rand_inds"][p] = inds
        uv = [(int(idx[1][i]), int(idx[0][i])) for i in range(q)]
        # planted matches: query 0 at the first pixel, query 1 at the last one, query 2 twice (the tie)
        res_b[p, 0, 0] = res_a[p, uv[0][1], uv[0][0]]
        res_b[p, h - 1, w - 1] = res_a[p, uv[1][1], uv[1][0]]
        ties = []
        if tie and p == 0:
            flat = np.sort(rng.choice(np.arange(1, h * w - 1), 2, replace=False))
            for f in flat:
                res_b[p, f // w, f % w] = res_a[p, uv[2][1], uv[2][0]]
            ties = [2]
        for i in range(q):
            t = stats(list(uv[i]), res_a[p], res_b[p])
            uv_b, diff, norm_diffs = fbm(list(uv[i]), res_a[p], res_b[p])
            assert t.values["norm_diff_descriptor_best_match"] == diff and norm_diffs.dtype == np.float32
            two = np.sort(norm_diffs.reshape(-1))[:2]
            assert two[0] == diff
            if i in ties:
                assert two[0] == two[1] == 0 and int(uv_b[1]) * w + int(uv_b[0]) == flat[0], "the tie is not a tie"
                z["tie_rows"].append(len(z["row_pair"]))
            elif not (two[1] - two[0]) > GAP * two[1]:
                return None
            z["row_pair"].append(p)
            z["u_a"].append(uv[i][0])
            z["v_a"].append(uv[i][1])
            z["u_b"].append(int(uv_b[0]))
            z["v_b"].append(int(uv_b[1]))
            z["best_match_diff"].append(diff)
        z["offsets"].append(len(z["row_pair"]))
    z.update(res_a=res_a, res_b=res_b, seed=np.array(seed), num_samples=np.array(q))
    for k in ("offsets", "u_a", "v_a", "u_b", "v_b"):
        z[k] = np.asarray(z[k], np.int64)
    z["row_pair"] = np.asarray(z["row_pair"], np.int32)
    z["tie_rows"] = np.asarray(z["tie_rows"], np.int64)
    z["best_match_diff"] = np.asarray(z["best_match_diff"], np.float32)
    return z


def case(ref, name, shape, d, q, masks, tie=False):
    cf, stats, fbm, columns = ref
    h, w = shape
    z = None
    for seed in range(1, 200):
        z = build(cf, stats, fbm, shape, d, q, masks, seed, tie)
        if z is not None:
            break
    assert z is not None, name
    z["columns"] = np.array(columns)
    flat = z["v_b"] * w + z["u_b"]
    assert (flat == 0).any() and (flat == h * w - 1).any(), "no best match at the first / last pixel"
    assert len(z["tie_rows"]) == (1 if tie else 0)
    nonzero = (z["mask_a"].reshape(len(masks), -1) != 0).sum(1)
    assert np.array_equal(np.diff(z["offsets"]), np.where(nonzero > 0, q, 0))
    for p in range(len(masks)):                              # rand_inds index numpy's nonzero() order
        lo, hi = z["offsets"][p], z["offsets"][p + 1]
        on = np.flatnonzero(z["mask_a"][p].reshape(-1))
        assert hi == lo or np.array_equal(on[z["rand_inds"][p]], z["v_a"][lo:hi] * w + z["u_a"][lo:hi])
    path = os.path.join(HERE, "acrossobj_ref_%s.npz" % name)
    write_npz(path, z)
    assert os.path.getsize(path) < 1 << 20, (name, "too large")
    print(name, "seed", int(z["seed"]), "rows", len(z["row_pair"]), "mask pixels", nonzero.tolist(), "tie rows",
          z["tie_rows"].tolist(), "bytes", os.path.getsize(path))
    return z


def blob(rng, h, w, fraction):
    return (rng.rand(h, w) < fraction).astype(np.uint8) * 255


def main():
    ref = load_reference()
    assert ref[3][-1] == "norm_diff_descriptor_best_match" and len(ref[3]) == 7
    rng = np.random.RandomState(7)
    case(ref, "37x53_d16", (37, 53), 16, 100, [blob(rng, 37, 53, 0.3), blob(rng, 37, 53, 0.08)])
    masks = [blob(rng, 48, 64, 0.25), np.zeros((48, 64), np.uint8), blob(rng, 48, 64, 0.5)]
    case(ref, "48x64_d3", (48, 64), 3, 100, masks, tie=True)
    case(ref, "1x64_d1", (1, 64), 1, 7, [blob(rng, 1, 64, 0.5)])
    case(ref, "48x1_d1", (48, 1), 1, 7, [blob(rng, 48, 1, 0.5)])


if __name__ == "__main__":
    main()
