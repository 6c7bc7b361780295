#!/usr/bin/env python3
"""Bitwise A/B of the device data path on the host emulation (no GPU): runs samples / frames / evaluate of THIS tree, with this
tree's emulation library, over a fixed matrix with fixed generator seeds and writes one sha256 per returned tensor.

    python tools/datapath_ab.py --out a.json          (in each of the two trees, a process of its own)
    python tools/datapath_ab.py --compare a.json b.json

Equal hashes mean equal bits in every output, and with them an unchanged number and order of draws from the generators.
Matrix: the five sample entry points x seeded / replay x 7 x 9 and 20 x 28 x n in {1, 3} x the flag combinations x with / without
RGB; select_frames for every data type on the stores of tests/frames_common.py; draw_training_batch with and without
per_pair_types; evaluate_frame_pairs and compute_descriptor_statistics_on_dataset on a 37 x 53 store."""
import argparse
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-dense-correspondence_amd"), ROOT):
    sys.path.insert(0, p)

TRAINING = {"training": {"num_matching_attempts": 60, "sample_matches_only_off_mask": True, "num_non_matches_per_match": 4,
                         "fraction_masked_non_matches": 0.5, "fraction_background_non_matches": 0.5,
                         "cross_scene_num_samples": 40, "use_image_b_mask_inv": True, "domain_randomize": True,
                         "data_type_probabilities": {"SINGLE_OBJECT_WITHIN_SCENE": 2.0, "SINGLE_OBJECT_ACROSS_SCENE": 1.0,
                                                     "DIFFERENT_OBJECT": 1.0, "MULTI_OBJECT": 0.0,
                                                     "SYNTHETIC_MULTI_OBJECT": 0.0}}}


def digest(x):
    if x is None:
        return "none"
    if torch.is_tensor(x):
        x = x.detach().cpu().contiguous()
        return hashlib.sha256(repr((str(x.dtype), tuple(x.shape))).encode() + x.numpy().tobytes()).hexdigest()
    if isinstance(x, np.ndarray):
        return hashlib.sha256(repr((str(x.dtype), x.shape)).encode() + np.ascontiguousarray(x).tobytes()).hexdigest()
    if isinstance(x, (tuple, list)):
        return hashlib.sha256("".join(digest(v) for v in x).encode()).hexdigest()
    return hashlib.sha256(repr(x).encode()).hexdigest()


def run_matrix():
    import datapath_common as dc
    import evaluate_common as ec
    import frames_common as fc
    from helpers import use_emulation_library
    use_emulation_library()
    from dcn_hip import evaluate, frames, samples
    out = {}

    def put(key, value):
        assert key not in out, key
        out[key] = digest(value)
    T = torch.from_numpy
    for (h, w), n, replay in itertools.product(((7, 9), (20, 28)), (1, 3), (False, True)):
        A, k1, k2, ns = (400 if h < 10 else 120), 2, 3, 25
        depth, masks, pa, pb = dc.example(n, h, w, seed=7)
        if n == 3:
            masks[1, 2] = 0
        da, db = T(depth[0].view(np.int16)), T(depth[1].view(np.int16))
        ma, mb = T(masks[0]), T(masks[1])
        rgb = torch.randint(0, 256, (2, n, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
        rng = np.random.RandomState(11)
        stream = lambda: [rng.rand(2 * A * k2 + h * w).astype(np.float32) for _ in range(n)]
        # (replay mode draws what is left -- augmentation records, order seeds -- from the global generator)
        rand = lambda: (torch.manual_seed(17), dict(draws={s: stream() for s in samples.SITES}) if replay else dict(
            generator=torch.Generator().manual_seed(5)))[1]
        tag = "%dx%d n%d %s" % (h, w, n, "replay" if replay else "seeded")
        batches = []
        for only_off, inv, with_rgb in itertools.product((False, True), (False, True), (False, True)):
            im = (rgb[0], rgb[1]) if with_rgb else (None, None)
            r = samples.build_within_scene_samples(da, db, ma, mb, pa, pb, dc.K_for(h), *im, num_matching_attempts=A,
                                                   sample_matches_only_off_mask=only_off, num_masked_non_matches_per_match=k1,
                                                   num_background_non_matches_per_match=k2, use_image_b_mask_inv=inv,
                                                   domain_randomize=True, **rand())
            put("within %s off%d inv%d rgb%d" % (tag, only_off, inv, with_rgb), r)
            batches.append(r)
        for with_rgb in (False, True):
            im = (rgb[0], rgb[1]) if with_rgb else (None, None)
            r = samples.build_across_scene_samples(ma, mb, *im, num_samples=ns, domain_randomize=True, **rand())
            put("across %s rgb%d" % (tag, with_rgb), r)
            batches.append(r)
        counts = rng.randint(0, 9, n)
        off = np.concatenate([[0], np.cumsum(counts)])
        uv = lambda hi: T(rng.randint(0, hi, int(off[-1])).astype(np.int64))
        ua, va, ub, vb = uv(w), uv(h), uv(w), uv(h)
        for inv, flt, with_params in itertools.product((False, True), (False, True), (False, True)):
            r = samples.complete_samples((ua, va), (ub.float(), vb.float()) if flt else (ub, vb), off.tolist() if inv else T(off),
                                         ma, mb, num_masked_non_matches_per_match=k1, num_background_non_matches_per_match=k2,
                                         use_image_b_mask_inv=inv,
                                         aug_params=dc.sc.params_from_flips([True] * n, [False] * n) if with_params else None,
                                         **rand())
            put("complete %s inv%d float%d params%d" % (tag, inv, flt, with_params), r)
        cams = samples._cameras(dc.K_for(h), pa, pb, n, torch.device("cpu"))
        put("cameras %s" % tag, cams)
        for num in (5, 500):
            kw = dict(draws={"cand": stream()}) if replay else dict(generator=torch.Generator().manual_seed(9))
            torch.manual_seed(19)
            m = evaluate.find_eval_matches(da, db, ma, cams, num, num_attempts=min(A, 100), **kw)
            put("eval %s num%d" % (tag, num), m)
            if replay:
                order = np.full((n, num), -1, np.int64)
                for p, t in enumerate(m.totals.tolist()):
                    k = min(num, t)
                    order[p, :k] = rng.permutation(t)[:k]
                put("eval %s num%d order" % (tag, num), evaluate.find_eval_matches(
                    da, db, ma, cams, num, num_attempts=min(A, 100), match_order=order, **kw))
        put("concat one %s" % tag, samples.concat_sample_batches(batches[:1]))
        put("concat within+across %s" % tag, samples.concat_sample_batches([batches[7], batches[9]]))
        put("concat all without rgb %s" % tag, samples.concat_sample_batches(batches[0:8:2] + batches[8:9]))
    for path, name in zip(fc.GOLDENS, fc.GOLDEN_IDS):
        z = np.load(path)
        for gather in (False, True):
            store, fb = fc.run_golden(z, "cpu", gather=gather)
            put("select replay %s gather%d" % (name, gather), fb)
            fb = frames.select_frames(store, 5, int(z["type"]), generator=torch.Generator().manual_seed(2), gather=gather)
            put("select seeded %s gather%d" % (name, gather), fb)
        put("store %s" % name, [store.scene_cams, store.poses, store.depth, store.mask, store.K] + store._tables)
    store = fc.store_from_golden(np.load(fc.GOLDENS[0]), "cpu", h=12, w=16)
    for per_pair, seed in itertools.product((False, True), range(4)):
        sb, dt, fb = frames.draw_training_batch(store, 6, TRAINING, generator=torch.Generator().manual_seed(seed),
                                                host_rng=np.random.RandomState(seed), per_pair_types=per_pair)
        put("draw_training_batch per_pair%d seed%d" % (per_pair, seed), [sb, np.asarray(dt), fb if per_pair else [fb]])
    import pytorch_segmentation_detection.models.resnet_dilated as rd
    from dense_correspondence.network.dense_correspondence_network import DenseCorrespondenceNetwork
    h, w = 37, 53
    torch.manual_seed(0)
    dcn = DenseCorrespondenceNetwork(rd.Resnet18_8s(num_classes=3, base_width=8), 3, image_width=w, image_height=h)
    dcn.config = {}
    store = ec.synthetic_store("cpu", h, w)
    chosen = evaluate.choose_pairs(store, 5, np.random.RandomState(2))
    put("choose_pairs", chosen)
    for batch_pairs in (2, 8):
        t = evaluate.evaluate_frame_pairs(dcn, store, chosen, 6, generator=torch.Generator().manual_seed(1),
                                          batch_pairs=batch_pairs)
        put("evaluate_frame_pairs batch%d" % batch_pairs, t)
    for num, step in ((5, 2), (4, 16)):
        d = evaluate.compute_descriptor_statistics_on_dataset(dcn, store, num_images=num, save_to_file=False,
                                                              host_rng=np.random.RandomState(1), batch_images=step)
        put("descriptor statistics n%d step%d" % (num, step), json.dumps(d, sort_keys=True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        x, y = (json.load(open(p)) for p in a.compare)
        differ = sorted(k for k in set(x) | set(y) if x.get(k) != y.get(k))
        print("%d runs, %d differ" % (len(set(x) | set(y)), len(differ)))
        for k in differ:
            print("  differs:", k)
        sys.exit(1 if differ else 0)
    out = run_matrix()
    if a.out:
        json.dump(out, open(a.out, "w"), indent=0, sort_keys=True)
    print("%d runs hashed" % len(out))


if __name__ == "__main__":
    main()
