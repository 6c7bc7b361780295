"""Training samples on the device (csrc/sample_kernels.hip, dcn_hip/samples.py) through the host-emulation build: the reference's
own get_within_scene_data / get_across_scene_data replayed bit for bit, a batch with an empty pair against single-pair replays,
drawn mode against the numpy restatement, the output layout, and the loss fed from ``pair_lists()``."""
import numpy as np
import pytest
import torch

import samples_common as sc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.mark.parametrize("path", sc.GOLDENS, ids=sc.GOLDEN_IDS)
def test_golden_replays_bit_exactly(path):
    z = np.load(path)
    r = sc.run_golden_batch([z], "cpu")
    sc.check_golden(r, 0, z)
    sc.check_layout(r)


def test_golden_set_is_complete():
    for need in sc.REQUIRED_GOLDENS:
        assert need in sc.GOLDEN_IDS, need


def test_batch_with_an_empty_pair_equals_single_replays():
    zs = [np.load(sc.GOLDENS[sc.GOLDEN_IDS.index(k)]) for k in ("flip_a_48x64", "empty_mask_b_48x64", "normal_48x64")]
    zs[1] = dict(zs[1])
    zs[1]["mask_a"] = np.zeros_like(zs[1]["mask_a"])                 # pair 1 becomes empty (mask a)
    for k in ("k1", "k2", "A", "inv", "only_off_mask"):
        assert all(int(z[k]) == int(zs[0][k]) for z in zs)
    r = sc.run_golden_batch(zs, "cpu")
    sc.check_layout(r)
    assert r.empty.tolist() == [False, True, False] and r.type.tolist() == [0, -1, 0]
    for p in (0, 2):
        sc.check_golden(r, p, zs[p])
        single = sc.run_golden_batch([zs[p]], "cpu")
        for a, b in zip(sc.batch_lists(r, p), sc.batch_lists(single, 0)):
            assert np.array_equal(a, b)


def _pose(ry, t):
    T = np.eye(4)
    T[:3, :3] = [[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]]
    T[:3, 3] = t
    return T


def _example(n, h, w, seed):
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    depth, masks = np.zeros((2, n, h, w), np.uint16), np.zeros((2, n, h, w), np.uint8)
    for k in range(2):
        for p in range(n):
            d = 900 + 60 * np.sin(xs / (6 + 4 * rng.rand())) + 50 * np.cos(ys / (5 + 3 * rng.rand()))
            d[rng.rand(h, w) < 0.05] = 0
            depth[k, p] = d.astype(np.uint16)
            cy, cx = rng.rand() * h, rng.rand() * w
            masks[k, p] = (((ys - cy) / (0.35 * h)) ** 2 + ((xs - cx) / (0.35 * w)) ** 2) <= 1.0
    pa = np.stack([_pose(0, [0, 0, 0])] * n)
    pb = np.stack([_pose(-0.003, [0.004, 0.002 * p, 0.001]) for p in range(n)])
    return depth, masks, pa, pb


@pytest.mark.parametrize("only_off,inv,h,w", [(True, True, 20, 28), (False, False, 20, 28), (True, True, 7, 9)])
def test_drawn_mode_matches_restatement(only_off, inv, h, w):
    """(7 x 9: more attempts than pixels)"""
    from dcn_hip import samples
    n, k1, k2 = 3, 2, 3
    A = 120 if h > 10 else 400
    depth, masks, pa, pb = _example(n, h, w, seed=7)
    masks[1, 2] = 0                                                  # pair 2: empty mask b (uniform fallbacks, no blind)
    t = lambda a: torch.from_numpy(a)
    params = sc.params_from_flips([True, False, True], [False, True, True])
    g = torch.Generator().manual_seed(5)
    K = sc.default_K() if h > 10 else np.array([[20.0, 0, 4.2], [0, 20.0, 3.1], [0, 0, 1]])
    r = samples.build_within_scene_samples(t(depth[0].view(np.int16)), t(depth[1].view(np.int16)), t(masks[0]), t(masks[1]),
                                           pa, pb, K, num_matching_attempts=A, sample_matches_only_off_mask=only_off,
                                           num_masked_non_matches_per_match=k1, num_background_non_matches_per_match=k2,
                                           use_image_b_mask_inv=inv, generator=g, aug_params=params)
    sc.check_layout(r)
    assert r.seeds.dtype == torch.int64 and r.seeds.shape == (n,)
    assert not bool(r.empty[0])
    if A > h * w:
        assert int(r.offsets[1] - r.offsets[0]) > h * w                # more matches than pixels
    for p in range(n):
        U = lambda site, k, s=int(r.seeds[p]): sc.hash_uniform(s, site, k)
        lists, typ = sc.restated_within(depth[0, p], depth[1, p], masks[0, p], masks[1, p], sc.cams_of(K, pa[p], pb[p]),
                                        params[p, 0] != 0, params[n + p, 0] != 0, A, only_off, k1, k2, inv, U)
        sc.check_against_restatement(r, p, lists, typ)
    r2 = samples.build_within_scene_samples(t(depth[0].view(np.int16)), t(depth[1].view(np.int16)), t(masks[0]), t(masks[1]),
                                            pa, pb, K, num_matching_attempts=A, sample_matches_only_off_mask=only_off,
                                            num_masked_non_matches_per_match=k1, num_background_non_matches_per_match=k2,
                                            use_image_b_mask_inv=inv, seeds=r.seeds, aug_params=params)
    assert torch.equal(r.idx_a, r2.idx_a) and torch.equal(r.idx_b, r2.idx_b) and torch.equal(r.offsets, r2.offsets)


def test_across_scene_drawn_matches_restatement():
    from dcn_hip import samples
    n, h, w, ns = 3, 12, 17, 25
    _, masks, _, _ = _example(n, h, w, seed=3)
    masks[0, 1] = 0
    params = sc.params_from_flips([True, False, False], [False, True, True])
    r = samples.build_across_scene_samples(torch.from_numpy(masks[0]), torch.from_numpy(masks[1]), num_samples=ns,
                                           generator=torch.Generator().manual_seed(2), aug_params=params,
                                           data_type=samples.DIFFERENT_OBJECT)
    sc.check_layout(r)
    assert r.type.tolist() == [2, -1, 2]
    for p in range(n):
        U = lambda site, k, s=int(r.seeds[p]): sc.hash_uniform(s, site, k)
        lists, typ = sc.restated_across(masks[0, p], masks[1, p], params[p, 0] != 0, params[n + p, 0] != 0, ns, U)
        sc.check_against_restatement(r, p, lists, 2 if typ == 1 else -1)


def test_complete_samples_matches_restated_tail():
    """complete_samples on given match lists = the within recipe's steps after the matches (no rotation)."""
    from dcn_hip import samples
    n, h, w, k1, k2 = 2, 10, 13, 2, 2
    _, masks, _, _ = _example(n, h, w, seed=4)
    rng = np.random.RandomState(1)
    counts = [7, 0]
    ua, va = rng.randint(0, w, 7), rng.randint(0, h, 7)
    ub, vb = rng.randint(0, w, 7), rng.randint(0, h, 7)
    cap_tail = np.full(5, -1)
    T = lambda a: torch.from_numpy(np.concatenate([a, cap_tail]).astype(np.int64))
    r = samples.complete_samples((T(ua), T(va)), (T(ub), T(vb)), [0, 7, 7], torch.from_numpy(masks[0]),
                                 torch.from_numpy(masks[1]), num_masked_non_matches_per_match=k1,
                                 num_background_non_matches_per_match=k2, use_image_b_mask_inv=True,
                                 generator=torch.Generator().manual_seed(9))
    sc.check_layout(r)
    assert r.empty.tolist() == [False, True] and counts[1] == 0
    got = sc.batch_lists(r, 0)
    assert np.array_equal(got[0], va * w + ua) and np.array_equal(got[1], vb * w + ub)
    U = lambda site, k, s=int(r.seeds[0]): sc.hash_uniform(s, site, k)
    lb = np.flatnonzero(masks[1, 0].reshape(-1))
    assert np.array_equal(got[2], np.repeat(va * w + ua, k1))
    assert np.array_equal(got[3], [sc._pick(lb, U(1, e)) for e in range(7 * k1)])
    matched = np.zeros(h * w, np.int64)
    matched[va * w + ua] = 1
    assert np.array_equal(got[6], np.flatnonzero((masks[0, 0].reshape(-1) != 0) - matched))


def test_replay_stream_too_short_sets_status():
    from dcn_hip import samples
    z = np.load(sc.GOLDENS[sc.GOLDEN_IDS.index("across_48x64")])
    r = samples.build_across_scene_samples(torch.from_numpy(z["mask_a"][None]), torch.from_numpy(z["mask_b"][None]),
                                           num_samples=int(z["n_across"]),
                                           draws={"across_a": [z["rand_across_a"][:5]], "across_b": [z["rand_across_b"]]})
    assert int(r.status[0]) & samples.BAD_DRAWS


def test_options_from_config_rounds_like_the_reference():
    from dcn_hip import samples
    cfg = {"training": dict(num_matching_attempts=10000, sample_matches_only_off_mask=True, num_non_matches_per_match=150,
                            fraction_masked_non_matches=0.5, fraction_background_non_matches=0.5, use_image_b_mask_inv=True,
                            cross_scene_num_samples=10000, domain_randomize=False)}
    o = samples.options_from_config(cfg)
    assert (o.num_matching_attempts, o.num_masked_non_matches_per_match, o.num_background_non_matches_per_match) == (10000, 75, 75)
    cfg["training"]["fraction_masked_non_matches"] = 0.333
    assert samples.options_from_config(cfg).num_masked_non_matches_per_match == int(0.333 * 150)


def test_pair_lists_feed_the_batched_loss_like_from_lists():
    from dcn_hip.loss import PairLists
    from dense_correspondence.dataset.spartan_dataset_masked import SpartanDatasetDataType
    from dense_correspondence.loss_functions import loss_composer
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    from oracle import synth
    zs = [np.load(sc.GOLDENS[sc.GOLDEN_IDS.index(k)]) for k in ("flip_b_48x64", "no_match_37x53")]
    zs[1] = np.load(sc.GOLDENS[sc.GOLDEN_IDS.index("normal_48x64")])
    r = sc.run_golden_batch(zs, "cpu")
    h, w, D = 48, 64, 3
    pcl = PixelwiseContrastiveLoss(image_shape=(h, w), config=synth.LOSS_CONFIG)
    torch.manual_seed(0)
    ya, yb = torch.randn(2, h * w, D), torch.randn(2, h * w, D)
    tuples = [tuple(torch.from_numpy(z[k]) for k in sc.KEYS) for z in zs]
    dt = SpartanDatasetDataType.SINGLE_OBJECT_WITHIN_SCENE
    got = loss_composer.get_loss_batched(pcl, dt, ya, yb, r.pair_lists())[0]
    want = loss_composer.get_loss_batched(pcl, dt, ya, yb, PairLists.from_lists(tuples, "cpu", hw=h * w))[0]
    assert torch.equal(got, want)
