"""The loss on device-built batches (dcn_contrastive_loss_mixed_*, dcn_concat_samples; loss_composer.get_loss_mixed,
samples.concat_sample_batches, frames.draw_training_batch(per_pair_types=True)) through the C ABI -- kernels compiled for the
host (tests/hostemu).  CPU only; the same properties at training sizes on the gfx950 build are in test_gpu_loss_mixed.py.

Yardsticks: ``get_loss_batched`` (the one-type call the mixed call must reproduce bit for bit where both apply), the oracle
(oracle/loss_oracle.py) and the reference's own goldens (tests/golden/loss_ref_*.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frames_common as fc
import loss_mixed_common as mc
from helpers import lists_from_golden, load_golden_loss, rel_err, use_emulation_library
from loss_mixed_common import (ACROSS, DIFFERENT, MULTI, SYNTHETIC, WITHIN, descriptors, device_lists, make_lists, pcl_for,
                               run_batched, run_mixed)

GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.fixture
def exact(monkeypatch):
    """DCN_LOSS_EXACT=1: the order-independent backward in both calls (the module reads the variable once, at import)."""
    from dcn_hip import loss as K
    monkeypatch.setattr(K, "EXACT_BACKWARD", True)


SIZES = [(50, 1100, 70, 33), (1, 3, 2, 5), (2049, 5, 1025, 600)]   # crosses the pairs-per-workgroup chunk boundaries


# ------------------------------------------------------------------------------------------------ 1. one type, no empty pair
@pytest.mark.parametrize("D", [3, 16])
@pytest.mark.parametrize("code", [WITHIN, DIFFERENT, ACROSS], ids=["within_scene", "different_object", "across_scene"])
def test_uniform_type_equals_the_batched_call_bit_for_bit(code, D, exact):
    H, W, B = 24, 32, 3
    g = torch.Generator().manual_seed(17 + code)
    pairs = [make_lists(code, H * W, s, g) for s in SIZES]
    A, Bt = descriptors(B, H * W, D, 5)
    pcl = pcl_for(H, W)
    ref = run_batched(pcl, code, A, Bt, pairs)
    got = run_mixed(pcl, A, Bt, device_lists(pairs, [code] * B))
    assert got["status"] == 0 and got["num_valid"] == B
    assert float(ref["loss"]) > 0
    for k in ("loss", "terms", "hard", "gA", "gB"):
        assert torch.equal(got[k], ref[k]), k


def test_uniform_type_many_pairs_takes_the_per_pair_finalize(exact):
    """B = 9: one finalize workgroup per pair and the mean kernel (B <= 8 is the single-launch finalize)."""
    H, W, B, D = 16, 20, 9, 3
    g = torch.Generator().manual_seed(4)
    pairs = [make_lists(WITHIN, H * W, (5 + 37 * b, 3 + 11 * b, 2 + 29 * (B - b), 7), g) for b in range(B)]
    A, Bt = descriptors(B, H * W, D, 6)
    pcl = pcl_for(H, W)
    ref = run_batched(pcl, WITHIN, A, Bt, pairs)
    got = run_mixed(pcl, A, Bt, device_lists(pairs, [WITHIN] * B))
    for k in ("loss", "terms", "hard", "gA", "gB"):
        assert torch.equal(got[k], ref[k]), k
    types = [WITHIN, -1] * 4 + [WITHIN]
    skipped = run_mixed(pcl, A, Bt, device_lists(pairs, types))
    assert skipped["num_valid"] == 5 and skipped["status"] == 0
    assert torch.equal(skipped["terms"][0::2], ref["terms"][0::2]) and not skipped["terms"][1::2].any()
    want = np.float32(sum(float(ref["terms"][p, 0]) for p in range(0, B, 2)) / 5.0)
    assert float(skipped["loss"]) == float(want)


# ------------------------------------------------------------------------------------------------ 2. mixed types
def _ulp_close(a, b):
    a, b = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
    return bool(np.all(np.abs(a - b) <= np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)))


@pytest.mark.parametrize("D", [3, 16])
def test_mixed_types_compose_each_pair_by_its_own_type(D, exact):
    from oracle import loss_oracle, synth
    H, W = 24, 32
    types = [WITHIN, DIFFERENT, ACROSS, MULTI]
    g = torch.Generator().manual_seed(23)
    pairs = [make_lists(t, H * W, s, g) for t, s in zip(types, SIZES + [(300, 600, 900, 40)])]
    A, Bt = descriptors(4, H * W, D, 9)
    pcl = pcl_for(H, W)
    got = run_mixed(pcl, A, Bt, device_lists(pairs, types))
    assert got["status"] == 0 and got["num_valid"] == 4
    opcl = loss_oracle.PixelwiseContrastiveLoss([H, W], synth.LOSS_CONFIG)
    e = torch.tensor([-1])
    total = 0.0
    for p, t in enumerate(types):
        one = run_batched(pcl, t, A[p:p + 1], Bt[p:p + 1], [pairs[p]])
        assert torch.equal(got["terms"][p], one["terms"][0]) and torch.equal(got["hard"][p], one["hard"][0]), p
        total += float(one["terms"][0, 0])
        # the single-pair gradient x 1/4 (another product order: 1 ulp)
        assert _ulp_close(got["gA"][p], one["gA"][0] * 0.25) and _ulp_close(got["gB"][p], one["gB"][0] * 0.25), p
        A2 = A[p:p + 1].detach().clone().requires_grad_(True)
        B2 = Bt[p:p + 1].detach().clone().requires_grad_(True)
        out = loss_oracle.get_loss(opcl, torch.tensor([t]), A2, B2, *[e if x is None else x for x in pairs[p]])
        np.testing.assert_allclose(got["terms"][p].numpy(), [float(o.detach().sum()) for o in out], rtol=1e-5, atol=1e-9)
        (out[0] / 4).backward()
        assert rel_err(got["gA"][p], A2.grad[0]) < 1e-5 and rel_err(got["gB"][p], B2.grad[0]) < 1e-5, p
    assert float(got["loss"]) == float(np.float32(total / 4.0))      # fp64 mean in pair order, rounded once


def test_synthetic_multi_object_composes_as_within_scene_on_complete_samples_lists():
    """Type 4 through the table, with the lists samples.complete_samples builds (SYNTHETIC_MULTI_OBJECT is its default type)."""
    from dcn_hip import samples
    h, w, n = 20, 24, 2
    g = torch.Generator().manual_seed(2)
    mask = torch.zeros((n, h, w), dtype=torch.uint8)
    mask[:, 4:16, 5:20] = 1
    cnt = [40, 25]
    ua = torch.randint(5, 20, (sum(cnt),), generator=g)
    va = torch.randint(4, 16, (sum(cnt),), generator=g)
    ub = torch.randint(0, w, (sum(cnt),), generator=g)
    vb = torch.randint(0, h, (sum(cnt),), generator=g)
    sb = samples.complete_samples((ua, va), (ub, vb), [0, cnt[0], sum(cnt)], mask, mask, num_masked_non_matches_per_match=3,
                                  num_background_non_matches_per_match=2, use_image_b_mask_inv=True, generator=g)
    assert sb.type.tolist() == [SYNTHETIC, SYNTHETIC] and int(sb.status) == 0
    assert sb.max_list_len == max(65 * 3, h * w) and sb.max_pair_len == 65 * 6 + h * w
    A, Bt = descriptors(n, h * w, 3, 3)
    pcl = pcl_for(h, w)
    got = run_mixed(pcl, A, Bt, sb.device_lists())
    ref = run_batched(pcl, SYNTHETIC, A, Bt, sb.pair_lists())
    assert got["status"] == 0 and got["num_valid"] == 2 and float(ref["loss"]) > 0
    assert torch.equal(got["loss"], ref["loss"]) and torch.equal(got["terms"], ref["terms"])


# (golden, data type the mixed table composes it with): the reference's own vectors, which share one loss configuration,
# image size and descriptor width, as one batch of mixed types
GOLDEN_BATCH = [("within_d3", WITHIN), ("different_object", DIFFERENT), ("multi_object", MULTI), ("within_blind", WITHIN)]


def test_reference_goldens_through_one_mixed_batch():
    from dcn_hip import loss as K
    zs = [load_golden_loss(os.path.join(GOLDEN_DIR, "loss_ref_%s.npz" % name)) for name, _ in GOLDEN_BATCH]
    cfg = zs[0][1]
    assert all(c == cfg for _, c in zs) and all(int(z["match_type"]) == t for (z, _), (_, t) in zip(zs, GOLDEN_BATCH))
    H, W = int(zs[0][0]["H"]), int(zs[0][0]["W"])
    A = torch.cat([torch.tensor(z["A"]) for z, _ in zs])
    B = torch.cat([torch.tensor(z["B"]) for z, _ in zs])
    pairs = [lists_from_golden(z) for z, _ in zs]                   # (host `[-1]` sentinels: stripped by from_lists)
    got = run_mixed(pcl_for(H, W, cfg), A, B, device_lists(pairs, [t for _, t in GOLDEN_BATCH]))
    assert got["status"] == 0 and got["num_valid"] == 4
    for p, (z, _) in enumerate(zs):
        np.testing.assert_allclose(got["terms"][p].numpy(), z["out"], rtol=2e-6, atol=1e-9)   # test_emu_loss.py's tolerance
        assert rel_err(got["gA"][p] * 4, z["gradA"][0]) < 1e-5 and rel_err(got["gB"][p] * 4, z["gradB"][0]) < 1e-5
    assert K.NUM_TYPES == 5


# ------------------------------------------------------------------------------------------------ 3. empty pairs
def test_empty_pair_is_left_out_of_the_mean(exact):
    H, W, D = 24, 32, 3
    g = torch.Generator().manual_seed(31)
    pairs = [make_lists(WITHIN, H * W, s, g) for s in SIZES]        # the middle pair: in-range garbage between its offsets
    A, Bt = descriptors(3, H * W, D, 12)
    pcl = pcl_for(H, W)
    got = run_mixed(pcl, A, Bt, device_lists(pairs, [WITHIN, -1, WITHIN]))
    two = run_mixed(pcl, A[[0, 2]], Bt[[0, 2]], device_lists([pairs[0], pairs[2]], [WITHIN, WITHIN]))
    assert got["num_valid"] == 2 and got["status"] == 0 and two["num_valid"] == 2
    assert torch.equal(got["loss"], two["loss"]) and torch.equal(got["terms"][[0, 2]], two["terms"])
    assert torch.equal(got["gA"][[0, 2]], two["gA"]) and torch.equal(got["gB"][[0, 2]], two["gB"])
    assert not got["terms"][1].any() and not got["hard"][1].any()
    assert not got["gA"][1].any() and not got["gB"][1].any()
    assert float(got["loss"]) > 0 and got["gA"][0].abs().max() > 0


@pytest.mark.parametrize("use_exact", [True, False], ids=["exact", "atomics"])
def test_all_pairs_empty(use_exact, monkeypatch):
    from dcn_hip import loss as K
    monkeypatch.setattr(K, "EXACT_BACKWARD", use_exact)
    H, W = 12, 16
    g = torch.Generator().manual_seed(1)
    pairs = [make_lists(WITHIN, H * W, (9, 18, 9, 4), g) for _ in range(2)]
    A, Bt = descriptors(2, H * W, 3, 2)
    got = run_mixed(pcl_for(H, W), A, Bt, device_lists(pairs, [-1, -1]))
    assert got["num_valid"] == 0 and got["status"] == 0
    assert float(got["loss"]) == 0.0 and not got["terms"].any() and not got["gA"].any() and not got["gB"].any()
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("loss", "terms", "gA", "gB"))


# ------------------------------------------------------------------------------------------------ 4. status bits
def _status_case():
    H, W = 12, 16
    g = torch.Generator().manual_seed(8)
    pairs = [make_lists(WITHIN, H * W, (10, 20, 30, 6), g), make_lists(WITHIN, H * W, (8, 16, 24, 5), g)]
    A, Bt = descriptors(2, H * W, 3, 4)
    return H, W, pairs, A, Bt


def _first_pair_alone(pcl, A, Bt, pairs):
    return run_mixed(pcl, A[:1], Bt[:1], device_lists(pairs[:1], [WITHIN]))


def test_status_index_out_of_range():
    from dcn_hip import loss as K
    H, W, pairs, A, Bt = _status_case()
    bad = list(pairs[1])
    bad[3] = bad[3].clone()
    bad[3][2] = H * W
    got = run_mixed(pcl_for(H, W), A, Bt, device_lists([pairs[0], tuple(bad)], [WITHIN, WITHIN]))
    assert got["status"] == K.BAD_INDEX and got["num_valid"] == 2


def test_status_unknown_type_skips_the_pair():
    from dcn_hip import loss as K
    H, W, pairs, A, Bt = _status_case()
    pcl = pcl_for(H, W)
    got = run_mixed(pcl, A, Bt, device_lists(pairs, [WITHIN, 7]))
    assert got["status"] == K.BAD_TYPE and got["num_valid"] == 1
    assert torch.equal(got["terms"][0], _first_pair_alone(pcl, A, Bt, pairs)["terms"][0])
    assert not got["terms"][1].any() and not got["gA"][1].any()


def test_status_list_longer_than_the_bound_skips_the_pair():
    from dcn_hip import loss as K
    H, W, pairs, A, Bt = _status_case()
    pcl = pcl_for(H, W)
    got = run_mixed(pcl, A, Bt, device_lists(pairs[::-1], [WITHIN, WITHIN], max_list_len=24))   # pair 1 now has a list of 30
    assert got["status"] == K.BAD_BOUNDS and got["num_valid"] == 1
    assert not got["terms"][1].any() and not got["gA"][1].any() and not got["gB"][1].any()
    alone = run_mixed(pcl, A[:1], Bt[:1], device_lists(pairs[1:], [WITHIN]))
    assert torch.equal(got["terms"][0], alone["terms"][0]) and torch.equal(got["loss"], alone["loss"])
    # the per-pair bound
    got = run_mixed(pcl, A, Bt, device_lists(pairs, [WITHIN, WITHIN], max_pair_len=60))          # 66 and 53 entries
    assert got["status"] == K.BAD_BOUNDS and got["num_valid"] == 1 and not got["terms"][0].any()


def test_status_total_beyond_the_capacity_skips_the_pair():
    """offsets[4B] > capacity, with valid memory behind the capacity: the lists are a view of a longer tensor."""
    from dcn_hip import loss as K
    H, W, pairs, A, Bt = _status_case()
    pcl = pcl_for(H, W)
    full = device_lists(pairs, [WITHIN, WITHIN], tail=64)
    total = int(full.offsets[-1])
    short = K.DeviceLists(full.idx_a[:total - 3], full.idx_b[:total - 3], full.offsets, full.types, 1000, 1000)
    assert short.capacity == total - 3
    got = run_mixed(pcl, A, Bt, short)
    assert got["status"] == K.BAD_BOUNDS and got["num_valid"] == 1
    assert torch.equal(got["terms"][0], _first_pair_alone(pcl, A, Bt, pairs)["terms"][0])
    assert not got["terms"][1].any() and not got["gA"][1].any() and not got["gB"][1].any()


def test_status_pixel_weight_layout_and_debug_raises():
    from dcn_hip import loss as K
    from oracle import synth
    H, W, pairs, A, Bt = _status_case()
    cfg = dict(synth.LOSS_CONFIG, use_l2_pixel_loss_on_masked_non_matches=True)
    pcl = pcl_for(H, W, cfg)
    assert run_mixed(pcl, A, Bt, device_lists(pairs, [WITHIN, WITHIN]))["status"] == 0      # 20 = 2 x 10, 16 = 2 x 8
    odd = list(pairs[1])
    odd[2], odd[3] = odd[2][:15], odd[3][:15]                                                # 15 masked for 8 matches
    lists = device_lists([pairs[0], tuple(odd)], [WITHIN, WITHIN])
    got = run_mixed(pcl, A, Bt, lists)
    assert got["status"] == K.BAD_PIXEL_LAYOUT and got["num_valid"] == 2
    # a different-object pair in the same batch does not use the weights: no flag for its lists
    assert run_mixed(pcl, A, Bt, device_lists([pairs[0], tuple(odd)], [WITHIN, DIFFERENT]))["status"] == 0
    pcl.debug = True
    with pytest.raises(RuntimeError, match="whole number"):
        run_mixed(pcl, A, Bt, lists)


def test_argument_checks():
    from dcn_hip import loss as K
    H, W, pairs, A, Bt = _status_case()
    lists = device_lists(pairs, [WITHIN, WITHIN])
    pcl = pcl_for(H, W)
    with pytest.raises(ValueError):
        run_mixed(pcl, A[:1], Bt[:1], lists)
    with pytest.raises(TypeError):
        run_mixed(pcl, A.double(), Bt.double(), lists)
    with pytest.raises(TypeError):
        K.DeviceLists(lists.idx_a, lists.idx_b, lists.offsets, lists.types.long(), 10, 10)
    with pytest.raises(ValueError):
        K.config_table([K.make_config([0, .5, .5, .5], W)] * 4)


# ------------------------------------------------------------------------------------------------ 5. joining sample batches
def _planar_frames(n, h, w, seed):
    rgb = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    depth = torch.full((n, h, w), 900, dtype=torch.int16)          # a wall at 0.9 m, cameras translated in its plane
    mask = torch.zeros((n, h, w), dtype=torch.uint8)
    mask[:, 4:20, 6:26] = 1
    return rgb, depth, mask


def _two_groups(h=24, w=32):
    from dcn_hip import samples
    rgb, depth, mask = _planar_frames(2, h, w, 3)
    pose_a = np.stack([np.eye(4)] * 2)
    pose_b = np.stack([np.eye(4)] * 2)
    pose_b[0, 0, 3], pose_b[1, 1, 3] = 0.005, 0.004
    g = torch.Generator().manual_seed(5)
    within = samples.build_within_scene_samples(depth, depth, mask, mask, pose_a, pose_b, None, rgb, rgb,
                                                num_matching_attempts=200, sample_matches_only_off_mask=True,
                                                num_masked_non_matches_per_match=2, num_background_non_matches_per_match=3,
                                                use_image_b_mask_inv=True, generator=g)
    across = samples.build_across_scene_samples(mask[:1], mask[1:], rgb[:1], rgb[1:], num_samples=150, generator=g,
                                                data_type=samples.SINGLE_OBJECT_ACROSS_SCENE)
    return within, across


def test_concat_sample_batches_keeps_every_list():
    from dcn_hip import samples
    within, across = _two_groups()
    assert within.type.tolist() == [WITHIN, WITHIN] and across.type.tolist() == [ACROSS]
    assert within.max_list_len == max(200 * 3, 24 * 32) and within.max_pair_len == 200 * 6 + 24 * 32
    assert across.max_list_len == 150 and across.max_pair_len == 150
    joined = samples.concat_sample_batches([within, across])
    off = joined.offsets.tolist()
    assert len(off) == 13 and off[0] == 0 and all(b >= a for a, b in zip(off, off[1:]))
    assert joined.idx_a.numel() == within.idx_a.numel() + across.idx_a.numel()
    assert bool((joined.idx_a[off[-1]:] == -1).all()) and bool((joined.idx_b[off[-1]:] == -1).all())
    p = 0
    for sb in (within, across):
        so = sb.offsets.tolist()
        for q in range(int(sb.type.numel())):
            for t in range(4):
                for mine, theirs in ((joined.idx_a, sb.idx_a), (joined.idx_b, sb.idx_b)):
                    assert torch.equal(mine[off[4 * p + t]:off[4 * p + t + 1]], theirs[so[4 * q + t]:so[4 * q + t + 1]]), (p, t)
            p += 1
    assert off[4] - off[0] > 100 and off[12] - off[11] == 150
    assert joined.type.tolist() == [WITHIN, WITHIN, ACROSS] and joined.empty.tolist() == [False] * 3
    assert int(joined.status) == 0
    assert torch.equal(joined.seeds, torch.cat([within.seeds, across.seeds]))
    assert torch.equal(joined.aug_params[:3], torch.cat([within.aug_params[:2], across.aug_params[:1]]))
    assert torch.equal(joined.aug_params[3:], torch.cat([within.aug_params[2:], across.aug_params[1:]]))
    assert torch.equal(joined.input_a, torch.cat([within.input_a, across.input_a]))
    assert torch.equal(joined.mask_b, torch.cat([within.mask_b, across.mask_b]))
    assert joined.max_list_len == within.max_list_len and joined.max_pair_len == within.max_pair_len
    # a batch whose status word is raised, and one whose offsets are not the builders' layout
    flagged = within._replace(status=torch.tensor([samples.BAD_DRAWS], dtype=torch.int32))
    assert int(samples.concat_sample_batches([flagged, across]).status) == samples.BAD_DRAWS
    broken = across._replace(offsets=torch.tensor([0, 0, 0, 0, 151]))
    j = samples.concat_sample_batches([within, broken])
    assert int(j.status) == samples.BAD_OFFSETS and j.offsets.tolist()[8:] == [off[8]] * 5


def test_loss_on_the_joined_batch_is_the_weighted_combination(exact):
    from dcn_hip import samples
    within, across = _two_groups()
    joined = samples.concat_sample_batches([within, across])
    h, w = 24, 32
    A, Bt = descriptors(3, h * w, 3, 21)
    pcl = pcl_for(h, w)
    got = run_mixed(pcl, A, Bt, joined.device_lists())
    g1 = run_mixed(pcl, A[:2], Bt[:2], within.device_lists())
    g2 = run_mixed(pcl, A[2:], Bt[2:], across.device_lists())
    assert got["status"] == 0 and got["num_valid"] == 3 and float(g1["loss"]) > 0 and float(g2["loss"]) > 0
    assert torch.equal(got["terms"], torch.cat([g1["terms"], g2["terms"]]))
    assert torch.equal(got["hard"], torch.cat([g1["hard"], g2["hard"]]))
    want = (2.0 * float(g1["loss"]) + 1.0 * float(g2["loss"])) / 3.0
    assert abs(float(got["loss"]) - want) <= 1e-6 * abs(want)
    assert rel_err(got["gA"][:2] * 3, g1["gA"] * 2) < 1e-6 and rel_err(got["gA"][2:] * 3, g2["gA"]) < 1e-6
    # ... and equals the parent's path on each group
    ref = run_batched(pcl, WITHIN, A[:2], Bt[:2], within.pair_lists())
    assert torch.equal(g1["loss"], ref["loss"]) and torch.equal(g1["gA"], ref["gA"])


# ------------------------------------------------------------------------------------------------ 6. one type per pair
TRAINING = {"training": {"num_matching_attempts": 60, "sample_matches_only_off_mask": True, "num_non_matches_per_match": 4,
                         "fraction_masked_non_matches": 0.5, "fraction_background_non_matches": 0.5,
                         "cross_scene_num_samples": 40, "use_image_b_mask_inv": True, "domain_randomize": False,
                         "data_type_probabilities": {"SINGLE_OBJECT_WITHIN_SCENE": 2.0, "SINGLE_OBJECT_ACROSS_SCENE": 1.0,
                                                     "DIFFERENT_OBJECT": 1.0, "MULTI_OBJECT": 0.0,
                                                     "SYNTHETIC_MULTI_OBJECT": 0.0}}}


def _store():
    return fc.store_from_golden(np.load(fc.GOLDENS[0]), "cpu", h=12, w=16)


def test_draw_training_batch_with_one_type_per_pair():
    from dcn_hip import frames
    store = _store()
    B = 6
    types, ps = frames.data_type_distribution(TRAINING)
    assert types == [0, 1, 2]
    seen = set()
    for seed in range(4):
        rng = np.random.RandomState(seed)
        want = [types[int(rng.choice(len(types), p=ps))] for _ in range(B)]
        sb, drawn, fbs = frames.draw_training_batch(store, B, TRAINING, generator=torch.Generator().manual_seed(seed),
                                                    host_rng=np.random.RandomState(seed), per_pair_types=True)
        assert list(drawn) == want
        seen.update(want)
        order = sorted(want)                                      # groups in ascending type order
        assert [fb.data_type for fb in fbs] == sorted(set(want))
        assert [int(fb.frames.shape[0]) for fb in fbs] == [order.count(t) for t in sorted(set(want))]
        dev = sb.type.tolist()
        assert len(dev) == B and all(d in (t, -1) for d, t in zip(dev, order))
        assert sb.empty.tolist() == [d == -1 for d in dev]
        off = sb.offsets.tolist()
        assert len(off) == 4 * B + 1 and all(b >= a for a, b in zip(off, off[1:])) and off[-1] <= sb.idx_a.numel()
        for p, d in enumerate(dev):
            if d in (ACROSS, DIFFERENT):
                assert off[4 * p + 3] - off[4 * p] == 0 and off[4 * p + 4] - off[4 * p + 3] == 40
            if d == -1:
                assert off[4 * p + 4] == off[4 * p]
        assert tuple(sb.input_a.shape) == (B, 3, 12, 16) and tuple(sb.aug_params.shape) == (2 * B, 16)
        lists = sb.device_lists()
        assert lists.num_pairs == B and lists.max_list_len <= lists.capacity
    assert seen == {0, 1, 2}


def test_draw_training_batch_default_is_unchanged():
    """per_pair_types=False: the type drawn once, then select_frames and the type's builder with the same generator -- the
    calls the function has always made, restated here."""
    from dcn_hip import frames, samples
    store = _store()
    o = samples.options_from_config(TRAINING)
    types, ps = frames.data_type_distribution(TRAINING)
    for seed in range(5):
        sb, dt, fb = frames.draw_training_batch(store, 3, TRAINING, generator=torch.Generator().manual_seed(seed),
                                                host_rng=np.random.RandomState(seed))
        assert isinstance(dt, int) and dt == types[int(np.random.RandomState(seed).choice(len(types), p=ps))]
        g = torch.Generator().manual_seed(seed)
        fb2 = frames.select_frames(store, 3, dt, generator=g)
        if dt == WITHIN:
            ref = samples.build_within_scene_samples(
                fb2.depth[0], fb2.depth[1], fb2.mask[0], fb2.mask[1], None, None, None, fb2.rgb[0], fb2.rgb[1],
                num_matching_attempts=o.num_matching_attempts, sample_matches_only_off_mask=o.sample_matches_only_off_mask,
                num_masked_non_matches_per_match=o.num_masked_non_matches_per_match,
                num_background_non_matches_per_match=o.num_background_non_matches_per_match,
                use_image_b_mask_inv=o.use_image_b_mask_inv, domain_randomize=o.domain_randomize, generator=g, data_type=dt,
                cameras=fb2.cams[0])
        else:
            ref = samples.build_across_scene_samples(fb2.mask[0], fb2.mask[1], fb2.rgb[0], fb2.rgb[1],
                                                     num_samples=o.cross_scene_num_samples, domain_randomize=o.domain_randomize,
                                                     generator=g, data_type=dt)
        assert torch.equal(fb.frames, fb2.frames)
        for k in ("input_a", "input_b", "idx_a", "idx_b", "offsets", "empty", "type", "status", "seeds", "aug_params"):
            assert torch.equal(getattr(sb, k), getattr(ref, k)), k
        assert sb[:12] == sb[:12] and len(sb) == 14 and sb._fields[:12] == (
            "input_a", "input_b", "idx_a", "idx_b", "offsets", "empty", "type", "status", "seeds", "aug_params", "mask_a", "mask_b")


# ------------------------------------------------------------------------------------------------ 7. every arm at every site
# (rtol / atol of the terms and the gradient bound: test_mixed_types_compose_each_pair_by_its_own_type's, against the same oracle)
@pytest.mark.parametrize("site,D", mc.ONE_TYPE_CASES)
def test_one_type_launch_sites_at_the_remaining_descriptor_widths(site, D):
    mc.check_one_type_dispatch(site, D, "cpu", rtol=1e-5, atol=1e-9, grad_tol=1e-5)


@pytest.mark.parametrize("site,D", mc.MIXED_CASES)
def test_mixed_launch_sites_at_the_remaining_descriptor_widths(site, D):
    mc.check_mixed_dispatch(site, D, "cpu", rtol=1e-5, atol=1e-9, grad_tol=1e-5)


# ------------------------------------------------------------------------------------------------ 8. refusal codes
OK, E_INVALID, E_UNSUPPORTED = 0, -1, -3                  # include/dcn_hip.h


class _Refusals(object):
    """Valid arguments of the six contrastive entry points at P = 1, HW = 16, D = 3 (or ``P`` pairs with empty lists), as
    name -> value in the order of the C signature; ``call(entry, name=value, ...)`` replaces some and returns the code."""

    def __init__(self, P=1, offsets=(0, 5, 9, 12, 14)):
        from dcn_hip import _lib as L
        from dcn_hip import loss as K
        self.L, self.lib = L, L.get()
        HW, D = 16, 3
        off = list(offsets) if P == 1 else [0] * (4 * P + 1)
        total = off[-1]
        self.keep = k = dict(
            desc=torch.zeros(2, P, HW, D), idx=torch.zeros(2, max(total, 1), dtype=torch.int64),
            off_dev=torch.tensor(off, dtype=torch.int64), types=torch.zeros(P, dtype=torch.int32),
            terms=torch.zeros(P, 5), sums=torch.zeros(P, 4), hard=torch.zeros(P, 4, dtype=torch.int32), loss=torch.zeros(1),
            status=torch.zeros(1, dtype=torch.int32), num_valid=torch.ones(1, dtype=torch.int32), gl=torch.ones(1),
            ws=torch.zeros(int(self.lib.dcn_loss_workspace_bytes(P, 5)), dtype=torch.uint8),
            records=torch.zeros(max(total, 1) * (D + 1)), grads=torch.ones(2, P, HW, D),
            xws=torch.full((int(self.lib.dcn_loss_exact_workspace_bytes(P, HW, D)),), 255, dtype=torch.uint8))
        self.off_c = (ctypes.c_int64 * len(off))(*off)
        self.cfg = K.make_config([0, .5, .5, .5], 4)
        self.table = K.config_table([self.cfg] * K.NUM_TYPES)
        p = L.ptr
        lists = [("idx_a", p(k["idx"][0])), ("idx_b", p(k["idx"][1]))]
        host = lists + [("offsets_host", ctypes.cast(self.off_c, ctypes.c_void_p)), ("offsets_dev", p(k["off_dev"])),
                        ("cfg", ctypes.byref(self.cfg))]
        mixed = lists + [("offsets_dev", p(k["off_dev"])), ("types_dev", p(k["types"])), ("cfgs", self.table),
                         ("max_list_len", 5), ("max_pair_len", 14), ("capacity", total)]
        shape = [("num_pairs", P), ("hw", HW), ("d", D)]
        descs = [("desc_a", p(k["desc"][0])), ("desc_b", p(k["desc"][1]))]
        outs = [("terms", p(k["terms"])), ("sums", p(k["sums"])), ("hard_neg", p(k["hard"])), ("loss", p(k["loss"]))]
        grads = [("grad_a", p(k["grads"][0])), ("grad_b", p(k["grads"][1])), ("stream", None)]
        back = [("hard_neg", p(k["hard"])), ("grad_loss", p(k["gl"])), ("pair_records", p(k["records"]))]
        mback = [("hard_neg", p(k["hard"])), ("num_valid", p(k["num_valid"])), ("grad_loss", p(k["gl"])),
                 ("pair_records", p(k["records"]))]
        fwd = descs + shape + host + outs + [("per_term", None), ("status", p(k["status"])), ("workspace", p(k["ws"]))]
        self.args = {
            "forward": fwd + [("stream", None)],
            "forward_save": fwd + [("pair_records", p(k["records"])), ("stream", None)],
            "backward": descs + shape + host + [("sums", p(k["sums"])), ("hard_neg", p(k["hard"])), ("grad_loss", p(k["gl"])),
                                                ("pair_grad", None)] + grads,
            "backward_saved": shape + host + back + [("prefilled", 0)] + grads,
            "backward_saved_exact": shape + host + back + [("workspace", p(k["xws"]))] + grads,
            "mixed_forward": descs + shape + mixed + outs + [("num_valid", p(k["num_valid"])), ("status", p(k["status"])),
                                                             ("workspace", p(k["ws"])), ("pair_records", p(k["records"])),
                                                             ("stream", None)],
            "mixed_backward_saved": shape + mixed + mback + [("prefilled", 0)] + grads,
            "mixed_backward_saved_exact": shape + mixed + mback + [("workspace", p(k["xws"]))] + grads,
        }

    def call(self, entry, **replace):
        names = [n for n, _ in self.args[entry]]
        assert set(replace) <= set(names), (entry, sorted(set(replace) - set(names)))
        fn = getattr(self.lib, "dcn_contrastive_loss_" + entry)
        assert len(names) == len(self.L.SYMBOLS["dcn_contrastive_loss_" + entry][1])
        return fn(*[replace.get(n, v) for n, v in self.args[entry]])


REQUIRED = {   # the pointers each entry point refuses as null whatever the lists hold
    "forward": ["desc_a", "desc_b", "offsets_host", "offsets_dev", "cfg", "terms", "sums", "hard_neg", "loss", "status", "workspace"],
    "forward_save": ["pair_records", "offsets_host", "desc_a", "workspace"],
    "backward": ["desc_a", "desc_b", "offsets_host", "offsets_dev", "cfg", "grad_a", "grad_b", "hard_neg", "grad_loss"],
    "backward_saved": ["offsets_host", "offsets_dev", "cfg", "hard_neg", "grad_loss", "pair_records", "grad_a", "grad_b"],
    "backward_saved_exact": ["offsets_host", "offsets_dev", "cfg", "hard_neg", "grad_loss", "pair_records", "workspace", "grad_a",
                             "grad_b"],
    "mixed_forward": ["offsets_dev", "types_dev", "cfgs", "idx_a", "idx_b", "desc_a", "desc_b", "terms", "sums", "hard_neg",
                      "loss", "num_valid", "status", "workspace"],
    "mixed_backward_saved": ["offsets_dev", "types_dev", "cfgs", "idx_a", "idx_b", "hard_neg", "num_valid", "grad_loss", "grad_a",
                             "grad_b"],
    "mixed_backward_saved_exact": ["offsets_dev", "types_dev", "cfgs", "idx_a", "idx_b", "hard_neg", "num_valid", "grad_loss",
                                   "workspace", "grad_a", "grad_b"],
}


@pytest.mark.parametrize("entry", sorted(REQUIRED))
def test_refusal_null_pointer_or_no_pairs(entry):
    r = _Refusals()
    for name in REQUIRED[entry]:
        assert r.call(entry, **{name: None}) == E_INVALID, name
    for bad in (dict(num_pairs=0), dict(hw=0), dict(d=0)):
        assert r.call(entry, **bad) == E_INVALID, bad
    if entry.startswith("mixed"):
        for bad in (dict(max_list_len=-1), dict(max_pair_len=-1), dict(capacity=-1)):
            assert r.call(entry, **bad) == E_INVALID, bad
    assert not r.keep["terms"].any() and bool((r.keep["grads"] == 1).all()) and bool((r.keep["xws"] == 255).all())   # nothing ran


def test_refusal_offsets_and_lists_of_the_forward():
    r = _Refusals()
    down = (ctypes.c_int64 * 5)(0, 5, 4, 12, 14)
    for entry in ("forward", "forward_save"):
        assert r.call(entry, offsets_host=ctypes.cast(down, ctypes.c_void_p)) == E_INVALID
        assert r.call(entry, idx_a=None) == E_INVALID and r.call(entry, idx_b=None) == E_INVALID    # 14 entries, no lists
    e = _Refusals(offsets=(0, 0, 0, 0, 0))
    assert e.call("forward", idx_a=None, idx_b=None) == OK                                           # nothing to read


def test_refusal_too_many_pairs_is_unsupported_after_invalid():
    P = 16384                                                     # grid.y = 4 P of the launches: past 65535
    r = _Refusals(P=P)
    for entry in ("backward_saved_exact", "mixed_forward", "mixed_backward_saved", "mixed_backward_saved_exact"):
        assert r.call(entry) == E_UNSUPPORTED, entry
    # DCN_E_INVALID first on the one-type entry; on the mixed ones mixed_args (with the pair count) before the entry's own
    # null checks
    assert r.call("backward_saved_exact", workspace=None) == E_INVALID
    assert r.call("backward_saved_exact", num_pairs=0) == E_INVALID
    assert r.call("mixed_forward", terms=None) == E_UNSUPPORTED
    assert r.call("mixed_backward_saved", grad_a=None) == E_UNSUPPORTED
    assert r.call("mixed_backward_saved_exact", workspace=None) == E_UNSUPPORTED
    assert r.call("mixed_forward", types_dev=None) == E_INVALID
    assert bool((r.keep["grads"] == 1).all())


def test_refusal_pair_of_two_to_the_22_entries():
    """The one-type entry reads the host offsets, the mixed one the host bound (clipped to the capacity): both return before
    anything on the device is read, so the lists themselves need not exist."""
    big = 1 << 22
    r = _Refusals()
    claimed = (ctypes.c_int64 * 5)(0, big, big, big, big)
    assert r.call("backward_saved_exact", offsets_host=ctypes.cast(claimed, ctypes.c_void_p)) == E_UNSUPPORTED
    assert r.call("backward_saved_exact", offsets_host=ctypes.cast(claimed, ctypes.c_void_p), grad_b=None) == E_INVALID
    assert r.call("mixed_backward_saved_exact", max_pair_len=big, capacity=big) == E_UNSUPPORTED
    assert r.call("mixed_backward_saved_exact", max_pair_len=big, capacity=big, workspace=None) == E_INVALID
    assert bool((r.keep["xws"] == 255).all()) and bool((r.keep["grads"] == 1).all())


def test_refusal_null_lists_or_records_after_the_fill():
    """Non-empty lists without idx_a / idx_b (one-type) or without pair_records (mixed): DCN_E_INVALID, after the gradient maps
    / the workspace have been zero-filled; with empty lists the same calls return DCN_OK after the fill."""
    for entry, missing in (("backward_saved", dict(idx_a=None)), ("backward_saved", dict(idx_b=None)),
                           ("mixed_backward_saved", dict(pair_records=None))):
        r = _Refusals()
        assert r.call(entry, **missing) == E_INVALID, (entry, missing)
        assert not r.keep["grads"].any()
        r = _Refusals()
        assert r.call(entry, prefilled=1, **missing) == E_INVALID
        assert bool((r.keep["grads"] == 1).all())                 # (prefilled: the caller's fill is kept)
    for entry, missing in (("backward_saved_exact", dict(idx_a=None)), ("mixed_backward_saved_exact", dict(pair_records=None))):
        r = _Refusals()
        assert r.call(entry, **missing) == E_INVALID, (entry, missing)
        assert not r.keep["xws"].any() and bool((r.keep["grads"] == 1).all())
    e = _Refusals(offsets=(0, 0, 0, 0, 0))
    assert e.call("backward_saved", idx_a=None, idx_b=None) == OK and not e.keep["grads"].any()
    e = _Refusals()
    assert e.call("mixed_backward_saved", max_list_len=0, pair_records=None) == OK and not e.keep["grads"].any()
    assert _Refusals().call("backward_saved", pair_records=None) == E_INVALID                          # required, lists or not
