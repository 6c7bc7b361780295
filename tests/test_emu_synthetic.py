"""SYNTHETIC_MULTI_OBJECT samples on the device (csrc/synthetic_kernels.hip, samples.build_synthetic_multi_object_samples,
frames.draw_training_batch(..., synthetic_multi_object=True)) through the host-emulation build: the reference's own
get_synthetic_multi_object_within_scene_data replayed, the fused chain against the composition of the existing entry points,
seeded mode against the numpy restatement, replay and argument errors, and the training batch."""
import ctypes

import numpy as np
import pytest
import torch

import frames_common as fc
import samples_common as sc
import synthetic_common as yc
from helpers import use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


@pytest.mark.parametrize("path", yc.GOLDENS, ids=yc.GOLDEN_IDS)
def test_golden_replays_bit_exactly(path):
    z = np.load(path)
    yc.check_golden(yc.replay_golden(z, "cpu"), z)


def test_golden_set_is_complete():
    for need in yc.REQUIRED_GOLDENS:
        assert need in yc.GOLDEN_IDS, need
    fgs = {tuple(np.load(p)["foreground"].tolist()) for p in yc.GOLDENS if int(np.load(p)["type"]) == 4}
    assert fgs == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("h,w", yc.SHAPES, ids=["%dx%d" % s for s in yc.SHAPES])
@pytest.mark.parametrize("only_off,inv", [(True, True), (False, False)])
def test_replay_equals_composition_of_existing_entries(h, w, only_off, inv):
    n, A, k1, k2 = 5, 60, 2, 3
    ex = yc.example_batch(n, h, w, seed=h * 100 + w)
    draws = yc.example_draws(n, A, k1, k2, seed=h + w)
    sb, fg = yc.run_fused(ex, "cpu", A, only_off, k1, k2, inv, draws=yc.fused_draws(ex, draws, only_off))
    merged, done = yc.run_composition(ex, "cpu", A, only_off, k1, k2, inv, draws)
    yc.check_equals_composition(sb, merged, done)
    sc.check_layout(sb)                                                          # (status 0: no stream was too short)
    assert torch.equal(fg, torch.from_numpy(ex["fg"])) and sb.aug_params is None and sb.seeds is None
    assert sb.max_list_len == 2 * A * max(k1, k2) and sb.max_pair_len == 2 * A * (1 + k1 + k2)
    assert sb.idx_a.numel() == n * sb.max_pair_len
    assert bool(sb.empty[3])                                                     # marked empty on input
    if only_off:
        assert bool(sb.empty[1])                                                 # empty mask a1
    if (h, w) == (24, 36):
        assert sb.empty.tolist() == [False, only_off, True, True, False]         # 2: b fully occluded in frame 2 only
        # ... and only there: without frame 2's rule sample 2 keeps entries of both objects
        ex2 = dict(ex, fg=ex["fg"].copy())
        ex2["fg"][2] = [yc.FG_B, yc.FG_B]
        sb2, _ = yc.run_fused(ex2, "cpu", A, only_off, k1, k2, inv, draws=yc.fused_draws(ex2, draws, only_off))
        assert not bool(sb2.empty[2])


def test_one_sample_and_no_images():
    n, A, k1, k2 = 1, 40, 1, 2
    ex = yc.example_batch(n, 13, 17, seed=3, specials=False)
    draws = yc.example_draws(n, A, k1, k2)
    sb, _ = yc.run_fused(ex, "cpu", A, True, k1, k2, True, draws=draws)
    merged, done = yc.run_composition(ex, "cpu", A, True, k1, k2, True, draws)
    yc.check_equals_composition(sb, merged, done)
    assert not bool(sb.empty[0])
    bare, _ = yc.run_fused(ex, "cpu", A, True, k1, k2, True, draws=draws, with_rgb=False, with_empty=False)
    assert bare.input_a is None and bare.input_b is None and bare.mask_a is None and bare.mask_b is None
    assert torch.equal(bare.idx_a, sb.idx_a) and torch.equal(bare.idx_b, sb.idx_b) and torch.equal(bare.offsets, sb.offsets)


@pytest.mark.parametrize("only_off,inv,h,w", [(True, True, 24, 36), (False, False, 24, 36), (True, False, 7, 9)])
def test_seeded_mode_matches_restatement_and_is_deterministic(only_off, inv, h, w):
    n, k1, k2 = 5, 2, 3
    A = 80 if h > 10 else 300                                                    # 7 x 9: more attempts than pixels
    ex = yc.example_batch(n, h, w, seed=11)
    sb, _ = yc.run_fused(ex, "cpu", A, only_off, k1, k2, inv, generator=torch.Generator().manual_seed(5))
    sc.check_layout(sb)
    assert sb.seeds.dtype == torch.int64 and sb.seeds.shape == (n,)
    mask = ex["mask"]
    some = False
    for s in range(n):
        U = lambda site, k, sd=int(sb.seeds[s]): sc.hash_uniform(sd, site, k)
        lists, typ, ka, kb = yc.restated_sample(ex, s, A, only_off, k1, k2, inv, U)
        sc.check_against_restatement(sb, s, lists, typ)
        if typ != 4:
            continue
        some = True
        got = sc.batch_lists(sb, s)
        M = len(ka) + len(kb)
        assert [len(got[2 * t]) for t in range(4)] == [M, k1 * M, k2 * M, 0]
        # a's entries precede b's; every kept entry of the object behind lies outside the front object's mask in both frames
        rows = np.array(ka + kb)
        assert np.array_equal(got[0], rows[:, 1] * w + rows[:, 0]) and np.array_equal(got[1], rows[:, 3] * w + rows[:, 2])
        for o, keep in ((0, ka), (1, kb)):
            for u1, v1, u2, v2 in keep:
                for f, (u, v) in enumerate(((u1, v1), (u2, v2))):
                    if (ex["fg"][s, f] == yc.FG_B) == (o == 0):
                        assert mask[2 * (1 - o) + f, s, v, u] == 0
        merged = ((mask[1, s] | mask[3, s]) != 0).reshape(-1)
        if merged.any():
            assert merged[got[3]].all()                                          # masked b-pixels inside the merged mask
        if inv and not merged.all():
            assert not merged[got[5]].any()                                      # background b-pixels outside it
    assert some
    again, _ = yc.run_fused(ex, "cpu", A, only_off, k1, k2, inv, generator=torch.Generator().manual_seed(5))
    for k in ("idx_a", "idx_b", "offsets", "seeds", "type", "empty", "input_a", "mask_b"):
        assert torch.equal(getattr(sb, k), getattr(again, k)), k
    by_seed, _ = yc.run_fused(ex, "cpu", A, only_off, k1, k2, inv, seeds=sb.seeds)
    assert torch.equal(by_seed.idx_a, sb.idx_a) and torch.equal(by_seed.idx_b, sb.idx_b)
    other, _ = yc.run_fused(ex, "cpu", A, only_off, k1, k2, inv, generator=torch.Generator().manual_seed(6))
    assert not (torch.equal(other.offsets, sb.offsets) and torch.equal(other.idx_a, sb.idx_a) and torch.equal(other.idx_b, sb.idx_b))


def test_replay_errors():
    from dcn_hip import samples
    n, A, k1, k2 = 5, 60, 2, 3
    ex = yc.example_batch(n, 24, 36, seed=2436)
    draws = yc.example_draws(n, A, k1, k2, seed=60)
    good = yc.fused_draws(ex, draws, True)
    ok, _ = yc.run_fused(ex, "cpu", A, True, k1, k2, True, draws=good)
    assert int(ok.status[0]) == 0 and good["cand_b"][1] is None and bool(ok.empty[1])   # a-empty sample without cand_b
    for site, cut in (("cand_a", A - 1), ("cand_b", A - 1), ("masked", 3), ("background", 0)):
        short = {k: list(v) for k, v in good.items()}
        short[site][0] = short[site][0][:cut]
        r, _ = yc.run_fused(ex, "cpu", A, True, k1, k2, True, draws=short)
        assert int(r.status[0]) == samples.BAD_DRAWS, site
    # a sample whose object a search FOUND something needs its cand_b stream, also when it ends up empty (sample 2)
    short = {k: list(v) for k, v in good.items()}
    short["cand_b"][2] = None
    r, _ = yc.run_fused(ex, "cpu", A, True, k1, k2, True, draws=short)
    assert int(r.status[0]) == samples.BAD_DRAWS
    with pytest.raises(ValueError, match="unknown draw sites"):
        yc.run_fused(ex, "cpu", A, True, k1, k2, True, draws=dict(good, cand=good["cand_a"]))
    with pytest.raises(ValueError, match="one entry per pair"):
        yc.run_fused(ex, "cpu", A, True, k1, k2, True, draws=dict(good, masked=good["masked"][:2]))


# ---- argument errors: one clause at a time on an otherwise valid n = 1, 7 x 9 call

N, H, W, A, K1, K2 = 1, 7, 9, 10, 2, 3
CAP = N * 2 * A * (1 + K1 + K2)
SENTINEL = 0x5A


def _valid_call():
    from dcn_hip import _lib
    lib = _lib.get()
    bufs = dict(depth=torch.full((4, N, H, W), 900, dtype=torch.int16), mask=torch.ones(4, N, H, W, dtype=torch.uint8),
                rgb=torch.zeros(4, N, H, W, 3, dtype=torch.uint8), cams=torch.zeros(2, N, 50),
                fg=torch.zeros(N, 2, dtype=torch.int32), seeds=torch.zeros(N, dtype=torch.int64),
                rand=torch.zeros(8), roff=torch.zeros(4, N + 1, dtype=torch.int64),
                ws=torch.empty(int(lib.dcn_synthetic_workspace(N, H, W, A)), dtype=torch.uint8))
    outs = dict(net_1=torch.empty(N, 3, H, W), net_2=torch.empty(N, 3, H, W), mask_1=torch.empty(N, H, W),
                mask_2=torch.empty(N, H, W), idx_a=torch.empty(CAP, dtype=torch.int64), idx_b=torch.empty(CAP, dtype=torch.int64),
                offsets=torch.empty(4 * N + 1, dtype=torch.int64), empty=torch.empty(N, dtype=torch.uint8),
                type=torch.empty(N, dtype=torch.int32), status=torch.empty(1, dtype=torch.int32))
    for t in outs.values():
        t.view(torch.uint8).fill_(SENTINEL)
    mean, std = np.array([0.5, 0.5, 0.5], np.float32), np.array([0.2, 0.2, 0.2], np.float32)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    args = dict(n=N, h=H, w=W, depth=P(bufs["depth"]), mask=P(bufs["mask"]), rgb=P(bufs["rgb"]), cams=P(bufs["cams"]),
                attempts=A, k_masked=K1, k_background=K2, flags=3, foreground=P(bufs["fg"]), empty_in=None,
                seeds=P(bufs["seeds"]), rand=None, rand_offsets=None, mean=mean.ctypes.data_as(ctypes.c_void_p),
                std=std.ctypes.data_as(ctypes.c_void_p), net_1=P(outs["net_1"]), net_2=P(outs["net_2"]),
                mask_1=P(outs["mask_1"]), mask_2=P(outs["mask_2"]), idx_a=P(outs["idx_a"]), idx_b=P(outs["idx_b"]),
                capacity=CAP, offsets=P(outs["offsets"]), empty=P(outs["empty"]), type=P(outs["type"]),
                status=P(outs["status"]), workspace=P(bufs["ws"]), stream=None)
    return lib, args, bufs, outs, (mean, std)


def test_valid_call_of_the_argument_tests_succeeds():
    lib, args, bufs, outs, keep = _valid_call()
    assert lib.dcn_synthetic_samples(*args.values()) == 0
    assert int(outs["status"][0]) == 0 and int(outs["offsets"][0]) == 0
    replay = dict(args, seeds=None, rand=ctypes.c_void_p(bufs["rand"].data_ptr()),
                  rand_offsets=ctypes.c_void_p(bufs["roff"].data_ptr()))
    assert lib.dcn_synthetic_samples(*replay.values()) == 0


BAD = [("n", 0), ("n", 1025), ("h", 0), ("w", 0), ("depth", None), ("mask", None), ("cams", None), ("attempts", 0),
       ("attempts", (1 << 30) + 1), ("k_masked", 0), ("k_background", 0), ("flags", 4), ("foreground", None), ("seeds", None),
       ("mean", None), ("std", None), ("idx_a", None), ("idx_b", None), ("idx_a", "misaligned"), ("idx_b", "misaligned"),
       ("capacity", CAP - 1), ("capacity", CAP + 1), ("offsets", None), ("empty", None), ("type", None), ("status", None),
       ("workspace", None), ("rgb", None)]


@pytest.mark.parametrize("name,value", BAD, ids=["%s=%s" % b for b in BAD])
def test_invalid_argument_is_refused_and_nothing_is_written(name, value):
    """(rgb = NULL with image outputs given is invalid; rgb = NULL without them is the no-image call.  seeds = NULL without
    rand / rand_offsets leaves no random source.)"""
    lib, args, bufs, outs, keep = _valid_call()
    if value == "misaligned":
        value = ctypes.c_void_p(outs[name].data_ptr() + 8)
    args[name] = value
    assert lib.dcn_synthetic_samples(*args.values()) == -1
    for k, t in outs.items():
        assert bool((t.view(torch.uint8) == SENTINEL).all()), k
    assert lib.dcn_synthetic_workspace(0, H, W, A) == 0 and lib.dcn_synthetic_workspace(N, H, W, 0) == 0


def test_python_argument_errors():
    from dcn_hip import samples
    ex = yc.example_batch(2, 7, 9, specials=False)
    t = lambda k: torch.from_numpy(ex[k].view(np.int16) if k == "depth" else ex[k])
    kw = dict(num_matching_attempts=10, sample_matches_only_off_mask=True, num_masked_non_matches_per_match=1,
              num_background_non_matches_per_match=1, use_image_b_mask_inv=True)
    f = samples.build_synthetic_multi_object_samples
    with pytest.raises(ValueError, match=r"mask must be \[4, B, H, W\]"):
        f(t("depth"), t("mask")[:2], t("cams"), **kw)
    with pytest.raises(ValueError, match="depth must be 16-bit integer"):
        f(t("depth")[:, :1], t("mask"), t("cams"), **kw)
    with pytest.raises(ValueError, match="depth must be 16-bit integer"):
        f(t("depth").float(), t("mask"), t("cams"), **kw)
    with pytest.raises(ValueError, match="cameras must be float32"):
        f(t("depth"), t("mask"), t("cams")[0], **kw)
    with pytest.raises(ValueError, match="rgb must be uint8"):
        f(t("depth"), t("mask"), t("cams"), t("rgb")[:, :, :, :, :2], **kw)
    with pytest.raises(ValueError, match="must be >= 1"):
        f(t("depth"), t("mask"), t("cams"), **dict(kw, num_matching_attempts=0))
    with pytest.raises(ValueError, match="foreground must be"):
        f(t("depth"), t("mask"), t("cams"), foreground=torch.zeros(3, 2), **kw)
    with pytest.raises(ValueError, match="empty must be"):
        f(t("depth"), t("mask"), t("cams"), empty=torch.zeros(3, dtype=torch.bool), **kw)
    with pytest.raises(ValueError, match="one int64 per pair"):
        f(t("depth"), t("mask"), t("cams"), seeds=torch.zeros(3, dtype=torch.int64), **kw)


# ---- the training batch

def _store(h=16, w=32):
    return yc.training_store("cpu", h, w, np.array([[20.0, 0, w / 2.0], [0, 20.0, h / 2.0], [0, 0, 1]]), still_scene=False)


def _cfg(probs, A=200):
    return yc.training_config(probs, A)


def test_training_batch_of_synthetic_samples_feeds_the_mixed_loss():
    from dcn_hip import frames
    from dense_correspondence.loss_functions import loss_composer
    from dense_correspondence.loss_functions.pixelwise_contrastive_loss import PixelwiseContrastiveLoss
    from oracle import synth
    store, cfg = _store(), _cfg({"SYNTHETIC_MULTI_OBJECT": 1.0})
    with pytest.raises(NotImplementedError, match="SYNTHETIC_MULTI_OBJECT"):
        frames.draw_training_batch(store, 4, cfg)
    n, h, w = 4, store.h, store.w
    sb, dt, fb = frames.draw_training_batch(store, n, cfg, generator=torch.Generator().manual_seed(3),
                                            host_rng=np.random.RandomState(3), synthetic_multi_object=True)
    assert dt == 4 and isinstance(fb, frames.FrameBatch) and fb.data_type == 4 and fb.rgb.shape == (4, n, h, w, 3)
    assert set(sb.type.tolist()) <= {4, -1} and 4 in sb.type.tolist()
    assert sb.input_a.shape == (n, 3, h, w) and sb.mask_b.shape == (n, h, w) and sb.aug_params is None
    sc.check_layout(sb)
    off = sb.offsets.numpy()
    assert all(off[4 * p + 4] == off[4 * p + 3] for p in range(n))               # no blind list
    pcl = PixelwiseContrastiveLoss(image_shape=(h, w), config=synth.LOSS_CONFIG)
    torch.manual_seed(0)
    ya, yb = torch.randn(n, h * w, 3, requires_grad=True), torch.randn(n, h * w, 3)
    out = loss_composer.get_loss_mixed(pcl, ya, yb, sb.device_lists())
    out[0].backward()
    assert bool(torch.isfinite(out[0])) and float(out[0]) > 0 and bool(torch.isfinite(ya.grad).all())


def test_training_batch_per_pair_types_groups_the_synthetic_type_last():
    from dcn_hip import frames
    store = _store()
    cfg = _cfg({"SINGLE_OBJECT_WITHIN_SCENE": 1.0, "SYNTHETIC_MULTI_OBJECT": 1.0})
    n = 6
    sb, drawn, fbs = frames.draw_training_batch(store, n, cfg, generator=torch.Generator().manual_seed(4),
                                                host_rng=np.random.RandomState(1), per_pair_types=True,
                                                synthetic_multi_object=True)
    assert set(drawn.tolist()) == {0, 4} and [f.data_type for f in fbs] == [0, 4]
    want = sorted(drawn.tolist())
    got = sb.type.tolist()
    assert all(g in (t, -1) for g, t in zip(got, want)) and 0 in got and 4 in got
    assert sb.input_a.shape[0] == n and sb.aug_params is None and sb.type.numel() == n
    sc.check_layout(sb)
    k = want.index(4)
    off = sb.offsets.numpy()
    assert all(off[4 * p + 4] == off[4 * p + 3] for p in range(k, n))
