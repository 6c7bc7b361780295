"""Shared by tests/test_emu_descstats.py and tests/test_gpu_descstats.py: the checks of the descriptor statistics
(csrc/descstats_kernels.hip, dcn_hip/evaluate/descstats.py) against the descstats goldens (the reference's own
compute_descriptor_statistics / update_stats loop on prepared descriptor images, tests/golden/
make_descstats_goldens_from_reference.py), a float64 numpy statement and a float32 numpy replay of the combine stage.

The bound on a per-image mean is derived, not measured: the kernel accumulates in float64 (fewer than 2^19 terms per image
here: at most 2^-34 * mean|x|) and rounds the quotient to float32 once (at most 2^-24 * |mean| <= 2^-24 * mean|x|), so
|mean - mean_f64| <= 2^-23 * mean|x| per channel, mean|x| over the pixels the mean is taken over.  Against the reference's own
float32 mean the bound is that plus the reference's recorded error (triangle inequality).  Min and max are exact."""
import glob
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "descstats_ref_*.npz")))
GOLDEN_IDS = [os.path.basename(p)[len("descstats_ref_"):-4] for p in GOLDENS]
EXPECTED_IDS = ["a_37x53_d16", "b_48x64_d3", "c_1x64_d1", "c_48x1_d1", "d_37x53_d5"]
MEAN_BOUND = 2.0 ** -23
CHANNELS = (1, 3, 5, 16, 64)
_cache = {}


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def same_bits(a, b):
    """float32 arrays equal bit for bit; a NaN matches a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32, (a.dtype, b.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def numpy_statement(res, mask):
    """float64 numpy: -> (lohi float32 [n, 2, 2, d] exact min / max, mean_f64 [n, 2, d], mean_abs [n, 2, d], mask_pixels [n]);
    NaN in the mask rows of an empty mask"""
    n, h, w, d = res.shape
    flat, on = res.reshape(n, h * w, d), mask.reshape(n, h * w) != 0
    lohi = np.full((n, 2, 2, d), np.nan, np.float32)
    mean, mabs = np.full((n, 2, d), np.nan), np.full((n, 2, d), np.nan)
    for i in range(n):
        for k, x in enumerate((flat[i], flat[i][on[i]])):
            if len(x):
                lohi[i, k, 0], lohi[i, k, 1] = x.min(0), x.max(0)
                mean[i, k], mabs[i, k] = x.astype(np.float64).mean(0), np.abs(x.astype(np.float64)).mean(0)
    return lohi, mean, mabs, on.sum(1).astype(np.int32)


def numpy_combine(per_image, mask_pixels, num_images):
    """update_stats and the final scaling (evaluation.py:2237-2292) replayed in float32 numpy, sequentially in image order
    -> (stats float32 [2, 3, d], used)"""
    per_image = np.asarray(per_image, np.float32)
    d = per_image.shape[3]
    used = [i for i in range(per_image.shape[0]) if mask_pixels[i] != 0]
    if not used:
        return np.full((2, 3, d), np.nan, np.float32), 0
    lo, hi, mean = (per_image[used[0], :, j].copy() for j in range(3))
    for i in used[1:]:
        lo, hi = np.minimum(lo, per_image[i, :, 0]), np.maximum(hi, per_image[i, :, 1])
        mean = (mean + per_image[i, :, 2]).astype(np.float32)
    mean = (np.float32(1.0 / num_images) * mean).astype(np.float32)
    return np.stack([lo, hi, mean], axis=1).astype(np.float32), len(used)


def run(res, mask, device):
    from dcn_hip import evaluate
    per, pix = evaluate.descriptor_statistics(dev_t(res, device), dev_t(mask, device))
    assert per.dtype == torch.float32 and tuple(per.shape) == (res.shape[0], 2, 3, res.shape[3])
    assert pix.dtype == torch.int32 and tuple(pix.shape) == (res.shape[0],)
    return per.cpu().numpy(), pix.cpu().numpy()


def check_per_image(per, pix, res, mask, what=""):
    """Check 1 against the float64 numpy statement: exact min / max and mask_pixels, the derived bound on the means.
    Prints each figure before it asserts."""
    lohi, mean, mabs, n_on = numpy_statement(res, mask)
    assert np.array_equal(pix, n_on), (what, pix, n_on)
    assert same_bits(per[:, :, 0], lohi[:, :, 0]) and same_bits(per[:, :, 1], lohi[:, :, 1]), what
    empty = n_on == 0
    assert np.isnan(per[empty][:, 1]).all() and np.isfinite(per[~empty]).all() and np.isfinite(per[:, 0]).all(), what
    err = np.abs(per[:, :, 2].astype(np.float64) - mean)
    ok = ~np.isnan(mean)
    print("%s: largest |mean - mean_f64| / (2^-23 mean|x|) = %.3f" % (what, np.max(err[ok] / (MEAN_BOUND * mabs[ok]))))
    assert (err[ok] <= MEAN_BOUND * mabs[ok]).all(), what
    return mean, mabs


def check_golden_per_image(path, device):
    z = np.load(path)
    res, mask = z["res"], z["mask"]
    per, pix = run(res, mask, device)
    mean, mabs = check_per_image(per, pix, res, mask, os.path.basename(path))
    assert np.array_equal(pix, z["mask_pixels"])
    np.testing.assert_array_equal(mean, z["mean_f64"])                 # (the fixture's float64 means are this statement's)
    used = z["ref_used"]
    ref = z["ref_per_image"]
    # min and max: the reference's, bit for bit, wherever it has a tuple
    assert same_bits(per[used][:, :, :2], ref[used][:, :, :2])
    # the reference's own float32 mean: within its recorded error plus the kernel's bound
    err = np.abs(per[used][:, :, 2].astype(np.float64) - ref[used][:, :, 2].astype(np.float64))
    bound = z["ref_mean_err"][used] + MEAN_BOUND * mabs[used]
    print("largest |mean - reference mean| / bound = %.3f" % np.max(err / bound))
    assert (err <= bound).all()
    return z, per, pix


def check_golden_combine(path, device):
    from dcn_hip import evaluate
    z = np.load(path)
    n = int(z["num_images"])
    # the reference's per-image tuples (NaN rows for the image it skipped) -> its final dict, bit for bit
    stats, used = evaluate.combine_descriptor_statistics(dev_t(z["ref_per_image"], device), dev_t(z["mask_pixels"], device))
    assert stats.dtype == torch.float32 and used.dtype == torch.int32 and tuple(used.shape) == (1,)
    assert same_bits(stats.cpu().numpy(), z["ref_stats"])
    assert int(used.cpu()[0]) == int(z["ref_used"].sum())
    assert same_bits(numpy_combine(z["ref_per_image"], z["mask_pixels"], n)[0], z["ref_stats"])   # (the replay itself)
    # the kernel's own per-image statistics: min / max the reference's, means the float32 replay of the kernel's means
    per, pix = evaluate.descriptor_statistics(dev_t(z["res"], device), dev_t(z["mask"], device))
    stats, used = evaluate.combine_descriptor_statistics(per, pix, n)
    stats = stats.cpu().numpy()
    assert same_bits(stats[:, :2], z["ref_stats"][:, :2])
    want, n_used = numpy_combine(per.cpu().numpy(), pix.cpu().numpy(), n)
    assert same_bits(stats, want) and int(used.cpu()[0]) == n_used
    # num_images is the divisor: another one scales the means only
    other, _ = evaluate.combine_descriptor_statistics(per, pix, 2 * n)
    assert same_bits(other.cpu().numpy(), numpy_combine(per.cpu().numpy(), pix.cpu().numpy(), 2 * n)[0])
    assert same_bits(other.cpu().numpy()[:, :2], stats[:, :2]) and not same_bits(other.cpu().numpy()[:, 2], stats[:, 2])


def check_no_image_used(device):
    from dcn_hip import evaluate
    res, mask = np.ones((2, 3, 4, 2), np.float32), np.zeros((2, 3, 4), np.uint8)
    per, pix = evaluate.descriptor_statistics(dev_t(res, device), dev_t(mask, device))
    assert pix.cpu().tolist() == [0, 0] and torch.isnan(per[:, 1]).all() and (per[:, 0] == 1).all()
    stats, used = evaluate.combine_descriptor_statistics(per, pix)
    assert int(used.cpu()[0]) == 0 and torch.isnan(stats).all()


def random_images(D):
    """float32 [3, 240, 320, D] (several workgroups per image at every D) and partial masks; one draw shared by all D"""
    if "base" not in _cache:
        rng = np.random.RandomState(7)
        base = (rng.standard_normal((3, 240, 320, 64)) * 1.5 + 0.25).astype(np.float32)
        ys, xs = np.mgrid[0:240, 0:320]
        mask = np.stack([((xs - 150 - 20 * i) ** 2 + (ys - 110) ** 2 < (60 + 15 * i) ** 2) for i in range(3)]).astype(np.uint8)
        mask[2, -1, -1] = 3                                          # (the very last pixel; any non-zero value counts)
        _cache["base"] = (base, mask)
    base, mask = _cache["base"]
    return np.ascontiguousarray(base[..., :D]), mask


def check_channels(D, device):
    """Check 3"""
    res, mask = random_images(D)
    assert 0 < (mask != 0).sum() < mask.size
    per, pix = run(res, mask, device)
    check_per_image(per, pix, res, mask, "240x320 D=%d" % D)
    again, pix2 = run(res, mask, device)
    assert same_bits(per, again) and np.array_equal(pix, pix2)


NAN_CASES = ("37x53_d3", "240x320_d3", "240x320_d64")


def check_nan(device, case):
    """Check 4: one NaN in one channel -- outside the mask, then under it.  D = 3, channel 1, at 37 x 53 and at 240 x 320 (many
    workgroups per image: the pixels lie far from the image's start, so the flags and the NaN sums pass through the fold of
    the workgroups' partials, in the second image of the batch); and D = 64, channel 41, at 240 x 320, where more partials
    than runs are folded and the channel is not in the first channel group."""
    if case == "37x53_d3":
        rng = np.random.RandomState(3)
        res = rng.standard_normal((1, 37, 53, 3)).astype(np.float32)
        mask = np.zeros((1, 37, 53), np.uint8)
        mask[0, 10:25, 12:40] = 1
        i, ch, spots = 0, 1, ((False, (30, 5)), (True, (17, 20)))
    else:
        res, mask = random_images(3 if case.endswith("_d3") else 64)
        res, mask = res[:2], mask[:2]
        i, ch, spots = 1, (1 if case.endswith("_d3") else 41), ((False, (230, 5)), (True, (110, 170)))
    D = res.shape[3]
    others = [c for c in range(D) if c != ch]
    clean, clean_pix = run(res, mask, device)
    check_per_image(clean, clean_pix, res, mask, "without NaN")
    from dcn_hip import evaluate
    for under, (v, u) in spots:
        assert bool(mask[i, v, u]) == under
        x = res.copy()
        x[i, v, u, ch] = np.nan
        per, pix = run(x, mask, device)
        assert np.array_equal(pix, clean_pix)                        # (the count, over all workgroups, next to a NaN)
        assert np.isnan(per[i, 0, :, ch]).all()                      # entire image, that channel: min, max and mean
        assert np.isnan(per[i, 1, :, ch]).all() if under else same_bits(per[i, 1, :, ch], clean[i, 1, :, ch])
        # the other channels, and the other images: as without the NaN
        assert np.isfinite(per[i][:, :, others]).all() and same_bits(per[i][:, :, others], clean[i][:, :, others])
        assert same_bits(np.delete(per, i, axis=0), np.delete(clean, i, axis=0))
        # and through the combine stage: NaN stays NaN, the rest stays
        stats, used = evaluate.combine_descriptor_statistics(dev_t(np.concatenate([clean, per]), device),
                                                             dev_t(np.concatenate([clean_pix, pix]), device))
        stats = stats.cpu().numpy()
        assert int(used.cpu()[0]) == 2 * len(res)
        assert np.isnan(stats[0, :, ch]).all() and np.isnan(stats[1, :, ch]).all() == under
        assert np.isfinite(stats[:, :, others]).all()


def check_argument_errors(device, on_emulation):
    """Check 5"""
    import pytest
    from dcn_hip import evaluate
    ok_res, ok_mask = torch.zeros((2, 5, 7, 3), device=device), torch.ones((2, 5, 7), dtype=torch.uint8, device=device)
    evaluate.descriptor_statistics(ok_res, ok_mask)
    for res, mask in ((torch.zeros((2, 5, 7, 0), device=device), ok_mask),                     # D = 0
                      (torch.zeros((2, 5, 7, 65), device=device), ok_mask),                    # D = 65
                      (ok_res, ok_mask[:, :, :-1]), (ok_res, ok_mask[:1]), (ok_res[0], ok_mask),  # shapes
                      (ok_res.double(), ok_mask), (ok_res.half(), ok_mask),                    # dtypes
                      (ok_res, ok_mask.float()), (ok_res, ok_mask.to(torch.int32))):
        with pytest.raises(ValueError):
            evaluate.descriptor_statistics(res, mask)
    per, pix = evaluate.descriptor_statistics(ok_res, ok_mask)
    for a, b, k in ((per[:, :1], pix, None), (per, pix[:1], None), (per, pix.long(), None), (per.double(), pix, None),
                    (per, pix, 0)):
        with pytest.raises(ValueError):
            evaluate.combine_descriptor_statistics(a, b, k)
    if not on_emulation:                                             # CPU tensors passed to the device library
        with pytest.raises(ValueError):
            evaluate.descriptor_statistics(ok_res.cpu(), ok_mask.cpu())
        with pytest.raises(ValueError):
            evaluate.descriptor_statistics(ok_res, ok_mask.cpu())
        with pytest.raises(ValueError):
            evaluate.combine_descriptor_statistics(per.cpu(), pix.cpu())


def check_choose_frames(device):
    """Check 7"""
    import evaluate_common as ec
    from dcn_hip import evaluate
    store = ec.synthetic_store(device, 8, 12)
    assert not store.multi_scenes_host and len(store.object_scenes_host) == 2      # single-object scenes only
    got = evaluate.choose_frames(store, 200, np.random.RandomState(5))
    assert got.shape == (200, 2) and got.dtype == np.int64
    first = np.asarray(store.scene_first_frame_host)
    assert ((first[got[:, 0]] <= got[:, 1]) & (got[:, 1] < first[got[:, 0] + 1])).all()
    assert np.array_equal(got, evaluate.choose_frames(store, 200, np.random.RandomState(5)))
    assert not np.array_equal(got, evaluate.choose_frames(store, 200, np.random.RandomState(6)))
    for scenes in store.object_scenes_host:                          # every object's scenes appear, and every frame of them
        for s in scenes:
            assert set(got[got[:, 0] == s, 1].tolist()) == set(range(first[s], first[s + 1])), s
    assert evaluate.choose_frames(store, 3, np.random.default_rng(1)).shape == (3, 2)
    assert evaluate.choose_frames(store, 0, np.random.RandomState(0)).shape == (0, 2)
    # the scene rule is choose_pairs': the same generator state gives the same first scene
    assert evaluate.choose_frames(store, 1, np.random.RandomState(9))[0, 0] == evaluate.choose_pairs(
        store, 1, np.random.RandomState(9), threshold=-1.0)[0, 0]


def _as_arrays(d):
    return np.array([[d[s][f] for f in ("min", "max", "mean")] for s in ("entire_image", "mask_image")])


def check_whole_call(device, h, w, dcn, tmp_path):
    """Check 6.  ``compute_descriptor_statistics_on_dataset(num_images=6, batch_images=4)`` against
      * the same frames through the same pieces with the network run on the SAME batches (4 + 2) but the statistics image by
        image: equal, bit for bit (gather order, slices, combine, the one copy);
      * the same frames one at a time through forward_image_tensors, descriptor_statistics and combine_descriptor_statistics.
        A batch of one has another shape than a batch of four, i.e. on the GPU other tiles and another summation order in the
        backbone, whose parity bound is 1e-4 of the descriptor image's largest magnitude per element (smoke(), the parity
        tests, tests/test_gpu_evaluate.py's chaining test): a min, a max or a mean of elements that each move by at most that
        moves by at most that.  On the host emulation the two are equal bit for bit, and that is asserted."""
    import evaluate_common as ec
    import dense_correspondence_manipulation.utils.utils as utils
    from dcn_hip import _lib, augment, evaluate
    store = ec.synthetic_store(device, h, w)
    dev = torch.device(device)
    dcn.config = {}
    dcn.train()
    filename = str(tmp_path / "descriptor_statistics.yaml")
    got = evaluate.compute_descriptor_statistics_on_dataset(dcn, store, num_images=6, batch_images=4,
                                                            host_rng=np.random.RandomState(1), filename=filename)
    assert dcn.training
    assert set(got) == {"entire_image", "mask_image"} and all(set(v) == {"min", "max", "mean"} for v in got.values())
    D = dcn.descriptor_dimension
    assert all(isinstance(x, float) for v in got.values() for f in v.values() for x in f)
    assert all(len(f) == D for v in got.values() for f in v.values())
    assert utils.getDictFromYamlFilename(filename) == got
    # pointing the network's params folder at that directory: the descriptor_image_stats property reads the file
    dcn.config = {"path_to_network_params_folder": str(tmp_path)}
    assert dcn.descriptor_image_stats == got
    # ... and it is the default file; eval mode stays eval mode
    folder = tmp_path / "other"
    folder.mkdir()
    dcn.config = {"path_to_network_params_folder": str(folder)}
    dcn.eval()
    one = evaluate.compute_descriptor_statistics_on_dataset(dcn, store, num_images=1, host_rng=np.random.RandomState(1))
    assert not dcn.training
    assert os.listdir(str(folder)) == ["descriptor_statistics.yaml"]
    assert utils.getDictFromYamlFilename(str(folder / "descriptor_statistics.yaml")) == one
    # the replays
    chosen = evaluate.choose_frames(store, 6, np.random.RandomState(1))
    zeros = lambda k: torch.zeros((k, augment.PARAM_WORDS), dtype=torch.int32, device=dev)

    def replay(batches):
        per, pix, top = [], [], 0.0
        for fr in batches:
            f = torch.from_numpy(np.asarray(fr)).to(dev)
            x = augment.augment_images(store.rgb[f], store.mask[f], zeros(len(fr)), want_mask=False)["input_a"]
            res = dcn.forward_image_tensors(x)
            top = max(top, float(res.abs().max()))
            for j in range(len(fr)):
                a, b = evaluate.descriptor_statistics(res[j:j + 1], store.mask[f[j:j + 1]])
                per.append(a)
                pix.append(b)
        stats, used = evaluate.combine_descriptor_statistics(torch.cat(per), torch.cat(pix), 6)
        assert int(used.cpu()[0]) == 6
        return stats.double().cpu().numpy(), top
    if not _lib.is_hostemu():      # (on the emulation the one-at-a-time replay below is itself bit for bit, and every forward costs)
        same, _ = replay([chosen[:4, 1], chosen[4:, 1]])
        assert np.array_equal(same, _as_arrays(got))
    single, top = replay([[f] for f in chosen[:, 1]])
    dev_max = np.abs(single - _as_arrays(got)).max()
    print("one at a time against batches of 4: largest deviation %.3e, bound %.3e" % (dev_max, 1e-4 * top))
    assert dev_max <= 1e-4 * top
    if _lib.is_hostemu():
        assert np.array_equal(single, _as_arrays(got))
    # every mask empty: no statistics
    empty = ec.synthetic_store(device, h, w)
    empty.mask.zero_()
    import pytest
    with pytest.raises(ValueError, match="empty mask"):
        evaluate.compute_descriptor_statistics_on_dataset(dcn, empty, num_images=1, save_to_file=False,
                                                          host_rng=np.random.RandomState(1))
    assert utils.getDictFromYamlFilename(str(folder / "descriptor_statistics.yaml")) == one
