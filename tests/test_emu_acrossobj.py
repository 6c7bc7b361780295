"""Across-object evaluation (csrc/acrossobj_kernels.hip, dcn_hip/evaluate/across_objects.py) through the host-emulation build: the reference's
own mask sampling and best-match search replayed (acrossobj goldens), the seeded sampling, the device-side status bits, ragged
batches, the host-side ValueErrors, the pair choice and evaluate_network_across_objects on a small store."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import acrossobj_common as ac
from dcn_hip import evaluate
from helpers import PKG, use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


def test_golden_set():
    assert sorted(ac.GOLDEN_IDS) == ["1x64_d1", "37x53_d16", "48x1_d1", "48x64_d3"]


@pytest.mark.parametrize("path", ac.GOLDENS, ids=ac.GOLDEN_IDS)
def test_golden_queries_and_best_matches(path):
    z = np.load(path)
    ac.check_golden(z, "cpu")
    assert list(z["columns"]) == list(evaluate.ACROSS_OBJECT_COLUMNS)


def _mask_and_descriptors(P=2, h=48, w=64, d=3, seed=5, fraction=0.3):
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(P, h, w, generator=g) < fraction).to(torch.uint8)
    return mask, torch.randn(P, h, w, d, generator=g)


def test_seeded_sampling_is_a_sample_without_replacement():
    mask, res = _mask_and_descriptors()
    P, h, w = mask.shape
    for Q in (100, 1):
        a = evaluate.across_object_queries(mask, res, Q, order_seeds=torch.arange(P) + 7)
        b = evaluate.across_object_queries(mask, res, Q, order_seeds=torch.arange(P) + 7)
        c = evaluate.across_object_queries(mask, res, Q, order_seeds=torch.arange(P) + 8)
        assert int(a.status[0]) == 0 and a.offsets.tolist() == [0, Q, 2 * Q]
        assert torch.equal(a.u_a, b.u_a) and torch.equal(a.v_a, b.v_a) and torch.equal(a.queries, b.queries)
        differs = False
        for p in range(P):
            u, v = a.u_a[p * Q:(p + 1) * Q], a.v_a[p * Q:(p + 1) * Q]
            assert (mask[p][v, u] != 0).all()                                   # inside the mask
            assert len(set((v * w + u).tolist())) == Q                         # distinct
            assert torch.equal(a.queries[p * Q:(p + 1) * Q], res[p][v, u])
            differs |= not torch.equal(u, c.u_a[p * Q:(p + 1) * Q])
        assert differs
    # as many samples as the mask has pixels: every pixel exactly once
    n = int(mask[0].sum())
    small = mask[:1].clone()
    keep = torch.nonzero(small[0].view(-1))[:50, 0]
    small.view(-1)[:] = 0
    small.view(-1)[keep] = 1
    e = evaluate.across_object_queries(small, res[:1], 50, generator=torch.Generator().manual_seed(1))
    assert n > 50 and int(e.status[0]) == 0
    assert sorted((e.v_a * w + e.u_a).tolist()) == keep.tolist()


def test_too_few_mask_pixels_gives_no_rows_and_the_status_bit():
    mask, res = _mask_and_descriptors(P=3)
    mask[1] = 0
    mask[1, 7, 3:12] = 1                                                         # 9 pixels, 10 asked
    q = evaluate.across_object_queries(mask, res, 10, order_seeds=[1, 2, 3])
    assert int(q.status[0]) == evaluate.TOO_FEW_MASK_PIXELS
    assert q.offsets.tolist() == [0, 10, 10, 20] and int(q.mask_pixels[1]) == 9
    assert (q.u_a[20:] == -1).all() and (q.v_a[20:] == -1).all() and (q.queries[20:] == 0).all()
    assert (mask[2][q.v_a[10:20], q.u_a[10:20]] != 0).all()
    m = evaluate.best_match_pairs(res, q.queries, q.offsets)
    assert int(m.status[0]) == 0 and m.row_pair.tolist() == [0] * 10 + [2] * 10 + [-1] * 10
    # exactly as many pixels as samples is enough
    q = evaluate.across_object_queries(mask, res, 9, order_seeds=[1, 2, 3])
    assert int(q.status[0]) == 0 and q.offsets.tolist() == [0, 9, 18, 27]


def test_bad_replay_ranks_are_flagged():
    mask, res = _mask_and_descriptors(P=2)
    n = [int(mask[p].sum()) for p in range(2)]
    good = np.stack([np.arange(5), np.arange(5) + 3])
    assert int(evaluate.across_object_queries(mask, res, 5, sample_order=good).status[0]) == 0
    for bad in ((1, 2, n[1]), (0, 0, -1), (1, 4, 3 + 1)):                       # past the mask's pixels, negative, repeated
        order = good.copy()
        order[bad[0], bad[1]] = bad[2]
        q = evaluate.across_object_queries(mask, res, 5, sample_order=order)
        assert int(q.status[0]) == evaluate.BAD_DRAWS, bad
        assert ((q.u_a >= 0) & (q.u_a < mask.shape[2]) & (q.v_a >= 0) & (q.v_a < mask.shape[1])).all()


def test_ragged_batch_offsets():
    """Pairs with and without rows interleaved; more queries than one LDS tile of the search holds"""
    P, h, w, d, Q = 6, 20, 28, 5, 70
    mask, res_a = _mask_and_descriptors(P, h, w, d, seed=9, fraction=0.4)
    mask[0] = 0
    mask[2] = 0
    mask[5] = 0
    g = torch.Generator().manual_seed(10)
    res_b = torch.randn(P, h, w, d, generator=g)
    q = evaluate.across_object_queries(mask, res_a, Q, order_seeds=torch.arange(P))
    assert int(q.status[0]) == 0 and q.offsets.tolist() == [0, 0, Q, Q, 2 * Q, 3 * Q, 3 * Q]
    m = evaluate.best_match_pairs(res_b, q.queries, q.offsets, max_pair_rows=Q)
    assert int(m.status[0]) == 0
    assert m.row_pair.tolist() == [1] * Q + [3] * Q + [4] * Q + [-1] * (3 * Q)
    for i, p in enumerate((1, 3, 4)):
        rows = slice(i * Q, (i + 1) * Q)
        assert (mask[p][q.v_a[rows], q.u_a[rows]] != 0).all()
        dist = torch.sqrt(((res_b[p].view(1, h * w, d) - q.queries[rows].view(Q, 1, d)) ** 2).sum(2))
        best = dist.argmin(1)
        assert torch.equal(m.best_uv[0, rows].long(), best % w) and torch.equal(m.best_uv[1, rows].long(), best // w)
        np.testing.assert_allclose(m.norm_diff_descriptor_best_match[rows].numpy(), dist.min(1).values.numpy(), rtol=1e-5)
    # the search checks the offsets it is given
    off = q.offsets.clone()
    off[-1] = 10 ** 6
    assert int(evaluate.best_match_pairs(res_b, q.queries, off).status[0]) & evaluate.BAD_OFFSETS
    cut = evaluate.best_match_pairs(res_b, q.queries, q.offsets, max_pair_rows=Q - 1)
    assert int(cut.status[0]) & evaluate.BAD_OFFSETS


def test_other_descriptor_dimensions():
    """A dimension without a kernel of its own (D = 7), the largest one (64), and a 16-byte-load dimension (D = 4)"""
    for d in (7, 64, 4):
        mask, res_a = _mask_and_descriptors(2, 9, 31, d, seed=d)
        res_b = torch.randn(2, 9, 31, d, generator=torch.Generator().manual_seed(d + 1))
        q = evaluate.across_object_queries(mask, res_a, 13, order_seeds=[4, 5])
        m = evaluate.best_match_pairs(res_b, q.queries, q.offsets)
        assert int(q.status[0]) == 0 and int(m.status[0]) == 0
        for p in range(2):
            rows = slice(13 * p, 13 * p + 13)
            dist = torch.sqrt(((res_b[p].view(1, -1, d) - q.queries[rows].view(13, 1, d)) ** 2).sum(2))
            assert torch.equal(m.best_uv[1, rows].long() * 31 + m.best_uv[0, rows].long(), dist.argmin(1))


def test_argument_validation():
    mask, res = _mask_and_descriptors()
    P, h, w = mask.shape
    for d in (0, 65):
        with pytest.raises(ValueError, match="descriptor dimension"):
            evaluate.across_object_queries(mask, torch.zeros(P, h, w, d), 5)
        with pytest.raises(ValueError, match="descriptor dimension"):
            evaluate.best_match_pairs(torch.zeros(P, h, w, d), torch.zeros(5, d), torch.zeros(P + 1, dtype=torch.int64))
    for Q in (0, 1025):
        with pytest.raises(ValueError, match="num_samples"):
            evaluate.across_object_queries(mask, res, Q)
    with pytest.raises(ValueError):                        # wrong dtypes
        evaluate.across_object_queries(mask, res.double(), 5)
    with pytest.raises(ValueError):
        evaluate.across_object_queries(mask.float(), res, 5)
    with pytest.raises(ValueError):
        evaluate.best_match_pairs(res.double(), torch.zeros(5, 3), torch.zeros(P + 1, dtype=torch.int64))
    with pytest.raises(ValueError):
        evaluate.best_match_pairs(res, torch.zeros(5, 3, dtype=torch.float64), torch.zeros(P + 1, dtype=torch.int64))
    with pytest.raises(ValueError):
        evaluate.best_match_pairs(res, torch.zeros(5, 3), torch.zeros(P + 1, dtype=torch.int32))
    with pytest.raises(ValueError):                        # shapes
        evaluate.across_object_queries(mask[:, :-1], res, 5)
    with pytest.raises(ValueError):
        evaluate.across_object_queries(mask, res, 5, sample_order=np.zeros((P, 4), np.int64))
    with pytest.raises(ValueError):
        evaluate.across_object_queries(mask, res, 5, order_seeds=[1, 2, 3])
    with pytest.raises(ValueError):
        evaluate.best_match_pairs(res, torch.zeros(5, 4), torch.zeros(P + 1, dtype=torch.int64))
    with pytest.raises(ValueError):
        evaluate.best_match_pairs(res, torch.zeros(5, 3), torch.zeros(P, dtype=torch.int64))
    store = ac.three_object_store("cpu", 8, 12)
    for bad in ([[0, store.num_frames]], [[-1, 0]], [[0, 1, 2]], []):
        with pytest.raises(ValueError):
            evaluate.evaluate_object_pairs(ac.StubNetwork(), store, np.asarray(bad, np.int64).reshape(len(bad), -1))


def test_the_device_library_refuses_cpu_tensors():
    """In a process of its own, which loads the shipped library (this one keeps the emulation)"""
    from dcn_hip import build
    code = r"""
import sys, torch
sys.path.insert(0, %r)
from dcn_hip import _lib, evaluate
_lib.load(%r)
said = []
for call in (lambda: evaluate.across_object_queries(torch.ones(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, 3), 2),
             lambda: evaluate.best_match_pairs(torch.zeros(1, 4, 4, 3), torch.zeros(2, 3), torch.tensor([0, 2]))):
    try:
        call()
    except ValueError as e:
        said.append("no CPU fallback" in str(e))
print("REFUSED" if said == [True, True] else said)
""" % (PKG, build.build_library())
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert b"REFUSED" in out.stdout, out.stderr.decode()[-2000:]


def test_choose_object_pairs_follows_the_rule():
    store = ac.three_object_store("cpu", 8, 12)
    got = evaluate.choose_object_pairs(store, 200, np.random.RandomState(5))
    assert got.shape == (200, 6) and got.dtype == np.int64
    assert np.array_equal(got, evaluate.choose_object_pairs(store, 200, np.random.RandomState(5)))
    first = np.asarray(store.scene_first_frame_host)
    for oa, ob, sa, sb, fa, fb in got:
        assert oa != ob
        assert sa in store.object_scenes_host[oa] and sb in store.object_scenes_host[ob]
        assert first[sa] <= fa < first[sa + 1] and first[sb] <= fb < first[sb + 1]
    # uniform over the ordered pairs of different objects, every scene and frame reachable
    ordered = {(a, b) for a, b in got[:, :2].tolist()}
    assert ordered == {(a, b) for a in range(3) for b in range(3) if a != b}
    counts = np.array([np.sum((got[:, 0] == a) & (got[:, 1] == b)) for a, b in sorted(ordered)])
    assert counts.min() > 200 / 6 / 2                                           # (expected 33 each; 6 sigma below is 0)
    assert set(got[:, 2].tolist()) | set(got[:, 3].tolist()) == set(range(5))
    assert set(got[:, 4].tolist()) | set(got[:, 5].tolist()) == set(range(store.num_frames))
    assert evaluate.choose_object_pairs(store, 3, np.random.default_rng(1)).shape == (3, 6)   # a numpy Generator works too
    assert evaluate.choose_object_pairs(store, 0).shape == (0, 6)
    one = ac.three_object_store("cpu", 8, 12)
    one.object_scenes_host = one.object_scenes_host[:1]
    with pytest.raises(ValueError, match="There is only one object, can't sample a different one"):
        evaluate.choose_object_pairs(one, 3, np.random.RandomState(0))
    store.object_scenes_host = [store.object_scenes_host[0], [], store.object_scenes_host[2]]
    with pytest.raises(ValueError, match="has no scene"):
        evaluate.choose_object_pairs(store, 50, np.random.RandomState(0))


def test_evaluate_network_across_objects_on_a_small_store():
    h, w, Q, N = 24, 32, 20, 7
    store = ac.three_object_store("cpu", h, w)
    dcn = ac.StubNetwork()
    dcn.train()
    gen = lambda: torch.Generator().manual_seed(4)
    table, df = evaluate.evaluate_network_across_objects(dcn, store, N, Q, host_rng=np.random.RandomState(2), generator=gen())
    assert dcn.training
    assert set(table) == {"scene_name_a", "scene_name_b", "img_a_idx", "img_b_idx", "object_id_a", "object_id_b",
                          "norm_diff_descriptor_best_match"}
    assert len(table["norm_diff_descriptor_best_match"]) == N * Q                # (every mask has at least Q pixels)
    assert list(df.columns) == list(evaluate.ACROSS_OBJECT_COLUMNS) and len(df) == N * Q
    chosen = evaluate.choose_object_pairs(store, N, np.random.RandomState(2))
    first = np.asarray(store.scene_first_frame_host)
    for p in range(N):
        rows = slice(p * Q, (p + 1) * Q)
        oa, ob, sa, sb, fa, fb = chosen[p]
        assert set(table["object_id_a"][rows]) == {store.object_ids[oa]} and set(table["object_id_b"][rows]) == {store.object_ids[ob]}
        assert set(table["scene_name_a"][rows]) == {store.scene_names[sa]} and set(table["scene_name_b"][rows]) == {store.scene_names[sb]}
        assert set(table["img_a_idx"][rows]) == {store.frame_ids[sa][fa - first[sa]]}
        assert set(table["img_b_idx"][rows]) == {store.frame_ids[sb][fb - first[sb]]}
    again, _ = evaluate.evaluate_network_across_objects(dcn, store, N, Q, host_rng=np.random.RandomState(2), generator=gen())
    assert np.array_equal(table["norm_diff_descriptor_best_match"], again["norm_diff_descriptor_best_match"])
    # the device chain by hand: the distances are those of the sampled pixels' best matches on the same descriptors
    net = ac.StubNetwork()
    t = evaluate.evaluate_object_pairs(net, store, chosen, Q, generator=gen(), batch_pairs=3)
    assert int(t.status[0]) == 0 and np.array_equal(t.norm_diff_descriptor_best_match.numpy(), table["norm_diff_descriptor_best_match"])
    res_a, res_b = net.descriptors()
    for p in range(N):
        rows = slice(p * Q, (p + 1) * Q)
        assert (store.mask[chosen[p, 4]][t.v_a[rows], t.u_a[rows]] != 0).all()
        dist = torch.sqrt(((res_b[p].view(1, h * w, 3) - res_a[p][t.v_a[rows], t.u_a[rows]].view(Q, 1, 3)) ** 2).sum(2))
        np.testing.assert_allclose(t.norm_diff_descriptor_best_match[rows].numpy(), dist.min(1).values.numpy(), rtol=1e-5)
    # a pair whose mask a is empty has no rows; one whose mask a has fewer pixels than samples is the reference's ValueError
    empty = ac.three_object_store("cpu", h, w)
    empty.mask[first[2]:first[3]] = 0                                            # object 1's only scene
    chosen = evaluate.choose_object_pairs(empty, 12, np.random.RandomState(3))
    table, _ = evaluate.evaluate_network_across_objects(ac.StubNetwork(), empty, 12, Q, host_rng=np.random.RandomState(3),
                                                        generator=gen())
    with_rows = int(np.sum(chosen[:, 0] != 1))
    assert 0 < with_rows < 12 and len(table["norm_diff_descriptor_best_match"]) == with_rows * Q
    assert "shoe" not in set(table["object_id_a"]) and "shoe" in set(table["object_id_b"])
    few = ac.three_object_store("cpu", h, w, small_mask_object=1)
    with pytest.raises(ValueError, match="Sample larger than population"):
        evaluate.evaluate_network_across_objects(ac.StubNetwork(), few, 12, Q, host_rng=np.random.RandomState(3), generator=gen())
    table, _ = evaluate.evaluate_network_across_objects(ac.StubNetwork(), few, 12, 5, host_rng=np.random.RandomState(3),
                                                        generator=gen())
    assert len(table["norm_diff_descriptor_best_match"]) == 12 * 5               # (5 pixels are enough for 5 samples)
