"""Shared checks of validation while training from a frame store (dcn_hip.train.Validation, StoreTrainer(validation=...)),
taking the stores, the network factory and the configuration of the calling test module.  Not a test module."""
import os

import numpy as np
import torch

import train_common as tc
from dcn_hip import evaluate
from dcn_hip.train import LOG_COLUMNS, VALIDATION_HEAD, StoreTrainer, Validation, validation_key

PAIRS, MATCHES = 4, 20
FIELDS = ("pixel_match_error_l2", "norm_diff_pred_3d", "norm_diff_descriptor_ground_truth",
          "fraction_pixels_closer_than_ground_truth")


def make_validation(vstore, seed, **kw):
    kw.setdefault("fields", FIELDS)
    return Validation(vstore, num_image_pairs=PAIRS, num_matches_per_image_pair=MATCHES, batch_pairs=2,
                      generator=torch.Generator(device=vstore.device).manual_seed(seed), host_rng=np.random.RandomState(seed),
                      **kw)


def trainer(make_dcn, pcl, store, cfg, B, seed, validation=None, **kw):
    return StoreTrainer(make_dcn(), pcl, store, cfg, generator=torch.Generator(device=store.device).manual_seed(seed),
                        host_rng=np.random.RandomState(seed), batch_size=B, validation=validation, **kw)


def loop(tr, n):
    for it in range(1, n + 1):
        tr.iteration(it)
        if tr.validation is not None and tr.validation.due(it):
            tr.validate(it)


def check_training_is_the_same_run(make_dcn, pcl, store, vstore, cfg, B, mixed):
    """V1: six iterations with Validation(rate=2, after=0) and without, from the same seeds"""
    seed = tc.find_seed(store, cfg, B, 6, 2, mixed=mixed)
    plain = trainer(make_dcn, pcl, store, cfg, B, seed)
    val = make_validation(vstore, 3, rate=2, after=0)
    with_v = trainer(make_dcn, pcl, store, cfg, B, seed, validation=val)
    for tr in (plain, with_v):
        tr.dcn.train()
        loop(tr, 6)
    assert with_v.dcn.training and val.rows == 3
    a, b = plain.read_log(), with_v.read_log()
    assert a.history.shape == (6, LOG_COLUMNS) and np.array_equal(a.history.view(np.int64), b.history.view(np.int64))
    assert 0 < a.num_active < 6 and (a.t, a.num_active, a.num_skipped) == (b.t, b.num_active, b.num_skipped)
    assert tc.bits64(a.lr) == tc.bits64(b.lr)
    for (k, p), q in zip(plain.dcn.named_parameters(), with_v.dcn.parameters()):
        assert tc.same_bits(p, q), k
    for (k, p), q in zip(plain.dcn.named_buffers(), with_v.dcn.buffers()):
        assert torch.equal(p, q), k
    for p, q in zip(plain.dcn.parameters(), with_v.dcn.parameters()):
        sa, sb = plain.optimizer.state[p], with_v.optimizer.state[q]
        assert tc.same_bits(sa["exp_avg"], sb["exp_avg"]) and tc.same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert set(plain.logging_dict) == {"train", "test"} and set(with_v.logging_dict) == {"train", "test", "validation"}
    assert plain.logging_dict["train"] == with_v.logging_dict["train"]
    assert with_v.validation_history[:, 0].tolist() == [2, 4, 6]
    assert with_v.validation_history[:, 1].tolist() == a.history[[1, 3, 5], 1].tolist()
    return with_v


def check_row_equals_the_pass_by_hand(make_dcn, pcl, store, vstore, cfg, B, mixed):
    """V2: rate=6, after=0"""
    seed = tc.find_seed(store, cfg, B, 6, 2, mixed=mixed)
    val = make_validation(vstore, 9, rate=6, after=0, fields=evaluate.CURVE_FIELDS)
    tr = trainer(make_dcn, pcl, store, cfg, B, seed, validation=val)
    tr.dcn.train()
    loop(tr, 6)
    snap = tr.read_log()
    rows = tr.validation_history
    C = len(evaluate.CURVE_FIELDS)
    assert rows.shape == (1, VALIDATION_HEAD + 8 * C) and rows[0, 0] == 6 and rows[0, 1] == snap.history[5][1]
    chosen = evaluate.choose_pairs(vstore, PAIRS, np.random.RandomState(9))
    t = evaluate.evaluate_frame_pairs(tr.dcn, vstore, chosen, MATCHES, batch_pairs=2,
                                      generator=torch.Generator(device=vstore.device).manual_seed(9))
    curves = evaluate.evaluation_curves(t, evaluate.CURVE_FIELDS, 100)
    assert tr.dcn.training
    want = curves.summary.cpu().numpy().reshape(-1)
    got = rows[0, VALIDATION_HEAD:]
    same = (got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (got, want)
    assert rows[0, 2] == int(t.status.cpu()[0]) == 0 and rows[0, 3] == int(curves.status.cpu()[0])
    assert want.reshape(C, 8)[:, 0].max() > 0                               # there were rows to reduce


def check_inactive_iteration(make_dcn, pcl, store, vstore, cfg, within_cfg, B, h, w, mixed):
    """V4: a pass on an iteration made inactive by a batch from a store whose every scene is still"""
    from dcn_hip import frames
    seed = tc.find_seed(store, cfg, B, 6, 2, mixed=mixed)
    types = tc.draws(store, cfg, B, seed, 3)
    val = make_validation(vstore, 5, rate=1, after=0)
    tr = trainer(make_dcn, pcl, store, cfg, B, seed, validation=val)
    still = tc.still_store(store.device, h, w)
    tr.dcn.train()
    for it in (1, 2, 3, 4):
        if it == 3:
            sb = frames.draw_training_batch(still, B, within_cfg, generator=tr.generator, host_rng=tr.host_rng,
                                            per_pair_types=True)[0]
            tr.step_on_batch(sb, it)
        else:
            tr.iteration(it)
        tr.validate(it)
    snap = tr.read_log()
    rows = tr.validation_history
    active = [bool(r[1]) for r in snap.history]
    assert rows[:, 0].tolist() == [1, 2, 3, 4] and not active[2] and any(active), active
    assert active[:2] == [not all(t == -1 for t in ts) for ts in types[:2]]
    assert [bool(a) for a in rows[:, 1]] == active
    d = tr.logging_dict["validation"]
    assert d["iteration"] == [it for it, a in zip((1, 2, 3, 4), active) if a] and 3 not in d["iteration"]
    assert set(d) == {"iteration"} | {validation_key(f) for f in FIELDS} | {f + "_count" for f in FIELDS}
    assert "norm_diff_3d_area_above_curve" in d
    for f in FIELDS:
        assert len(d[validation_key(f)]) == len(d[f + "_count"]) == len(d["iteration"])
        assert all(np.isfinite(v) and v >= 0 for v in d[validation_key(f)]), (f, d[validation_key(f)])
        assert all(isinstance(c, int) and c > 0 for c in d[f + "_count"])
    # the inactive row was evaluated all the same: the host could not know
    assert rows[2, VALIDATION_HEAD] > 0 and np.isfinite(rows[2, VALIDATION_HEAD + 6])


def check_save_point(make_dcn, pcl, store, vstore, cfg, B, tmp_path):
    """V5, and V6's schedule through run()"""
    import yaml
    cfg = {"training": dict(cfg["training"], save_rate=2, num_iterations=3, steps_between_learning_rate_decay=2)}
    seed = tc.find_seed(store, cfg, B, 4, 2, accept=lambda ts: not all(t == -1 for t in ts[3]))
    folder = str(tmp_path / "run")
    val = make_validation(vstore, 2, rate=2, after=1)
    tr = trainer(make_dcn, pcl, store, cfg, B, seed, validation=val, logging_dir=folder)
    log = tr.run()                             # ends at iteration 4, the first active one past 3
    assert set(log) == {"train", "test", "validation"} and log is tr.logging_dict
    assert tr.validation_history[:, 0].tolist() == [2, 4] and log["validation"]["iteration"][-1] == 4
    with open(os.path.join(folder, "000004_log_history.yaml")) as f:
        assert yaml.safe_load(f) == log
    with open(os.path.join(folder, "loss.yaml")) as f:
        assert set(yaml.safe_load(f)) == {"train", "test"}
    lines = [r.split("\t") for r in open(os.path.join(folder, "tensorboard", "scalars.tsv")).read().strip().split("\n")]
    for f in FIELDS:
        got = [(int(s), float(v)) for s, name, v in lines if name == "validation %s area above curve" % f]
        assert got == list(zip(log["validation"]["iteration"], log["validation"][validation_key(f)])), f
    assert any(name.startswith("train loss") for _, name, _ in lines)
    # without the option: the reference's two keys, the same files
    plain_folder = str(tmp_path / "plain")
    plain = trainer(make_dcn, pcl, store, cfg, B, seed, logging_dir=plain_folder)
    plain_log = plain.run()
    assert set(plain_log) == {"train", "test"} and plain_log["train"] == log["train"]
    assert sorted(os.listdir(plain_folder)) == sorted(os.listdir(folder))
    assert not any("validation" in r for r in open(os.path.join(plain_folder, "tensorboard", "scalars.tsv")))


def check_schedule_and_arguments(make_dcn, pcl, store, vstore, other_size_store, cfg):
    """V6"""
    import pytest
    val = make_validation(vstore, 1, rate=3, after=5)
    assert [it for it in range(1, 16) if val.due(it)] == [6, 9, 12, 15]
    assert [it for it in range(1, 12) if make_validation(vstore, 1, rate=5).due(it)] == [10]       # after=5, the default
    assert [it for it in range(1, 6) if make_validation(vstore, 1, rate=2, after=0).due(it)] == [2, 4]
    with pytest.raises(ValueError, match="validation store of"):
        StoreTrainer(make_dcn(), pcl, store, cfg, validation=make_validation(other_size_store, 1, rate=2))
    with pytest.raises(TypeError, match="Validation"):
        StoreTrainer(make_dcn(), pcl, store, cfg, validation=vstore)
    with pytest.raises(ValueError, match="rate"):
        make_validation(vstore, 1, rate=0)
    with pytest.raises(ValueError, match="fields"):
        make_validation(vstore, 1, rate=2, fields=("no_such_column",))
    with pytest.raises(ValueError, match="num_bins"):
        make_validation(vstore, 1, rate=2, num_bins=1)
    with pytest.raises(ValueError, match="no validation"):
        StoreTrainer(make_dcn(), pcl, store, cfg).validate(1)
