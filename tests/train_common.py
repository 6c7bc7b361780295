"""Shared by tests/test_emu_train.py and tests/test_gpu_train.py (not a test module): the checks of the device-resident
training state (csrc/train_kernels.hip, dcn_hip.optim.GuardedAdam, dcn_hip.train) on whichever library the caller has loaded.

Yardsticks: ``dcn_hip.optim.Adam`` (dcn_adam_step) for the guarded optimizer step, a Python replay in double for the state,
and for the whole loop a plain loop that reads the types on the host after every draw and ``continue``s on an all-empty batch
before anything else, as training.py:304-306 does."""
import ctypes
import math
import struct

import numpy as np
import torch

NUMELS = (1, 3, 4096, 4097, 8195)
WITHIN, ACROSS, DIFFERENT = 0, 1, 2


# ------------------------------------------------------------------------------------------------ helpers
def make_state(device, lr=1.0e-3, every=1000, decay=0.9, rows=64):
    from dcn_hip.train import TrainState
    return TrainState(device, lr, every, decay, rows=rows)


def types_tensor(values, device):
    return torch.tensor(values, dtype=torch.int32, device=device)


def bits64(x):
    return struct.pack("<d", float(x))


def bits32(x):
    return struct.pack("<f", float(x))


def adam_tensors(device, seed=0):
    """81 parameters (the 80-entry table is crossed): numels 1, 3, 4096, 4097, 8195 in turn, and one that is a view starting
    one float into its storage (4-byte aligned only: the scalar path)."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(NUMELS[i % len(NUMELS)], generator=g).to(device) for i in range(80)]
    ps.append(torch.randn(4098, generator=g).to(device)[1:])
    assert ps[-1].data_ptr() % 16 == 4 and len(ps) == 81
    return [torch.nn.Parameter(p) for p in ps]


def set_grads(ps, seed):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = (torch.randn(p.shape, generator=g) * 10.0 ** float(torch.randint(-4, 3, (1,), generator=g))).to(p.device)


def same_bits(a, b):
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def assert_same_optimizer_tensors(ps_a, opt_a, ps_b, opt_b, what):
    for i, (a, b) in enumerate(zip(ps_a, ps_b)):
        assert same_bits(a, b), (what, "p", i)
        assert same_bits(opt_a.state[a]["exp_avg"], opt_b.state[b]["exp_avg"]), (what, "exp_avg", i)
        assert same_bits(opt_a.state[a]["exp_avg_sq"], opt_b.state[b]["exp_avg_sq"]), (what, "exp_avg_sq", i)


# ------------------------------------------------------------------------------------------------ T1
def check_guarded_adam_three_steps(device):
    """Three active steps, the learning rate decayed (on the device) between the second and the third: p, exp_avg and
    exp_avg_sq equal Adam.step()'s driven with the same learning rate, bit for bit."""
    from dcn_hip.optim import Adam, GuardedAdam
    ref, ours = adam_tensors(device), adam_tensors(device)
    lr = 1.0e-3
    r = Adam(ref, lr=lr, weight_decay=1.0e-4)
    o = GuardedAdam(ours, lr=lr, weight_decay=1.0e-4)
    state = make_state(device, lr=lr, every=3, decay=0.9)
    active = types_tensor([0], device)
    for it in (1, 2, 3):
        set_grads(ref, 40 + it)
        set_grads(ours, 40 + it)
        if it % 3 == 0:
            for gr in r.param_groups:
                gr["lr"] = gr["lr"] * 0.9
        r.step()
        state.advance(active, it)
        o.step(state)
        assert_same_optimizer_tensors(ours, o, ref, r, it)
    snap = state.read()
    assert snap.t == 3 and bits64(snap.lr) == bits64(r.param_groups[0]["lr"]) and snap.num_active == 3 and snap.num_skipped == 0


def check_guarded_adam_inactive_step(device):
    """An inactive step between two active ones: every p, m and v, the device t and the following active step are those of a
    run without it."""
    from dcn_hip.optim import GuardedAdam
    with_it, without = adam_tensors(device, 1), adam_tensors(device, 1)
    a = GuardedAdam(with_it, lr=2.0e-3, weight_decay=1.0e-4)
    b = GuardedAdam(without, lr=2.0e-3, weight_decay=1.0e-4)
    sa, sb = make_state(device, lr=2.0e-3), make_state(device, lr=2.0e-3)
    active, empty = types_tensor([-1, 2], device), types_tensor([-1, -1], device)
    for ps, opt, st in ((with_it, a, sa), (without, b, sb)):
        set_grads(ps, 7)
        st.advance(active, 1)
        opt.step(st)
    before = [(p.detach().clone(), a.state[p]["exp_avg"].clone(), a.state[p]["exp_avg_sq"].clone()) for p in with_it]
    set_grads(with_it, 8)                        # a gradient that would move everything
    sa.advance(empty, 2)
    a.step(sa)
    for i, (p, (p0, m0, v0)) in enumerate(zip(with_it, before)):
        assert same_bits(p, p0) and same_bits(a.state[p]["exp_avg"], m0) and same_bits(a.state[p]["exp_avg_sq"], v0), i
    snap = sa.read()
    assert snap.t == 1 and snap.active == 0 and snap.num_active == 1 and snap.num_skipped == 1
    set_grads(with_it, 9)
    set_grads(without, 9)
    sa.advance(active, 3)
    sb.advance(active, 2)
    a.step(sa)
    b.step(sb)
    assert_same_optimizer_tensors(with_it, a, without, b, "after the inactive step")
    sa_, sb_ = sa.read(), sb.read()
    assert sa_.t == sb_.t == 2 and bits32(sa_.step_size) == bits32(sb_.step_size) and bits32(sa_.bc2_sqrt) == bits32(sb_.bc2_sqrt)
    assert any(not same_bits(p, p0) for p, (p0, _, _) in zip(with_it, before))


def check_guarded_adam_state_dict_round_trip(device):
    """state_dict() -> torch.optim.Adam.load_state_dict -> its state_dict() -> a fresh GuardedAdam on a fresh state: steps and
    learning rate are the device's, and the next step equals the original's bit for bit."""
    import copy
    from dcn_hip.optim import GuardedAdam
    ps, qs = adam_tensors(device, 2), adam_tensors(device, 2)
    o = GuardedAdam(ps, lr=1.0e-3, weight_decay=1.0e-4)
    state = make_state(device, lr=1.0e-3, every=2, decay=0.5)
    active = types_tensor([0], device)
    for it in (1, 2, 3):
        set_grads(ps, it)
        state.advance(active, it)
        o.step(state)
    sd = o.state_dict()
    assert all(float(s["step"]) == 3.0 for s in sd["state"].values()) and len(sd["state"]) == 81
    assert sd["param_groups"][0]["lr"] == 1.0e-3 * 0.5
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    t = torch.optim.Adam(qs, lr=1.0)
    t.load_state_dict(copy.deepcopy(sd))
    o2 = GuardedAdam(qs, lr=1.0)
    o2.load_state_dict(copy.deepcopy(t.state_dict()))
    state2 = o2.bind(make_state(device, lr=123.0, every=2, decay=0.5))       # seeded with the loaded step and learning rate
    set_grads(ps, 4)
    set_grads(qs, 4)
    state.advance(active, 4)
    o.step(state)
    state2.advance(active, 4)
    o2.step(state2)
    assert_same_optimizer_tensors(qs, o2, ps, o, "restored")
    s1, s2 = state.read(), state2.read()
    assert s1.t == s2.t == 4 and bits64(s1.lr) == bits64(s2.lr) == bits64(1.0e-3 * 0.5 * 0.5)
    assert sorted(o2.state_dict()["state"]) == sorted(sd["state"])


# ------------------------------------------------------------------------------------------------ T2
GUARD_F, GUARD_I = -12345.5, -0x0123456789ABCDEF


def check_guarded_copy(device):
    """Float tensors of 1, 64 and 2048 elements and int64 scalars in one table: copied with the matching flag (or no state),
    untouched with the other, and the words on both sides of every destination keep their guard value."""
    from dcn_hip import _lib
    g = torch.Generator().manual_seed(3)
    state = make_state(device)

    def fresh():
        srcs, bigs, dsts = [], [], []
        for n in (1, 64, 2048, 64, 1):
            srcs.append(torch.randn(n, generator=g).to(device))
            bigs.append(torch.full((n + 2,), GUARD_F, device=device))
            dsts.append(bigs[-1][1:n + 1])
        for k in range(3):
            srcs.append(torch.tensor(1000 + k, dtype=torch.int64, device=device))
            bigs.append(torch.full((3,), GUARD_I, dtype=torch.int64, device=device))
            dsts.append(bigs[-1][1])
        return srcs, bigs, dsts

    def run(active, when, use_state=True):
        srcs, bigs, dsts = fresh()
        state.advance(types_tensor([0 if active else -1], device), 1)
        n = len(srcs)
        d = (ctypes.c_void_p * n)(*[x.data_ptr() for x in dsts])
        s = (ctypes.c_void_p * n)(*[x.data_ptr() for x in srcs])
        b = (ctypes.c_int64 * n)(*[x.numel() * x.element_size() for x in srcs])
        rc = _lib.get().dcn_guarded_copy(n, d, s, b, ctypes.c_void_p(state.state_ptr()) if use_state else None, when,
                                         _lib.stream_ptr())
        assert rc == 0
        copied = [torch.equal(x, y) for x, y in zip(dsts, srcs)]
        untouched = [bool((x == (GUARD_F if x.dtype == torch.float32 else GUARD_I)).all()) for x in dsts]
        for big in bigs:
            guard = GUARD_F if big.dtype == torch.float32 else GUARD_I
            assert big[0].item() == guard and big[-1].item() == guard
        return all(copied), all(untouched)
    assert run(True, 1) == (True, False) and run(False, 0) == (True, False)
    assert run(True, 0) == (False, True) and run(False, 1) == (False, True)
    assert run(True, 0, use_state=False) == (True, False)
    lib = _lib.get()
    one = (ctypes.c_void_p * 1)(state.buf.data_ptr())
    assert lib.dcn_guarded_copy(1, one, one, (ctypes.c_int64 * 1)(6), None, 0, _lib.stream_ptr()) == -1       # not whole words
    odd = (ctypes.c_void_p * 1)(state.buf.data_ptr() + 2)
    assert lib.dcn_guarded_copy(1, odd, one, (ctypes.c_int64 * 1)(8), None, 0, _lib.stream_ptr()) == -1       # misaligned


# ------------------------------------------------------------------------------------------------ T3
def host_bias_corrections(lr, t, beta1=0.9, beta2=0.999):
    """The host formula of dcn_adam_step (csrc/adam_update.h): beta^t by repeated squaring in double, one rounding to float."""
    b1t, b2t, a, b, e = 1.0, 1.0, beta1, beta2, int(t)
    while e > 0:
        if e & 1:
            b1t *= a
            b2t *= b
        a *= a
        b *= b
        e >>= 1
    return np.float32(lr / (1.0 - b1t)), np.float32(math.sqrt(1.0 - b2t))


ADVANCE_ACTIVE = [True, True, False, True, False, True, True, True, True, False, True, True]   # iterations 1 .. 12


def check_advance(device):
    """12 iterations, decay 0.9 every 3: iteration 3 is inactive ON a decay boundary (the decay is not applied), 6, 9 and 12
    are active ones, 5 and 10 inactive elsewhere.  lr after every iteration is the Python replay's double, t counts the
    active iterations, step_size / bc2_sqrt are the host formula's floats."""
    assert not ADVANCE_ACTIVE[2] and ADVANCE_ACTIVE[5] and not ADVANCE_ACTIVE[4]
    lr0 = 1.0e-4
    state = make_state(device, lr=lr0, every=3, decay=0.9)
    lr, t = lr0, 0
    for it, act in enumerate(ADVANCE_ACTIVE, 1):
        state.advance(types_tensor([-1, 1 if it % 2 else 0, -1] if act else [-1, -1, -1], device), it)
        if act:
            if it % 3 == 0:
                lr = lr * 0.9
            t += 1
        s = state.read()
        assert bits64(s.lr) == bits64(lr), (it, s.lr, lr)
        assert s.t == t and s.active == int(act), (it, s.t, t)
        if t:
            want = host_bias_corrections(lr, t)
            assert bits32(s.step_size) == bits32(want[0]) and bits32(s.bc2_sqrt) == bits32(want[1]), (it, s.step_size, want)
    assert t == 9 and s.num_active == 9 and s.num_skipped == 3 and bits64(lr) == bits64(lr0 * 0.9 * 0.9 * 0.9)
    for lr_t in (lr0, lr, 1.0e-3 * 0.9 ** 7):
        for t in (1, 2, 3, 255, 256, 1000, 3500):
            state.seed(t - 1, lr_t)
            state.advance(types_tensor([0], device), 1)
            s = state.read()
            want = host_bias_corrections(lr_t, t)
            assert s.t == t and bits64(s.lr) == bits64(lr_t)
            assert bits32(s.step_size) == bits32(want[0]), (t, lr_t, s.step_size, want[0])
            assert bits32(s.bc2_sqrt) == bits32(want[1]), (t, lr_t, s.bc2_sqrt, want[1])


# ------------------------------------------------------------------------------------------------ the log kernel
def check_log_rows(device):
    """One row per call: the means follow the pair's TYPE (within scene composes every term, across scene / different object
    the loss and the blind term, an empty pair none), added in pair order in double."""
    state = make_state(device, lr=0.25, rows=1)          # (one row allocated: the second call grows the buffer on the device)
    g = torch.Generator().manual_seed(5)
    terms = torch.rand(4, 5, generator=g).to(device)
    loss = torch.tensor([0.375], device=device)
    types = types_tensor([-1, 2, 0, 3], device)
    state.advance(types, 7)
    state.log(7, loss, terms, types)
    empty = types_tensor([-1, -1, -1, -1], device)
    state.advance(empty, 8)
    state.log(8, loss, terms, empty)
    h = state.read().history
    assert h.shape == (2, 16)
    t = terms.cpu().numpy()
    want = [7.0, 1.0, 0.25, 3.0, 0.375]
    for k in range(5):
        rows = [1, 2, 3] if k in (0, 4) else [2, 3]
        s = 0.0
        for p in rows:
            s += float(t[p, k])
        want += [s / len(rows), float(len(rows))]
    want.append(2.0)
    assert h[0].tolist() == want, (h[0].tolist(), want)
    assert h[1].tolist() == [8.0, 0.0, 0.25, 0.0, 0.375] + [0.0] * 10 + [-1.0]


# ------------------------------------------------------------------------------------------------ T4 / T6: the whole loop
def training_config(steps_between_decay=2, within_only=True, attempts=10000, non_matches=150, cross=10000, **training):
    probs = {"SINGLE_OBJECT_WITHIN_SCENE": 1.0 if within_only else 2.0, "SINGLE_OBJECT_ACROSS_SCENE": 0.0 if within_only else 1.0,
             "DIFFERENT_OBJECT": 0.0 if within_only else 1.0, "MULTI_OBJECT": 0.0, "SYNTHETIC_MULTI_OBJECT": 0.0}
    t = {"num_matching_attempts": attempts, "sample_matches_only_off_mask": True, "num_non_matches_per_match": non_matches,
         "fraction_masked_non_matches": 0.5, "fraction_background_non_matches": 0.5, "cross_scene_num_samples": cross,
         "use_image_b_mask_inv": True, "domain_randomize": False, "data_type_probabilities": probs,
         "learning_rate": 1.0e-4, "learning_rate_decay": 0.9, "steps_between_learning_rate_decay": steps_between_decay,
         "weight_decay": 1.0e-4, "num_iterations": 8, "batch_size": 1, "logging_rate": 100, "save_rate": 1000}
    t.update(training)
    return {"training": t}


def still_store(device, h, w):
    """One object, two scenes, every frame at the same pose: no image b is ever far enough from image a, every pair is empty."""
    from dcn_hip import frames
    F = 8
    g = torch.Generator().manual_seed(2)
    rgb = torch.randint(0, 256, (F, h, w, 3), dtype=torch.uint8, generator=g).to(device)
    depth = torch.full((F, h, w), 900, dtype=torch.int16).to(device)
    mask = torch.zeros((F, h, w), dtype=torch.uint8)
    mask[:, h // 4:3 * h // 4, w // 6:5 * w // 6] = 1
    return frames.FrameStore.from_tensors(rgb, depth, mask.to(device), np.stack([np.eye(4)] * F), [0, 4, 8], [0, 0])


def draws(store, cfg, B, seed, n):
    """The per-pair device types of n consecutive draws with this seed (drawing only)."""
    from dcn_hip import frames
    g = torch.Generator(device=store.device).manual_seed(seed)
    host = np.random.RandomState(seed)
    return [frames.draw_training_batch(store, B, cfg, generator=g, host_rng=host, per_pair_types=True)[0].type.tolist()
            for _ in range(n)]


def wanted_pattern(types_per_iteration, period=2, max_empty=4, mixed=False):
    empty = [all(t == -1 for t in ts) for ts in types_per_iteration]
    on = [e for it, e in enumerate(empty, 1) if it % period == 0]
    ok = any(on) and not all(on) and sum(empty) <= max_empty
    if mixed:   # at least two data types among the pairs that count
        ok = ok and len(set(t for ts in types_per_iteration for t in ts if t >= 0)) >= 2
    return ok


def find_seed(store, cfg, B, n=8, period=2, mixed=False, accept=None):
    for seed in range(64):
        ts = draws(store, cfg, B, seed, n)
        if wanted_pattern(ts, period, mixed=mixed) and (accept is None or accept(ts)):
            return seed
    raise AssertionError("no seed gave an empty and an active iteration on a multiple of %d with at most 4 empties" % period)


def host_logging_calls(loss, terms, types):
    """What the plain loop logs with .item() calls for one active iteration: the dict appends of update_plots
    (training.py:353-413), a term being there when a pair's type composes it; at B = 1 the values are the .item() of the
    reference's five returns, for larger batches the mean over the composing pairs in pair order."""
    full = {WITHIN, 3, 4}
    out = [("learning_rate", None)]
    for k, key in ((1, "match_loss"), (2, "masked_non_match_loss"), (3, "background_non_match_loss")):
        vals = [terms[p, k].item() for p, t in enumerate(types) if t in full]
        if vals:
            s = 0.0
            for v in vals:
                s += v
            out.append((key, s / len(vals)))
    return out


def oracle_loop(dcn, pcl, store, cfg, B, seed, n, stop_after_first_empty=False, guard=True):
    """The plain loop.  ``guard``: read the types on the host and ``continue`` on an all-empty batch before anything else (the
    oracle); without it this is the loop INTEGRATION.md prints under "Drawing batches from a frame store" with the schedule
    applied on the host to every iteration."""
    from dcn_hip import frames
    from dcn_hip.optim import Adam
    from dcn_hip.train import empty_logging_dict
    from dense_correspondence.loss_functions import loss_composer
    t = cfg["training"]
    opt = Adam(dcn.parameters(), lr=float(t["learning_rate"]), weight_decay=float(t["weight_decay"]))
    g = torch.Generator(device=store.device).manual_seed(seed)
    host = np.random.RandomState(seed)
    log = empty_logging_dict()
    empties, before_first_empty = [], None
    dcn.train()
    for it in range(1, n + 1):
        sb, _, _ = frames.draw_training_batch(store, B, cfg, generator=g, host_rng=host, per_pair_types=True)
        types = sb.type.tolist()
        empty = all(x == -1 for x in types)
        empties.append(empty)
        if empty and before_first_empty is None:
            before_first_empty = [p.detach().clone() for p in dcn.parameters()]
        if empty and guard:
            if stop_after_first_empty:
                break
            continue
        opt.zero_grad()
        if it % int(t["steps_between_learning_rate_decay"]) == 0:
            for group in opt.param_groups:
                group["lr"] = group["lr"] * t["learning_rate_decay"]
        ya, yb = dcn.forward_pair(sb.input_a, sb.input_b)
        loss, terms, _, _ = loss_composer.get_loss_mixed(pcl, dcn.process_network_output(ya, B),
                                                         dcn.process_network_output(yb, B), sb.device_lists())
        loss.backward()
        opt.step()
        if not empty:
            for key, value in host_logging_calls(loss, terms, types):
                # (the reference's own rule, is_zero_loss: a value below 1e-20 is not logged -- the same decision here)
                assert value is None or B > 1 or not value < 1e-20, (it, key, value)
                log["train"][key].append(opt.param_groups[0]["lr"] if value is None else value)
        if empty and stop_after_first_empty:
            break
    return {"opt": opt, "log": log, "empties": empties, "before_first_empty": before_first_empty,
            "lr": opt.param_groups[0]["lr"]}


def check_whole_loop(make_dcn, pcl, store, cfg, B, n=8, mixed=False):
    """Trainer against the host-reading oracle loop after n iterations, bit for bit: parameters, batch-norm buffers, moments,
    step and learning rate; the logging dict; and, as the documented negative, the unguarded loop on the same draws leaves the
    oracle's parameters at the first empty iteration."""
    from dcn_hip.train import StoreTrainer
    period = int(cfg["training"]["steps_between_learning_rate_decay"])
    seed = find_seed(store, cfg, B, n, period, mixed=mixed)
    # ---- the oracle, and the three facts about its own run
    dcn_o = make_dcn()
    o = oracle_loop(dcn_o, pcl, store, cfg, B, seed, n)
    on = [e for it, e in enumerate(o["empties"], 1) if it % period == 0]
    assert any(on), "an all-empty iteration on a multiple of the decay period"
    assert not all(on), "an active iteration on a multiple of the decay period"
    assert sum(o["empties"]) <= 4, "at most 4 empties"
    # ---- the trainer
    dcn_t = make_dcn()
    tr = StoreTrainer(dcn_t, pcl, store, cfg, generator=torch.Generator(device=store.device).manual_seed(seed),
                      host_rng=np.random.RandomState(seed), batch_size=B)
    for it in range(1, n + 1):
        tr.iteration(it)
    snap = tr.read_log()
    assert snap.num_active == n - sum(o["empties"]) and snap.num_skipped == sum(o["empties"])
    assert [bool(r[1] == 0) for r in snap.history] == o["empties"]
    for (k, a), b in zip(dcn_t.named_parameters(), dcn_o.parameters()):
        assert same_bits(a, b), k
    for (k, a), b in zip(dcn_t.named_buffers(), dcn_o.buffers()):
        assert torch.equal(a, b), k
    sd = tr.optimizer.state_dict()
    for a, b in zip(dcn_t.parameters(), dcn_o.parameters()):
        sa, so = tr.optimizer.state[a], o["opt"].state[b]
        assert same_bits(sa["exp_avg"], so["exp_avg"]) and same_bits(sa["exp_avg_sq"], so["exp_avg_sq"])
        assert float(sa["step"]) == float(so["step"]) == n - sum(o["empties"])
    assert bits64(sd["param_groups"][0]["lr"]) == bits64(o["lr"]) == bits64(snap.lr)
    assert tr.logging_dict == o["log"], (tr.logging_dict, o["log"])
    assert len(o["log"]["train"]["learning_rate"]) == n - sum(o["empties"])
    # ---- the negative: without the guard, the first empty iteration moves the parameters
    dcn_n = make_dcn()
    neg = oracle_loop(dcn_n, pcl, store, cfg, B, seed, n, stop_after_first_empty=True, guard=False)
    # (identical up to that iteration; the oracle skips it, so its parameters behind it are those in front of it)
    assert all(same_bits(a, b) for a, b in zip(neg["before_first_empty"], o["before_first_empty"]))
    assert any(not same_bits(a, b) for a, b in zip(dcn_n.parameters(), o["before_first_empty"]))
    return tr, o


def check_save_point(make_dcn, pcl, store, cfg, B, tmp_path, load_dcn, expect_match_loss=False):
    """save_rate 2, a run whose iteration 2 is inactive and iteration 4 active: no 000002.pth; 000004.pth, .pth.opt and the two
    yaml files; a network loaded from the folder with a torch.optim.Adam loaded from the .opt file reproduces the trainer's
    next step bit for bit."""
    import os
    import yaml
    from dcn_hip.optim import GuardedAdam
    from dcn_hip.train import StoreTrainer
    cfg = {"training": dict(cfg["training"], save_rate=2, num_iterations=3, steps_between_learning_rate_decay=2)}
    pattern = lambda ts: all(t == -1 for t in ts[1]) and not all(t == -1 for t in ts[3])
    seed = find_seed(store, cfg, B, 4, 2, accept=pattern)
    dcn = make_dcn()
    cfg["dense_correspondence_network"] = dict(dcn.config)
    folder = str(tmp_path / "run")
    tr = StoreTrainer(dcn, pcl, store, cfg, generator=torch.Generator(device=store.device).manual_seed(seed),
                      host_rng=np.random.RandomState(seed), batch_size=B, logging_dir=folder)
    log = tr.run()                             # 3 + 0 iterations, `>`: ends at iteration 4, the first active one past 3
    files = sorted(os.listdir(folder))
    assert "000002.pth" not in files and "000002.pth.opt" not in files, files
    for f in ("000004.pth", "000004.pth.opt", "000004_log_history.yaml", "loss.yaml", "training.yaml"):
        assert f in files, (f, files)
    snap = tr.state.read()
    assert int(snap.history[-1][0]) == 4 and snap.history[1][1] == 0 and snap.history[3][1] == 1
    with open(os.path.join(folder, "000004_log_history.yaml")) as f:
        assert yaml.safe_load(f) == log
    assert len(log["train"]["learning_rate"]) == snap.num_active
    if expect_match_loss:                      # within-scene pairs: every active iteration logs its match loss
        assert len(log["train"]["match_loss"]) == len(log["train"]["background_non_match_loss"]) == snap.num_active > 0
        assert all(v > 0 for v in log["train"]["match_loss"])
    rows = open(os.path.join(folder, "tensorboard", "scalars.tsv")).read().strip().split("\n")
    steps = [int(r.split("\t")[0]) for r in rows]
    assert steps == sorted(steps) and 2 not in steps and 4 in steps
    # ---- the restored pair takes the trainer's next step
    loaded = load_dcn(folder)
    t_opt = torch.optim.Adam(loaded.parameters(), lr=1.0, weight_decay=0.5)
    t_opt.load_state_dict(torch.load(os.path.join(folder, "000004.pth.opt")))
    assert t_opt.param_groups[0]["lr"] == snap.lr and t_opt.param_groups[0]["weight_decay"] == 1.0e-4
    opt2 = GuardedAdam(loaded.parameters(), lr=1.0)
    opt2.load_state_dict(t_opt.state_dict())
    tr2 = StoreTrainer(loaded, pcl, store, cfg, optimizer=opt2, batch_size=B)
    sb = tr.last[3]
    # (iteration 5 is no decay boundary; the same batch for both: an active one, the trainer's latest)
    tr.step_on_batch(sb, 5)
    tr2.step_on_batch(sb, 5)
    for (k, a), b in zip(dcn.named_parameters(), loaded.parameters()):
        assert same_bits(a, b), k
    for (k, a), b in zip(dcn.named_buffers(), loaded.buffers()):
        assert torch.equal(a, b), k
    s1, s2 = tr.state.read(), tr2.state.read()
    assert s1.t == s2.t == snap.t + 1 and bits64(s1.lr) == bits64(s2.lr)
