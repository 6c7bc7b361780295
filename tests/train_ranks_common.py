"""Shared by tests/test_emu_train_ranks.py and tests/test_gpu_train_ranks.py (not a test module): the checks of the
data-parallel ``StoreTrainer`` (dcn_train_advance_ranks, dcn_train_log_ranks, ``FlatGradients(reduce="sum")``,
``gather_ranks``, ``StoreTrainer(gradients=...)``) on whichever library the caller has loaded.

Yardsticks: ``dcn_train_advance`` / ``dcn_train_log`` on the flattened global batch for the two kernels, numpy for the rank
weight, and for the whole loop a loop that reads the types on the host after every draw, gathers the counts as Python objects,
``continue``s when no rank has a pair, decays the learning rate on the host and scales its loss with ``np.float32(n_r / N)``."""
import os
import queue
import socket
import time

import numpy as np
import torch

import train_common as tc

PATTERN = (0, -1, 2, 1, -1, 3, 4, 0, 1, -1, -1, 2)


# ------------------------------------------------------------------------------------------------ T1, T2: the two kernels
def type_tables():
    """(G, B, [G][B] types): for every G in {1, 2, 3, 8} and B in {1, 2, 4} a mixed table (empty and non-empty pairs of every
    type, unequal counts per rank), the all-empty table and the table where only the last rank has a pair."""
    out = []
    for G in (1, 2, 3, 8):
        for B in (1, 2, 4):
            mixed = [[PATTERN[(3 * r + 5 * p + r * p) % len(PATTERN)] for p in range(B)] for r in range(G)]
            if all(t == -1 for row in mixed for t in row):
                mixed[0][0] = 2
            empty = [[-1] * B for _ in range(G)]
            last = [[-1] * B for _ in range(G)]
            last[G - 1][B - 1] = 1
            out += [(G, B, mixed), (G, B, empty), (G, B, last)]
    return out


def check_advance_ranks(device):
    """Every rank's state after dcn_train_advance_ranks equals, word for word, the state after dcn_train_advance on the
    flattened types, over four consecutive iterations of which the second is all-empty ON a decay boundary and the fourth is
    the table again on the next boundary; the weight is numpy's float32(float64(n_r) / float64(N)), 0 where n_r or N is 0."""
    saw_zero_n, saw_zero_N, saw_fraction = False, False, False
    for G, B, table in type_tables():
        empty = [[-1] * B for _ in range(G)]
        ref = tc.make_state(device, lr=1.0e-4, every=2, decay=0.9)
        states = [tc.make_state(device, lr=1.0e-4, every=2, decay=0.9) for _ in range(G)]
        weight = torch.full((1,), -7.0, device=device)
        for it, tab in enumerate((table, empty, table, table), 1):
            flat = [t for row in tab for t in row]
            ref.advance(tc.types_tensor(flat, device), it)
            types_all = tc.types_tensor(tab, device)
            counts = [sum(t != -1 for t in row) for row in tab]
            N = sum(counts)
            for r in range(G):
                weight.fill_(-7.0)
                states[r].advance_ranks(types_all, r, weight, it)
                assert torch.equal(states[r].buf[:6], ref.buf[:6]), (G, B, it, r)
                want = np.float32(np.float64(counts[r]) / np.float64(N)) if N > 0 else np.float32(0.0)
                assert tc.bits32(weight.item()) == tc.bits32(want), (G, B, it, r, weight.item(), want)
                if N == 0:
                    saw_zero_N = True
                    assert weight.item() == 0.0
                elif counts[r] == 0:
                    saw_zero_n = True
                    assert weight.item() == 0.0
                elif 0 < counts[r] < N and (N & (N - 1)):
                    saw_fraction = True
        snap = ref.read()
        assert snap.num_active + snap.num_skipped == 4 and snap.num_skipped >= 1
    assert saw_zero_n and saw_zero_N and saw_fraction


def check_advance_ranks_refusals(device):
    import ctypes
    from dcn_hip import _lib
    state = tc.make_state(device)
    types_all = tc.types_tensor([[0, -1], [1, 2]], device)
    w = torch.zeros(1, device=device)
    lib, sp = _lib.get(), ctypes.c_void_p(state.state_ptr())
    call = lambda G, B, rank, every=1: lib.dcn_train_advance_ranks(sp, _lib.ptr(types_all), G, B, rank, _lib.ptr(w), 1, every,
                                                                   0.9, 0.9, 0.999, _lib.stream_ptr())
    assert call(2, 2, 0) == 0
    assert call(0, 2, 0) == -1 and call(2, 0, 0) == -1 and call(2, 2, 2) == -1 and call(2, 2, -1) == -1
    assert call(2, 2, 0, every=0) == -1 and call(65536, 65536, 0) == -1
    assert lib.dcn_train_advance_ranks(sp, _lib.ptr(types_all), 2, 2, 0, None, 1, 1, 0.9, 0.9, 0.999, _lib.stream_ptr()) == -1
    hist = ctypes.c_void_p(state._history_ptr())
    g = torch.zeros(2, 11, device=device)
    assert lib.dcn_train_log_ranks(hist, 0, 1, sp, _lib.ptr(g), _lib.ptr(types_all), 2, 2, _lib.stream_ptr()) == 0
    assert lib.dcn_train_log_ranks(hist, 0, 1, sp, None, _lib.ptr(types_all), 2, 2, _lib.stream_ptr()) == -1
    assert lib.dcn_train_log_ranks(hist, -1, 1, sp, _lib.ptr(g), _lib.ptr(types_all), 2, 2, _lib.stream_ptr()) == -1
    assert lib.dcn_train_log_ranks(hist, 0, 1, sp, _lib.ptr(g), _lib.ptr(types_all), 0, 2, _lib.stream_ptr()) == -1
    with_np = torch.zeros(2, 2, dtype=torch.int64, device=device)
    try:
        state.advance_ranks(with_np, 0, w, 1)
        raise AssertionError("int64 types accepted")
    except TypeError:
        pass


def check_log_ranks(device):
    """dcn_train_log_ranks on [G][1 + 5 B] rows against dcn_train_log on the flattened terms and types: every column but the
    fourth is the same double; the fourth is the sum of the weighted losses added in rank order in double."""
    g = torch.Generator().manual_seed(9)
    for G, B, table in type_tables():
        terms = torch.rand(G, B, 5, generator=g)
        losses = torch.rand(G, generator=g) * 3.0
        gathered = torch.cat([losses.reshape(G, 1), terms.reshape(G, 5 * B)], dim=1).contiguous().to(device)
        types_all = tc.types_tensor(table, device)
        a, b = tc.make_state(device, lr=0.25, rows=1), tc.make_state(device, lr=0.25, rows=1)
        w = torch.zeros(1, device=device)
        for it in (5, 6):                                # (the second row grows the buffer on the device)
            a.advance_ranks(types_all, G - 1, w, it)
            b.advance(types_all.reshape(-1), it)
            a.log_ranks(it, gathered, types_all)
            b.log(it, torch.tensor([123.0], device=device), terms.reshape(G * B, 5).contiguous().to(device),
                  types_all.reshape(-1))
        ha, hb = a.read().history, b.read().history
        assert ha.shape == hb.shape == (2, 16)
        cols = [c for c in range(16) if c != 4]
        assert ha[:, cols].tobytes() == hb[:, cols].tobytes(), (G, B, ha, hb)
        want = 0.0
        for r in range(G):
            want += float(losses[r])
        assert tc.bits64(ha[0, 4]) == tc.bits64(ha[1, 4]) == tc.bits64(want), (G, B, ha[0, 4], want)
        flat = [t for row in table for t in row]
        assert ha[0, 3] == sum(0 <= t < 5 for t in flat)
        assert ha[0, 15] == next((t for t in flat if t != -1), -1)


# ------------------------------------------------------------------------------------------------ seeds
def counts_of(store, cfg, B, seed, n):
    return [sum(t != -1 for t in ts) for ts in tc.draws(store, cfg, B, seed, n)]


def pattern_two_ranks(counts, B, period=2):
    """counts[rank][iteration - 1]: an all-empty iteration on a decay boundary and an active one on another, an iteration where
    one rank is empty and the other is not, one with unequal non-zero counts, and a full one."""
    its = list(zip(*counts))
    on = [sum(c) == 0 for it, c in enumerate(its, 1) if it % period == 0]
    return (any(on) and not all(on) and any(min(c) == 0 and max(c) > 0 for c in its)
            and any(0 < min(c) < max(c) for c in its) and any(min(c) == B for c in its))


def pattern_three_ranks(counts, B=1, period=2):
    """B = 1 on three ranks: totals of 1, 2 and 3 occur (weights 1, 1/2 and 1/3), and an active iteration on a boundary"""
    totals = [sum(c) for c in zip(*counts)]
    return {1, 2, 3} <= set(totals) and any(t > 0 for it, t in enumerate(totals, 1) if it % period == 0)


def find_seeds(store, cfg, B, world, n, accept, first):
    """``first`` if the counts drawn with it satisfy ``accept``, else the first of at most 64 further seed tuples that does
    (drawing only)."""
    cache = {}

    def counts(seed):
        if seed not in cache:
            cache[seed] = counts_of(store, cfg, B, seed, n)
        return cache[seed]
    tried = [tuple(first)]
    if world == 2:
        tried += [(a, 8 + b) for a in range(8) for b in range(8)]
    else:
        tried += [tuple(s + r for r in range(world)) for s in range(64)]
    for seeds in tried[:65]:
        if accept([counts(s) for s in seeds]):
            return seeds
    raise AssertionError("no seed tuple among %d gave the wanted pattern of empty and non-empty pairs" % len(tried[:65]))


# ------------------------------------------------------------------------------------------------ T3, T4: the whole loop
def flat_parameters(dcn):
    return torch.cat([p.detach().reshape(-1) for p in dcn.parameters()])


def global_log_appends(all_terms, all_types):
    """tc.host_logging_calls over the global batch in (rank, pair) order"""
    terms = torch.tensor([row for rank in all_terms for row in rank], dtype=torch.float32).reshape(-1, 5)
    return tc.host_logging_calls(None, terms, [t for rank in all_types for t in rank])


def oracle_ranks_loop(dcn, pcl, store, cfg, B, seed, n, bucketed):
    """The host-reading data-parallel loop of one rank.  Issues collectives of Python objects: every rank must run it."""
    import torch.distributed as dist
    from dcn_hip import frames
    from dcn_hip.distributed import FlatGradients
    from dcn_hip.optim import Adam
    from dcn_hip.train import empty_logging_dict
    from dense_correspondence.loss_functions import loss_composer
    t = cfg["training"]
    world = dist.get_world_size()
    grads = FlatGradients(dcn, reduce="sum", bucketed=bucketed)
    opt = grads.attach(Adam(dcn.parameters(), lr=float(t["learning_rate"]), weight_decay=float(t["weight_decay"])))
    g = torch.Generator(device=store.device).manual_seed(seed)
    host = np.random.RandomState(seed)
    log = empty_logging_dict()
    counts, active, weights = [], [], []
    dcn.train()
    for it in range(1, n + 1):
        sb, _, _ = frames.draw_training_batch(store, B, cfg, generator=g, host_rng=host, per_pair_types=True)
        types = sb.type.tolist()
        said = [None] * world
        dist.all_gather_object(said, types)
        per_rank = [sum(x != -1 for x in ts) for ts in said]
        n_r, N = per_rank[dist.get_rank()], sum(per_rank)
        counts.append(per_rank)
        active.append(N > 0)
        if N == 0:
            continue
        opt.zero_grad()
        if it % int(t["steps_between_learning_rate_decay"]) == 0:
            for group in opt.param_groups:
                group["lr"] = group["lr"] * t["learning_rate_decay"]
        ya, yb = dcn.forward_pair(sb.input_a, sb.input_b)
        loss, terms, _, _ = loss_composer.get_loss_mixed(pcl, dcn.process_network_output(ya, B),
                                                         dcn.process_network_output(yb, B), sb.device_lists())
        w = np.float32(np.float64(n_r) / np.float64(N))
        weights.append(float(w))
        (loss * float(w)).backward()
        grads.all_reduce_mean()
        opt.step()
        all_terms = [None] * world
        dist.all_gather_object(all_terms, terms.detach().cpu().tolist())
        for key, value in global_log_appends(all_terms, said):
            log["train"][key].append(opt.param_groups[0]["lr"] if value is None else value)
    return {"opt": opt, "log": log, "counts": counts, "active": active, "lr": opt.param_groups[0]["lr"], "weights": weights,
            "stats": dict(grads.stats)}


def make_ranks_trainer(dcn, pcl, store, cfg, B, seed, bucketed, single_rank_collectives=False):
    from dcn_hip.distributed import FlatGradients
    from dcn_hip.optim import GuardedAdam
    from dcn_hip.train import StoreTrainer
    t = cfg["training"]
    grads = FlatGradients(dcn, reduce="sum", bucketed=bucketed, single_rank_collectives=single_rank_collectives)
    opt = grads.attach(GuardedAdam(dcn.parameters(), lr=float(t["learning_rate"]), weight_decay=float(t["weight_decay"])))
    return StoreTrainer(dcn, pcl, store, cfg, optimizer=opt, gradients=grads, batch_size=B,
                        generator=torch.Generator(device=store.device).manual_seed(seed), host_rng=np.random.RandomState(seed))


def same_on_all_ranks(tensor):
    """-> True when every rank holds the bits of rank 0 (a collective: every rank calls it)"""
    import torch.distributed as dist
    mine = tensor.detach().contiguous().view(-1).view(torch.uint8).cpu() if tensor.dtype != torch.uint8 else tensor.cpu()
    said = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(said, mine)
    return all(bool(torch.equal(said[0], x)) for x in said[1:])


def whole_loop_on_rank(make_dcn, pcl, store, cfg, B, seed, n, trainer_bucketed, oracle_bucketed):
    """Trainer against oracle on this rank, bit for bit, and the ranks against each other -> what the parent asserts on."""
    dcn_o = make_dcn()
    o = oracle_ranks_loop(dcn_o, pcl, store, cfg, B, seed, n, oracle_bucketed)
    dcn_t = make_dcn()
    tr = make_ranks_trainer(dcn_t, pcl, store, cfg, B, seed, trainer_bucketed)
    for it in range(1, n + 1):
        tr.iteration(it)
    snap = tr.read_log()
    res = {"counts": o["counts"], "weights": o["weights"], "num_active": snap.num_active, "num_skipped": snap.num_skipped,
           "oracle_active": o["active"], "active_column": [bool(r[1] != 0) for r in snap.history],
           "trainer_stats": dict(tr.gradients.stats), "oracle_stats": o["stats"]}
    res["parameters"] = all(tc.same_bits(a, b) for a, b in zip(dcn_t.parameters(), dcn_o.parameters()))
    res["buffers"] = all(bool(torch.equal(a, b)) for a, b in zip(dcn_t.buffers(), dcn_o.buffers()))
    sd = tr.optimizer.state_dict()
    moments, steps = True, True
    for a, b in zip(dcn_t.parameters(), dcn_o.parameters()):
        sa, so = tr.optimizer.state[a], o["opt"].state[b]
        moments = moments and tc.same_bits(sa["exp_avg"], so["exp_avg"]) and tc.same_bits(sa["exp_avg_sq"], so["exp_avg_sq"])
        steps = steps and float(sa["step"]) == float(so["step"]) == sum(o["active"])
    res["moments"], res["steps"] = moments, steps
    res["lr"] = tc.bits64(sd["param_groups"][0]["lr"]) == tc.bits64(o["lr"]) == tc.bits64(snap.lr)
    res["logging_dict"] = tr.logging_dict == o["log"]
    res["logged"] = len(o["log"]["train"]["learning_rate"])
    res["loss_column"] = [float(r[4]) for r in snap.history]
    res["ranks_parameters"] = same_on_all_ranks(flat_parameters(dcn_t))
    res["ranks_moments"] = same_on_all_ranks(torch.cat([tr.optimizer.state[p][k].reshape(-1) for p in dcn_t.parameters()
                                                        for k in ("exp_avg", "exp_avg_sq")]))
    res["ranks_history"] = same_on_all_ranks(torch.from_numpy(snap.history.copy()))
    res["ranks_state"] = same_on_all_ranks(tr.state.buf[:6])
    return res


def assert_whole_loop(results, n, expect_bucketed=None):
    for rank, r in sorted(results.items()):
        for key in ("parameters", "buffers", "moments", "steps", "lr", "logging_dict", "ranks_parameters", "ranks_moments",
                    "ranks_history", "ranks_state"):
            assert r[key], (rank, key, r)
        assert r["active_column"] == r["oracle_active"], (rank, r)
        assert r["num_active"] == sum(r["oracle_active"]) and r["num_skipped"] == n - sum(r["oracle_active"]), (rank, r)
        assert r["logged"] == r["num_active"], (rank, r)
        if expect_bucketed is not None:
            t_b, o_b = expect_bucketed
            assert (r["trainer_stats"]["bucketed_steps"] > 0) == t_b and (r["trainer_stats"]["monolithic_steps"] > 0) != t_b, r
            assert (r["oracle_stats"]["bucketed_steps"] > 0) == o_b and (r["oracle_stats"]["monolithic_steps"] > 0) != o_b, r


# ------------------------------------------------------------------------------------------------ T5: an idle rank
def idle_rank_on_rank(make_dcn, pcl, store, still, cfg, still_cfg, B, seed, n, rank):
    """Rank 1 draws from ``still`` with ``still_cfg`` (within scene only: always empty; the same schedule and optimizer keys as
    ``cfg``).  Rank 0 compares itself with the single-process trainer on its draws."""
    from dcn_hip.train import StoreTrainer
    dcn = make_dcn()
    tr = make_ranks_trainer(dcn, pcl, store if rank == 0 else still, cfg if rank == 0 else still_cfg, B, seed, None)
    for it in range(1, n + 1):
        tr.iteration(it)
    snap = tr.read_log()
    res = {"ranks_parameters": same_on_all_ranks(flat_parameters(dcn)), "num_active": snap.num_active,
           "num_skipped": snap.num_skipped}
    if rank == 0:
        plain_dcn = make_dcn()
        plain = StoreTrainer(plain_dcn, pcl, store, cfg, batch_size=B,
                             generator=torch.Generator(device=store.device).manual_seed(seed),
                             host_rng=np.random.RandomState(seed))
        for it in range(1, n + 1):
            plain.iteration(it)
        ps = plain.read_log()
        res["parameters"] = all(bool(torch.equal(a, b)) for a, b in zip(dcn.parameters(), plain_dcn.parameters()))
        res["moments"] = all(bool(torch.equal(tr.optimizer.state[a][k], plain.optimizer.state[b][k]))
                             for a, b in zip(dcn.parameters(), plain_dcn.parameters()) for k in ("exp_avg", "exp_avg_sq"))
        res["history"] = bool(np.array_equal(snap.history[:, :15], ps.history[:, :15]))
        res["plain_active"] = ps.num_active
        res["moved"] = any(not bool(torch.equal(a, b)) for a, b in zip(make_dcn().parameters(), dcn.parameters()))
    return res


def assert_idle_rank(results, n):
    r0, r1 = results[0], results[1]
    assert r0["parameters"] and r0["moments"] and r0["history"], r0
    assert r0["ranks_parameters"] and r1["ranks_parameters"]
    assert r0["num_active"] == r1["num_active"] == r0["plain_active"] and 0 < r0["num_active"] and r0["moved"], (r0, r1)
    assert r0["num_active"] + r0["num_skipped"] == n


def run_on_rank(make_dcn, pcl, store, cfg, B, seed, rank, folder):
    """``run()`` with a save point at every iteration and ``num_iterations`` 2 on every rank, each with a folder of its own:
    -> the files this rank wrote and the iteration it stopped at."""
    cfg = {"training": dict(cfg["training"], save_rate=1, num_iterations=2)}
    dcn = make_dcn()
    cfg["dense_correspondence_network"] = dict(dcn.config)
    tr = make_ranks_trainer(dcn, pcl, store, cfg, B, seed, None)
    tr.logging_dir = folder
    tr.run()
    return {"files": sorted(os.listdir(folder)) if os.path.isdir(folder) else None, "stopped_at": int(tr.history[-1][0]),
            "active": [bool(r[1] != 0) for r in tr.history], "ranks_parameters": same_on_all_ranks(flat_parameters(dcn))}


def assert_run(results):
    r0, r1 = results[0], results[1]
    assert r1["files"] is None, r1                       # only save_rank (0) writes
    assert r0["stopped_at"] == r1["stopped_at"] >= 3 and r0["active"] == r1["active"] and r0["active"][-1], (r0, r1)
    assert r0["ranks_parameters"] and r1["ranks_parameters"]
    last = "%06d" % r0["stopped_at"]
    for f in ("000000.pth", last + ".pth", last + ".pth.opt", last + "_log_history.yaml", "loss.yaml", "training.yaml"):
        assert f in r0["files"], (f, r0["files"])
    for it, act in enumerate(r0["active"], 1):
        assert (("%06d.pth" % it) in r0["files"]) == act, (it, r0)


# ------------------------------------------------------------------------------------------------ T6: refusals, no group
def check_refusals(make_dcn, pcl, store, cfg):
    import pytest
    from dcn_hip.distributed import FlatGradients
    from dcn_hip.optim import GuardedAdam
    from dcn_hip.train import StoreTrainer
    with pytest.raises(ValueError, match="reduce"):
        FlatGradients(make_dcn(), reduce="average")
    dcn = make_dcn()
    g = FlatGradients(dcn)                               # reduce="mean"
    with pytest.raises(ValueError, match="reduce='sum'"):
        StoreTrainer(dcn, pcl, store, cfg, optimizer=g.attach(GuardedAdam(dcn.parameters(), lr=1e-4)), gradients=g)
    dcn, other = make_dcn(), make_dcn()
    g = FlatGradients(other, reduce="sum")
    with pytest.raises(ValueError, match="does not own"):
        StoreTrainer(dcn, pcl, store, cfg, optimizer=g.attach(GuardedAdam(dcn.parameters(), lr=1e-4)), gradients=g)
    dcn = make_dcn()
    g = FlatGradients(dcn, reduce="sum")
    with pytest.raises(ValueError, match="not attached"):
        StoreTrainer(dcn, pcl, store, cfg, optimizer=GuardedAdam(dcn.parameters(), lr=1e-4), gradients=g)
    with pytest.raises(TypeError, match="FlatGradients"):
        StoreTrainer(make_dcn(), pcl, store, cfg, gradients=object())
    # the present refusal stays for gradients the trainer was not given
    dcn = make_dcn()
    opt = FlatGradients(dcn, reduce="sum").attach(GuardedAdam(dcn.parameters(), lr=1e-4))
    with pytest.raises(NotImplementedError, match="distributed"):
        StoreTrainer(dcn, pcl, store, cfg, optimizer=opt)


def check_no_process_group_equals_plain(make_dcn, pcl, store, cfg, B, n, monkeypatch):
    """Without a process group the ``gradients=`` trainer is the plain one, value for value, and issues no collective."""
    import torch.distributed as dist
    from dcn_hip.train import StoreTrainer
    assert not dist.is_initialized()

    def refuse(*a, **k):
        raise AssertionError("a collective was issued without a process group")
    for name in ("all_gather", "all_gather_into_tensor", "all_reduce", "all_gather_object", "broadcast"):
        monkeypatch.setattr(dist, name, refuse)
    seed = tc.find_seed(store, cfg, B, n, 2)
    dcn_a, dcn_b = make_dcn(), make_dcn()
    a = make_ranks_trainer(dcn_a, pcl, store, cfg, B, seed, None)
    b = StoreTrainer(dcn_b, pcl, store, cfg, batch_size=B, generator=torch.Generator(device=store.device).manual_seed(seed),
                     host_rng=np.random.RandomState(seed))
    for it in range(1, n + 1):
        a.iteration(it)
        b.iteration(it)
    sa, sb = a.read_log(), b.read_log()
    assert a.world == 1 and a.rank == 0
    assert 0 < sa.num_active == sb.num_active < n and sa.t == sb.t and tc.bits64(sa.lr) == tc.bits64(sb.lr)
    assert np.array_equal(sa.history, sb.history), (sa.history, sb.history)
    for (k, x), y in zip(dcn_a.named_parameters(), dcn_b.parameters()):
        assert torch.equal(x, y), k
        for m in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a.optimizer.state[x][m], b.optimizer.state[y][m]), (k, m)
    for (k, x), y in zip(dcn_a.named_buffers(), dcn_b.buffers()):
        assert torch.equal(x, y), k
    assert a.logging_dict == b.logging_dict
    assert a.gradients.stats["bucket_collectives"] == 0 and a.gradients.stats["monolithic_steps"] == 0


def check_gather_ranks_without_group(device):
    from dcn_hip.distributed import gather_ranks
    x = torch.arange(6, dtype=torch.int32, device=device).reshape(2, 3)
    out = gather_ranks(x)
    assert out.shape == (1, 2, 3) and torch.equal(out[0], x) and out.data_ptr() != x.data_ptr()
    out, work = gather_ranks(x, async_op=True)
    work.wait()
    assert torch.equal(out[0], x)


# ------------------------------------------------------------------------------------------------ the parents' side
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def init_worker(rank, world, port, backend, device_id=None):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if device_id is not None:
        dist.init_process_group(backend, rank=rank, world_size=world, device_id=device_id)
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)


def run_workers(target, world, args, limit):
    """Spawn ``world`` (<= 4) processes ``target(rank, world, port, queue, *args)``, each with ``limit`` seconds, and collect
    one ``(rank, result)`` from each.  The exit codes are polled: after the first worker that died or ran out of time the others
    are ended and the test fails at once -- nothing further is started and nothing is retried."""
    import pytest
    import torch.multiprocessing as mp
    assert 1 <= world <= 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    deadline = []
    for p in procs:
        p.start()
        deadline.append(time.monotonic() + limit)
    results, failed = {}, None
    while len(results) < world and failed is None:
        try:
            rank, res = q.get(timeout=0.25)
            results[rank] = res
            continue
        except queue.Empty:
            pass
        for r, p in enumerate(procs):
            if r in results:
                continue
            if p.exitcode is not None:                   # ended without a result (whatever the code), or died
                try:
                    while True:
                        rank, res = q.get(timeout=0.5)
                        results[rank] = res
                except queue.Empty:
                    pass
                if r not in results:
                    failed = "rank %d ended with exit code %s and no result" % (r, p.exitcode)
                    break
            elif time.monotonic() > deadline[r]:
                failed = "rank %d did not finish within %d s" % (r, limit)
                break
    if failed is not None:
        for p in procs:
            if p.exitcode is None:
                p.kill()
        for p in procs:
            p.join(10)
        pytest.fail(failed)
    for r, p in enumerate(procs):
        p.join(max(1.0, deadline[r] - time.monotonic()))
        if p.exitcode is None:
            p.kill()
            p.join(10)
            pytest.fail("rank %d did not exit" % r)
        assert p.exitcode == 0, (r, p.exitcode)
    return results
