"""The engine's stream schedule, read from the host emulation's call log (tests/hostemu/hipemu_runtime.cpp: one line per kernel
launch, event record and stream wait).  Real execution at 64 x 64, base width 8; the kernels' results are checked elsewhere --
here only WHAT was enqueued WHERE, and which event orders it.  Stream 0 is the caller's; the only other one is the plan's side
stream (forward: weight images next to the stem; backward: weight-gradient GEMMs next to the dgrad / batch-norm chain)."""
import re

import pytest
import torch

from helpers import CallLog, use_emulation_library


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_emulation_library()


_LAUNCH = re.compile(r"^launch (.*) grid=\((\d+),(\d+),(\d+)\) block=\((\d+),(\d+),(\d+)\) stream=(\d+)$")
_EVENT = re.compile(r"^(record|wait) stream=(\d+) event=(\d+)$")


def _parse(lines):
    """-> [("launch", kernel, stream) | ("record", event, stream) | ("wait", event, stream)]"""
    out = []
    for ln in lines:
        m = _LAUNCH.match(ln)
        if m:
            out.append(("launch", m.group(1), int(m.group(8))))
            continue
        m = _EVENT.match(ln)
        assert m, ln
        out.append((m.group(1), int(m.group(3)), int(m.group(2))))
    return out


_RUNS = {}


def _run(dcn_env, arch, groups, overlap):
    """One training round on a fresh plan -> {"forward": [entries of each engine call], "backward": [...], "buckets": [the
    event of bucket 0, 1, ... of each backward call's plan]}.  Computed once per configuration and shared."""
    key = (arch, groups, overlap)
    if key in _RUNS:
        return _RUNS[key]
    from dcn_hip import _lib, backbone
    from pytorch_segmentation_detection.models import resnet_dilated as prod
    dcn_env(DCN_BACKWARD_OVERLAP=overlap)
    backbone._PLANS.clear()   # (a plan decides once whether it has a side stream)
    backbone.set_conv_mode("f16x3")
    try:
        m = getattr(prod, arch)(num_classes=3, base_width=8)
        m.train()
        g = torch.Generator().manual_seed(3)
        xa, xb = torch.randn(1, 3, 64, 64, generator=g), torch.randn(1, 3, 64, 64, generator=g)
        run = {"forward": [], "backward": [], "buckets": []}
        with CallLog(_lib.get()) as log:
            def call(kind, fn):
                n = len(log.lines())
                r = fn()
                run[kind].append(_parse(log.lines()[n:]))
                return r
            if groups == 2:
                ys = call("forward", lambda: m.forward_pair(xa, xb))
                assert m._last_plan.groups == 2
                call("backward", lambda: (ys[0].sum() + ys[1].sum()).backward())
            else:
                y = call("forward", lambda: m(xa))
                call("backward", lambda: y.sum().backward())
            plan = m._last_plan
            for k in range(len(plan.grad_buckets)):   # which event belongs to bucket k: make stream 0 wait on it
                n = len(log.lines())
                plan.stream_wait_grad_bucket(k, None)
                (entry,) = _parse(log.lines()[n:])
                assert entry[0] == "wait" and entry[2] == 0
                run["buckets"].append(entry[1])
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    finally:
        backbone.set_conv_mode(None)
        backbone._PLANS.clear()
    _RUNS[key] = run
    return run


CONFIGS = [(arch, groups, overlap) for arch in ("Resnet18_8s", "Resnet50_8s") for groups in (1, 2) for overlap in (1, 0)]
configs = pytest.mark.parametrize("arch,groups,overlap", CONFIGS)


def _calls(run):
    return run["forward"] + run["backward"]


def _streams(entries):
    return {e[2] for e in entries}


def _is_bn_bwd_apply(entries, i):
    """The batch-norm backward's apply launch.  Names are the text at the launch site (csrc/elementwise_kernels.hip,
    launch_bn_bwd): the unblocked pass is launched by name; the finalize pass and the blocked apply pass -- the one that writes
    the gradient images -- each through a local `kernel`, one right after the other on the same stream."""
    kind, name, stream = entries[i]
    if kind != "launch":
        return False
    if name == "bn_bwd_apply_kernel":
        return True
    before = [e for e in entries[:i] if e[0] == "launch" and e[2] == stream]
    return name == "kernel" and bool(before) and before[-1][1] == "kernel"


@configs
def test_no_wait_on_an_event_not_recorded_in_the_call(dcn_env, arch, groups, overlap):
    run = _run(dcn_env, arch, groups, overlap)
    for entries in _calls(run):
        recorded = set()
        for kind, what, stream in entries:
            if kind == "record":
                recorded.add(what)
            elif kind == "wait":
                assert what in recorded, (what, stream)
        if not overlap:
            assert _streams(entries) == {0}
    if overlap:   # (the schedule under test is there at all)
        assert all(_streams(entries) == {0, 1} for entries in run["backward"])


@configs
def test_side_stream_is_joined_before_the_call_returns(dcn_env, arch, groups, overlap):
    """Every stream but the caller's that was given a launch has, after its last launch, an event record that the caller's
    stream waits on later in the call."""
    run = _run(dcn_env, arch, groups, overlap)
    for entries in _calls(run):
        if not overlap:
            assert _streams(entries) == {0}
        for s in _streams(entries) - {0}:
            launches = [i for i, e in enumerate(entries) if e[0] == "launch" and e[2] == s]
            if not launches:
                continue
            joined = False
            for j in range(launches[-1] + 1, len(entries)):
                if entries[j][0] == "record" and entries[j][2] == s:
                    joined = joined or any(e == ("wait", entries[j][1], 0) for e in entries[j + 1:])
            assert joined, s


@configs
def test_slot_is_not_rewritten_before_its_reader_is_waited_for(dcn_env, arch, groups, overlap):
    """The two gradient-image slots alternate, so the batch-norm backward apply launches two apart write the same slot.  The
    side-stream launches between an apply launch and the next one are the readers of what it wrote (the weight-gradient GEMM of
    that gradient; the launches after the next apply read the OTHER slot): before the slot is written again, stream 0 waits on
    an event recorded on the side stream after every one of them."""
    run = _run(dcn_env, arch, groups, overlap)
    for entries in run["backward"]:
        if not overlap:
            assert _streams(entries) == {0}
            continue
        applies = [i for i in range(len(entries)) if entries[i][2] == 0 and _is_bn_bwd_apply(entries, i)]
        assert len(applies) > 4
        checked = 0
        for a, b, c in zip(applies, applies[1:], applies[2:]):
            readers = [i for i in range(a + 1, b) if entries[i][0] == "launch" and entries[i][2] != 0]
            if not readers:
                continue
            ok = False
            for w in range(readers[-1] + 1, c):
                if entries[w][0] != "wait" or entries[w][2] != 0:
                    continue
                records = [i for i in range(w) if entries[i][0] == "record" and entries[i][1] == entries[w][1]]
                ok = ok or (bool(records) and entries[records[-1]][2] != 0 and records[-1] > readers[-1])
            assert ok, (a, b, c)
            checked += 1
        assert checked > 4


@configs
def test_bucket_events_once_in_order_behind_a_join(dcn_env, arch, groups, overlap):
    """Each gradient bucket's event is recorded exactly once per backward call, in bucket order, on the caller's stream, and
    nothing was given to the side stream between the last join and that record."""
    run = _run(dcn_env, arch, groups, overlap)
    (entries,) = run["backward"]
    buckets = run["buckets"]
    assert len(buckets) == 3 and len(set(buckets)) == 3
    records = [i for i, e in enumerate(entries) if e[0] == "record" and e[1] in buckets]
    assert [entries[i][1] for i in records] == buckets
    assert all(entries[i][2] == 0 for i in records)
    if not overlap:
        assert _streams(entries) == {0}
        return
    for i in records:
        side = [j for j in range(i) if entries[j][2] != 0 and entries[j][0] in ("launch", "record")]
        assert side and entries[side[-1]][0] == "record"                      # the side stream's last act: the join's record
        assert ("wait", entries[side[-1]][1], 0) in entries[side[-1] + 1:i]   # ... which stream 0 waited on before the bucket's


def test_refused_backward_call_still_joins_the_side_stream(dcn_env, monkeypatch):
    """An error return after the side stream was given work: a null gradient pointer for a trunk convolution's weight is refused
    by that layer's weight-gradient launcher (DCN_E_INVALID before anything is launched), behind the side stream's wait.  The
    caller's stream must still be made to wait for the side stream: the call's log ends with the join."""
    from dcn_hip import _lib, backbone
    from pytorch_segmentation_detection.models import resnet_dilated as prod
    dcn_env(DCN_BACKWARD_OVERLAP=1)
    backbone._PLANS.clear()
    backbone.set_conv_mode("f16x3")
    try:
        m = prod.Resnet18_8s(num_classes=3, base_width=8)
        m.train()
        y = m(torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3)))
        lib = _lib.get()
        victim = m._last_plan.param_names.index("layer4.1.conv2.weight")
        real = lib.dcn_backbone_backward

        def refused(plan, g, params, saved, ws, grads, normalize, stream):
            grads[victim] = None
            return real(plan, g, params, saved, ws, grads, normalize, stream)
        monkeypatch.setattr(lib, "dcn_backbone_backward", refused)
        with CallLog(lib) as log:
            with pytest.raises(RuntimeError, match="DCN_E_INVALID"):
                y.sum().backward()
            entries = _parse(log.lines())
        assert any(e[0] == "wait" and e[2] == 1 for e in entries)              # the side stream was engaged ...
        assert not any(e[0] == "launch" and e[2] == 1 for e in entries)        # ... and the refused launcher launched nothing
        (kind_r, ev_r, st_r), (kind_w, ev_w, st_w) = entries[-2:]
        assert (kind_r, st_r) == ("record", 1) and (kind_w, ev_w, st_w) == ("wait", ev_r, 0)
    finally:
        backbone.set_conv_mode(None)
        backbone._PLANS.clear()
