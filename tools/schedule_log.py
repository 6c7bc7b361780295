#!/usr/bin/env python3
"""The engine's schedule as text, without a GPU: the host-emulation build with HIPEMU_NOEXEC=1 (launches return at once) and
its call log -- every kernel launch (name, grid, block, stream), event record and stream wait of two training rounds
(forward + backward each) at real layer widths and image sizes, so the size-dependent routing is the real one.
TEST / ANALYSIS TOOL for refactors of the engine: two checkouts must give the same text.
    python tools/schedule_log.py --all OUT_DIR            every case below, one fresh process each (switches are read once)
    python tools/schedule_log.py --compare DIR_A DIR_B    one line per case: entries, equal or not
    python tools/schedule_log.py --case NAME --out FILE"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

R34 = dict(arch="Resnet34_8s", h=480, w=640, bw=64)
# name -> (network / call pattern, environment)
CASES = {}
for _b in (1, 4):
    CASES["r34_b%d_pair" % _b] = (dict(R34, batch=_b, pattern="pair"), {})
    CASES["r34_b%d_two_calls" % _b] = (dict(R34, batch=_b, pattern="two"), {})
    CASES["r34_b%d_pair_normalize" % _b] = (dict(R34, batch=_b, pattern="pair", normalize=True), {})
CASES["r50_b1_pair"] = (dict(R34, arch="Resnet50_8s", batch=1, pattern="pair"), {})
CASES["r18_64x64_bw8_pair"] = (dict(arch="Resnet18_8s", h=64, w=64, bw=8, batch=2, pattern="pair"), {})
for _env in ("DCN_BACKWARD_OVERLAP=0", "DCN_HL_PRODUCERS=0", "DCN_BN_BWD_FUSED=1", "DCN_DEFER_RESIDUAL_ADD=0",
             "DCN_GEMM_HL=0 DCN_WGRAD_HL=2", "DCN_GEMM_HL=2 DCN_WGRAD_HL=2", "DCN_WSPLIT_OVERLAP=0", "DCN_BN_BWD_LEAN=0",
             "DCN_BN_BWD_LEAN_DEPTH=1"):
    CASES["r34_b4_pair_" + _env.replace(" ", "_").replace("=", "")] = (
        dict(R34, batch=4, pattern="pair"), dict(kv.split("=") for kv in _env.split()))
CASES["r34_b4_pair_fp32"] = (dict(R34, batch=4, pattern="pair", mode="fp32"), {})
CASES["r34_b4_pair_profiled"] = (dict(R34, batch=4, pattern="pair", profile=True), {})
# the backward pass runs under routes whose transposed hl32 weight images the forward call did not make
CASES["r34_b4_pair_no_saved_wt"] = (dict(R34, batch=4, pattern="pair", backward_env={"DCN_GEMM_HL": "2"}), {"DCN_GEMM_HL": "0"})


def run_case(name, out):
    cfg, _ = CASES[name]
    for p in (ROOT, os.path.join(ROOT, "pytorch-dense-correspondence_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    from helpers import CallLog, use_emulation_library
    lib = use_emulation_library().get()
    import torch
    from dcn_hip import backbone
    from pytorch_segmentation_detection.models import resnet_dilated as prod
    backbone.set_conv_mode(cfg.get("mode", "f16x3"))
    m = getattr(prod, cfg["arch"])(num_classes=3, base_width=cfg["bw"])
    m.train()
    xa, xb = (torch.zeros(cfg["batch"], 3, cfg["h"], cfg["w"]) for _ in range(2))
    normalize = bool(cfg.get("normalize"))
    with CallLog(lib) as log:
        for _ in range(2):
            if cfg["pattern"] == "pair":
                ya, yb = m.forward_pair(xa, xb, normalize)
                assert m._last_plan.groups == 2
            else:
                ya, yb = m(xa, normalize), m(xb, normalize)
            if cfg.get("profile"):
                m._last_plan.profile_begin()
            for k, v in cfg.get("backward_env", {}).items():
                os.environ[k] = v
            lib.dcn_reload_env()
            (ya.sum() + yb.sum()).backward()
            if cfg.get("profile"):
                m._last_plan.profile_end()
            for k in cfg.get("backward_env", {}):
                os.environ[k] = CASES[name][1][k]
            lib.dcn_reload_env()
        lines = log.lines()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%s: %d entries" % (name, len(lines)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all")
    ap.add_argument("--case")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        bad = 0
        for name in CASES:
            ta, tb = (open(os.path.join(d, name + ".log")).read().splitlines() for d in a.compare)
            bad += ta != tb
            print("%-44s %6d / %6d entries  %s" % (name, len(ta), len(tb), "equal" if ta == tb else "DIFFERENT"))
        sys.exit(1 if bad else 0)
    if a.all:
        os.makedirs(a.all, exist_ok=True)
        for name, (_, env) in CASES.items():
            e = dict(os.environ, HIPEMU_NOEXEC="1", **env)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case", name, "--out",
                                   os.path.join(a.all, name + ".log")], env=e)
        return
    run_case(a.case, a.out)


if __name__ == "__main__":
    main()
