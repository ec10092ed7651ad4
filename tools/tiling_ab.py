#!/usr/bin/env python3
"""TILING_MODE (every nn.Conv2d circular, src/depthmap_generation.py: apply_tiling_mode), one float16 forward: the circular 3x3
convolutions and the head tail in-tree (ds_conv3x3_nhwc_circular, ds_dpt_head_tail_circular, the circularly padded gather of the
strided 3x3) against DS_CONV_CIRCULAR=0 (the library convolutions with separate bias / ReLU passes and the unfused torch head),
alternating in one process, `--reps` pairs of `--iters` forwards each.
    python tools/tiling_ab.py [--reps 5] [--iters 5] [--steps beitl,dav2,head]
Steps: beitl = dpt_beit_large_512 at 8 x 3 x 512 x 512; dav2 = Depth-Anything-V2 ViT-L at 1 x 3 x 518 x 518; head = the head tail
alone at the two networks' shapes (8 x 128 x 256^2 -> 512^2, 1 x 128 x 296^2 -> 518^2) against upsample -> circular conv3x3 -> ReLU ->
conv1x1 -> ReLU in torch.  Every step runs in a child process of its own under its own time limit, and the first step that fails
(non-zero exit, time limit) ends the run: nothing more is started on the device after it.  Prints per-forward ms of each route per
pair, median / min / max, and the output difference between the routes.  Name-seeded synthetic weights
(tests/golden/model_weights.py)."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

STEP_SECONDS = {"beitl": 300, "dav2": 240, "head": 120}          # time limit of each step's process


def build(step):
    import model_weights as mw
    import torch
    from src.depthmap_generation import apply_tiling_mode
    if step == "beitl":
        from dmidas.dpt_depth import DPTDepthModel
        m = DPTDepthModel(path=None, backbone="beitl16_512", non_negative=True).eval()
        m.load_state_dict(mw.fill_state_dict_beit(m.state_dict()), strict=True)
        shape = (8, 3, 512, 512)
    else:
        from ddepth_anything_v2 import DepthAnythingV2
        m = DepthAnythingV2('vitl', features=256, out_channels=[256, 512, 1024, 1024]).eval()
        m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
        shape = (1, 3, 518, 518)
    n = apply_tiling_mode(m)
    x = mw.synthetic_image(shape, seed=41).half().cuda().contiguous(memory_format=torch.channels_last)
    return m.cuda().half(), x, n


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(what, routes, reps, iters):
    """routes: {"in-tree": fn, "DS_CONV_CIRCULAR=0": fn}; warm-up, the output difference, then reps alternating timed pairs."""
    for fn in routes.values():
        for _ in range(3):
            fn()
    (na, fa), (nb, fb) = routes.items()
    ya, yb = fa().float(), fb().float()
    diff = ((ya - yb).abs().max() / yb.abs().max()).item()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa, iters))
        tb.append(timed(fb, iters))
        print(f"  [{what}] {na} {ta[-1]:8.3f} ms   {nb} {tb[-1]:8.3f} ms", flush=True)
    print(f"{what}: per forward {na} median {statistics.median(ta):.3f} ms (min {min(ta):.3f}, max {max(ta):.3f}), {nb} median "
          f"{statistics.median(tb):.3f} ms (min {min(tb):.3f}, max {max(tb):.3f}); speed-up {statistics.median(tb) / statistics.median(ta):.3f}x; "
          f"max |difference| of the routes / max |output| {diff:.3e}", flush=True)


def run_step(step, reps, iters):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from src import _native
    from src import vit_mi355x as vm
    print(f"step {step} on {torch.cuda.get_device_name(0)}", flush=True)
    if step in ("beitl", "dav2"):
        m, x, n = build(step)

        def forward(hip):
            vm.CONV_CIRCULAR_HIP = hip
            with torch.no_grad():
                return m(x)
        before = dict(_native.CALLS)
        forward(True)
        calls = {k: _native.CALLS[k] - before.get(k, 0) for k in ("ds_conv3x3_nhwc_circular", "ds_dpt_head_tail_circular", "ds_conv3x3_nhwc", "ds_dpt_head_tail")}
        print(f"{step}: input {tuple(x.shape)} f16, {n} circular convolutions, in-tree launches per forward {calls}", flush=True)
        alternate(step, {"in-tree": lambda: forward(True), "DS_CONV_CIRCULAR=0": lambda: forward(False)}, reps, iters)
        vm.CONV_CIRCULAR_HIP = True
        return
    torch.manual_seed(4)
    conv3, conv1 = nn.Conv2d(128, 32, 3, padding=1).cuda().half(), nn.Conv2d(32, 1, 1).cuda().half()
    conv3.padding_mode = "circular"
    for (b, ih, iw, oh, ow) in ((8, 256, 256, 512, 512), (1, 296, 296, 518, 518)):
        x = torch.randn((b, 128, ih, iw), device="cuda").half().contiguous(memory_format=torch.channels_last)

        def fused():
            with torch.no_grad():
                return _native.dpt_head_tail(x, (oh, ow), conv3, conv1)

        def unfused():
            with torch.no_grad():
                return F.relu(conv1(F.relu(conv3(vm.interpolate_bilinear(x, size=(oh, ow), align_corners=True)))))
        alternate(f"head tail {b} x {ih} x {iw} -> {oh} x {ow}", {"ds_dpt_head_tail_circular": fused, "unfused torch sequence": unfused}, reps, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--steps", default="beitl,dav2,head")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        run_step(args.child, args.reps, args.iters)
        return 0
    for step in args.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(args.reps), "--iters", str(args.iters)]
        try:
            rc = subprocess.run(cmd, timeout=STEP_SECONDS[step]).returncode
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {STEP_SECONDS[step]} s; stopping here", flush=True)
            return 124
        if rc != 0:
            print(f"step {step}: exit status {rc}; stopping here", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
