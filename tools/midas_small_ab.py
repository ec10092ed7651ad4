#!/usr/bin/env python3
"""MiDaS v2.1 small (model id 6), one float16 forward: the depthwise convolutions in-tree (ds_dwconv_nhwc) against DS_DWCONV=0 (the
library's F.conv2d with groups = channels on the folded weights, with torch's bias / clamp passes around it), alternating in one
process, `--reps` pairs of `--iters` forwards each.
    python tools/midas_small_ab.py [--reps 7] [--iters 10] [--workload a|b|all]
    python tools/midas_small_ab.py --profile         (in-tree route of workload (a) only, 3 + 10 forwards: for rocprofv3 --kernel-trace --stats)
Workloads: (a) 32 frames of 1920 x 1080 at net width 512 -> 32 x 3 x 288 x 512 (upper_bound resize); (b) one 1024^2 image at the
default net size 256 -> 1 x 3 x 256 x 256.  Prints per-forward ms of each route per pair, median / min / max, the output difference
between the routes, and the algorithmic bytes of the depthwise convolutions per forward (f16 x read once + y written once, from the
shapes the kernel sees).  Name-seeded synthetic weights (tests/golden/model_weights.py: torch's default initialisation leaves this
network's head dead, and the two routes would agree on a constant)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import model_weights as mw  # noqa: E402
import torch  # noqa: E402
from dmidas.backbones import efficientnet_lite as effl  # noqa: E402
from dmidas.dpt_depth import midas_net_size  # noqa: E402
from dmidas.midas_net_custom import MidasNet_small  # noqa: E402
from src import _native  # noqa: E402

WORKLOADS = {"a": (32, 1920, 1080, 512), "b": (1, 1024, 1024, 256)}       # (images, width, height, net width)


def net_input(key):
    b, w, h, net = WORKLOADS[key]
    nw, nh = midas_net_size(w, h, net, net, "upper_bound")
    x = torch.rand((b, 3, nh, nw), generator=torch.Generator().manual_seed(1)) * 4 - 2
    return x.half().cuda().contiguous(memory_format=torch.channels_last)


def forward(m, x, hip, n=1):
    effl.DWCONV_HIP = hip
    with torch.no_grad():
        for _ in range(n):
            y = m(x)
    return y


def dw_bytes(m, x):
    total = [0, 0]
    orig = _native.dwconv

    def spy(xx, *a, **k):
        y = orig(xx, *a, **k)
        total[0] += (xx.numel() + y.numel()) * xx.element_size()
        total[1] += 1
        return y
    _native.dwconv = spy
    try:
        forward(m, x, True)
    finally:
        _native.dwconv = orig
    return total


def timed(m, x, hip, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    forward(m, x, hip, iters)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--workload", default="all")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    m = MidasNet_small(path=None, features=64, backbone="efficientnet_lite3", exportable=True, non_negative=True, blocks={'expand': True})
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    m = m.eval().cuda().half()
    if args.profile:
        x = net_input("a")
        forward(m, x, True, 13)
        torch.cuda.synchronize()
        print(f"profile: workload a {tuple(x.shape)}, 13 forwards (3 warm-up + 10), in-tree route")
        return
    for key in (("a", "b") if args.workload == "all" else (args.workload,)):
        x = net_input(key)
        for hip in (True, False):
            forward(m, x, hip, 3)                                   # warm-up: library algorithm choice, caches
        y_hip, y_lib = forward(m, x, True).float(), forward(m, x, False).float()
        diff = ((y_hip - y_lib).abs().max() / y_lib.abs().max()).item()
        nbytes, ncalls = dw_bytes(m, x)
        t_hip, t_lib = [], []
        for _ in range(args.reps):
            t_hip.append(timed(m, x, True, args.iters))
            t_lib.append(timed(m, x, False, args.iters))
            print(f"  [{key}] in-tree {t_hip[-1]:8.3f} ms   DS_DWCONV=0 {t_lib[-1]:8.3f} ms")
        print(f"workload {key}: input {tuple(x.shape)} f16; per forward: in-tree median {statistics.median(t_hip):.3f} ms "
              f"(min {min(t_hip):.3f}, max {max(t_hip):.3f}), DS_DWCONV=0 median {statistics.median(t_lib):.3f} ms "
              f"(min {min(t_lib):.3f}, max {max(t_lib):.3f}); speed-up {statistics.median(t_lib) / statistics.median(t_hip):.3f}x; "
              f"max |difference| of the routes / max |output| {diff:.3e}; ds_dwconv_nhwc: {ncalls} launches, "
              f"{nbytes / 1e6:.1f} MB read + written per forward")
    effl.DWCONV_HIP = True


if __name__ == "__main__":
    main()
