#!/usr/bin/env python3
"""Depth refinement (ds_joint_bilateral_u16: the joint bilateral filter of a uint16 depth map guided by the RGB image) beside its
yardstick ds_bilateral_u16 (the depth-guided sibling in front of the normal map: the same tap count and the same float64 arithmetic;
what differs is the 4-byte guide read per tap, the 766-entry colour table in LDS instead of a 2048-entry slice plus memory, and a
uint16 store instead of a float64 one), one pass each, on 32 x 1024^2 and on 8 x 1080p, for d = 9 and d = 15, alternating in one
process, `--reps` rounds of `--iters` calls each.
    python tools/depth_refine_ab.py [--reps 5] [--iters 10]
Timed through the library's own kernel timers (an event pair around the one launch): DS_KT_DEPTH_REFINE and DS_KT_NORMALMAP.  Two
inputs: a depth-map-like map (a smooth ramp with +-3 levels of noise and one cliff) with a photograph-like guide (two smoothly shaded
colour regions with +-4 levels of noise per channel, meeting 3 columns off the cliff), and white noise for both (the worst case for
the data-dependent table reads of both kernels).  Printed beside each time: the float64 vector-issue bound -- taps inside the circle x
3 float64 operations per pixel, at the datasheet's 78.6 TFLOP/s float64 vector peak counted as 39.3e12 operations/s -- and the ratio
joint / sibling.  The measuring runs in a child process under a time limit; if it fails or runs out of time nothing more is started on
the device."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd")):
    sys.path.insert(0, p)

CHILD_SECONDS = 300
SHAPES = ((32, 1024, 1024), (8, 1080, 1920))
DIAMETERS = (9, 15)
SIGMA_COLOR_GUIDE = 25.0              # summed 8-bit channel difference
SIGMA_COLOR_DEPTH = 300.0             # uint16 levels (the sibling's range weight)
F64_OPS_PER_SECOND = 39.3e12          # 78.6 TFLOP/s float64 vector (datasheet), a fused multiply-add counted as 2: operations issued / s


def inputs(np, n, h, w):
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:h, 0:w]
    ramp = (20000 + 9 * x + 5 * y + np.where(x >= w // 2, 4096, 0)).astype(np.int32)[None] + rng.integers(-3, 4, (n, h, w), dtype=np.int8)
    shade = (x * 40 // w + y * 24 // h)[..., None]
    photo = np.where((x >= w // 2 - 3)[..., None], np.array([150, 120, 60]), np.array([40, 90, 70])) + shade
    photo = photo.astype(np.int16)[None] + rng.integers(-4, 5, (n, h, w, 3), dtype=np.int8)
    return [("depth-map-like, photograph-like guide", ramp.astype(np.uint16), photo.astype(np.uint8)),
            ("white noise, white-noise guide", rng.integers(0, 65536, (n, h, w), dtype=np.uint16),
             rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8))]


def measure(reps, iters):
    import numpy as np
    import torch
    from src import _native
    dev = torch.cuda.current_device()
    print(f"depth_refine_ab on {torch.cuda.get_device_name(dev)}: {reps} rounds of {iters} calls, kernel timers", flush=True)

    def timed(kind, fn):
        _native.kernel_timer_enable(dev, True)
        for _ in range(iters):
            fn()
        k, ms = _native.kernel_timer_read(dev, kind)
        _native.kernel_timer_enable(dev, False)
        assert k == iters, (kind, k, iters)
        return ms / k * 1e3                                           # us per launch

    def med(v):
        return f"median {statistics.median(v):9.1f} us (min {min(v):.1f}, max {max(v):.1f})"
    for n, h, w in SHAPES:
        for what, depth, guide in inputs(np, n, h, w):
            d, g = torch.from_numpy(depth).cuda(), torch.from_numpy(guide).cuda()
            for dia in DIAMETERS:
                pj, pb = (dia, SIGMA_COLOR_GUIDE, dia / 3.0), (dia, SIGMA_COLOR_DEPTH, dia / 3.0)
                taps = int(np.count_nonzero(_native.depth_refine_tables(*pj)[0]))
                bound = n * h * w * taps * 3 / F64_OPS_PER_SECOND * 1e6

                def joint():
                    return _native.joint_bilateral_u16(d, g, *pj)

                def sibling():
                    return _native.bilateral_u16(d, *pb)
                for _ in range(2):
                    joint(), sibling()
                tj, tb = [], []
                for _ in range(reps):
                    tj.append(timed("depth_refine", joint))
                    tb.append(timed("normalmap", sibling))
                j, b = statistics.median(tj), statistics.median(tb)
                print(f"[{n} x {h} x {w}; {what}] d = {dia:2d} ({taps:3d} taps in the circle)\n"
                      f"    ds_joint_bilateral_u16  {med(tj)}; float64 issue bound {bound:7.1f} us, x {j / bound:.2f}\n"
                      f"    ds_bilateral_u16        {med(tb)}; x {b / bound:.2f}\n"
                      f"    joint / sibling         {j / b:.3f}", flush=True)
            del d, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        measure(args.reps, args.iters)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--iters", str(args.iters)]
    try:
        rc = subprocess.run(cmd, timeout=CHILD_SECONDS).returncode
    except subprocess.TimeoutExpired:
        print(f"no result within {CHILD_SECONDS} s; stopping here", flush=True)
        return 124
    if rc != 0:
        print(f"exit status {rc}; stopping here", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
