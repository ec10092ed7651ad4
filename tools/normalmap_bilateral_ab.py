#!/usr/bin/env python3
"""The bilateral pre-filter of the normal map (create_normalmap_batch(bilateral=(d, sigma_color, sigma_space)): ds_bilateral_u16 ->
ds_normalmap_f64) against the unfiltered route (ds_normalmap, the fused uint16 kernel), on 32 x 1024^2 uint16 maps, Sobel 3, for
d = 5, 9, 15 (sigma_color 300, sigma_space d / 4), alternating in one process, `--reps` rounds of `--iters` calls each.
    python tools/normalmap_bilateral_ab.py [--reps 5] [--iters 10]
Timed: ds_bilateral_u16 alone through the library's own DS_KT_NORMALMAP kernel timer (an event pair around the one launch), and the
whole normal map with and without the filter by a device event pair around the calls (the filtered route is 1 + 7 launches: the
filter, then the separable float64 passes of ds_normalmap_f64, which the kernel timer does not bracket).  Two inputs: a smooth ramp
with +-3 levels of noise plus one cliff (what a depth map looks like: nearly every range-table read is served from the kernel's LDS
slice) and full-range white noise (the worst case: nearly every read goes to memory).  Printed beside each kernel time: the float64 vector-issue bound -- taps inside the circle x 3 float64
operations per pixel, at the datasheet's 78.6 TFLOP/s float64 vector peak counted as 39.3e12 operations/s -- and the time as a
multiple of it.  The measuring runs in a child process under a time limit; if it fails or runs out of time nothing more is started
on the device."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd")):
    sys.path.insert(0, p)

CHILD_SECONDS = 300
N, H, W = 32, 1024, 1024
DIAMETERS = (5, 9, 15)
SIGMA_COLOR = 300.0
F64_OPS_PER_SECOND = 39.3e12          # 78.6 TFLOP/s float64 vector (datasheet), a fused multiply-add counted as 2: operations issued / s


def inputs(np):
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:H, 0:W]
    ramp = (20000 + 9 * x + 5 * y + np.where(x >= W // 2, 4096, 0))[None] + rng.integers(-3, 4, (N, H, W))
    return [("ramp + noise + cliff", ramp.astype(np.uint16)), ("white noise", rng.integers(0, 65536, (N, H, W), dtype=np.uint16))]


def measure(reps, iters):
    import numpy as np
    import torch
    from src import _native
    import src.normalmap_generation as nm
    dev = torch.cuda.current_device()
    print(f"normalmap_bilateral_ab on {torch.cuda.get_device_name(dev)}: {N} x {H} x {W} uint16, {reps} rounds of {iters} calls", flush=True)

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters * 1e3                        # us per call

    def med(v):
        return f"median {statistics.median(v):9.1f} us (min {min(v):.1f}, max {max(v):.1f})"
    for what, host in inputs(np):
        d = torch.from_numpy(host).cuda()
        for dia in DIAMETERS:
            params = (dia, SIGMA_COLOR, dia / 4.0)
            taps = int(np.count_nonzero(_native.bilateral_tables(*params)[0]))
            bound = N * H * W * taps * 3 / F64_OPS_PER_SECOND * 1e6

            def kernel():                                             # the library's timer: one event pair around each launch
                _native.kernel_timer_enable(dev, True)
                for _ in range(iters):
                    _native.bilateral_u16(d, *params)
                k, ms = _native.kernel_timer_read(dev, "normalmap")
                _native.kernel_timer_enable(dev, False)
                assert k == iters, (k, iters)
                return ms / k * 1e3

            def plain():
                return nm.create_normalmap_batch(d, None, 3, None, False)

            def filtered():
                return nm.create_normalmap_batch(d, None, 3, None, False, bilateral=params)

            def f64_only(f=_native.bilateral_u16(d, *params)):        # the float64 normal map of the already filtered plane
                return nm.create_normalmap_batch(f, None, 3, None, False)
            for _ in range(2):
                plain(), filtered(), f64_only()
            tk, tp, tf, t64 = [], [], [], []
            for _ in range(reps):
                tk.append(kernel())
                tp.append(events(plain))
                tf.append(events(filtered))
                t64.append(events(f64_only))
            k = statistics.median(tk)
            print(f"[{what}] d = {dia:2d} ({taps:3d} taps in the circle)\n"
                  f"    ds_bilateral_u16            {med(tk)}; float64 issue bound {bound:7.1f} us, x {k / bound:.2f}\n"
                  f"    normal map, unfiltered      {med(tp)}   (ds_normalmap, fused uint16 kernel)\n"
                  f"    normal map, filtered        {med(tf)}   (ds_bilateral_u16 + ds_normalmap_f64)\n"
                  f"    ds_normalmap_f64 part alone {med(t64)}   (reads the 8 B / pixel plane the filter wrote)\n"
                  f"    filter share of the filtered route {k / statistics.median(tf):.3f}", flush=True)
        del d


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
