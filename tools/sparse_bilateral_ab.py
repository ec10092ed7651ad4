#!/usr/bin/env python3
"""The 3D-photo depth preparation (ds_sparse_bilateral_f32: one pass of the discontinuity-masked median of a float32 depth map) beside
its floor, a device copy of the bytes a pass must move (the float32 map in and out, the uint8 jump map out), on one 1024 x 1024 map,
for the windows 5, 7 and 15, alternating in one process, `--reps` rounds of `--iters` calls each.
    python tools/sparse_bilateral_ab.py [--reps 5] [--iters 20]
    python tools/sparse_bilateral_ab.py --reference <path of the reference checkout>      (host only: needs no GPU)
The kernel is timed through the library's own kernel timer (an event pair around the one launch, DS_KT_SPARSE_BILATERAL), the copies
through an event pair around the two of them.  Two inputs: a depth-map-like map (a smooth disparity ramp, three objects with a
disparity step around each, noise far below the threshold: jumps are sparse and nearly every wave only copies) and white disparity
noise of +-0.03 around 0.5 (about a third of the pixels are jumps: every window holds masked and valid taps, so every pixel selects
-- the worst case).  Printed beside each time: the share of pixels that are jumps, the bytes a pass moves over the time, and the
ratio to the copies.  --reference times the reference's own Python loop on the host instead: all five default passes on one 256 x 256
depth-map-like map, once.  The measuring runs in a child process under a time limit; if it fails or runs out of time nothing more is
started on the device."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd")):
    sys.path.insert(0, p)

CHILD_SECONDS = 300
SIDE = 1024
WINDOWS = (5, 7, 15)
THRESHOLD = 0.04
REFERENCE_WINDOWS = [7, 7, 5, 5, 5]


def inputs(np, side):
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:side, 0:side]
    disp = 0.2 + 0.3 * y / side + 0.05 * np.sin(x / (side / 12.0))
    for cy, cx, r, lift in ((0.3, 0.3, 0.12, 0.25), (0.6, 0.7, 0.18, 0.4), (0.8, 0.25, 0.08, 0.15)):
        disp = disp + lift * ((y - cy * side)**2 + (x - cx * side)**2 < (r * side)**2)
    disp = disp + rng.uniform(-0.002, 0.002, disp.shape)
    noise = 0.5 + rng.uniform(-0.03, 0.03, disp.shape)
    return [("depth-map-like, sparse jumps", (1.0 / disp).astype(np.float32)), ("white noise, every window selects", (1.0 / noise).astype(np.float32))]


def measure(reps, iters):
    import numpy as np
    import torch
    from src import _native
    dev = torch.cuda.current_device()
    print(f"sparse_bilateral_ab on {torch.cuda.get_device_name(dev)}: 1 x {SIDE} x {SIDE}, {reps} rounds of {iters} calls", flush=True)
    moved = SIDE * SIDE * (4 + 4 + 1)

    def med(v):
        return f"median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})"
    for what, depth in inputs(np, SIDE):
        v = torch.from_numpy(depth).cuda()[None]
        dst, jsrc = torch.empty_like(v), torch.zeros(v.shape, dtype=torch.uint8, device=v.device)
        jdst = torch.empty_like(jsrc)

        def copies():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                dst.copy_(v)
                jdst.copy_(jsrc)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) / iters * 1e3

        def kernel(window):
            _native.kernel_timer_enable(dev, True)
            for _ in range(iters):
                _native.sparse_bilateral_pass_f32(v, v, window, THRESHOLD)
            k, ms = _native.kernel_timer_read(dev, "sparse_bilateral")
            _native.kernel_timer_enable(dev, False)
            assert k == iters, (k, iters)
            return ms / k * 1e3
        out, jump = _native.sparse_bilateral_pass_f32(v, v, 7, THRESHOLD)
        print(f"[{what}] jumps: {float(jump.float().mean()) * 100:.2f} % of the pixels; a window-7 pass changes "
              f"{float((out != v).float().mean()) * 100:.2f} %", flush=True)
        for window in WINDOWS:
            for _ in range(2):
                kernel(window), copies()
            tk, tc = [], []
            for _ in range(reps):
                tk.append(kernel(window))
                tc.append(copies())
            k, c = statistics.median(tk), statistics.median(tc)
            print(f"    window {window:2d}: ds_sparse_bilateral_f32 {med(tk)}, {moved / k / 1e6:7.2f} TB/s of its 9 B per pixel\n"
                  f"               copies of those bytes   {med(tc)}; kernel / copies {k / c:.2f}", flush=True)
        del v, dst, jsrc, jdst


def reference_on_host(path):
    import numpy as np
    sys.path.insert(0, path)
    from inpaint.bilateral_filtering import sparse_bilateral_filtering
    depth = inputs(np, 256)[0][1]
    image = np.full((256, 256, 3), 128, np.uint8)
    config = {'filter_size': REFERENCE_WINDOWS, 'depth_threshold': THRESHOLD, 'sigma_s': 4.0, 'sigma_r': 0.5}
    t0 = time.perf_counter()
    sparse_bilateral_filtering(depth, image, config, num_iter=len(REFERENCE_WINDOWS))
    dt = time.perf_counter() - t0
    print(f"reference sparse_bilateral_filtering on the host CPU, 256 x 256 depth-map-like, windows {REFERENCE_WINDOWS}: {dt:.2f} s "
          f"for the five passes ({dt / 5 * 1e3:.0f} ms per pass), one run", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reference", help="time the reference's own function on the host instead (path of its checkout)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reference:
        reference_on_host(args.reference)
        return 0
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
