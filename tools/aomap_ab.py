#!/usr/bin/env python3
"""The ambient-occlusion kernel (ds_aomap_u16: the horizon scan of a uint16 depth map) beside a device copy of the bytes a pass moves,
on one 1024 x 1024 map, for (radius, directions) = (8, 8), (16, 8), (32, 16), `--reps` rounds of `--iters` calls each.
    python tools/aomap_ab.py [--reps 5] [--iters 20] [--maps 1]
    python tools/aomap_ab.py --model           (host only: needs no GPU)
The kernel is timed through the library's own kernel timer (an event pair around the one launch, DS_KT_AOMAP), the copy -- 1.5 B per
pixel read and as much written: the 3 B per pixel a pass that writes the uint8 map alone moves -- by a device event pair in the same
process.
Two inputs: full-range white noise (every tap rises for some pixel: the compare flips often) and a depth-map-like one (smooth ramp, +-3
levels of noise, one cliff).  Printed per row: the time per pixel and tap (flat across the rows if the tap loop is the limit; the
per-ray division and square roots weigh more where a ray has few taps) and the taps a CU retires per clock, 256 CUs at 2.4 GHz.
--maps n times a batch of n maps in one launch (one 1024 x 1024 map is 512 workgroups, two per CU; a batch fills the device).
Bit-exactness against the NumPy model is tests/test_gpu_aomap.py's business.  --model times the NumPy model of tests/aomap_cases.py on one 256 x 256 map on the host, as
context.  The measuring runs in a child process under a time limit; if it fails or runs out of time nothing more is started on the
device."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

CHILD_SECONDS = 300
SIDE = 1024
ROWS = ((8, 8), (16, 8), (32, 16))
RELIEF = 32.0
CUS, CLOCK = 256, 2.4e9


def inputs(np, side=SIDE, maps=1):
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:side, 0:side]
    ramp = (20000 + 9 * x + 5 * y + np.where(x >= side // 2, 4096, 0))[None] + rng.integers(-3, 4, (maps, side, side))
    return [("depth-map-like (ramp + noise + cliff)", ramp.astype(np.uint16)),
            ("white noise", rng.integers(0, 65536, (maps, side, side), dtype=np.uint16))]


def measure(reps, iters, maps):
    import numpy as np
    import torch
    from src import _native
    dev = torch.cuda.current_device()
    print(f"aomap_ab on {torch.cuda.get_device_name(dev)}: {maps} x {SIDE} x {SIDE} uint16, relief {RELIEF}, {reps} rounds of {iters} calls", flush=True)

    def med(v):
        return f"median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})"
    src = torch.zeros((maps * SIDE * SIDE * 3 // 2,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def copy():                                                       # 1.5 B per pixel read and as much written: the pass's 3 B per pixel
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters * 1e3
    for what, host in inputs(np, maps=maps):
        d = torch.from_numpy(host).cuda()
        print(f"[{what}]", flush=True)
        for radius, directions in ROWS:
            taps = int(_native.aomap_offsets(radius, directions)[1][-1])
            out = torch.empty((maps, SIDE, SIDE), dtype=torch.uint8, device="cuda")

            def kernel(wrap):
                _native.kernel_timer_enable(dev, True)
                for _ in range(iters):
                    _native.aomap_u16(d, radius, directions, RELIEF, wrap=wrap, out=out)
                k, ms = _native.kernel_timer_read(dev, "aomap")
                _native.kernel_timer_enable(dev, False)
                assert k == iters, (k, iters)
                return ms / k * 1e3
            for _ in range(2):
                kernel(False), kernel(True), copy()
            tk, tw, tc = [], [], []
            for _ in range(reps):
                tk.append(kernel(False))
                tw.append(kernel(True))
                tc.append(copy())
            k = statistics.median(tk)
            per_tap = k * 1e-6 / (maps * SIDE * SIDE * taps)
            print(f"    R = {radius:2d}, K = {directions:2d} ({taps:3d} taps per pixel)\n"
                  f"        ds_aomap_u16          {med(tk)}\n"
                  f"        ds_aomap_u16, wrap    {med(tw)}\n"
                  f"        copy moving 3 B/pixel {med(tc)}   (ratio {k / statistics.median(tc):.1f})\n"
                  f"        {per_tap * 1e12:.3f} ps per pixel and tap = {1.0 / (per_tap * CUS * CLOCK):.1f} taps per CU and clock; "
                  f"darkest {int(out.min())}, mean {float(out.float().mean()):.1f}", flush=True)
        del d


def model_time():
    import numpy as np
    import aomap_cases as ac
    for what, host in inputs(np, 256):
        for radius, directions in ROWS:
            t0 = time.perf_counter()
            ac.model(host[0], radius, directions, RELIEF)
            print(f"NumPy model on the host CPU, 256 x 256 {what}, R = {radius}, K = {directions}: {time.perf_counter() - t0:.2f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--maps", type=int, default=1)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.model:
        model_time()
        return 0
    if args.child:
        measure(args.reps, args.iters, args.maps)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--iters", str(args.iters), "--maps", str(args.maps)]
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
