#!/usr/bin/env python3
"""The autostereogram kernel (ds_autostereogram_u8: one launch, one workgroup per image row) beside the floor its design cannot beat,
on one 1024 x 1024 map and one 1080p frame (1080 x 1920), `--reps` rounds of `--iters` calls each.
    python tools/autostereogram_ab.py [--reps 5] [--iters 20]
    python tools/autostereogram_ab.py --model           (host only: needs no GPU)
The entry point is timed by a stream-event pair around `--iters` calls of the C entry point (no Python between two calls but the ctypes
call).  The yardstick, by an event pair in the same process, alternating with it: a device copy of the output's bytes (3 B per pixel
read and as much written) plus a device copy of the depth map (2 B per pixel read and written: the kernel only reads them, so the
yardstick moves 2 B per pixel more than the kernel must).
Four inputs: a depth-map-like one (smooth ramp, +-3 levels of noise, a near rectangle), a flat far map, full-range white noise (most
columns hidden, the links that remain irregular), all three at the defaults of src/autostereogram_generation.py (period 96, depth
factor 1/3, coloured dots), and the longest chains the definition allows: a flat near map at period 16, depth factor 0.5 (separation
11, so a component has width / 11 members).  Beside the times: the rounds of label propagation per row (maximum and mean over the
rows; the last, idle round included), from one call of ds_autostereogram_rounds_u8 outside the timed region.  Bit-exactness against
the NumPy model is tests/test_gpu_autostereogram.py's business.  --model times the NumPy model of tests/autostereogram_cases.py on
one 256 x 256 map on the host, as context.  The measuring runs in a child process under a time limit; if it fails or runs out of time
nothing more is started on the device."""
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
SIZES = ((1024, 1024), (1080, 1920))
PERIOD, M = 96, 85


def inputs(np, h, w):
    """[(name, depth [1,h,w], period, m)]"""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:h, 0:w]
    near = (x >= w // 3) & (x < 2 * w // 3) & (y >= h // 4) & (y < 3 * h // 4)
    ramp = (12000 + (8 * x * 1024) // w + (5 * y * 1024) // h + np.where(near, 30000, 0))[None] + rng.integers(-3, 4, (1, h, w))
    return [("depth-map-like (ramp + noise + a near rectangle)", ramp.astype(np.uint16), PERIOD, M),
            ("flat far map", np.zeros((1, h, w), np.uint16), PERIOD, M),
            ("white noise", rng.integers(0, 65536, (1, h, w), dtype=np.uint16), PERIOD, M),
            ("longest chains (flat near map, period 16, depth factor 0.5)", np.full((1, h, w), 65535, np.uint16), 16, 128)]


def measure(reps, iters):
    import numpy as np
    import torch
    from src import _native
    dev = torch.cuda.current_device()
    L, ctx = _native.lib(), _native.ctx_for(dev)
    stream = torch.cuda.current_stream().cuda_stream
    print(f"autostereogram_ab on {torch.cuda.get_device_name(dev)}: {reps} rounds of {iters} calls, coloured dots, "
          f"library {os.path.basename(_native.LIB_PATH)}", flush=True)

    def med(v):
        return f"median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})"

    def timed(fn, count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(count):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / count * 1e3
    for h, w in SIZES:
        pixels = h * w
        src = torch.zeros((3 * pixels,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        out = torch.empty((1, h, w, 3), dtype=torch.uint8, device="cuda")
        rounds = torch.empty((h,), dtype=torch.int16, device="cuda")
        for what, depth, period, m in inputs(np, h, w):
            d = torch.from_numpy(depth).cuda()
            d2 = torch.empty_like(d)
            print(f"[1 x {h} x {w}: {what}]", flush=True)

            def entry():
                rc = L.ds_autostereogram_u8(ctx, d.data_ptr(), 1, h, w, period, m, 0, 1, None, 0, 0, 0, out.data_ptr(), stream)
                assert rc == 0, rc

            def floor():
                dst.copy_(src)
                d2.copy_(d)
            rc = L.ds_autostereogram_rounds_u8(ctx, d.data_ptr(), 1, h, w, period, m, 0, 1, None, 0, 0, 0, out.data_ptr(), rounds.data_ptr(), stream)
            assert rc == 0, rc
            r = rounds.cpu().numpy()
            for _ in range(2):
                timed(entry, iters), timed(floor, iters)
            tk, tc = [], []
            for _ in range(reps):
                tk.append(timed(entry, iters))
                tc.append(timed(floor, iters))
            k = statistics.median(tk)
            print(f"        ds_autostereogram_u8 (one launch)            {med(tk)}\n"
                  f"        copy of the output's bytes + copy of the depth {med(tc)}   (ratio {k / statistics.median(tc):.2f})\n"
                  f"        rounds per row: max {int(r.max())}, mean {float(r.mean()):.2f};  {k * 1e-6 / pixels * 1e12:.1f} ps per pixel", flush=True)
            del d, d2


def model_time():
    import numpy as np
    import autostereogram_cases as ac
    for what, depth, period, m in inputs(np, 256, 256):
        t0 = time.perf_counter()
        ac.model(depth[0], period, m, 0, 1)
        print(f"NumPy model on the host CPU, 256 x 256, {what}: {time.perf_counter() - t0:.2f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.model:
        model_time()
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
