#!/usr/bin/env python3
"""The parallax renderer (ds_parallax_u8: a memset of the key workspace, the splat launch, the resolve launch) beside the floor its
design cannot beat, on one 1024 x 1024 image x 24 views of the 'circle' path at the defaults of src/parallax_generation.py
(shift (12, 6), zoom 0.04, focus ('point', 0.5, 0.5), fill 32), `--reps` rounds of `--iters` calls each.
    python tools/parallax_ab.py [--reps 5] [--iters 10] [--views 24]
    python tools/parallax_ab.py --model           (host only: needs no GPU)
The entry point is timed by a stream-event pair around `--iters` calls of the C entry point (no Python between two calls but the ctypes
call).  The yardstick, by an event pair in the same process, alternating: a device copy of the output's bytes (3 B per target pixel
read and as much written) plus a clear of the key buffer (8 B per target pixel) -- what any renderer of this design must move.
The two launches are timed apart from each other OUTSIDE the timed region: with ds_profile_enable the entry point brackets the splat
and the resolve launch with the context's two event pairs; one call per reading, `--reps` readings.
Three inputs: a depth-map-like one (smooth ramp, +-3 levels of noise, one cliff), an all-in-focus one (a flat map at its focus depth:
every pixel lands on itself, no collisions, no holes) and full-range white noise (every pixel flung somewhere else: the most
collisions and holes).  Printed per input: the offers inside the image per source pixel and view (each is one 8-byte atomic unless the
read in front of it skips it), the share of target pixels that are holes (filled / not filled), and the offered bytes per second of
the splat launch.  Bit-exactness against the NumPy model is tests/test_gpu_parallax.py's business.  --model times the NumPy model
of tests/parallax_cases.py on one 256 x 256 image x 24 views on the host, as context.  The measuring runs in a child process under a
time limit; if it fails or runs out of time nothing more is started on the device.  DS_NATIVE_LIB=<path> times another build of the
library (ds_parallax.hip compiled with -DPX_PRECHECK=0: every offer is an atomic)."""
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
PATH, SHIFT, ZOOM, FOCUS, FILL = 'circle', (12.0, 6.0), 0.04, ('point', 0.5, 0.5), 32


def inputs(np, side=SIDE):
    """[(name, image, depth)]"""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:side, 0:side]
    image = rng.integers(0, 256, (1, side, side, 3), dtype=np.uint8)
    near = (x >= side // 3) & (x < 2 * side // 3) & (y >= side // 4) & (y < 3 * side // 4)
    ramp = (12000 + (8 * x + 5 * y) * 1024 // side + np.where(near, 30000, 0))[None] + rng.integers(-3, 4, (1, side, side))
    return [("depth-map-like (ramp + noise + a near rectangle, focus on the rectangle)", image, ramp.astype(np.uint16)),
            ("all in focus (flat map at its focus depth)", image, np.full((1, side, side), 30000, np.uint16)),
            ("white noise", image, rng.integers(0, 65536, (1, side, side), dtype=np.uint16))]


def offers_inside(torch, depth_u16, focus_t, poses):
    """Offers that land inside the image, summed over the views: the definition's landing point and footprint as torch passes."""
    _, h, w = depth_u16.shape
    z = (depth_u16.view(torch.int16).to(torch.int64) & 0xffff)[0]
    e = z - (int(focus_t.view(torch.int16)[0]) & 0xffff)
    y, x = torch.meshgrid(torch.arange(h, device=z.device), torch.arange(w, device=z.device), indexing='ij')
    cx, cy = 16 * x + 8 - 8 * w, 16 * y + 8 - 8 * h
    total = 0
    for tx, ty, tz in poses.tolist():
        m = (e * tz + 32768) >> 16
        ux = 16 * x + 8 + ((e * tx + 32768) >> 16) + ((cx * m + 2048) >> 12)
        uy = 16 * y + 8 + ((e * ty + 32768) >> 16) + ((cy * m + 2048) >> 12)
        nx = (torch.clamp(((ux + 19) >> 4) - 1, max=w - 1) - torch.clamp((ux - 5) >> 4, min=0) + 1).clamp(min=0)
        ny = (torch.clamp(((uy + 19) >> 4) - 1, max=h - 1) - torch.clamp((uy - 5) >> 4, min=0) + 1).clamp(min=0)
        total += int((nx * ny).sum())
    return total


def measure(reps, iters, views):
    import numpy as np
    import torch
    from src import _native
    dev = torch.cuda.current_device()
    L, ctx = _native.lib(), _native.ctx_for(dev)
    poses = _native.parallax_poses(PATH, views, SHIFT[0], SHIFT[1], ZOOM)
    targets = views * SIDE * SIDE
    print(f"parallax_ab on {torch.cuda.get_device_name(dev)}: 1 x {SIDE} x {SIDE} x {views} views ('{PATH}', shift {SHIFT}, zoom {ZOOM}, fill {FILL}), "
          f"{reps} rounds of {iters} calls, library {os.path.basename(_native.LIB_PATH)}", flush=True)
    print(f"    output {3 * targets / 2**20:.0f} MiB, key workspace {8 * targets / 2**20:.0f} MiB", flush=True)

    def med(v):
        return f"median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})"
    src = torch.zeros((3 * targets,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    keys = torch.empty((targets,), dtype=torch.int64, device="cuda")
    out = torch.empty((1, views, SIDE, SIDE, 3), dtype=torch.uint8, device="cuda")
    mask = torch.empty((1, views, SIDE, SIDE), dtype=torch.uint8, device="cuda")
    poses_t = torch.from_numpy(poses).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn, count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(count):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / count * 1e3
    for what, image, depth in inputs(np):
        im, d = torch.from_numpy(image).cuda(), torch.from_numpy(depth).cuda()
        f = _native._focus_on_device("parallax_ab", FOCUS, d)
        print(f"[{what}]", flush=True)

        def entry(mp=None):
            rc = L.ds_parallax_u8(ctx, im.data_ptr(), d.data_ptr(), f.data_ptr(), 1, SIDE, SIDE, poses_t.data_ptr(), views, FILL, 0,
                                  keys.data_ptr(), out.data_ptr(), mp, stream)
            assert rc == 0, rc

        def floor():
            dst.copy_(src)
            keys.zero_()
        entry(mask.data_ptr())
        holes = [int((mask == v).sum()) for v in (1, 2)]
        offers = offers_inside(torch, d, f, poses)
        for _ in range(2):
            timed(entry, iters), timed(floor, iters)
        tk, tc = [], []
        for _ in range(reps):
            tk.append(timed(entry, iters))
            tc.append(timed(floor, iters))
        # the two launches, apart: outside the timed region, one call per reading
        _native.profile_enable(dev, True)
        splat, resolve = [], []
        for _ in range(reps):
            entry()
            a, b = _native.profile_last_ms(dev)
            splat.append(a * 1e3)
            resolve.append(b * 1e3)
        _native.profile_enable(dev, False)
        k, s = statistics.median(tk), statistics.median(splat)
        print(f"    offers inside the image: {offers / targets:.3f} per source pixel and view; holes: {100 * holes[0] / targets:.2f} % of the targets filled, "
              f"{100 * holes[1] / targets:.3f} % not filled\n"
              f"        ds_parallax_u8 (memset + splat + resolve)    {med(tk)}\n"
              f"        copy of the output's bytes + key-buffer clear {med(tc)}   (ratio {k / statistics.median(tc):.2f})\n"
              f"        splat launch alone                            {med(splat)}   = {8 * offers / (s * 1e-6) / 1e12:.2f} TB/s of offered key bytes\n"
              f"        resolve launch alone                          {med(resolve)}\n"
              f"        {k * 1e-6 / targets * 1e12:.1f} ps per target pixel; {k / views:.1f} us per view", flush=True)
        del im, d


def model_time():
    import numpy as np
    import parallax_cases as pc
    from src import _native
    poses = _native.parallax_poses(PATH, 24, SHIFT[0], SHIFT[1], ZOOM).tolist()
    for what, image, depth in inputs(np, 256):
        t0 = time.perf_counter()
        pc.model(image[0], depth[0], FOCUS, poses, FILL)
        print(f"NumPy model on the host CPU, 256 x 256 x 24 views, {what}: {time.perf_counter() - t0:.2f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.model:
        model_time()
        return 0
    if args.child:
        measure(args.reps, args.iters, args.views)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--iters", str(args.iters), "--views", str(args.views)]
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
