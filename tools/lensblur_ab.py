#!/usr/bin/env python3
"""The lens-blur kernel (ds_lensblur_u8: the depth-of-field gather of an image by its uint16 depth map) beside a device copy of the
bytes a pass moves, on 1024 x 1024 maps, for (radius, aperture) = (8, 32), (16, 64), (32, 128), `--reps` rounds of `--iters` calls each.
    python tools/lensblur_ab.py [--reps 5] [--iters 20] [--maps 1]
    python tools/lensblur_ab.py --model           (host only: needs no GPU)
The kernel has no kernel-timer kind: it is timed by a stream-event pair around `--iters` calls of the C entry point (no Python between
two launches but the ctypes call), the copy -- 4 B per pixel read and as much written: the 8 B per pixel of a pass that reads the
image and the depth and writes the image -- by an event pair in the same process, alternating.
Three inputs: a depth-map-like one (smooth ramp, +-3 levels of noise, one cliff, focus on the near plane), an all-in-focus one (a flat
map at its focus depth: every workgroup visits the self tap alone, which is what leaving out taps that cannot count buys) and
full-range white noise (nearly every rho at its clamp: every tap of the largest disc is visited).
Printed per row: the taps a pixel VISITS (exact: from the kernel's own rho output, per tile (64 x --tile-height) the disc of the largest rho in the
tile and its halo) and the taps that COUNT (exact: the definition's test, as torch passes on the device after the timing), the time per
pixel and visited tap and per pixel and counted tap, and the visited taps a CU retires per clock, 256 CUs at 2.4 GHz.
--maps n times a batch of n maps in one launch (one 1024 x 1024 map is 512 workgroups, two per CU).
Bit-exactness against the NumPy model is tests/test_gpu_lensblur.py's business.  --model times the NumPy model of
tests/lensblur_cases.py on one 256 x 256 map on the host, as context.  The measuring runs in a child process under a time limit; if it
fails or runs out of time nothing more is started on the device.  DS_NATIVE_LIB=<path> times another build of the library
(ds_lensblur.hip compiled with -DLB_TH=16: pass --tile-height 16)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

CHILD_SECONDS = 420
SIDE = 1024
ROWS = ((8, 32.0), (16, 64.0), (32, 128.0))
CUS, CLOCK = 256, 2.4e9
TW = 64


def inputs(np, side=SIDE, maps=1):
    """[(name, image, depth, focus per map)]"""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:side, 0:side]
    image = rng.integers(0, 256, (maps, side, side, 3), dtype=np.uint8)
    near = x >= side // 2
    ramp = (12000 + (8 * x + 5 * y) * 1024 // side + np.where(near, 16384, 0))[None] + rng.integers(-3, 4, (maps, side, side))
    return [("depth-map-like (ramp + noise + cliff, focus on the near plane)", image, ramp.astype(np.uint16), [int(ramp[m][near].min()) + 4000 for m in range(maps)]),
            ("all in focus (flat map at its focus depth)", image, np.full((maps, side, side), 30000, np.uint16), [30000] * maps),
            ("white noise", image, rng.integers(0, 65536, (maps, side, side), dtype=np.uint16), [32768] * maps)]


def visited_taps(np, coc, radius, TH):
    """Taps the kernel visits, summed over the pixels of one map: per tile the disc of the largest rho in the tile and its halo."""
    h, w = coc.shape
    padded = np.pad(coc, radius)
    dy, dx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    d2 = 16 * (dx * dx + dy * dy)
    total = 0
    for y0 in range(0, h, TH):
        for x0 in range(0, w, TW):
            top = int(padded[y0:y0 + TH + 2 * radius, x0:x0 + TW + 2 * radius].max())
            total += int((d2 <= top * top).sum()) * min(TH, h - y0) * min(TW, w - x0)
    return total


def counted_taps(torch, depth_u16, coc_u8, radius):
    """Taps that count, summed over the pixels of one map [h, w]: the definition's test, one pass per offset, on the device."""
    F = torch.nn.functional
    h, w = coc_u8.shape
    z = depth_u16.view(torch.int16).to(torch.int32) & 0xffff
    rho = coc_u8.to(torch.int32)
    zq_all, rq_all = F.pad(z, (radius,) * 4), F.pad(rho, (radius,) * 4)
    in_all = F.pad(torch.ones_like(rho, dtype=torch.bool), (radius,) * 4)
    total = torch.zeros((), dtype=torch.int64, device=rho.device)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            d2 = dx * dx + dy * dy
            if d2 > radius * radius:
                continue
            win = (slice(radius + dy, radius + dy + h), slice(radius + dx, radius + dx + w))
            rq = rq_all[win]
            rho_e = torch.where(zq_all[win] < z, torch.minimum(rq, rho), rq)
            total += (in_all[win] & (rho_e * rho_e >= 16 * d2)).sum()
    return int(total)


def measure(reps, iters, maps, tile_height):
    import numpy as np
    import torch
    from src import _native
    dev = torch.cuda.current_device()
    L, ctx = _native.lib(), _native.ctx_for(dev)
    print(f"lensblur_ab on {torch.cuda.get_device_name(dev)}: {maps} x {SIDE} x {SIDE}, {reps} rounds of {iters} calls, library {os.path.basename(_native.LIB_PATH)}",
          flush=True)

    def med(v):
        return f"median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})"
    src = torch.zeros((maps * SIDE * SIDE * 4,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters * 1e3
    for what, image, depth, focus in inputs(np, maps=maps):
        im, d = torch.from_numpy(image).cuda(), torch.from_numpy(depth).cuda()
        f = torch.from_numpy(np.asarray(focus, np.uint16)).cuda()
        print(f"[{what}]", flush=True)
        for radius, aperture in ROWS:
            A = _native.lensblur_quarter_pixels(aperture)
            out, coc = _native.lensblur_u8(im, d, radius, A, 0, f, want_coc=True)          # (uploads the table, warms the kernel up)
            (table,) = _native._tables_on("lensblur", d.device, (radius,), _native.lensblur_table)
            stream = torch.cuda.current_stream().cuda_stream

            def kernel():
                rc = L.ds_lensblur_u8(ctx, im.data_ptr(), d.data_ptr(), f.data_ptr(), maps, SIDE, SIDE, radius, A, 0, 0, table.data_ptr(),
                                      out.data_ptr(), None, stream)
                assert rc == 0, rc

            def copy():
                dst.copy_(src)
            for _ in range(2):
                timed(kernel), timed(copy)
            tk, tc = [], []
            for _ in range(reps):
                tk.append(timed(kernel))
                tc.append(timed(copy))
            k = statistics.median(tk)
            coc0 = coc[0].cpu().numpy()
            visited = visited_taps(np, coc0, radius, tile_height) / (SIDE * SIDE)
            counted = counted_taps(torch, d[0], coc[0], radius) / (SIDE * SIDE)
            per_pixel = k * 1e-6 / (maps * SIDE * SIDE)
            print(f"    R = {radius:2d}, aperture {aperture:5.1f} (per pixel of map 0: {visited:7.1f} taps visited, {counted:7.1f} counted; mean rho {coc0.mean():.1f}, max {coc0.max()})\n"
                  f"        ds_lensblur_u8        {med(tk)}\n"
                  f"        copy moving 8 B/pixel {med(tc)}   (ratio {k / statistics.median(tc):.1f})\n"
                  f"        {per_pixel / visited * 1e12:.3f} ps per pixel and visited tap = {visited / (per_pixel * CUS * CLOCK):.1f} visited taps per CU and clock; "
                  f"{per_pixel / counted * 1e12:.3f} ps per pixel and counted tap", flush=True)
        del im, d


def model_time():
    import numpy as np
    import lensblur_cases as lc
    for what, image, depth, focus in inputs(np, 256):
        for radius, aperture in ROWS:
            t0 = time.perf_counter()
            lc.model(image[0], depth[0], focus[0], radius, lc.quarter_pixels(aperture), 0)
            print(f"NumPy model on the host CPU, 256 x 256 {what}, R = {radius}, aperture {aperture}: {time.perf_counter() - t0:.2f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--maps", type=int, default=1)
    ap.add_argument("--tile-height", type=int, default=32, help="the library's LB_TH (32 as committed): only the count of visited taps uses it")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.model:
        model_time()
        return 0
    if args.child:
        measure(args.reps, args.iters, args.maps, args.tile_height)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--iters", str(args.iters), "--maps", str(args.maps), "--tile-height", str(args.tile_height)]
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
