#!/usr/bin/env python3
"""Depth from stereo pairs (ds_stereo_match_u8: census, horizontal paths, vertical paths, winner + fill, median, depth -- six launches)
beside the bytes one path pass must move at the least, on one 1024 x 1024 pair and one 1080 x 960 pair (one half of a 1080p
side-by-side frame), for D = 64 and D = 128, `--reps` rounds of `--iters` calls each.
    python tools/stereo_match_ab.py [--reps 5] [--iters 5]
    python tools/stereo_match_ab.py --model           (host only: needs no GPU)
The entry point is timed by a stream-event pair around `--iters` calls of the C entry point (no Python between two calls but the ctypes
call).  Each launch is timed apart the same way, through ds_stereo_match_stages_u8, which makes only the launches its `stages` argument
names (repeating the vertical pass keeps adding into S, which wraps around in uint16: no address depends on a value, and the time is
the same).  The yardstick, by an event pair in the same process, alternating with the entry point: one device-to-device copy of the S
volume's bytes (h w D 2 read and written once) -- what a single path pass must move at the least while S lives in HBM.
Three inputs: a noise-textured two-plane pair (background at disparity 4, a rectangle at 40); a pair made by the project's own
create_stereoimages (stereo_balance -1: the left view is the image itself, so the disparity the warp applied is known per left
pixel) from a depth-map-like ramp with a near rectangle and a noise-textured image, at a divergence of 48 pixels; and the same with a
flat-colour image, the worst case for matching.  Beside the times, for every pair: the share of valid pixels, and the share of pixels
whose disparity is within 1 pixel of the disparity the warp applied -- a recorded observation, not a bar.  Bit-exactness against the
NumPy model is tests/test_gpu_stereo_match.py's business.  --model times the NumPy model of tests/stereo_match_cases.py on one
96 x 300 pair at D = 64 on the host, as context.  The measuring runs in a child process under a time limit; if it fails or runs out of
time nothing more is started on the device."""
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
SIZES = ((1024, 1024), (1080, 960))
DISPARITIES = (64, 128)
PARAMS = (0, 4, 48, 5, 1)               # d0, P1, P2, u, lr: the defaults
DIVERGENCE_PX = 48
STAGES = (("census", 1), ("horizontal paths", 2), ("vertical paths", 4), ("winner + fill", 8), ("median + min/max", 16), ("depth", 32))


def inputs(np, h, w):
    """[(name, left [h,w,3], right [h,w,3], truth [h,w] in pixels)]; the project-made pairs need the GPU."""
    from src.stereoimage_generation import create_stereoimages
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:h, 0:w]
    near = (x >= w // 3) & (x < 2 * w // 3) & (y >= h // 4) & (y < 3 * h // 4)
    pad, bg_d, fg_d = 64, 4, 40
    bg = rng.integers(0, 256, (h, w + 2 * pad, 3), dtype=np.uint8)
    fg = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    left = np.where(near[:, :, None], fg, bg[:, pad:pad + w])
    shifted = np.zeros((h, w), bool)
    shifted[:, :w - fg_d] = near[:, fg_d:]
    fg_right = np.zeros_like(fg)
    fg_right[:, :w - fg_d] = fg[:, fg_d:]
    right = np.where(shifted[:, :, None], fg_right, bg[:, pad + bg_d:pad + bg_d + w])
    out = [("noise-textured two-plane pair (disparities 4 and 40)", left, right, np.where(near, fg_d, bg_d).astype(np.float64))]
    depth = ((8000 + (16 * x * 1024) // w + (8 * y * 1024) // h + np.where(near, 30000, 0))).astype(np.uint16)
    norm = (depth.astype(np.float64) - depth.min()) / (float(depth.max()) - float(depth.min()))
    for what, image in (("create_stereoimages pair, ramp + near rectangle, noise-textured image", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
                        ("create_stereoimages pair, ramp + near rectangle, flat-colour image", np.full((h, w, 3), 128, np.uint8))):
        sbs = np.asarray(create_stereoimages(image, depth, 100.0 * DIVERGENCE_PX / w, modes=['left-right'], stereo_balance=-1.0)[0])
        out.append((what, sbs[:, :w], sbs[:, w:], norm * DIVERGENCE_PX))
    return out


def measure(reps, iters):
    import numpy as np
    import torch
    from src import _native
    dev = torch.cuda.current_device()
    L, ctx = _native.lib(), _native.ctx_for(dev)
    stream = torch.cuda.current_stream().cuda_stream
    print(f"stereo_match_ab on {torch.cuda.get_device_name(dev)}: {reps} rounds of {iters} calls, d0 P1 P2 u lr = {PARAMS}, "
          f"library {os.path.basename(_native.LIB_PATH)}", flush=True)

    def med(v):
        return f"median {statistics.median(v):9.1f} us (min {min(v):.1f}, max {max(v):.1f})"

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
        pairs = inputs(np, h, w)
        for D in DISPARITIES:
            s_bytes = 2 * h * w * D
            src = torch.zeros((s_bytes,), dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            ws = torch.empty((_native.stereo_match_workspace_bytes(h, w, D),), dtype=torch.uint8, device="cuda")
            disparity = torch.empty((1, h, w), dtype=torch.int16, device="cuda")
            valid = torch.empty((1, h, w), dtype=torch.uint8, device="cuda")
            depth = torch.empty((1, h, w), dtype=torch.uint16, device="cuda")
            for what, left, right, truth in pairs:
                lt, rt = torch.from_numpy(np.array(left, order='C')).cuda()[None], torch.from_numpy(np.array(right, order='C')).cuda()[None]
                print(f"[1 x {h} x {w}, D = {D}: {what}]", flush=True)

                def run(stages):
                    rc = L.ds_stereo_match_stages_u8(ctx, lt.data_ptr(), rt.data_ptr(), 1, h, w, 3, D, *PARAMS, ws.data_ptr(), 1, disparity.data_ptr(),
                                                     valid.data_ptr(), depth.data_ptr(), stages, stream)
                    assert rc == 0, rc

                def entry():
                    rc = L.ds_stereo_match_u8(ctx, lt.data_ptr(), rt.data_ptr(), 1, h, w, 3, D, *PARAMS, ws.data_ptr(), 1, disparity.data_ptr(),
                                              valid.data_ptr(), depth.data_ptr(), stream)
                    assert rc == 0, rc

                def floor():
                    dst.copy_(src)
                for _ in range(2):
                    timed(entry, iters), timed(floor, iters)
                tk, tc = [], []
                for _ in range(reps):
                    tk.append(timed(entry, iters))
                    tc.append(timed(floor, iters))
                k, c = statistics.median(tk), statistics.median(tc)
                got = disparity[0].cpu().numpy().astype(np.float64) / 16.0
                ok = valid[0].cpu().numpy() == 1
                print(f"        ds_stereo_match_u8 (six launches)              {med(tk)}\n"
                      f"        one copy of the S volume ({s_bytes / 2**20:6.0f} MiB r + w)     {med(tc)}   (ratio {k / c:.2f})\n"
                      f"        valid {100.0 * ok.mean():5.1f} %;  within 1 px of the applied disparity: {100.0 * (np.abs(got - truth) <= 1.0).mean():5.1f} % of all, "
                      f"{100.0 * (np.abs(got - truth) <= 1.0)[ok].mean() if ok.any() else 0.0:5.1f} % of the valid;  {k * 1e-6 / (h * w * D) * 1e12:.1f} ps per pixel and disparity",
                      flush=True)
                entry()
                for name, bit in STAGES:
                    timed(lambda: run(bit), iters)
                    ts = [timed(lambda: run(bit), iters) for _ in range(reps)]
                    print(f"          {name:18s} {med(ts)}   ({statistics.median(ts) / c:.2f} copies of S)", flush=True)
                del lt, rt
            del src, dst, ws


def model_time():
    import numpy as np
    import stereo_match_cases as sc
    l, r = sc.pair("planes", (1, 96, 300))
    t0 = time.perf_counter()
    sc.model(l, r, 64, *PARAMS)
    print(f"NumPy model on the host CPU, 96 x 300, D = 64, the two-plane pair: {time.perf_counter() - t0:.2f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
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
