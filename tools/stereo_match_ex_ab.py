#!/usr/bin/env python3
"""Eight paths and the speckle filter of ds_stereo_match_ex_u8 beside the launches they join, on the pairs, sizes and D of
tools/stereo_match_ab.py (one 1024 x 1024 pair, one 1080 x 960 pair; D = 64 and 128), `--reps` rounds of `--iters` calls each.
    python tools/stereo_match_ex_ab.py [--reps 5] [--iters 5]
The protocol is that tool's: a stream-event pair around a round of `--iters` calls of the C entry point, medians over the rounds, and
as the yardstick, in the same process and alternating, one device-to-device copy of the S volume's bytes.  Timed: the whole call at 4
paths (ds_stereo_match_u8), at 8 paths, and at 8 paths with the filter at the documented starting point (64, 1); then, through
ds_stereo_match_ex_stages_u8, the vertical launch, the two diagonal launches (one `stages` bit names both, so the figure is halved; the
comparison for a diagonal launch is the vertical launch of the same run, which makes the same steps), the winner launch that stops
before its fill, and the filter's four launches together with the row fill; and ds_speckle_filter_i16 alone on the same disp16 and
mask, so that the fill is the difference.  The filter's times depend on the mask (how far the links reach), so they are shown per
input; the path launches' do not.  Beside the times, for every pair: the share of pixels whose disparity is within 1 pixel of the
applied one at 4 and 8 paths, without and with the filter -- a recorded observation, not a bar.  Bit-exactness is the tests' business.
The measuring runs in a child process under a time limit; if it fails or runs out of time nothing more is started on the device."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

CHILD_SECONDS = 420
PRESET = (8, 64, 1)


def measure(reps, iters):
    import numpy as np
    import torch
    from src import _native
    import stereo_match_ab as ab
    dev = torch.cuda.current_device()
    L, ctx = _native.lib(), _native.ctx_for(dev)
    stream = torch.cuda.current_stream().cuda_stream
    print(f"stereo_match_ex_ab on {torch.cuda.get_device_name(dev)}: {reps} rounds of {iters} calls, d0 P1 P2 u lr = {ab.PARAMS}, "
          f"filter (size, range) = {PRESET[1:]}, library {os.path.basename(_native.LIB_PATH)}", flush=True)

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

    def rounds(fn):
        timed(fn, iters)
        return [timed(fn, iters) for _ in range(reps)]
    for h, w in ab.SIZES:
        pairs = ab.inputs(np, h, w)
        for D in ab.DISPARITIES:
            s_bytes = 2 * h * w * D
            src = torch.zeros((s_bytes,), dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            ws = torch.empty((_native.stereo_match_ex_workspace_bytes(h, w, D, 8, PRESET[1]),), dtype=torch.uint8, device="cuda")
            sp_ws = torch.empty((_native.speckle_filter_workspace_bytes(h, w),), dtype=torch.uint8, device="cuda")
            disparity = torch.empty((1, h, w), dtype=torch.int16, device="cuda")
            valid = torch.empty((1, h, w), dtype=torch.uint8, device="cuda")
            valid2 = torch.empty((1, h, w), dtype=torch.uint8, device="cuda")
            depth = torch.empty((1, h, w), dtype=torch.uint16, device="cuda")
            for what, left, right, truth in pairs:
                lt, rt = torch.from_numpy(np.array(left, order='C')).cuda()[None], torch.from_numpy(np.array(right, order='C')).cuda()[None]
                print(f"[1 x {h} x {w}, D = {D}: {what}]", flush=True)

                def run(e, stages=255):
                    rc = L.ds_stereo_match_ex_stages_u8(ctx, lt.data_ptr(), rt.data_ptr(), 1, h, w, 3, D, *ab.PARAMS, *e, ws.data_ptr(), 1,
                                                        disparity.data_ptr(), valid.data_ptr(), depth.data_ptr(), stages, stream)
                    assert rc == 0, rc

                def old():
                    rc = L.ds_stereo_match_u8(ctx, lt.data_ptr(), rt.data_ptr(), 1, h, w, 3, D, *ab.PARAMS, ws.data_ptr(), 1, disparity.data_ptr(),
                                              valid.data_ptr(), depth.data_ptr(), stream)
                    assert rc == 0, rc

                def floor():
                    dst.copy_(src)
                # the shares first: they double as the warm-up
                for e in ((4, 0, 0), (4,) + PRESET[1:], (8, 0, 0), PRESET):
                    run(e)
                    got = disparity[0].cpu().numpy().astype(np.float64) / 16.0
                    ok = valid[0].cpu().numpy() == 1
                    near = np.abs(got - truth) <= 1.0
                    print(f"        paths {e[0]}, filter {'on ' if e[1] else 'off'}: valid {100.0 * ok.mean():5.1f} %;  within 1 px of the applied disparity: "
                          f"{100.0 * near.mean():5.1f} % of all, {100.0 * near[ok].mean() if ok.any() else 0.0:5.1f} % of the valid", flush=True)
                tc = []
                calls = (("ds_stereo_match_u8 (4 paths)", old), ("ex, 8 paths", lambda: run((8, 0, 0))), ("ex, 8 paths + filter", lambda: run(PRESET)))
                times = {name: [] for name, _ in calls}
                for name, fn in calls:
                    timed(fn, iters)
                timed(floor, iters)
                for _ in range(reps):
                    for name, fn in calls:
                        times[name].append(timed(fn, iters))
                    tc.append(timed(floor, iters))
                c = statistics.median(tc)
                for name, _ in calls:
                    print(f"        {name:30s} {med(times[name])}   ({statistics.median(times[name]) / c:.1f} copies of S)", flush=True)
                print(f"        one copy of the S volume ({s_bytes / 2**20:4.0f} MiB) {med(tc)}", flush=True)
                run(PRESET)                                                    # leaves disp16 and the mask of step 7 in the workspace
                tv = rounds(lambda: run(PRESET, 4))
                td = [t / 2 for t in rounds(lambda: run(PRESET, 64))]
                v, d = statistics.median(tv), statistics.median(td)
                print(f"          vertical paths                 {med(tv)}\n"
                      f"          one diagonal launch (of two)   {med(td)}   ({d / v:.2f} of the vertical launch)", flush=True)
                run(PRESET)
                tw = rounds(lambda: run(PRESET, 8))
                tf = rounds(lambda: run(PRESET, 128))
                run((8, 0, 0))                                                 # disparity and valid: an input of the same kind for the filter alone

                def alone():
                    rc = L.ds_speckle_filter_i16(ctx, disparity.data_ptr(), valid.data_ptr(), 1, h, w, PRESET[1], 16 * PRESET[2], sp_ws.data_ptr(), 1,
                                                 valid2.data_ptr(), None, stream)
                    assert rc == 0, rc
                ta = rounds(alone)
                print(f"          winner, stopping before its fill {med(tw)}\n"
                      f"          filter (4 launches) + row fill  {med(tf)}\n"
                      f"          ds_speckle_filter_i16 alone     {med(ta)}   (so the row fill is about "
                      f"{statistics.median(tf) - statistics.median(ta):.1f} us)", flush=True)
                del lt, rt
            del src, dst, ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
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
