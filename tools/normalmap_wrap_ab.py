#!/usr/bin/env python3
"""The wrap-around border mode of the normal-map kernels (create_normalmap_batch(wrap=True): ds_normalmap_wrap) against the
reference's borders (wrap=False: ds_normalmap, whose kernels are the parent commit's instruction for instruction), alternating in one
process, `--reps` pairs of `--iters` launches each.
    python tools/normalmap_wrap_ab.py [--reps 5] [--iters 20]
Cases: uint16, 32 x 1024^2, Sobel 3 and np.gradient (the fused four-pixel kernel: timed by the library's own DS_KT_NORMALMAP kernel
timer, i.e. an event pair around the one launch), and the general path blur 5 / Sobel 5 / blur 5 at 8 x 1024^2 (15 launches of the
separable float64 passes, which the kernel timer does not bracket: a device event pair around the calls).  The measuring runs in a
child process under a time limit; if it fails or runs out of time nothing more is started on the device.  Prints the per-launch
(per-call) time of each route per pair, then median / min / max, and whether wrap equals the non-wrap result away from the border."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd")):
    sys.path.insert(0, p)

CHILD_SECONDS = 240
CASES = [("sobel 3, 32 x 1024^2 (fused4)", 32, (0, 3, 0), True),
         ("np.gradient, 32 x 1024^2 (fused4)", 32, (0, 0, 0), True),
         ("blur 5 / sobel 5 / blur 5, 8 x 1024^2 (separable passes)", 8, (5, 5, 5), False)]


def measure(reps, iters):
    import torch
    from src import _native
    import src.normalmap_generation as nm
    dev = torch.cuda.current_device()
    print(f"normalmap_wrap_ab on {torch.cuda.get_device_name(dev)}: {reps} pairs of {iters} launches", flush=True)
    import numpy as np
    rng = np.random.default_rng(5)
    for what, n, opt, fused in CASES:
        d = torch.from_numpy(rng.integers(0, 65536, (n, 1024, 1024), dtype=np.uint16)).cuda()

        def run(wrap):
            return nm.create_normalmap_batch(d, opt[0], opt[1], opt[2], False, wrap=wrap)

        def timed(wrap):
            if fused:                                   # the library's timer: one event pair around each kernel launch
                _native.kernel_timer_enable(dev, True)
                for _ in range(iters):
                    run(wrap)
                k, ms = _native.kernel_timer_read(dev, "normalmap")
                _native.kernel_timer_enable(dev, False)
                assert k == iters, (k, iters)
                return ms / k
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(iters):
                run(wrap)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / iters
        for wrap in (False, True):
            for _ in range(3):
                run(wrap)
        r = sum(k // 2 for k in opt if k) + (0 if opt[1] else 1)           # summed radii (sobel 0: np.gradient, radius 1)
        yw, yr = run(True), run(False)
        inner = torch.equal(yw[:, r:-r, r:-r], yr[:, r:-r, r:-r])
        ring = not torch.equal(yw, yr)
        tw, tr = [], []
        for _ in range(reps):
            tr.append(timed(False))
            tw.append(timed(True))
            print(f"  [{what}] reflect {tr[-1] * 1e3:9.2f} us   wrap {tw[-1] * 1e3:9.2f} us", flush=True)
        print(f"{what}: reflect median {statistics.median(tr) * 1e3:.2f} us (min {min(tr) * 1e3:.2f}, max {max(tr) * 1e3:.2f}), "
              f"wrap median {statistics.median(tw) * 1e3:.2f} us (min {min(tw) * 1e3:.2f}, max {max(tw) * 1e3:.2f}); "
              f"wrap / reflect {statistics.median(tw) / statistics.median(tr):.4f}; equal {r} pixels from the border: {inner}, "
              f"different on the border: {ring}", flush=True)
        del d, yw, yr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
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
