#!/usr/bin/env python3
"""The funnel on custom depth maps (no model: BASELINE config 1, video mode's second pass) with the ingest of the depth maps on the
host (DS_CUSTOM_DEPTH_DEVICE=0: Pillow's LANCZOS resize, np.asarray(dtype=float), max and divide per image on the host thread,
float64 planes across the link) against the ingest on the device (csrc/ds_resample.hip), alternating off, on, off, on ... in one
process: `--reps` pairs of one funnel call each after one warm-up call per route.
    python tools/custom_depth_ab.py [--images 32] [--size 1024] [--depth-size 512] [--reps 4]
One setting per process: run it once with --depth-size equal to --size (no resize) and once with a smaller one.  Prints the wall
time of every call (the call ends with its last PIL result on the host), median / min / max per route, the depth maps each route
ingested where (core.FUNNEL_STATS), and whether the two routes yielded the same bytes.  Inputs are seeded: random RGB images, smooth
I;16 depth maps with a few occluders, stereo (left-right) and normal map on."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402
import util  # noqa: E402
from src import core  # noqa: E402

OPTS = {'gen_stereo': True, 'gen_normalmap': True, 'stereo_modes': ['left-right']}


def inputs(n, size, depth_size):
    rng = np.random.default_rng(0)
    images = [Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)) for _ in range(n)]
    f = util.smooth_depth(depth_size, depth_size, 1)
    base = ((f - f.min()) / (f.max() - f.min()) * 65535.0).astype(np.uint16)
    depthmaps = [Image.fromarray(np.roll(base, 7 * j, axis=1)) for j in range(n)]
    assert depthmaps[0].mode == "I;16"
    return images, depthmaps


def call(images, depthmaps, device_route):
    core.CUSTOM_DEPTH_DEVICE = device_route
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = list(core.core_generation_funnel(None, list(images), list(depthmaps), None, OPTS))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res, dict(core.FUNNEL_STATS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--depth-size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=4)
    args = ap.parse_args()
    images, depthmaps = inputs(args.images, args.size, args.depth_size)
    first = {}
    for route in (False, True):                                   # warm-up: code objects, pinned staging, Pillow's block arena
        _, res, stats = call(images, depthmaps, route)
        first[route] = ([(i, k, r.tobytes()) for i, k, r in res], stats)
    same = first[False][0] == first[True][0]
    t = {False: [], True: []}
    for _ in range(args.reps):
        for route in (False, True):
            ms, _, stats = call(images, depthmaps, route)
            t[route].append(ms)
        print(f"  [{args.depth_size}^2 -> {args.size}^2] host ingest {t[False][-1]:9.2f} ms   device ingest {t[True][-1]:9.2f} ms", flush=True)
    off, on = t[False], t[True]
    print(f"{args.images} x {args.size}^2 RGB, I;16 depth maps at {args.depth_size}^2, stereo + normal map; per funnel call: "
          f"host ingest median {statistics.median(off):.2f} ms (min {min(off):.2f}, max {max(off):.2f}), device ingest median "
          f"{statistics.median(on):.2f} ms (min {min(on):.2f}, max {max(on):.2f}); speed-up {statistics.median(off) / statistics.median(on):.2f}x; "
          f"pairs/s {args.images / statistics.median(off) * 1e3:.0f} -> {args.images / statistics.median(on) * 1e3:.0f}; depth maps ingested "
          f"(device, host): switch off {first[False][1].get('custom_depth_device', 'n/a'), first[False][1].get('custom_depth_host', 'n/a')}, "
          f"on {first[True][1].get('custom_depth_device', 'n/a'), first[True][1].get('custom_depth_host', 'n/a')}; "
          f"{len(first[True][0])} results per call, the two routes' bytes {'equal' if same else 'DIFFER'}")
    core.CUSTOM_DEPTH_DEVICE = True
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
