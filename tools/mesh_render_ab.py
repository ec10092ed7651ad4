#!/usr/bin/env python3
"""The mesh renderer (ds_mesh_render_u8: a memset of keys and counters, then the vertex, face, listed-face and resolve launches) beside
the floor its design cannot beat, on the simple mesh of one 1024 x 1024 image x 24 frames of the 'double-straight-line' path at the
defaults of src/mesh_render.py (shift (0.15, 0, 0.3), one sample per pixel), `--reps` rounds of `--iters` calls each.
    python tools/mesh_render_ab.py [--reps 5] [--iters 5] [--frames 24] [--side 1024] [--ssaa 1]
    python tools/mesh_render_ab.py --model           (host only: needs no GPU)
The entry point is timed by a stream-event pair around `--iters` calls of the C entry point (no Python between two calls but the ctypes
call), once per small_cap in {0, 4, 16, 64}.  The yardstick, by an event pair in the same process, alternating: a clear of one group's
key buffer plus a device-to-device copy of it -- the visibility buffer written once and read once, which any renderer of this design
must do.  Each launch is timed alone OUTSIDE the timed region through ds_mesh_render_stages_u8: one call per reading, the launches it
depends on run untimed in front of it, `--reps` readings, at the binding's default small_cap.
Two meshes of one depth-map-like input (a smooth ramp from 1 to 4 units with a near rectangle at 1.2, +-0.002 of noise): the stretched
mesh (every quad kept: the cliff's quads become long faces under a moved camera) and the occluded one (the cliff's quads removed).
Printed per mesh: vertices, faces, the faces listed for the large path per frame at the default small_cap, and the share of samples
hit.  Bit-exactness against the NumPy model is tests/test_gpu_mesh_render.py's business.  --model times the NumPy model of
tests/mesh_render_cases.py on a 128 x 128 image x 24 frames on the host, as context.  The measuring runs in a child process under a time
limit; if it fails or runs out of time nothing more is started on the device."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

CHILD_SECONDS = 400
TRAJ, SHIFT = 'double-straight-line', (0.15, 0.0, 0.3)
CAPS = (0, 4, 16, 64)


def scene(np, side):
    """(image uint8 [side, side, 3], depth float64 [side, side])"""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:side, 0:side]
    image = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    near = (x >= side // 3) & (x < 2 * side // 3) & (y >= side // 4) & (y < 3 * side // 4)
    depth = np.where(near, 1.2, 1.0 + 3.0 * (8 * x + 5 * y) / (13.0 * side)) + rng.uniform(-0.002, 0.002, (side, side))
    return image, depth


def measure(reps, iters, frames, side, ssaa):
    import numpy as np
    import torch
    from src import _native, mesh_render as mr, mesh_generation as mg
    dev = torch.cuda.current_device()
    L, ctx = _native.lib(), _native.ctx_for(dev)
    H = W = side
    print(f"mesh_render_ab on {torch.cuda.get_device_name(dev)}: the simple mesh of {side} x {side}, {frames} frames ('{TRAJ}', shift {SHIFT}), "
          f"s = {ssaa}, {reps} rounds of {iters} calls, default small_cap {_native.MESH_RENDER_SMALL_CAP}, library {os.path.basename(_native.LIB_PATH)}",
          flush=True)

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
    image, depth = scene(np, side)
    rgb_t, depth_t = torch.from_numpy(image).cuda(), torch.from_numpy(depth).cuda()
    cams = mr._grid_cameras(side, side, H, W, mr.camera_path(TRAJ, frames, *SHIFT), None)
    F = len(cams)
    cams_t = torch.from_numpy(np.array(cams, np.float64, order='C')).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    samples = F * (ssaa * H) * (ssaa * W)
    key_bytes = 8 * samples
    src = torch.zeros((key_bytes,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def floor():
        src.zero_()
        dst.copy_(src)
    for what, keep_edges in (("stretched mesh (keep_edges: every quad kept)", True), ("occluded mesh (the depth edges' quads removed)", False)):
        verts, faces, colors = mg.create_mesh_arrays(rgb_t, depth_t, keep_edges=keep_edges)
        verts, faces, colors = verts.contiguous(), faces.to(torch.int32).contiguous(), colors.contiguous()
        N, M = verts.shape[0], faces.shape[0]
        share = _native.mesh_render_workspace_bytes(N, M, H, W, ssaa)
        ws = torch.empty((F * share,), dtype=torch.uint8, device="cuda")
        out = torch.empty((F, H, W, 3), dtype=torch.uint8, device="cuda")
        hits = torch.empty((F, H, W), dtype=torch.uint8, device="cuda")

        def entry(cap=_native.MESH_RENDER_SMALL_CAP, stages=31, hp=None):
            rc = L.ds_mesh_render_stages_u8(ctx, verts.data_ptr(), colors.data_ptr(), faces.data_ptr(), N, M, cams_t.data_ptr(), F, H, W, ssaa, 0.05,
                                            0, 0, 0, cap, ws.data_ptr(), F, out.data_ptr(), hp, stages, stream)
            assert rc == 0, rc
        entry(hp=hits.data_ptr())
        torch.cuda.synchronize()
        keys_stride = (8 * ssaa * H * ssaa * W + 255) // 256 * 256
        listed = ws[F * keys_stride:F * keys_stride + 256 * F].view(torch.int32).view(F, 64)[:, 0].cpu().numpy()
        hit = float(hits.sum()) / samples
        print(f"[{what}]\n    {N} vertices, {M} faces; listed for the large path per frame: median {int(np.median(listed))}, max {int(listed.max())} "
              f"({100.0 * listed.max() / max(M, 1):.2f} % of the faces); {100 * hit:.1f} % of the samples hit; workspace {F * share / 2**20:.0f} MiB, "
              f"of it keys {key_bytes / 2**20:.0f} MiB", flush=True)
        for _ in range(2):
            timed(entry, iters), timed(floor, iters)
        per_cap = {}
        for cap in CAPS:
            tk, tc = [], []
            for _ in range(reps):
                tk.append(timed(lambda: entry(cap), iters))
                tc.append(timed(floor, iters))
            per_cap[cap] = statistics.median(tk)
            print(f"        ds_mesh_render_u8, small_cap {cap:2d}                   {med(tk)}   clear + copy of the keys {med(tc)}   "
                  f"(ratio {statistics.median(tk) / statistics.median(tc):.2f})", flush=True)
        best = min(per_cap, key=per_cap.get)
        print(f"        fastest small_cap: {best}; {per_cap[best] * 1e-6 / samples * 1e12:.1f} ps per sample; {per_cap[best] / F:.1f} us per frame", flush=True)
        # each launch alone, outside the timed region: what it depends on runs untimed in front of it; one call per reading
        for name, bit, prep in (("memset of keys and counters", 1, 0), ("k_mr_project", 2, 0), ("k_mr_raster", 4, 3), ("k_mr_raster_large", 8, 7),
                                ("k_mr_resolve", 16, 15)):
            t = []
            for _ in range(reps):
                if prep:
                    entry(stages=prep)
                t.append(timed(lambda: entry(stages=bit), 1))
            print(f"        {name:28s} alone          {med(t)}", flush=True)
        del ws, out, hits, verts, faces, colors


def model_time():
    import numpy as np
    import mesh_render_cases as mc
    from src import mesh_render as mr
    image, depth = scene(np, 128)
    for what, keep_edges in (("stretched", True), ("occluded", False)):
        verts, colors, faces = mc.grid_mesh(image, depth, keep_edges)
        cams = mc.cameras_for(mr.camera_path(TRAJ, 24, *SHIFT), *mc.intrinsics(128, 128))
        t0 = time.perf_counter()
        mc.model(verts, colors, faces, cams, 128, 128)
        print(f"NumPy model on the host CPU, 128 x 128 x 24 frames, {what} mesh: {time.perf_counter() - t0:.2f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--ssaa", type=int, default=1)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.model:
        model_time()
        return 0
    if args.child:
        measure(args.reps, args.iters, args.frames, args.side, args.ssaa)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for k in ("reps", "iters", "frames", "side", "ssaa")
                                                                    for a in ("--" + k, str(getattr(args, k)))]
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
