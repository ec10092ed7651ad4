#!/usr/bin/env python3
"""Video mode's two kernels (csrc/ds_video.hip) on a clip of 64 frames of 1080p, one fresh process per side, the sides alternating
`--rounds` times so that the spread between two processes of the SAME side is on the page beside the difference between the sides.
    python tools/video_cuts_ab.py [--frames 64] [--height 1080] [--width 1920] [--reps 20] [--rounds 2]
(a) ds_frame_luma_hist on uint8 RGB frames: HIP events around `--reps` calls after warm-up; the bytes it must read (the clip) plus the
    1 KiB per frame it writes, over the time, against the HBM figures of benchlib/rooflines.py.  Two inputs: seeded noise, and a clip of
    one colour (every pixel of a wave in one bin).
(b) 'experimental' smoothening without cuts on float32 device predictions: the kernel route against DS_VIDEO_SMOOTH=0 (the five torch
    passes over a haloed copy).  Timed twice per side: the temporal filter alone (what the switch changes), and the whole
    process_predictions_sharded call (filter + the exact percentiles by bisection + the float64 normalisation, the same on both
    sides).  The parent also checks that both sides returned the same bits (a checksum of the result's bit patterns).
Prints one line per child and a summary; exit status 1 when the two sides' results differ."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _event_ms(torch, fn, reps, warm=3):
    """Every call timed on its own: [ms] * reps."""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def child(args):
    for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd")):
        sys.path.insert(0, p)
    import torch
    from benchlib.rooflines import HBM_COPY_GBPS, HBM_PEAK_GBPS
    from src import _native, video_mode
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing to measure")
    n, h, w = args.frames, args.height, args.width
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"side": args.child}
    if args.child == "hist":
        nbytes = n * h * w * 3 + n * 1024
        for name, frames in (("noise", torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)),
                             ("one colour", torch.full((n, h, w, 3), 90, dtype=torch.uint8, device="cuda"))):
            out = torch.empty((n, 256), dtype=torch.int32, device="cuda")
            st = _stats(_event_ms(torch, lambda: _native.frame_luma_hist(frames, out=out), args.reps))
            assert int(out.to(torch.int64).sum()) == n * h * w
            st.update(bytes=nbytes, gbps=nbytes / st["median_ms"] / 1e6, frac_of_copy=nbytes / st["median_ms"] / 1e6 / HBM_COPY_GBPS,
                      frac_of_spec=nbytes / st["median_ms"] / 1e6 / HBM_PEAK_GBPS)
            res[name] = st
    else:
        assert (os.environ.get("DS_VIDEO_SMOOTH") == "0") == (args.child == "torch")
        local = torch.randn((n, h, w), dtype=torch.float32, device="cuda", generator=g) * 2.0 + 3.0

        def passes():                                            # the torch route's filter, as process_predictions_sharded runs it
            ext = torch.cat((torch.stack([local[0]] * 2), local, torch.stack([local[-1]] * 2)), dim=0)
            processed = torch.zeros_like(local)
            for u, mul in enumerate([0.10, 0.20, 0.40, 0.20, 0.10]):
                processed += mul * ext[u:u + n]
            return processed
        filt = (lambda: _native.temporal_smooth5(local, 0, n, 0, n - 1)) if args.child == "kernel" else passes
        res["filter"] = _stats(_event_ms(torch, filt, args.reps))
        res["filter"]["bytes_2_planes"] = 2 * local.numel() * 4
        before = _native.CALLS["ds_temporal_smooth5_f32"]
        res["call"] = _stats(_event_ms(torch, lambda: video_mode.process_predictions_sharded(local, "experimental", group=video_mode._LOCAL),
                                       max(args.reps // 4, 3), warm=1))
        res["kernel_launches_per_call"] = (_native.CALLS["ds_temporal_smooth5_f32"] - before) / (max(args.reps // 4, 3) + 1)
        out = video_mode.process_predictions_sharded(local, "experimental", group=video_mode._LOCAL)
        res["checksum"] = [int(filt().view(torch.int32).to(torch.int64).sum()), int((out.view(torch.int64) >> 11).sum())]
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", choices=["hist", "kernel", "torch"])
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    for side in ["hist"] + ["kernel", "torch"] * args.rounds:
        env = dict(os.environ)
        env.pop("DS_VIDEO_SMOOTH", None)
        if side == "torch":
            env["DS_VIDEO_SMOOTH"] = "0"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", side] + [a for k in ("frames", "height", "width", "reps")
                                                                               for a in ("--" + k, str(getattr(args, k)))]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=600)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout)
            print(f"child {side} failed with status {p.returncode}: stopping", flush=True)
            return 2
        runs.append(json.loads(line[-1][7:]))
        print(json.dumps(runs[-1]), flush=True)
    shape = f"{args.frames} x {args.height} x {args.width}"
    hist = runs[0]
    for name in ("noise", "one colour"):
        s = hist[name]
        print(f"(a) ds_frame_luma_hist, {shape} x 3 uint8, {name}: median {s['median_ms']:.3f} ms (min {s['min_ms']:.3f}, max {s['max_ms']:.3f}, "
              f"n {s['n']}); {s['bytes'] / 1e6:.1f} MB -> {s['gbps']:.0f} GB/s = {100 * s['frac_of_copy']:.0f} % of a float4 copy, "
              f"{100 * s['frac_of_spec']:.0f} % of the HBM spec peak")
    k = [r for r in runs if r["side"] == "kernel"]
    t = [r for r in runs if r["side"] == "torch"]
    for what in ("filter", "call"):
        km, tm = [r[what]["median_ms"] for r in k], [r[what]["median_ms"] for r in t]
        print(f"(b) {what}, {shape} float32: kernel route medians per process {['%.3f' % x for x in km]} ms, DS_VIDEO_SMOOTH=0 "
              f"{['%.3f' % x for x in tm]} ms (min/max inside a process: kernel {min(r[what]['min_ms'] for r in k):.3f}/"
              f"{max(r[what]['max_ms'] for r in k):.3f}, torch {min(r[what]['min_ms'] for r in t):.3f}/{max(r[what]['max_ms'] for r in t):.3f}); "
              f"torch / kernel = {statistics.median(tm) / statistics.median(km):.2f}x")
    fb = k[0]["filter"]["bytes_2_planes"]
    print(f"    the filter's two clip-sized transfers are {fb / 1e6:.0f} MB: kernel {fb / statistics.median(r['filter']['median_ms'] for r in k) / 1e6:.0f} GB/s; "
          f"kernel launches per call: kernel route {k[0]['kernel_launches_per_call']:.0f}, DS_VIDEO_SMOOTH=0 {t[0]['kernel_launches_per_call']:.0f}")
    same = all(r["checksum"] == k[0]["checksum"] for r in k + t)
    print("    results of the two routes (filter output and normalised clip, checksums of the bit patterns): " + ("equal" if same else "DIFFER"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
