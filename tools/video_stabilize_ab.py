#!/usr/bin/env python3
"""Video mode's temporal depth filter (csrc/ds_video.hip, ds_temporal_joint_bilateral_u16) on a clip of 64 frames of 1080p, at radius 2
and radius 4, one fresh process per side, the sides alternating `--rounds` times so that the spread between two processes of the SAME
side is on the page beside the difference between the sides.
    python tools/video_stabilize_ab.py [--frames 64] [--height 1080] [--width 1920] [--reps 20] [--rounds 2] [--content mixed|static|noise]
        [--out profiles/video_stabilize_ab.txt]
Side A, "kernel": one launch for the whole clip (video_mode.stabilize_depth's device route).
Side B, "torch":  the same filter as float64 torch ops on the device (video_mode._stabilize_torch: the route CPU tensors take).
Every process also times a device-to-device copy of (c + 2 + 2) * H * W * F bytes -- the bytes the filter must move at the least: every
guide byte and every depth value read once, every output value written once -- as the yardstick of that process and that moment.  The
copy reads AND writes its size, so its rate is 2 * size / time; the filter's rate is its least traffic / time.
HIP events around every call after warm-up.  The parent checks that both sides returned the same bits (a checksum of the uint16
results), prints one line per child and a summary, and writes the summary to --out; exit status 1 when the results differ, 2 when a
child failed (nothing more is started then)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = (2, 4)
SIGMAS = {2: (12.0, 1.5), 4: (12.0, 2.5)}                 # the documented mild and strong settings


def _event_ms(torch, fn, reps, warm=2):
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


def make_clip(torch, n, h, w, c, device, content="mixed"):
    """A seeded clip with a static background under +-3 levels of colour noise (small k: the weights of a static region) and a band of
    white noise that changes every frame (k all over 0..765: the LDS gather at its worst) over the middle third of the rows; depth is a
    ramp plus +-300 levels of noise per pixel and frame.  content 'static': no band; 'noise': the band is the whole frame."""
    g = torch.Generator(device=device).manual_seed(0)
    base = torch.randint(20, 236, (1, h, w, c), dtype=torch.int16, device=device, generator=g)
    frames = (base + torch.randint(-3, 4, (n, h, w, c), dtype=torch.int16, device=device, generator=g)).to(torch.uint8)
    r0, r1 = {"mixed": (h // 3, 2 * h // 3), "static": (0, 0), "noise": (0, h)}[content]
    if r1 > r0:
        frames[:, r0:r1] = torch.randint(0, 256, (n, r1 - r0, w, c), dtype=torch.uint8, device=device, generator=g)
    ramp = 20000 + 10 * torch.arange(w, device=device).view(1, 1, w) + 5 * torch.arange(h, device=device).view(1, h, 1)
    depth = (ramp + torch.randint(-300, 301, (n, h, w), device=device, generator=g)).to(torch.int16).view(torch.uint16)      # modulo 2^16
    return frames, depth


def child(args):
    for p in (ROOT, os.path.join(ROOT, "stable-diffusion-webui-depthmap-script_amd")):
        sys.path.insert(0, p)
    import torch
    from src import _native, video_mode
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing to measure")
    n, h, w, c = args.frames, args.height, args.width, 3
    frames, depth = make_clip(torch, n, h, w, c, "cuda", args.content)
    traffic = (c + 2 + 2) * h * w * n
    src = torch.empty(traffic, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    res = {"side": args.child, "traffic_bytes": traffic}
    res["copy"] = _stats(_event_ms(torch, lambda: dst.copy_(src), args.reps))
    for radius in RADII:
        params = (radius,) + SIGMAS[radius]
        if args.child == "kernel":
            before = _native.CALLS["ds_temporal_joint_bilateral_u16"]
            fn = lambda: video_mode.stabilize_depth(frames, depth, params)                                 # noqa: E731
            st = _stats(_event_ms(torch, fn, args.reps))
            st["launches_per_call"] = (_native.CALLS["ds_temporal_joint_bilateral_u16"] - before) / (args.reps + 2)
        else:
            wt, wc = _native.stabilize_tables_on(depth.device, *params)
            fn = lambda: video_mode._stabilize_torch(depth, frames, radius, wt, wc, 0, n, 0, n - 1)        # noqa: E731
            st = _stats(_event_ms(torch, fn, max(args.reps // 4, 3), warm=1))
        out = fn()
        st["checksum"] = int(out.view(torch.int16).to(torch.int64).sum()) ^ int((out.view(torch.int16).to(torch.int64)[:, ::7, ::5] * 3).sum())
        st["changed"] = float((out.view(torch.int16) != depth.view(torch.int16)).float().mean())
        res["r%d" % radius] = st
        del out
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--content", choices=["mixed", "static", "noise"], default="mixed", help="what the frames show (see make_clip)")
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_stabilize_ab.txt"))
    ap.add_argument("--child", choices=["kernel", "torch"])
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    for side in ["kernel", "torch"] * args.rounds:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", side] + [a for k in ("frames", "height", "width", "reps", "content")
                                                                               for a in ("--" + k, str(getattr(args, k)))]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
        except subprocess.TimeoutExpired:
            print(f"child {side} ran into its time limit of {args.child_timeout} s: stopping", flush=True)
            return 2
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout)
            print(f"child {side} failed with status {p.returncode}: stopping", flush=True)
            return 2
        runs.append(json.loads(line[-1][7:]))
        print(json.dumps(runs[-1]), flush=True)
    n = args.frames
    k = [r for r in runs if r["side"] == "kernel"]
    t = [r for r in runs if r["side"] == "torch"]
    traffic = k[0]["traffic_bytes"]
    lines = [f"tools/video_stabilize_ab.py: {n} frames of {args.height} x {args.width} x 3 uint8 ({args.content}) + uint16 depth; {args.rounds} processes per side, "
             f"alternating; HIP events around each call; medians per process",
             f"least traffic of the filter (3 + 2 + 2) * H * W * F = {traffic / 1e6:.1f} MB"]
    cm = [r["copy"]["median_ms"] for r in runs]
    copy_ms = statistics.median(cm)
    lines.append(f"device-to-device copy of {traffic / 1e6:.1f} MB (reads and writes that much): medians per process {['%.3f' % x for x in cm]} ms "
                 f"-> {1e3 * copy_ms / n:.1f} us per frame, {2 * traffic / copy_ms / 1e6:.0f} GB/s of traffic")
    same = True
    for radius in RADII:
        key = "r%d" % radius
        km, tm = [r[key]["median_ms"] for r in k], [r[key]["median_ms"] for r in t]
        kmed, tmed = statistics.median(km), statistics.median(tm)
        share = (traffic / kmed) / (2 * traffic / copy_ms)
        lines.append(f"radius {radius}, sigmas {SIGMAS[radius]}: kernel {['%.3f' % x for x in km]} ms (min/max inside a process "
                     f"{min(r[key]['min_ms'] for r in k):.3f}/{max(r[key]['max_ms'] for r in k):.3f}) -> {1e3 * kmed / n:.1f} us per frame, "
                     f"{traffic / kmed / 1e6:.0f} GB/s = {100 * share:.0f} % of the copy's rate; torch ops {['%.1f' % x for x in tm]} ms -> "
                     f"{1e3 * tmed / n:.1f} us per frame; torch / kernel = {tmed / kmed:.1f}x; {k[0][key]['launches_per_call']:.0f} launch per call; "
                     f"{100 * k[0][key]['changed']:.0f} % of the values changed")
        same = same and all(r[key]["checksum"] == k[0][key]["checksum"] for r in k + t)
    lines.append("results of the two sides (checksums of the uint16 output): " + ("equal" if same else "DIFFER"))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
