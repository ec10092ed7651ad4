#!/usr/bin/env python3
"""Golden vectors of video mode's per-scene normalisation: the REFERENCE's own ``process_predicitons`` (src/video_mode.py:103-128)
run on every scene of a clip on its own, the results concatenated -- what ``process_predicitons(..., cuts=)`` must return.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_video_cuts.py

Loader, seeds and predictions are make_golden_video's; the reference function runs unmodified.  Output: video_cuts_cases.npz (the
reference outputs per case and mode; the tests regenerate the inputs from the seeds).
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_video as mgv  # noqa: E402

# case of make_golden_video.CASES -> the frames at which a new scene starts
CUTS = {"n12": [1, 4, 9],               # scenes of 1, 3, 5 and 3 frames
        "n9": [2],
        "n7_ties": [3],
        "n5_wide": [1, 2, 3, 4]}        # every frame its own scene


def predictions(name):
    spec = {c[0]: c for c in mgv.CASES}[name]
    return mgv.make_predictions(*spec[1:])


def main():
    vm = mgv.load_reference_video_mode()
    out = {}
    for name, cuts in CUTS.items():
        p = predictions(name)
        bounds = [0] + cuts + [p.shape[0]]
        for mode in ("none", "experimental"):
            parts = []
            for a, b in zip(bounds[:-1], bounds[1:]):
                parts += vm.process_predicitons([x for x in p[a:b]], mode)
            out[f"{name}/{mode}"] = np.stack(parts)
            print(name, mode, out[f"{name}/{mode}"].dtype, out[f"{name}/{mode}"].shape, "finite:", bool(np.isfinite(out[f"{name}/{mode}"]).all()))
    np.savez_compressed(os.path.join(HERE, "video_cuts_cases.npz"), **out)


if __name__ == "__main__":
    main()
