"""Golden output for TILING_MODE on a Depth-Anything-V2 whose decoder is wide enough for the in-tree kernels (features = 256:
every 3x3 of the decoder has channels % 128 == 0 and the head's 128 -> 32 convolution is the fused head tail's), from the
reference's own module, hijacked like make_golden_tiling.py hijacks it (reference src/depthmap_generation.py:251-260).  Only the
output is stored.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tiling_heads.py        -> tiling_head_cases.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden_models as mgm  # noqa: E402
import make_golden_tiling as mgt  # noqa: E402
import model_weights as mw  # noqa: E402

DAV2 = ('vits', 256, [256, 512, 1024, 1024])          # encoder, features, out_channels
SHAPE, SEED = (2, 3, 140, 182), 11


def main():
    out = {}
    m = mgm.reference_dav2(*DAV2).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    out["dav2_vits_f256_n_convs"] = np.array([mgt.hijack(m)])
    with torch.no_grad():
        out["dav2_vits_f256_140x182_out"] = m(mw.synthetic_image(SHAPE, seed=SEED)).numpy()
    np.savez_compressed(os.path.join(HERE, "tiling_head_cases.npz"), **out)
    print({k: (v.shape, v.ravel()[:1]) for k, v in out.items()})


if __name__ == "__main__":
    main()
