"""Generates tests/golden/midas_small_cases.npz by running the REFERENCE's own dmidas.midas_net_custom.MidasNet_small (MiDaS v2.1
small, model id 6; imported from the reference checkout like make_golden_models.py does) with torch.hub.load patched to the
gen-efficientnet stand-in fake_geffnet.py (fake_timm.install() covers blocks.py's other imports), on name-seeded synthetic weights
(model_weights.py: BatchNorm in eval mode, positive running_var).

What is pinned: the MidasNet_small decoder, the _make_efficientnet_backbone wrapping and the checkpoint key layout are the
reference's code.  What is not: the EfficientNet-Lite3 body is restated on both sides (fake_geffnet.py here,
dmidas/backbones/efficientnet_lite.py in the package), so its structure is pinned and its fidelity to gen-efficientnet is not.
One fresh reference model per input size: the exportable "SAME" convolution keeps the pads of the first input it sees.

    python tests/golden/make_golden_midas_small.py
"""
import json
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import model_weights as mw  # noqa: E402
from make_golden_models import REF  # noqa: E402

# tag -> (input shape: multiples of 32, as the network always sees them; seed of the synthetic image)
CASES = {"b2_96x128": ((2, 3, 96, 128), 31), "b1_256x192": ((1, 3, 256, 192), 32)}


def reference_midas_small():
    import fake_geffnet
    import fake_timm
    fake_timm.install()
    fake_geffnet.install()
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = mock.MagicMock()
    sys.path.insert(0, REF)
    from dmidas.midas_net_custom import MidasNet_small
    sys.path.pop(0)
    m = MidasNet_small(None, features=64, backbone="efficientnet_lite3", exportable=True, non_negative=True, blocks={'expand': True})
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    return m.eval()


def run(m, x):
    with torch.no_grad():
        y = m(x)
        l1 = m.pretrained.layer1(x)
        l2 = m.pretrained.layer2(l1)
        l4 = m.pretrained.layer4(m.pretrained.layer3(l2))
    return y, l2, l4


def main():
    out = {}
    m = reference_midas_small()
    out["keys"] = np.frombuffer(json.dumps(sorted(m.state_dict().keys())).encode(), dtype=np.uint8)
    out["n_convs"] = np.array([sum(1 for layer in m.modules() if type(layer) is torch.nn.Conv2d)])
    for tag, (shape, seed) in CASES.items():
        y, l2, l4 = run(reference_midas_small(), mw.synthetic_image(shape, seed))
        out[f"{tag}_out"] = y.numpy()
        out[f"{tag}_layer2"] = l2[:, ::4].numpy()            # every fourth channel of the /8 tap
        out[f"{tag}_layer4"] = l4.numpy()
    # TILING_MODE: the reference's hijack (src/depthmap_generation.py:250-260) -- exact type nn.Conv2d pads circularly
    m = reference_midas_small()
    for layer in m.modules():
        if type(layer) is torch.nn.Conv2d:
            layer.padding_mode = 'circular'
    shape, seed = CASES["b2_96x128"]
    out["b2_96x128_tiled_out"] = run(m, mw.synthetic_image(shape, seed))[0].numpy()
    np.savez_compressed(os.path.join(HERE, "midas_small_cases.npz"), **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype, float(np.abs(v.astype(np.float64)).mean()), float((v > 0).mean()) if v.dtype == np.float32 else "")


if __name__ == "__main__":
    main()
