"""MiDaS v2.1 small (model id 6) on the CPU, float32: the built module against outputs of the REFERENCE's own MidasNet_small
(tests/golden/midas_small_cases.npz, made by tests/golden/make_golden_midas_small.py on the gen-efficientnet stand-in
fake_geffnet.py with name-seeded synthetic weights), and the ModelHolder / TILING_MODE / Boost wiring of id 6.  Tolerance: 1e-4
relative to the output scale, float32 against float32."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (sys.path)
import model_weights as mw

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "midas_small_cases.npz")
CASES = {"b2_96x128": ((2, 3, 96, 128), 31), "b1_256x192": ((1, 3, 256, 192), 32)}


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _model():
    from dmidas.midas_net_custom import MidasNet_small
    m = MidasNet_small(path=None, features=64, backbone="efficientnet_lite3", exportable=True, non_negative=True,
                       blocks={'expand': True}).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    return m


def test_state_dict_keys_equal_reference_module(gold):
    keys = sorted(_model().state_dict().keys())
    assert keys == json.loads(bytes(gold["keys"]).decode())
    for k in ("pretrained.layer1.0.weight", "pretrained.layer1.1.running_var", "pretrained.layer1.3.0.conv_dw.weight",
              "pretrained.layer1.4.2.conv_pwl.weight", "pretrained.layer4.1.0.bn3.bias", "scratch.layer4_rn.weight",
              "scratch.refinenet4.out_conv.weight", "scratch.output_conv.4.bias"):
        assert k in keys, k


def test_encoder_stage_table():
    """(repeats, kernel, first stride, width, first / last expanded width) of every stage: the table of the module docstring."""
    p = _model().pretrained
    stages = [p.layer1[3], p.layer1[4], *p.layer2, *p.layer3, *p.layer4]
    got = [(len(st), st[0].conv_dw.kernel_size[0], st[0].conv_dw.stride[0], (st[-1].bn3 if hasattr(st[-1], "bn3") else st[-1].bn2).num_features,
            st[0].conv_dw.out_channels, st[-1].conv_dw.out_channels) for st in stages]
    assert got == [(1, 3, 1, 24, 32, 32), (3, 3, 2, 32, 144, 192), (3, 5, 2, 48, 192, 288), (5, 3, 2, 96, 288, 576),
                   (5, 5, 1, 136, 576, 816), (6, 5, 2, 232, 816, 1392), (1, 3, 1, 384, 1392, 1392)]
    assert p.layer1[0].out_channels == 32 and p.layer1[0].stride == (2, 2)


def test_forward_matches_reference_module(gold):
    """ONE module for both input sizes: the "SAME" pads follow every input (the reference's exportable convolution keeps its first)."""
    from dmidas.backbones.efficientnet_lite import forward_encoder
    m = _model()
    for tag, (shape, seed) in CASES.items():
        x = mw.synthetic_image(shape, seed)
        with torch.no_grad():
            y = m(x).numpy()
            _, l2, _, l4 = forward_encoder(m.pretrained, x)
        assert y.shape == gold[f"{tag}_out"].shape
        assert _rel(y, gold[f"{tag}_out"]) < 1e-4
        assert _rel(l2[:, ::4].numpy(), gold[f"{tag}_layer2"]) < 1e-4
        assert _rel(l4.numpy(), gold[f"{tag}_layer4"]) < 1e-4


def test_tiling_mode_matches_reference_module(gold):
    from dmidas.backbones.efficientnet_lite import Conv2dSame
    from src.depthmap_generation import apply_tiling_mode
    m = _model()
    assert apply_tiling_mode(m) == int(gold["n_convs"][0])
    same = [layer for layer in m.modules() if isinstance(layer, Conv2dSame)]
    assert len(same) == 5 and all(layer.padding_mode == 'zeros' for layer in same)      # the stem + four stride-2 depthwise
    shape, seed = CASES["b2_96x128"]
    with torch.no_grad():
        assert _rel(m(mw.synthetic_image(shape, seed)).numpy(), gold["b2_96x128_tiled_out"]) < 1e-4


def test_model_holder_builds_midas_small(tmp_path, monkeypatch):
    """ensure_models(6): no checkpoint -> FileNotFoundError (Boost too: there the merge network's is missing first); with
    allow_random_init the network is built and predicts like estimatemidas: upper_bound resize, BGR order, ImageNet statistics."""
    from src.depthmap_generation import ModelHolder
    monkeypatch.chdir(tmp_path)                  # ./models/* resolve to an empty directory
    mh = ModelHolder()
    with pytest.raises(FileNotFoundError):
        mh.ensure_models(6, 'cpu', False)
    with pytest.raises(FileNotFoundError):
        mh.ensure_models(6, 'cpu', True)
    mh.allow_random_init = True
    mh.ensure_models(6, 'cpu', False)
    assert mh.get_default_net_size(6) == [256, 256]
    net = mh.depth_model.net
    assert type(net).__name__ == "MidasNet_small" and next(net.parameters()).dtype == torch.float32
    img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (1, 70, 100, 3), dtype=np.uint8))
    pred = mh.depth_model.predict_batch(img, 96, 96)
    x = F.interpolate(img.flip(-1).permute(0, 3, 1, 2).float() / 255.0, size=(64, 96), mode="bicubic", align_corners=False)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    with torch.no_grad():
        want = F.interpolate(net((x - mean) / std).unsqueeze(1), size=(70, 100), mode="bicubic", align_corners=False).squeeze(1)
    assert tuple(pred.shape) == (1, 70, 100) and torch.allclose(pred, want, rtol=1e-6, atol=1e-6)


def test_boost_single_estimates_for_midas_small():
    """estimatemidasBoost (:1180-1220) for id 6: upper_bound resize, ImageNet statistics, min-max normalised, as written out by hand."""
    from dmidas.dpt_depth import midas_net_size
    from src import boost
    torch.manual_seed(3)
    patches = [torch.rand((70, 100, 3), dtype=torch.float64), torch.rand((90, 64, 3), dtype=torch.float64)]
    net = _model()
    with torch.no_grad():
        outs = boost._single_estimates(patches, 384, net, 6, 8)
        p = patches[0]
        nw, nh = midas_net_size(100, 70, 384, 384, "upper_bound")
        assert (nw, nh) == (384, 256)
        x = F.interpolate(p.permute(2, 0, 1)[None].reshape(3, 1, 70, 100), size=(nh, nw), mode='bicubic', align_corners=False)
        x = x.reshape(1, 3, nh, nw).float()
        mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
        want = F.interpolate(net((x - mean) / std)[:, None].float(), size=(70, 100), mode='bicubic', align_corners=False)[0, 0]
        want = (want - want.min()) / (want.max() - want.min())
    assert [tuple(o.shape) for o in outs] == [(70, 100), (90, 64)]
    assert float(outs[0].min()) == 0.0 and float(outs[0].max()) == 1.0
    assert torch.allclose(outs[0], want, atol=1e-6)
