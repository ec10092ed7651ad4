"""The shared launches of the stage between encoder and fusion blocks inside the whole network: dpt_beit_large_512 at 512^2, batch 8,
float16 (the smallest batch at which the read-outs take the in-tree route; the shapes of tests/test_gpu_models.py's batch test).
With DS_READOUT_CLS4 (ds_linear_rows4) and DS_CONV_PAIR (ds_conv3x3_nhwc_pair) on, the prediction is torch.equal to the one with
both off, and the binding's counters tell the routes apart while the numbers of in-tree GEMMs and convolutions read the same."""
import pytest
import torch

import conftest  # noqa: F401
import model_weights as mw

pytestmark = pytest.mark.gpu
NAMES = ("ds_linear_rows4", "ds_conv3x3_nhwc_pair", "ds_linear", "ds_linear_readout", "ds_conv3x3_nhwc")


def test_dpt_beit_large_512_keeps_its_bits_and_takes_the_routes(gpu, monkeypatch):
    from dmidas.dpt_depth import DPTDepthModel
    from src import _native
    from src import vit_mi355x as vm
    from src.hip_graph import GraphedForward
    m = DPTDepthModel(path=None, backbone="beitl16_512", non_negative=True).eval()
    m.load_state_dict(mw.fill_state_dict_beit(m.state_dict()), strict=True)
    m = m.cuda().half()
    base = mw.synthetic_image((1, 3, 512, 512), seed=31)
    x = torch.cat([base.roll(17 * i, dims=3) for i in range(8)]).cuda().half().contiguous(memory_format=torch.channels_last)

    def run(on):
        monkeypatch.setattr(vm, "READOUT_CLS4", on)
        monkeypatch.setattr(vm, "CONV_PAIR", on)
        before = dict(_native.CALLS)
        with torch.no_grad():
            y = m(x)
        torch.cuda.synchronize()
        return y, {n: _native.CALLS[n] - before.get(n, 0) for n in NAMES}
    y1, calls1 = run(True)
    y0, calls0 = run(False)
    assert calls1["ds_linear_rows4"] == 1 and calls0["ds_linear_rows4"] == 0, (calls1, calls0)
    assert calls1["ds_conv3x3_nhwc_pair"] == 1 and calls0["ds_conv3x3_nhwc_pair"] == 0, (calls1, calls0)
    for n in ("ds_linear", "ds_linear_readout", "ds_conv3x3_nhwc"):
        assert calls1[n] == calls0[n] > 0, (n, calls1, calls0)
    assert bool(torch.isfinite(y1.float()).all())
    assert torch.equal(y1, y0), "the shared launches changed the prediction"
    # the same forward captured and replayed as a hipGraph: the new launches hold no allocation or synchronisation of their own
    monkeypatch.setattr(vm, "READOUT_CLS4", True)
    monkeypatch.setattr(vm, "CONV_PAIR", True)
    with torch.no_grad():
        gf = GraphedForward(lambda t: m(t))
        yg = gf(x)
        yg = gf(x)
    torch.cuda.synchronize()
    assert gf.graphs, "the forward was not captured"
    assert torch.equal(yg, y0), "the replayed forward differs"
