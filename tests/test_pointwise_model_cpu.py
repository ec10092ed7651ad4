"""CPU evidence that tests/test_gpu_pointwise_exact.py would notice a subtly wrong kernel: the checkers it uses
(tests/pointwise_cases.py) are run here on float32 restatements of the four kernels (tools/pointwise_model.py).  The faithful
restatement passes every case that fits on the CPU in a second (the two grid-stride shapes are left out); each named mutant -- one
plausible mistake each -- is rejected by the checker of its kernel."""
import os
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401
import pointwise_cases as pc
from util import bicubic_taps, preprocess_ref, triple

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pointwise_model as pm  # noqa: E402


# ---- every case against the model; mutant=None must pass, a mutant may fail anywhere -----------------------------------------------
def run_bias_act(mutant=None):
    for dtype in pc.HALF:
        for shape in pc.BIAS_ACT_SHAPES:
            ops = pc.bias_act_operands(dtype, shape)
            wants = pc.bias_act_wants(ops)
            for relu, nres in pc.BIAS_ACT_COMBOS:
                got = pm.bias_act(*pc.bias_act_args(ops, nres), relu, mutant=mutant)
                pc.check_bias_act(got, wants[(relu, nres)], f"bias_act {dtype} {shape} relu={relu} residuals={nres}")
        ops = pc.bias_act_special_operands(dtype)
        for relu, nres in pc.BIAS_ACT_COMBOS:
            got = pm.bias_act(*pc.bias_act_args(ops, nres), relu, mutant=mutant)
            pc.check_specials(got, pc.bias_act_special_want(ops, relu, nres), f"bias_act specials {dtype} relu={relu} residuals={nres}")


def run_readout(mutant=None):
    worst = {}
    for dtype in pc.HALF:
        for shape in pc.READOUT_SHAPES:
            ops = pc.readout_operands(dtype, shape)
            ratio, off, report = pc.check_readout(pm.reassemble_readout(ops["proj"], ops["cls"], mutant=mutant), ops, f"read-out {dtype} {shape}")
            print(report)
            worst[dtype] = max(worst.get(dtype, 0.0), ratio)
    return worst


def run_preprocess(mutant=None):
    worst = {}
    for in_hw, out_hw in pc.PRE_SHAPES:
        for kind in ("random", "white"):
            img = pc.pre_image(kind, in_hw)
            for mean, std in pc.PRE_NORMS:
                for flip in (True, False):
                    ref, s = preprocess_ref(img, out_hw, mean, std, flip)
                    for dtype in pc.PRE_DTYPES:
                        tag = f"preprocess {in_hw} -> {out_hw} {kind} flip={flip} mean={mean} {dtype}"
                        got = pm.preprocess_bicubic(img, out_hw, triple(mean), triple(std), flip, dtype, mutant=mutant)
                        worst[dtype] = max(worst.get(dtype, 0.0), pc.check_preprocess(got, ref, s, mean, std, tag))
                        if (in_hw, out_hw) == pc.PRE_IDENTITY and dtype == torch.float32:
                            want = pc.pre_identity_want(img, mean, std, flip)
                            assert torch.equal(got, want), f"{tag}: {pc.first_mismatches(got, want)}"
    return worst


def run_gconv(mutant=None):
    worst = 0.0
    for shape in pc.GCONV_SHAPES:
        for cpg in pc.GCONV_CPGS:
            groups = shape[1] // cpg
            ops = pc.gconv_int_operands(shape, cpg)
            img = pc.weight_image(ops["w"], groups)
            for use_bias, relu in ((True, True), (False, False), (True, False)):
                got = pm.gconv3x3(ops["x"], img, ops["bias"] if use_bias else None, relu, cpg, mutant=mutant)
                pc.check_gconv_exact(got, ops, cpg, use_bias, relu, f"gconv exact {shape} cpg={cpg} bias={use_bias} relu={relu}")
            wimg = pc.weight_image(pc.impulse_weight(shape[1], cpg), groups)
            for site in pc.impulse_sites(shape):
                got = pm.gconv3x3(pc.impulse_x(shape, site), wimg, None, False, cpg, mutant=mutant)
                pc.check_gconv_impulse(got, shape, cpg, site, f"gconv impulse {shape} cpg={cpg}")
            ops = pc.gconv_real_operands(shape, cpg)
            img = pc.weight_image(ops["w"], groups)
            for use_bias, relu in ((True, True), (False, False)):
                got = pm.gconv3x3(ops["x"], img, ops["bias"] if use_bias else None, relu, cpg, mutant=mutant)
                worst = max(worst, pc.check_gconv_bound(got, ops, cpg, use_bias, relu, f"gconv bound {shape} cpg={cpg} bias={use_bias} relu={relu}"))
    return worst


RUNNERS = {"bias_act": run_bias_act, "reassemble_readout": run_readout, "preprocess_bicubic": run_preprocess, "gconv3x3": run_gconv}


@pytest.mark.parametrize("kernel", sorted(RUNNERS))
def test_faithful_restatement_passes_every_case(kernel):
    worst = RUNNERS[kernel]()
    print(f"{kernel}: faithful float32 restatement, worst error / bound {worst}")


@pytest.mark.parametrize("kernel,mutant", [(k, m) for k in sorted(pm.MUTANTS) for m in pm.MUTANTS[k]])
def test_mutant_is_rejected(kernel, mutant):
    with pytest.raises(AssertionError) as err:
        RUNNERS[kernel](mutant)
    print(f"{kernel} / {mutant} rejected: {str(err.value)[:300]}")


def test_every_mutant_the_issue_names_is_listed():
    assert sum(len(v) for v in pm.MUTANTS.values()) == 13 and set(pm.MUTANTS) == set(RUNNERS)


# ---- the references themselves ----------------------------------------------------------------------------------------------------------
def test_bicubic_taps_properties():
    """Identity: weights exactly (0, 1, 0, 0) and tap 1 is the pixel itself.  Any size: indices inside [0, n_in), weights summing to 1
    within float32 rounding; a one-pixel axis clamps all four taps onto pixel 0."""
    idx, c = bicubic_taps(41, 41)
    assert np.array_equal(c, np.tile(np.float32([0, 1, 0, 0]), (41, 1))) and np.array_equal(idx[:, 1], np.arange(41))
    for n_in, n_out in [(1, 5), (2, 7), (9, 20), (7, 1), (70, 48), (300, 32)]:
        idx, c = bicubic_taps(n_in, n_out)
        assert idx.shape == c.shape == (n_out, 4) and idx.dtype == np.int64 and c.dtype == np.float32
        assert idx.min() >= 0 and idx.max() <= n_in - 1 and np.all(np.diff(idx, axis=1) >= 0)
        # six float32 operations per weight on intermediates below 8: at most 4 x 6 x 2^-24 x 4 = 5.8e-6 off an exact sum of 1
        assert np.abs(c.astype(np.float64).sum(1) - 1.0).max() < 6e-6
    assert not bicubic_taps(1, 5)[0].any()


def test_preprocess_ref_matches_torch_bicubic():
    """The float64 reference against torch's own CPU bicubic (align_corners=False) on the same normalised image: same kernel, same
    centres, same border -- float32 against float64 arithmetic only."""
    import torch.nn.functional as F
    for (in_hw, out_hw) in [((20, 30), (32, 48)), ((45, 70), (32, 48)), ((2, 3), (7, 5)), ((5, 7), (1, 1))]:
        img = pc.pre_image("random", in_hw)
        mean, std = pc.IMAGENET
        ref, s = preprocess_ref(img, out_hw, mean, std, True)
        x = torch.from_numpy(img[..., ::-1].copy()).permute(0, 3, 1, 2).double() / 255.0
        want = (F.interpolate(x, size=out_hw, mode="bicubic", align_corners=False) - torch.tensor(mean).double().view(1, 3, 1, 1)) / torch.tensor(std).double().view(1, 3, 1, 1)
        # float32 source coordinates (up to 70: two roundings of 3.8e-6) against torch's float64 ones, a weight slope below 1.5 per
        # tap, pixel values up to 1 and 1 / std = 4.5: 2e-4; a wrong tap, centre or border is off by 1e-2 and more
        assert float((ref - want).abs().max()) < 2e-4 and bool((s >= 0).all())
