"""The normal-map entry points at the sizes and on the kernel no other test checks by value, bit for bit against the CPU oracle:

  * single-row, single-column and 1 x 1 Sobel maps (uint16 without blur and with Sobel 3 takes the one-pixel-per-lane fused kernel,
    everything else the separable float64 passes; BORDER_REFLECT_101 and wrap both name index 0 on an axis of one sample);
  * the one-pixel-per-lane fused kernel WITHOUT wrap on a misaligned uint16 slice, against the four-pixel kernel on the aligned
    tensor (tests/test_gpu_normalmap_wrap.py has the wrap twin of this test): the two share one arithmetic;
  * np.gradient at the smallest legal sizes (2 x 2: both samples of an axis are ends; 2 x 3 and 3 x 4: one interior sample), in
    all four dtypes."""
import numpy as np
import pytest

import normalmap_wrap_cases as wc

pytestmark = pytest.mark.gpu

FLAT = [128, 128, 255]                                  # the normal of a map without slope: (0, 0, 1)


def _gpu(torch, d, opt, inv, wrap=False):
    import src.normalmap_generation as nm
    x = d if isinstance(d, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(d)).cuda().unsqueeze(0)
    return nm.create_normalmap_batch(x, opt[0], opt[1], opt[2], inv, wrap=wrap)


@pytest.mark.parametrize("shape", [(1, 5), (5, 1), (1, 8), (8, 1)], ids=lambda s: "%dx%d" % s)
def test_single_row_and_single_column_sobel_maps(gpu, oracle, shape):
    torch = gpu
    h, w = shape
    for dtype in (np.uint16, np.float64):
        d = wc.depth(h, w, dtype, seed=100 * h + w)
        for opt in ((0, 3, 0), (0, 5, 0), (0, 1, 0), (0, 7, 0), (3, 3, 3)):
            for inv in (False, True):
                got = _gpu(torch, d, opt, inv)[0].cpu().numpy()
                want = wc.plain(oracle.create_normalmap_array, d, *opt, invert=inv)
                assert np.array_equal(got, want), (np.dtype(dtype).name, opt, inv, got.tolist(), np.asarray(want).tolist())
                got = _gpu(torch, d, opt, inv, wrap=True)[0].cpu().numpy()
                want = wc.wrap_by_definition(oracle.create_normalmap_array, d, *opt, invert=inv)
                assert np.array_equal(got, want), ("wrap", np.dtype(dtype).name, opt, inv, got.tolist(), np.asarray(want).tolist())


def test_one_by_one_sobel_map_is_flat(gpu):
    """The oracle's numpy route does not take a 1 x 1 array; every tap of every pass is the one sample, so both derivatives are 0."""
    torch = gpu
    for dtype in (np.uint16, np.float64):
        d = np.full((1, 1), 12345, dtype)
        for sob in (3, 5):
            for wrap in (False, True):
                got = _gpu(torch, d, (0, sob, 0), False, wrap=wrap)[0].cpu().numpy()
                assert got.shape == (1, 1, 3) and got[0, 0].tolist() == FLAT, (np.dtype(dtype).name, sob, wrap, got.tolist())


@pytest.mark.parametrize("shape", [(2, 4), (8, 8), (33, 260)], ids=lambda s: "%dx%d" % s)
def test_scalar_fused_kernel_on_a_misaligned_slice_equals_fused4(gpu, oracle, shape):
    """w % 4 == 0 but the depth pointer is not 8-byte aligned: the launcher takes the one-pixel-per-lane kernel, whose bytes must
    be those of the four-pixel kernel on the aligned tensor, and the oracle's."""
    torch = gpu
    h, w = shape
    d = wc.depth(h, w, np.uint16, seed=h + w + 1)
    host = np.zeros(h * w + 4, np.uint16)
    host[1:1 + h * w] = d.ravel()
    view = torch.from_numpy(host).cuda()[1:1 + h * w].view(1, h, w)
    aligned = torch.from_numpy(d).cuda().unsqueeze(0)
    assert view.data_ptr() % 8 == 2 and view.is_contiguous() and aligned.data_ptr() % 8 == 0
    for sob in (3, 0):
        for inv in (False, True):
            got = _gpu(torch, view, (0, sob, 0), inv)
            assert torch.equal(got, _gpu(torch, aligned, (0, sob, 0), inv)), (sob, inv)
            want = wc.plain(oracle.create_normalmap_array, d, 0, sob, 0, invert=inv)
            assert np.array_equal(got[0].cpu().numpy(), want), (sob, inv)


@pytest.mark.parametrize("shape", [(2, 2), (2, 3), (3, 4)], ids=lambda s: "%dx%d" % s)
def test_np_gradient_at_the_smallest_legal_sizes(gpu, oracle, shape):
    torch = gpu
    h, w = shape
    with np.errstate(all='ignore'):                     # float16: numpy's own overflow warnings, as in tests/test_gpu_parity.py
        for dtype in (np.uint16, np.float64, np.float32, np.float16):
            d = wc.depth(h, w, dtype, seed=10 * h + w)
            for inv in (False, True):
                got = _gpu(torch, d, (0, 0, 0), inv)[0].cpu().numpy()
                want = np.asarray(oracle.create_normalmap_array(d, None, None, None, inv))
                assert np.array_equal(got, want), (np.dtype(dtype).name, inv, got.tolist(), want.tolist())
