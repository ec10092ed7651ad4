"""The host half of the custom-depth ingest (src/resample_model.py): the LANCZOS coefficient builder plus the numpy model of the
kernel arithmetic of csrc/ds_resample.hip against Pillow's own Image.resize -- zero differing pixels --, the Pillow probe and
the bit-depth rule of reference src/core.py:158-164.  No GPU."""
import numpy as np
import pytest
from PIL import Image

from src import resample_model as rm

# (in_h, in_w) -> (out_h, out_w): both directions, one-axis passes, mixed enlarge / reduce, degenerate sizes
SHAPES = [((37, 53), (64, 91)), ((64, 91), (37, 53)), ((40, 40), (40, 77)), ((50, 31), (23, 31)), ((33, 47), (100, 20)),
          ((61, 45), (200, 131)), ((331, 67), (17, 9)), ((5, 4), (9, 7)), ((4, 5), (1, 1)), ((3, 200), (3, 11)), ((9, 2), (64, 64))]
MODES = ["L", "I;16", "I", "F"]


def random_plane(mode, shape, rng):
    """Uniformly random over the full range of the type."""
    if mode == "L":
        return rng.integers(0, 256, shape).astype(np.uint8)
    if mode == "I;16":
        return rng.integers(0, 65536, shape).astype(np.uint16)
    if mode == "I":
        return rng.integers(-(1 << 20), (1 << 20) + 1, shape).astype(np.int32)
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


def pillow_resize(plane, out_hw):
    im = Image.fromarray(plane)
    return np.asarray(im.resize((out_hw[1], out_hw[0]), Image.Resampling.LANCZOS))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("in_hw,out_hw", SHAPES)
def test_model_equals_pillow(mode, in_hw, out_hw):
    rng = np.random.default_rng(1000 * in_hw[0] + in_hw[1] + len(mode))
    plane = random_plane(mode, in_hw, rng)
    assert Image.fromarray(plane).mode == mode
    want = pillow_resize(plane, out_hw)
    got = rm.resize_model(plane[None], rm.PIX_OF_MODE[mode], out_hw)[0]
    assert got.dtype == want.dtype and got.shape == want.shape
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.itemsize]        # (compared as bit patterns: -0.0 is not 0.0)
    differing = int(np.count_nonzero(got.view(bits) != np.ascontiguousarray(want).view(bits)))
    assert differing == 0, f"{mode} {in_hw}->{out_hw}: {differing} pixels differ"


def test_i16_high_byte_clip_is_exercised():
    """Enlarging a random I;16 plane overshoots 65535: Pillow clips the high byte and keeps the low one, and so must the model."""
    rng = np.random.default_rng(7)
    plane = random_plane("I;16", (37, 53), rng)
    ksize, bounds, kk = rm.lanczos_coeffs(53, 91)
    ss = np.zeros((37, 91))
    for t in range(ksize):
        ss = ss + plane[:, np.minimum(bounds[:, 0] + t, 52)] * kk[:, t]
    over = np.floor(ss + 0.5) > 65535
    assert over.sum() > 10
    got = rm.resize_model(plane[None], rm.PIX_U16, (37, 91))[0]
    assert np.all(got[over] >= 0xFF00)
    assert np.array_equal(got, pillow_resize(plane, (37, 91)))


@pytest.mark.parametrize("in_hw,out_hw", [((37, 53), (64, 91)), ((64, 91), (37, 53)), ((5, 4), (9, 7))])
def test_rgb_band0(in_hw, out_hw):
    """The reference reads channel 0 of a multi-band depth map only; band 0 of the resized image is the resized band 0."""
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, in_hw + (3,)).astype(np.uint8)
    want = pillow_resize(rgb, out_hw)[..., 0]
    got = rm.resize_model(rgb[None, ..., 0], rm.PIX_U8, out_hw)[0]
    assert np.array_equal(got, want)


def test_coefficients_follow_the_stated_rule():
    ksize, bounds, kk = rm.lanczos_coeffs(91, 53)
    scale = 91 / 53
    assert ksize == int(np.ceil(3.0 * scale)) * 2 + 1 and kk.shape == (53, ksize) and bounds.shape == (53, 2)
    assert np.all(bounds[:, 0] >= 0) and np.all(bounds[:, 0] + bounds[:, 1] <= 91) and np.all(bounds[:, 1] <= ksize)
    assert np.allclose(kk.sum(1), 1.0, atol=1e-12)
    ksize, bounds, kk = rm.lanczos_coeffs(53, 91)           # enlarging: the filter is not stretched
    assert ksize == 7
    ki = rm.fixed_point_coeffs(np.array([[0.25, -0.25, 1e-9, -1e-9]]))
    assert ki.tolist() == [[1 << 20, -(1 << 20), 0, 0]]


def test_probe_accepts_the_installed_pillow():
    rm._PROBE.clear()
    assert rm.pillow_matches_model() is True
    assert rm._PROBE == {"ok": True}


def test_probe_rejects_a_different_resampler(monkeypatch):
    """A Pillow whose arithmetic differs (here: one that answers with another filter) sends the ingest to the host route."""
    real = Image.Image.resize
    monkeypatch.setattr(Image.Image, "resize", lambda self, size, resample=None, **kw: real(self, size, Image.Resampling.BICUBIC))
    rm._PROBE.clear()
    try:
        assert rm.pillow_matches_model() is False
    finally:
        rm._PROBE.clear()


def test_bit_depth_rule():
    assert [rm.bit_depth(v) for v in (255.0, 256.0, 65535.0, 65536.0, float("nan"))] == [8, 16, 16, 32, 32]
    assert rm.bit_depth(np.float64("nan")) == 32 and rm.bit_depth(0.0) == 8


def test_ingest_routing_with_modelled_kernels(monkeypatch):
    """core._ingest_custom_depth with the two native calls replaced by their numpy models: which depth maps take the device route,
    how consecutive ones are grouped, and that the planes equal the host route's as float64 bits.  (The kernels themselves:
    tests/test_gpu_resample.py.)"""
    import types
    import torch
    from src import _native, core
    calls = []

    def resize(src, out_hw):
        a = src.numpy()
        calls.append(("resize", a.shape[0]))
        a = a[..., 0] if a.ndim == 4 else a
        pix = [p for p, d in rm.PIX_DTYPE.items() if np.dtype(d) == a.dtype][0]
        return torch.from_numpy(rm.resize_model(a, pix, out_hw))

    def widen(src, rule, out=None):
        a = src.numpy()
        calls.append(("widen", a.shape[0]))
        a = (a[..., 0] if a.ndim == 4 else a).astype(np.float64)
        div = {_native.CD_WIDEN: 1.0, _native.CD_MULTI_BAND: 256.0}.get(rule)
        if div is None:
            div = np.array([2.0 ** rm.bit_depth(p.max()) for p in a]).reshape(-1, 1, 1)
        out.copy_(torch.from_numpy(a / div))
        return out, None
    monkeypatch.setattr(_native, "resize_lanczos", resize)
    monkeypatch.setattr(_native, "custom_depth_to_f64", widen)
    monkeypatch.setattr(core, "CUSTOM_DEPTH_DEVICE", True)
    rng = np.random.default_rng(9)
    size, full = (45, 31), (31, 45)
    small = [Image.fromarray(random_plane("I;16", (17, 23), rng)) for _ in range(3)]
    maps = small + [Image.fromarray(random_plane("L", full, rng)), Image.fromarray(rng.integers(0, 256, (20, 30, 4)).astype(np.uint8)),
                    Image.fromarray(rng.integers(0, 256, (64, 91, 3)).astype(np.uint8)), rng.uniform(0, 1, full).astype(np.float32),
                    rng.uniform(0, 1, full), Image.fromarray(random_plane("I", (6000, 3), rng))]
    keys = [core._depth_device_key(dp, size) for dp in maps]
    assert keys == [("pil", "I;16", (23, 17))] * 3 + [("pil", "L", (45, 31)), None, ("pil", "RGB", (91, 64)), ("array", np.dtype(np.float32)),
                                                     None, None]        # RGBA, float64, and a 6000 -> 31 reduction (1163 taps)
    stats = {}
    got = core._ingest_custom_depth(maps, size, "cpu", lambda arrays, tag, dtype: torch.from_numpy(np.stack(arrays)), stats).numpy()
    like = types.SimpleNamespace(width=size[0], height=size[1])
    for j, dp in enumerate(maps):
        want = np.asarray(core._custom_depth_to_float(dp, like), dtype=np.float64)
        assert got[j].tobytes() == want.tobytes(), j
    assert stats == {"custom_depth_device": 6, "custom_depth_host": 3}
    assert calls == [("resize", 3), ("widen", 3), ("widen", 1), ("resize", 1), ("widen", 1), ("widen", 1)]
    monkeypatch.setattr(core, "CUSTOM_DEPTH_DEVICE", False)
    stats, n = {}, len(calls)
    off = core._ingest_custom_depth(maps, size, "cpu", lambda arrays, tag, dtype: torch.from_numpy(np.stack(arrays)), stats).numpy()
    assert off.tobytes() == got.tobytes() and stats == {"custom_depth_host": 9} and len(calls) == n
