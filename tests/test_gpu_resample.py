"""The custom-depth branch on the device (csrc/ds_resample.hip, reference src/core.py:145-174): ds_resize_lanczos against Pillow's own
Image.resize byte for byte, the ingest helper against the host route as float64 bits, and the funnel with the switch off and on."""
import numpy as np
import pytest
from PIL import Image

from test_resample_cpu import MODES, SHAPES, pillow_resize, random_plane

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native(gpu):
    import src._native as nat
    nat.lib()
    return nat


def _same_bytes(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == np.ascontiguousarray(want).tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_kernel_equals_pillow(gpu, native, mode):
    """Every shape of the CPU test, batch 3 with different content per image."""
    torch = gpu
    rng = np.random.default_rng(len(mode))
    for in_hw, out_hw in SHAPES:
        planes = np.stack([random_plane(mode, in_hw, rng) for _ in range(3)])
        got = native.resize_lanczos(torch.from_numpy(planes).cuda(), out_hw).cpu().numpy()
        for j in range(3):
            assert _same_bytes(got[j], pillow_resize(planes[j], out_hw)), (mode, in_hw, out_hw, j)


def test_kernel_reads_rgb_band0_in_place(gpu, native):
    """Interleaved RGB (pixel stride 3) and RGBX (4): band 0 of Pillow's resized image."""
    torch = gpu
    rng = np.random.default_rng(5)
    for in_hw, out_hw in SHAPES:
        rgb = rng.integers(0, 256, (3,) + in_hw + (3,)).astype(np.uint8)
        rgbx = np.concatenate([rgb, rng.integers(0, 256, (3,) + in_hw + (1,)).astype(np.uint8)], axis=3)
        got3 = native.resize_lanczos(torch.from_numpy(rgb).cuda(), out_hw).cpu().numpy()
        got4 = native.resize_lanczos(torch.from_numpy(rgbx).cuda(), out_hw).cpu().numpy()
        for j in range(3):
            want = pillow_resize(rgb[j], out_hw)[..., 0]
            assert _same_bytes(got3[j], want) and _same_bytes(got4[j], want), (in_hw, out_hw, j)


def test_kernel_limits(gpu, native):
    torch = gpu
    a = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(native.DepthStereoError, match="nothing to resize"):
        native.resize_lanczos(a, (8, 8))
    with pytest.raises(native.DepthStereoError, match="unsupported pixel tensor"):
        native.resize_lanczos(a.double(), (4, 4))
    tall = torch.zeros((1, 2000, 2), dtype=torch.uint8, device="cuda")          # 2000 -> 1 rows: 6001 taps
    with pytest.raises(native.DepthStereoError, match="taps"):
        native.resize_lanczos(tall, (1, 2))


def _pil(mode, plane):
    im = Image.fromarray(plane)
    assert im.mode == mode
    return im


def _host(core, dp, size):
    import types
    return np.asarray(core._custom_depth_to_float(dp, types.SimpleNamespace(width=size[0], height=size[1])), dtype=np.float64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_ingest_equals_host_route(gpu, native):
    """ingest_custom_depth_batch against _custom_depth_to_float for each mode (resized and not; maxima on both sides of 256 and
    65536) and each supported ndarray dtype, as float64 bits; the NaN plane included."""
    import src.core as core
    rng = np.random.default_rng(11)
    size = (45, 31)                                              # (width, height)
    full = (31, 45)
    maps = []
    for mode in MODES:
        maps.append(_pil(mode, random_plane(mode, full, rng)))                      # no resize
        maps.append(_pil(mode, random_plane(mode, (17, 23), rng)))                  # enlarged
        maps.append(_pil(mode, random_plane(mode, (64, 91), rng)))                  # reduced
    maps.append(_pil("I;16", rng.integers(0, 256, full).astype(np.uint16)))         # maximum < 256: 8 bits
    maps.append(_pil("I", rng.integers(0, 1 << 20, full).astype(np.int32)))         # maximum >= 65536: 32 bits
    maps.append(_pil("I", np.full(full, 65536, np.int32)))
    maps.append(_pil("I;16", np.full(full, 65535, np.uint16)))
    maps.append(_pil("L", np.full(full, 255, np.uint8)))
    nan_plane = rng.uniform(0, 300, full).astype(np.float32)
    nan_plane[7, 9] = np.nan
    maps.append(_pil("F", nan_plane))                                               # a NaN maximum: 32 bits, NaN stays NaN
    maps.append(_pil("F", rng.uniform(0, 300, full).astype(np.float32)))
    for shape in (full, (17, 23), (64, 91)):
        maps.append(_pil("RGB", rng.integers(0, 256, shape + (3,)).astype(np.uint8)))
    arrays = [rng.integers(0, 256, full).astype(np.uint8), rng.integers(0, 65536, full).astype(np.uint16),
              rng.integers(-5, 1 << 20, full).astype(np.int32), rng.uniform(0, 1, full).astype(np.float32),
              nan_plane, rng.uniform(0, 1, full)]                                   # (float64: the host route)
    maps += arrays
    native.CALLS.clear()
    core.CUSTOM_DEPTH_DEVICE = True
    got = core.ingest_custom_depth_batch(maps, size)
    assert got.is_cuda and got.dtype == gpu.float64 and tuple(got.shape) == (len(maps), 31, 45)
    assert native.CALLS["ds_custom_depth_to_f64"] > 0 and native.CALLS["ds_resize_lanczos"] > 0
    got = got.cpu().numpy()
    for j, dp in enumerate(maps):
        assert np.array_equal(_bits(got[j]), _bits(_host(core, dp, size))), (j, getattr(dp, "mode", getattr(dp, "dtype", None)))
    # consecutive depth maps of one (mode, size) share a launch: 4 equal I;16 maps -> one resize, one widening
    same = [_pil("I;16", random_plane("I;16", (17, 23), rng)) for _ in range(4)]
    native.CALLS.clear()
    got = core.ingest_custom_depth_batch(same, size).cpu().numpy()
    assert native.CALLS["ds_resize_lanczos"] == 1 and native.CALLS["ds_custom_depth_to_f64"] == 1
    for j, dp in enumerate(same):
        assert np.array_equal(_bits(got[j]), _bits(_host(core, dp, size)))
    # the switch is read per call
    core.CUSTOM_DEPTH_DEVICE = False
    try:
        native.CALLS.clear()
        off = core.ingest_custom_depth_batch(same, size).cpu().numpy()
        assert native.CALLS["ds_resize_lanczos"] == 0 and native.CALLS["ds_custom_depth_to_f64"] == 0
        assert np.array_equal(_bits(off), _bits(got))
    finally:
        core.CUSTOM_DEPTH_DEVICE = True


def test_ingest_reports_maximum_and_divisor(gpu, native):
    """np.max on the device: 255 / 256 / 65535 / 65536 / NaN -> 2^8, 2^16, 2^16, 2^32, 2^32."""
    torch = gpu
    planes = np.zeros((5, 9, 70), np.float32)
    for j, m in enumerate((255.0, 256.0, 65535.0, 65536.0, np.nan)):
        planes[j, 8, 69 - j] = m
    planes[4, 0, 0] = 1e9                                        # a NaN wins whatever else the plane holds
    out, md = native.custom_depth_to_f64(torch.from_numpy(planes).cuda(), native.CD_SINGLE_BAND)
    md = md.cpu().numpy()
    assert md[:4, 0].tolist() == [255.0, 256.0, 65535.0, 65536.0] and np.isnan(md[4, 0])
    assert md[:, 1].tolist() == [2.0 ** 8, 2.0 ** 16, 2.0 ** 16, 2.0 ** 32, 2.0 ** 32]
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(planes.astype(np.float64) / md[:, 1].reshape(5, 1, 1)))


def _funnel(core, images, depthmaps, opts, device_route, outpath=None):
    core.CUSTOM_DEPTH_DEVICE = device_route
    try:
        res = list(core.core_generation_funnel(outpath, list(images), list(depthmaps), None, opts))
    finally:
        core.CUSTOM_DEPTH_DEVICE = True
    return res, dict(core.FUNNEL_STATS)


def test_funnel_same_results_either_route(gpu, native):
    """Four 96x128 RGB images with stereo and normal map on; depth maps I;16 at 48x64, I;16 at 96x128 (no resize), L at 200x150 and
    one RGBA map (host route): every yielded result byte-identical with the switch off and on, three device ingests and one on the host."""
    import src.core as core
    rng = np.random.default_rng(21)
    images = [Image.fromarray(rng.integers(0, 256, (96, 128, 3)).astype(np.uint8)) for _ in range(4)]
    depthmaps = [_pil("I;16", random_plane("I;16", (48, 64), rng)), _pil("I;16", random_plane("I;16", (96, 128), rng)),
                 _pil("L", random_plane("L", (200, 150), rng)),
                 Image.fromarray(rng.integers(0, 256, (60, 70, 4)).astype(np.uint8))]
    assert depthmaps[3].mode == "RGBA"
    opts = {'gen_stereo': True, 'gen_normalmap': True, 'stereo_modes': ['left-right', 'red-cyan-anaglyph']}
    off, stats_off = _funnel(core, images, depthmaps, opts, False)
    on, stats_on = _funnel(core, images, depthmaps, opts, True)
    assert (stats_off["custom_depth_device"], stats_off["custom_depth_host"]) == (0, 4)
    assert (stats_on["custom_depth_device"], stats_on["custom_depth_host"]) == (3, 1)
    assert [(i, k) for i, k, _ in on] == [(i, k) for i, k, _ in off] and len(on) == 16
    for (i, kind, a), (_, _, b) in zip(off, on):
        assert a.mode == b.mode and a.size == b.size and a.tobytes() == b.tobytes(), (i, kind)
    # the depth output is what the reference's ingest and convert_to_i16 make of the map
    want = np.clip(_host(core, depthmaps[0], (128, 96)) * 65536 + 0.0001, 0, 65535.9).astype(np.uint16)
    assert np.array_equal(np.asarray(on[0][2]), want)


def test_funnel_mesh_same_vertices_either_route(gpu, native, tmp_path):
    """GEN_SIMPLE_MESH reads the float64 plane of the ingest (mesh_source): same file either way."""
    import src.core as core
    rng = np.random.default_rng(22)
    image = Image.fromarray(rng.integers(0, 256, (24, 32, 3)).astype(np.uint8))
    dp = _pil("I;16", random_plane("I;16", (12, 20), rng))
    opts = {'gen_simple_mesh': True, 'do_output_depth': False}
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    off, _ = _funnel(core, [image], [dp], opts, False, str(tmp_path / "off"))
    on, stats = _funnel(core, [image], [dp], opts, True, str(tmp_path / "on"))
    assert [k for _, k, _ in off] == [k for _, k, _ in on] == ['simple_mesh'] and stats["custom_depth_device"] == 1
    assert open(off[0][2]).read() == open(on[0][2]).read()
