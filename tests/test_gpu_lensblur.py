"""Lens blur from depth (include/depthstereo.h: ds_lensblur_u8; src/lensblur_generation.py; ops={'lensblur': ...}) against the NumPy
model, tests/lensblur_cases.py.  Every comparison is torch.equal / np.array_equal: the definition is all-integer, so there is nothing
to tolerate.  Shapes: smaller than a tile (5 x 7), ragged in both directions with a focus per image (9 x 33), several 64 x 32 tiles at
the largest halo (40 x 70), narrower than the halo (17 x 16), 4 x 6 at R = 32 with A = 65535; radii 2 and 8, 16, 32 take the
kernel's three instantiations.  tests/test_lensblur_cpu.py shows that every case contains occluded taps, taps limited by the centre's
own blur, clamped and banded rho and skipped border taps."""
import numpy as np
import pytest

import lensblur_cases as lc

pytestmark = pytest.mark.gpu


def _case(case):
    shape, (R, aperture, focus, band) = lc.KERNEL_CASES[case]
    A = lc.quarter_pixels(aperture)
    image, depths = lc.inputs(shape, R, A)
    return shape, R, A, focus, band, image, depths


def _run(torch, image, depth, R, A, band, focus, invert=False, want_coc=True, out=None):
    from src import _native
    return _native.lensblur_u8(torch.from_numpy(np.array(image, order='C')).cuda(), torch.from_numpy(np.array(depth, order='C')).cuda(),
                               R, A, band, focus, invert=invert, want_coc=want_coc, out=out)


def _mismatch(got, want):
    return np.argwhere(got != want)[:6].tolist()


@pytest.mark.parametrize("case", range(len(lc.KERNEL_CASES)), ids=lc.KERNEL_IDS)
def test_kernel_equals_the_model_bit_for_bit(gpu, case):
    torch = gpu
    from src import _native
    shape, R, A, focus, band, image, depths = _case(case)
    for name in lc.DEPTHS:
        depth = depths[name]
        for invert in (False, True):
            before = _native.CALLS["ds_lensblur_u8"]
            rgb, coc = _run(torch, image, depth, R, A, band, lc.focus_list(depth, focus), invert)
            assert _native.CALLS["ds_lensblur_u8"] == before + 1
            assert rgb.dtype == torch.uint8 and coc.dtype == torch.uint8 and tuple(rgb.shape) == shape + (3,) and tuple(coc.shape) == shape
            assert rgb.is_cuda and coc.is_cuda
            want_rgb, want_coc = lc.want(case, name, invert)
            got_rgb, got_coc = rgb.cpu().numpy(), coc.cpu().numpy()
            assert np.array_equal(got_coc, want_coc), (name, invert, _mismatch(got_coc, want_coc))
            assert np.array_equal(got_rgb, want_rgb), (name, invert, _mismatch(got_rgb, want_rgb))
            alone = _run(torch, image, depth, R, A, band, lc.focus_list(depth, focus), invert, want_coc=False)         # out_coc == NULL
            assert torch.equal(alone, rgb), (name, invert)


def test_buffers_at_odd_addresses_give_the_same_bits(gpu):
    """image and out_rgb at odd byte addresses, depth at ptr % 8 == 2; nothing beside the output view is written."""
    torch = gpu
    from src import _native
    for case in range(4):
        shape, R, A, focus, band, image, depths = _case(case)
        n, h, w = shape
        count = n * h * w
        depth = depths["ramp"]
        ibuf = torch.zeros(3 * count + 8, dtype=torch.uint8, device="cuda")
        iview = ibuf[1:1 + 3 * count]
        iview.copy_(torch.from_numpy(image.copy()).cuda().view(-1))
        iview = iview.view(n, h, w, 3)
        dbuf = torch.zeros(count + 4, dtype=torch.uint16, device="cuda")
        dview = dbuf[1:1 + count]
        dview.copy_(torch.from_numpy(depth.copy()).cuda().view(-1))
        dview = dview.view(n, h, w)
        obuf = torch.full((3 * count + 8,), 77, dtype=torch.uint8, device="cuda")
        oview = obuf[3:3 + 3 * count].view(n, h, w, 3)
        assert iview.data_ptr() % 2 == 1 and dview.data_ptr() % 8 == 2 and oview.data_ptr() % 2 == 1
        assert iview.is_contiguous() and dview.is_contiguous() and oview.is_contiguous()
        got = _native.lensblur_u8(iview, dview, R, A, band, lc.focus_list(depth, focus), out=oview)
        assert got.data_ptr() == oview.data_ptr()
        assert np.array_equal(got.cpu().numpy(), lc.want(case, "ramp", False)[0]), shape
        assert bool((obuf[:3] == 77).all()) and bool((obuf[3 + 3 * count:] == 77).all())


def test_batch_invariance_and_independence(gpu):
    """Image 2 of a batch of 3 with three different focus values equals that image run alone; changing image 0 changes only output 0."""
    torch = gpu
    for (h, w), (R, A, band) in (((9, 33), (8, 96, 686)), ((40, 70), (32, 512, 130)), ((17, 16), (16, 160, 412))):
        span = lc.span_of(R, A)
        image = lc.random_image(h, w, h, n=3)
        depth = lc.ramp_noise(h, w, w, span, n=3)
        depth[1] = lc.cliff(h, w, 5, span // 2)
        focus = [int(depth[0, 0, 0]), int(depth[1].max()), int(depth[2, h // 2, w // 3])]
        assert len(set(focus)) == 3
        y3 = _run(torch, image, depth, R, A, band, focus)
        y1 = _run(torch, image[2:3], depth[2:3], R, A, band, focus[2:3])
        assert torch.equal(y3[0][2:3], y1[0]) and torch.equal(y3[1][2:3], y1[1]), (h, w)
        image2, depth2 = image.copy(), depth.copy()
        image2[0] = lc.random_image(h, w, h + 1)
        depth2[0] = lc.random_depth(h, w, w + 1)
        z3 = _run(torch, image2, depth2, R, A, band, focus)
        assert torch.equal(z3[0][1:], y3[0][1:]) and torch.equal(z3[1][1:], y3[1][1:]) and not torch.equal(z3[0][0], y3[0][0]), (h, w)
        # the focus values as a device tensor: the same launch
        f_t = torch.from_numpy(np.asarray(focus, np.uint16)).cuda()
        t3 = _run(torch, image, depth, R, A, band, f_t)
        assert torch.equal(t3[0], y3[0]) and torch.equal(t3[1], y3[1])


def test_point_focus_is_the_depth_read_there(gpu):
    torch = gpu
    shape, R, A, _, band, image, depths = _case(1)
    n, h, w = shape
    depth = depths["ramp"]
    for fx, fy in ((0.0, 0.0), (1.0, 1.0), (0.25, 0.5), (0.999, 0.001), (0.5, 1.0)):
        y, x = min(h - 1, int(np.floor(fy * h))), min(w - 1, int(np.floor(fx * w)))
        explicit = [int(depth[i, y, x]) for i in range(n)]
        a = _run(torch, image, depth, R, A, band, ('point', fx, fy))
        b = _run(torch, image, depth, R, A, band, explicit)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (fx, fy)
        assert np.array_equal(a[0].cpu().numpy(), lc.model(image, depth, [('point', fx, fy)] * n, R, A, band)[0])
    one = _run(torch, image, depth, R, A, band, 40000)                      # one integer for every image, above 32767
    assert np.array_equal(one[0].cpu().numpy(), lc.model(image, depth, [40000] * n, R, A, band)[0])


def test_table_cache_is_bounded(gpu):
    torch = gpu
    from src import _native
    image, depth = lc.random_image(8, 8, 1, n=1), lc.ramp_noise(8, 8, 2, 30000, n=1)
    first = _run(torch, image, depth, 3, 400, 0, 9000)[0]
    for r in range(4, 10):
        _run(torch, image, depth, r, 400, 0, 9000)
    assert _native.cached_tables("lensblur") == 4
    _run(torch, image, depth, 9, 999, 5, 10000)                             # A, band and focus are no part of the key
    assert _native.cached_tables("lensblur") == 4
    assert torch.equal(_run(torch, image, depth, 3, 400, 0, 9000)[0], first)   # evicted and rebuilt: same bits
    assert _native.cached_tables("lensblur") == 4
    assert np.array_equal(first.cpu().numpy(), lc.model(image, depth, [9000], 3, 400, 0)[0])


def test_entry_point_checks_its_arguments_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    ctx = _native.ctx_for(torch.cuda.current_device())
    EINVAL, SENT = -1, 93
    n, h, w, r = 1, 8, 12, 2
    count = n * h * w
    tabs = {R: torch.from_numpy(_native.lensblur_table(R)[0]).cuda() for R in (1, 2, 32)}
    img = torch.full((n, h, w, 3), 50, dtype=torch.uint8, device="cuda")
    dep = torch.zeros((n, h, w), dtype=torch.int16, device="cuda")
    foc = torch.zeros((4,), dtype=torch.int16, device="cuda")
    out = torch.full((n, h, w, 3), SENT, dtype=torch.uint8, device="cuda")
    coc = torch.full((n, h, w), SENT, dtype=torch.uint8, device="cuda")
    big = torch.full((16 * count,), SENT, dtype=torch.uint8, device="cuda")  # one block to carve overlapping buffers from
    B = big.data_ptr()
    assert B % 8 == 0 and count % 2 == 0

    def call(c=ctx, ip=img.data_ptr(), dp=dep.data_ptr(), fp=foc.data_ptr(), n=n, h=h, w=w, r=r, a=200, band=0, invert=0, tp=-1,
             op=out.data_ptr(), cp=coc.data_ptr()):
        table = tabs.get(r, tabs[2])                                          # (an illegal r gets some real table)
        return L.ds_lensblur_u8(c, ip, dp, fp, n, h, w, r, a, band, invert, table.data_ptr() if tp == -1 else tp, op, cp, None)
    assert call(c=None) == EINVAL and call(ip=None) == EINVAL and call(dp=None) == EINVAL and call(fp=None) == EINVAL
    assert call(tp=None) == EINVAL and call(op=None) == EINVAL
    assert call(n=0) == EINVAL and call(h=0) == EINVAL and call(w=-3) == EINVAL and call(n=-1) == EINVAL
    assert call(r=0) == EINVAL and call(r=33) == EINVAL and call(r=-1) == EINVAL
    assert call(a=0) == EINVAL and call(a=65536) == EINVAL and call(a=-5) == EINVAL
    assert call(band=-1) == EINVAL and call(band=65536) == EINVAL
    # alignment: table 4 bytes; focus and depth 2 bytes
    assert call(tp=tabs[2].data_ptr() + 2) == EINVAL and call(tp=tabs[2].data_ptr() + 1) == EINVAL
    assert call(fp=foc.data_ptr() + 1) == EINVAL and call(dp=dep.data_ptr() + 1) == EINVAL
    # out_rgb (3 count bytes) against every input: equal pointers, and beginning in the other's last byte
    assert call(ip=B, op=B) == EINVAL and call(ip=B, op=B + 3 * count - 1) == EINVAL and call(ip=B + 3 * count - 1, op=B) == EINVAL
    assert call(dp=B, op=B) == EINVAL and call(dp=B, op=B + 2 * count - 1) == EINVAL and call(dp=B + 3 * count - 2, op=B) == EINVAL
    assert call(fp=B, op=B) == EINVAL and call(fp=B + 2, op=B + 3) == EINVAL and call(fp=B + 3 * count - 2, op=B) == EINVAL
    assert call(tp=B, op=B) == EINVAL and call(tp=B, op=B + 4 * (4 * r + 1) - 1) == EINVAL and call(tp=B + 3 * count - 4, op=B) == EINVAL
    # out_coc (count bytes) against every input and against out_rgb
    assert call(ip=B, cp=B) == EINVAL and call(ip=B, cp=B + 3 * count - 1) == EINVAL and call(ip=B + count - 1, cp=B) == EINVAL
    assert call(dp=B, cp=B) == EINVAL and call(dp=B + count - 2, cp=B) == EINVAL
    assert call(fp=B, cp=B + 1) == EINVAL and call(tp=B, cp=B + 4 * (4 * r + 1) - 1) == EINVAL
    assert call(op=B, cp=B) == EINVAL and call(op=B, cp=B + 3 * count - 1) == EINVAL and call(op=B + count - 1, cp=B) == EINVAL
    # the grid limit: n = 65536 one-pixel images (every buffer really that large): DS_EUNSUPPORTED
    imn = torch.full((65536, 1, 1, 3), 9, dtype=torch.uint8, device="cuda")
    den = torch.zeros((65536, 1, 1), dtype=torch.int16, device="cuda")
    fon = torch.zeros((65536,), dtype=torch.int16, device="cuda")
    on = torch.full((65536, 1, 1, 3), SENT, dtype=torch.uint8, device="cuda")
    many = dict(ip=imn.data_ptr(), dp=den.data_ptr(), fp=fon.data_ptr(), op=on.data_ptr(), cp=None, h=1, w=1)
    assert call(n=65536, **many) == -2
    torch.cuda.synchronize()
    assert b"ds_lensblur_u8" in L.ds_last_error()
    assert bool((out == SENT).all()) and bool((coc == SENT).all()) and bool((big == SENT).all()) and bool((on == SENT).all())
    # and the legal neighbours of those cases run: the ends of every range, out_coc == NULL, outputs at odd addresses, adjacent but
    # disjoint blocks
    assert call(r=1, a=1) == 0 and call(r=32, a=65535, band=65535) == 0 and call(invert=1) == 0
    assert call(cp=None) == 0 and call(op=B + 1, cp=B + 1 + 3 * count) == 0
    assert call(ip=B + 4 * count + 1, op=B, cp=B + 3 * count) == 0           # image behind the outputs, at an odd address
    assert call(dp=B + 4 * count, fp=B + 6 * count, op=B, cp=B + 3 * count) == 0   # depth begins where out_coc ends, focus where depth ends
    assert call(n=65535, **many) == 0
    torch.cuda.synchronize()
    assert bool((on[:65535] == 9).all()) and bool((on[65535] == SENT).all())
    assert bool((out == 50).all()) and bool((coc == 0).all())                # flat depth at the focus: the image, rho 0, written


def test_public_interface(gpu):
    torch = gpu
    from PIL import Image
    from src import _native
    import src.lensblur_generation as lg
    h, w = 12, 20
    image = lc.random_image(h, w, 3)
    d = lc.ramp_noise(h, w, 4, 30000)
    x, im = torch.from_numpy(d).cuda()[None], torch.from_numpy(image).cuda()[None]
    for kwargs in ({}, {'radius': 5, 'aperture': 20.0, 'focus': 20000, 'band': 300, 'invert': True}, {'focus': ('point', 0.9, 0.1)}):
        R, ap = kwargs.get('radius', 12), kwargs.get('aperture', 48.0)
        want = lc.model(image, d, kwargs.get('focus', ('point', 0.5, 0.5)), R, lc.quarter_pixels(ap), kwargs.get('band', 0),
                        kwargs.get('invert', False))[0]
        batch = lg.create_lensblur_batch(im, x, **kwargs)
        assert batch.is_cuda and batch.dtype == torch.uint8 and tuple(batch.shape) == (1, h, w, 3)
        assert np.array_equal(batch[0].cpu().numpy(), want)
        for pixels in (image, Image.fromarray(image)):
            for depth in (d, Image.fromarray(d)):
                got = lg.create_lensblur(pixels, depth, **kwargs)
                assert isinstance(got, Image.Image) and got.mode == 'RGB' and got.size == (w, h)
                assert np.array_equal(np.asarray(got), want)
    # per-image focus in the batch interface: a list and a device tensor
    im2, x2 = torch.cat([im, im]), torch.cat([x, x])
    two = lg.create_lensblur_batch(im2, x2, 6, 30.0, [12000, 30000], 100)
    for i, f in enumerate((12000, 30000)):
        assert np.array_equal(two[i].cpu().numpy(), lc.model(image, d, f, 6, 120, 100)[0])
    assert torch.equal(lg.create_lensblur_batch(im2, x2, 6, 30.0, torch.from_numpy(np.array([12000, 30000], np.uint16)).cuda(), 100), two)
    before = dict(_native.CALLS)
    for bad_depth in (d.astype(np.float32), d.astype(np.int32), d.astype(np.uint8), d.astype(np.int16), d.astype(np.float64),
                      Image.fromarray(d.astype(np.uint8)), d[None], d[:0], d[:, :-1], d[:-1]):
        with pytest.raises(_native.DepthStereoError):
            lg.create_lensblur(image, bad_depth)
    for bad_image in (image.astype(np.float32), image[..., :2], image[None]):
        with pytest.raises(_native.DepthStereoError):
            lg.create_lensblur(bad_image, d)
    for bad in ({'radius': 0}, {'radius': 33}, {'radius': True}, {'radius': 2.5}, {'aperture': 0.0}, {'aperture': float('nan')},
                {'aperture': 20000.0}, {'focus': -1}, {'focus': 65536}, {'focus': ('point', 2.0, 0.5)}, {'focus': 'near'}, {'band': -1},
                {'band': 65536}, {'band': True}):
        with pytest.raises(_native.DepthStereoError):
            lg.create_lensblur(image, d, **bad)
        with pytest.raises(_native.DepthStereoError):
            lg.create_lensblur_batch(im, x, **bad)
    for bad_x in (x.to(torch.int32), x.view(torch.int16), x.to(torch.float32), x[0], x.cpu(), d, x[:, :-1]):
        with pytest.raises(_native.DepthStereoError):
            lg.create_lensblur_batch(im, bad_x)
    for bad_im in (im.to(torch.float32), im[..., :2], im[0], im.cpu(), image):
        with pytest.raises(_native.DepthStereoError):
            lg.create_lensblur_batch(bad_im, x)
    for bad_focus in ([1, 2], [1.5], torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int16, device="cuda").view(torch.uint16)):
        with pytest.raises(_native.DepthStereoError):
            lg.create_lensblur_batch(im, x, focus=bad_focus)
    assert dict(_native.CALLS) == before


def test_funnel_lensblur_is_an_option_of_the_call(gpu):
    """core_generation_funnel(..., ops={'lensblur': P}) with caller-supplied I;16 depth maps (no network involved)."""
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.lensblur_generation as lg
    from src import _native
    h, w = 24, 40
    P = (6, 30.0, ('point', 0.25, 0.5), 200)
    AO = (6, 8, 300.0)
    rng = np.random.default_rng(5)
    imgs = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(2)]
    d16 = [lc.cliff(h, w, 1, 30000), lc.ramp_noise(h, w, 40, 40000)]
    base = {'gen_stereo': True, 'gen_normalmap': True, 'gen_heatmap': True, 'stereo_modes': ['left-right']}
    plain_kinds = ['depth', 'left-right', 'normalmap', 'heatmap']

    def run(ops, opts=base, kinds=plain_kinds, images=imgs):
        got = list(core.core_generation_funnel(None, list(images), [Image.fromarray(d) for d in d16], None, dict(opts), ops))
        assert [(i, k) for i, k, _ in got] == [(i, k) for i in range(2) for k in kinds], [(i, k) for i, k, _ in got]
        for _, k, r in got:
            if k == 'lensblur':
                assert isinstance(r, Image.Image) and r.mode == 'RGB' and r.size == (w, h)
        return {k: [r if isinstance(r, str) else np.asarray(r) for _, kk, r in got if kk == k] for k in kinds}

    def same(a, b):
        return set(a) == set(b) and all(len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) for k in a)

    def delta(before):
        return {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}

    run(None)                                                                 # (whatever a first call does once is done)
    before = dict(_native.CALLS)
    plain = run(None)
    plain_delta = delta(before)
    assert "ds_lensblur_u8" not in plain_delta
    own = plain['depth']                                                      # the funnel's own uint16 depth output

    def expect(params, images=imgs):
        return dict(plain, lensblur=[np.asarray(lg.create_lensblur(im, d, *params)) for im, d in zip(images, own)])

    want = expect(P)
    for got, im, d in zip(want['lensblur'], imgs, own):
        assert np.array_equal(got, lc.model(np.asarray(im), d, P[2], P[0], lc.quarter_pixels(P[1]), P[3])[0]) and not np.array_equal(got, np.asarray(im))
    before = dict(_native.CALLS)
    got = run({'lensblur': P}, kinds=plain_kinds + ['lensblur'])              # after 'heatmap', every other output as it was
    assert same(got, want)
    assert delta(before) == dict(plain_delta, ds_lensblur_u8=1)               # one group: one launch, nothing else changes
    # gone on the next call; absent, None and {} make the launches and the bytes of a plain call
    for ops in (None, {}, {'lensblur': None}):
        before = dict(_native.CALLS)
        assert same(run(ops), plain), ops
        assert delta(before) == plain_delta, ops
    assert same(run({'lensblur': list(P[:3])}, kinds=plain_kinds + ['lensblur']), expect(P[:3]))        # band defaults to 0
    # after 'aomap' when both are asked for
    both = run({'lensblur': P, 'aomap': AO}, kinds=plain_kinds + ['aomap', 'lensblur'])
    assert same({k: both[k] for k in want}, want)
    # alone (the pixels are uploaded for it), and from images that are not RGB (taken as their convert("RGB"))
    only = run({'lensblur': P}, {'do_output_depth': False}, ['lensblur'])
    assert same(only, {'lensblur': want['lensblur']})
    rgba = [im.convert('RGBA') for im in imgs]
    assert same(run({'lensblur': P}, {'do_output_depth': False}, ['lensblur'], images=rgba), {'lensblur': want['lensblur']})
    assert not hasattr(core.model_holder, 'lensblur')                         # the option does not become a holder setting
    for bad in ({'lensblur': (0, 30.0, 0)}, {'lensblur': (6, 0.0, 0)}, {'lensblur': (6, 30.0)}, {'lensblur': "6"}, {'lensblur': (6, 30.0, -1)},
                {'lensblur': (True, 30.0, 0)}, {'lensblur': (6, 30.0, ('point', 2.0, 0.5))}, {'lensblur': (6, 30.0, 0, 70000)}):
        before = dict(_native.CALLS)
        with pytest.raises(ValueError):
            run(bad)
        assert dict(_native.CALLS) == before, bad                             # before any device work
    assert same(run(None), plain)


def test_funnel_lensblur_reads_the_refined_map_and_precedes_the_mesh(gpu, tmp_path):
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.lensblur_generation as lg
    h, w = 24, 40
    P, REFINE = (6, 30.0, 9000, 100), (5, 60.0, 2.0)
    rng = np.random.default_rng(6)
    img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    d = lc.cliff(h, w, 2, 30000)
    got = list(core.core_generation_funnel(str(tmp_path), [img], [Image.fromarray(d)], None,
                                           {'gen_heatmap': True, 'gen_simple_mesh': True}, {'lensblur': P, 'depth_refine': REFINE}))
    assert [k for _, k, _ in got] == ['depth', 'heatmap', 'lensblur', 'simple_mesh']
    refined = np.asarray(got[0][2])
    plain = np.asarray(next(r for _, k, r in core.core_generation_funnel(None, [img], [Image.fromarray(d)], None, {}, None) if k == 'depth'))
    assert not np.array_equal(refined, plain)
    assert np.array_equal(np.asarray(got[2][2]), np.asarray(lg.create_lensblur(img, refined, *P)))
    assert not np.array_equal(np.asarray(got[2][2]), np.asarray(lg.create_lensblur(img, plain, *P)))
