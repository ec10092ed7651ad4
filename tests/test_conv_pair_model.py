"""CPU checks of the two-segment tile list of ds_conv3x3_nhwc_pair (tools/conv_pair_model.py restates k_linear256<.., VT 5>'s set_tile
and the dummy-row rule of its epilogue) against brute force: every output row of both segments is stored in every column panel, no
row of the other segment or behind the dummy row is touched, every workgroup renders its share, and the shapes of the benchmark fit
one round."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import conv_pair_model as pm  # noqa: E402

# (name, grid, pixels of segment 0, pixels of segment 1, out_channels): the shapes of tests/test_gpu_conv3x3_pair.py, then layer3_rn +
# layer4_rn of dpt_beit_large_512 at batch 32 (c3) and of its net-1024 form (c3match: 640 tiles, more than one round)
SHAPES = [("4+1", 8, 1024, 256, 256), ("4+partial", 8, 1024, 192, 256), ("4+1 default", 256, 1024, 256, 256), ("16+partial", 8, 4096, 192, 256),
          ("shifted", 8, 480, 300, 256), ("two column panels", 8, 700, 100, 512), ("c3", 256, 32768, 8192, 256), ("c3match", 256, 131072, 32768, 256)]


@pytest.mark.parametrize("name,grid,p0,p1,n", SHAPES)
def test_every_output_row_is_stored_and_nothing_else(name, grid, p0, p1, n):
    got = set(pm.stores(p0, p1, n, grid))
    want = {(seg, r, bn) for seg, pixels in ((0, p0), (1, p1)) for r in range(pixels) for bn in range(n // 256)}
    dummy = {(seg, pixels, bn) for seg, pixels in ((0, p0), (1, p1)) for bn in range(n // 256)}
    assert want <= got and got - want <= dummy
    assert (got & dummy) == {d for d in dummy if (p1 if d[0] else p0) < 256}        # only a segment below one tile has rows to drop


@pytest.mark.parametrize("name,grid,p0,p1,n", SHAPES)
def test_the_walk_is_a_partition_of_the_tile_list(name, grid, p0, p1, n):
    nbm0, nbm1, nbn = pm.geometry(p0, p1, n)
    walk = pm.walk(p0, p1, n, grid)
    assert len(walk) == (nbm0 + nbm1) * nbn == len({(seg, r0, bn) for _, seg, r0, bn in walk})
    per_wg = [sum(1 for w in walk if w[0] == wg) for wg in range(min(grid, len(walk)))]
    assert max(per_wg) - min(per_wg) <= 1 and min(per_wg) >= 1


def test_which_shapes_fit_one_round():
    assert pm.fits_one_round(32768, 8192, 256, 256)             # c3: 128 + 32 tiles on 256 workgroups
    assert not pm.fits_one_round(131072, 32768, 256, 256)       # c3match: 512 + 128
    walk = pm.walk(4096, 192, 256, 8)
    last = [w for w in walk if w[0] == 7]
    assert [w[1] for w in last] == [0, 1], last                 # one workgroup walks from segment 0 into segment 1
