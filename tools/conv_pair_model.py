"""Python restatement of the two-segment tile list of ds_conv3x3_nhwc_pair (csrc/ds_linear.hip: k_linear256<.., VT 5>): the tiles of
the first convolution followed by those of the second, walked by one persistent launch; rows of a partial tile behind a segment's
last pixel go to that segment's dummy row.  Integer arithmetic only; tests/test_conv_pair_model.py checks the coverage against brute
force.  (tile_origin and position_to_tile are the single-list formulas of tools/linear_qkv_model.py.)"""
from linear_qkv_model import position_to_tile, tile_origin


def geometry(pixels0, pixels1, out_channels):
    """(nbm0, nbm1, nbn): row panels of the two segments, common column panels."""
    assert pixels0 >= 1 and pixels1 >= 1 and out_channels % 256 == 0
    return (pixels0 + 255) // 256, (pixels1 + 255) // 256, out_channels // 256


def first_row(nbm, pixels, bm):
    """Origin row of row panel bm: the last panel is shifted up to end at the last pixel; a segment below 256 pixels starts at 0."""
    return max(min(bm * 256, pixels - 256), 0)


def walk(pixels0, pixels1, out_channels, grid):
    """Every (workgroup, segment, first row, column panel) of the launch, in walk order."""
    nbm0, nbm1, nbn = geometry(pixels0, pixels1, out_channels)
    t0, n = nbm0 * nbn, (nbm0 + nbm1) * nbn
    out = []
    for wg in range(min(grid, n)):
        for orig in range(wg, n, grid):
            tile = position_to_tile(orig, n)
            seg = 1 if tile >= t0 else 0
            bm, bn = tile_origin(nbm1 if seg else nbm0, nbn, tile - (t0 if seg else 0))
            out.append((wg, seg, first_row(nbm1 if seg else nbm0, pixels1 if seg else pixels0, bm), bn))
    return out


def stores(pixels0, pixels1, out_channels, grid):
    """(segment, output row, column panel) of every 256-column row a tile stores; rows behind the segment become its dummy row."""
    out = []
    for _, seg, r0, bn in walk(pixels0, pixels1, out_channels, grid):
        pixels = pixels1 if seg else pixels0
        out += [(seg, r if r < pixels else pixels, bn) for r in range(r0, r0 + 256)]
    return out


def fits_one_round(pixels0, pixels1, out_channels, grid):
    """The routing rule of vit_mi355x.conv2d_pair: both tile lists together are at most one tile per workgroup."""
    nbm0, nbm1, nbn = geometry(pixels0, pixels1, out_channels)
    return (nbm0 + nbm1) * nbn <= grid
