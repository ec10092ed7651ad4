"""Python restatement of the two-segment tile list of csrc/ds_linear.hip (k_linear256<.., VT 4>, ln_launch_qkv): the Q/K
projection's tiles followed by V^T's, walked by one persistent launch, and the launch rule that hands the left-over tiles of
the concatenated list to the V^T ragged kernel.  Integer arithmetic only; tests/test_linear_qkv_model.py checks the coverage."""


def tile_origin(nbm, nbn, tile):
    """ln_tile_origin: position in ONE GEMM's list -> (row panel, column panel); groups of 8 row panels, rows fastest in a group."""
    grp8, rem8 = divmod(tile, 8 * nbn)
    rows8 = min(8, nbm - 8 * grp8)
    bn, r = divmod(rem8, rows8)
    return 8 * grp8 + r, bn


def position_to_tile(orig, n_main):
    """set_tile's XCD-aware formula: workgroup position -> index into the walked list [0, n_main)."""
    xcd, q8, r8 = orig & 7, n_main >> 3, n_main & 7
    start = xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8
    return start + (orig >> 3)


def geometry(batch, tokens, qk_features, v_channels):
    """(nbm0, nbn0, nbm1, nbn1): segment 0 = tokens x Q/K features, segment 1 = V channels x tokens (ds_linear_qkv)."""
    rows = batch * tokens
    assert rows % 256 == 0 and qk_features % 256 == 0 and v_channels >= 256
    return rows // 256, qk_features // 256, (v_channels + 255) // 256, rows // 256


def launch_plan(t0, t1, grid, ragged_on=True, den=4):
    """ln_launch_qkv: (n_main of the persistent kernel, R tiles of the ragged launch, n_main of the V^T-alone ragged parameters)."""
    ntiles, ragged = t0 + t1, 0
    if ntiles > grid:
        r = ntiles % grid
        if ragged_on and r > 0 and den > 0 and den * r <= grid and r <= t1:
            ragged = r
    return ntiles - ragged, ragged, t1 - ragged


def main_tiles(geom, n_main, grid):
    """Every (segment, row panel, column panel) the persistent kernel renders, workgroup by workgroup, in walk order."""
    nbm0, nbn0, nbm1, nbn1 = geom
    t0 = nbm0 * nbn0
    out = []
    for wg in range(min(grid, n_main)):
        for orig in range(wg, n_main, grid):
            tile = position_to_tile(orig, n_main)
            if tile >= t0:
                out.append((wg, (1,) + tile_origin(nbm1, nbn1, tile - t0)))
            else:
                out.append((wg, (0,) + tile_origin(nbm0, nbn0, tile)))
    return out


def ragged_tiles(geom, ragged, vt_n_main):
    """The tiles k_linear_ragged renders from the V^T-alone parameters: positions vt_n_main .. of the V^T list."""
    _, _, nbm1, nbn1 = geom
    return [(1,) + tile_origin(nbm1, nbn1, vt_n_main + i) for i in range(ragged)]


def rounds(n_main, grid):
    """(whole rounds, tiles of a partial last round) of the persistent walk."""
    return divmod(n_main, grid)
