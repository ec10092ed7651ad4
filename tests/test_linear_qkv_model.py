"""CPU checks of the two-segment tile list of ds_linear_qkv (tools/linear_qkv_model.py restates k_linear256<.., VT 4>'s set_tile and
ln_launch_qkv's launch rule): every tile of both GEMMs is rendered exactly once by the persistent launch and the ragged launch
together, the ragged tiles are V^T tiles, and the shapes of the benchmark give the round counts the route was built for."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import linear_qkv_model as qm  # noqa: E402

# (name, grid, batch, tokens, qk_features, v_channels): (a) - (d) are the shapes of tests/test_gpu_linear_qkv.py, c3 / c5 the
# encoder blocks of bench.py's configurations (dpt_beit_large_512 at batch 32; Depth-Anything-V2 ViT-L with 77 row panels)
SHAPES = [("a", 8, 2, 768, 512, 256), ("a2", 8, 1, 768, 768, 768), ("b", 8, 2, 640, 512, 256), ("c", 8, 1, 256, 2304, 256), ("d", 256, 32, 1032, 2048, 1024),
          ("c3", 256, 32, 1032, 2048, 1024), ("c5", 256, 1, 77 * 256, 2048, 1024), ("block_g", 256, 8, 1056, 2048, 1024)]


def _all_tiles(geom):
    nbm0, nbn0, nbm1, nbn1 = geom
    return sorted([(0, m, n) for m in range(nbm0) for n in range(nbn0)] + [(1, m, n) for m in range(nbm1) for n in range(nbn1)])


@pytest.mark.parametrize("name,grid,batch,tokens,nqk,c", SHAPES)
@pytest.mark.parametrize("ragged_on", [True, False])
def test_every_tile_is_rendered_exactly_once(name, grid, batch, tokens, nqk, c, ragged_on):
    geom = qm.geometry(batch, tokens, nqk, c)
    t0, t1 = geom[0] * geom[1], geom[2] * geom[3]
    n_main, ragged, vt_n_main = qm.launch_plan(t0, t1, grid, ragged_on)
    assert n_main + ragged == t0 + t1 and vt_n_main == t1 - ragged and 0 <= ragged <= t1
    main = [t for _, t in qm.main_tiles(geom, n_main, grid)]
    rag = qm.ragged_tiles(geom, ragged, vt_n_main)
    assert all(t[0] == 1 for t in rag), "a ragged tile that is not V^T"
    assert sorted(main + rag) == _all_tiles(geom)
    if not ragged_on:
        assert ragged == 0
    assert len(main) == n_main and len(rag) == ragged


def _crossing(geom, n_main, grid):
    """Workgroups that render a tile of segment 0 and then one of segment 1."""
    walk = qm.main_tiles(geom, n_main, grid)
    out = []
    for wg in range(min(grid, n_main)):
        segs = [t[0] for w, t in walk if w == wg]
        assert segs == sorted(segs), "a workgroup walks back from V^T into Q/K"
        if set(segs) == {0, 1}:
            out.append(wg)
    return out


def test_small_shapes_take_the_paths_they_were_chosen_for():
    plan = {n: (qm.geometry(b, t, q, c), g) for n, g, b, t, q, c in SHAPES}
    geom, grid = plan["a"]                                      # 12 + 6 tiles: two whole rounds + 2 ragged V^T tiles
    assert (geom[0] * geom[1], geom[2] * geom[3]) == (12, 6) and qm.launch_plan(12, 6, grid) == (16, 2, 4)
    # (an XCD takes a CONTIGUOUS range of the list, here 2 tiles per workgroup, and 12 is even: the boundary falls BETWEEN two
    # workgroups.  Shape a2, 9 + 9 tiles, puts it inside workgroup 4's range -- a tile of segment 0 followed by one of segment 1, the
    # order in which the early mode's set_tile(next) changes the segment under the running epilogue -- and so does the benchmark's)
    assert _crossing(geom, 16, grid) == []
    geom, grid = plan["a2"]
    assert (geom[0] * geom[1], geom[2] * geom[3]) == (9, 9) and qm.launch_plan(9, 9, grid) == (16, 2, 7)
    assert _crossing(geom, 16, grid) == [4]
    geom, grid = plan["d"]
    assert len(_crossing(geom, 1536, grid)) == 32               # XCD 5's range [960, 1152) holds the boundary at 1032: all its workgroups
    geom, grid = plan["b"]                                      # 10 + 5 tiles: no ragged round, one whole round + 7, ends inside V^T
    assert qm.launch_plan(10, 5, grid) == (15, 0, 5) and qm.rounds(15, grid) == (1, 7)
    assert max(qm.position_to_tile(o, 15) for o in range(15)) == 14
    geom, grid = plan["c"]                                      # 9 + 1 tiles: R = 2 > T1 = 1, the persistent kernel walks everything
    assert (geom[0] * geom[1], geom[2] * geom[3]) == (9, 1) and qm.launch_plan(9, 1, grid) == (10, 0, 1)
    assert sorted(t for _, t in qm.main_tiles(geom, 10, grid)) == _all_tiles(geom)


def test_benchmark_shapes_give_six_rounds_plus_twelve_and_four_rounds():
    geom = qm.geometry(32, 1032, 2048, 1024)                    # c3: 129 row panels
    t0, t1 = geom[0] * geom[1], geom[2] * geom[3]
    assert (t0, t1) == (1032, 516)
    n_main, ragged, vt_n_main = qm.launch_plan(t0, t1, 256)
    assert (n_main, ragged, vt_n_main) == (6 * 256, 12, 504) and qm.rounds(n_main, 256) == (6, 0)
    # the two launches it replaces: 4 rounds + 8 left over (one row panel: the thin round), 2 rounds + 4 left over
    assert divmod(t0, 256) == (4, 8) and divmod(t1, 256) == (2, 4)
    geom = qm.geometry(1, 77 * 256, 2048, 1024)                 # c5: 77 row panels
    t0, t1 = geom[0] * geom[1], geom[2] * geom[3]
    assert (t0, t1) == (616, 308) and qm.launch_plan(t0, t1, 256) == (924, 0, 308) and qm.rounds(924, 256) == (3, 156)
    assert -(-t0 // 256) == 3 and divmod(t1, 256) == (1, 52)    # before: 3 rounds, and 1 round + a ragged round of 52 tiles


def test_xcd_map_is_a_bijection_for_every_list_length():
    for n in range(1, 70):
        assert sorted(qm.position_to_tile(o, n) for o in range(n)) == list(range(n))
