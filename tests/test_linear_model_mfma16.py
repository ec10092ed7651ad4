"""CPU checks of the 16x16x32 chain of csrc/ds_linear.hip (tools/linear_model.py): its fragment reads of the unchanged swizzled
LDS image are bank-conflict free, and the index chain (DMA source swizzle -> LDS image -> 16 x 32 fragment reads -> MFMA
16x16x32 operand / accumulator layout -> permlane16_swap epilogue, shifted last row panel) reproduces x @ W.T with every
output written."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import linear_model as lm  # noqa: E402


def test_16x16x32_fragment_reads_are_bank_conflict_free():
    assert lm.bank_conflicts16() == 0


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (256, 512, 64)])
def test_16x16x32_index_chain_reproduces_the_product(M, N, K):
    assert lm.check_indexing16(M=M, N=N, K=K) < 1e-9


def test_permlane16_swap_gives_each_lane_8_consecutive_columns():
    """accumulator register r of column block cb = column 16 cb + 4 (lane >> 4) + r; after the swap a lane holds the 8 columns
    epilogue_cols16(lane) .. + 7 and the four 16-lane groups cover the 32 columns of the W half once"""
    lanes = np.arange(64)
    blk = [np.stack([16 * cb + 4 * (lanes >> 4) + r for r in range(4)], 1).astype(float) for cb in range(2)]
    lo, hi = lm.permlane16_swap(blk[0], blk[1])
    cover = set()
    for lane in range(64):
        c0 = lm.epilogue_cols16(lane)
        assert list(np.concatenate([lo[lane], hi[lane]])) == list(range(c0, c0 + 8))
        if lane & 15 == 0:
            cover.update(range(c0, c0 + 8))
    assert cover == set(range(32))
