"""Python restatement of the row layout ds_preprocess_bicubic_rows writes (csrc/ds_forward_ends.hip, include/depthstereo.h): the zero
padded operand of the patch-embedding GEMM, one row per token slot of the padded sequence.  Integer indexing only;
tests/test_patch_rows_cpu.py checks it against the torch chain it replaces (patch gather + cat(cls) + pad_tokens)."""


def geometry(height, width, patch):
    """(gh, gw, n_valid, kpad) of an image of height x width pixels (n_pad is the caller's: vit_mi355x.pad_len of n_valid)."""
    gh, gw = height // patch, width // patch
    k = 3 * patch * patch
    return gh, gw, gh * gw + 1, (k + 127) // 128 * 128


def element(image, b, row, col, patch, gh, gw):
    """rows[b][row][col] for image[b][y][x][c] (any indexable of numbers).  Row 0 (the cls slot), the rows past the last patch and the
    columns past 3 * patch^2 are zero; pixels beyond gh * patch x gw * patch are never read."""
    k = 3 * patch * patch
    if row == 0 or row > gh * gw or col >= k:
        return 0
    gy, gx = divmod(row - 1, gw)
    pix, c = divmod(col, 3)
    py, px = divmod(pix, patch)
    return image[b][gy * patch + py][gx * patch + px][c]


def rows(image, batch, height, width, patch, n_pad, kpad):
    """The whole operand as nested lists [batch][n_pad][kpad]."""
    gh, gw = height // patch, width // patch
    assert n_pad >= 1 + gh * gw and kpad >= 3 * patch * patch
    return [[[element(image, b, r, col, patch, gh, gw) for col in range(kpad)] for r in range(n_pad)] for b in range(batch)]
