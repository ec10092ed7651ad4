#!/usr/bin/env python3
"""Golden outputs of the REFERENCE's own ``sparse_bilateral_filtering`` (inpaint/bilateral_filtering.py), imported unmodified, on the
seeded inputs of tests/sparse_bilateral_cases.py.

Build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sparse_bilateral.py <path of the reference checkout>

Output: sparse_bilateral_cases.npz, the returned arrays only (``<case>__depth<i>``, ``<case>__image<i>``); the inputs are regenerated
from their seeds by the tests.  Before anything is written the census of the inputs is checked: the windows met must include every
n <= 49 at which the reference's rank is not n // 2, n == 0, and one such n above 49 -- an input that misses one is changed, never the
condition.  The model of the cases file is NOT consulted for the outputs, only for that census."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], 'inpaint', 'bilateral_filtering.py')):
        sys.exit(__doc__)
    import sparse_bilateral_cases as sc
    seen = sc.census_of_all_cases()
    assert sc.census_is_complete(seen), sorted(seen)
    sys.path.insert(0, sys.argv[1])
    from inpaint.bilateral_filtering import sparse_bilateral_filtering
    out = {}
    for name, (depth, image, config, num_iter) in sc.cases().items():
        images, depths = sparse_bilateral_filtering(depth.copy(), image.copy(), dict(config), num_iter=num_iter)
        assert len(images) == len(depths) == num_iter
        for i, (im, d) in enumerate(zip(images, depths)):
            assert d.dtype == np.float32 and im.dtype == np.uint8
            out[f'{name}__depth{i}'] = d
            out[f'{name}__image{i}'] = im
    np.savez_compressed(os.path.join(HERE, 'sparse_bilateral_cases.npz'), **out)
    print('wrote', len(sc.cases()), 'cases,', len(out), 'arrays; census', sorted(seen))


if __name__ == '__main__':
    main()
