"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as DIR/<name>.npy, so that two builds of the
project can be compared output by output on the same inputs.

Every output of a step is an image batch [units, rows, ...] (stereo pair [N, H, 2W, 3], uint16 depth [N, H, W], normal map
[N, H, W, 3]).  The files hold whole image rows: all of them when they fit in the budget, otherwise the SAME fixed, seeded sample
of (unit, row) pairs for every output (numpy default_rng(SAMPLE_SEED) over the N * H rows, sorted).  Integer sources are written
as float32 (exact for uint8 / uint16), float64 sources as float64.  manifest.json beside them records the source shapes and
dtypes and which rows were kept."""
import json
import os

import numpy as np

DUMP_BUDGET_BYTES = 60 * 2 ** 20       # all files together stay below 64 MB, .npy headers included
SAMPLE_SEED = 0


def kept_rows(n_rows, row_bytes, budget=DUMP_BUDGET_BYTES, seed=SAMPLE_SEED):
    """Indices of the rows to write: every row when they fit in `budget`, else a fixed seeded sample of them (sorted)."""
    keep = min(n_rows, budget // max(row_bytes, 1))
    if keep >= n_rows:
        return np.arange(n_rows)
    return np.sort(np.random.default_rng(seed).choice(n_rows, keep, replace=False))


def _host(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def dump_outputs(outdir, outputs, budget=DUMP_BUDGET_BYTES):
    """Write {name: array [units, rows, ...]} (torch tensors or numpy arrays with the same two leading axes) under `outdir`."""
    arrays = {name: _host(x) for name, x in outputs.items() if x is not None}
    lead = {a.shape[:2] for a in arrays.values()}
    assert len(lead) == 1, f"outputs do not share their (unit, row) axes: { {k: a.shape for k, a in arrays.items()} }"
    n_units, n_img_rows = lead.pop()
    out_type = {name: (np.float64 if a.dtype == np.float64 else np.float32) for name, a in arrays.items()}
    row_bytes = sum(int(np.prod(a.shape[2:], dtype=np.int64)) * np.dtype(out_type[n]).itemsize for n, a in arrays.items())
    rows = kept_rows(n_units * n_img_rows, row_bytes, budget)
    os.makedirs(outdir, exist_ok=True)
    manifest = {"rows_kept": int(rows.size), "rows_total": int(n_units * n_img_rows),
                "sample": None if rows.size == n_units * n_img_rows else
                f"numpy default_rng({SAMPLE_SEED}).choice(rows_total, rows_kept, replace=False), sorted; row r = unit r // "
                f"{n_img_rows}, image row r % {n_img_rows}",
                "rows": rows.tolist() if rows.size < n_units * n_img_rows else None, "files": {}}
    for name, a in arrays.items():
        flat = a.reshape((n_units * n_img_rows,) + a.shape[2:])
        np.save(os.path.join(outdir, name + ".npy"), flat[rows].astype(out_type[name]))
        manifest["files"][name + ".npy"] = {"source_shape": list(a.shape), "source_dtype": str(a.dtype),
                                            "dtype": np.dtype(out_type[name]).name}
    with open(os.path.join(outdir, "manifest.json"), "w") as f:
        json.dump(manifest, f)
    return manifest
