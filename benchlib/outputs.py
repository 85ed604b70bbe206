"""--dump-outputs DIR: the arrays the timed path computed in its last step, one DIR/<name>.npy each, so that two builds run with the
same arguments can be compared output for output.  Floating-point arrays are written as they are (float32 / float64), flags, bits
and indices as float32 where every value is exact in it (below 2^24) and as float64 otherwise.  An array of more than MAX_ELEMS
elements is cut to a fixed, seeded sample of its rows (ascending), the same rows in every run of the same shape."""
import os

import numpy as np

MAX_ELEMS = 4_000_000            # per array: 16 MB of float32
MAX_TOTAL_BYTES = 64 * 1000 * 1000
SAMPLE_SEED = 20240


def as_float(a):
    a = np.asarray(a)
    if a.dtype in (np.float32, np.float64):
        return a
    if a.size and int(np.abs(a.astype(np.int64)).max()) >= 1 << 24:
        return a.astype(np.float64)
    return a.astype(np.float32)


def sample_rows(a):
    if a.size <= MAX_ELEMS:
        return a
    per_row = a.size // a.shape[0]
    keep = np.sort(np.random.default_rng(SAMPLE_SEED).choice(a.shape[0], MAX_ELEMS // per_row, replace=False))
    return a[keep]


def write(out_dir, arrays):
    """arrays: {name: array}.  Returns {name: path}."""
    os.makedirs(out_dir, exist_ok=True)
    ready = {name: np.ascontiguousarray(as_float(sample_rows(np.asarray(a)))) for name, a in arrays.items()}
    total = sum(a.nbytes for a in ready.values())
    if total > MAX_TOTAL_BYTES:
        raise ValueError(f"--dump-outputs: {total} bytes in {len(ready)} arrays, over the {MAX_TOTAL_BYTES} allowed")
    paths = {}
    for name, a in ready.items():
        paths[name] = os.path.join(out_dir, name + ".npy")
        np.save(paths[name], a)
    return paths
