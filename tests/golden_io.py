"""Loaders for the committed golden fixtures (tests/golden/, made by make_golden.py)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# a committed fixture file stays under this size: larger sets are stored as <name>.partNN.npz
PART_BYTES = 900_000


class Parts:
    """The arrays of several .npz files behind the part of NpzFile's interface the tests use."""

    def __init__(self, paths):
        self._where = {}
        for p in paths:
            z = np.load(p, allow_pickle=False)
            for k in z.files:
                self._where[k] = z
        self.files = list(self._where)

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where


def save(name, arrays, golden=GOLDEN):
    """Write the arrays as <name>.npz, or as <name>.part00.npz, <name>.part01.npz, ... (keys in
    order, each file under PART_BYTES) when one file would be larger."""
    import glob
    import io
    import zipfile
    for old in [os.path.join(golden, name + ".npz")] + glob.glob(os.path.join(golden, name + ".part*.npz")):
        if os.path.exists(old):
            os.remove(old)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    if buf.tell() <= PART_BYTES:
        with open(os.path.join(golden, name + ".npz"), "wb") as f:
            f.write(buf.getvalue())
        return 1
    size = {i.filename[:-len(".npy")]: i.compress_size + 2 * len(i.filename) + 128
            for i in zipfile.ZipFile(buf).infolist()}
    parts, cur, cur_bytes = [], {}, 0
    for k, v in arrays.items():
        if cur and cur_bytes + size[k] > PART_BYTES:
            parts.append(cur)
            cur, cur_bytes = {}, 0
        cur[k] = v
        cur_bytes += size[k]
    parts.append(cur)
    for i, part in enumerate(parts):
        np.savez_compressed(os.path.join(golden, f"{name}.part{i:02d}.npz"), **part)
    return len(parts)


def load(name):
    import glob
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)
    one = os.path.join(GOLDEN, name + ".npz")
    if os.path.exists(one):
        return meta, np.load(one, allow_pickle=False)
    parts = sorted(glob.glob(os.path.join(GOLDEN, name + ".part*.npz")))
    if not parts:
        raise FileNotFoundError(one)
    return meta, Parts(parts)


def shift_inputs(seed, D):
    """Inputs of the shift fixtures (make_golden_shift.py): g, b and a third vector (MARINA's g_prev)."""
    g = np.random.default_rng(seed)
    a = g.standard_normal(D).astype(np.float32)
    b = (a + 0.3 * g.standard_normal(D)).astype(np.float32)
    b[:5] = a[:5]                                     # exact zeros in the difference
    x3 = g.standard_normal(D).astype(np.float32)
    return a, b, x3


def shift_fingerprint(*xs):
    return [float(np.sum(x.astype(np.float64))) for x in xs]
