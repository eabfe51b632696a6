#!/usr/bin/env python3
"""Generate tests/golden/edges.{npz,json}: the REAL reference's compressVector on the edge rows of
tests/edge_rows.py (subnormals, every power of two with its neighbours, FLT_MAX, +-inf, NaN, norms
outside the fast-division window, elements on and next to every dithering level, draws on and next to
every probability).

Test infrastructure only, run in the development container where the reference is mounted read-only
(compressors.py imports only torch, math and numpy and is imported directly from
/root/reference/fl_pytorch/utils); the fixtures it writes are committed and travel instead.  CPU fp32
tensors throughout.  The pattern is forced by setting ``testp`` (compressors.py:204-212 only draw it);
for the levels rows the norm is forced too: ``torch.norm`` is replaced, for that one call, by a
function that returns the given norm (compressors.py:272 / 303 is the only use).

Stored per case: the output (fp32), the norm the reference used (fp32 bits; dithering), and the sha256
of the input row and of the uniform vector — not the inputs, which the tests regenerate from
tests/edge_rows.py and check against the digests.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference/fl_pytorch/utils")
import compressors  # noqa: E402  (the reference module, imported, never copied)

from tests import edge_rows as er  # noqa: E402
from tests import golden_io  # noqa: E402

SPECS = ["natural", "qsgd:8", "std.dithering:8:1", "std.dithering:5", "std.dithering:300:2", "terngrad",
         "nat.dithering:6:2", "bernulli:0.5", "ident"]
LAZY_DRAWS = {"keep": 0.25, "drop": 0.75}          # testp < P = 0.5 and not


def cases():
    """(key, spec, kind, lazy draw name or None) of every fixture case, in file order."""
    out = []
    for si, spec in enumerate(SPECS):
        kinds = er.KINDS + (list(er.LEVEL_KINDS) if er.dither_spec(spec) else [])
        for kind in kinds:
            for lz in (LAZY_DRAWS if spec.startswith("bernulli") else [None]):
                out.append((f"s{si}_{kind}" + (f"_{lz}" if lz else ""), spec, kind, lz))
    return out


def reference_output(spec, x, u, pnorm):
    c = compressors.initCompressor(spec, x.size)
    t = int(c.compressorType)
    if t == 2:
        c.testp = float(u)
    elif t in (4, 5, 6):
        c.testp = torch.from_numpy(u.copy())
    xt = torch.from_numpy(x.copy())
    used = None
    if t in (5, 6):
        if pnorm is None:
            used = torch.norm(xt, p=c.p)
            y = c.compressVector(xt)
        else:
            real = torch.norm
            used = torch.tensor(float(pnorm), dtype=torch.float32)
            torch.norm = lambda *a, **k: used
            try:
                y = c.compressVector(xt)
            finally:
                torch.norm = real
    else:
        y = c.compressVector(xt)
    return y.numpy().astype(np.float32).copy(), used


def main():
    arrays, meta = {}, {}
    for key, spec, kind, lz in cases():
        x = er.row(kind, spec)
        draws = spec.split(":")[0] not in ("ident", "bernulli")
        u = er.uniforms(kind, spec, x) if draws else (LAZY_DRAWS[lz] if lz else None)
        pn = er.given_norm(kind)
        y, used = reference_output(spec, x, u, pn)
        m = {"spec": spec, "kind": kind, "x_sha": er.sha(x), "given_norm": pn is not None}
        if draws:
            m["u_sha"] = er.sha(u)
        if lz:
            m["lazy_u"] = LAZY_DRAWS[lz]
        if used is not None:
            m["pnorm_bits"] = int(np.float32(used.item()).view(np.uint32))
        if spec == "ident":
            assert np.array_equal(y.view(np.uint32), x.view(np.uint32))    # the input itself: a digest is enough
            m["out_sha"] = er.sha(y)
        else:
            arrays[key] = y
        meta[key] = m
    n = golden_io.save("edges", arrays)
    with open(os.path.join(HERE, "edges.json"), "w") as f:
        json.dump({"torch": torch.__version__, "numpy": np.__version__, "cases": meta}, f, indent=1)
    print(f"{len(meta)} edge cases written in {n} file(s)")


if __name__ == "__main__":
    main()
