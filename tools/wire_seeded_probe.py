"""Seeded RandK messages against FMT_SPARSE, pack and fold, in one process on one allocation.

N = 128, D = 25 M, K = 1 % and 10 %, device draws.  The seeded call and the FMT_SPARSE call are
interleaved: 5 repeats of 2 calls each, the fold outputs compared as int32 after every repeat;
median [min-max] of the per-call times.  One JSON line per (K, leg) on stdout; --out DIR also writes
them to DIR/wire_seeded.jsonl (profiles/r18/wire_seeded/ is the place for a recorded run).

    python tools/wire_seeded_probe.py --out profiles/r18/wire_seeded
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flpytorch_amd import aggregation as ag  # noqa: E402


def timed(fn, calls):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for i in range(calls):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(calls)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--d", type=int, default=25_000_000)
    ap.add_argument("--ks", default="1%,10%")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    x = torch.randn(a.d, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    for k in a.ks.split(","):
        comps = [ag.initCompressor("randk:" + k, a.d) for _ in range(a.n)]
        for i, c in enumerate(comps):
            c.device_rng = (2024, i)
        sizes = {s: comps[0].payloadBytes(a.d, seeded=s) for s in (False, True)}
        bufs = {s: torch.zeros((a.n, sizes[s]), dtype=torch.uint8, device="cuda") for s in sizes}
        for s in sizes:
            for i, c in enumerate(comps):
                c.compressPayload(x.roll(i), out=bufs[s][i], seeded=s)
        red = {s: ag.PayloadReducer(comps[0], seeded=s) for s in sizes}
        outs = {s: torch.empty(a.d, device="cuda") for s in sizes}
        legs = {
            "pack": {s: (lambda s=s: comps[0].compressPayload(x, out=bufs[s][0], seeded=s)) for s in sizes},
            "fold": {s: (lambda s=s: red[s](bufs[s], d=a.d, out=outs[s])) for s in sizes},
        }
        for leg, fns in legs.items():
            for fn in fns.values():
                fn()                                       # warm-up: workspaces, code objects
            t = {s: [] for s in sizes}
            for _ in range(a.repeats):
                for s in (True, False):
                    t[s] += timed(fns[s], a.calls)
                if leg == "fold":
                    assert torch.equal(outs[True].view(torch.int32), outs[False].view(torch.int32)), "fold outputs differ"
            for s in sizes:
                lines.append({"k": k, "leg": leg, "format": "seeded" if s else "sparse", "bytes": sizes[s],
                              "ms_median": statistics.median(t[s]), "ms_min": min(t[s]), "ms_max": max(t[s]),
                              "n": a.n, "d": a.d, "repeats": a.repeats, "calls": a.calls})
                print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "wire_seeded.jsonl"), "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
