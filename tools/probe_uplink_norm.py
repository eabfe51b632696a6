#!/usr/bin/env python3
"""Price of the fused QSGD uplink's norm modes on ONE resident allocation (GPU box), built like
tools/ab_inproc.py: one process, one flc_rows_alloc allocation, the variants interleaved step by
step (the rows' placement moves a whole step by several % between allocations; inside one it is
matched).

Variants (C4's shard by default: 512 x 25 M, qsgd:127, device RNG):
  exact   norm_mode="exact": the filter's own partials (the parent's path)
  tn      norm_mode="torch_cpu", the product default: the filter emits the torch lanes' sums,
          k_tn_maps is the one extra read of the rows
  tn3     norm_mode="torch_cpu" as the three-read composition (k_tn_sums reads the rows once more):
          the library --three-read names, an A/B build with -DFLC_DS_TNSUMS=0
          (XFLAGS=-DFLC_DS_TNSUMS=0 tools/ab_build.sh tn3); left out when that build is missing
  given   pnorms_in = the exact run's pnorms_out

2 warm-ups and --steps timed steps per variant, every step timed on its own (events), kernel
times from the library's profile scopes.  One JSON line per variant: median, min, max and the
spread (max - min) of the steps, and the kernels' ms per step; then a "compare" line.  The torch-order
variants' output must be equal to each other bit for bit, and `given` to `exact`.

usage: python tools/probe_uplink_norm.py [--n 512] [--d 25000000] [--steps 10] [--three-read tn3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ["k_ds_filter", "k_tn_sums", "k_tn_item_prefix", "k_tn_maps", "k_tn_walk", "k_ds_resolve", "k_ds_accum"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--d", type=int, default=25_000_000)
    ap.add_argument("--spec", default="qsgd:127")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--three-read", default="tn3", help="abvar tag of the -DFLC_DS_TNSUMS=0 build")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    from flpytorch_amd import _lib
    from flpytorch_amd import aggregation as ag
    from flpytorch_amd.resident import resident_rows
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows, placement = resident_rows(a.n, a.d, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1000)
    for i in range(0, a.n, 64):
        rows[i:i + 64].normal_(generator=gen)
    out = torch.empty(a.d, dtype=torch.float32, device=dev)
    pn = torch.empty(a.n, dtype=torch.float32, device=dev)
    prod = _lib.open_variant("prod")
    libs = {"exact": prod, "tn": prod, "given": prod}
    order = ["exact", "tn", "given"]
    try:
        libs["tn3"] = _lib.open_variant(a.three_read)
        order.insert(2, "tn3")
    except ImportError as e:
        print(f"note: no three-read build ({e}); variant tn3 left out", file=sys.stderr)

    def reducer(mode):
        c = ag.initCompressor(a.spec, a.d)
        c.norm_mode = mode
        return ag.UplinkReducer(c, device=dev, seed=20241015)
    reds = {"exact": reducer("exact"), "tn": reducer("torch_cpu"), "tn3": reducer("torch_cpu"), "given": reducer("exact")}
    given = torch.empty_like(pn)

    def step(v):
        kw = {"pnorms_in": given} if v == "given" else {}
        with _lib.use(libs[v]):
            reds[v](rows, out=out, pnorms_out=pn, **kw)

    # warm-ups (workspaces, side streams), the bit checks between the variants
    bits = {}
    for w in range(a.warmup):
        for v in order:
            step(v)
            torch.cuda.synchronize()
            if v == "exact":
                given.copy_(pn)
            bits[v] = (out.clone().view(torch.int32), pn.clone().view(torch.int32)) if w == 0 else bits[v]
    assert torch.equal(bits["given"][0], bits["exact"][0]) and torch.equal(bits["given"][1], bits["exact"][1])
    if "tn3" in order:
        assert torch.equal(bits["tn3"][0], bits["tn"][0]) and torch.equal(bits["tn3"][1], bits["tn"][1])
    del bits
    ms = {v: [] for v in order}
    ks = {v: {k: 0.0 for k in KERNELS} for v in order}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.steps):
        for v in order:
            with _lib.use(libs[v]):
                _lib.profile_enable(True)
                for k in KERNELS:
                    _lib.profile_collect(k)
            e0.record()
            step(v)
            e1.record()
            e1.synchronize()
            ms[v].append(e0.elapsed_time(e1))
            with _lib.use(libs[v]):
                _lib.profile_enable(False)
                for k in KERNELS:
                    ks[v][k] += _lib.profile_collect(k)[0]
    lines = []
    for v in order:
        s = ms[v]
        lines.append({"variant": v, "n": a.n, "d": a.d, "spec": a.spec, "rows": placement, "steps": a.steps,
                      "median_ms": round(statistics.median(s), 4), "min_ms": round(min(s), 4), "max_ms": round(max(s), 4),
                      "spread_ms": round(max(s) - min(s), 4), "steps_ms": [round(x, 4) for x in s],
                      "kernels_ms_per_step": {k: round(t / a.steps, 4) for k, t in ks[v].items() if t},
                      "build": libs[v].flc_build_id().decode()})
    med = {v: statistics.median(ms[v]) for v in order}
    cmp_ = {"compare": "medians", "tn_minus_exact_ms": round(med["tn"] - med["exact"], 4),
            "given_minus_exact_ms": round(med["given"] - med["exact"], 4)}
    if "tn3" in order:
        cmp_["tn3_minus_tn_ms"] = round(med["tn3"] - med["tn"], 4)
        cmp_["spread_ms"] = round(max(max(ms[v]) - min(ms[v]) for v in ("tn", "tn3")), 4)
    lines.append(cmp_)
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
