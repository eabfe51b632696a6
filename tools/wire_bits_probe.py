#!/usr/bin/env python
"""Bit-packed wire formats against the byte formats, in one process on one allocation.

Server: flc_unpack_reduce_bits over N bit-packed messages against flc_unpack_reduce over the byte
messages of the same rows (device draws), the two interleaved: `--repeats` rounds of `--steps` calls
each, device events around each round, the two outputs compared as int32 after the warm-up and after
every repeat.  Client: flc_pack_bits against flc_pack of one row, measured the same way, the decoded
messages compared.  Byte models: the fold reads N payload bodies and writes 4 D; the pack reads x
twice (the norm pass; natural: once) and writes one body.

Writes <out-dir>/<spec>.jsonl (default profiles/r16/wire_bits): one record per repeat and variant,
then a summary with medians, ranges and the kernels' own times of one call.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 2024


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--specs", default="natural,terngrad,qsgd:7,qsgd:63")
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--d", type=int, default=25_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r16", "wire_bits"))
    a = ap.parse_args()
    import torch

    from flpytorch_amd import _lib
    from flpytorch_amd import aggregation as ag
    _lib.require_gpu()
    bid = _lib.check_provenance()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d = a.n, a.d
    os.makedirs(a.out_dir, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(1000)
    x = torch.empty(d, dtype=torch.float32, device=dev)
    outs = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in ("bits", "bytes")}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernels = ("k_unpack_bits_accum", "k_unpack_accum", "k_ew_code_bits", "k_norm_partials")

    def timed(fh, runs, agree, model, extra):
        def emit(rec):
            line = json.dumps(rec)
            fh.write(line + "\n")
            fh.flush()
            print(line, flush=True)
        for _ in range(2):                              # warm: code objects, workspaces
            for f in runs.values():
                f()
        torch.cuda.synchronize()
        if not agree():
            raise SystemExit(f"{extra}: the two forms differ after the warm-up")
        ms = {v: [] for v in runs}
        for r in range(a.repeats):
            for v, f in runs.items():
                e0.record()
                for _ in range(a.steps):
                    f()
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1) / a.steps
                ms[v].append(t)
                emit(dict(extra, repeat=r, variant=v, ms_per_call=round(t, 4), model_bytes=model[v],
                          GBps=round(model[v] / t / 1e6, 1)))
            if not agree():
                raise SystemExit(f"{extra}: the two forms differ after repeat {r}")
        kms = {}
        for v, f in runs.items():                       # the kernels' own times, one call each
            _lib.profile_enable(True)
            for kn in kernels:
                _lib.profile_collect(kn)
            f()
            torch.cuda.synchronize()
            _lib.profile_enable(False)
            kms[v] = {kn: [round(t, 4), c] for kn in kernels for t, c in [_lib.profile_collect(kn)] if c}
        med = {v: statistics.median(ms[v]) for v in runs}
        emit(dict(extra, summary=True, build=bid, repeats=a.repeats, steps=a.steps,
                  median_ms={v: round(med[v], 4) for v in runs}, min_ms={v: round(min(ms[v]), 4) for v in runs},
                  max_ms={v: round(max(ms[v]), 4) for v in runs}, model_bytes=model,
                  GBps_of_model_at_median={v: round(model[v] / med[v] / 1e6, 1) for v in runs},
                  bytes_over_bits=round(med["bytes"] / med["bits"], 3),
                  byte_model_bytes_over_bits=round(model["bytes"] / model["bits"], 3),
                  bits_faster_beyond_spread=max(ms["bits"]) < min(ms["bytes"]),
                  bits_slower_beyond_spread=min(ms["bits"]) > max(ms["bytes"]),
                  outputs_equal_every_repeat=True, kernel_ms_and_records_one_call=kms))

    for spec in a.specs.split(","):
        comp = ag.initCompressor(spec, d)
        nb = {"bits": comp.payloadBytes(d, bits=True), "bytes": comp.payloadBytes(d)}
        P = {v: torch.empty((n, nb[v]), dtype=torch.uint8, device=dev) for v in nb}
        for i in range(n):
            x.normal_(generator=gen)
            comp.device_rng = (SEED, i)
            comp.compressPayload(x, out=P["bits"][i], bits=True)
            comp.compressPayload(x, out=P["bytes"][i])
        reds = {"bits": ag.PayloadReducer(comp, device=dev, bits=True), "bytes": ag.PayloadReducer(comp, device=dev)}
        path = os.path.join(a.out_dir, spec.replace(":", "_") + ".jsonl")
        with open(path, "w") as fh:
            timed(fh, {v: (lambda v=v: reds[v](P[v], d, out=outs[v])) for v in nb},
                  lambda: torch.equal(outs["bits"].view(torch.int32), outs["bytes"].view(torch.int32)),
                  {v: n * (nb[v] - 16) + 4 * d for v in nb}, {"spec": spec, "side": "fold", "n": n, "d": d})
            # ---- client: one row ----------------------------------------------------------------
            reads = 4 * d if spec == "natural" else 8 * d
            one = {v: P[v][0] for v in nb}
            timed(fh, {v: (lambda v=v: comp.compressPayload(x, out=one[v], bits=(v == "bits"))) for v in nb},
                  lambda: torch.equal(comp.decompressPayload(one["bits"], d, bits=True).view(torch.int32),
                                      comp.decompressPayload(one["bytes"], d).view(torch.int32)),
                  {v: reads + nb[v] - 16 for v in nb}, {"spec": spec, "side": "pack", "d": d})
        print("wrote", path, flush=True)
        del P, reds, one


if __name__ == "__main__":
    main()
