#!/usr/bin/env python
"""Sparse level messages against the Q8 byte format, in one process on one allocation.

Server: flc_unpack_reduce_slev over N sparse level messages (a pointer array of used-length views
into one buffer) against flc_unpack_reduce over the Q8 messages of the same rows (device draws), the
two interleaved: `--repeats` rounds of `--steps` calls each, device events around each round, the two
outputs compared as canon(a) = bits(a + 0.0f) after the warm-up and after every repeat.  Client:
flc_pack_slev against flc_pack of one row, measured the same way (the sparse call includes its 4-byte
read-back of tab[C]), the decoded messages compared.  Byte models: the Q8 fold reads N bodies and
writes 4 D, the sparse fold reads the used bytes and writes 4 D; the Q8 pack reads x twice and writes
one body, the sparse pack reads x twice and moves about 6 bytes per listed element twice.

Writes <out-dir>/<spec>.jsonl (default profiles/r19/wire_slev): one record per repeat and variant,
then a summary with medians, ranges, the used bytes per message and the kernels' own times of one call.
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
    ap.add_argument("--specs", default="qsgd:127,terngrad")
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--d", type=int, default=25_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r19", "wire_slev"))
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
    outs = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in ("slev", "q8")}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernels = ("k_unpack_slev_accum", "k_unpack_accum", "k_slev_stage", "k_norm_partials")

    def canon_equal(p, q):
        return torch.equal((p + 0.0).view(torch.int32), (q + 0.0).view(torch.int32))

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
                  q8_over_slev=round(med["q8"] / med["slev"], 3),
                  byte_model_q8_over_slev=round(model["q8"] / model["slev"], 3),
                  slev_faster_beyond_spread=max(ms["slev"]) < min(ms["q8"]),
                  slev_slower_beyond_spread=min(ms["slev"]) > max(ms["q8"]),
                  outputs_agree_every_repeat=True, kernel_ms_and_records_one_call=kms))

    for spec in a.specs.split(","):
        comp = ag.initCompressor(spec, d)
        cap, nb = comp.payloadBytes(d, sparse_levels=True), comp.payloadBytes(d)
        q8 = torch.empty((n, nb), dtype=torch.uint8, device=dev)
        one = torch.empty(cap, dtype=torch.uint8, device=dev)        # one capacity buffer, reused by every pack
        msgs, used = [], []
        for i in range(n):
            x.normal_(generator=gen)
            comp.device_rng = (SEED, i)
            comp.compressPayload(x, out=q8[i])
            m = comp.compressPayload(x, out=one, sparse_levels=True)
            used.append(m.numel())
            msgs.append(m.clone())
        flat = torch.empty(sum(used), dtype=torch.uint8, device=dev)  # the N messages back to back (used sizes are 16 k)
        views, at = [], 0
        for m in msgs:
            flat[at:at + m.numel()] = m
            views.append(flat[at:at + m.numel()])
            at += m.numel()
        del msgs
        reds = {"slev": ag.PayloadReducer(comp, device=dev, sparse_levels=True), "q8": ag.PayloadReducer(comp, device=dev)}
        pay = {"slev": views, "q8": q8}
        stats = {"used_bytes_median": int(statistics.median(used)), "used_bytes_min": min(used), "used_bytes_max": max(used),
                 "q8_bytes": nb, "capacity_bytes": cap}
        path = os.path.join(a.out_dir, spec.replace(":", "_") + ".jsonl")
        with open(path, "w") as fh:
            timed(fh, {v: (lambda v=v: reds[v](pay[v], d, out=outs[v])) for v in pay},
                  lambda: canon_equal(outs["slev"], outs["q8"]),
                  {"slev": sum(used) + 4 * d, "q8": n * (nb - 16) + 4 * d},
                  dict(stats, spec=spec, side="fold", n=n, d=d))
            # ---- client: the last row ------------------------------------------------------------
            last = {}
            packs = {"slev": lambda: last.__setitem__("slev", comp.compressPayload(x, out=one, sparse_levels=True)),
                     "q8": lambda: last.__setitem__("q8", comp.compressPayload(x, out=q8[0]))}
            timed(fh, packs,
                  lambda: canon_equal(comp.decompressPayload(last["slev"], d, sparse_levels=True),
                                      comp.decompressPayload(last["q8"], d)),
                  {"slev": 8 * d + 2 * 6 * (used[-1] // 3), "q8": 8 * d + nb - 16}, dict(stats, spec=spec, side="pack", d=d))
        print("wrote", path, flush=True)
        del q8, flat, views, pay, reds


if __name__ == "__main__":
    main()
