#!/usr/bin/env python
"""The Rank-K fold from the factor payloads against the dense-row fold, in one process.

Server: flc_unpack_reduce_factored (k_rk_fold: one fp32 MFMA GEMM over the message bodies in place)
against flc_unpack_reduce (block gather, rocBLAS strided-batched GEMM into n dense rows, the row fold)
over the same N Rank-K messages, made once outside the clock (by default well-formed messages of drawn
factors — the fold's work does not depend on the values; `--svd` packs real rows).  The two are interleaved: `--repeats`
rounds of `--steps` calls each, device events around each round; after the warm-up and after every
repeat the relative difference ||factored - dense|| / ||dense|| of the two outputs is taken (they are
not the same bits: the factored fold weights the factor, the dense one the reconstructed row).
Byte and flop models: the factored fold reads 4 N K' (A + B) bytes of messages and writes 4 D, 2 D N K'
flops; the dense fold moves about 8 N D + 4 D bytes.

Writes <out-dir>/<spec>.jsonl (default profiles/r20/wire_rankk): one record per repeat and variant,
then a summary with medians, ranges, the workspace bytes of both and the kernel's own time of one call.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--spec", default="rank_k:10")
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--d", type=int, default=25_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--svd", action="store_true", help="pack real rows (one thin SVD each: minutes at the default shape)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r20", "wire_rankk"))
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
    comp = ag.initCompressor(a.spec, d)
    A, B, kp = comp.A, comp.B, min(comp.K, comp.A, comp.B)
    nb = comp.payloadBytes(d)
    gen = torch.Generator(device=dev).manual_seed(1000)
    pay = torch.zeros((n, nb), dtype=torch.uint8, device=dev)
    uoff = (B * kp + 3) & ~3
    if a.svd:                                           # the clients' own messages: one thin SVD per row
        for i in range(n):
            left = torch.randn((A, 2 * kp), generator=gen, device=dev)
            x = left @ torch.randn((2 * kp, B), generator=gen, device=dev)
            comp.compressPayload(x.reshape(-1), out=pay[i])
            del left, x
    else:                                               # well-formed messages of drawn factors (the fold's time
        for i in range(n):                              # does not depend on the values): header {6, K', 0, 0}
            pay[i, :16].view(torch.int32).copy_(torch.tensor([6, kp, 0, 0], dtype=torch.int32))
            body = pay[i, 16:].view(torch.float32)
            body[:B * kp].normal_(generator=gen).mul_(B ** -0.5)
            body[uoff:uoff + kp * A].normal_(generator=gen)
    comp.validatePayload(pay[0].cpu(), d)
    weights = [1.0 + (i % 7) / 8.0 for i in range(n)]
    reds = {"factored": ag.PayloadReducer(comp, device=dev, factored=True), "dense": ag.PayloadReducer(comp, device=dev)}
    outs = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in reds}
    runs = {v: (lambda v=v: reds[v](pay, d, out=outs[v], weights=weights)) for v in reds}
    lib = _lib.load()
    prm, _keep = comp.codec_params(dev)
    ws = {"factored": int(lib.flc_unpack_reduce_factored_workspace_size(ctypes.byref(prm), n, d)),
          "dense": int(lib.flc_unpack_reduce_workspace_size(ctypes.byref(prm), n, d))}
    model = {"factored": 4 * n * kp * (A + B) + 4 * d, "dense": 8 * n * d + 4 * d}
    flops = 2 * d * n * kp
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def rel_diff():
        return float((outs["factored"].double() - outs["dense"].double()).norm() / outs["dense"].double().norm())

    path = os.path.join(a.out_dir, a.spec.replace(":", "_") + ".jsonl")
    with open(path, "w") as fh:
        def emit(rec):
            line = json.dumps(rec)
            fh.write(line + "\n")
            fh.flush()
            print(line, flush=True)
        for _ in range(2):                              # warm: code objects, workspaces, rocBLAS's kernel choice
            for f in runs.values():
                f()
        torch.cuda.synchronize()
        diffs = [rel_diff()]
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
                emit(dict(spec=a.spec, n=n, d=d, repeat=r, variant=v, ms_per_call=round(t, 4), model_bytes=model[v],
                          GBps=round(model[v] / t / 1e6, 1), TFLOPs=round(flops / t / 1e9, 2) if v == "factored" else None))
            diffs.append(rel_diff())
            emit(dict(spec=a.spec, repeat=r, rel_diff_factored_vs_dense=diffs[-1]))
        _lib.profile_enable(True)                       # the kernel's own time, one call
        _lib.profile_collect("k_rk_fold")
        runs["factored"]()
        torch.cuda.synchronize()
        _lib.profile_enable(False)
        kt, kc = _lib.profile_collect("k_rk_fold")
        med = {v: statistics.median(ms[v]) for v in runs}
        emit(dict(spec=a.spec, n=n, d=d, A=A, B=B, K=kp, summary=True, build=bid, repeats=a.repeats, steps=a.steps,
                  median_ms={v: round(med[v], 4) for v in runs}, min_ms={v: round(min(ms[v]), 4) for v in runs},
                  max_ms={v: round(max(ms[v]), 4) for v in runs}, model_bytes=model, model_flops=flops,
                  workspace_bytes=ws, message_bytes=nb,
                  dense_over_factored=round(med["dense"] / med["factored"], 3),
                  factored_faster_beyond_spread=max(ms["factored"]) < min(ms["dense"]),
                  factored_slower_beyond_spread=min(ms["factored"]) > max(ms["dense"]),
                  TFLOPs_at_median=round(flops / med["factored"] / 1e9, 2),
                  max_rel_diff=max(diffs), k_rk_fold_ms_and_records_one_call=[round(kt, 4), kc]))
    print("wrote", path, flush=True)


if __name__ == "__main__":
    main()
