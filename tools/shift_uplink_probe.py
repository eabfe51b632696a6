#!/usr/bin/env python3
"""Price of a shifted round (DIANA in place) three ways, in ONE process on ONE allocation (GPU box).

Per codec, interleaved repeat by repeat (as tools/ab_inproc.py does: the rows' placement moves a
step by up to ~10 % between allocations, so the variants share one):

  fused        ShiftUplinkReducer(G, H, alpha, shift = shift_out = H)       flc_encode_shift_reduce
  composition  N x compressShift(G_i, H_i) into stored message rows, then reduce_rows over them — what
               the library offered before the fused call
  yardstick    UplinkReducer's dense fold of the same codec over the G rows alone: the read-only
               tile-owner pass (k_ew_accum_vec) the fused kernel is modelled on

fused and composition start from equal shifts and update their own copy, so after every repeat
their outputs and shifts must agree bit for bit (checked).  Algorithmic bytes: fused 12 N D + 4 D
(natural: read G and H, write H) or 20 N D + 4 D (dithering: the norm pass reads G and H once
more); composition 20 / 28 N D + 4 D (the message rows written and read back); yardstick 4 / 8 N D
+ 4 D.  A last pass with the library's kernel timers on gives the kernels' own times.

usage: python tools/shift_uplink_probe.py [--specs natural,qsgd:127] [--n 128] [--d 25000000]
           [--repeats 5] [--steps 2] [--out-dir profiles/r09/shift_uplink] [--fused-libs tagA,tagB]
--fused-libs: A/B builds of the library (abvar/libflcodec_<tag>.so, tools/ab_build.sh) whose fused
call is timed in the same rounds as "fused@<tag>" ON THE SAME shift matrix as "fused" (a matrix of
their own reads up to ~10 % differently: placement).  A timing-only mode: the shifts then take several
updates per repeat, so the bit check against the composition is off.
Writes <out-dir>/<spec>.jsonl: one line per (repeat, variant) and a summary line.

--sparse (RandK specs, e.g. --specs randk:1%,randk:10%): the same in-place DIANA round three ways,
  sparse     ShiftUplinkReducer(..., sparse=True)                           flc_randk_shift_reduce
  general    ShiftUplinkReducer(...) on its own copy of the shifts          flc_encode_shift_reduce
  yardstick  UplinkReducer's RandK fold of the G rows alone (for scale: one gather per member, no store)
interleaved in one process on one allocation; after every repeat the two outputs and the two shift
matrices must agree bit for bit (Gaussian shifts hold no -0).  The summary carries the 128-B line
floor of the sparse round: the expected number of lines a row's K members touch, (D / 32) *
(1 - (1 - K / D)^32), times 128 B, for a, for b and for the write-back, N rows.

--topk (TopK specs, e.g. --specs topk:1%): the in-place DIANA round and the in-place EF21 round, each
  batched    ShiftUplinkReducer(..., batched=True)                          flc_topk_shift_reduce
  general    ShiftUplinkReducer(...) on its own copy of the in-place operand flc_encode_shift_reduce
  yardstick  UplinkReducer's read-only TopK fold of the G rows alone (for scale)
interleaved in one process on one allocation; after every repeat the two outputs and the two in-place
matrices are compared as int32.  Byte model: batched 16 N D + 4 D (+ 4 N D for EF21's dense fold)
against ~48 N D for the general entry's row loop.  Writes <out-dir>/<spec>_<shape>.jsonl
(default out-dir with --topk: profiles/r11/topk_shift).

--one-read (QSGD specs, default qsgd:127): the in-place DIANA round and the in-place EF21 round, each
  one_read   ShiftUplinkReducer(..., one_read=True)                         flc_dither_shift_reduce
  general    ShiftUplinkReducer(...) on its own copy of the in-place operand flc_encode_shift_reduce
interleaved in one process on one allocation, device draws; after every repeat the two outputs and the
two in-place matrices are compared as int32.  Byte model: one_read 8 N D + 4 D (+ 4 N D for EF21's dense
fold) against 20 N D + 4 D; the summary carries the kernels' own times and the number of rows the
one-read call folded dense.  Writes <out-dir>/<spec>_<shape>.jsonl (default profiles/r12/dither_shift).

--wire (dense-format specs, default qsgd:127,natural; device draws): the shifted steps on the wire,
  client  fused        compressShiftPayload(g, h, alpha, shift = shift_out = h)   flc_pack_shift, DIANA in place
          composition  torch (g - h) + compressPayload + compressShift(message=False): the only bit-equal
                       way to the same payload and shift without flc_pack_shift
  server  fused        ShiftPayloadReducer(P, base = msg_out = M, scale = mult)    flc_unpack_shift_reduce,
                       the EF21 mirror in place over N payloads
          composition  N x decompressPayload + the two torch expressions (dec * mult, M_i + t) + reduce_rows
interleaved in one process on one allocation; after every repeat the payloads, the shifts, the mirrors
and the folds are compared (bytes / int32).  Byte models: client 21 d (QSGD; natural 14 d: no norm pass,
2-byte codes) against 41 d (30 d); server (c + 8) N d + 4 d against (c + 28) N d with c code bytes per
element.  Writes <out-dir>/<spec>_client.jsonl and <spec>_server.jsonl (default profiles/r13/shift_wire).

--frecon (elementwise specs, default qsgd:127,natural; device draws): the FRECON round with its server tail,
  one_call     FreconUplinkReducer(G, H, P, alpha, server=...)                flc_frecon_reduce
  composition  ShiftUplinkReducer twice (in-place DIANA over (G, H), the plain fold over (G, P)) and the
               server's expressions in torch (about seven D-sized ops)
each on its own copy of H and of h_prev, interleaved in one process on one allocation; after every repeat
the results, the H matrices and the two h_prev vectors are compared as int32.  Byte models (N D terms):
QSGD 28 N D against 36 N D, natural 16 N D against 20 N D.  Writes <out-dir>/<spec>.jsonl (default
profiles/r14/frecon).  --fused-libs adds "one_call@<tag>" legs as above (timing only, the bit check off).

--sampled (partial participation; default specs qsgd:127,natural,randk:1%,topk:1%; device draws): n = --n
participants of --n-total resident clients (default 512), their ids a seeded draw without replacement, the
state an [n_total, d] matrix.  The in-place DIANA round (qsgd, natural: the general entry; randk: sparse=True)
or the in-place EF21 round (topk: batched=True) three ways,
  sampled    ShiftUplinkReducer(G, S, ..., clients=ids)                     the _sampled entry
  gathered   S.index_select(0, ids), the contiguous entry on the copy, S.index_copy_(0, ids, copy): what a
             caller had to do before (16 n d more bytes)
  pregather  the contiguous entry on rows gathered once, outside the clock: what the indirection itself costs
each on its own state, interleaved in one process on one allocation.  After every repeat the participants'
rows and the outputs of gathered and pregather are compared as int32, and so are sampled's wherever the codec
draws nothing (TopK): with device draws the sampled call keys client ids[i] where the contiguous entry keys
position i, so their bits differ by design (tests/test_gpu_sampled_round.py pins the sampled bits).  Byte
models (n d terms): qsgd 20 against 36, natural 12 against 28.  Writes <out-dir>/<spec>.jsonl (default
profiles/r15/sampled).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20241015


def byte_model(spec, n, d):
    dither = not spec.startswith("natural")
    return {"fused": (20 if dither else 12) * n * d + 4 * d,
            "composition": (28 if dither else 20) * n * d + 4 * d,
            "yardstick": (8 if dither else 4) * n * d + 4 * d}


def main_sparse(a):
    import torch

    from flpytorch_amd import _lib
    from flpytorch_amd import aggregation as ag
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d = a.n, a.d
    os.makedirs(a.out_dir, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(1000)

    def filled():
        t = torch.empty((n, d), dtype=torch.float32, device=dev)
        for i in range(0, n, 64):
            t[i:i + 64].normal_(generator=gen)
        return t
    G, H0 = filled(), filled()
    Hs, Hg = torch.empty_like(H0), torch.empty_like(H0)
    outs = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in ("sparse", "general", "yardstick")}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for spec in a.specs.split(","):
        if not spec.startswith("randk"):
            raise SystemExit("--sparse times RandK specs only")
        comp_s, comp_g, comp_y = (ag.initCompressor(spec, d) for _ in range(3))
        k = comp_s.K
        alpha = 1.0 / (1.0 + comp_s.getW())
        red_s = ag.ShiftUplinkReducer(comp_s, device=dev, seed=SEED)
        red_g = ag.ShiftUplinkReducer(comp_g, device=dev, seed=SEED)
        yard = ag.UplinkReducer(comp_y, device=dev, seed=SEED)
        Hs.copy_(H0)
        Hg.copy_(H0)
        runs = {"sparse": lambda: red_s(G, Hs, alpha=alpha, shift=Hs, shift_out=Hs, out=outs["sparse"], sparse=True),
                "general": lambda: red_g(G, Hg, alpha=alpha, shift=Hg, shift_out=Hg, out=outs["general"]),
                "yardstick": lambda: yard(G, out=outs["yardstick"])}
        lines = (d / 32.0) * (1.0 - (1.0 - k / d) ** 32)
        model = {"sparse": int(3 * n * lines * 128) + 4 * d,          # the line floor: a, b, the write-back
                 "general": 44 * n * d,                               # sub 12, scatter 4 + memset-free dense e 4, epi 16, fold 12 (- first row)
                 "yardstick": int(n * lines * 128) + 4 * d}
        for f in runs.values():                        # warm: code objects, workspaces
            f()
        torch.cuda.synchronize()

        def agree():
            return (torch.equal(outs["sparse"].view(torch.int32), outs["general"].view(torch.int32))
                    and torch.equal(Hs.view(torch.int32), Hg.view(torch.int32)))
        if not agree():
            raise SystemExit(f"{spec}: the sparse and the general round differ after the warm-up round")
        ms = {v: [] for v in runs}
        path = os.path.join(a.out_dir, spec.replace(":", "_").replace(".", "_").replace("%", "pct") + ".jsonl")
        with open(path, "w") as fh:
            def emit(rec):
                line = json.dumps(rec)
                fh.write(line + "\n")
                fh.flush()
                print(line, flush=True)
            for r in range(a.repeats):
                for v, f in runs.items():
                    e0.record()
                    for _ in range(a.steps):
                        f()
                    e1.record()
                    e1.synchronize()
                    t = e0.elapsed_time(e1) / a.steps
                    ms[v].append(t)
                    emit({"spec": spec, "n": n, "d": d, "k": k, "repeat": r, "variant": v, "ms_per_call": round(t, 4)})
                if not agree():
                    raise SystemExit(f"{spec}: the sparse and the general round differ after repeat {r}")
            kernels = ("k_randk_shift", "k_randk_counts", "k_randk_fold", "k_randk_gen", "k_chunk_accum")
            kms = {}
            for v in ("sparse", "yardstick"):         # (the general round's kernels carry no timers)
                _lib.profile_enable(True)
                for kn in kernels:
                    _lib.profile_collect(kn)
                runs[v]()
                torch.cuda.synchronize()
                _lib.profile_enable(False)
                kms[v] = {kn: round(t, 4) for kn in kernels for t, c in [_lib.profile_collect(kn)] if c}
            if not agree():
                raise SystemExit(f"{spec}: the sparse and the general round differ after the timer pass")
            med = {v: statistics.median(ms[v]) for v in runs}
            emit({"spec": spec, "n": n, "d": d, "k": k, "summary": True, "repeats": a.repeats, "steps": a.steps,
                  "median_ms": {v: round(med[v], 4) for v in runs},
                  "min_ms": {v: round(min(ms[v]), 4) for v in runs},
                  "max_ms": {v: round(max(ms[v]), 4) for v in runs},
                  "general_over_sparse": round(med["general"] / med["sparse"], 3),
                  "sparse_over_yardstick": round(med["sparse"] / med["yardstick"], 3),
                  "sparse_faster_beyond_spread": max(ms["sparse"]) < min(ms["general"]),
                  "touched_lines_per_row": round(lines, 1), "lines_per_row": d / 32.0,
                  "line_floor_bytes": model["sparse"], "general_model_bytes": model["general"],
                  "line_floor_ratio": round(model["general"] / model["sparse"], 2),
                  "GBps_of_line_floor_at_median": round(model["sparse"] / med["sparse"] / 1e6, 1),
                  "bits_equal_every_repeat": True,
                  "kernel_ms_one_call": kms})
        print("wrote", path, flush=True)


def main_topk(a):
    import torch

    from flpytorch_amd import _lib
    from flpytorch_amd import aggregation as ag
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d = a.n, a.d
    os.makedirs(a.out_dir, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(1000)

    def filled():
        t = torch.empty((n, d), dtype=torch.float32, device=dev)
        for i in range(0, n, 64):
            t[i:i + 64].normal_(generator=gen)
        return t
    G, H0 = filled(), filled()
    Hb, Hg = torch.empty_like(H0), torch.empty_like(H0)
    variants = ("batched", "general", "yardstick")
    outs = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernels = ("k_shift_sub_rows", "k_topk_sample", "k_topk_filter", "k_cand_select", "k_topk_exact_rows",
               "k_topk_shift_lists", "k_chunk_accum", "k_reduce_vec", "k_lone_resident")
    for spec in a.specs.split(","):
        if not spec.startswith("topk"):
            raise SystemExit("--topk times TopK specs only")
        for shape in a.shapes.split(","):
            if shape not in ("diana", "ef21"):
                raise SystemExit("--shapes: diana, ef21")
            comp_b, comp_g, comp_y = (ag.initCompressor(spec, d) for _ in range(3))
            k = comp_b.K
            red_b = ag.ShiftUplinkReducer(comp_b, device=dev)
            red_g = ag.ShiftUplinkReducer(comp_g, device=dev)
            yard = ag.UplinkReducer(comp_y, device=dev)
            Hb.copy_(H0)
            Hg.copy_(H0)
            if shape == "diana":
                runs = {"batched": lambda: red_b(G, Hb, alpha=0.5, shift=Hb, shift_out=Hb, out=outs["batched"], batched=True),
                        "general": lambda: red_g(G, Hg, alpha=0.5, shift=Hg, shift_out=Hg, out=outs["general"])}
            else:
                runs = {"batched": lambda: red_b(G, Hb, base=Hb, msg_out=Hb, out=outs["batched"], batched=True),
                        "general": lambda: red_g(G, Hg, base=Hg, msg_out=Hg, out=outs["general"])}
            runs["yardstick"] = lambda: yard(G, out=outs["yardstick"])
            model = {"batched": (16 if shape == "diana" else 20) * n * d + 4 * d,
                     "general": 48 * n * d,                # sub 12, select 8, epilogue 16, fold step 12
                     "yardstick": 4 * n * d + 4 * d}
            for f in runs.values():                        # warm: code objects, workspaces
                f()
            torch.cuda.synchronize()

            def agree():
                return (torch.equal(outs["batched"].view(torch.int32), outs["general"].view(torch.int32))
                        and torch.equal(Hb.view(torch.int32), Hg.view(torch.int32)))
            if not agree():
                raise SystemExit(f"{spec} {shape}: the batched and the general round differ after the warm-up round")
            ms = {v: [] for v in runs}
            tag = spec.replace(":", "_").replace(".", "_").replace("%", "pct") + "_" + shape
            path = os.path.join(a.out_dir, tag + ".jsonl")
            with open(path, "w") as fh:
                def emit(rec):
                    line = json.dumps(rec)
                    fh.write(line + "\n")
                    fh.flush()
                    print(line, flush=True)
                for r in range(a.repeats):
                    for v, f in runs.items():
                        e0.record()
                        for _ in range(a.steps):
                            f()
                        e1.record()
                        e1.synchronize()
                        t = e0.elapsed_time(e1) / a.steps
                        ms[v].append(t)
                        emit({"spec": spec, "shape": shape, "n": n, "d": d, "k": k, "repeat": r, "variant": v,
                              "ms_per_call": round(t, 4), "model_bytes": model[v], "GBps": round(model[v] / t / 1e6, 1)})
                    if not agree():
                        raise SystemExit(f"{spec} {shape}: the batched and the general round differ after repeat {r}")
                kms = {}
                for v in variants:                         # the kernels' own times, one call each, outside the timed repeats
                    _lib.profile_enable(True)
                    for kn in kernels:
                        _lib.profile_collect(kn)
                    runs[v]()
                    torch.cuda.synchronize()
                    _lib.profile_enable(False)
                    kms[v] = {kn: [round(t, 4), c] for kn in kernels for t, c in [_lib.profile_collect(kn)] if c}
                if not agree():
                    raise SystemExit(f"{spec} {shape}: the batched and the general round differ after the timer pass")
                flags = ag.select_row_flags(comp_b, n, d)
                med = {v: statistics.median(ms[v]) for v in runs}
                emit({"spec": spec, "shape": shape, "n": n, "d": d, "k": k, "summary": True, "repeats": a.repeats,
                      "steps": a.steps,
                      "median_ms": {v: round(med[v], 4) for v in runs},
                      "min_ms": {v: round(min(ms[v]), 4) for v in runs},
                      "max_ms": {v: round(max(ms[v]), 4) for v in runs},
                      "model_bytes": model,
                      "GBps_of_model_at_median": {v: round(model[v] / med[v] / 1e6, 1) for v in runs},
                      "general_over_batched": round(med["general"] / med["batched"], 3),
                      "byte_model_general_over_batched": round(model["general"] / model["batched"], 3),
                      "batched_over_yardstick": round(med["batched"] / med["yardstick"], 3),
                      "batched_faster_beyond_spread": max(ms["batched"]) < min(ms["general"]),
                      "bits_equal_every_repeat": True,
                      "rows_on_exact_path_last_batched_call": int(((flags & 8) != 0).sum()),
                      "kernel_ms_and_records_one_call": kms})
            print("wrote", path, flush=True)


def main_one_read(a):
    import ctypes

    import torch

    from flpytorch_amd import _lib
    from flpytorch_amd import aggregation as ag
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d = a.n, a.d
    os.makedirs(a.out_dir, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(1000)

    def filled():
        t = torch.empty((n, d), dtype=torch.float32, device=dev)
        for i in range(0, n, 64):
            t[i:i + 64].normal_(generator=gen)
        return t
    G, H0 = filled(), filled()
    Ho, Hg = torch.empty_like(H0), torch.empty_like(H0)
    variants = ("one_read", "general")
    outs = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernels = ("k_ds_sample", "k_ds_filter", "k_ds_final", "k_ds_resolve", "k_ds_accum", "k_ds_shift_lists",
               "k_ds_shift_dense_rows", "k_reduce_vec", "k_norm_partials", "k_ew_shift_accum")
    for spec in a.specs.split(","):
        if not spec.startswith("qsgd"):
            raise SystemExit("--one-read times QSGD specs only")
        for shape in a.shapes.split(","):
            if shape not in ("diana", "ef21"):
                raise SystemExit("--shapes: diana, ef21")
            comp_o, comp_g = (ag.initCompressor(spec, d) for _ in range(2))
            mult = 1.0 if comp_o.isContractionCompressor() else 1.0 / (1.0 + comp_o.getW())
            red_o = ag.ShiftUplinkReducer(comp_o, device=dev, seed=SEED)
            red_g = ag.ShiftUplinkReducer(comp_g, device=dev, seed=SEED)
            Ho.copy_(H0)
            Hg.copy_(H0)
            if shape == "diana":
                runs = {"one_read": lambda: red_o(G, Ho, alpha=0.5, shift=Ho, shift_out=Ho, out=outs["one_read"], one_read=True),
                        "general": lambda: red_g(G, Hg, alpha=0.5, shift=Hg, shift_out=Hg, out=outs["general"])}
            else:
                runs = {"one_read": lambda: red_o(G, Ho, scale=mult, base=Ho, msg_out=Ho, out=outs["one_read"], one_read=True),
                        "general": lambda: red_g(G, Hg, scale=mult, base=Hg, msg_out=Hg, out=outs["general"])}
            # algorithmic bytes: a and b once (+ EF21's dense fold of the updated rows) against two reads and a full store
            model = {"one_read": (8 if shape == "diana" else 12) * n * d + 4 * d, "general": 20 * n * d + 4 * d}
            for f in runs.values():                        # warm: code objects, workspaces
                f()
            torch.cuda.synchronize()

            def agree():
                return (torch.equal(outs["one_read"].view(torch.int32), outs["general"].view(torch.int32))
                        and torch.equal(Ho.view(torch.int32), Hg.view(torch.int32)))
            if not agree():
                raise SystemExit(f"{spec} {shape}: the one-read and the general round differ after the warm-up round")
            ms = {v: [] for v in runs}
            tag = spec.replace(":", "_").replace(".", "_") + "_" + shape
            path = os.path.join(a.out_dir, tag + ".jsonl")
            with open(path, "w") as fh:
                def emit(rec):
                    line = json.dumps(rec)
                    fh.write(line + "\n")
                    fh.flush()
                    print(line, flush=True)
                for r in range(a.repeats):
                    for v, f in runs.items():
                        e0.record()
                        for _ in range(a.steps):
                            f()
                        e1.record()
                        e1.synchronize()
                        t = e0.elapsed_time(e1) / a.steps
                        ms[v].append(t)
                        emit({"spec": spec, "shape": shape, "n": n, "d": d, "repeat": r, "variant": v,
                              "ms_per_call": round(t, 4), "model_bytes": model[v], "GBps": round(model[v] / t / 1e6, 1)})
                    if not agree():
                        raise SystemExit(f"{spec} {shape}: the one-read and the general round differ after repeat {r}")
                kms = {}
                for v in variants:                         # the kernels' own times, one call each, outside the timed repeats
                    _lib.profile_enable(True)
                    for kn in kernels:
                        _lib.profile_collect(kn)
                    runs[v]()
                    torch.cuda.synchronize()
                    _lib.profile_enable(False)
                    kms[v] = {kn: [round(t, 4), c] for kn in kernels for t, c in [_lib.profile_collect(kn)] if c}
                # the rows a one-read call folds dense: read from the stream's workspace before the next call reuses it
                runs["one_read"]()
                ws = _lib.WORKSPACE.get(dev, 0)
                fl = torch.zeros(n, dtype=torch.int32, device=dev)
                _lib.check(_lib.load().flc_dither_row_flags(n, d, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                                            ctypes.c_void_p(fl.data_ptr()), _lib.stream_ptr(dev)),
                           "flc_dither_row_flags")
                runs["general"]()                          # (keeps the two operands in step)
                torch.cuda.synchronize()
                if not agree():
                    raise SystemExit(f"{spec} {shape}: the one-read and the general round differ after the timer pass")
                med = {v: statistics.median(ms[v]) for v in runs}
                emit({"spec": spec, "shape": shape, "n": n, "d": d, "summary": True, "repeats": a.repeats, "steps": a.steps,
                      "median_ms": {v: round(med[v], 4) for v in runs},
                      "min_ms": {v: round(min(ms[v]), 4) for v in runs},
                      "max_ms": {v: round(max(ms[v]), 4) for v in runs},
                      "model_bytes": model,
                      "GBps_of_model_at_median": {v: round(model[v] / med[v] / 1e6, 1) for v in runs},
                      "general_over_one_read": round(med["general"] / med["one_read"], 3),
                      "byte_model_general_over_one_read": round(model["general"] / model["one_read"], 3),
                      "line_granularity_model_general_over_one_read": 1.9 if shape == "diana" else None,
                      "one_read_median_below_general_min": med["one_read"] < min(ms["general"]),
                      "bits_equal_every_repeat": True,
                      "dense_flagged_rows": int(((fl & 1) != 0).sum()),
                      "kernel_ms_and_records_one_call": kms})
            print("wrote", path, flush=True)


def main_wire(a):
    import torch

    from flpytorch_amd import _lib
    from flpytorch_amd import aggregation as ag
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d = a.n, a.d
    os.makedirs(a.out_dir, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(1000)

    def filled():
        t = torch.empty((n, d), dtype=torch.float32, device=dev)
        for i in range(0, n, 64):
            t[i:i + 64].normal_(generator=gen)
        return t
    G, M0 = filled(), filled()
    Mf, Mc = torch.empty_like(M0), torch.empty_like(M0)
    diff, tmp = torch.empty(d, dtype=torch.float32, device=dev), torch.empty(d, dtype=torch.float32, device=dev)
    outs = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in ("fused", "composition")}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernels = ("k_ew_shift_code", "k_unpack_shift_accum", "k_norm_partials", "k_ew_shift", "k_reduce_vec")

    def timed(runs, agree, what, path, model, extra):
        for _ in range(2):                             # warm: code objects, workspaces, the allocator's blocks
            for f in runs.values():
                f()
        torch.cuda.synchronize()
        if not agree():
            raise SystemExit(f"{what}: fused and composition differ after the warm-up rounds")
        ms = {v: [] for v in runs}
        with open(path, "w") as fh:
            def emit(rec):
                line = json.dumps(rec)
                fh.write(line + "\n")
                fh.flush()
                print(line, flush=True)
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
                    raise SystemExit(f"{what}: fused and composition differ after repeat {r}")
            kms = {}
            for v, f in runs.items():                  # the kernels' own times, one call each
                _lib.profile_enable(True)
                for kn in kernels:
                    _lib.profile_collect(kn)
                f()
                torch.cuda.synchronize()
                _lib.profile_enable(False)
                kms[v] = {kn: [round(t, 4), c] for kn in kernels for t, c in [_lib.profile_collect(kn)] if c}
            if not agree():
                raise SystemExit(f"{what}: fused and composition differ after the timer pass")
            med = {v: statistics.median(ms[v]) for v in runs}
            emit(dict(extra, summary=True, repeats=a.repeats, steps=a.steps,
                      median_ms={v: round(med[v], 4) for v in runs}, min_ms={v: round(min(ms[v]), 4) for v in runs},
                      max_ms={v: round(max(ms[v]), 4) for v in runs}, model_bytes=model,
                      GBps_of_model_at_median={v: round(model[v] / med[v] / 1e6, 1) for v in runs},
                      composition_over_fused=round(med["composition"] / med["fused"], 3),
                      byte_model_composition_over_fused=round(model["composition"] / model["fused"], 3),
                      fused_faster_beyond_spread=max(ms["fused"]) < min(ms["composition"]),
                      bits_equal_every_repeat=True, kernel_ms_and_records_one_call=kms))
        print("wrote", path, flush=True)

    for spec in a.specs.split(","):
        tag = spec.replace(":", "_").replace(".", "_")
        comp_f, comp_c, comp_p = (ag.initCompressor(spec, d) for _ in range(3))
        for c in (comp_f, comp_c, comp_p):
            c.device_rng = (SEED, 0)
        pb = comp_f.payloadBytes(d)
        code = (pb - 16) / d                           # code bytes per element
        norm = 8 if not spec.startswith("natural") else 0      # the norm pass reads a and b once more
        alpha = 1.0 / (1.0 + comp_f.getW())
        mult = 1.0 if comp_f.isContractionCompressor() else 1.0 / (1.0 + comp_f.getW())
        # ---- client: one row, DIANA in place --------------------------------------------------
        g, hf, hc = G[0], Mf[0], Mc[0]
        hf.copy_(M0[0])
        hc.copy_(M0[0])
        pf = torch.empty(pb, dtype=torch.uint8, device=dev)
        pc = torch.empty(pb, dtype=torch.uint8, device=dev)

        def client_fused():
            comp_f.compressShiftPayload(g, hf, alpha=alpha, shift=hf, shift_out=hf, payload_out=pf)

        def client_composition():
            torch.sub(g, hc, out=diff)
            comp_c.compressPayload(diff, out=pc)
            comp_c.compressShift(g, hc, alpha=alpha, shift=hc, shift_out=hc, message=False)
        timed({"fused": client_fused, "composition": client_composition},
              lambda: torch.equal(pf, pc) and torch.equal(hf.view(torch.int32), hc.view(torch.int32)),
              f"{spec} client", os.path.join(a.out_dir, tag + "_client.jsonl"),
              {"fused": int((norm + 8 + 4 + code) * d),
               "composition": int((12 + norm // 2 + 4 + code + norm + 8 + 4) * d)},   # (the payload leg's norm pass reads the stored difference)
              {"spec": spec, "side": "client", "d": d})
        # ---- server: the EF21 mirror in place over n payloads ---------------------------------
        P = torch.empty((n, pb), dtype=torch.uint8, device=dev)
        for i in range(n):
            comp_p.device_rng = (SEED, i)
            comp_p.compressShiftPayload(G[i], M0[i], payload_out=P[i])
        Mf.copy_(M0)
        Mc.copy_(M0)
        red = ag.ShiftPayloadReducer(comp_f, device=dev)

        def server_fused():
            red(P, d, scale=mult, base=Mf, msg_out=Mf, out=outs["fused"])

        def server_composition():
            for i in range(n):
                dec = comp_c.decompressPayload(P[i], d)
                torch.mul(dec, mult, out=tmp)
                torch.add(Mc[i], tmp, out=Mc[i])
            ag.reduce_rows(outs["composition"], Mc, relative=False, out=outs["composition"])
        timed({"fused": server_fused, "composition": server_composition},
              lambda: (torch.equal(outs["fused"].view(torch.int32), outs["composition"].view(torch.int32))
                       and torch.equal(Mf.view(torch.int32), Mc.view(torch.int32))),
              f"{spec} server", os.path.join(a.out_dir, tag + "_server.jsonl"),
              {"fused": int((code + 8) * n * d + 4 * d), "composition": int((code + 28) * n * d + 4 * d)},
              {"spec": spec, "side": "server", "n": n, "d": d})
        del P


def main_frecon(a):
    import torch

    from flpytorch_amd import _lib
    from flpytorch_amd import aggregation as ag
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d = a.n, a.d
    os.makedirs(a.out_dir, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(1000)

    def filled(rows=n):
        t = torch.empty((rows, d), dtype=torch.float32, device=dev)
        for i in range(0, rows, 64):
            t[i:i + 64].normal_(generator=gen)
        return t
    G, H0, P = filled(), filled(), filled()
    Hf, Hc = torch.empty_like(H0), torch.empty_like(H0)
    gsp, hp0 = filled(1)[0], filled(1)[0]
    variants = ("one_call", "composition")
    res = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in variants}
    hp = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in variants}
    cu, cq = (torch.empty(d, dtype=torch.float32, device=dev) for _ in range(2))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernels = ("k_ew_frecon_accum", "k_norm_partials2", "k_ew_shift_accum", "k_norm_partials")
    lam, alpha_update = 0.5, 0.25
    extra = {t: _lib.open_variant(t) for t in a.fused_libs.split(",") if t}
    for spec in a.specs.split(","):
        comp_f, comp_c = (ag.initCompressor(spec, d) for _ in range(2))
        alpha = 1.0 / (1.0 + comp_f.getW())
        red_f = ag.FreconUplinkReducer(comp_f, device=dev, seed=SEED)
        red_c = ag.ShiftUplinkReducer(comp_c, device=dev, seed=SEED)
        Hf.copy_(H0)
        Hc.copy_(H0)
        for v in variants:
            hp[v].copy_(hp0)

        def run_one_call():
            red_f(G, Hf, P, alpha, server={"lambda_": lam, "g_server_prev": gsp, "h_prev": hp["one_call"],
                                           "alpha_update": alpha_update, "h_prev_out": hp["one_call"],
                                           "out": res["one_call"]})

        def run_composition():
            # what the library offered before: two fused rounds, then the server's expressions in torch
            red_c(G, Hc, alpha=alpha, shift=Hc, shift_out=Hc, out=cu)
            red_c(G, P, out=cq)
            h = hp["composition"]
            torch.add(cq + (1.0 - lam) * gsp, lam * (cu + h), out=res["composition"])
            torch.add(h, alpha_update * cu, out=h)
        runs = {"one_call": run_one_call, "composition": run_composition}

        def run_variant(lib):
            def f():
                with _lib.use(lib):
                    run_one_call()
            return f
        for t, lib in extra.items():               # (timing only: they advance one_call's H and h_prev as well)
            runs["one_call@" + t] = run_variant(lib)
        dither = not spec.startswith("natural")
        # algorithmic bytes (issue's models): the N D terms plus the [D] vectors of the tail
        model = {"one_call": (28 if dither else 16) * n * d, "composition": (36 if dither else 20) * n * d}
        for t in extra:
            model["one_call@" + t] = model["one_call"]
        for f in runs.values():                        # warm: code objects, workspaces, the allocator's blocks
            f()
        torch.cuda.synchronize()

        def agree():
            return bool(extra) or (torch.equal(res["one_call"].view(torch.int32), res["composition"].view(torch.int32))
                    and torch.equal(hp["one_call"].view(torch.int32), hp["composition"].view(torch.int32))
                    and torch.equal(Hf.view(torch.int32), Hc.view(torch.int32)))
        if not agree():
            raise SystemExit(f"{spec}: the one-call round and the composition differ after the warm-up round")
        ms = {v: [] for v in runs}
        path = os.path.join(a.out_dir, spec.replace(":", "_").replace(".", "_") + ".jsonl")
        with open(path, "w") as fh:
            def emit(rec):
                line = json.dumps(rec)
                fh.write(line + "\n")
                fh.flush()
                print(line, flush=True)
            for r in range(a.repeats):
                for v, f in runs.items():
                    e0.record()
                    for _ in range(a.steps):
                        f()
                    e1.record()
                    e1.synchronize()
                    t = e0.elapsed_time(e1) / a.steps
                    ms[v].append(t)
                    emit({"spec": spec, "n": n, "d": d, "repeat": r, "variant": v, "ms_per_call": round(t, 4),
                          "model_bytes": model[v], "GBps": round(model[v] / t / 1e6, 1)})
                if not agree():
                    raise SystemExit(f"{spec}: the one-call round and the composition differ after repeat {r}")
            kms = {}
            for v, f in runs.items():                  # the kernels' own times, one call each, outside the timed repeats
                _lib.profile_enable(True)
                for kn in kernels:
                    _lib.profile_collect(kn)
                f()
                torch.cuda.synchronize()
                _lib.profile_enable(False)
                kms[v] = {kn: [round(t, 4), c] for kn in kernels for t, c in [_lib.profile_collect(kn)] if c}
            if not agree():
                raise SystemExit(f"{spec}: the one-call round and the composition differ after the timer pass")
            med = {v: statistics.median(ms[v]) for v in runs}
            emit({"spec": spec, "n": n, "d": d, "summary": True, "repeats": a.repeats, "steps": a.steps,
                  "median_ms": {v: round(med[v], 4) for v in runs},
                  "min_ms": {v: round(min(ms[v]), 4) for v in runs},
                  "max_ms": {v: round(max(ms[v]), 4) for v in runs},
                  "model_bytes": model,
                  "GBps_of_model_at_median": {v: round(model[v] / med[v] / 1e6, 1) for v in runs},
                  "composition_over_one_call": round(med["composition"] / med["one_call"], 3),
                  "byte_model_composition_over_one_call": round(model["composition"] / model["one_call"], 3),
                  "one_call_faster_beyond_spread": max(ms["one_call"]) < min(ms["composition"]),
                  "bits_equal_every_repeat": not extra,
                  "kernel_ms_and_records_one_call": kms})
        print("wrote", path, flush=True)


def main_sampled(a):
    import numpy as np
    import torch

    from flpytorch_amd import _lib
    from flpytorch_amd import aggregation as ag
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d, nt = a.n, a.d, a.n_total
    if n > nt:
        raise SystemExit("--sampled: --n participants of --n-total clients")
    os.makedirs(a.out_dir, exist_ok=True)
    gen = torch.Generator(device=dev)

    def fill(t, seed):
        gen.manual_seed(seed)
        for i in range(0, t.shape[0], 64):
            t[i:i + 64].normal_(generator=gen)
        return t
    ids = [int(c) for c in np.random.RandomState(SEED % (1 << 31)).choice(nt, n, replace=False)]
    ids_t = torch.tensor(ids, dtype=torch.int64, device=dev)
    G = fill(torch.empty((n, d), dtype=torch.float32, device=dev), 1000)
    Sa, Sb = (torch.empty((nt, d), dtype=torch.float32, device=dev) for _ in range(2))   # (no third copy: refilled per spec)
    T, Hc = torch.empty_like(G), torch.empty_like(G)
    outs = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in ("sampled", "gathered", "pregather")}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for spec in a.specs.split(","):
        comps = [ag.initCompressor(spec, d) for _ in range(3)]
        reds = [ag.ShiftUplinkReducer(c, device=dev, seed=SEED) for c in comps]
        fast = {"sparse": True} if spec.startswith("randk") else {"batched": True} if spec.startswith("topk") else {}
        ef21 = spec.startswith("topk")
        alpha = None if ef21 else 1.0 / (1.0 + comps[0].getW())

        def round_on(red, H, out, **kw):
            if ef21:
                red(G, H, base=H, msg_out=H, out=out, **fast, **kw)
            else:
                red(G, H, alpha=alpha, shift=H, shift_out=H, out=out, **fast, **kw)
        Sb.copy_(fill(Sa, 1001))
        torch.index_select(Sa, 0, ids_t, out=Hc)

        def run_sampled():
            round_on(reds[0], Sa, outs["sampled"], clients=ids)

        def run_gathered():
            torch.index_select(Sb, 0, ids_t, out=T)
            round_on(reds[1], T, outs["gathered"])
            Sb.index_copy_(0, ids_t, T)

        def run_pregather():
            round_on(reds[2], Hc, outs["pregather"])
        runs = {"sampled": run_sampled, "gathered": run_gathered, "pregather": run_pregather}
        dither = not (spec.startswith("natural") or fast)
        model = None
        if not fast:
            per = 20 if dither else 12
            model = {"sampled": per * n * d + 4 * d, "gathered": (per + 16) * n * d + 4 * d, "pregather": per * n * d + 4 * d}
        for f in runs.values():                        # warm: code objects, workspaces
            f()
        torch.cuda.synchronize()

        def same_rows(X, Y_rows):
            return all(torch.equal(X[c].view(torch.int32), Y_rows[i].view(torch.int32)) for i, c in enumerate(ids))

        def agree():
            ok = torch.equal(outs["gathered"].view(torch.int32), outs["pregather"].view(torch.int32)) and same_rows(Sb, Hc)
            if ok and ef21:                            # no draws: the sampled call's bits are the contiguous entry's
                ok = torch.equal(outs["sampled"].view(torch.int32), outs["pregather"].view(torch.int32)) and same_rows(Sa, Hc)
            return ok
        if not agree():
            raise SystemExit(f"{spec}: the legs differ after the warm-up round")
        ms = {v: [] for v in runs}
        path = os.path.join(a.out_dir, spec.replace(":", "_").replace(".", "_").replace("%", "pct") + ".jsonl")
        with open(path, "w") as fh:
            def emit(rec):
                line = json.dumps(rec)
                fh.write(line + "\n")
                fh.flush()
                print(line, flush=True)
            for r in range(a.repeats):
                for v, f in runs.items():
                    e0.record()
                    for _ in range(a.steps):
                        f()
                    e1.record()
                    e1.synchronize()
                    t = e0.elapsed_time(e1) / a.steps
                    ms[v].append(t)
                    emit({"spec": spec, "n": n, "n_total": nt, "d": d, "repeat": r, "variant": v, "ms_per_call": round(t, 4)})
                if not agree():
                    raise SystemExit(f"{spec}: the legs differ after repeat {r}")
            kernels = ("k_ew_shift_accum", "k_norm_partials", "k_randk_shift", "k_randk_counts", "k_shift_sub_rows",
                       "k_topk_shift_lists", "k_topk_filter", "k_chunk_accum", "k_reduce_vec")
            kms = {}
            for v in ("sampled", "pregather"):
                _lib.profile_enable(True)
                for kn in kernels:
                    _lib.profile_collect(kn)
                runs[v]()
                torch.cuda.synchronize()
                _lib.profile_enable(False)
                kms[v] = {kn: round(t, 4) for kn in kernels for t, c in [_lib.profile_collect(kn)] if c}
            med = {v: statistics.median(ms[v]) for v in runs}
            rec = {"spec": spec, "n": n, "n_total": nt, "d": d, "summary": True, "repeats": a.repeats, "steps": a.steps,
                   "round": ("ef21 in place" if ef21 else "diana in place") + (", " + next(iter(fast)) if fast else ""),
                   "median_ms": {v: round(med[v], 4) for v in runs},
                   "min_ms": {v: round(min(ms[v]), 4) for v in runs},
                   "max_ms": {v: round(max(ms[v]), 4) for v in runs},
                   "gathered_over_sampled": round(med["gathered"] / med["sampled"], 3),
                   "sampled_over_pregather": round(med["sampled"] / med["pregather"], 3),
                   "sampled_faster_than_gathered_beyond_spread": max(ms["sampled"]) < min(ms["gathered"]),
                   "sampled_slower_than_pregather_beyond_spread": min(ms["sampled"]) > max(ms["pregather"]),
                   "bits_compared": "gathered = pregather" + (" = sampled" if ef21 else " (sampled draws by client id)"),
                   "kernel_ms_one_call": kms}
            if model:
                rec["algorithmic_bytes"] = model
                rec["GBps_at_median"] = {v: round(model[v] / med[v] / 1e6, 1) for v in runs}
                rec["byte_model_gathered_over_sampled"] = round(model["gathered"] / model["sampled"], 3)
            emit(rec)
        print("wrote", path, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--specs", default="natural,qsgd:127")
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--d", type=int, default=25_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r09", "shift_uplink"))
    ap.add_argument("--fused-libs", default="")
    ap.add_argument("--sparse", action="store_true", help="RandK specs: flc_randk_shift_reduce against the general entry")
    ap.add_argument("--topk", action="store_true", help="TopK specs: flc_topk_shift_reduce against the general entry")
    ap.add_argument("--one-read", action="store_true", help="QSGD specs: flc_dither_shift_reduce against the general entry")
    ap.add_argument("--wire", action="store_true", help="flc_pack_shift / flc_unpack_shift_reduce against their compositions")
    ap.add_argument("--frecon", action="store_true", help="flc_frecon_reduce against two fused rounds plus the tail in torch")
    ap.add_argument("--shapes", default="diana,ef21", help="--topk / --one-read: the in-place rounds to time")
    ap.add_argument("--sampled", action="store_true", help="the _sampled entries against gather + contiguous entry + scatter")
    ap.add_argument("--n-total", type=int, default=512, help="--sampled: resident clients (rows of the state matrix)")
    a = ap.parse_args()
    if a.sampled and a.out_dir == ap.get_default("out_dir"):
        a.out_dir = os.path.join(ROOT, "profiles", "r15", "sampled")
    if a.sampled and a.specs == ap.get_default("specs"):
        a.specs = "qsgd:127,natural,randk:1%,topk:1%"
    if a.topk and a.out_dir == ap.get_default("out_dir"):
        a.out_dir = os.path.join(ROOT, "profiles", "r11", "topk_shift")
    if a.one_read and a.out_dir == ap.get_default("out_dir"):
        a.out_dir = os.path.join(ROOT, "profiles", "r12", "dither_shift")
    if a.one_read and a.specs == ap.get_default("specs"):
        a.specs = "qsgd:127"
    if a.wire and a.out_dir == ap.get_default("out_dir"):
        a.out_dir = os.path.join(ROOT, "profiles", "r13", "shift_wire")
    if a.wire and a.specs == ap.get_default("specs"):
        a.specs = "qsgd:127,natural"
    if a.frecon and a.out_dir == ap.get_default("out_dir"):
        a.out_dir = os.path.join(ROOT, "profiles", "r14", "frecon")
    if a.frecon and a.specs == ap.get_default("specs"):
        a.specs = "qsgd:127,natural"
    if a.repeats < 1 or a.steps < 1 or a.n < 1 or a.d < 1:
        ap.error("--repeats, --steps, --n and --d are positive")
    if a.sampled:
        return main_sampled(a)
    if a.sparse:
        return main_sparse(a)
    if a.topk:
        return main_topk(a)
    if a.one_read:
        return main_one_read(a)
    if a.wire:
        return main_wire(a)
    if a.frecon:
        return main_frecon(a)
    import torch

    from flpytorch_amd import _lib
    from flpytorch_amd import aggregation as ag
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d = a.n, a.d
    os.makedirs(a.out_dir, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(1000)

    def filled():
        t = torch.empty((n, d), dtype=torch.float32, device=dev)
        for i in range(0, n, 64):
            t[i:i + 64].normal_(generator=gen)
        return t
    G, H0 = filled(), filled()
    Hf, Hc, M = torch.empty_like(H0), torch.empty_like(H0), torch.empty_like(H0)
    outs = {v: torch.empty(d, dtype=torch.float32, device=dev) for v in ("fused", "composition", "yardstick")}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    extra = {t: _lib.open_variant(t) for t in a.fused_libs.split(",") if t}
    for spec in a.specs.split(","):
        comp_f, comp_c, comp_y = (ag.initCompressor(spec, d) for _ in range(3))
        if spec.startswith("qsgd") or spec.startswith("std.dithering"):
            comp_y.dither_path = "dense"               # the two-pass dense fold, not the sparse QSGD path
        alpha = 1.0 / (1.0 + comp_f.getW())
        fused = ag.ShiftUplinkReducer(comp_f, device=dev, seed=SEED)
        yard = ag.UplinkReducer(comp_y, device=dev, seed=SEED)
        Hf.copy_(H0)
        Hc.copy_(H0)

        def run_fused():
            fused(G, Hf, alpha=alpha, shift=Hf, shift_out=Hf, out=outs["fused"])

        def run_composition():
            for i in range(n):
                comp_c.device_rng = (SEED, i)
                comp_c.compressShift(G[i], Hc[i], out=M[i], alpha=alpha, shift=Hc[i], shift_out=Hc[i])
            ag.reduce_rows(outs["composition"], M, relative=False, out=outs["composition"])

        def run_yardstick():
            yard(G, out=outs["yardstick"])
        runs = {"fused": run_fused, "composition": run_composition, "yardstick": run_yardstick}
        model = byte_model(spec, n, d)

        def run_variant(lib):
            def f():
                with _lib.use(lib):
                    fused(G, Hf, alpha=alpha, shift=Hf, shift_out=Hf, out=outs["fused"])
            return f
        for t, lib in extra.items():
            runs["fused@" + t] = run_variant(lib)
            model["fused@" + t] = model["fused"]
        for f in runs.values():                        # warm: code objects, workspaces
            f()
        torch.cuda.synchronize()

        def agree():
            return bool(extra) or (torch.equal(outs["fused"].view(torch.int32), outs["composition"].view(torch.int32))
                    and torch.equal(Hf.view(torch.int32), Hc.view(torch.int32)))
        if not agree():
            raise SystemExit(f"{spec}: fused and composition differ after the warm-up round")
        ms = {v: [] for v in runs}
        path = os.path.join(a.out_dir, spec.replace(":", "_").replace(".", "_") + ".jsonl")
        with open(path, "w") as fh:
            def emit(rec):
                line = json.dumps(rec)
                fh.write(line + "\n")
                fh.flush()
                print(line, flush=True)
            for r in range(a.repeats):
                for v, f in runs.items():
                    e0.record()
                    for _ in range(a.steps):
                        f()
                    e1.record()
                    e1.synchronize()
                    t = e0.elapsed_time(e1) / a.steps
                    ms[v].append(t)
                    emit({"spec": spec, "n": n, "d": d, "repeat": r, "variant": v, "ms_per_call": round(t, 4),
                          "algorithmic_bytes": model[v], "GBps": round(model[v] / t / 1e6, 1)})
                if not agree():
                    raise SystemExit(f"{spec}: fused and composition differ after repeat {r}")
            # the kernels' own times (the library's event timers), one call each, outside the timed repeats
            kernels = ("k_ew_shift_accum", "k_norm_partials", "k_ew_accum_vec", "k_ew_shift", "k_reduce_vec")
            kms = {}
            for v, f in runs.items():
                _lib.profile_enable(True)
                for k in kernels:
                    _lib.profile_collect(k)
                f()
                torch.cuda.synchronize()
                _lib.profile_enable(False)
                kms[v] = {k: round(t, 4) for k in kernels for t, c in [_lib.profile_collect(k)] if c}
            med = {v: statistics.median(ms[v]) for v in runs}
            emit({"spec": spec, "n": n, "d": d, "summary": True, "repeats": a.repeats, "steps": a.steps,
                  "median_ms": {v: round(med[v], 4) for v in runs},
                  "min_ms": {v: round(min(ms[v]), 4) for v in runs},
                  "max_ms": {v: round(max(ms[v]), 4) for v in runs},
                  "algorithmic_bytes": model,
                  "GBps_at_median": {v: round(model[v] / med[v] / 1e6, 1) for v in runs},
                  "composition_over_fused": round(med["composition"] / med["fused"], 3),
                  "fused_over_yardstick": round(med["fused"] / med["yardstick"], 3),
                  "byte_model_composition_over_fused": round(model["composition"] / model["fused"], 3),
                  "fused_faster_beyond_spread": max(ms["fused"]) < min(ms["composition"]),
                  "bits_equal_every_repeat": not extra,
                  "kernel_ms_one_call": kms})
        print("wrote", path, flush=True)


if __name__ == "__main__":
    main()
