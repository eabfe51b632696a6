// The selection core's host end: workspace sizes and carving, sel_run — a dispatcher over the TopK
// regimes and the RandK paths — the lists on their own for the shifted rounds, and the sparse wire
// unpack.  The TopK kernels with their launchers: topk_filter.hip (sample, filters), topk_select.hip
// (candidate selects, radix and exact fallback, tie kernels), lone_row.hip (the lone resident row).
// RandK: randk.hip; the chunk-owner fold: chunk_accum.hip.  Data flow, workspace and switches:
// select_impl.hpp.
#include "select_impl.hpp"

namespace flc {

// ------------------------------------------------------------------------------------------
// Host orchestration
// ------------------------------------------------------------------------------------------
int64_t sel_capacity(int codec, int64_t d, int64_t K) {
    if (codec == FLC_RANDK) return std::max<int64_t>(K, 1);
    // candidates of the fast path (~K (1 + 4/sqrt(ks))) with margin; the exact path needs K + CHUNK
    int64_t cap = 2 * K + 2 * CHUNK;
    cap = std::min<int64_t>(std::max<int64_t>(cap, 1), std::max<int64_t>(d, 1));
    return (cap + 3) & ~int64_t(3);        // rows of the candidate lists start 16 B aligned
}

SelWs carve_sel(void* base, int codec, int64_t n, int64_t d, int64_t K, size_t* bytes) {
    Carver cv(base);
    const int64_t C = std::max<int64_t>(host_chunks(d), 1), nn = std::max<int64_t>(n, 1);
    SelWs s;
    s.tie_hi = 0;
    s.cap = sel_capacity(codec, d, K);
    s.tab = cv.take<uint2>((size_t)C * nn);
    s.ent_idx = cv.take<uint32_t>((size_t)nn * s.cap);
    s.ent_val = cv.take<float>((size_t)nn * s.cap);
    s.rowcnt = cv.take<uint32_t>((size_t)nn * RCS);
    s.flags = cv.take<uint32_t>(nn);
    s.thr = cv.take<uint32_t>(nn);
    s.prefix = cv.take<uint32_t>(nn);
    s.krem = cv.take<uint32_t>(nn);
    s.worklist = cv.take<uint32_t>(nn);
    s.nwork = cv.take<uint32_t>(4);
    s.zm = cv.take<uint32_t>((size_t)C * (CHUNK / 32));
    s.part = codec == FLC_TOPK ? cv.take<float>((size_t)C * CHUNK) : nullptr;
    if (codec == FLC_TOPK) {
        s.tieprefix = cv.take<uint32_t>((size_t)C * nn);
        s.tiecut = cv.take<uint32_t>(nn);
        s.hist = cv.take<uint32_t>((size_t)nn * HBINS);
        s.cursor = nullptr;
        s.cstate = cv.take<uint32_t>((size_t)nn * CS_ST);
        s.clist = cv.take<uint64_t>((size_t)std::min<int64_t>(nn, CS_FEW) * CS_LCAP);
        s.carrive = cv.take<uint32_t>((size_t)nn * RCS);
        s.shcnt = cv.take<uint32_t>((size_t)std::min<int64_t>(nn, CS_FEW) * CS_SH * RCS);
    } else {
        s.tieprefix = nullptr;
        s.tiecut = nullptr;
        s.hist = nullptr;
        s.cursor = cv.take<uint32_t>((size_t)std::max<int64_t>(C, RK_SB) * nn);   // RandK: [N][RK_SB] segment offsets
        s.cstate = nullptr;
        s.clist = nullptr;
        s.carrive = nullptr;
        s.shcnt = nullptr;
    }
    if (bytes) *bytes = cv.bytes();
    return s;
}

size_t sel_workspace(const flc_codec_params* prm, int64_t n, int64_t d) {
    size_t b = 0;
    carve_sel(nullptr, prm->codec, n, d, prm->k, &b);
    // RandK: the pattern (compat lists or device draws) is not known at the size query; device
    // draws use the same lists plus the count tree
    if (prm->codec == FLC_RANDK) b += randk_device_workspace(n, d);
    return b;
}

static bool assign_fold() {          // tuning runs: FLC_ASSIGN_FOLD=1 writes a lone row's output chunk by chunk
    static const bool v = [] { const char* e = tuning_env("FLC_ASSIGN_FOLD"); return e && atoi(e) == 1; }();
    return v;
}

static bool cs_single() {            // tuning runs: FLC_CS_SINGLE=1 keeps the one-workgroup select for few rows
    static const bool v = [] { const char* e = tuning_env("FLC_CS_SINGLE"); return e && atoi(e) == 1; }();
    return v;
}

static int lone_path() {           // tuning runs: env FLC_LONE_PATH overrides
    static const int v = [] { const char* e = tuning_env("FLC_LONE_PATH"); return e ? atoi(e) : FLC_LONE_PATH; }();
    return v;
}

// Row groups of the TopK fast path whose candidate select + exact fallback run on a side stream
// under the next group's filter (one fold of all rows at the end), at least 64 rows each: 4
// (measured at C3, same box, two runs each: 8.18 ms / step with 1 group, 8.15 with 2, 8.00-8.01
// with 4, 8.04 with 8; profiles/r03/ab_tailov.txt); tuning builds FLC_TK_TAILOV=g.  (The same
// overlap of the sparse QSGD norm + resolve lost at C4, 10.20 -> 10.27-10.44 ms: its filter split
// in groups runs slower, and dither_sparse.hip no longer carries it.)
static int tk_tail_groups(const flc_codec_params* prm, int64_t n) {
    static const int g = [] { const char* e = tuning_env("FLC_TK_TAILOV"); return e ? std::max(1, atoi(e)) : 4; }();
    const int hint = (prm->flags >> 8) & 0xFF;                       // FLC_ROW_GROUPS(g): the caller's
    if (hint) return (int)std::max<int64_t>(1, std::min<int64_t>(hint, n));
    return (int)std::max<int64_t>(1, std::min<int64_t>(g, n / 64));
}
namespace {
struct TkCtx {
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ev;
};
std::mutex g_tk_mu;
std::map<int, TkCtx> g_tk_ctx;
}  // namespace

static uint32_t tie_hi_of(const flc_codec_params* prm) { return prm->tie == FLC_TIE_HIGHEST ? 1u : 0u; }

// A lone compressVector row up to RS_U * 4096 elements per CU (any K): in registers, one
// launch.  Not inside a stream capture (the call's sequence number and the cross-stream
// serialisation are host state a replayed graph would not redo): the list path there.
static int topk_lone_resident(const TkCall& c, bool* took) {
    *took = false;
    if (!(c.assign && c.n == 1 && !assign_fold() && lone_path() == 2)) return FLC_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    FLC_CHECK_HIP(hipStreamIsCapturing(c.st, &cap));
    if (cap != hipStreamCaptureStatusNone) return FLC_OK;
    return lone_resident_launch(c.rows, c.d, c.K, c.ws, c.out, c.st, took);
}

// Every K that is not dense (K <= D / 16): the sample, then per row group the filter (the full
// read), the candidate select and the exact fallback of the group's rows; with TG > 1 groups the
// select + fallback of group g run on a side stream under the filter of group g + 1 (both per-row,
// other rows' lists), and the side stream is joined back to st at the end.
static int topk_fast_groups(const TkCall& c) {
    const int64_t n = c.n, d = c.d;
    const SelWs& ws = c.ws;
    const hipStream_t st = c.st;
    const bool few = c.few;
    const int TG = few ? 1 : tk_tail_groups(c.prm, n);
    hipStream_t sside = st;
    TkCtx* cx = nullptr;
    std::unique_lock<std::mutex> lk;
    if (TG > 1) {
        int dev = 0;
        FLC_CHECK_HIP(hipGetDevice(&dev));
        lk = std::unique_lock<std::mutex>(g_tk_mu);
        cx = &g_tk_ctx[dev];
        if (!cx->side) {
            int lo = 0, hi = 0;
            FLC_CHECK_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
            FLC_CHECK_HIP(hipStreamCreateWithPriority(&cx->side, hipStreamNonBlocking, hi));
        }
        while ((int)cx->ev.size() < TG + 3) {
            hipEvent_t e;
            FLC_CHECK_HIP(hipEventCreateWithFlags(&e, FLC_SYNC_EVENT_FLAGS));
            cx->ev.push_back(e);
        }
        sside = cx->side;
    }
    // the sample: group 0's rows before its filter; with row groups the other rows' samples run
    // on the side stream beside group 0's filter (after the work queued before this call), and
    // group 1's filter waits for them — only group 0's share of the sample is exposed
    const bool split = FLC_TK_SPLIT_SAMPLE && TG > 1;
    const int64_t rs1 = split ? group_row(n, TG, 1, FLC_TK_LASTPCT) : n;
    if (split) {
        FLC_CHECK_HIP(hipEventRecord(cx->ev[TG + 1], st));
        FLC_CHECK_HIP(hipStreamWaitEvent(sside, cx->ev[TG + 1], 0));
    }
    launch_sample(c, 0, rs1, st);
    FLC_CHECK_LAUNCH("k_topk_sample");
    if (split) {
        launch_sample(c, rs1, n, sside);
        FLC_CHECK_LAUNCH("k_topk_sample (side)");
        FLC_CHECK_HIP(hipEventRecord(cx->ev[TG + 2], sside));
    }
    for (int g = 0; g < TG; ++g) {
        const int64_t r0 = group_row(n, TG, g, FLC_TK_LASTPCT), rn = group_row(n, TG, g + 1, FLC_TK_LASTPCT) - r0;
        if (split && g == 1) FLC_CHECK_HIP(hipStreamWaitEvent(st, cx->ev[TG + 2], 0));
        { ProfScope _ps("k_topk_filter", st);
        launch_filter_rows(c, r0, rn); }
        FLC_CHECK_LAUNCH("k_topk_filter");
        if (TG > 1) {
            FLC_CHECK_HIP(hipEventRecord(cx->ev[g], st));
            FLC_CHECK_HIP(hipStreamWaitEvent(sside, cx->ev[g], 0));
        }
        { ProfScope _ps("k_cand_select", sside);
        launch_select(c, r0, rn, c.gfold ? g == TG - 1 : (TG > 1 && g == TG - 1), sside); }
        FLC_CHECK_LAUNCH("k_cand_select");
        if (c.gfold) {
            // the group's rows folded into the running tiles, on the side stream under the next
            // group's filter (the last group's: exposed)
            const bool lastg = g == TG - 1;
            if (int rc = launch_group_fold(n, d, ws, c.w, c.wt, c.out, r0, r0 + rn, g == 0, lastg, lastg || TG == 1, sside))
                return rc;
        }
    }
    if (!c.lone_assign && !c.gfold) {
        // rows the fast path failed (rare): exact selection of every group's failed rows in
        // ONE launch after the last group's select (a workgroup per row, grid-stride, rows
        // that did not fail return at once).  Per-group launches beside the next group's
        // filter held whole CUs (1024-thread workgroups) while doing nothing: the filters
        // beside them ran 40-110 us slower
        if (int rc = launch_exact_rows(c, sside)) return rc;
    }
    if (TG > 1) {
        FLC_CHECK_HIP(hipEventRecord(cx->ev[TG], sside));
        FLC_CHECK_HIP(hipStreamWaitEvent(st, cx->ev[TG], 0));
    }
    return FLC_OK;
}

// Dense K (K > D / 16: the candidate list would not be smaller than the row): every row takes the
// exact multi-launch path
static int topk_dense_k(const TkCall& c) {
    FLC_CHECK_HIP(hipMemsetAsync(c.ws.hist, 0, (size_t)c.n * HBINS * sizeof(uint32_t), c.st));
    FLC_CHECK_HIP(hipMemsetAsync(c.ws.flags, 0, (size_t)c.n * sizeof(uint32_t), c.st));
    if (int rc = launch_radix_full(c)) return rc;
    return launch_filter_exact(c);
}

// From the rows' final lists to out.  Every row's list now holds exactly its admitted entries plus,
// on the fast path, candidates below the exact threshold; k_chunk_accum admits key >= thr.
static int topk_epilogue(const TkCall& c) {
    if (c.lone_assign) return launch_assign_finish(c);   // output zeros written by the filter
    if (c.gfold) return FLC_OK;                     // the last group's fold wrote out
    if (c.assign && c.n == 1 && !assign_fold()) {
        FLC_CHECK_HIP(hipMemsetAsync(c.out, 0, (size_t)c.d * sizeof(float), c.st));
        launch_assign_scatter(c.ws, c.out, c.few, c.st);
        FLC_CHECK_LAUNCH("k_assign_scatter");
        return FLC_OK;
    }
    return launch_chunk_accum(c.n, c.d, c.ws, c.assign, c.w, c.wt, c.out, c.st);
}

// Runs the TopK / RandK pipeline for n rows and writes out (ASSIGN: n == 1 dense encode): the
// argument checks, the carve and the tie rule, then one call per regime.
// lists_only (topk_lists_build, TopK): everything up to the rows' final lists and admission state — no
// lone-row path (assign false), no row-group folds, no final fold; the side stream is joined back to st
static int sel_run_impl(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, bool vec, int64_t n, int64_t d,
                        bool assign, const float* w, float wt, float* out, void* wsp, size_t ws_bytes, hipStream_t st,
                        bool lists_only) {
    const int codec = prm->codec;
    const int64_t K = prm->k;
    if (d == 0) return FLC_OK;
    if (n == 0) { FLC_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)d * sizeof(float), st)); return FLC_OK; }
    if (K < 1 || K > d) { set_error("K=%lld outside [1, D=%lld]", (long long)K, (long long)d); return FLC_ERR_ARG; }
    if (d >= (int64_t)0xFFFFFFFF) { set_error("D too large for 32-bit entry indices"); return FLC_ERR_ARG; }
    if (codec == FLC_RANDK && !(pat && pat->d_randk_idx))
        return randk_device_run(prm, pat, rows, n, d, w, wt, out, wsp, ws_bytes, st);
    size_t need = 0;
    carve_sel(nullptr, codec, n, d, K, &need);
    if (ws_bytes < need) { set_error("select: workspace %zu < %zu", ws_bytes, need); return FLC_ERR_WORKSPACE; }
    SelWs ws = carve_sel(wsp, codec, n, d, K, nullptr);
    if (codec == FLC_RANDK) {
        if (int rc = randk_lists_launch(prm, pat, rows, n, d, ws, st)) return rc;
        return launch_chunk_accum(n, d, ws, assign, w, wt, out, st);
    }
    if (prm->tie != FLC_TIE_LOWEST && prm->tie != FLC_TIE_HIGHEST) { set_error("topk: unknown tie rule %d", prm->tie); return FLC_ERR_ARG; }
    ws.tie_hi = tie_hi_of(prm);
    TkCall c{prm, rows, vec, n, d, K, assign, w, wt, out, ws, st, false, false, false};
    bool took = false;
    if (int rc = topk_lone_resident(c, &took)) return rc;
    if (took) return FLC_OK;
    const bool dense_k = K * 16 > d;   // large K: the candidate list would not be smaller than the row
    // TopK, few rows: sharded candidate lists (k_topk_filter_fast) and the spread select (k_cs_pass)
    c.few = n <= CS_FEW && !cs_single() && sel_capacity(codec, d, K) >= (int64_t)CS_SH * GCAP;
    // a lone compressVector (assign, one row) on the fast path: output zeros from the filter, the
    // exact fallback and the scatter in one launch (k_assign_finish)
    c.lone_assign = assign && n == 1 && c.few && !dense_k && !assign_fold();
    // many rows: each group's select does its own exact fallback and its rows are folded
    // right after it (tiles carried in ws.part), under the next group's filter
    c.gfold = FLC_TK_GFOLD && !c.few && !assign && !dense_k && !lists_only;
    if (int rc = dense_k ? topk_dense_k(c) : topk_fast_groups(c)) return rc;
    return lists_only ? FLC_OK : topk_epilogue(c);
}

int sel_run(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, bool vec, int64_t n, int64_t d,
            bool assign, const float* w, float wt, float* out, void* wsp, size_t ws_bytes, hipStream_t st) {
    return sel_run_impl(prm, pat, rows, vec, n, d, assign, w, wt, out, wsp, ws_bytes, st, false);
}

// The many-row TopK selection on its own (topk_shift.hip: the batched shifted round turns the admitted
// entries into messages between the selection and the fold).  build: sel_run's TopK branch over `rows`
// up to the final lists, whichever regime (few rows, 2- / 4-chunk filter, dense K, exact fallback);
// fold: k_chunk_accum over the lists and admission state as they then stand.
int topk_lists_build(const flc_codec_params* prm, RowSrc rows, bool vec, int64_t n, int64_t d, void* wsp, size_t ws_bytes,
                     TkLists* lists, hipStream_t st) {
    if (prm->codec != FLC_TOPK) { set_error("topk_lists_build: TopK only"); return FLC_ERR_ARG; }
    if (int rc = sel_run_impl(prm, nullptr, rows, vec, n, d, /*assign=*/false, nullptr, 1.f, nullptr, wsp, ws_bytes, st, true))
        return rc;
    const SelWs ws = carve_sel(wsp, FLC_TOPK, n, d, prm->k, nullptr);
    *lists = TkLists{ws.tab, ws.ent_idx, ws.ent_val, ws.cap, ws.thr, ws.flags, ws.tiecut, tie_hi_of(prm)};
    return FLC_OK;
}

int topk_lists_fold(const flc_codec_params* prm, int64_t n, int64_t d, void* wsp, const float* w, float wt, float* out,
                    hipStream_t st) {
    SelWs ws = carve_sel(wsp, FLC_TOPK, n, d, prm->k, nullptr);
    ws.tie_hi = tie_hi_of(prm);
    return launch_chunk_accum(n, d, ws, false, w, wt, out, st);
}

// flc_select_row_flags: the rows' state words the last TopK sel_run left in the workspace
int sel_row_flags(const flc_codec_params* prm, int64_t n, int64_t d, const void* wsp, size_t ws_bytes,
                  uint32_t* flags, hipStream_t st) {
    if (prm->codec != FLC_TOPK) { set_error("flc_select_row_flags: TopK only"); return FLC_ERR_ARG; }
    if (n <= 0 || d <= 0) return FLC_OK;
    size_t need = 0;
    carve_sel(nullptr, prm->codec, n, d, prm->k, &need);
    if (ws_bytes < need) { set_error("flc_select_row_flags: workspace %zu < %zu", ws_bytes, need); return FLC_ERR_WORKSPACE; }
    const SelWs ws = carve_sel(const_cast<void*>(wsp), prm->codec, n, d, prm->k, nullptr);
    FLC_CHECK_HIP(hipMemcpyAsync(flags, ws.flags, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    return FLC_OK;
}

// ------------------------------------------------------------------------------------------
// Decode + reduce of sparse wire payloads (wire.hip, SPARSE: 16-B header {fmt, count, norm, bad},
// u32 idx[cap], f32 val[cap], ascending idx): the entries are copied into the selection lists,
// each (chunk, row) range is found by binary search, and k_chunk_accum folds them in row order —
// the same fold as flc_encode_reduce, so the result is the same bits.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unpack_lists(const char* __restrict__ base, int64_t ld,
                                                      const char* const* __restrict__ ptrs, int64_t n, int64_t cap,
                                                      int64_t pcap, SelWs ws) {
    const int64_t row = blockIdx.y;
    const char* p = base ? base + row * ld : ptrs[row];
    const uint32_t cnt = (uint32_t)min<int64_t>(reinterpret_cast<const uint32_t*>(p)[1], min(cap, pcap));
    const uint32_t* pi = reinterpret_cast<const uint32_t*>(p + 16);
    const float* pv = reinterpret_cast<const float*>(p + 16 + ((4 * pcap + 15) & ~int64_t(15)));
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < cnt; e += (int64_t)gridDim.x * 256) {
        ws.ent_idx[row * ws.cap + e] = pi[e];
        ws.ent_val[row * ws.cap + e] = pv[e];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ws.thr[row] = 0;
        ws.flags[row] = F_EXACT;
        ws.rowcnt[row * RCS] = cnt;
    }
}

__global__ __launch_bounds__(256) void k_unpack_tab(int64_t n, int64_t d, SelWs ws) {
    const int64_t row = blockIdx.y, C = nchunks(d);
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const uint32_t cnt = ws.rowcnt[row * RCS];
    const uint32_t* idx = ws.ent_idx + row * ws.cap;
    auto lb = [&](uint64_t key) {
        uint32_t lo = 0, hi = cnt;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((uint64_t)idx[mid] < key) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    const uint32_t a = lb((uint64_t)c << CHUNK_SHIFT), b = lb((uint64_t)(c + 1) << CHUNK_SHIFT);
    ws.tab[c * n + row] = make_uint2(a, b - a);
}

size_t sel_unpack_workspace(const flc_codec_params* prm, int64_t n, int64_t d) {
    size_t b = 0;
    carve_sel(nullptr, FLC_RANDK, n, d, std::max<int64_t>(1, std::min(prm->k, d)), &b);
    return b;
}

int sel_unpack_reduce(const flc_codec_params* prm, const void* base, int64_t ld_bytes, const void* const* ptrs,
                      int64_t n, int64_t d, const float* w, float wt, float* out, void* wsp, size_t ws_bytes,
                      hipStream_t st) {
    const int64_t K = std::max<int64_t>(1, std::min(prm->k, d));
    if (ws_bytes < sel_unpack_workspace(prm, n, d)) { set_error("flc_unpack_reduce: workspace too small"); return FLC_ERR_WORKSPACE; }
    if (d >= (int64_t)0xFFFFFFFF) { set_error("D too large for 32-bit entry indices"); return FLC_ERR_ARG; }
    SelWs ws = carve_sel(wsp, FLC_RANDK, n, d, K, nullptr);
    const int64_t C = host_chunks(d);
    dim3 g1((unsigned)std::max<int64_t>(1, std::min<int64_t>((K + 255) / 256, 64)), (unsigned)n);
    hipLaunchKernelGGL(k_unpack_lists, g1, dim3(256), 0, st, (const char*)base, ld_bytes, (const char* const*)ptrs, n,
                       ws.cap, K, ws);
    FLC_CHECK_LAUNCH("k_unpack_lists");
    hipLaunchKernelGGL(k_unpack_tab, dim3((unsigned)((C + 255) / 256), (unsigned)n), dim3(256), 0, st, n, d, ws);
    FLC_CHECK_LAUNCH("k_unpack_tab");
    return launch_chunk_accum_whole(n, d, ws, w, wt, out, st);
}

}  // namespace flc
