// Shift codecs: the client-side update of the compressed algorithms,
//     e = C(a - b);   msg = base + e * scale;   h_out = h_in + alpha * e
// DIANA  m_i = C(g - h_i), h_i += alpha m_i                      algorithms.py:1383-1391
// EF21   g_next = g_prev + C(g - g_prev) * (1 / (1 + w) | 1)     algorithms.py:1506-1517
// MARINA g_next = g_prev + C(g - g_prev_x)                       algorithms.py:537, 691
// FRECON / COFIG u_i = C(g - h_i), h_i += alpha u_i              algorithms.py:1104-1110, 1265-1269
// (FRECON's second message q_i = C(g - g(x_prev)) and its round of n clients: codecs.hip
// k_ew_frecon_accum, flc_frecon_reduce)
//
// Elementwise codecs (ident, lazy, natural, dithering) run one fused pass (codecs.hip k_ew_shift,
// after the norm pass over a - b for dithering): a, b [, base, h_in] read once, msg [, h_out]
// written once, e never stored.  RandK / TopK / Rank-K select or factor the whole difference first:
// a - b is formed once in the workspace, encoded by the ordinary single-row path into a second
// workspace row, and k_shift_epi applies the same epilogue.
#include <cmath>

#include "common.hpp"

namespace flc {

__global__ __launch_bounds__(256) void k_shift_sub(const float* __restrict__ a, const float* __restrict__ b, int64_t d,
                                                   float* __restrict__ diff) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t g4 = d / 4;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < g4; g += stride) {
        const float4 x = reinterpret_cast<const float4*>(a)[g], y = reinterpret_cast<const float4*>(b)[g];
        reinterpret_cast<float4*>(diff)[g] = make_float4(x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w);
    }
    for (int64_t j = g4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < d; j += stride) diff[j] = a[j] - b[j];
}

__global__ __launch_bounds__(256) void k_shift_sub_scalar(const float* __restrict__ a, const float* __restrict__ b,
                                                          int64_t d, float* __restrict__ diff) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < d; j += (int64_t)gridDim.x * blockDim.x)
        diff[j] = a[j] - b[j];
}

// the epilogue over a stored e (scalar loads: the caller's msg / base / h may be unaligned views)
__global__ __launch_bounds__(256) void k_shift_epi(const float* __restrict__ e, int64_t d, ShiftArgs sh) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < d; j += (int64_t)gridDim.x * blockDim.x) {
        const float v = e[j];
        if (sh.msg) {
            const float t = v * sh.scale;
            sh.msg[j] = sh.base ? sh.base[j] + t : t;
        }
        if (sh.hout) sh.hout[j] = sh.hin[j] + sh.alpha * v;
    }
}

static bool shift_elementwise(int codec) { return codec != FLC_RANDK && codec != FLC_TOPK && codec != FLC_RANK_K; }

static size_t inner_workspace(const flc_codec_params* prm, int64_t d) {
    if (prm->codec == FLC_TOPK) return sel_workspace(prm, 1, d);
    if (prm->codec == FLC_RANK_K) return rk_workspace(prm, 1, d, false);
    return randk_device_workspace(1, d);   // RandK: the device draws' chunk counts
}

size_t shift_workspace(const flc_codec_params* prm, int64_t d) {
    if (shift_elementwise(prm->codec)) return ew_workspace(prm, 1, d);
    Carver c(nullptr);
    c.take<float>((size_t)d);
    c.take<float>((size_t)d);
    c.take<char>(inner_workspace(prm, d));
    return c.bytes();
}

int shift_run(const flc_codec_params* prm, const flc_pattern* pat, const float* a, int64_t d, const ShiftArgs& sh,
              float* pnorm_out, void* ws, size_t ws_bytes, hipStream_t st) {
    if (d == 0) return FLC_OK;
    if (ws_bytes < shift_workspace(prm, d)) { set_error("flc_encode_shift: workspace too small"); return FLC_ERR_WORKSPACE; }
    if (shift_elementwise(prm->codec)) {
        const bool vec = (((uintptr_t)a | (uintptr_t)sh.b) & 15u) == 0;
        RowSrc s{a, d, nullptr};
        return ew_run(prm, pat, s, vec, 1, d, nullptr, pnorm_out, /*dense=*/true, nullptr, nullptr, 1.f, ws, ws_bytes,
                      st, &sh);
    }
    float* e = nullptr;
    if (int rc = shift_encode_dense(prm, pat, a, sh.b, d, &e, ws, ws_bytes, st)) return rc;
    return shift_epi_launch(e, d, sh, st);
}

int shift_encode_dense(const flc_codec_params* prm, const flc_pattern* pat, const float* a, const float* b, int64_t d,
                       float** e_out, void* ws, size_t ws_bytes, hipStream_t st) {
    (void)ws_bytes;
    Carver c(ws);
    float* diff = c.take<float>((size_t)d);
    float* e = c.take<float>((size_t)d);
    const size_t inner = inner_workspace(prm, d);
    void* iws = c.take<char>(inner);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((d + 1023) / 1024, 4096));
    if ((((uintptr_t)a | (uintptr_t)b) & 15u) == 0)
        hipLaunchKernelGGL(k_shift_sub, dim3(grid), dim3(256), 0, st, a, b, d, diff);
    else
        hipLaunchKernelGGL(k_shift_sub_scalar, dim3(grid), dim3(256), 0, st, a, b, d, diff);
    FLC_CHECK_LAUNCH("k_shift_sub");
    int rc = FLC_OK;
    RowSrc r{diff, d, nullptr};
    if (prm->codec == FLC_RANDK) {
        if (!(pat && pat->d_randk_idx) && prm->k > d) { set_error("randk: K > D"); return FLC_ERR_ARG; }
        rc = randk_dense(prm, pat, diff, d, e, iws, inner, st);
    } else if (prm->codec == FLC_TOPK) {
        rc = sel_run(prm, pat, r, true, 1, d, /*assign=*/true, nullptr, 1.f, e, iws, inner, st);
    } else {
        rc = rk_run(prm, r, 1, d, /*reduce=*/false, nullptr, 1.f, e, iws, inner, st);
    }
    if (rc) return rc;
    *e_out = e;
    return FLC_OK;
}

int shift_epi_launch(const float* e, int64_t d, const ShiftArgs& sh, hipStream_t st) {
    const int g2 = (int)std::max<int64_t>(1, std::min<int64_t>((d + 255) / 256, 8192));
    hipLaunchKernelGGL(k_shift_epi, dim3(g2), dim3(256), 0, st, e, d, sh);
    FLC_CHECK_LAUNCH("k_shift_epi");
    return FLC_OK;
}

// ------------------------------------------------------------------------------------------
// The shifted fold over n rows (flc_encode_shift_reduce).  Elementwise codecs: one tile-owner pass
// (codecs.hip k_ew_shift_accum).  RandK / TopK / Rank-K: the rows in order through shift_run into
// a message row (the workspace's, or the caller's d_msg row i), each followed by one fold step
// into d_out — acc = first ? w m : acc + w m, divided after the last row.  Correct and bounded in
// workspace, not a fast path (n selections, 2 n small launches).  RandK's in-place and store-free
// rounds have their sparse entry (flc_randk_shift_reduce, randk_shift.hip: work ~ n K) and TopK's a
// batched one over the many-row selection's lists (flc_topk_shift_reduce, topk_shift.hip); a
// list-based fold for Rank-K is future work.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_shift_fold(const float* __restrict__ m, int64_t d, const float* __restrict__ w,
                                                    int64_t i, int last, float wt, float* __restrict__ acc) {
    const float wi = w ? w[i] : 1.f;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < d; j += (int64_t)gridDim.x * blockDim.x) {
        const float t = w ? wi * m[j] : m[j];
        float a = (i == 0) ? t : acc[j] + t;
        if (last) a = a / wt;
        acc[j] = a;
    }
}

int shift_fold_launch(const float* m, int64_t d, const float* w, int64_t i, bool last, float wt, float* acc,
                      hipStream_t st) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((d + 255) / 256, 8192));
    hipLaunchKernelGGL(k_shift_fold, dim3(grid), dim3(256), 0, st, m, d, w, i, last ? 1 : 0, wt, acc);
    FLC_CHECK_LAUNCH("k_shift_fold");
    return FLC_OK;
}

size_t shift_reduce_workspace(const flc_codec_params* prm, int64_t n, int64_t d) {
    if (shift_elementwise(prm->codec)) return ew_shift_reduce_workspace(prm, n, d);
    Carver c(nullptr);
    c.take<float>((size_t)d);
    c.take<char>(shift_workspace(prm, d));
    return c.bytes();
}

// map (flc_encode_shift_reduce_sampled): participant i is client map->h_ids[i]; the elementwise
// kernels read the device ids, the row loop below takes its row pointers and keys from the host ids
int shift_reduce_run(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows& sr, int64_t n, int64_t d,
                     const float* w, float wt, float* pnorms_out, float* out, void* ws, size_t ws_bytes, hipStream_t st,
                     const flc_row_map* map) {
    if (n == 0 || d == 0) return FLC_OK;
    const char* me = map ? "flc_encode_shift_reduce_sampled" : "flc_encode_shift_reduce";
    if (ws_bytes < shift_reduce_workspace(prm, n, d)) { set_error("%s: workspace too small", me); return FLC_ERR_WORKSPACE; }
    if (shift_elementwise(prm->codec)) {
        const bool vec = ((((uintptr_t)sr.d_a | (uintptr_t)sr.d_b) & 15u) == 0) && (((sr.lda | sr.ldb) & 3) == 0);
        RowSrc a{sr.d_a, sr.lda, nullptr};
        return ew_run(prm, pat, a, vec, n, d, nullptr, pnorms_out, /*dense=*/false, out, w, wt, ws, ws_bytes, st, nullptr,
                      nullptr, FLC_NORMMODE_EXACT, &sr, map);
    }
    if (prm->codec == FLC_RANDK && !(pat && pat->d_randk_idx) && prm->k > d) { set_error("randk: K > D"); return FLC_ERR_ARG; }
    Carver c(ws);
    float* mrow = c.take<float>((size_t)d);
    const size_t inner = shift_workspace(prm, d);
    void* iws = c.take<char>(inner);
    for (int64_t i = 0; i < n; ++i) {
        flc_pattern pi;
        memset(&pi, 0, sizeof(pi));
        if (pat) {
            pi = *pat;
            if (pat->d_randk_idx) pi.d_randk_idx = pat->d_randk_idx + i * (pat->idx_ld ? pat->idx_ld : prm->k);
            if (pat->d_uniforms) pi.d_uniforms = pat->d_uniforms + i * (pat->uniforms_ld ? pat->uniforms_ld : d);
            if (pat->d_lazy_u) pi.d_lazy_u = pat->d_lazy_u + i;
            pi.d_randk_counts = nullptr;        // (laid out [chunk][n]: one row's are computed inside)
        }
        const int64_t ci = map ? (int64_t)map->h_ids[i] : i;
        auto at = [&](uint32_t bit) { return map_has(map, bit) ? ci : i; };   // the operand's row of participant i
        pi.client0 = (pat ? pat->client0 : 0) + ci;
        float* m = sr.d_msg ? sr.d_msg + at(FLC_IDX_MSG) * sr.ldmsg : mrow;
        ShiftArgs sh{sr.d_b + at(FLC_IDX_B) * sr.ldb, sr.msg_scale, sr.d_base ? sr.d_base + at(FLC_IDX_BASE) * sr.ldbase : nullptr, m,
                     sr.shift_alpha, sr.d_shift_out ? sr.d_shift_in + at(FLC_IDX_SHIFT_IN) * sr.ldin : nullptr,
                     sr.d_shift_out ? sr.d_shift_out + at(FLC_IDX_SHIFT_OUT) * sr.ldout : nullptr};
        if (int rc = shift_run(prm, &pi, sr.d_a + i * sr.lda, d, sh, nullptr, iws, inner, st)) return rc;
        if (int rc = shift_fold_launch(m, d, w, i, i == n - 1, wt, out, st)) return rc;
    }
    return FLC_OK;
}

// ------------------------------------------------------------------------------------------
// Host plumbing shared by the sparse rounds (randk_shift.hip, topk_shift.hip, dither_shift.hip)
// ------------------------------------------------------------------------------------------
// sr: api.hip's normalised copy (no shift_in without a shift_out, leading dimensions of absent
// operands zeroed)
int shift_shape(const flc_shift_rows& sr, const char* me) {
    if (!(std::isfinite(sr.msg_scale) && sr.msg_scale > 0.f)) {
        set_error("%s: msg_scale must be finite and > 0 (got %g)", me, (double)sr.msg_scale);
        return -1;
    }
    if (sr.d_shift_out) {
        if (sr.d_base || sr.d_msg) { set_error("%s: a shift together with a base or stored messages is not a sparse shape", me); return -1; }
        if ((const float*)sr.d_shift_out != sr.d_b || sr.d_shift_in != sr.d_b || sr.ldout != sr.ldb || sr.ldin != sr.ldb) {
            set_error("%s: the shift must be updated in place over the b rows (d_shift_in == d_shift_out == d_b, equal leading dimensions)", me);
            return -1;
        }
        if (!(std::isfinite(sr.shift_alpha) && sr.shift_alpha > 0.f)) {
            set_error("%s: shift_alpha must be finite and > 0 (got %g)", me, (double)sr.shift_alpha);
            return -1;
        }
        return SHAPE_A;
    }
    if (sr.d_msg) {
        if (sr.d_base != sr.d_b || (const float*)sr.d_msg != sr.d_b || sr.ldbase != sr.ldb || sr.ldmsg != sr.ldb) {
            set_error("%s: stored messages only as the in-place EF21 step (d_base == d_msg == d_b, equal leading dimensions)", me);
            return -1;
        }
        return SHAPE_B;
    }
    if (sr.d_base) {
        if (sr.ldbase != 0) { set_error("%s: a per-row base that is not d_msg == d_b (only ONE shared base, ldbase == 0, folds without a store)", me); return -1; }
        return SHAPE_C;
    }
    return SHAPE_D;
}

int inplace_rows_check(const char* me, int shape, const flc_shift_rows& sr, int64_t n, int64_t d) {
    // (n: the rows of the in-place matrix; a sampled round over indexed rows passes n_total)
    if (n > 1 && (shape == SHAPE_A || shape == SHAPE_B) && (sr.ldb < 0 ? -sr.ldb : sr.ldb) < d) {
        set_error("%s: the in-place rows overlap (|ldb| < d)", me);
        return FLC_ERR_ARG;
    }
    return FLC_OK;
}

int sparse_round_precheck(const char* me, int shape, const flc_shift_rows& sr, int64_t n, int64_t d, int64_t K) {
    if (K < 1 || K > d) { set_error("%s: K=%lld outside [1, D=%lld]", me, (long long)K, (long long)d); return FLC_ERR_ARG; }
    if (d >= (int64_t)0xFFFFFFFF) { set_error("%s: D too large for 32-bit entry indices", me); return FLC_ERR_ARG; }
    return inplace_rows_check(me, shape, sr, n, d);
}

// the rows of an indexed operand as a pointer table: tab[i] = base + ids[i] * ld
__global__ __launch_bounds__(256) void k_row_ptrs(const float* base, int64_t ld, MapIds map, int64_t n, const float** tab) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) tab[i] = base + map.id(i) * ld;
}

int row_ptrs_launch(const float* base, int64_t ld, const flc_row_map* map, int64_t n, const float** tab, hipStream_t st) {
    hipLaunchKernelGGL(k_row_ptrs, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 256)), dim3(256), 0, st, base, ld,
                       map_ids(map), n, tab);
    FLC_CHECK_LAUNCH("k_row_ptrs");
    return FLC_OK;
}

size_t sampled_tab_bytes(int64_t n) { return align_up((size_t)std::max<int64_t>(n, 1) * sizeof(const float*), 256); }

int fold_updated_rows(const flc_shift_rows& sr, int64_t n, int64_t d, const float* w, float wt, float* out, hipStream_t st,
                      const flc_row_map* map, const float** tab) {
    const bool vec = (((uintptr_t)sr.d_b & 15u) == 0) && (sr.ldb % 4 == 0);
    if (map_has(map, FLC_IDX_B)) {
        if (int rc = row_ptrs_launch(sr.d_b, sr.ldb, map, n, tab, st)) return rc;
        RowSrc rows{nullptr, 0, tab};
        return reduce_impl(rows, vec, n, d, nullptr, w, wt, FLC_REDUCE_PLAIN, out, st);
    }
    RowSrc rows{sr.d_b, sr.ldb, nullptr};
    return reduce_impl(rows, vec, n, d, nullptr, w, wt, FLC_REDUCE_PLAIN, out, st);
}

}  // namespace flc
