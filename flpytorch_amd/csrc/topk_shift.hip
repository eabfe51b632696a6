// The batched TopK shifted round (flc_topk_shift_reduce).
//
// A DIANA / EF21 / MARINA round with TopK,
//     v = a_i[j] - b_i[j];  S_i = the K largest |v| of row i;  for j in S_i:  e = v;  t = e * msg_scale;
//     m = base ? base[j] + t : t;   h' = shift_in[j] + shift_alpha * e
// for all n rows in a constant number of launches instead of the general entry's row loop:
//   k_shift_sub_rows      the n differences into a workspace matrix [n][ldd], one streaming launch
//   topk_lists_build      the selection core's many-row TopK (select.hip's dispatcher; kernels in
//                         topk_filter.hip, topk_select.hip) over that matrix, unchanged, up to the rows'
//                         final (index, value) lists and admission state
//   k_topk_shift_lists    the sparse epilogue: every admitted entry becomes its message value t and, in
//                         the in-place shapes, the thread that gathered b_i[j] stores the updated element;
//                         entries the admission rule rejects are turned into "no column"
//   k_topk_shift_admit    the rows' admission state set to admit-all (the values' keys have changed)
//   the fold              k_chunk_accum (A, D), k_randk_shift_lfold (C), reduce_impl over the rows (B)
// Every operation is rounded separately, in the order above: a selected element and d_out carry
// flc_encode_shift_reduce's bits; an in-place operand is written at the row's K members only.
//
// Shapes A - D: the table in flcodec.h, the folds as the RandK round's (randk_shift.hip).
#include <algorithm>
#include <cmath>

#include "chunks.hpp"

namespace flc {

struct TksArgs {
    const float* a; int64_t lda;
    float* b;       int64_t ldb;      // written at the members in shapes A (h') and B (m)
    float* diff;    int64_t ldd;      // the workspace matrix of differences
    float ms;                         // msg_scale
    float alpha;                      // shift_alpha
};

constexpr int TKS_U = 4;              // float4 load pairs a thread keeps in flight

// diff[r][j] = a_r[j] - b_r[j], j < d (nothing at [d, ldd)).  VEC: every a and b row 16-B aligned; a and
// b are read once (nontemporal), the difference is stored plainly: the filter reads it next.
// M (flc_topk_shift_reduce_sampled): b_r is the participant's client row where b is indexed.
template <bool VEC, class M = MapNone>
__global__ __launch_bounds__(256) void k_shift_sub_rows(TksArgs g, int64_t n, int64_t d, M map) {
    for (int64_t row = blockIdx.y; row < n; row += gridDim.y) {
        const float* ap = g.a + row * g.lda;
        const float* bp = g.b + map.at_s(row, FLC_IDX_B) * g.ldb;
        float* dp = g.diff + row * g.ldd;
        int64_t done = 0;
        if (VEC) {
            const int64_t u4 = d / 4;
            const float4* a4 = reinterpret_cast<const float4*>(ap);
            const float4* b4 = reinterpret_cast<const float4*>(bp);
            float4* d4 = reinterpret_cast<float4*>(dp);
            const int64_t step = (int64_t)gridDim.x * 256 * TKS_U;
            for (int64_t g0 = (int64_t)blockIdx.x * 256 * TKS_U + threadIdx.x; g0 < u4; g0 += step) {
                float4 x[TKS_U], y[TKS_U];
#pragma unroll
                for (int k = 0; k < TKS_U; ++k) {
                    const int64_t i = g0 + k * 256;
                    if (i < u4) { x[k] = ld_row4(a4 + i); y[k] = ld_row4(b4 + i); }
                }
#pragma unroll
                for (int k = 0; k < TKS_U; ++k) {
                    const int64_t i = g0 + k * 256;
                    if (i < u4) d4[i] = make_float4(x[k].x - y[k].x, x[k].y - y[k].y, x[k].z - y[k].z, x[k].w - y[k].w);
                }
            }
            done = u4 * 4;
        }
        for (int64_t j = done + (int64_t)blockIdx.x * 256 + threadIdx.x; j < d; j += (int64_t)gridDim.x * 256)
            dp[j] = ap[j] - bp[j];
    }
}

// The sparse epilogue: one wave per (row, chunk) walks the row's entries of the chunk through tab, as
// the fold does (the few-row lists are sharded: never "the first rowcnt entries").  Admission is
// chunk_accum_body's (mag_key(val), idx ^ txm) >= (T, cut), T and cut as load_meta takes them.  An
// admitted entry's value is e = v: the in-place element is stored by the thread that gathered it
// (a row's admitted indices are distinct) and, in A / C / D, the value becomes t = e * msg_scale.  A
// rejected entry (or an index >= d) becomes 0xFFFFFFFF, "no column" to every list consumer.
template <int MODE, class M = MapNone>
__global__ __launch_bounds__(256) void k_topk_shift_lists(TksArgs g, int64_t n, int64_t d, TkLists L, M map) {
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int64_t C = nchunks(d);
    const uint32_t txm = L.tie_hi ? 0u : 0xFFFFFFFFu;         // tie_pref(ix) = ix ^ txm
    for (int64_t row = blockIdx.y; row < n; row += gridDim.y) {
        uint32_t T = L.thr[row], cut = 0u;
        const uint32_t f = L.flags[row];
        if (f & TK_F_EXACT) T = 0u;                            // exact list: every entry admitted
        else if (f & TK_F_TIES) cut = L.tiecut[row] ^ txm;
        const uint64_t bound = ((uint64_t)T << 32) | (uint64_t)cut;
        float* bp = g.b + map.at_s(row, FLC_IDX_B) * g.ldb;
        for (int64_t c = (int64_t)blockIdx.x * 4 + wv; c < C; c += (int64_t)gridDim.x * 4) {
            const uint2 te = L.tab[c * n + row];
            for (uint32_t e = (uint32_t)lane; e < te.y; e += 64) {
                const int64_t p = row * L.cap + te.x + e;
                const uint32_t ix = L.ent_idx[p];
                const float ev = L.ent_val[p];
                const uint64_t key = ((uint64_t)mag_key(ev) << 32) | (uint64_t)(ix ^ txm);
                if (key >= bound && (int64_t)ix < d) {
                    const float t = ev * g.ms;
                    if (MODE == SHAPE_A) {
                        const float bv = bp[ix];
                        bp[ix] = bv + g.alpha * ev;
                    }
                    if (MODE == SHAPE_B) {
                        const float bv = bp[ix];
                        bp[ix] = bv + t;
                    } else {
                        L.ent_val[p] = t;
                    }
                } else {
                    L.ent_idx[p] = 0xFFFFFFFFu;
                }
            }
        }
    }
}

// After the walk (a launch of its own: the walk reads the state): every row admits all of its entries
// that still name a column.  Flag bits 1, 2 and 8 stay for flc_select_row_flags.
__global__ __launch_bounds__(256) void k_topk_shift_admit(int64_t n, TkLists L) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        L.thr[r] = 0u;
        L.flags[r] = L.flags[r] & ~TK_F_TIES;
    }
}

// ------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------
static int64_t tks_ldd(int64_t d) { return (d + 3) & ~int64_t(3); }

// the selection state first, exactly flc_encode_reduce's carve (flc_select_row_flags reads it at the
// workspace base), then the difference matrix; a sampled round: then shape B's pointer table
size_t topk_shift_workspace(const flc_codec_params* prm, int64_t n, int64_t d, bool sampled) {
    if (n <= 0 || d <= 0) return 0;
    Carver c(nullptr);
    c.take<char>(sel_workspace(prm, n, d));
    c.take<float>((size_t)n * (size_t)tks_ldd(d));
    if (sampled) c.take<char>(sampled_tab_bytes(n));
    return c.bytes();
}

// mk: MapNone{} (the contiguous round: its launches as they were) or the sampled round's MapIds
template <class M>
static int topk_shift_go(const flc_codec_params* prm, const flc_shift_rows& sr, int64_t n, int64_t d, const float* w, float wt,
                         float* out, void* ws, size_t ws_bytes, hipStream_t st, const flc_row_map* map, M mk) {
    const char* me = map ? "flc_topk_shift_reduce_sampled" : "flc_topk_shift_reduce";
    const int shape = shift_shape(sr, me);
    if (shape < 0) return FLC_ERR_UNSUPPORTED;
    const int64_t K = prm->k;
    const bool b_mapped = map_has(map, FLC_IDX_B);
    if (int rc = sparse_round_precheck(me, shape, sr, b_mapped ? map->n_total : n, d, K)) return rc;
    if (ws_bytes < topk_shift_workspace(prm, n, d, map != nullptr)) { set_error("%s: workspace too small", me); return FLC_ERR_WORKSPACE; }
    const int64_t ldd = tks_ldd(d);
    Carver cv(ws);
    const size_t sel_bytes = sel_workspace(prm, n, d);
    void* sws = cv.take<char>(sel_bytes);
    float* diff = cv.take<float>((size_t)n * (size_t)ldd);
    const float** tab = map ? reinterpret_cast<const float**>(cv.take<char>(sampled_tab_bytes(n))) : nullptr;
    TksArgs g{sr.d_a, sr.lda, const_cast<float*>(sr.d_b), sr.ldb, diff, ldd, sr.msg_scale, sr.shift_alpha};
    const unsigned gy = (unsigned)std::min<int64_t>(n, 65535);
    {
        ProfScope _ps("k_shift_sub_rows", st);
        // (b's leading dimension matters as soon as a second row of the matrix can be read)
        const bool one_b = b_mapped ? map->n_total == 1 : n == 1;
        const bool vec = ((((uintptr_t)sr.d_a | (uintptr_t)sr.d_b) & 15u) == 0) && ((n == 1 || (sr.lda & 3) == 0) && (one_b || (sr.ldb & 3) == 0));
        // capped and strided like the other streaming kernels: ~16 K workgroups over all rows
        const int64_t per_row = vec ? (d / 4 + 256 * TKS_U - 1) / (256 * TKS_U) : (d + 1023) / 1024;
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(per_row, std::max<int64_t>(1, 16384 / gy)));
        if (vec) hipLaunchKernelGGL((k_shift_sub_rows<true, M>), dim3(gx, gy), dim3(256), 0, st, g, n, d, mk);
        else hipLaunchKernelGGL((k_shift_sub_rows<false, M>), dim3(gx, gy), dim3(256), 0, st, g, n, d, mk);
        FLC_CHECK_LAUNCH("k_shift_sub_rows");
    }
    TkLists L;
    RowSrc rows{diff, ldd, nullptr};
    if (int rc = topk_lists_build(prm, rows, /*vec=*/true, n, d, sws, sel_bytes, &L, st)) return rc;
    {
        ProfScope _ps("k_topk_shift_lists", st);
        const int64_t C = nchunks(d);
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((C + 3) / 4, std::max<int64_t>(1, 32768 / gy)));
        const dim3 grid(gx, gy);
        if (shape == SHAPE_A) hipLaunchKernelGGL((k_topk_shift_lists<SHAPE_A, M>), grid, dim3(256), 0, st, g, n, d, L, mk);
        else if (shape == SHAPE_B) hipLaunchKernelGGL((k_topk_shift_lists<SHAPE_B, M>), grid, dim3(256), 0, st, g, n, d, L, mk);
        else hipLaunchKernelGGL((k_topk_shift_lists<SHAPE_D, M>), grid, dim3(256), 0, st, g, n, d, L, mk);
        FLC_CHECK_LAUNCH("k_topk_shift_lists");
    }
    hipLaunchKernelGGL(k_topk_shift_admit, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 256)), dim3(256), 0, st, n, L);
    FLC_CHECK_LAUNCH("k_topk_shift_admit");
    if (shape == SHAPE_B) return fold_updated_rows(sr, n, d, w, wt, out, st, map, tab);
    if (shape == SHAPE_C) {
        RkLists R{L.tab, L.ent_idx, L.ent_val, L.cap};
        return randk_shift_lfold_launch(sr.d_base, n, d, R, w, wt, out, st);
    }
    return topk_lists_fold(prm, n, d, sws, w, wt, out, st);
}

int topk_shift_run(const flc_codec_params* prm, const flc_shift_rows& sr, int64_t n, int64_t d, const float* w, float wt,
                   float* out, void* ws, size_t ws_bytes, hipStream_t st, const flc_row_map* map) {
    if (map) return topk_shift_go(prm, sr, n, d, w, wt, out, ws, ws_bytes, st, map, map_ids(map));
    return topk_shift_go(prm, sr, n, d, w, wt, out, ws, ws_bytes, st, nullptr, MapNone{});
}

}  // namespace flc
