// The sparse shifted-wire fold (flc_unpack_shift_reduce_sparse): the server step of a shifted round
// from n SPARSE messages (RandK / TopK payloads) in one pass,
//     t = v * scale;  m = base ? base_i[j] + t : t   for an entry (j, v) of payload i
//     out = (sum_i w_i m_i) / wt   folded in row order, the first term assigned
// in the shapes B (EF21's server mirror in place), C (MARINA's one shared base) and D (the plain
// fold) of the shape table in flcodec.h.  flc_unpack_shift_reduce takes these payloads row by row
// through a dense [d] workspace row (four launches and about 28 d bytes per client); here a mirror
// row is read once and written at the listed elements only: 4 n d + 12 n K + 4 d bytes in shape B.
//
// Two launches.  k_sparse_tile_tab cuts every payload's ascending index list at the boundaries of
// the 4096-element tiles: tab[c * n + i] = (first entry, count) of payload i in tile c, the whole
// workspace (8 n C bytes, no [d]-sized row).  k_sparse_shift_accum is a tile owner like
// k_unpack_shift_accum: one 256-thread workgroup folds one tile for all n rows in order, so every
// element of a mirror row is read, and where listed written, by one thread, the load before the store.
//
// A thread owns 16 elements of the tile as four float4 (element q * 1024 + 4 * thread + r is its
// number k = 4 q + r) and keeps their 16 sums in registers.  Per row the first `count` lanes stage
// the row's entries of this tile into LDS: t at the element's local slot and one mark bit, bit k of
// the owner's 16-bit mark word.  The owner reads its word; only a nonzero word (few threads at
// K = 1 %) sends it to the t slots, and it clears the word it has consumed, so no pass over the
// marks is needed between rows and a slot is never read unless this row wrote it.  Two LDS buffers
// alternate by row: the entries of row i + 1 are staged before row i is folded, one barrier per row.
// The base float4s of the next PF rows are in flight in a register ring (shape B); shape C keeps
// the shared base, and base + 0 * scale for the unlisted elements, in registers and reads no
// per-row HBM besides the entries; shape D has no base.
//
// What a malformed message can do is bounded as in k_unpack_sparse: the count is cut at cap, an
// index >= d is never stored to, and an entry outside the tile its position claims (an index list
// that does not ascend) is dropped.
#include <cmath>

#include "chunks.hpp"
#include "wire_codes.hpp"

namespace flc {

struct SparsePayloads {
    const char* pbase;
    int64_t ld;
    const char* const* ptrs;
    int64_t cap;
    // wave-uniform i: a pointer list is read through the scalar cache
    __device__ inline const char* row(int64_t i) const { return pbase ? pbase + i * ld : sload(ptrs + i); }
    __device__ inline const uint32_t* idx(const char* p) const { return reinterpret_cast<const uint32_t*>(p + 16); }
    __device__ inline const float* val(const char* p) const { return reinterpret_cast<const float*>(p + 16 + a16(4 * cap)); }
};

// grid (ceil(C / 256), n): thread (c, i) finds the entries of payload i whose index lies in tile c
__global__ __launch_bounds__(256) void k_sparse_tile_tab(SparsePayloads pr, int64_t n, int64_t C, uint2* __restrict__ tab) {
    const int64_t i = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const char* p = pr.row(i);
    const uint32_t cnt = (uint32_t)min<int64_t>(reinterpret_cast<const PayloadHeader*>(p)->count, pr.cap);
    const uint32_t* idx = pr.idx(p);
    auto lower = [&](uint64_t key) {                    // the first entry whose index is >= key
        uint32_t lo = 0, hi = cnt;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if ((uint64_t)idx[mid] < key) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    const uint32_t first = lower((uint64_t)c << CHUNK_SHIFT), last = lower((uint64_t)(c + 1) << CHUNK_SHIFT);
    tab[c * n + i] = make_uint2(first, last > first ? last - first : 0u);
}

// n == 0: the empty sum (a kernel, so that the call can be recorded into a graph)
__global__ __launch_bounds__(256) void k_sparse_zero(float* __restrict__ out, int64_t d) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < d; j += (int64_t)gridDim.x * 256) out[j] = 0.f;
}

// four consecutive elements of a row at element o; past the row's end: 0, never read
template <bool VEC>
__device__ inline float4 st_load4(const float* row, int64_t o, int64_t d) {
    if (VEC && o + 4 <= d) return *reinterpret_cast<const float4*>(row + o);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o < d) r.x = row[o];
    if (o + 1 < d) r.y = row[o + 1];
    if (o + 2 < d) r.z = row[o + 2];
    if (o + 3 < d) r.w = row[o + 3];
    return r;
}

enum { SB_NONE = 0, SB_ROWS = 1, SB_SHARED = 2 };     // shapes D, B, C

constexpr int ST_Q = 4;                                // float4s per thread
constexpr int ST_E = 4 * ST_Q;                         // elements per thread: 256 threads own a tile
constexpr int ST_QSTRIDE = CHUNK / ST_Q;               // elements between a thread's float4s

template <int BASE_MODE, bool W, class M, bool VEC, int PF>
__global__ __launch_bounds__(256) void k_sparse_shift_accum(SparsePayloads pr, const uint2* __restrict__ tab, int64_t n,
                                                            int64_t d, float scale, float* base, int64_t ldbase, M map,
                                                            const float* __restrict__ w, float wt, float* __restrict__ out) {
    static_assert(ST_E * 256 == CHUNK, "256 threads own one tile");
    __shared__ float tv[2][CHUNK];
    __shared__ uint32_t mk[2][256];
    const int t = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x << CHUNK_SHIFT;
    const uint2* trow = tab + (int64_t)blockIdx.x * n;
    mk[0][t] = 0u;
    mk[1][t] = 0u;
    __syncthreads();

    // row i's entries of this tile into buffer i & 1: t at the local slot, the owner's mark bit
    auto stage = [&](int64_t i) {
        const uint64_t pairw = sload(reinterpret_cast<const uint64_t*>(trow + i));   // one 8-byte scalar load
        const uint2 fc = make_uint2((uint32_t)pairw, (uint32_t)(pairw >> 32));
        const char* p = pr.row(i);
        const uint32_t* idx = pr.idx(p) + fc.x;
        const float* val = pr.val(p) + fc.x;
        float* tvb = tv[i & 1];
        uint32_t* mkb = mk[i & 1];
        for (uint32_t e = t; e < fc.y; e += 256) {
            const uint32_t j = idx[e];
            const int64_t l = (int64_t)j - tile0;
            if (l >= 0 && l < CHUNK && (int64_t)j < d) {
                tvb[l] = val[e] * scale;
                atomicOr(&mkb[(l >> 2) & 255], 1u << (((l / ST_QSTRIDE) << 2) | (l & 3)));
            }
        }
    };
    auto mirror = [&](int64_t i) -> float* { return base + map.at_s(i, FLC_IDX_BASE) * ldbase; };
    auto load_row = [&](int64_t i, float4 (&r)[ST_Q]) {
        const float* br = mirror(i);
#pragma unroll
        for (int q = 0; q < ST_Q; ++q) r[q] = st_load4<VEC>(br, tile0 + q * ST_QSTRIDE + 4 * t, d);
    };
    auto spread = [](const float4 (&r)[ST_Q], float (&v)[ST_E]) {
#pragma unroll
        for (int q = 0; q < ST_Q; ++q) { v[4 * q] = r[q].x; v[4 * q + 1] = r[q].y; v[4 * q + 2] = r[q].z; v[4 * q + 3] = r[q].w; }
    };

    float4 ring[PF][ST_Q];
    if (BASE_MODE == SB_ROWS) {
#pragma unroll
        for (int p = 0; p < PF; ++p)
            if (p < n) load_row(p, ring[p]);
    }
    const float z = 0.0f * scale;                      // an unlisted element's t: evaluated, not assumed
    float sb[ST_E], sbz[ST_E];                         // the shared base and base + z
    if (BASE_MODE == SB_SHARED) {
        float4 r[ST_Q];
#pragma unroll
        for (int q = 0; q < ST_Q; ++q) r[q] = st_load4<VEC>(base, tile0 + q * ST_QSTRIDE + 4 * t, d);
        spread(r, sb);
#pragma unroll
        for (int k = 0; k < ST_E; ++k) sbz[k] = sb[k] + z;
    }

    float acc[ST_E];
    stage(0);
    for (int64_t i0 = 0; i0 < n; i0 += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int64_t i = i0 + p;
            if (i < n) {
                __syncthreads();                       // row i is staged; buffer (i + 1) & 1 has been consumed
                if (i + 1 < n) stage(i + 1);
                float bs[ST_E], m[ST_E];
                if (BASE_MODE == SB_ROWS) {
                    spread(ring[p], bs);
                    if (i + PF < n) load_row(i + PF, ring[p]);
                }
#pragma unroll
                for (int k = 0; k < ST_E; ++k) m[k] = BASE_MODE == SB_ROWS ? bs[k] : (BASE_MODE == SB_SHARED ? sbz[k] : z);
                const uint32_t word = mk[i & 1][t];
                if (word) {
                    mk[i & 1][t] = 0u;
                    const float* tvb = tv[i & 1];
                    float* mr = BASE_MODE == SB_ROWS ? mirror(i) + tile0 : nullptr;
#pragma unroll
                    for (int k = 0; k < ST_E; ++k) {
                        if (word & (1u << k)) {
                            const int l = (k >> 2) * ST_QSTRIDE + 4 * t + (k & 3);
                            const float tt = tvb[l];
                            m[k] = BASE_MODE == SB_ROWS ? bs[k] + tt : (BASE_MODE == SB_SHARED ? sb[k] + tt : tt);
                            if (BASE_MODE == SB_ROWS) mr[l] = m[k];
                        }
                    }
                }
                const float wi = W ? w[i] : 1.f;
#pragma unroll
                for (int k = 0; k < ST_E; ++k) {
                    const float wm = W ? wi * m[k] : m[k];
                    acc[k] = (i == 0) ? wm : acc[k] + wm;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < ST_Q; ++q) {
        const int64_t o = tile0 + q * ST_QSTRIDE + 4 * t;
        if (o + 4 <= d && ((uintptr_t)(out + o) & 15u) == 0) {
            *reinterpret_cast<float4*>(out + o) = make_float4(acc[4 * q] / wt, acc[4 * q + 1] / wt, acc[4 * q + 2] / wt, acc[4 * q + 3] / wt);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (o + r < d) out[o + r] = acc[4 * q + r] / wt;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------
size_t unpack_shift_sparse_workspace(int64_t n, int64_t d) {
    Carver c(nullptr);
    c.take<uint2>((size_t)n * (size_t)nchunks(d));
    return c.bytes();
}

// The accepted shape of a call (SHAPE_B / C / D of the table in flcodec.h), recognised by pointer and
// leading dimension, or -1 with the reason set: pr is api.hip's normalised copy.
int unpack_shift_sparse_shape(const flc_payload_rows& pr, const char* me) {
    if (!(std::isfinite(pr.msg_scale) && pr.msg_scale > 0.f)) {
        set_error("%s: msg_scale must be finite and > 0 (got %g)", me, (double)pr.msg_scale);
        return -1;
    }
    if (pr.d_msg) {
        if ((const float*)pr.d_msg != pr.d_base || pr.ldmsg != pr.ldbase) {
            set_error("%s: stored messages only as the mirror in place (d_msg == d_base, equal leading dimensions)", me);
            return -1;
        }
        return SHAPE_B;
    }
    if (pr.d_base) {
        if (pr.ldbase != 0) { set_error("%s: a per-row base without d_msg == d_base (only ONE shared base, ldbase == 0, folds without a store)", me); return -1; }
        return SHAPE_C;
    }
    return SHAPE_D;
}

template <int BASE_MODE, class M>
static void sparse_accum_launch(bool weighted, bool vec, int64_t C, hipStream_t st, SparsePayloads sp, const uint2* tab,
                                int64_t n, int64_t d, const flc_payload_rows& pr, M map, const float* w, float wt, float* out) {
    float* base = const_cast<float*>(pr.d_base);       // shape B: d_msg, the rows stored to
#define SPARSE_ACCUM_GO(WW, VV)                                                                                    \
    hipLaunchKernelGGL((k_sparse_shift_accum<BASE_MODE, WW, M, VV, 4>), dim3((unsigned)C), dim3(256), 0, st, sp, tab, n, d, \
                       pr.msg_scale, base, pr.ldbase, map, w, wt, out)
    if (weighted) { if (vec) SPARSE_ACCUM_GO(true, true); else SPARSE_ACCUM_GO(true, false); }
    else { if (vec) SPARSE_ACCUM_GO(false, true); else SPARSE_ACCUM_GO(false, false); }
#undef SPARSE_ACCUM_GO
}

int unpack_shift_sparse_run(const flc_codec_params* prm, const flc_payload_rows& pr, int shape, const flc_row_map* map,
                            int64_t n, int64_t d, const float* w, float wt, float* out, void* ws, size_t ws_bytes,
                            hipStream_t st) {
    if (ws_bytes < unpack_shift_sparse_workspace(n, d)) { set_error("flc_unpack_shift_reduce_sparse: workspace too small"); return FLC_ERR_WORKSPACE; }
    if (n == 0) {
        hipLaunchKernelGGL(k_sparse_zero, dim3((unsigned)std::min<int64_t>((d + 255) / 256, 4096)), dim3(256), 0, st, out, d);
        FLC_CHECK_LAUNCH("k_sparse_zero");
        return FLC_OK;
    }
    const int64_t C = nchunks(d);
    Carver c(ws);
    uint2* tab = c.take<uint2>((size_t)n * (size_t)C);
    SparsePayloads sp{static_cast<const char*>(pr.d_payloads), pr.ld_bytes, reinterpret_cast<const char* const*>(pr.d_payload_ptrs),
                      std::max<int64_t>(1, std::min(prm->k, d))};
    { ProfScope _ps("k_sparse_tile_tab", st);
    hipLaunchKernelGGL(k_sparse_tile_tab, dim3((unsigned)((C + 255) / 256), (unsigned)n), dim3(256), 0, st, sp, n, C, tab); }
    FLC_CHECK_LAUNCH("k_sparse_tile_tab");
    const bool vec = pr.d_base && ((uintptr_t)pr.d_base & 15u) == 0 && ((uint64_t)pr.ldbase & 3u) == 0;
    { ProfScope _ps("k_sparse_shift_accum", st);
    if (shape == SHAPE_B) {
        if (map_has(map, FLC_IDX_BASE)) sparse_accum_launch<SB_ROWS>(w != nullptr, vec, C, st, sp, tab, n, d, pr, map_ids(map), w, wt, out);
        else sparse_accum_launch<SB_ROWS>(w != nullptr, vec, C, st, sp, tab, n, d, pr, MapNone{}, w, wt, out);
    } else if (shape == SHAPE_C) {
        sparse_accum_launch<SB_SHARED>(w != nullptr, vec, C, st, sp, tab, n, d, pr, MapNone{}, w, wt, out);
    } else {
        sparse_accum_launch<SB_NONE>(w != nullptr, false, C, st, sp, tab, n, d, pr, MapNone{}, w, wt, out);
    } }
    FLC_CHECK_LAUNCH("k_sparse_shift_accum");
    return FLC_OK;
}

}  // namespace flc
