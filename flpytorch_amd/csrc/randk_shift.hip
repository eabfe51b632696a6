// The sparse in-place RandK shifted round (flc_randk_shift_reduce).
//
// RandK's index set does not depend on the data, so of a DIANA / EF21 / MARINA round
//     v = a_i[j] - b_i[j];  e = randk_scale * v;  t = e * msg_scale;  m = base ? base[j] + t : t;
//     h' = shift_in[j] + shift_alpha * e
// only the K selected elements of a row are ever needed: nothing dense is formed, an in-place
// operand is written at the row's K members only, and the work is proportional to N K (plus the
// 128-B line granularity of the gathers), not to N D.  Every operation is rounded separately, in
// the order above: a selected element and d_out carry flc_encode_shift_reduce's bits.
//
// Shapes A - D: the table in flcodec.h (shift_shape, shift.hip).  A stores h' and folds t, B stores m
// and folds the updated rows (fold_updated_rows), C folds base + t, D folds t.
//
// Device draws: k_randk_shift, k_randk_fold's walk (randk.hip) with two gathers per member and an
// epilogue — one wave per chunk (or 1/2, 1/4 of its columns), rows in order, AP rows' gathers in
// flight.  The lane that loaded b_q[j] is the only one that stores to (q, j), and a row's members
// are distinct, so in place is safe.  Shape C keeps the sum in registers (the LDS tile holds the
// current row's t by column, +0 elsewhere): every column takes w_q * (base[j] + tile[j]) per row,
// which is w_q * (base[j] + 0.0f * msg_scale) outside the row's set (msg_scale is finite and > 0).
// Compat draws: the chunk-bucketed lists of randk.hip (k_randk_coarse / k_randk_fine), their values
// rewritten to t by k_randk_shift_lists (which also stores the in-place element), then k_chunk_accum
// (A, D) or the list form of the shape C fold.  Shape B needs no lists.
#include <algorithm>
#include <cmath>

#include "chunks.hpp"
#include "randk_tree.hpp"

namespace flc {

struct RksArgs {
    const float* a; int64_t lda;
    float* b;       int64_t ldb;      // written at the members in shapes A (h') and B (m)
    const float* base;                // shape C: the shared [d] vector
    float scale;                      // randk_scale (D / K)
    float ms;                         // msg_scale
    float alpha;                      // shift_alpha
};

__device__ inline uint64_t rks_join64(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | (uint64_t)lo; }

struct RksMeta {           // lane = row of a 64-row batch
    uint32_t m;            // members of this chunk
    uint32_t klo, khi;     // client key
    float w;
    uint32_t brow;         // a sampled round: the participant's row of b (its client id where b is indexed)
};

template <class M>
__device__ inline RksMeta rks_meta(const uint32_t* cnt, const uint64_t* ckey, const float* w, int64_t c, int64_t n,
                                   int64_t r, uint32_t clen, const M& map) {
    RksMeta m{0u, 0u, 0u, 1.f, 0u};
    if (r < n) {
        if (M::ON) m.brow = (uint32_t)map.at(r, FLC_IDX_B);
        m.m = min(cnt[c * n + r], clen);                 // <= clen by construction; never index past it
        const uint64_t k = ckey[r];
        m.klo = (uint32_t)k;
        m.khi = (uint32_t)(k >> 32);
        if (w) m.w = w[r];
    }
    return m;
}

// The lanes of a wave exchange values through its LDS tile.  To the compiler every lane is a thread of
// its own: without a fence it forwards a lane's own earlier store (the tile's reset) to its later
// load on the paths where that lane stored nothing, although another lane did.  Wavefront scope:
// no instruction is emitted (a wave's LDS operations execute in order).
__device__ inline void rks_tile_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

constexpr int RKS_AP = 8;                                 // rows in flight (their two gathers)

// M (flc_randk_shift_reduce_sampled): the b row of participant r travels with its key in RksMeta
template <int TS, int MODE, class M = MapNone>
__global__ __launch_bounds__(256) void k_randk_shift(RksArgs g, int64_t n, int64_t d, const uint32_t* __restrict__ cnt,
                                                     const uint64_t* __restrict__ ckey, const float* __restrict__ w,
                                                     float wt, float* __restrict__ out, M map) {
    constexpr int PARTS = CHUNK / TS;
    constexpr int AP = RKS_AP;
    constexpr int NR = MODE == SHAPE_C ? TS / 64 : 1;        // shape C: columns per lane, summed in registers
    constexpr uint32_t NOCOL = 0xFFFFu;                    // past the chunk: the buffer load returns 0
    static_assert(64 % AP == 0, "the ring walks a 64-row batch in whole turns");
    __shared__ __attribute__((aligned(16))) float tile[4][TS];
    __shared__ uint32_t zmask[4][TS / 32];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t C = nchunks(d);
    float* tl = tile[wv];
    const int64_t nb = (n + 63) / 64;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wv; t < C * PARTS; t += (int64_t)gridDim.x * 4) {
        const int64_t c = t / PARTS;
        const uint32_t pbase = (uint32_t)((t % PARTS) * TS);
        const int64_t cbase = c * CHUNK;
        const uint32_t clen = (uint32_t)min((int64_t)CHUNK, d - cbase);
        float acc[NR], bs[NR];
        if (MODE == SHAPE_C) {
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const uint32_t col = pbase + (uint32_t)(k * 64 + lane);
                acc[k] = -0.f;                                 // the additive identity: the first term is assigned
                bs[k] = col < clen ? g.base[cbase + col] : 0.f;
                tl[k * 64 + lane] = 0.f;
            }
        } else {
            for (int i = lane; i < TS; i += 64) tl[i] = -0.f;
        }
        uint32_t ro[AP];                                      // ring: part-local column (>= TS: none)
        float ra[AP], rb[AP];                                 //       gathered a, b
        // row r's members of this part for this lane: two gathers in flight
        auto fetch = [&](int slot, int64_t r, uint32_t m, uint64_t k, int64_t br) {
            const int64_t rr = min(r, n - 1);                 // (rows past n have m == 0: nothing is loaded)
            const int64_t rowb = M::ON ? br : rr;             // (M::ON: row 0 past n)
            const rktree::ChunkPerm P(k, c, clen);
            uint32_t col = (uint32_t)lane < m ? P((uint32_t)lane) : NOCOL;
            if (PARTS > 1 && col - pbase >= (uint32_t)TS) col = NOCOL;   // another wave's part: no gather
            const auto rsa = chunk_rsrc(g.a + rr * g.lda, cbase, d);
            const auto rsb = chunk_rsrc(g.b + rowb * g.ldb, cbase, d);
            ro[slot] = col - pbase;
            ra[slot] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsa, (int)(col * 4u), 0, 0));
            rb[slot] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsb, (int)(col * 4u), 0, 0));
        };
        // one member (part-local column loc < TS) of row r: the epilogue, the in-place store, the fold
        auto member = [&](uint32_t loc, float av, float bv, int64_t rowb, float wi) {
            const float v = av - bv;
            const float e = g.scale * v;
            const float tt = e * g.ms;
            if (MODE == SHAPE_A) {
                const auto rsb = chunk_rsrc(g.b + rowb * g.ldb, cbase, d);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(bv + g.alpha * e), rsb, (int)((pbase + loc) * 4u), 0, 0);
            }
            if (MODE == SHAPE_C) tl[loc] = tt;
            else tl[loc] = tl[loc] + wi * tt;
        };
        RksMeta cur = rks_meta(cnt, ckey, w, c, n, lane, clen, map), nxt;
#pragma unroll
        for (int q = 0; q < AP; ++q)
            fetch(q, q, (uint32_t)__builtin_amdgcn_readlane(cur.m, q),
                  rks_join64((uint32_t)__builtin_amdgcn_readlane(cur.khi, q), (uint32_t)__builtin_amdgcn_readlane(cur.klo, q)),
                  M::ON ? (int64_t)(uint32_t)__builtin_amdgcn_readlane(cur.brow, q) : (int64_t)q);
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t i0 = b * 64;
            nxt = rks_meta(cnt, ckey, w, c, n, i0 + 64 + lane, clen, map);
#pragma unroll 1
            for (int q0 = 0; q0 < 64; q0 += AP) {
                const bool wrap = q0 + AP >= 64;              // the refills come from the next batch
#pragma unroll
                for (int z = 0; z < AP; ++z) {
                    const int q = q0 + z;
                    const int64_t r = i0 + q;
                    if (r < n) {
                        const float wi = __uint_as_float((uint32_t)__builtin_amdgcn_readlane(__float_as_uint(cur.w), q));
                        const uint32_t m = (uint32_t)__builtin_amdgcn_readlane(cur.m, q);
                        const int64_t rowb = M::ON ? (int64_t)(uint32_t)__builtin_amdgcn_readlane(cur.brow, q) : r;
                        if (ro[z] < (uint32_t)TS) member(ro[z], ra[z], rb[z], rowb, wi);
                        if (m > 64u) {                        // a row with more than 64 members here: its tail in place
                            const uint64_t k = rks_join64((uint32_t)__builtin_amdgcn_readlane(cur.khi, q),
                                                          (uint32_t)__builtin_amdgcn_readlane(cur.klo, q));
                            const rktree::ChunkPerm P(k, c, clen);
                            const float* ap = g.a + r * g.lda + cbase;
                            const float* bp = g.b + rowb * g.ldb + cbase;
                            for (uint32_t e = 64u + lane; e < m; e += 64) {
                                const uint32_t col = P(e), l2 = col - pbase;
                                if (l2 < (uint32_t)TS) member(l2, ap[col], bp[col], rowb, wi);
                            }
                        }
                        if (MODE == SHAPE_C) {                  // every column: w * (base + t), t = +0 outside the set
                            rks_tile_fence();
#pragma unroll
                            for (int k = 0; k < NR; ++k) {
                                acc[k] = acc[k] + wi * (bs[k] + tl[k * 64 + lane]);
                                tl[k * 64 + lane] = 0.f;
                            }
                        }
                    }
                    const int qq = (q + AP) & 63;
                    const uint32_t mn = (uint32_t)(wrap ? __builtin_amdgcn_readlane(nxt.m, qq) : __builtin_amdgcn_readlane(cur.m, qq));
                    const uint32_t kh = (uint32_t)(wrap ? __builtin_amdgcn_readlane(nxt.khi, qq) : __builtin_amdgcn_readlane(cur.khi, qq));
                    const uint32_t kl = (uint32_t)(wrap ? __builtin_amdgcn_readlane(nxt.klo, qq) : __builtin_amdgcn_readlane(cur.klo, qq));
                    const int64_t bn = M::ON ? (int64_t)(uint32_t)(wrap ? __builtin_amdgcn_readlane(nxt.brow, qq) : __builtin_amdgcn_readlane(cur.brow, qq))
                                             : r + AP;
                    fetch(z, r + AP, mn, rks_join64(kh, kl), bn);
                }
            }
            cur = nxt;
        }
        const int64_t len = min((int64_t)TS, (int64_t)clen - (int64_t)pbase);
        rks_tile_fence();
        if (MODE == SHAPE_C) {
#pragma unroll
            for (int k = 0; k < NR; ++k)
                if (k * 64 + lane < len) out[cbase + pbase + k * 64 + lane] = acc[k] / wt;
        } else {
            rk_resolve_neg_zero<TS>(tl, zmask[wv], cnt, ckey, c, n, pbase, clen, len, w, lane);
            for (int64_t i = lane; i < len; i += 64) out[cbase + pbase + i] = tl[i] / wt;
        }
    }
}

// Shape B, device draws: no fold here (reduce_impl reads the updated rows afterwards), so the walk is
// row-major like k_randk_gen — a wave stays inside one row, chunk after chunk.
template <class M = MapNone>
__global__ __launch_bounds__(256) void k_randk_shift_scatter(RksArgs g, int64_t n, int64_t d,
                                                             const uint32_t* __restrict__ cnt,
                                                             const uint64_t* __restrict__ ckey, M map) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t C = nchunks(d);
    for (int64_t row = blockIdx.y; row < n; row += gridDim.y) {
        const uint64_t k = ckey[row];
        const float* ap = g.a + row * g.lda;
        float* bp = g.b + map.at_s(row, FLC_IDX_B) * g.ldb;
        for (int64_t c = (int64_t)blockIdx.x * 4 + wv; c < C; c += (int64_t)gridDim.x * 4) {
            const int64_t cbase = c * CHUNK;
            const uint32_t clen = (uint32_t)min((int64_t)CHUNK, d - cbase);
            const uint32_t m = min(cnt[c * n + row], clen);
            const rktree::ChunkPerm P(k, c, clen);
            for (uint32_t t = (uint32_t)lane; t < m; t += 64) {
                const int64_t j = cbase + P(t);               // < cbase + clen <= d
                const float bv = bp[j];
                const float e = g.scale * (ap[j] - bv);
                bp[j] = bv + e * g.ms;
            }
        }
    }
}

// Compat, shapes A / C / D: entry (row, t) of the bucketed lists gets its value t = e * msg_scale and,
// in shape A, the thread that gathered b[j] stores h'.  An index >= d stores nothing.
template <int MODE, class M = MapNone>
__global__ __launch_bounds__(256) void k_randk_shift_lists(RksArgs g, int64_t n, int64_t d, int64_t K, RkLists L, M map) {
    for (int64_t row = blockIdx.y; row < n; row += gridDim.y) {
        const float* ap = g.a + row * g.lda;
        float* bp = g.b + map.at_s(row, FLC_IDX_B) * g.ldb;
        for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < K; t += (int64_t)gridDim.x * 256) {
            const int64_t j = (int64_t)L.idx[row * L.cap + t];
            float tt = 0.f;
            if (j < d) {
                const float bv = bp[j];
                const float e = g.scale * (ap[j] - bv);
                tt = e * g.ms;
                if (MODE == SHAPE_A) bp[j] = bv + g.alpha * e;
            }
            L.val[row * L.cap + t] = tt;
        }
    }
}

// Compat, shape B: one thread per (row, t) straight from the caller's index rows
template <class M = MapNone>
__global__ __launch_bounds__(256) void k_randk_shift_idx(RksArgs g, int64_t n, int64_t d, int64_t K,
                                                         const int64_t* __restrict__ idx, int64_t ldi, M map) {
    for (int64_t row = blockIdx.y; row < n; row += gridDim.y) {
        const float* ap = g.a + row * g.lda;
        float* bp = g.b + map.at_s(row, FLC_IDX_B) * g.ldb;
        for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < K; t += (int64_t)gridDim.x * 256) {
            const int64_t j = idx[row * ldi + t];
            if ((uint64_t)j < (uint64_t)d) {
                const float bv = bp[j];
                const float e = g.scale * (ap[j] - bv);
                bp[j] = bv + e * g.ms;
            }
        }
    }
}

// Compat, shape C: the fold of base + t from the lists, the form of k_randk_shift<TS, SHAPE_C>
template <int TS>
__global__ __launch_bounds__(256) void k_randk_shift_lfold(const float* __restrict__ base, int64_t n, int64_t d, RkLists L,
                                                           const float* __restrict__ w, float wt, float* __restrict__ out) {
    constexpr int PARTS = CHUNK / TS;
    constexpr int NR = TS / 64;
    __shared__ __attribute__((aligned(16))) float tile[4][TS];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t C = nchunks(d);
    float* tl = tile[wv];
    for (int64_t t = (int64_t)blockIdx.x * 4 + wv; t < C * PARTS; t += (int64_t)gridDim.x * 4) {
        const int64_t c = t / PARTS;
        const uint32_t pbase = (uint32_t)((t % PARTS) * TS);
        const int64_t cbase = c * CHUNK;
        const uint32_t clen = (uint32_t)min((int64_t)CHUNK, d - cbase);
        float acc[NR], bs[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const uint32_t col = pbase + (uint32_t)(k * 64 + lane);
            acc[k] = -0.f;
            bs[k] = col < clen ? base[cbase + col] : 0.f;
            tl[k * 64 + lane] = 0.f;
        }
        for (int64_t r = 0; r < n; ++r) {
            const uint2 te = L.tab[c * n + r];
            const float wi = w ? w[r] : 1.f;
            for (uint32_t e = (uint32_t)lane; e < te.y; e += 64) {
                const int64_t p = r * L.cap + te.x + e;
                const uint32_t loc = L.idx[p] - (uint32_t)cbase - pbase;
                if (loc < (uint32_t)TS) tl[loc] = L.val[p];
            }
            rks_tile_fence();
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                acc[k] = acc[k] + wi * (bs[k] + tl[k * 64 + lane]);
                tl[k * 64 + lane] = 0.f;
            }
        }
        const int64_t len = min((int64_t)TS, (int64_t)clen - (int64_t)pbase);
#pragma unroll
        for (int k = 0; k < NR; ++k)
            if (k * 64 + lane < len) out[cbase + pbase + k * 64 + lane] = acc[k] / wt;
    }
}

// ------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------
constexpr int RKS_CTS = 1024;                               // shape C's part: 16 sums + 16 base values per lane

static int64_t rks_chunks(int64_t d) { return (d + CHUNK - 1) / CHUNK; }
static int rks_blocks(int64_t items, int64_t cap) { return (int)std::max<int64_t>(1, std::min<int64_t>(items, cap)); }

int randk_shift_lfold_launch(const float* base, int64_t n, int64_t d, RkLists L, const float* w, float wt, float* out,
                             hipStream_t st) {
    ProfScope _ps("k_randk_shift_lfold", st);
    const int ab = rks_blocks((rks_chunks(d) * (CHUNK / RKS_CTS) + 3) / 4, 16384);
    hipLaunchKernelGGL(k_randk_shift_lfold<RKS_CTS>, dim3(ab), dim3(256), 0, st, base, n, d, L, w, wt, out);
    FLC_CHECK_LAUNCH("k_randk_shift_lfold");
    return FLC_OK;
}

size_t randk_shift_workspace(const flc_codec_params* prm, bool compat, int64_t n, int64_t d, bool sampled) {
    if (n <= 0 || d <= 0) return 0;
    const size_t b = compat ? randk_lists_workspace(n, d, std::max<int64_t>(1, prm->k)) : randk_device_workspace(n, d);
    return sampled ? align_up(b, 256) + sampled_tab_bytes(n) : b;   // + shape B's pointer table of the mapped rows
}

// mk: MapNone{} (the contiguous round: its launches as they were) or the sampled round's MapIds
template <class M>
static int randk_shift_go(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows& sr, int64_t n, int64_t d,
                          const float* w, float wt, float* out, void* ws, size_t ws_bytes, hipStream_t st,
                          const flc_row_map* map, M mk) {
    const char* me = map ? "flc_randk_shift_reduce_sampled" : "flc_randk_shift_reduce";
    const int shape = shift_shape(sr, me);
    if (shape < 0) return FLC_ERR_UNSUPPORTED;
    const bool compat = pat && pat->d_randk_idx;
    const int64_t K = prm->k;
    if (int rc = sparse_round_precheck(me, shape, sr, map_has(map, FLC_IDX_B) ? map->n_total : n, d, K)) return rc;
    const size_t base_ws = randk_shift_workspace(prm, compat, n, d);
    if (ws_bytes < randk_shift_workspace(prm, compat, n, d, map != nullptr)) { set_error("%s: workspace too small", me); return FLC_ERR_WORKSPACE; }
    const float** tab = map ? reinterpret_cast<const float**>(static_cast<char*>(ws) + align_up(base_ws, 256)) : nullptr;
    const int64_t C = rks_chunks(d);
    RksArgs g{sr.d_a, sr.lda, const_cast<float*>(sr.d_b), sr.ldb, sr.d_base, prm->randk_scale, sr.msg_scale, sr.shift_alpha};
    const unsigned gy = (unsigned)std::min<int64_t>(n, 65535);
    if (compat) {
        if (shape == SHAPE_B) {
            {
                ProfScope _ps("k_randk_shift_lists", st);
                const int gx = rks_blocks((K + 255) / 256, 1024);
                hipLaunchKernelGGL(k_randk_shift_idx<M>, dim3((unsigned)gx, gy), dim3(256), 0, st, g, n, d, K, pat->d_randk_idx,
                                   pat->idx_ld ? pat->idx_ld : K, mk);
                FLC_CHECK_LAUNCH("k_randk_shift_idx");
            }
            return fold_updated_rows(sr, n, d, w, wt, out, st, map, tab);
        }
        RkLists L;
        RowSrc rows{sr.d_a, sr.lda, nullptr};
        if (int rc = randk_lists_build(prm, pat, rows, n, d, ws, &L, st)) return rc;
        {
            ProfScope _ps("k_randk_shift_lists", st);
            const int gx = rks_blocks((K + 255) / 256, 1024);
            if (shape == SHAPE_A) hipLaunchKernelGGL((k_randk_shift_lists<SHAPE_A, M>), dim3((unsigned)gx, gy), dim3(256), 0, st, g, n, d, K, L, mk);
            else hipLaunchKernelGGL((k_randk_shift_lists<SHAPE_D, M>), dim3((unsigned)gx, gy), dim3(256), 0, st, g, n, d, K, L, mk);
            FLC_CHECK_LAUNCH("k_randk_shift_lists");
        }
        if (shape != SHAPE_C) return randk_lists_fold(n, d, K, ws, w, wt, out, st);
        return randk_shift_lfold_launch(sr.d_base, n, d, L, w, wt, out, st);
    }
    const uint32_t* cnt = nullptr;
    const uint64_t* ckey = nullptr;
    if (int rc = randk_device_prepare(prm, pat, n, d, ws, &cnt, &ckey, st, map)) return rc;
    if (shape == SHAPE_B) {
        {
            ProfScope _ps("k_randk_shift", st);
            const int gx = rks_blocks((C + 3) / 4, 4096);
            hipLaunchKernelGGL(k_randk_shift_scatter<M>, dim3((unsigned)gx, gy), dim3(256), 0, st, g, n, d, cnt, ckey, mk);
            FLC_CHECK_LAUNCH("k_randk_shift_scatter");
        }
        return fold_updated_rows(sr, n, d, w, wt, out, st, map, tab);
    }
    ProfScope _ps("k_randk_shift", st);
    // few chunks (short rows): split each chunk's columns over 2 or 4 waves, as k_chunk_accum does
    const int parts = shape == SHAPE_C ? CHUNK / RKS_CTS : (C >= 1024 ? 1 : (C >= 256 ? 2 : 4));
    const int ab = rks_blocks((C * parts + 3) / 4, 16384);
    auto go = [&](auto ts, auto mode) {
        hipLaunchKernelGGL((k_randk_shift<decltype(ts)::value, decltype(mode)::value, M>), dim3(ab), dim3(256), 0, st, g, n, d,
                           cnt, ckey, w, wt, out, mk);
    };
    auto by_parts = [&](auto mode) {
        if (parts == 1) go(std::integral_constant<int, CHUNK>{}, mode);
        else if (parts == 2) go(std::integral_constant<int, CHUNK / 2>{}, mode);
        else go(std::integral_constant<int, CHUNK / 4>{}, mode);
    };
    if (shape == SHAPE_C) go(std::integral_constant<int, RKS_CTS>{}, std::integral_constant<int, SHAPE_C>{});
    else if (shape == SHAPE_A) by_parts(std::integral_constant<int, SHAPE_A>{});
    else by_parts(std::integral_constant<int, SHAPE_D>{});
    FLC_CHECK_LAUNCH("k_randk_shift");
    return FLC_OK;
}

int randk_shift_run(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows& sr, int64_t n, int64_t d,
                    const float* w, float wt, float* out, void* ws, size_t ws_bytes, hipStream_t st, const flc_row_map* map) {
    if (map) return randk_shift_go(prm, pat, sr, n, d, w, wt, out, ws, ws_bytes, st, map, map_ids(map));
    return randk_shift_go(prm, pat, sr, n, d, w, wt, out, ws, ws_bytes, st, nullptr, MapNone{});
}

}  // namespace flc
