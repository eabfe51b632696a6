// The seeded RandK message (FMT_SEEDED; include/flcodec.h "Seeded RandK messages"):
// the K' kept values alone, in the device sampler's own order, and the 64-bit key both ends draw the
// index set from.  No index is written by the client and none is read by the server.
//
//   header     {u32 fmt = 9, u32 count = K', f32 norm = 0, u32 bad = 0}
//   draw block {u32 key_lo, u32 key_hi, u32 d_lo, u32 d_hi}
//   f32 val[K'], 16-B padded with zero bytes: chunk by chunk (4096 elements, ascending), inside chunk
//   c in draw order — val[off_c + t] is element c * 4096 + ChunkPerm(key, c, clen)(t), t < m_c,
//   off_c the exclusive scan of the chunk counts m_c (randk_tree.hpp; oracle/devrng.py randk_indices)
//
// Every entry starts from the chunk counts of the key (randk.hip k_randk_counts; the server's pass
// reads each row's key from its message) and their exclusive scan per row (k_seeded_segsum /
// k_seeded_offsets: lane = row, so the [C][n] arrays are read and written in whole lines):
//   pack    k_seeded_pack   each wave takes SD_CPW consecutive chunks: lane t < m_c computes P(t),
//                           loads x[c * 4096 + P(t)] (every chunk's loads before any store) and
//                           stores scale * v at val[off_c + t] — O(K) work, nothing dense is formed
//   decode  k_seeded_unpack one wave per chunk: a +0 LDS tile, the members written at P(t), the
//                           chunk stored in whole lines
//   fold    k_seeded_fold   k_randk_fold's walk (one wave per chunk or 1/2, 1/4 of its columns, the
//                           rows in client order, SD_AP rows' loads in flight) whose gather source is
//                           the message: row q's lane t loads val_q[off_c + t], consecutive
//                           addresses, and adds w_q * v at tile[P(t)]; the -0 columns are resolved by
//                           rk_resolve_neg_zero and the tile leaves through one division by w_total
// What a kernel takes from a message is its key, and the message's d and count only to compare them
// with the call's: the counts come from the count pass (a permutation's, so m_c <= clen and their sum
// is K' whatever the key), a message of another d or count has every count 0, and a value is read
// only at a position below K'.
#include <algorithm>
#include <cstring>

#include "chunks.hpp"
#include "randk_tree.hpp"
#include "wire_codes.hpp"

namespace flc {

constexpr int SD_HEAD = 32;                               // header + draw block
constexpr int SD_CPW = 4;                                 // pack: chunks per wave trip
constexpr int SD_AP = 8;                                  // fold: rows in flight
constexpr int64_t SD_SEG = 64, SD_MAXSEG = 256;           // the scan's segments of chunks

static inline int64_t sd_chunks(int64_t d) { return (d + CHUNK - 1) / CHUNK; }
static inline int64_t sd_count(const flc_codec_params* prm, int64_t d) { return std::max<int64_t>(1, std::min(prm->k, d)); }
// chunks per scan segment: at least SD_SEG, at most SD_MAXSEG segments a row
static inline int64_t sd_seg(int64_t C) { return std::max<int64_t>(SD_SEG, (C + SD_MAXSEG - 1) / SD_MAXSEG); }

int64_t seeded_payload_bytes(const flc_codec_params* prm, int64_t d) {
    return d == 0 ? SD_HEAD : SD_HEAD + a16(4 * sd_count(prm, d));
}

// (see rks_tile_fence, randk_shift.hip: a wave's lanes exchange values through its LDS tile)
__device__ inline void sd_tile_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
__host__ __device__ inline uint64_t sd_join64(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | (uint64_t)lo; }

// ---- offsets: the exclusive scan of each row's chunk counts --------------------------------------
// Wave = one segment of `seg` chunks, lane = row: psum[s][row] = the row's members in segment s.
__global__ __launch_bounds__(256) void k_seeded_segsum(const uint32_t* __restrict__ cnt, int64_t n, int64_t C, int64_t seg,
                                                       uint32_t* __restrict__ psum) {
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t row = (int64_t)blockIdx.y * 64 + (threadIdx.x & 63);
    const int64_t c0 = s * seg, c1 = min(C, c0 + seg);
    if (row >= n || c0 >= C) return;
    uint32_t sum = 0;
    for (int64_t c = c0; c < c1; ++c) sum += cnt[c * n + row];
    psum[s * n + row] = sum;
}

// off[c][row] = the row's members in chunks before c: the segments before (<= SD_MAXSEG sums), then
// the running count inside the segment.
__global__ __launch_bounds__(256) void k_seeded_offsets(const uint32_t* __restrict__ cnt, int64_t n, int64_t C, int64_t seg,
                                                        const uint32_t* __restrict__ psum, uint32_t* __restrict__ off) {
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t row = (int64_t)blockIdx.y * 64 + (threadIdx.x & 63);
    const int64_t c0 = s * seg, c1 = min(C, c0 + seg);
    if (row >= n || c0 >= C) return;
    uint32_t run = 0;
    for (int64_t q = 0; q < s; ++q) run += psum[q * n + row];
    for (int64_t c = c0; c < c1; ++c) {
        off[c * n + row] = run;
        run += cnt[c * n + row];
    }
}

// ---- pack ---------------------------------------------------------------------------------------
// One row (cnt / off are [C]).  The header, the draw block and the padding after val[K - 1] are
// written by one lane, so a payload's bytes are a function of the row, the key and K alone.
__global__ __launch_bounds__(256) void k_seeded_pack(const float* __restrict__ x, int64_t d, int64_t K,
                                                     const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                                                     uint64_t key, float scale, char* __restrict__ payload) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t C = nchunks(d);
    float* val = reinterpret_cast<float*>(payload + SD_HEAD);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint4* h = reinterpret_cast<uint4*>(payload);
        h[0] = make_uint4((uint32_t)FMT_SEEDED, (uint32_t)K, 0u, 0u);
        h[1] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)d, (uint32_t)((uint64_t)d >> 32));
        for (int64_t i = K; i < a16(4 * K) / 4; ++i) val[i] = 0.f;
    }
    for (int64_t c0 = ((int64_t)blockIdx.x * 4 + wv) * SD_CPW; c0 < C; c0 += (int64_t)gridDim.x * 4 * SD_CPW) {
        uint32_t m[SD_CPW], o[SD_CPW];
        float v[SD_CPW];
#pragma unroll
        for (int q = 0; q < SD_CPW; ++q) {
            const int64_t c = c0 + q;
            const uint32_t clen = c < C ? (uint32_t)min((int64_t)CHUNK, d - c * CHUNK) : 1u;
            m[q] = c < C ? min(cnt[c], clen) : 0u;
            o[q] = c < C ? off[c] : 0u;
            const bool on = (uint32_t)lane < m[q] && (int64_t)o[q] + lane < K;
            const rktree::ChunkPerm P(key, c, clen);
            v[q] = on ? x[c * CHUNK + P((uint32_t)lane)] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < SD_CPW; ++q) {
            const int64_t c = c0 + q;
            if ((uint32_t)lane < m[q] && (int64_t)o[q] + lane < K) val[o[q] + lane] = scale * v[q];
            if (m[q] > 64u) {                              // a chunk with more than 64 members
                const uint32_t clen = (uint32_t)min((int64_t)CHUNK, d - c * CHUNK);
                const rktree::ChunkPerm P(key, c, clen);
                for (uint32_t t = 64u + lane; t < m[q]; t += 64)
                    if ((int64_t)o[q] + t < K) val[o[q] + t] = scale * x[c * CHUNK + P(t)];
            }
        }
    }
}

// ---- single-row decode --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_seeded_unpack(const char* __restrict__ payload, int64_t d, int64_t K,
                                                       const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                                                       const uint64_t* __restrict__ ckey, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[4][CHUNK];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t C = nchunks(d);
    const uint64_t key = ckey[0];
    const float* val = reinterpret_cast<const float*>(payload + SD_HEAD);
    float* tl = tile[wv];
    for (int64_t c = (int64_t)blockIdx.x * 4 + wv; c < C; c += (int64_t)gridDim.x * 4) {
        const int64_t cbase = c * CHUNK;
        const uint32_t clen = (uint32_t)min((int64_t)CHUNK, d - cbase);
        for (int i = lane; i < CHUNK; i += 64) tl[i] = 0.f;
        sd_tile_fence();
        const uint32_t m = min(cnt[c], clen), o = off[c];
        const rktree::ChunkPerm P(key, c, clen);
        for (uint32_t t = (uint32_t)lane; t < m; t += 64)
            if ((int64_t)o + t < K) tl[P(t)] = val[o + t];
        sd_tile_fence();
        for (uint32_t i = (uint32_t)lane; i < clen; i += 64) out[cbase + i] = tl[i];
        sd_tile_fence();
    }
}

// ---- fold ---------------------------------------------------------------------------------------
struct SdMeta {            // lane = row of a 64-row batch
    uint32_t m;            // members of this chunk
    uint32_t klo, khi;     // the message's key
    uint32_t plo, phi;     // its value list
    uint32_t off;          // the chunk's first value
    float w;
};

__device__ inline SdMeta sd_meta(const char* base, int64_t ld, const char* const* ptrs, const uint32_t* cnt,
                                 const uint32_t* off, const uint64_t* ckey, const float* w, int64_t c, int64_t n, int64_t r,
                                 uint32_t clen) {
    SdMeta m{0u, 0u, 0u, 0u, 0u, 0u, 1.f};
    if (r < n) {
        m.m = min(cnt[c * n + r], clen);                 // <= clen by construction; never index past it
        m.off = off[c * n + r];
        const uint64_t k = ckey[r];
        m.klo = (uint32_t)k;
        m.khi = (uint32_t)(k >> 32);
        const uintptr_t p = (uintptr_t)((base ? base + r * ld : ptrs[r]) + SD_HEAD);
        m.plo = (uint32_t)p;
        m.phi = (uint32_t)((uint64_t)p >> 32);
        if (w) m.w = w[r];
    }
    return m;
}

template <int TS>
__global__ __launch_bounds__(256) void k_seeded_fold(const char* __restrict__ base, int64_t ld, const char* const* __restrict__ ptrs,
                                                     int64_t n, int64_t d, int64_t K, const uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ off, const uint64_t* __restrict__ ckey,
                                                     const float* __restrict__ w, float wt, float* __restrict__ out) {
    constexpr int PARTS = CHUNK / TS;
    constexpr int AP = SD_AP;
    constexpr uint32_t NOCOL = 0xFFFFu;                    // no member of this part on this lane
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
        for (int i = lane; i < TS; i += 64) tl[i] = -0.f;     // the additive identity
        uint32_t ro[AP];                                      // ring: part-local column (>= TS: none)
        float rv[AP];                                         //       the member's value
        // a row's first 64 members of this chunk: lane t's column, and its value in flight
        auto fetch = [&](int slot, uint32_t m, uint64_t k, const float* vp, uint32_t o) {
            const rktree::ChunkPerm P(k, c, clen);
            uint32_t col = (uint32_t)lane < m ? P((uint32_t)lane) : NOCOL;
            if (PARTS > 1 && col - pbase >= (uint32_t)TS) col = NOCOL;   // another wave's part: no load
            ro[slot] = col - pbase;
            rv[slot] = (col != NOCOL && (int64_t)o + lane < K) ? vp[o + lane] : 0.f;
        };
        auto fetch_q = [&](int slot, const SdMeta& mt, int q) {
            // readlane returns int: widen through uint32_t (a sign-extended low word would set the high one)
            fetch(slot, (uint32_t)__builtin_amdgcn_readlane(mt.m, q),
                  sd_join64((uint32_t)__builtin_amdgcn_readlane(mt.khi, q), (uint32_t)__builtin_amdgcn_readlane(mt.klo, q)),
                  (const float*)sd_join64((uint32_t)__builtin_amdgcn_readlane(mt.phi, q),
                                          (uint32_t)__builtin_amdgcn_readlane(mt.plo, q)),
                  (uint32_t)__builtin_amdgcn_readlane(mt.off, q));
        };
        SdMeta cur = sd_meta(base, ld, ptrs, cnt, off, ckey, w, c, n, lane, clen), nxt;
#pragma unroll
        for (int q = 0; q < AP; ++q) fetch_q(q, cur, q);
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t i0 = b * 64;
            nxt = sd_meta(base, ld, ptrs, cnt, off, ckey, w, c, n, i0 + 64 + lane, clen);
#pragma unroll 1
            for (int q0 = 0; q0 < 64; q0 += AP) {
                const bool wrap = q0 + AP >= 64;              // the refills come from the next batch
#pragma unroll
                for (int z = 0; z < AP; ++z) {
                    const int q = q0 + z;
                    const float wi = __uint_as_float((uint32_t)__builtin_amdgcn_readlane(__float_as_uint(cur.w), q));
                    if (ro[z] < (uint32_t)TS) tl[ro[z]] = tl[ro[z]] + wi * rv[z];
                    const uint32_t m = (uint32_t)__builtin_amdgcn_readlane(cur.m, q);
                    if (m > 64u) {                            // a row with more than 64 members here: its tail in place
                        const uint64_t k = sd_join64((uint32_t)__builtin_amdgcn_readlane(cur.khi, q),
                                                     (uint32_t)__builtin_amdgcn_readlane(cur.klo, q));
                        const float* vp = (const float*)sd_join64((uint32_t)__builtin_amdgcn_readlane(cur.phi, q),
                                                                  (uint32_t)__builtin_amdgcn_readlane(cur.plo, q));
                        const uint32_t o = (uint32_t)__builtin_amdgcn_readlane(cur.off, q);
                        const rktree::ChunkPerm P(k, c, clen);
                        for (uint32_t e = 64u + lane; e < m; e += 64) {
                            const uint32_t l2 = P(e) - pbase;
                            if (l2 < (uint32_t)TS && (int64_t)o + e < K) tl[l2] = tl[l2] + wi * vp[o + e];
                        }
                    }
                    if (wrap) fetch_q(z, nxt, (q + AP) & 63);
                    else fetch_q(z, cur, q + AP);
                }
            }
            cur = nxt;
        }
        const int64_t len = min((int64_t)TS, (int64_t)clen - (int64_t)pbase);
        sd_tile_fence();
        rk_resolve_neg_zero<TS>(tl, zmask[wv], cnt, ckey, c, n, pbase, clen, len, w, lane);
        for (int64_t i = lane; i < len; i += 64) out[cbase + pbase + i] = tl[i] / wt;
        sd_tile_fence();
    }
}

// out = +0 (n == 0: the empty fold), by a kernel so the entry may be recorded into a graph
__global__ __launch_bounds__(256) void k_seeded_zero(float* __restrict__ out, int64_t d) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < d; i += (int64_t)gridDim.x * 256) out[i] = 0.f;
}

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
struct SdWs {
    uint32_t* cnt;     // [C][n]
    uint32_t* off;     // [C][n]
    uint32_t* psum;    // [segments][n]
    uint64_t* ckey;    // [n]
};

static SdWs carve_sd(void* base, int64_t n, int64_t d, size_t* bytes) {
    Carver cv(base);
    const int64_t C = std::max<int64_t>(sd_chunks(d), 1), nn = std::max<int64_t>(n, 1);
    SdWs s;
    s.cnt = cv.take<uint32_t>((size_t)C * nn);
    s.off = cv.take<uint32_t>((size_t)C * nn);
    s.psum = cv.take<uint32_t>((size_t)((C + sd_seg(C) - 1) / sd_seg(C)) * nn);
    s.ckey = cv.take<uint64_t>((size_t)nn);
    if (bytes) *bytes = cv.bytes();
    return s;
}

size_t seeded_workspace(int64_t n, int64_t d) {
    size_t b = 0;
    carve_sd(nullptr, n, d, &b);
    return b;
}

static int sd_offsets(const SdWs& ws, int64_t n, int64_t d, hipStream_t st) {
    ProfScope _ps("k_seeded_offsets", st);
    const int64_t C = sd_chunks(d), seg = sd_seg(C), S = (C + seg - 1) / seg;
    const dim3 grid((unsigned)((S + 3) / 4), (unsigned)((n + 63) / 64));
    hipLaunchKernelGGL(k_seeded_segsum, grid, dim3(256), 0, st, ws.cnt, n, C, seg, ws.psum);
    FLC_CHECK_LAUNCH("k_seeded_segsum");
    hipLaunchKernelGGL(k_seeded_offsets, grid, dim3(256), 0, st, ws.cnt, n, C, seg, ws.psum, ws.off);
    FLC_CHECK_LAUNCH("k_seeded_offsets");
    return FLC_OK;
}

int seeded_pack_run(const flc_codec_params* prm, const flc_pattern* pat, const float* x, int64_t d, char* payload, void* wsp,
                    size_t ws_bytes, hipStream_t st) {
    const char* me = "flc_pack_seeded";
    if (pat && pat->d_randk_idx) {
        set_error("%s: given (numpy-stream) indices cannot be redrawn by the server; only device draws have a seeded form", me);
        return FLC_ERR_UNSUPPORTED;
    }
    if ((uintptr_t)payload & 15u) { set_error("%s: payload must be 16-byte aligned", me); return FLC_ERR_ARG; }
    if (d > 0 && (prm->k < 1 || prm->k > d)) { set_error("%s: K outside [1, D]", me); return FLC_ERR_ARG; }
    if (ws_bytes < seeded_workspace(1, d)) { set_error("%s: workspace too small", me); return FLC_ERR_WORKSPACE; }
    const int64_t client = pat ? pat->client0 : 0;
    const uint64_t key = client_key(prm->seed, client);
    const int64_t K = d > 0 ? sd_count(prm, d) : 0, C = sd_chunks(d);
    SdWs ws = carve_sd(wsp, 1, d, nullptr);
    if (d > 0) {
        if (int rc = randk_counts_keyed(prm->seed, client, 1, d, K, ws.cnt, ws.ckey, st)) return rc;
        if (int rc = sd_offsets(ws, 1, d, st)) return rc;
    }
    ProfScope _ps("k_seeded_pack", st);
    const int64_t gx = std::max<int64_t>(1, std::min<int64_t>((C + 4 * SD_CPW - 1) / (4 * SD_CPW), 4096));
    hipLaunchKernelGGL(k_seeded_pack, dim3((unsigned)gx), dim3(256), 0, st, x, d, K, ws.cnt, ws.off, key, prm->randk_scale,
                       payload);
    FLC_CHECK_LAUNCH("k_seeded_pack");
    return FLC_OK;
}

int seeded_unpack_run(const flc_codec_params* prm, const char* payload, int64_t d, float* out, void* wsp, size_t ws_bytes,
                      hipStream_t st) {
    const char* me = "flc_unpack_seeded";
    if (d == 0) return FLC_OK;
    if ((uintptr_t)payload & 15u) { set_error("%s: payload must be 16-byte aligned", me); return FLC_ERR_ARG; }
    if (ws_bytes < seeded_workspace(1, d)) { set_error("%s: workspace too small", me); return FLC_ERR_WORKSPACE; }
    const int64_t K = sd_count(prm, d), C = sd_chunks(d);
    SdWs ws = carve_sd(wsp, 1, d, nullptr);
    if (int rc = randk_counts_from_messages(payload, 0, nullptr, 1, d, K, ws.cnt, ws.ckey, st)) return rc;
    if (int rc = sd_offsets(ws, 1, d, st)) return rc;
    ProfScope _ps("k_seeded_unpack", st);
    const int64_t gx = std::max<int64_t>(1, std::min<int64_t>((C + 3) / 4, 4096));
    hipLaunchKernelGGL(k_seeded_unpack, dim3((unsigned)gx), dim3(256), 0, st, payload, d, K, ws.cnt, ws.off, ws.ckey, out);
    FLC_CHECK_LAUNCH("k_seeded_unpack");
    return FLC_OK;
}

int seeded_unpack_reduce_run(const flc_codec_params* prm, const char* base, int64_t ld, const char* const* ptrs, int64_t n,
                             int64_t d, const float* w, float wt, float* out, void* wsp, size_t ws_bytes, hipStream_t st) {
    const char* me = "flc_unpack_reduce_seeded";
    if (d == 0) return FLC_OK;
    if (n == 0) {
        hipLaunchKernelGGL(k_seeded_zero, dim3((unsigned)std::min<int64_t>((d + 255) / 256, 4096)), dim3(256), 0, st, out, d);
        FLC_CHECK_LAUNCH("k_seeded_zero");
        return FLC_OK;
    }
    if (base && ((ld & 15) || ((uintptr_t)base & 15u))) { set_error("%s: payload rows must be 16-byte aligned", me); return FLC_ERR_ARG; }
    if (ws_bytes < seeded_workspace(n, d)) { set_error("%s: workspace too small", me); return FLC_ERR_WORKSPACE; }
    const int64_t K = sd_count(prm, d), C = sd_chunks(d);
    if (base) ptrs = nullptr;
    SdWs ws = carve_sd(wsp, n, d, nullptr);
    if (int rc = randk_counts_from_messages(base, ld, ptrs, n, d, K, ws.cnt, ws.ckey, st)) return rc;
    if (int rc = sd_offsets(ws, n, d, st)) return rc;
    ProfScope _ps("k_seeded_fold", st);
    // few chunks (short rows): split each chunk's columns over 2 or 4 waves, as k_chunk_accum does
    const int parts = C >= 1024 ? 1 : (C >= 256 ? 2 : 4);
    const int ab = (int)std::max<int64_t>(1, std::min<int64_t>((C * parts + 3) / 4, 16384));
    auto go = [&](auto ts) {
        hipLaunchKernelGGL((k_seeded_fold<decltype(ts)::value>), dim3(ab), dim3(256), 0, st, base, ld, ptrs, n, d, K, ws.cnt,
                           ws.off, ws.ckey, w, wt, out);
    };
    if (parts == 1) go(std::integral_constant<int, CHUNK>{});
    else if (parts == 2) go(std::integral_constant<int, CHUNK / 2>{});
    else go(std::integral_constant<int, CHUNK / 4>{});
    FLC_CHECK_LAUNCH("k_seeded_fold");
    return FLC_OK;
}

// Host check of one seeded message as it comes off the network (flc_payload_validate_seeded)
int seeded_payload_validate(const flc_codec_params* prm, const uint8_t* p, int64_t nbytes, int64_t d, int64_t client) {
    const int64_t pb = seeded_payload_bytes(prm, d);
    if (nbytes < pb) { set_error("payload: %lld bytes, the seeded message of d=%lld is %lld", (long long)nbytes, (long long)d, (long long)pb); return FLC_ERR_ARG; }
    uint32_t h[8];
    std::memcpy(h, p, sizeof h);
    const uint32_t want = d > 0 ? (uint32_t)sd_count(prm, d) : 0u;
    const uint64_t key = sd_join64(h[5], h[4]), md = sd_join64(h[7], h[6]);
    if (h[0] != (uint32_t)FMT_SEEDED) { set_error("payload: header format %u, the seeded message's is %d", h[0], (int)FMT_SEEDED); return FLC_ERR_ARG; }
    if (h[1] != want) { set_error("payload: count %u, the message of K and d carries %u values", h[1], want); return FLC_ERR_ARG; }
    if (h[2] != 0u) { set_error("payload: norm bits %08x in a seeded message (0 expected)", h[2]); return FLC_ERR_ARG; }
    if (h[3] != 0u) { set_error("payload: %u elements flagged unrepresentable by the sender", h[3]); return FLC_ERR_ARG; }
    if (md != (uint64_t)d) { set_error("payload: drawn for d=%llu, not d=%lld", (unsigned long long)md, (long long)d); return FLC_ERR_ARG; }
    if (client >= 0 && key != client_key(prm->seed, client)) {
        set_error("payload: key %016llx is not client %lld's", (unsigned long long)key, (long long)client);
        return FLC_ERR_ARG;
    }
    return FLC_OK;
}

}  // namespace flc
