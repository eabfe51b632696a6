// RandK: the compat bucketing of given indices (k_randk_coarse / k_randk_fine), the device sampler
// (counts, list-free fold, short-row lists), the lists on their own for the shifted round, and the
// dense single-vector encode.  Data flow, workspace and switches: select_impl.hpp.
#include "select_impl.hpp"

namespace flc {

// ------------------------------------------------------------------------------------------
// RandK compat lists (indices given: the reference's numpy-stream draws)
// ------------------------------------------------------------------------------------------
// Chunk-bucketed RandK lists in two coalesced levels.
//   k_randk_coarse (one workgroup per row): the row's K indices copied once into the row's ent_val region;
//     LDS counts per superchunk (SB buckets of SPC chunks), LDS scan, then each index appended to
//     its superchunk's segment of ent_idx: SB write frontiers per row, which stay in L2.
//   k_randk_fine (one workgroup per (superchunk, row)): counting sort of the segment by chunk with
//     LDS counters (the segment is copied to ent_val first, scattered back inside the segment),
//     the (offset, count) table entries, then the gather (D/K) * x[j] in ascending chunk order.
constexpr int RK_T = 1024;
constexpr int RK_TILE = 8192;                // indices per LDS multi-split tile (32 KB)

__host__ __device__ inline int64_t rk_spc(int64_t C) { return (C + RK_SB - 1) / RK_SB; }   // chunks per superchunk

template <class Emit>
__device__ inline void randk_walk(const flc_pattern& pat, int64_t row, int64_t K, int64_t ldi, int tid, Emit emit) {
    for (int64_t t = tid; t < K; t += RK_T) emit(t, (uint32_t)pat.d_randk_idx[row * ldi + t]);
}

// FINAL (one chunk per superchunk, C <= RK_SB): the superchunks are the chunks, so this kernel also
// writes the (offset, count) table and gathers the values; k_randk_fine is skipped.
template <bool FINAL>
__global__ __launch_bounds__(RK_T) void k_randk_coarse(RowSrc rows, int64_t n, int64_t d, int64_t K, flc_pattern pat,
                                                       int64_t ldi, float scale, SelWs ws) {
    __shared__ uint32_t cnt[RK_SB], tcnt[RK_SB], toff[RK_SB], gbase[RK_SB];
    __shared__ uint32_t tile[RK_TILE];
    const int64_t row = blockIdx.x;
    const int64_t C = nchunks(d), spc = rk_spc(C);
    const int tid = threadIdx.x;
    if (tid < RK_SB) cnt[tid] = 0;
    __syncthreads();
    uint32_t* jbuf = reinterpret_cast<uint32_t*>(ws.ent_val + row * ws.cap);
    randk_walk(pat, row, K, ldi, tid, [&](int64_t t, uint32_t j) {
        jbuf[t] = j;
        atomicAdd(&cnt[(j >> CHUNK_SHIFT) / spc], 1u);
    });
    __syncthreads();
    if (tid < 64) {                          // exclusive scan of the RK_SB counts: 4 per lane
        uint32_t v[RK_SB / 64], loc = 0;
#pragma unroll
        for (int q = 0; q < RK_SB / 64; ++q) { v[q] = cnt[tid * (RK_SB / 64) + q]; loc += v[q]; }
        uint32_t incl = loc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, WAVE);
            if (tid >= o) incl += u;
        }
        uint32_t run = incl - loc;
#pragma unroll
        for (int q = 0; q < RK_SB / 64; ++q) {
            const int b = tid * (RK_SB / 64) + q;
            if (FINAL) {
                if (b < C) ws.tab[(int64_t)b * n + row] = make_uint2(run, v[q]);
            } else {
                ws.cursor[row * RK_SB + b] = run;         // segment offsets, read by k_randk_fine
            }
            cnt[b] = run;
            run += v[q];
        }
    }
    __syncthreads();
    // Append to the superchunk segments tile by tile: an LDS counting sort of RK_TILE indices, then
    // each bucket's run of the tile is written contiguously (a scattered 4-B store per index would
    // run at a small fraction of the store rate).  Thread tid only re-reads jbuf slots it wrote.
    uint32_t* oi = ws.ent_idx + row * ws.cap;
    constexpr int Q = RK_TILE / RK_T;
    for (int64_t t0 = 0; t0 < K; t0 += RK_TILE) {
        const int m = (int)min<int64_t>(RK_TILE, K - t0);
        if (tid < RK_SB) tcnt[tid] = 0;
        __syncthreads();
        uint32_t jj[Q], rnk[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int k = tid + q * RK_T;
            if (k < m) {
                jj[q] = jbuf[t0 + k];
                rnk[q] = atomicAdd(&tcnt[(jj[q] >> CHUNK_SHIFT) / spc], 1u);
            }
        }
        __syncthreads();
        if (tid < 64) {
            uint32_t v[RK_SB / 64], loc = 0;
#pragma unroll
            for (int q = 0; q < RK_SB / 64; ++q) { v[q] = tcnt[tid * (RK_SB / 64) + q]; loc += v[q]; }
            uint32_t incl = loc;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t u = __shfl_up(incl, o, WAVE);
                if (tid >= o) incl += u;
            }
            uint32_t run = incl - loc;
#pragma unroll
            for (int q = 0; q < RK_SB / 64; ++q) {
                const int b = tid * (RK_SB / 64) + q;
                toff[b] = run;
                gbase[b] = cnt[b];
                cnt[b] += v[q];
                run += v[q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int k = tid + q * RK_T;
            if (k < m) tile[toff[(jj[q] >> CHUNK_SHIFT) / spc] + rnk[q]] = jj[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int k = tid + q * RK_T;
            if (k < m) {
                const uint32_t j = tile[k];
                const uint32_t b = (j >> CHUNK_SHIFT) / spc;
                oi[gbase[b] + (uint32_t)k - toff[b]] = j;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        ws.thr[row] = 0;
        ws.flags[row] = F_EXACT;
        ws.rowcnt[row * RCS] = (uint32_t)K;
    }
    if (FINAL) {
        __syncthreads();                                  // block-scope visibility of the idx writes
        const float* r = rows.row(row);
        float* val = ws.ent_val + row * ws.cap;
        for (int64_t t = tid; t < K; t += RK_T) val[t] = scale * r[oi[t]];   // (D/K) * x[S] in fp32
    }
}

// Segments up to RK_FT entries (the device sampler's ~K / RK_SB, far above any binomial tail) are
// sorted in LDS and written back, with the values, in one coalesced sweep; a larger segment (an
// arbitrary compat index list) takes the slower in-memory counting sort.
constexpr int RK_FT = 8192, RK_FTHR = 512;
__global__ __launch_bounds__(RK_FTHR) void k_randk_fine(RowSrc rows, int64_t n, int64_t d, int64_t K, float scale,
                                                        SelWs ws) {
    extern __shared__ uint32_t fc[];                       // [spc] counts, then offsets / cursors
    __shared__ uint32_t wsum[RK_FTHR / 64];
    __shared__ uint32_t tile[RK_FT];
    const int64_t row = blockIdx.y, b = blockIdx.x;
    const int64_t C = nchunks(d), spc = rk_spc(C);
    const int64_t cb0 = b * spc, cb1 = min(C, cb0 + spc);
    const int tid = threadIdx.x;
    if (cb0 >= C) return;
    const uint32_t s0 = ws.cursor[row * RK_SB + b];
    const uint32_t s1 = (b + 1 < RK_SB) ? ws.cursor[row * RK_SB + b + 1] : (uint32_t)K;
    const int64_t nc = cb1 - cb0;
    const bool in_lds = s1 - s0 <= (uint32_t)RK_FT;
    for (int64_t c = tid; c < nc; c += RK_FTHR) fc[c] = 0;
    __syncthreads();
    uint32_t* idx = ws.ent_idx + row * ws.cap;
    uint32_t* tmp = reinterpret_cast<uint32_t*>(ws.ent_val + row * ws.cap);
    constexpr int Q = RK_FT / RK_FTHR;
    uint32_t jj[Q], rnk[Q];
    if (in_lds) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const uint32_t t = s0 + tid + q * RK_FTHR;
            if (t < s1) {
                jj[q] = idx[t];
                rnk[q] = atomicAdd(&fc[(jj[q] >> CHUNK_SHIFT) - cb0], 1u);
            }
        }
    } else {
        for (uint32_t t = s0 + tid; t < s1; t += RK_FTHR) {
            const uint32_t j = idx[t];
            tmp[t] = j;
            atomicAdd(&fc[(j >> CHUNK_SHIFT) - cb0], 1u);
        }
    }
    __syncthreads();
    // exclusive scan of nc counters: thread t owns a contiguous block
    const int64_t per = (nc + RK_FTHR - 1) / RK_FTHR;
    const int64_t q0 = min<int64_t>(nc, tid * per), q1 = min<int64_t>(nc, q0 + per);
    uint32_t loc = 0;
    for (int64_t c = q0; c < q1; ++c) loc += fc[c];
    uint32_t incl = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o, WAVE);
        if ((tid & 63) >= o) incl += u;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    uint32_t run = incl - loc;
    for (int w = 0; w < (tid >> 6); ++w) run += wsum[w];
    for (int64_t c = q0; c < q1; ++c) {
        const uint32_t v = fc[c];
        ws.tab[(cb0 + c) * n + row] = make_uint2(s0 + run, v);
        fc[c] = run;                                        // segment-relative offset
        run += v;
    }
    __syncthreads();
    const float* r = rows.row(row);
    float* val = ws.ent_val + row * ws.cap;
    if (in_lds) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const uint32_t t = s0 + tid + q * RK_FTHR;
            if (t < s1) tile[fc[(jj[q] >> CHUNK_SHIFT) - cb0] + rnk[q]] = jj[q];
        }
        __syncthreads();
        for (uint32_t k = tid; k < s1 - s0; k += RK_FTHR) {
            const uint32_t j = tile[k];
            idx[s0 + k] = j;
            val[s0 + k] = scale * r[j];                     // (D/K) * x[S] in fp32, ascending columns
        }
        return;
    }
    for (uint32_t t = s0 + tid; t < s1; t += RK_FTHR) {
        const uint32_t j = tmp[t];
        idx[s0 + atomicAdd(&fc[(j >> CHUNK_SHIFT) - cb0], 1u)] = j;
    }
    __syncthreads();                                        // block-scope visibility of the idx writes
    for (uint32_t t = s0 + tid; t < s1; t += RK_FTHR) val[t] = scale * r[idx[t]];
}

// ------------------------------------------------------------------------------------------
// RandK device mode (randk_tree.hpp): no index lists.
//   k_randk_counts : one workgroup per row walks the hypergeometric tree level by level (ping-pong
//                    level arrays in the workspace) -> cnt[c][row] = the row's members in chunk c,
//                    and the row's client key
//   k_randk_fold   : one wave per chunk (or 1/2, 1/4 of its columns when the rows are short) folds
//                    the rows in order into an fp32 LDS tile: row q's members of the chunk are the
//                    first cnt[c][q] images of the chunk permutation (lane t -> offset P(t)), their
//                    values (D/K) * x_q[j] gathered with range-checked buffer loads (AP rows in
//                    flight), added as w_q * v — the sequential fold of the dense compressVector
//                    outputs, bit for bit (a row's members are distinct)
// ------------------------------------------------------------------------------------------
// Chunk counts of the device sampler (randk_tree.hpp): each workgroup takes one row and a range of
// RKC_BINS chunks, evaluates Pi(t) for all t < K with a persistent cycle walk (every lane does
// useful work each trip) and histograms the chunk ids in LDS (16-bit bins: a chunk holds <= 4096).
constexpr int RKC_NT = 1024;
constexpr int64_t RKC_BINS = 32768;

// the client keys of the device sampler (k_randk_counts writes them beside the counts)
__global__ __launch_bounds__(256) void k_randk_ckeys(int64_t n, uint64_t seed, int64_t client0, uint64_t* __restrict__ ckey) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row < n) ckey[row] = client_key(seed, client0 + row);
}

// M (the sampled sparse round): row `row` is the participant, its key the client's (client0 + ids[row])
template <class M = MapNone>
__global__ __launch_bounds__(RKC_NT) void k_randk_counts(int64_t n, int64_t d, int64_t K, uint64_t seed, int64_t client0,
                                                         RkdWs ws, M map) {
    __shared__ uint32_t bins[RKC_BINS / 2];
    const int64_t row = blockIdx.y;
    const int tid = threadIdx.x;
    const int64_t C = nchunks(d);
    const int64_t c0 = (int64_t)blockIdx.x * RKC_BINS, nc = min(C, c0 + RKC_BINS) - c0;
    const uint64_t ck = client_key(seed, client0 + (M::ON ? map.id_s(row) : row));
    for (int64_t i = tid; i < (nc + 1) / 2; i += RKC_NT) bins[i] = 0;
    __syncthreads();
    const rktree::RowPerm P(ck, (uint64_t)d);
    int64_t t = tid;
    bool live = t < K;
    uint64_t x = (uint64_t)t;
    while (__ballot(live) != 0ull) {
        const uint64_t v = P.once(x);
        if (live) {
            if (v < (uint64_t)d) {
                const int64_t c = (int64_t)(v >> CHUNK_SHIFT) - c0;
                if ((uint64_t)c < (uint64_t)nc) atomicAdd(&bins[c >> 1], 1u << (16 * (c & 1)));
                t += RKC_NT;
                live = t < K;
                x = (uint64_t)t;
            } else {
                x = v;
            }
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) ws.ckey[row] = ck;
    for (int64_t c = tid; c < nc; c += RKC_NT) ws.cnt[(c0 + c) * n + row] = (bins[c >> 1] >> (16 * (c & 1))) & 0xFFFFu;
}

// lists view of the counts (the short-row path): tab[c][row] = (offset, count) with the members
// laid out chunk by chunk, and the F_EXACT row state (every listed entry is kept)
__global__ __launch_bounds__(256) void k_randk_tab(int64_t n, int64_t d, int64_t K, const uint32_t* __restrict__ cnt,
                                                   SelWs ls) {
    __shared__ uint32_t part[256];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t C = nchunks(d), per = (C + 255) / 256;
    const int64_t c0 = min(C, tid * per), c1 = min(C, c0 + per);
    uint32_t loc = 0;
    for (int64_t c = c0; c < c1; ++c) loc += cnt[c * n + row];
    part[tid] = loc;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t v = tid >= off ? part[tid - off] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - loc;
    for (int64_t c = c0; c < c1; ++c) {
        const uint32_t m = cnt[c * n + row];
        ls.tab[c * n + row] = make_uint2(run, m);
        run += m;
    }
    if (tid == 0) {
        ls.thr[row] = 0;
        ls.flags[row] = F_EXACT;
        ls.rowcnt[row * RCS] = (uint32_t)K;
    }
}

// Row-major member generation + gather: each wave takes RKG_CPW consecutive chunks of one row,
// lane t < m_c writes member t of chunk c (its global index and (D/K) x[j]) at the row's list
// position tab[c][row].x + t — the lists k_chunk_accum folds.  The gathers of a wave stay inside one
// row's 16 KB windows, chunk after chunk (page- and DRAM-row-local, like the compat path's
// k_randk_fine); the RKG_CPW chunks' loads are issued before any store.
constexpr int RKG_CPW = 4;
__global__ __launch_bounds__(256) void k_randk_gen(RowSrc rows, int64_t n, int64_t d, const uint64_t* __restrict__ ckey,
                                                   float scale, SelWs ws) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t C = nchunks(d);
    for (int64_t row = blockIdx.y; row < n; row += gridDim.y) {
        const uint64_t k = ckey[row];
        const float* r = rows.row_s(row);
        uint32_t* oi = ws.ent_idx + row * ws.cap;
        float* ov = ws.ent_val + row * ws.cap;
        for (int64_t c0 = ((int64_t)blockIdx.x * 4 + wv) * RKG_CPW; c0 < C; c0 += (int64_t)gridDim.x * 4 * RKG_CPW) {
            uint2 te[RKG_CPW];
            uint32_t col[RKG_CPW];
            float v[RKG_CPW];
#pragma unroll
            for (int q = 0; q < RKG_CPW; ++q) {
                const int64_t c = c0 + q;
                te[q] = c < C ? ws.tab[c * n + row] : make_uint2(0u, 0u);
                const uint32_t clen = (uint32_t)min((int64_t)CHUNK, d - c * CHUNK);
                const rktree::ChunkPerm P(k, c, clen);
                col[q] = (uint32_t)lane < te[q].y ? P((uint32_t)lane) : 0u;
                v[q] = (uint32_t)lane < te[q].y ? r[c * CHUNK + col[q]] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < RKG_CPW; ++q) {
                const int64_t c = c0 + q;
                if ((uint32_t)lane < te[q].y) {
                    oi[te[q].x + lane] = (uint32_t)(c * CHUNK + col[q]);
                    ov[te[q].x + lane] = scale * v[q];
                }
                if (te[q].y > 64u) {                      // a chunk with more than 64 members
                    const uint32_t clen = (uint32_t)min((int64_t)CHUNK, d - c * CHUNK);
                    const rktree::ChunkPerm P(k, c, clen);
                    for (uint32_t t = 64u + lane; t < te[q].y; t += 64) {
                        const uint32_t cc = P(t);
                        oi[te[q].x + t] = (uint32_t)(c * CHUNK + cc);
                        ov[te[q].x + t] = scale * r[c * CHUNK + cc];
                    }
                }
            }
        }
    }
}

__device__ inline uint64_t join64(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | (uint64_t)lo; }

struct RkMeta {            // lane = row of a 64-row batch
    uint32_t m;            // members of this chunk
    uint32_t klo, khi;     // client key
    uint32_t plo, phi;     // row pointer
    float w;
};

__device__ inline RkMeta rk_meta(RowSrc rows, const uint32_t* cnt, const uint64_t* ckey, const float* w, int64_t c,
                                 int64_t n, int64_t r, uint32_t clen) {
    RkMeta m{0u, 0u, 0u, 0u, 0u, 1.f};
    if (r < n) {
        m.m = min(cnt[c * n + r], clen);                 // <= clen by construction; never index past it
        const uint64_t k = ckey[r];
        m.klo = (uint32_t)k;
        m.khi = (uint32_t)(k >> 32);
        const uintptr_t p = (uintptr_t)rows.row(r);
        m.plo = (uint32_t)p;
        m.phi = (uint32_t)((uint64_t)p >> 32);
        if (w) m.w = w[r];
    }
    return m;
}

// (rk_resolve_neg_zero, the -0 column rule after the fold: randk_tree.hpp, shared with randk_shift.hip)

constexpr int RK_AP = FLC_RK_AP;
template <int TS>
__global__ __launch_bounds__(256) void k_randk_fold(RowSrc rows, int64_t n, int64_t d, const uint32_t* __restrict__ cnt,
                                                    const uint64_t* __restrict__ ckey, float scale,
                                                    const float* __restrict__ w, float wt, float* __restrict__ out) {
    constexpr int PARTS = CHUNK / TS;
    constexpr uint32_t NOCOL = 0xFFFFu;                    // past the chunk: the buffer load returns 0
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
        constexpr int AP = RK_AP;                             // rows in flight (their gathers)
        uint32_t ro[AP];                                      // ring: part-local column (>= TS: none)
        float rv[AP];                                         //       gathered x
        // row q of the current batch: its members' columns for this lane, one gather in flight
        auto fetch = [&](const RkMeta& mt, int q, int slot) {
            const uint32_t m = __builtin_amdgcn_readlane(mt.m, q);
            // readlane returns int: widen through uint32_t (a sign-extended low word would set the high one)
            const uint64_t k = join64((uint32_t)__builtin_amdgcn_readlane(mt.khi, q), (uint32_t)__builtin_amdgcn_readlane(mt.klo, q));
            const float* rp = (const float*)join64((uint32_t)__builtin_amdgcn_readlane(mt.phi, q),
                                                   (uint32_t)__builtin_amdgcn_readlane(mt.plo, q));
            const rktree::ChunkPerm P(k, c, clen);
            uint32_t col = (uint32_t)lane < m ? P((uint32_t)lane) : NOCOL;
            if (PARTS > 1 && col - pbase >= (uint32_t)TS) col = NOCOL;   // another wave's part: no gather
            const auto rs = chunk_rsrc(rp ? rp : rows.base, cbase, d);
            ro[slot] = col - pbase;
            rv[slot] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(col * 4u), 0, 0));
        };
        auto fold = [&](int slot, float wi) {
            const uint32_t loc = ro[slot];
            if (loc < (uint32_t)TS) tl[loc] = tl[loc] + wi * (scale * rv[slot]);
        };
        RkMeta cur = rk_meta(rows, cnt, ckey, w, c, n, lane, clen), nxt;
#pragma unroll
        for (int q = 0; q < AP; ++q) fetch(cur, q, q);
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t i0 = b * 64;
            nxt = rk_meta(rows, cnt, ckey, w, c, n, i0 + 64 + lane, clen);
            if (__builtin_expect(__ballot(cur.m > 64u) == 0ull, 1)) {
#pragma unroll
                for (int q = 0; q < 64; ++q) {
                    const int slot = q % AP;
                    fold(slot, __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(cur.w), q)));
                    if (q + AP < 64) fetch(cur, q + AP, slot);
                    else fetch(nxt, q + AP - 64, slot);
                }
            } else {
                // a row with more than 64 members here: the same walk with its tail folded in place
                for (int q = 0; q < 64; ++q) {
                    const int slot = q % AP;
                    const float wi = __shfl(cur.w, q, WAVE);
                    uint32_t lo = NOCOL;
                    float vv = 0.f;
#pragma unroll
                    for (int z = 0; z < AP; ++z)
                        if (z == slot) { lo = ro[z]; vv = rv[z]; }
                    if (lo < (uint32_t)TS) tl[lo] = tl[lo] + wi * (scale * vv);
                    const uint32_t m = __shfl(cur.m, q, WAVE);
                    if (m > 64u) {
                        const int64_t row = i0 + q;
                        const rktree::ChunkPerm P(ckey[row], c, clen);
                        const float* rp = rows.row(row);
                        for (uint32_t e = 64u + lane; e < m; e += 64) {
                            const uint32_t col = P(e), l2 = col - pbase;
                            if (l2 < (uint32_t)TS) tl[l2] = tl[l2] + wi * (scale * rp[cbase + col]);
                        }
                    }
                    // refill the slot (same contract as the straight-line path)
                    const RkMeta& mt = (q + AP < 64) ? cur : nxt;
                    const int qq = (q + AP) & 63;
                    const uint32_t mn = __shfl(mt.m, qq, WAVE);
                    const uint64_t kn = join64((uint32_t)__shfl(mt.khi, qq, WAVE), (uint32_t)__shfl(mt.klo, qq, WAVE));
                    const float* rpn = (const float*)join64((uint32_t)__shfl(mt.phi, qq, WAVE), (uint32_t)__shfl(mt.plo, qq, WAVE));
                    const rktree::ChunkPerm Pn(kn, c, clen);
                    const uint32_t col = (uint32_t)lane < mn ? Pn((uint32_t)lane) : NOCOL;
                    const float xv = col < clen ? rpn[cbase + col] : 0.f;
#pragma unroll
                    for (int z = 0; z < AP; ++z)
                        if (z == slot) { ro[z] = col - pbase; rv[z] = xv; }
                }
            }
            cur = nxt;
        }
        const int64_t len = min((int64_t)TS, (int64_t)clen - (int64_t)pbase);
        rk_resolve_neg_zero<TS>(tl, zmask[wv], cnt, ckey, c, n, pbase, clen, len, w, lane);
        for (int64_t i = lane; i < len; i += 64) out[cbase + pbase + i] = tl[i] / wt;
    }
}

// Single row (compressVector): out = 0, then each wave writes the members of its chunks
__global__ __launch_bounds__(256) void k_randk_scatter_dev(const float* __restrict__ x, int64_t d, const uint32_t* cnt,
                                                           const uint64_t* ckey, float scale, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t C = nchunks(d);
    const uint64_t k = ckey[0];
    for (int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) / 64; c < C; c += (int64_t)gridDim.x * 4) {
        const int64_t cbase = c * CHUNK;
        const uint32_t clen = (uint32_t)min((int64_t)CHUNK, d - cbase);
        const rktree::ChunkPerm P(k, c, clen);
        const uint32_t m = min(cnt[c], clen);
        for (uint32_t t = (uint32_t)lane; t < m; t += 64) {
            const int64_t j = cbase + P(t);
            out[j] = scale * x[j];
        }
    }
}

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
static RkdWs carve_rkd(void* base, int64_t n, int64_t d, size_t* bytes) {
    Carver cv(base);
    const int64_t C = std::max<int64_t>(host_chunks(d), 1), nn = std::max<int64_t>(n, 1);
    RkdWs s;
    s.cnt = cv.take<uint32_t>((size_t)C * nn);
    s.ckey = cv.take<uint64_t>((size_t)nn);
    if (bytes) *bytes = cv.bytes();
    return s;
}

size_t randk_device_workspace(int64_t n, int64_t d) {
    size_t b = 0;
    carve_rkd(nullptr, n, d, &b);
    return b;
}

static int randk_counts(const flc_codec_params* prm, const flc_pattern* pat, int64_t n, int64_t d, RkdWs ws,
                        hipStream_t st, const flc_row_map* map = nullptr) {
    ProfScope _ps("k_randk_counts", st);
    const int64_t parts = (host_chunks(d) + RKC_BINS - 1) / RKC_BINS;
    if (map) hipLaunchKernelGGL(k_randk_counts<MapIds>, dim3((unsigned)parts, (unsigned)n), dim3(RKC_NT), 0, st, n, d, prm->k,
                                prm->seed, pat ? pat->client0 : (int64_t)0, ws, map_ids(map));
    else hipLaunchKernelGGL(k_randk_counts<MapNone>, dim3((unsigned)parts, (unsigned)n), dim3(RKC_NT), 0, st, n, d, prm->k, prm->seed,
                       pat ? pat->client0 : (int64_t)0, ws, MapNone{});
    FLC_CHECK_LAUNCH("k_randk_counts");
    return FLC_OK;
}

// chunk counts of a fold: the caller's (flc_pattern.d_randk_counts, made by flc_device_randk_counts) or
// computed into ws; the client keys are cheap and always computed here
static int randk_counts_or_given(const flc_codec_params* prm, const flc_pattern* pat, int64_t n, int64_t d, RkdWs* rw,
                                 hipStream_t st) {
    if (pat && pat->d_randk_counts) {
        rw->cnt = const_cast<uint32_t*>(pat->d_randk_counts);          // read only by the folds
        hipLaunchKernelGGL(k_randk_ckeys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, prm->seed,
                           pat->client0, rw->ckey);
        FLC_CHECK_LAUNCH("k_randk_ckeys");
        return FLC_OK;
    }
    return randk_counts(prm, pat, n, d, *rw, st);
}

// the same for randk_shift.hip: wsp holds randk_device_workspace(n, d) bytes
int randk_device_prepare(const flc_codec_params* prm, const flc_pattern* pat, int64_t n, int64_t d, void* wsp,
                         const uint32_t** cnt, const uint64_t** ckey, hipStream_t st, const flc_row_map* map) {
    RkdWs rw = carve_rkd(wsp, n, d, nullptr);
    // a sampled round: counts and keys by client id, always computed (given counts are refused before)
    if (int rc = map ? randk_counts(prm, pat, n, d, rw, st, map) : randk_counts_or_given(prm, pat, n, d, &rw, st)) return rc;
    *cnt = rw.cnt;
    *ckey = rw.ckey;
    return FLC_OK;
}

// the device sampler's chunk counts of n clients (flc_device_randk_counts: the sampler's test hook)
int randk_device_counts(uint64_t seed, int64_t client0, int64_t n, int64_t d, int64_t k, uint32_t* cnt, void* wsp,
                        size_t ws_bytes, hipStream_t st) {
    if (ws_bytes < randk_device_workspace(n, d)) { set_error("randk counts: workspace too small"); return FLC_ERR_WORKSPACE; }
    RkdWs ws = carve_rkd(wsp, n, d, nullptr);
    ws.cnt = cnt;                                    // the counts straight into the caller's array
    flc_codec_params prm{};
    prm.codec = FLC_RANDK;
    prm.k = k;
    prm.seed = seed;
    flc_pattern pat{};
    pat.client0 = client0;
    return randk_counts(&prm, &pat, n, d, ws, st);
}

// device-RNG RandK encode + reduce: counts, then the list-free chunk fold
int randk_device_run(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, int64_t n, int64_t d,
                     const float* w, float wt, float* out, void* wsp, size_t ws_bytes, hipStream_t st) {
    size_t lb = 0;
    carve_sel(nullptr, FLC_RANDK, n, d, prm->k, &lb);
    if (ws_bytes < lb + randk_device_workspace(n, d)) { set_error("randk: workspace too small"); return FLC_ERR_WORKSPACE; }
    SelWs sw = carve_sel(wsp, FLC_RANDK, n, d, prm->k, nullptr);
    RkdWs rw = carve_rkd(static_cast<char*>(wsp) + lb, n, d, nullptr);
    const int64_t C = host_chunks(d);
    // Long rows (>= 1024 chunks, one wave per chunk fills the chip): the list-free chunk fold, each
    // wave regenerating the rows' members of its chunk.  Short rows: too few chunks for the
    // row-serial fold, so the members are written per row (k_randk_gen) and the chunk fold runs
    // over the lists with its column split (k_chunk_accum).
    // chunk counts: the caller's (flc_pattern.d_randk_counts, made by flc_device_randk_counts) or
    // computed here; the client keys are cheap and always computed here
    auto counts = [&]() -> int { return randk_counts_or_given(prm, pat, n, d, &rw, st); };
    if (C >= 1024) {
        if (int rc = counts()) return rc;
        ProfScope _ps("k_randk_fold", st);
        const int ab = grid_stride_blocks((C + 3) / 4, 16384);
        hipLaunchKernelGGL((k_randk_fold<CHUNK>), dim3(ab), dim3(256), 0, st, rows, n, d, rw.cnt, rw.ckey,
                           prm->randk_scale, w, wt, out);
        FLC_CHECK_LAUNCH("k_randk_fold");
        return FLC_OK;
    }
    if (int rc = counts()) return rc;
    hipLaunchKernelGGL(k_randk_tab, dim3((unsigned)n), dim3(256), 0, st, n, d, prm->k, rw.cnt, sw);
    FLC_CHECK_LAUNCH("k_randk_tab");
    {
        ProfScope _ps("k_randk_gen", st);
        const int64_t gx = std::max<int64_t>(1, std::min<int64_t>((C + 4 * RKG_CPW - 1) / (4 * RKG_CPW), 4096));
        hipLaunchKernelGGL(k_randk_gen, dim3((unsigned)gx, (unsigned)std::min<int64_t>(n, 65535)), dim3(256), 0, st, rows,
                           n, d, rw.ckey, prm->randk_scale, sw);
        FLC_CHECK_LAUNCH("k_randk_gen");
    }
    return launch_chunk_accum(n, d, sw, false, w, wt, out, st);
}

// The compat RandK lists on their own (randk_shift.hip: the sparse shifted round rewrites the entry
// values between the bucketing and the fold).  build: k_randk_coarse / k_randk_fine over `rows`
// exactly as sel_run launches them; fold: k_chunk_accum over the lists as they then stand.
size_t randk_lists_workspace(int64_t n, int64_t d, int64_t K) {
    size_t b = 0;
    carve_sel(nullptr, FLC_RANDK, n, d, K, &b);
    return b;
}

int randk_lists_launch(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, int64_t n, int64_t d, SelWs ws,
                       hipStream_t st) {
    const int64_t K = prm->k, C = host_chunks(d);
    const int64_t ldi = pat->idx_ld ? pat->idx_ld : K;
    const int64_t spc = rk_spc(C), sb = (C + spc - 1) / spc;
    { ProfScope _ps("k_randk_coarse", st);
    if (spc == 1)
        hipLaunchKernelGGL(k_randk_coarse<true>, dim3((unsigned)n), dim3(RK_T), 0, st, rows, n, d, K, *pat, ldi,
                           prm->randk_scale, ws);
    else
        hipLaunchKernelGGL(k_randk_coarse<false>, dim3((unsigned)n), dim3(RK_T), 0, st, rows, n, d, K, *pat, ldi,
                           prm->randk_scale, ws); }
    FLC_CHECK_LAUNCH("k_randk_coarse");
    if (spc > 1) {
        ProfScope _ps("k_randk_fine", st);
        hipLaunchKernelGGL(k_randk_fine, dim3((unsigned)sb, (unsigned)n), dim3(RK_FTHR), (size_t)spc * sizeof(uint32_t),
                           st, rows, n, d, K, prm->randk_scale, ws);
        FLC_CHECK_LAUNCH("k_randk_fine");
    }
    return FLC_OK;
}

int randk_lists_build(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, int64_t n, int64_t d, void* wsp,
                      RkLists* lists, hipStream_t st) {
    SelWs ws = carve_sel(wsp, FLC_RANDK, n, d, prm->k, nullptr);
    lists->tab = ws.tab;
    lists->idx = ws.ent_idx;
    lists->val = ws.ent_val;
    lists->cap = ws.cap;
    return randk_lists_launch(prm, pat, rows, n, d, ws, st);
}

int randk_lists_fold(int64_t n, int64_t d, int64_t K, void* wsp, const float* w, float wt, float* out, hipStream_t st) {
    return launch_chunk_accum(n, d, carve_sel(wsp, FLC_RANDK, n, d, K, nullptr), false, w, wt, out, st);
}

// Dense single-vector RandK: out = 0; out[S] = scale * x[S]  (compressors.py:242-243)
__global__ __launch_bounds__(256) void k_randk_dense(const float* __restrict__ x, int64_t K, const int64_t* __restrict__ idx,
                                                     float scale, float* __restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < K; t += (int64_t)gridDim.x * 256) {
        const int64_t j = idx[t];
        out[j] = scale * x[j];
    }
}

int randk_dense(const flc_codec_params* prm, const flc_pattern* pat, const float* x, int64_t d, float* out,
                void* wsp, size_t ws_bytes, hipStream_t st) {
    if (d == 0) return FLC_OK;
    if (prm->k < 1 || prm->k > d) { set_error("randk: K outside [1, D]"); return FLC_ERR_ARG; }
    FLC_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)d * sizeof(float), st));
    if (pat && pat->d_randk_idx) {
        int g = (int)std::max<int64_t>(1, std::min<int64_t>((prm->k + 255) / 256, 1024));
        hipLaunchKernelGGL(k_randk_dense, dim3(g), dim3(256), 0, st, x, prm->k, pat->d_randk_idx, prm->randk_scale, out);
        FLC_CHECK_LAUNCH("k_randk_dense");
        return FLC_OK;
    }
    if (ws_bytes < randk_device_workspace(1, d)) { set_error("randk: workspace too small"); return FLC_ERR_WORKSPACE; }
    RkdWs ws = carve_rkd(wsp, 1, d, nullptr);
    if (int rc = randk_counts(prm, pat, 1, d, ws, st)) return rc;
    const int g = grid_stride_blocks((host_chunks(d) + 3) / 4, 4096);
    hipLaunchKernelGGL(k_randk_scatter_dev, dim3(g), dim3(256), 0, st, x, d, ws.cnt, ws.ckey, prm->randk_scale, out);
    FLC_CHECK_LAUNCH("k_randk_scatter_dev");
    return FLC_OK;
}

}  // namespace flc
