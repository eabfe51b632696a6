// The chunk-owner fold of the rows' (index, value) lists — TopK candidates, RandK members, unpacked
// wire payloads — and a lone row's list scattered into its dense output.
// Data flow, workspace and switches: select_impl.hpp.
#include "select_impl.hpp"

namespace flc {

// ------------------------------------------------------------------------------------------
// Chunk-owner accumulation.  One wave per chunk, fp32 tile in LDS; rows folded in order.
// ASSIGN (single row, no weights): out = tile with the entry values stored, not added
// (keeps -0.0 like torch's out[ind] = x[ind]).
// ------------------------------------------------------------------------------------------
// Admission per entry: exact-path rows (F_EXACT) hold exactly their admitted entries; fast-path
// rows admit key > thr, and key == thr either all (no F_TIES) or up to the row's tie cut (the
// largest index admitted among the ties, k_cand_select).
//
// One wave owns one chunk: a 4096-float LDS tile into which the rows are folded in row order
// (bit-exact sequential sum; within a row the entries' columns are distinct).  The walk over the
// N rows is a software pipeline: the per-row state (tab entry, thr, cut, mode, weight) of 64 rows
// is fetched one batch ahead with lane = row, and the entry lists of the next AP rows are in
// flight while a row is folded (a ring of AP register slots, 2 x 64 entries per row), so the
// wave never waits on a dependent tab -> entries round trip.
// ------------------------------------------------------------------------------------------
constexpr int AP = FLC_CA_AP;              // rows of entry lists in flight

struct RowMeta {
    uint2 te;          // (offset, count) of the row's list in this chunk
    uint32_t thr, cut, mode;   // cut: tie_pref of the row's tie cut (0 admits every tie)
    float w;
};

__device__ inline RowMeta load_meta(const SelWs& ws, int64_t c, int64_t n, int64_t r, const float* w, int64_t rend = -1) {
    RowMeta m;
    m.te = make_uint2(0, 0);
    m.thr = 0; m.cut = 0u; m.mode = 0; m.w = 1.f;
    if (r < (rend < 0 ? n : rend)) {
        m.te = ws.tab[c * n + r];
        m.thr = ws.thr[r];
        const uint32_t f = ws.flags[r];
        m.mode = (f & F_EXACT) ? 2u : ((f & F_TIES) ? 1u : 0u);
        if (m.mode == 1u) m.cut = tie_pref(ws.tiecut[r], ws.tie_hi);
        if (m.mode == 2u) m.thr = 0u;          // exact list: every entry admitted (key >= 0, cut ~0)
        if (w) m.w = w[r];
    }
    return m;
}


// Sign of zero.  The reference adds every client's DENSE row, so a column a row did not keep
// receives the term w_i * (+0) (-0 when w_i's sign bit is set).  The fold skips those terms and
// starts its tile at -0 (the additive identity), which gives the same bits for every nonzero
// result.  A sum is -0 only if every term was -0: the tile ends at -0 exactly when every KEPT
// term was -0 (or none was kept), and the reference's sum is then -0 iff, in addition, every row
// that did not keep the column has a negative-signed weight.  Those columns are resolved here:
// for each row with a positive-signed weight (stopping once no candidate is left) the -0
// columns it does not keep turn +0.  Untouched columns die at the first such row, so this costs
// one extra list walk for chunks that have them and nothing for the others.
template <int TS>
__device__ void resolve_neg_zero(float* tl, uint32_t* rm, const SelWs& ws, int64_t c, int64_t n, uint32_t cbase,
                                 int64_t len, const float* w, int lane) {
    constexpr int NW = TS / 32;                        // mask words (32 columns each)
    constexpr int WL = (NW + 63) / 64;                 // mask words per lane (word k = lane + 64 j)
    bool any = false;
    for (int k = 0; k < TS / 64; ++k) {
        const int64_t i = (int64_t)k * 64 + lane;
        const uint64_t b = __ballot(i < len && __float_as_uint(tl[i]) == 0x80000000u);
        if (lane == 0) { rm[2 * k] = (uint32_t)b; rm[2 * k + 1] = (uint32_t)(b >> 32); }
        any |= b != 0ull;
    }
    if (!any) return;
    uint32_t z0[WL], zc[WL];
#pragma unroll
    for (int j = 0; j < WL; ++j) {
        const int k = lane + 64 * j;
        z0[j] = k < NW ? rm[k] : 0u;
        zc[j] = z0[j];
    }
    for (int64_t r = 0; r < n; ++r) {
        if (w && (__float_as_uint(w[r]) >> 31)) continue;      // its skipped term is -0: no constraint
#pragma unroll
        for (int j = 0; j < WL; ++j) if (lane + 64 * j < NW) rm[lane + 64 * j] = 0u;
        const RowMeta m = load_meta(ws, c, n, r, w);
        const uint32_t mode = m.mode, T = m.thr, cut = m.cut;
        for (uint32_t e = (uint32_t)lane; e < m.te.y; e += 64) {
            const uint32_t ix = ws.ent_idx[r * ws.cap + m.te.x + e];
            const uint32_t key = mag_key(ws.ent_val[r * ws.cap + m.te.x + e]);
            const uint32_t loc = ix - cbase;
            if (loc < (uint32_t)TS && (mode == 2u || key > T || (key == T && tie_pref(ix, ws.tie_hi) >= cut)))
                atomicOr(&rm[loc >> 5], 1u << (loc & 31));
        }
        bool left = false;
#pragma unroll
        for (int j = 0; j < WL; ++j) {
            if (lane + 64 * j < NW) zc[j] &= rm[lane + 64 * j];
            left |= zc[j] != 0u;
        }
        if (__ballot(left) == 0ull) break;
    }
#pragma unroll
    for (int j = 0; j < WL; ++j) {
        uint32_t dead = z0[j] & ~zc[j];
        while (dead) {
            const int b = __builtin_ctz(dead);
            dead &= dead - 1u;
            tl[(lane + 64 * j) * 32 + b] = 0.f;
        }
    }
}

// resolve_neg_zero for one-wave workgroups whose LDS holds only the tile: the -0 column masks
// live in registers (word k of the tile's TS / 32 in lane k % 64), a row's kept columns are OR-ed
// into the job's global scratch `rm` (TS / 32 words) and read back at L2 (atomic reads: no stale
// L1 line).  Same rule, same bits; it runs once per job and usually stops after one row.
template <int TS>
__device__ void resolve_neg_zero_g(float* tl, uint32_t* rm, const SelWs& ws, int64_t c, int64_t n, uint32_t cbase,
                                   int64_t len, const float* w, int lane) {
    constexpr int NW = TS / 32;                        // mask words (32 columns each)
    constexpr int WL = (NW + 63) / 64;                 // mask words per lane (word k = lane + 64 j)
    uint32_t z0[WL], zc[WL];
#pragma unroll
    for (int j = 0; j < WL; ++j) z0[j] = 0u;
    bool any = false;
#pragma unroll 4
    for (int k = 0; k < TS / 64; ++k) {
        const int64_t i = (int64_t)k * 64 + lane;
        const uint64_t b = __ballot(i < len && __float_as_uint(tl[i]) == 0x80000000u);
        const int w0 = 2 * k, w1 = 2 * k + 1;          // words of columns 64 k .. 64 k + 63
#pragma unroll
        for (int j = 0; j < WL; ++j) {
            if (lane == (w0 & 63) && (w0 >> 6) == j) z0[j] = (uint32_t)b;
            if (lane == (w1 & 63) && (w1 >> 6) == j) z0[j] = (uint32_t)(b >> 32);
        }
        any |= b != 0ull;
    }
    if (!any) return;
#pragma unroll
    for (int j = 0; j < WL; ++j) zc[j] = z0[j];
    for (int64_t r = 0; r < n; ++r) {
        if (w && (__float_as_uint(w[r]) >> 31)) continue;      // its skipped term is -0: no constraint
#pragma unroll
        for (int j = 0; j < WL; ++j) if (lane + 64 * j < NW) rm[lane + 64 * j] = 0u;
        __threadfence_block();
        const RowMeta m = load_meta(ws, c, n, r, w);
        const uint32_t mode = m.mode, T = m.thr, cut = m.cut;
        for (uint32_t e = (uint32_t)lane; e < m.te.y; e += 64) {
            const uint32_t ix = ws.ent_idx[r * ws.cap + m.te.x + e];
            const uint32_t key = mag_key(ws.ent_val[r * ws.cap + m.te.x + e]);
            const uint32_t loc = ix - cbase;
            if (loc < (uint32_t)TS && (mode == 2u || key > T || (key == T && tie_pref(ix, ws.tie_hi) >= cut)))
                atomicOr(&rm[loc >> 5], 1u << (loc & 31));
        }
        __threadfence_block();
        bool left = false;
#pragma unroll
        for (int j = 0; j < WL; ++j) {
            if (lane + 64 * j < NW) zc[j] &= atomicOr(&rm[lane + 64 * j], 0u);
            left |= zc[j] != 0u;
        }
        if (__ballot(left) == 0ull) break;
    }
#pragma unroll
    for (int j = 0; j < WL; ++j) {
        uint32_t dead = z0[j] & ~zc[j];
        while (dead) {
            const int b = __builtin_ctz(dead);
            dead &= dead - 1u;
            tl[(lane + 64 * j) * 32 + b] = 0.f;
        }
    }
}

// TS < CHUNK: a wave owns TS columns of a chunk (CHUNK / TS waves read the same lists and each
// folds its part): a smaller LDS tile per wave, so more waves per CU hide the list latency.
// WPB = 1 (whole chunks): one-wave workgroups holding only their 16 KB tile, so ten fit a CU's
// 160 KB and every chunk of a 10 M row (2442) has its wave resident at once — with 4-wave blocks
// (67.5 KB with the masks) two fit a CU, 2048 chunk waves ran and the last 394 formed a second
// round of the same length.
// Row groups: rows [r0, rend) only; `first` starts the tiles at -0, else from ws.part (the previous
// group's tiles); `last` resolves the -0 columns over ALL n rows and writes out = sums / wt, else
// the tiles go back to ws.part.  (r0 = 0, rend = n, first = last = 1: one fold of every row.)
template <bool ASSIGN, int TS, bool W, int WPB, int AP = AP>
__device__ __forceinline__ void chunk_accum_body(int64_t n, int64_t d, SelWs ws, const float* __restrict__ w, float wt,
                                                 float* __restrict__ out, int64_t r0, int64_t rend, int first, int last,
                                                 float (*tile)[TS], uint32_t (*zmask)[WPB == 1 ? 1 : TS / 32]) {
    if (rend < 0) rend = n;
    constexpr int PARTS = CHUNK / TS;
    const int lane = threadIdx.x & 63;
    const int wv = WPB == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t C = nchunks(d);
    float* tl = tile[wv];
    const int64_t nb = (rend - r0 + 63) / 64;          // row batches
    for (int64_t t = (int64_t)blockIdx.x * WPB + wv; t < C * PARTS; t += (int64_t)gridDim.x * WPB) {
        const int64_t c = t / PARTS;
        const uint32_t cbase = (uint32_t)(c * CHUNK + (t % PARTS) * TS);
        // ASSIGN (compressVector: out = zeros, out[kept] = x) stores into +0; the fold adds into -0
        if (FLC_TILE_V4 && !ASSIGN && !first && (int64_t)cbase + TS <= d) {
            // the carried tile with its loads in flight 8 float4 at a time (the loop of load -> LDS
            // write pairs below waits one memory latency per 64 columns: 64 per 4096-column tile)
            const float4* p4 = reinterpret_cast<const float4*>(ws.part + cbase);
#pragma unroll
            for (int k0 = 0; k0 < TS / 256; k0 += 8) {
                float4 v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = k0 + k < TS / 256 ? p4[(k0 + k) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k0 + k < TS / 256) reinterpret_cast<float4*>(tl)[(k0 + k) * 64 + lane] = v[k];
            }
        } else {
            for (int i = lane; i < TS; i += 64)
                tl[i] = ASSIGN ? 0.f : (first || (int64_t)cbase + i >= d ? -0.f : ws.part[cbase + i]);
        }
        RowMeta cur = load_meta(ws, c, n, r0 + lane, w, rend), nxt;
        // ring of AP rows' entries (the first 128 of each list; range-checked buffer loads, lanes
        // past the list end get index ~0 = no column)
        uint32_t ri[AP][2];
        float rv[AP][2];
        auto fetch = [&](const RowMeta& m, int q, int64_t row, int slot) {
            const uint32_t off = __builtin_amdgcn_readlane(m.te.x, q), cnt = __builtin_amdgcn_readlane(m.te.y, q);
            const auto di = list_rsrc(ws.ent_idx + row * ws.cap + off, cnt);
            const auto dv = list_rsrc(ws.ent_val + row * ws.cap + off, cnt);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t e = (uint32_t)lane + 64u * h;
                const uint32_t x = __builtin_amdgcn_raw_buffer_load_b32(di, lane * 4, h * 256, 0);
                ri[slot][h] = e < cnt ? x : 0xFFFFFFFFu;
                rv[slot][h] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(dv, lane * 4, h * 256, 0));
            }
        };
        // admission (key > T, or key == T and tie_pref(ix) >= tie_pref(cut); load_meta folds the
        // exact mode into T = 0, cut 0) as ONE 64-bit compare: (key, tie_pref(ix)) >= (T, cut)
        const uint32_t txm = ws.tie_hi ? 0u : 0xFFFFFFFFu;   // tie_pref(ix) = ix ^ txm
        auto fold = [&](uint32_t ix, float vv, uint32_t T, uint32_t cut, uint32_t mode, float wi) {
            (void)mode;
            const uint32_t loc = ix - cbase;                   // ~0 index / other part: loc >= TS
            const uint64_t a = ((uint64_t)mag_key(vv) << 32) | (uint64_t)(ix ^ txm);
            const uint64_t b = ((uint64_t)T << 32) | (uint64_t)cut;
            if (FLC_CA_PROBE == 1) {                          // cost probe: no tile update
                if (loc < (uint32_t)TS && a >= b && vv == 1.2345f) tl[0] = vv;
                return;
            }
            if (loc < (uint32_t)TS && a >= b) {
                if (ASSIGN) tl[loc] = vv;
                else tl[loc] = W ? tl[loc] + wi * vv : tl[loc] + vv;
            }
        };
#pragma unroll
        for (int q = 0; q < AP; ++q) fetch(cur, q, r0 + q, q);
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t i0 = r0 + b * 64;
            nxt = load_meta(ws, c, n, i0 + 64 + lane, w, rend);   // next batch's state, one batch ahead
            if (__builtin_expect(__ballot(cur.te.y > 128u) == 0ull, 1)) {
                // every list of the batch fits the ring slots: straight-line pipeline
#pragma unroll
                for (int q = 0; q < 64; ++q) {
                    const int slot = q % AP;
                    const uint32_t T = __builtin_amdgcn_readlane(cur.thr, q);
                    const uint32_t cut = __builtin_amdgcn_readlane(cur.cut, q);
                    const uint32_t mode = 0u;
                    const float wi = W ? __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(cur.w), q)) : 1.f;
                    fold(ri[slot][0], rv[slot][0], T, cut, mode, wi);
                    // the second slot holds entries only when the list is longer than 64
                    if (__builtin_amdgcn_readlane(cur.te.y, q) > 64u) fold(ri[slot][1], rv[slot][1], T, cut, mode, wi);
                    if (q + AP < 64) fetch(cur, q + AP, i0 + q + AP, slot);
                    else fetch(nxt, q + AP - 64, i0 + q + AP, slot);   // past n: empty lists
                }
            } else {
                // some list is longer than 128 entries: the same walk with the tails folded in place
                for (int q = 0; q < 64; ++q) {
                    const int slot = q % AP;
                    const uint32_t T = __shfl(cur.thr, q, WAVE), cut = __shfl(cur.cut, q, WAVE);
                    const uint32_t mode = __shfl(cur.mode, q, WAVE), cnt = __shfl(cur.te.y, q, WAVE);
                    const uint32_t off = __shfl(cur.te.x, q, WAVE);
                    const float wi = W ? __shfl(cur.w, q, WAVE) : 1.f;
                    uint32_t i_0 = 0, i_1 = 0;
                    float v_0 = 0.f, v_1 = 0.f;
#pragma unroll
                    for (int z = 0; z < AP; ++z)
                        if (z == slot) { i_0 = ri[z][0]; i_1 = ri[z][1]; v_0 = rv[z][0]; v_1 = rv[z][1]; }
                    fold(i_0, v_0, T, cut, mode, wi);
                    fold(i_1, v_1, T, cut, mode, wi);
                    const int64_t row = i0 + q;
                    for (uint32_t e = 128u + lane; e < cnt; e += 64)
                        fold(ws.ent_idx[row * ws.cap + off + e], ws.ent_val[row * ws.cap + off + e], T, cut, mode, wi);
                    // refill the slot (same contract as the straight-line path)
                    const RowMeta& m = (q + AP < 64) ? cur : nxt;
                    const int qq = (q + AP) & 63;
                    const uint32_t offn = __shfl(m.te.x, qq, WAVE), cntn = __shfl(m.te.y, qq, WAVE);
                    const int64_t rown = i0 + q + AP;
                    uint32_t xi[2];
                    float xv[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const uint32_t e = (uint32_t)lane + 64u * h;
                        xi[h] = e < cntn ? ws.ent_idx[rown * ws.cap + offn + e] : 0xFFFFFFFFu;
                        xv[h] = e < cntn ? ws.ent_val[rown * ws.cap + offn + e] : 0.f;
                    }
#pragma unroll
                    for (int z = 0; z < AP; ++z)
                        if (z == slot) { ri[z][0] = xi[0]; ri[z][1] = xi[1]; rv[z][0] = xv[0]; rv[z][1] = xv[1]; }
                }
            }
            cur = nxt;
        }
        const int64_t len = min((int64_t)TS, d - (int64_t)cbase);
        if (!last) {                                   // row groups: the tiles carry on to the next group
            for (int64_t i = lane; i < len; i += 64) ws.part[cbase + i] = tl[i];
            continue;
        }
        if (!ASSIGN) {
            if (WPB == 1) resolve_neg_zero_g<TS>(tl, ws.zm + t * (TS / 32), ws, c, n, cbase, len, w, lane);
            else resolve_neg_zero<TS>(tl, zmask[wv], ws, c, n, cbase, len, w, lane);
        }
        for (int64_t i = lane; i < len; i += 64) out[cbase + i] = ASSIGN ? tl[i] : tl[i] / wt;
    }
}

template <bool ASSIGN, int TS = CHUNK, bool W = true>
__global__ __launch_bounds__(256) void k_chunk_accum(int64_t n, int64_t d, SelWs ws, const float* __restrict__ w, float wt,
                                                     float* __restrict__ out, int64_t r0 = 0, int64_t rend = -1,
                                                     int first = 1, int last = 1) {
    __shared__ __attribute__((aligned(16))) float tile[4][TS];
    __shared__ uint32_t zmask[4][TS / 32];
    chunk_accum_body<ASSIGN, TS, W, 4>(n, d, ws, w, wt, out, r0, rend, first, last, tile, zmask);
}

// one-wave workgroups holding only their tile (16 KB) and at most FLC_CA_VGPR1 VGPRs: they fit in
// what the TopK filter's waves leave free on a CU (row-group folds under the next group's filter)
// (the tile is dynamic LDS, CHUNK floats given at launch: with a static 16 KB array the compiler
// takes LDS as the occupancy limit and ignores the waves-per-EU request)
template <bool W>
__global__ __launch_bounds__(64) void k_chunk_accum1(
        int64_t n, int64_t d, SelWs ws, const float* __restrict__ w, float wt, float* __restrict__ out, int64_t r0,
        int64_t rend, int first, int last) {
    extern __shared__ __attribute__((aligned(16))) float dyn_tile[];
    chunk_accum_body<false, CHUNK, W, 1, FLC_CA_AP1>(n, d, ws, w, wt, out, r0, rend, first, last,
                                         reinterpret_cast<float (*)[CHUNK]>(dyn_tile), nullptr);
}

// Single-row dense output (compressVector: out = zeros; out[admitted] = x, stored not added, so a
// selected -0.0 stays -0.0 like torch's out[ind] = x[ind]): after a memset, the row's list
// (entries [0, rowcnt), distinct indices) is scattered with the fold's admission rule — no per-chunk
// tile walk for one row.
__global__ __launch_bounds__(256) void k_assign_scatter(SelWs ws, float* __restrict__ out, int sharded) {
    const uint32_t T = ws.thr[0], f = ws.flags[0];
    const uint32_t mode = (f & F_EXACT) ? 2u : ((f & F_TIES) ? 1u : 0u);
    const uint32_t cut = mode == 1u ? tie_pref(ws.tiecut[0], ws.tie_hi) : 0u;
    // the list: [0, rowcnt) (one reservation counter, or rewritten by the exact path), else the
    // filter's CS_SH shards, block b taking shards b, b + gridDim.x, ...
    const bool shd = sharded && mode != 2u;
    const int64_t segcap = (ws.cap / CS_SH) & ~int64_t(3);
    for (int sh = shd ? (int)blockIdx.x : 0; sh < (shd ? CS_SH : 1); sh += shd ? (int)gridDim.x : 1) {
        const uint32_t cnt = shd ? ws.shcnt[sh * RCS] : ws.rowcnt[0];
        const int64_t o = shd ? sh * segcap : 0;
        for (uint32_t e = (shd ? 0u : blockIdx.x * 256u) + threadIdx.x; e < cnt; e += shd ? 256u : gridDim.x * 256u) {
            const uint32_t ix = ws.ent_idx[o + e];
            const float v = ws.ent_val[o + e];
            const uint32_t key = mag_key(v);
            if (mode == 2u || key > T || (key == T && tie_pref(ix, ws.tie_hi) >= cut)) out[ix] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Host launchers
// ------------------------------------------------------------------------------------------
static int accum_parts() {
    static const int p = [] {
        const char* e = tuning_env("FLC_ACCUM_PARTS");   // tuning runs only (0 / unset: by chunk count)
        const int v = e ? atoi(e) : 0;
        return (v == 1 || v == 2 || v == 4) ? v : 0;
    }();
    return p;
}

// TopK row-group fold: rows [r0, r1) into the running tiles (ws.part); beside a filter the
// one-wave workgroups (<= 102 VGPRs, 16 KB of LDS: room is left beside the filter's waves), the
// exposed last group in 4-wave workgroups
int launch_group_fold(int64_t n, int64_t d, SelWs ws, const float* w, float wt, float* out, int64_t r0, int64_t r1,
                      bool first, bool last, bool exposed, hipStream_t st) {
    const int64_t C = host_chunks(d);
    ProfScope _ps("k_chunk_accum", st);
    if (!exposed) {
        const int ab = grid_stride_blocks(C, 16384);
        if (w) hipLaunchKernelGGL((k_chunk_accum1<true>), dim3(ab), dim3(64), CHUNK * sizeof(float), st, n, d, ws, w, wt, out, r0, r1,
                                  first ? 1 : 0, last ? 1 : 0);
        else hipLaunchKernelGGL((k_chunk_accum1<false>), dim3(ab), dim3(64), CHUNK * sizeof(float), st, n, d, ws, w, wt, out, r0, r1,
                                first ? 1 : 0, last ? 1 : 0);
    } else {
        constexpr int LTS = FLC_TK_LAST_TS;
        const int ab = grid_stride_blocks((C * (CHUNK / LTS) + 3) / 4, 4096);
        if (w) hipLaunchKernelGGL((k_chunk_accum<false, LTS, true>), dim3(ab), dim3(256), 0, st, n, d, ws, w, wt, out, r0, r1,
                                  first ? 1 : 0, last ? 1 : 0);
        else hipLaunchKernelGGL((k_chunk_accum<false, LTS, false>), dim3(ab), dim3(256), 0, st, n, d, ws, w, wt, out, r0, r1,
                                first ? 1 : 0, last ? 1 : 0);
    }
    FLC_CHECK_LAUNCH("k_chunk_accum(group)");
    return FLC_OK;
}

// chunk-owner fold of the rows' lists (TopK candidates, RandK members)
int launch_chunk_accum(int64_t n, int64_t d, SelWs ws, bool assign, const float* w, float wt, float* out, hipStream_t st) {
    const int64_t C = host_chunks(d);
    { ProfScope _ps("k_chunk_accum", st);
    // few chunks (short rows: C2's D = 1 M has 245): split each chunk's columns over 2 or 4 waves so
    // the latency-bound row walk runs on more of the chip (many chunks: one wave each, measured best)
    int parts = accum_parts();
    if (parts == 0) parts = C >= 1024 ? 1 : (C >= 256 ? 2 : 4);
    auto go = [&](auto ts, int ab) {
        constexpr int TS = decltype(ts)::value;
        if (assign) hipLaunchKernelGGL((k_chunk_accum<true, TS>), dim3(ab), dim3(256), 0, st, n, d, ws, w, wt, out);
        else if (w) hipLaunchKernelGGL((k_chunk_accum<false, TS, true>), dim3(ab), dim3(256), 0, st, n, d, ws, w, wt, out);
        else hipLaunchKernelGGL((k_chunk_accum<false, TS, false>), dim3(ab), dim3(256), 0, st, n, d, ws, w, wt, out);
    };
    if (parts == 4) go(std::integral_constant<int, CHUNK / 4>{}, grid_stride_blocks((4 * C + 3) / 4, 8192));
    else if (parts == 2) go(std::integral_constant<int, CHUNK / 2>{}, grid_stride_blocks((2 * C + 3) / 4, 8192));
    else if (FLC_CA_WPB1 && !assign) {
        // one-wave workgroups (the tile alone in LDS), one per chunk
        const int ab = grid_stride_blocks(C, 16384);
        if (w) hipLaunchKernelGGL((k_chunk_accum1<true>), dim3(ab), dim3(64), CHUNK * sizeof(float), st, n, d, ws, w, wt, out, (int64_t)0, n, 1, 1);
        else hipLaunchKernelGGL((k_chunk_accum1<false>), dim3(ab), dim3(64), CHUNK * sizeof(float), st, n, d, ws, w, wt, out, (int64_t)0, n, 1, 1);
    } else go(std::integral_constant<int, CHUNK>{}, grid_stride_blocks((C + 3) / 4, 4096));
    }
    FLC_CHECK_LAUNCH("k_chunk_accum");
    return FLC_OK;
}

// the same fold over whole chunks whatever their number (sel_unpack_reduce: lists in index order)
int launch_chunk_accum_whole(int64_t n, int64_t d, SelWs ws, const float* w, float wt, float* out, hipStream_t st) {
    const int ab = grid_stride_blocks((host_chunks(d) + 3) / 4, 4096);
    { ProfScope _ps("k_chunk_accum", st);
    hipLaunchKernelGGL((k_chunk_accum<false>), dim3(ab), dim3(256), 0, st, n, d, ws, w, wt, out); }
    FLC_CHECK_LAUNCH("k_chunk_accum");
    return FLC_OK;
}

// a lone row's list (few: the filter's CS_SH shards) into the zeroed dense output
void launch_assign_scatter(SelWs ws, float* out, bool few, hipStream_t st) {
    const int sb = (int)std::max<int64_t>(1, std::min<int64_t>((ws.cap + 255) / 256, 2048));
    hipLaunchKernelGGL(k_assign_scatter, dim3(sb), dim3(256), 0, st, ws, out, few ? 1 : 0);
}

}  // namespace flc
