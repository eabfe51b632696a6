// The selection core's TopK threshold stage: the sample that picks each row's threshold, the filters
// that append a row's candidates (or, on the exact path, its selection) to its list, and their
// launchers.  Data flow, workspace and switches: select_impl.hpp.
#include "select_impl.hpp"

namespace flc {

// ------------------------------------------------------------------------------------------
// TopK: sample threshold (one workgroup per row)
// ------------------------------------------------------------------------------------------
// DUAL (few rows: latency-bound): the two rank searches share their passes over the sample; the
// second histogram costs 8 KB of LDS, which would halve the workgroups per CU of a many-row launch.
template <int NT, bool DUAL>
__global__ __launch_bounds__(NT) void k_topk_sample(RowSrc rows, int64_t n, int64_t d, int64_t K, SelWs ws, int few,
                                                    int64_t r_off) {
    __shared__ uint32_t keys[SMAX];
    __shared__ uint32_t h[HBINS], h2[DUAL ? HBINS : 1];
    __shared__ uint32_t scratch[260], scratch2[DUAL ? 260 : 1];
    const int64_t row = r_off + blockIdx.x;                               // (a launch may take a row range)
    if (row >= n) return;
    const float* r = rows.row(row);
    // sample: the whole row if it fits, else P pieces of 256 contiguous elements spread evenly
    int S;
    if (d <= SMAX) {
        S = (int)d;
        for (int i = threadIdx.x; i < S; i += NT) keys[i] = mag_key(r[i]);
    } else {
        const int P = SMAX / 256;
        S = SMAX;
        // piece p = 256 contiguous elements at p (d - 256) / (P - 1); thread t reads element t of
        // 32 pieces per round trip (a lone row's sample is latency-bound: few trips)
        // NT / 256 groups of threads take interleaved pieces
        constexpr int GR = NT / 256, PU = 32 / GR;
        const int e = threadIdx.x & 255, g0 = threadIdx.x >> 8;
        for (int p0 = 0; p0 < P; p0 += 32) {
            float x[PU];
#pragma unroll
            for (int u = 0; u < PU; ++u) x[u] = r[((int64_t)(p0 + u * GR + g0) * (d - 256)) / (P - 1) + e];
#pragma unroll
            for (int u = 0; u < PU; ++u) keys[(p0 + u * GR + g0) * 256 + e] = mag_key(x[u]);
        }
    }
    // a spread sample (S < d) only bounds the threshold: its keys to 22 bits (two passes, the low 9
    // bits 0: a lower bound, ~6e-5 relative below the key); the whole row (S == d) exactly
    const int NP = S == d ? 3 : 2;
    // rank (from the top) of the sample element whose key is the threshold
    uint32_t rank;
    if (S == d) {
        rank = (uint32_t)K;                                   // exact
    } else {
        double ks = (double)K * (double)S / (double)d;
        double rr = ks + 4.0 * sqrt(ks) + 8.0;
        rank = (uint32_t)min((double)S, ceil(rr));
    }
    // keys of sample ranks ra and rb (from the top) together: three 11/11/9-bit passes over the LDS
    // sample, one histogram while the two prefixes agree (always in the first pass), the two
    // searches side by side
    static_assert(!DUAL || NT >= 512, "hist_find2 takes 512 threads");
    auto rank_key = [&](uint32_t r) {
        uint32_t prefix = 0, krem = r;
        for (int p = 0; p < NP; ++p) {
            for (int i = threadIdx.x; i < HBINS; i += NT) h[i] = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < S; i += NT) {
                uint32_t k = keys[i];
                if (key_in_prefix(k, p, prefix)) atomicAdd(&h[key_bin(k, p)], 1u);
            }
            __syncthreads();
            uint32_t bin, above;
            hist_find(h, krem, bin, above, scratch);
            prefix = (prefix << pass_bits(p)) | bin;
            krem -= above;
            __syncthreads();
        }
        return NP == 3 ? prefix : prefix << 9;
    };
    auto rank_keys = [&](uint32_t ra, uint32_t rb, uint32_t& ka, uint32_t& kb) {
        if constexpr (!DUAL) {
            ka = rank_key(ra);
            kb = rb == ra ? ka : rank_key(rb);
            return;
        }
        uint32_t pa = 0, pb = 0, ma = ra, mb = rb;
        for (int p = 0; p < NP; ++p) {
            const bool same = pa == pb;
            for (int i = threadIdx.x; i < HBINS; i += NT) { h[i] = 0; h2[i] = 0; }
            __syncthreads();
            for (int i = threadIdx.x; i < S; i += NT) {
                const uint32_t k = keys[i];
                if (key_in_prefix(k, p, pa)) atomicAdd(&h[key_bin(k, p)], 1u);
                if (!same && key_in_prefix(k, p, pb)) atomicAdd(&h2[key_bin(k, p)], 1u);
            }
            __syncthreads();
            uint32_t ba, aa, bb, ab;
            hist_find2(h, ma, ba, aa, scratch, same ? h : h2, mb, bb, ab, scratch2);
            pa = (pa << pass_bits(p)) | ba;
            ma -= aa;
            pb = (pb << pass_bits(p)) | bb;
            mb -= ab;
        }
        ka = NP == 3 ? pa : pa << 9;
        kb = NP == 3 ? pb : pb << 9;
    };
    // the threshold key (rank), and the estimate of the K-th key (sample rank ks) that sizes the
    // first digit of k_cand_select
    uint32_t tkey, kest;
    rank_keys(rank, S == d ? rank : (uint32_t)max(1.0, min((double)S, (double)K * (double)S / (double)d)), tkey, kest);
    if (threadIdx.x == 0) {
        ws.thr[row] = (rank >= (uint32_t)S && S != d) ? 0u : tkey;
        ws.prefix[row] = kest;
        ws.flags[row] = 0;
        ws.rowcnt[(row) * RCS] = 0;
        if (few) { ws.cstate[row * CS_ST + 3] = 0; ws.cstate[row * CS_ST + 5] = 0; ws.carrive[row * RCS] = 0; }
    }
    if (few && threadIdx.x < CS_SH) ws.shcnt[(row * CS_SH + threadIdx.x) * RCS] = 0;
    if (few)                                              // the row's global histogram of k_cs_pass
        for (int i = threadIdx.x; i < HBINS; i += NT) ws.hist[row * HBINS + i] = 0;
}

// ------------------------------------------------------------------------------------------
// Filter: append entries with key >= thr (fast path) or the exact selection (exact path).
// One wave per chunk; a workgroup takes 4 chunks of one row; grid-stride over (row, 4-chunk).
// Exact mode (rows on the worklist, F_EXACT): key > thr always; key == thr only while the
// tie rank (tieprefix + rank in index order inside the chunk) < krem.
// ------------------------------------------------------------------------------------------
template <bool EXACT, bool VEC>
__global__ __launch_bounds__(256) void k_topk_filter(RowSrc rows, int64_t n, int64_t d, SelWs ws) {
    const int64_t C = nchunks(d);
    const int64_t bpr = (C + 3) / 4;                   // 4-chunk blocks per row
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nrows = EXACT ? (int64_t)(*ws.nwork) : n;
    const int64_t items = nrows * bpr;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t li = it / bpr;
        const int64_t row = EXACT ? (int64_t)ws.worklist[li] : li;
        const int64_t c = (it % bpr) * 4 + wv;
        if (!EXACT && ws.flags[row]) continue;          // already failed (row-uniform)
        if (c >= C) continue;
        const float* r = rows.row(row);
        const int64_t j0 = c * CHUNK;
        const uint32_t T = ws.thr[row];
        // load the chunk: 16 x float4 per lane, element j0 + (t*64 + lane)*4 + q
        float v[16][4];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int64_t j = j0 + (int64_t)(t * 64 + lane) * 4;
            if (VEC && j + 3 < d) {
                float4 f = *reinterpret_cast<const float4*>(r + j);
                v[t][0] = f.x; v[t][1] = f.y; v[t][2] = f.z; v[t][3] = f.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[t][q] = (j + q < d) ? r[j + q] : 0.f;
            }
        }
        // ties (key == T) admitted: tie ranks [tie_from, tie_need) in index order — the first krem
        // (lowest-index rule) or the last krem of the row's tot (highest-index rule; k_radix_select
        // left tot in tiecut)
        uint32_t tie_base = 0, tie_need = ALL, tie_from = 0;
        if (EXACT) {
            tie_base = ws.tieprefix[c * n + row];
            tie_need = ws.krem[row];
            if (ws.tie_hi) { const uint32_t tot = ws.tiecut[row]; tie_from = tot - tie_need; tie_need = tot; }
        }
        // pass 1: count
        uint32_t cnt = 0;
        uint32_t tie_run = tie_base;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int64_t jb = j0 + (int64_t)(t * 64 + lane) * 4;
            bool gt[4], eq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t k = mag_key(v[t][q]);
                const bool inb = (jb + q) < d;
                gt[q] = inb && (EXACT ? k > T : k >= T);
                eq[q] = inb && EXACT && k == T;
            }
            if (EXACT) {
                uint64_t m[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) m[q] = __ballot(eq[q]);
                const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
                uint32_t before = __popcll(m[0] & lt) + __popcll(m[1] & lt) + __popcll(m[2] & lt) + __popcll(m[3] & lt);
                uint32_t inlane = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (eq[q]) { const uint32_t tr = tie_run + before + inlane; gt[q] = tr >= tie_from && tr < tie_need; }
                    inlane += eq[q] ? 1u : 0u;
                }
                tie_run += __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) cnt += gt[q] ? 1u : 0u;
        }
        cnt = wave_sum(cnt);
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&ws.rowcnt[(row) * RCS], cnt);
        base = __shfl(base, 0, WAVE);
        const bool fits = (int64_t)base + cnt <= ws.cap;
        if (lane == 0) {
            ws.tab[c * n + row] = make_uint2(base, fits ? cnt : 0u);
            if (!fits) atomicOr(&ws.flags[row], F_OVERFLOW);
        }
        if (!fits || cnt == 0) continue;
        // pass 2: write (order inside the chunk is irrelevant to the result)
        uint32_t run = base;
        tie_run = tie_base;
        uint32_t* oi = ws.ent_idx + row * ws.cap;
        float* ov = ws.ent_val + row * ws.cap;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int64_t jb = j0 + (int64_t)(t * 64 + lane) * 4;
            bool gt[4], eq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t k = mag_key(v[t][q]);
                const bool inb = (jb + q) < d;
                gt[q] = inb && (EXACT ? k > T : k >= T);
                eq[q] = inb && EXACT && k == T;
            }
            if (EXACT) {
                uint64_t m[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) m[q] = __ballot(eq[q]);
                const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
                uint32_t before = __popcll(m[0] & lt) + __popcll(m[1] & lt) + __popcll(m[2] & lt) + __popcll(m[3] & lt);
                uint32_t inlane = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (eq[q]) { const uint32_t tr = tie_run + before + inlane; gt[q] = tr >= tie_from && tr < tie_need; }
                    inlane += eq[q] ? 1u : 0u;
                }
                tie_run += __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t m = __ballot(gt[q]);
                if (gt[q]) {
                    const uint32_t pos = run + (uint32_t)__popcll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
                    oi[pos] = (uint32_t)(jb + q);
                    ov[pos] = v[t][q];
                }
                run += (uint32_t)__popcll(m);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// Fast-path filter.  A work item is a group of GS consecutive 4096-element chunks of one row; waves
// walk items grid-stride.  Every chunk streams in through a RING-deep buffer-load pipeline that
// runs across chunk and item boundaries; entries with key >= T_lo are compacted (ballot / mbcnt)
// into a wave-private LDS staging buffer.  One atomic per group reserves the row-buffer space; its
// return is consumed only after the NEXT group has been compacted (double-buffered staging), when
// the group's entries are copied out coalesced and its GS tab entries are written.
//
// Why groups: on gfx950 vmcnt retires in order, so every atomic / store sits in front of the loads
// issued after it.  Per-chunk reservations (one atomic + a short copy-out per 4096 elements) cost
// ~20 % of the filter's bandwidth (tools/probe_filter.hip); a group of 4 amortises them 4x and the
// copy-out stores become full 256 B wave writes.
// ------------------------------------------------------------------------------------------

// Copy-out of one 4-chunk group's staged entries (tot of them, indices at si, values at sv) to
// position pos of row's list, as 16-B stores of 4 entries a lane (the group's whole quads) plus the
// last partial quad's entries as 4-B stores: a FIXED sequence of 2 GCAP / 256 + 2 range-checked
// buffer stores (none written when the group did not fit) instead of 2 GCAP / 64 exec-masked 4-B
// stores.  The list position is any dword: the 16-B stores need only dword alignment.
// wslot: the calling wave's number in the grid (FLC_TK_PROBE 4 only).  POL: the stores' cache policy.
template <int POL = FLC_TK_STPOL>
__device__ inline void tk_copy_out(const uint32_t* si, const uint32_t* sv, const SelWs& ws, int64_t n, int64_t row,
                                   uint32_t pos, uint32_t tot, bool fits, int lane, int64_t wslot) {
    int64_t at = row * ws.cap + pos;
    if (FLC_TK_PROBE == 4) at = (wslot % max((n * ws.cap) >> 10, (int64_t)1)) << 10;   // 4 KB per wave and array, rewritten in place
    const uint32_t nrec = (fits && FLC_TK_PROBE != 2) ? tot * 4u : 0u;
    const auto di = __builtin_amdgcn_make_buffer_rsrc(ws.ent_idx + at, (short)0, (int)nrec, 0x00020000);
    const auto dv = __builtin_amdgcn_make_buffer_rsrc(ws.ent_val + at, (short)0, (int)nrec, 0x00020000);
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    const uint32_t nq = min(tot, (uint32_t)GCAP) >> 2;
#pragma unroll
    for (int k = 0; k < GCAP / 256; ++k) {
        const uint32_t q = (uint32_t)(k * 64 + lane);
        const uint4 a = reinterpret_cast<const uint4*>(si)[q];
        const uint4 b = reinterpret_cast<const uint4*>(sv)[q];
        const uint32_t off = q < nq ? q * 16u : 0x7FFFFFF0u;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, a), di, off, 0, POL);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, b), dv, off, 0, POL);
    }
    const uint32_t e = nq * 4u + (uint32_t)(lane & 3);          // the partial quad (range-checked)
    const uint32_t off = lane < 3 ? e * 4u : 0x7FFFFFF0u;
    __builtin_amdgcn_raw_buffer_store_b32(si[e], di, off, 0, POL);
    __builtin_amdgcn_raw_buffer_store_b32(sv[e], dv, off, 0, POL);
}

// A chunk is 16 wave-loads of 1 KB.  RING float4 registers per lane hold a software pipeline RING-1
// loads deep (the next chunk's descriptor is built up front; past the last item it has
// num_records 0 and its loads return zeros without touching memory).
// FGS: chunks per work item (group).
template <int RING, int FGS, int LONE = 0>
// LONE (a lone compressVector row on the list path): every float4 read is also written as zeros to
// zout, the dense output the selected entries are then scattered into (no separate fill of the output).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FLC_TK_WPE))) void k_topk_filter_fast(RowSrc rows, int64_t n, int64_t r0, int64_t rn, int64_t rb, int64_t d, SelWs ws, int shards,
                                                                                                float* __restrict__ zout) {
    static_assert(16 % RING == 0, "ring must divide the 16 loads of a chunk");
    // staging per (buffer, wave): GCAP + 64 indices then GCAP + 64 values (one ds_write2st64_b32
    // per entry; the 64 spare slots take a wave-instruction starting at GCAP, i.e. an overflow)
    constexpr int SROW = GCAP + 64;
    static_assert((SROW * 4) % 256 == 0, "value block offset in 256-byte units");
    __shared__ __attribute__((aligned(16))) uint32_t st[2][4][2 * SROW];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: keeps the item walk in SGPRs
    const int64_t C = nchunks(d);
    const int64_t G = (C + FGS - 1) / FGS;                               // groups per row
    const int64_t items = rn * G;                                        // this launch's rows: [r0, r0 + rn)
    const int64_t stride = (int64_t)gridDim.x * 4;
    int64_t it = (int64_t)blockIdx.x * 4 + wv;
    if (it >= items) return;
    float4 ring[RING];
    // item order: blocks of rb rows, inside a block (group, row) with the row fastest (rb = 1:
    // row-major)
    auto item_at = [&](int64_t t, int64_t& r, int64_t& cc) {
        const int64_t blk = t / (rb * G), rem = t - blk * rb * G;
        const int64_t bn = min(rb, rn - blk * rb);
        const int64_t g = rem / bn;
        r = r0 + blk * rb + (rem - g * bn);
        cc = g * FGS;
    };
    int64_t row, c;                                                      // current row, chunk
    item_at(it, row, c);
    auto rs = chunk_rsrc(rows.row_s(row), c * CHUNK, d);
#pragma unroll
    for (int L = 0; L < RING - 1; ++L) {
        ring[L] = load_q(rs, lane, L);
        __builtin_amdgcn_sched_barrier(0);   // issue in ring order: the loop's static vmcnt waits assume it
    }
    // few rows (shards > 1): group g of a row reserves in shard g % shards of its list (a counter and a
    // region of its own): one counter per row would serialise the reservation atomics of every
    // wave on one address (~90 per microsecond), a lone 10 M row's ~1.2 K of them took longer than
    // its loads
    const int64_t segcap = shards > 1 ? (ws.cap / shards) & ~int64_t(3) : ws.cap;
    // previous group, reservation in flight
    bool pv = false;
    int64_t prow = 0, pc0 = 0, pseg = 0;
    uint64_t pcc = 0;                        // per-chunk counts, 16 bits each
    uint32_t ptot = 0, pres = 0;
    int par = 0;
    auto finish = [&](int pb) {
        uint32_t base = 0;
        bool fits = ptot <= GCAP;
        if (fits && ptot) {
            base = __shfl(pres, 0, WAVE);
            fits = (int64_t)base + ptot <= segcap;
            base += (uint32_t)(pseg * segcap);                           // the shard's region
        }
        if (lane < FGS && pc0 + lane < C) {
            uint32_t off = 0, cc = 0;
#pragma unroll
            for (int u = 0; u < FGS; ++u) {
                const uint32_t cu = (uint32_t)(pcc >> (16 * u)) & 0xFFFFu;
                off += u < lane ? cu : 0u;
                cc = u == lane ? cu : cc;
            }
            ws.tab[(pc0 + lane) * n + prow] = make_uint2(base + off, fits ? cc : 0u);
        }
        if (!fits && lane == 0) atomicOr(&ws.flags[prow], F_OVERFLOW);
#if FLC_TK_COPY4
        tk_copy_out(st[pb][wv], st[pb][wv] + SROW, ws, n, prow, base, ptot, fits, lane, (int64_t)blockIdx.x * 4 + wv);
#else
        if (fits && FLC_TK_PROBE != 2) {
            const uint32_t* si = st[pb][wv];
            const float* sv = reinterpret_cast<const float*>(st[pb][wv] + SROW);
            uint32_t* oi = ws.ent_idx + prow * ws.cap + base;
            float* ov = ws.ent_val + prow * ws.cap + base;
            // fixed trip count (GCAP / 64 predicated slots): the compiler's vmcnt bookkeeping
            // stays exact for the loads in flight behind these stores
#pragma unroll
            for (int k = 0; k < GCAP / 64; ++k) {
                const uint32_t e = (uint32_t)(k * 64 + lane);
                if (e < ptot) { oi[e] = si[e]; ov[e] = sv[e]; }
            }
        }
#endif
    };
    while (it < items) {
        // key >= max(T, 1): the loads past the row end return +0 (key 0), so no per-element range
        // test; a row whose K-th magnitude is 0 (fewer than K nonzeros) comes up short and takes
        // the exact path, which admits zeros
        const uint32_t T = max(sload(ws.thr + row), 1u);
        const int64_t nit = it + stride;
        // LDS byte address of this group's staging (wave-uniform)
        const uint32_t sla = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t*)st[par][wv]);
        uint32_t cnt = 0;                    // entries in this group so far
        uint64_t ccp = 0;
        const int64_t cg0 = c;
        int64_t nrow = row, nc = c;
        // straight-line over the group, no early exit: the chunks of a row's short last group
        // past the row end have empty descriptors (their loads return zeros), so the
        // compiler's vmcnt bookkeeping stays exact from one group's atomic to its use
#pragma unroll
        for (int sub = 0; sub < FGS; ++sub, ++c) {
            const int64_t j0 = c * CHUNK;
            // descriptor of the chunk after this one (same group, else the next item's first)
            __amdgpu_buffer_rsrc_t rsn;
            if (sub + 1 < FGS) {
                rsn = chunk_rsrc(rows.row_s(row), j0 + CHUNK, d);
            } else if (nit < items) {
                item_at(nit, nrow, nc);
                rsn = chunk_rsrc(rows.row_s(nrow), nc * CHUNK, d);
            } else {
                rsn = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rows.row_s(row)), (short)0, 0, 0x00020000);
            }
            const uint32_t cnt0 = cnt;
            __amdgpu_buffer_rsrc_t ro;
            if constexpr (LONE != 0) ro = chunk_rsrc(zout, j0, d);
            // opaque per-chunk copy of the lane offset: stops LICM from hoisting the 64 per-(load,
            // component) index constants out of the loop into 64 live VGPRs
            uint32_t lb = (uint32_t)j0 + (uint32_t)lane * 4u;   // row index of the lane's element 0
            asm volatile("" : "+v"(lb));
#pragma unroll
            for (int L = 0; L < 16; ++L) {
                const int P = L + RING - 1;
                ring[P % RING] = P < 16 ? load_q(rs, lane, P) : load_q(rsn, lane, P - 16);
                const float4 x = ring[L % RING];
                if constexpr (LONE != 0) {
                    // unconditional (range-checked): one more store per step in the vmcnt queue
                    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
                    const u4v z = {0u, 0u, 0u, 0u};
                    __builtin_amdgcn_raw_buffer_store_b128(z, ro, lane * 16, L * 1024, 0);
                }
                const uint32_t jl = lb + (uint32_t)(L * 256);             // index in the row
                const float vq[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (FLC_TK_PROBE == 3) { cnt += __float_as_uint(vq[q]) == 0x7F800001u ? 1u : 0u; continue; }
                    const bool f = mag_key(vq[q]) >= T;
                    const uint64_t m = __ballot(f);
                    if (FLC_TK_PROBE != 1 && f) {
                        // slot = min(cnt, GCAP) + entries in lower lanes (< GCAP + 64): exact while
                        // the group fits; past GCAP it overflows (its row takes the exact path) and
                        // the writes land in the spare slots.  The scalar part folded into the LDS
                        // address in SALU, index and value out as one ds_write2st64_b32 (values
                        // SROW words on)
                        const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        uint32_t sb = sla + min(cnt, (uint32_t)GCAP) * 4u;
                        asm volatile("" : "+s"(sb));
                        asm volatile("ds_write2st64_b32 %0, %1, %2 offset1:%3" ::"v"(sb + pre * 4u),
                                     "v"(jl + q), "v"(__float_as_uint(vq[q])), "i"(SROW * 4 / 256) : "memory");
                    }
                    cnt += (uint32_t)__popcll(m);
                }
            }
            ccp |= (uint64_t)min(cnt - cnt0, 0xFFFFu) << (16 * (c - cg0));
            rs = rsn;
        }
        if (pv) finish(par ^ 1);
        uint32_t res = 0;
        // the shard of the group's index within its row (the item order interleaves rows: `it % shards`
        // put each of n rows' items into only 64 / n shards, which overflowed them)
        const int64_t shard = shards > 1 ? (cg0 / FGS) % shards : 0;
        if (cnt && cnt <= GCAP && lane == 0)
            res = atomicAdd(shards > 1 ? &ws.shcnt[(row * shards + shard) * RCS] : &ws.rowcnt[(row) * RCS], cnt);
        pv = true; prow = row; pc0 = cg0; pcc = ccp; ptot = cnt; pres = res; pseg = shard;
        // the staging writes of this group and the copy-out reads of the buffer's next use are in
        // the wave's own program order; the fence keeps the compiler from moving LDS ops across
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        par ^= 1;
        it = nit;
        row = nrow;
        c = nc;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    finish(par ^ 1);
}

// ------------------------------------------------------------------------------------------
// Many-row fast-path filter (one list per row, no zout): workgroup items.  An item is NL
// consecutive 4-chunk groups of ONE row.  Waves 0 .. NL-1 are loaders: each streams one group of
// the item exactly as k_topk_filter_fast does (the RING-deep nontemporal load pipeline across item
// boundaries, ballot / mbcnt compaction into its own double-buffered staging, GCAP per group,
// threshold max(T, 1)) and issues NO global store or atomic, so its vmcnt queue holds loads only.
// Wave NL is the writer: it loads no rows; per item it takes the NL groups' counts from LDS, makes
// ONE reservation on the row's counter for the groups that fit, writes the item's 4 NL tab entries
// and the overflow flag, and copies the staged entries out as one contiguous piece per array.
//
// Hand-over through LDS words only, per (buffer, loader) {chunk counts lo, hi, total, filled} and
// per buffer {freed}: a loader publishes filled = k + 1 after staging its k-th item (LDS executes a
// wave's operations in order), the writer publishes freed = k + 1 after its last read of that
// item's staging, and a loader refills a buffer (item k >= 2) only once freed == k - 1.
// Progress: NO wave ever waits on another workgroup.  The writer waits only for the loaders of its
// own workgroup to stage item k, a loader only for the writer to have drained item k - 2, and all
// waves of a workgroup are resident together; by induction over k nothing waits for ever.
// ------------------------------------------------------------------------------------------
__device__ inline uint32_t lds_addr(const void* p) {
    return (uint32_t)(size_t)(const __attribute__((address_space(3))) void*)p;
}
// a word another wave of the workgroup writes: read and waited for in one statement
__device__ inline uint32_t lds_peek(uint32_t addr) {
    uint32_t v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr) : "memory");
    return __builtin_amdgcn_readfirstlane(v);
}
template <int RING, int NL>
__global__ __launch_bounds__((NL + 1) * 64) __attribute__((amdgpu_waves_per_eu(FLC_TK_WG_WPE))) void k_topk_filter_fast_wg(RowSrc rows, int64_t n, int64_t r0, int64_t rn, int64_t rb, int64_t d,
                                                                        SelWs ws) {
    static_assert(16 % RING == 0, "ring must divide the 16 loads of a chunk");
    constexpr int FGS = 4;
    constexpr int SROW = GCAP + 64;       // as k_topk_filter_fast: 64 spare slots take the wave-instruction that overflows
    __shared__ __attribute__((aligned(16))) uint32_t st[2][NL][2 * SROW];
    __shared__ __attribute__((aligned(16))) uint32_t hs[2][NL][4];   // chunk counts (4 x 16 bits), total, filled
    __shared__ uint32_t fr[2];                                         // freed
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < 2 * NL * 4) (&hs[0][0][0])[threadIdx.x] = 0;
    if (threadIdx.x < 2) fr[threadIdx.x] = 0;
    __syncthreads();                                                   // the only barrier: before any load is issued
    const int64_t C = nchunks(d);
    const int64_t G = (C + FGS * NL - 1) / (FGS * NL);                  // items per row
    const int64_t items = rn * G;
    const int64_t stride = gridDim.x;
    int64_t it = blockIdx.x;
    if (it >= items) return;
    // item order as k_topk_filter_fast: blocks of rb rows, inside a block (item, row) with the row fastest
    auto item_at = [&](int64_t t, int64_t& r, int64_t& cc) {
        const int64_t blk = t / (rb * G), rem = t - blk * rb * G;
        const int64_t bn = min(rb, rn - blk * rb);
        const int64_t g = rem / bn;
        r = r0 + blk * rb + (rem - g * bn);
        cc = g * (FGS * NL);
    };
    if (wv == NL) {
        // ---- writer ----
        for (uint32_t k = 0; it < items; it += stride, ++k) {
            const int b = k & 1;
            int64_t row, c0;
            item_at(it, row, c0);
            const uint32_t fa = lds_addr(&hs[b][min(lane, NL - 1)][3]);
            for (;;) {
                uint32_t f;
                asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(f) : "v"(fa) : "memory");
                if (__ballot(f != k + 1) == 0) break;
                __builtin_amdgcn_s_sleep(4);
            }
            uint32_t pre[NL], tot[NL], sum = 0;
            uint64_t cc[NL];
            bool allfit = true;
#pragma unroll
            for (int w = 0; w < NL; ++w) {
                const uint4 h = *reinterpret_cast<const uint4*>(hs[b][w]);
                cc[w] = (uint64_t)h.x | ((uint64_t)h.y << 32);
                tot[w] = h.z;
                pre[w] = sum;
                sum += tot[w] <= GCAP ? tot[w] : 0u;                     // a group past GCAP contributes nothing
                allfit = allfit && tot[w] <= GCAP;
            }
            uint32_t base = 0;
            bool fits = true;                                            // the item's reservation is inside the row's list
            if (sum) {
                uint32_t res = 0;
                if (lane == 0) res = atomicAdd(&ws.rowcnt[row * RCS], sum);
                base = __shfl(res, 0, WAVE);
                fits = (int64_t)base + sum <= ws.cap;
            }
            if (lane < FGS * NL && c0 + lane < C) {
                uint32_t off = 0, cu = 0;
                bool gf = false;
#pragma unroll
                for (int w = 0; w < NL; ++w)
                    if ((lane >> 2) == w) {
                        off = pre[w];
                        gf = tot[w] <= GCAP;
#pragma unroll
                        for (int u = 0; u < FGS; ++u) {
                            const uint32_t x = (uint32_t)(cc[w] >> (16 * u)) & 0xFFFFu;
                            off += u < (lane & 3) ? x : 0u;
                            cu = u == (lane & 3) ? x : cu;
                        }
                    }
                ws.tab[(c0 + lane) * n + row] = make_uint2(base + off, fits && gf ? cu : 0u);
            }
            if (!(fits && allfit) && lane == 0) atomicOr(&ws.flags[row], F_OVERFLOW);
#pragma unroll
            for (int w = 0; w < NL; ++w)
                tk_copy_out<FLC_TK_WG_STPOL>(st[b][w], st[b][w] + SROW, ws, n, row, base + pre[w], tot[w], fits && tot[w] <= GCAP, lane,
                            (int64_t)blockIdx.x * NL + w);
            // the staging reads above are done before the loaders may refill the buffer
            asm volatile("s_waitcnt lgkmcnt(0)\n\tds_write_b32 %0, %1" ::"v"(lds_addr(&fr[b])), "v"(k + 1) : "memory");
        }
        return;
    }
    // ---- loaders ----
    float4 ring[RING];
    int64_t row, c;                                                      // current row, this wave's chunk
    item_at(it, row, c);
    c += wv * FGS;
    auto rs = chunk_rsrc(rows.row_s(row), c * CHUNK, d);
#pragma unroll
    for (int L = 0; L < RING - 1; ++L) {
        ring[L] = load_q(rs, lane, L);
        __builtin_amdgcn_sched_barrier(0);   // issue in ring order: the loop's static vmcnt waits assume it
    }
    for (uint32_t k = 0; it < items; ++k) {
        const int b = k & 1;
        if (k >= 2) {
            const uint32_t fa = lds_addr(&fr[b]);
            while (lds_peek(fa) != k - 1) __builtin_amdgcn_s_sleep(2);
        }
        const uint32_t T = max(sload(ws.thr + row), 1u);                 // as k_topk_filter_fast
        const int64_t nit = it + stride;
        const uint32_t sla = __builtin_amdgcn_readfirstlane(lds_addr(st[b][wv]));
        uint32_t cnt = 0;
        uint64_t ccp = 0;
        const int64_t cg0 = c;
        int64_t nrow = row, nc = c;
        // straight-line over the group; chunks past the row end (a short or empty last group) have
        // empty descriptors and their loads return zeros
#pragma unroll
        for (int sub = 0; sub < FGS; ++sub, ++c) {
            const int64_t j0 = c * CHUNK;
            __amdgpu_buffer_rsrc_t rsn;
            if (sub + 1 < FGS) {
                rsn = chunk_rsrc(rows.row_s(row), j0 + CHUNK, d);
            } else if (nit < items) {
                item_at(nit, nrow, nc);
                nc += wv * FGS;
                rsn = chunk_rsrc(rows.row_s(nrow), nc * CHUNK, d);
            } else {
                rsn = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rows.row_s(row)), (short)0, 0, 0x00020000);
            }
            const uint32_t cnt0 = cnt;
            uint32_t lb = (uint32_t)j0 + (uint32_t)lane * 4u;   // row index of the lane's element 0 (opaque: see k_topk_filter_fast)
            asm volatile("" : "+v"(lb));
#pragma unroll
            for (int L = 0; L < 16; ++L) {
                const int P = L + RING - 1;
                ring[P % RING] = P < 16 ? load_q(rs, lane, P) : load_q(rsn, lane, P - 16);
                const float4 x = ring[L % RING];
                const uint32_t jl = lb + (uint32_t)(L * 256);
                const float vq[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool f = mag_key(vq[q]) >= T;
                    const uint64_t m = __ballot(f);
                    if (f) {
                        const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        uint32_t sb = sla + min(cnt, (uint32_t)GCAP) * 4u;
                        asm volatile("" : "+s"(sb));
                        asm volatile("ds_write2st64_b32 %0, %1, %2 offset1:%3" ::"v"(sb + pre * 4u),
                                     "v"(jl + q), "v"(__float_as_uint(vq[q])), "i"(SROW * 4 / 256) : "memory");
                    }
                    cnt += (uint32_t)__popcll(m);
                }
            }
            ccp |= (uint64_t)min(cnt - cnt0, 0xFFFFu) << (16 * (c - cg0));
            rs = rsn;
        }
        // counts, then filled: in this order behind the staging writes (one wave's LDS operations execute in order)
        if (lane == 0)
            asm volatile("ds_write_b64 %0, %1\n\tds_write_b32 %0, %2 offset:8\n\tds_write_b32 %0, %3 offset:12"
                         ::"v"(lds_addr(hs[b][wv])), "v"(ccp), "v"(cnt), "v"(k + 1) : "memory");
        it = nit;
        row = nrow;
        c = nc;
    }
}

static int filter_group() {
    static const int g = [] {
        const char* e = tuning_env("FLC_FILTER_GS");     // tuning runs only
        return (e && atoi(e) == 2) ? 2 : 4;
    }();
    return g;
}

template <int FGS>
static void launch_filter(RowSrc rows, int64_t n, int64_t r0, int64_t rn, int64_t d, SelWs ws, hipStream_t st,
                          int shards, float* zout = nullptr) {
    // oversubscribed grid (measured: 16-32 K blocks beat a resident-only persistent grid by ~5 %,
    // the hardware dispatcher balances the tail)
    const int64_t waves = rn * ((nchunks(d) + FGS - 1) / FGS);
    const int gw = (int)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, 32768));
    static const int64_t rb = [] {
        // rows per block of the item order: 64 measured 0.5 % faster than row-major (1) at C3
        const char* e = tuning_env("FLC_TK_RB");          // tuning runs only
        return e ? std::max<int64_t>(1, atoll(e)) : (int64_t)64;
    }();
    ProfScope _pv(FGS == 4 ? "k_topk_filter_g4" : "k_topk_filter_g2", st);   // which variant ran (tests)
    if constexpr (FGS == 4 && FLC_TK_WG != 0 && FLC_TK_PROBE != 1 && FLC_TK_PROBE != 3) {   // (probes 1 and 3 exist in k_topk_filter_fast only)
        // many rows (one list per row, no zout): workgroup items; tuning builds FLC_FILTER_WG=0 keep
        // the per-wave groups for the A/B
        static const bool wg = [] { const char* e = tuning_env("FLC_FILTER_WG"); return !(e && atoi(e) == 0); }();
        if (wg && shards == 1 && !zout) {
            constexpr int NL = FLC_TK_WG_NL;
            const int64_t items = rn * ((nchunks(d) + 4 * NL - 1) / (4 * NL));
            const int gi = (int)std::max<int64_t>(1, std::min<int64_t>(items, 32768));
            // rows per block of the item order: 16 and 1 measured 0.10 ms a C3 step under 64, 256 0.03 over it
            // (each against k_topk_filter_fast in its own process, profiles/r07/wgfilter/rb.jsonl)
            static const int64_t rbw = [] {
                const char* e = tuning_env("FLC_TK_RB");  // tuning runs only
                return e ? std::max<int64_t>(1, atoll(e)) : (int64_t)16;
            }();
            hipLaunchKernelGGL((k_topk_filter_fast_wg<FLC_TK_WG_RING, NL>), dim3(gi), dim3((NL + 1) * 64), 0, st, rows, n, r0,
                               rn, std::min(rbw, std::max<int64_t>(rn, 1)), d, ws);
            return;
        }
    }
    if (zout)
        hipLaunchKernelGGL((k_topk_filter_fast<FLC_TK_RING, FGS, 1>), dim3(gw), dim3(256), 0, st, rows, n, r0, rn,
                           std::min(rb, std::max<int64_t>(rn, 1)), d, ws, shards, zout);
    else
        hipLaunchKernelGGL((k_topk_filter_fast<FLC_TK_RING, FGS>), dim3(gw), dim3(256), 0, st, rows, n, r0, rn,
                           std::min(rb, std::max<int64_t>(rn, 1)), d, ws, shards, (float*)nullptr);
}

void launch_filter_rows(const TkCall& c, int64_t r0, int64_t rn) {
    // few rows: 2-chunk groups (twice the waves in flight for a lone row)
    // (one-chunk items for a lone 10 M row measured slower: 26 -> 36 us)
    // a lone compressVector row: the filter also writes the dense output's zeros
    float* zout = c.lone_assign ? c.out : nullptr;
    if (filter_group() == 2 || c.n * c.d < ((int64_t)64 << 20)) launch_filter<2>(c.rows, c.n, r0, rn, c.d, c.ws, c.st, c.few ? CS_SH : 1, zout);
    else launch_filter<4>(c.rows, c.n, r0, rn, c.d, c.ws, c.st, c.few ? CS_SH : 1, zout);
}

void launch_sample(const TkCall& c, int64_t a, int64_t b, hipStream_t sx) {
    if (b <= a) return;
    ProfScope _ps("k_topk_sample", sx);
    // 1024-thread workgroups for any row count (measured 0.098 -> 0.066 ms against 256 at C3)
    hipLaunchKernelGGL((c.few ? k_topk_sample<1024, true> : k_topk_sample<1024, false>), dim3((unsigned)(b - a)), dim3(1024), 0, sx,
                       c.rows, c.n, c.d, c.K, c.ws, c.few ? 1 : 0, a);
}

// dense K: the exact selection of every row (thr, krem and the tie prefixes are final)
int launch_filter_exact(const TkCall& c) {
    const int64_t bpr = (host_chunks(c.d) + 3) / 4;
    const int gb = grid_stride_blocks(c.n * bpr, 8192);
    { ProfScope _ps("k_topk_filter_exact", c.st);
    with_vec(c.vec, [&](auto v) {
        hipLaunchKernelGGL((k_topk_filter<true, decltype(v)::value>), dim3(gb), dim3(256), 0, c.st, c.rows, c.n, c.d, c.ws);
    }); }
    FLC_CHECK_LAUNCH("k_topk_filter(exact)");
    return FLC_OK;
}

}  // namespace flc
