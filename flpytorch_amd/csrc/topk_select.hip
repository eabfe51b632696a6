// The selection core's TopK selects: the exact K-th key over a row's candidate list (k_cand_select,
// k_cs_pass), the exact path over full rows (radix passes, worklist, exact_row, tie kernels) and the
// kernels that combine the two (k_cand_select_x, k_assign_finish), with their launchers.
// cand_select_row and exact_row are each shared by several of these kernels: one unit.
// Data flow, workspace and switches: select_impl.hpp.
#include "select_impl.hpp"

namespace flc {

// ------------------------------------------------------------------------------------------
// Exact K-th key over a row's candidate list (fast path), one workgroup per row.
// Every candidate has key >= T (the sample threshold), and the K-th largest key of the row is
// among them when the list holds >= K entries.  Digits are taken of the offset dk = key - T:
// the first digit is dk >> s0 clamped to HBINS-1, with s0 sized so that the sample's estimate of
// the K-th key falls in the lowest quarter of the bins; the following digits are 11-bit slices
// of dk below s0 (usually one, exact: 2 passes over the list instead of 3 full-key passes, and
// the bins spread over the populated range instead of the few exponent values a full-key first
// digit sees).  A K-th key in the clamp bin (estimate off by > 4x) sends the row to the exact
// path.  Result as k_radix_select's last pass: thr = K-th key, krem = ties to admit, F_TIES when
// the list has more keys equal to thr than that.
// ------------------------------------------------------------------------------------------
// candidate values of a row, read twice per launch (FLC_CS_NT: nontemporal loads)
__device__ inline float4 cs_ld(const float4* p) {
#if FLC_CS_NT
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
template <int NT>
__device__ void cand_select_row(int64_t row, int64_t K, SelWs ws, uint32_t* h, uint32_t* scratch) {
    {
        if (ws.flags[row]) return;                                       // overflowed in the filter
        const uint32_t cnt = ws.rowcnt[(row) * RCS];
        if (cnt < (uint32_t)K) {                                          // sample threshold too high
            if (threadIdx.x == 0) ws.flags[row] |= F_SHORT;
            return;
        }
        const uint32_t T = ws.thr[row];
        const uint32_t span = ws.prefix[row] - T;                         // kest >= T
        int s = 0;
        while (s < 21 && (((uint64_t)span * 4u) >> s) >= (uint64_t)HBINS) ++s;
        const float* vals = ws.ent_val + row * ws.cap;                    // cap % 4 == 0: 16 B rows
        const float4* v4 = reinterpret_cast<const float4*>(vals);
        const uint32_t n4 = cnt >> 2;
        uint32_t prefix = 0, krem = (uint32_t)K, last = 0;
        bool first = true, fail = false;
        int sh = s;
        while (true) {
            const int s1 = first ? sh : max(0, sh - 11);
            const uint32_t mask = first ? 0xFFFFFFFFu : ((1u << (sh - s1)) - 1u);
            for (int i = threadIdx.x; i < HBINS; i += NT) h[i] = 0;
            __syncthreads();
            auto add = [&](float x) {
                const uint32_t dk = mag_key(x) - T;
                if (first) atomicAdd(&h[min(dk >> s1, (uint32_t)(HBINS - 1))], 1u);
                else if ((dk >> sh) == prefix) atomicAdd(&h[(dk >> s1) & mask], 1u);
            };
            // 8 float4 per thread in flight per round trip (the walk is latency-bound otherwise)
            uint32_t i = threadIdx.x;
            for (; i + 7 * NT < n4; i += 8 * NT) {
                float4 q[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) q[u] = cs_ld(v4 + i + u * NT);
#pragma unroll
                for (int u = 0; u < 8; ++u) { add(q[u].x); add(q[u].y); add(q[u].z); add(q[u].w); }
            }
            for (; i < n4; i += NT) {
                const float4 q = v4[i];
                add(q.x); add(q.y); add(q.z); add(q.w);
            }
            for (uint32_t i = n4 * 4 + threadIdx.x; i < cnt; i += NT) add(vals[i]);
            __syncthreads();
            uint32_t bin, above;
            hist_find(h, krem, bin, above, scratch);
            last = h[bin];
            if (first && bin == HBINS - 1) { fail = true; break; }
            prefix = first ? bin : ((prefix << (sh - s1)) | bin);
            krem -= above;
            sh = s1;
            first = false;
            __syncthreads();
            if (sh == 0) break;
        }
        __syncthreads();
        // ambiguous ties (more entries with key == thr than places left): the reference keeps the
        // lowest indices (torch.topk on CPU; oracle.codecs.topk_indices).  Gather the tie indices
        // and find the krem-th smallest: the admission cut for k_chunk_accum.
        const uint32_t thr = T + prefix;
        bool ties = !fail && last > krem;
        if (ties && last > TIECAP) { fail = true; ties = false; }      // pathological: exact path
        if (ties) {
            uint32_t* tix = h;                                           // reuse the histogram
            if (threadIdx.x == 0) scratch[0] = 0;
            __syncthreads();
            const uint32_t* idxs = ws.ent_idx + row * ws.cap;
            for (uint32_t i = threadIdx.x; i < n4; i += NT) {
                const float4 q = v4[i];
                const float qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (mag_key(qv[u]) == thr) tix[atomicAdd(&scratch[0], 1u)] = idxs[i * 4 + u];
            }
            for (uint32_t i = n4 * 4 + threadIdx.x; i < cnt; i += NT) {
                if (mag_key(vals[i]) == thr) tix[atomicAdd(&scratch[0], 1u)] = idxs[i];
            }
            __syncthreads();
            const uint32_t m = scratch[0];                              // == last
            for (uint32_t a = threadIdx.x; a < m; a += NT) {
                const uint32_t ia = tix[a];
                uint32_t rank = 0;
                for (uint32_t b = 0; b < m; ++b) rank += tie_pref(tix[b], ws.tie_hi) > tie_pref(ia, ws.tie_hi) ? 1u : 0u;
                if (rank == krem - 1) ws.tiecut[row] = ia;              // indices are distinct
            }
        }
        if (threadIdx.x == 0) {
            if (fail) {
                ws.flags[row] |= F_SHORT;
            } else {
                ws.thr[row] = thr;
                ws.krem[row] = krem;
                if (ties) ws.flags[row] |= F_TIES;
            }
        }
        __syncthreads();
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_cand_select(int64_t r0, int64_t rn, int64_t K, SelWs ws) {
    __shared__ uint32_t h[HBINS];
    __shared__ uint32_t scratch[260];
    for (int64_t row = r0 + blockIdx.x; row < r0 + rn; row += gridDim.x) {
        cand_select_row<NT>(row, K, ws, h, scratch);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// The same selection for a few rows (a lone compressVector), spread over the chip: each row's
// list is split over gridDim.x workgroups that histogram their slices (LDS) into the row's global
// histogram (atomics); the last workgroup to arrive picks the digit (the same digits, bins and
// results as k_cand_select) and leaves the row's state for the next launch — one launch per digit
// instead of one latency-bound workgroup walking 1.4 K candidates twice.  Ambiguous ties at the
// K-th key (more entries equal to it than places left; ~1 row in 8 at D = 10 M) are resolved by the
// last arriver as k_cand_select does: the tie indices gathered over all shards, the krem-th smallest
// is the admission cut (the reference keeps the lowest indices).  Only more than TIECAP ties take
// the exact path.
// ------------------------------------------------------------------------------------------
constexpr int CS_NT = 256;
// final_pass: no launch follows this one (a row the digits have not settled by then takes the exact
// path); list mode (second pass, the first digit's bin holding at most CS_LCAP entries): every
// workgroup copies its shard's entries of that bin to the row's list and the last arriver ranks them
// by (key desc, index asc) — the K-th key and the tie cut at once, whatever bits are left below the
// first digit, so two launches settle the row.
__global__ __launch_bounds__(CS_NT) void k_cs_pass(int64_t K, SelWs ws, int final_pass) {
    __shared__ uint32_t h[HBINS];
    __shared__ uint32_t scratch[260];
    __shared__ uint32_t last_wg;
    __shared__ uint64_t lst[FLC_CS_LIST ? CS_LCAP : 1];
    const int64_t row = blockIdx.y;
    const uint32_t B = gridDim.x, b = blockIdx.x;
    uint32_t* cs = ws.cstate + row * CS_ST;                              // shift, prefix, krem, stage, bin count, list fill
    const uint32_t stage = cs[3];
    if (stage >= 2u) return;                                             // done: the whole grid row
    // the row's list is CS_SH shards (the filter's reservations): workgroup b walks shard b
    const uint32_t* shc = ws.shcnt + row * CS_SH * RCS;
    uint32_t cnt = 0;
    for (int k = 0; k < CS_SH; ++k) cnt += shc[k * RCS];
    const uint32_t mycnt = shc[b * RCS];
    const bool first = stage == 0u;
    if (first && (ws.flags[row] != 0u || cnt < (uint32_t)K)) {          // overflowed / sample too high
        if (b == 0 && threadIdx.x == 0) {
            if (ws.flags[row] == 0u) ws.flags[row] = F_SHORT;
            cs[3] = 2u;
        }
        return;
    }
    const uint32_t T = ws.thr[row];
    uint32_t sh, prefix, krem;
    if (first) {
        const uint32_t span = ws.prefix[row] - T;                        // kest >= T
        uint32_t s0 = 0;
        while (s0 < 21 && (((uint64_t)span * 4u) >> s0) >= (uint64_t)HBINS) ++s0;
        sh = s0; prefix = 0; krem = (uint32_t)K;
    } else {
        sh = cs[0]; prefix = cs[1]; krem = cs[2];
    }
    const uint32_t s1 = first ? sh : (sh > 11u ? sh - 11u : 0u);
    const uint32_t mask = first ? 0xFFFFFFFFu : ((1u << (sh - s1)) - 1u);
    const int64_t segcap = (ws.cap / CS_SH) & ~int64_t(3);
    if (FLC_CS_LIST && !first && cs[4] <= (uint32_t)CS_LCAP) {
        // list mode: this shard's entries of the first digit's bin, as (key << 32 | ~index)
        if (threadIdx.x == 0) scratch[0] = 0;
        __syncthreads();
        const float* sv = ws.ent_val + row * ws.cap + b * segcap;
        const uint32_t* si = ws.ent_idx + row * ws.cap + b * segcap;
        for (uint32_t e = threadIdx.x; e < mycnt; e += CS_NT) {
            const uint32_t key = mag_key(sv[e]);
            if (((key - T) >> sh) == prefix) {
                const uint32_t slot = atomicAdd(&scratch[0], 1u);
                if (slot < (uint32_t)CS_LCAP) lst[slot] = ((uint64_t)key << 32) | (uint64_t)tie_pref(si[e], ws.tie_hi);
            }
        }
        __syncthreads();
        const uint32_t nl = min(scratch[0], (uint32_t)CS_LCAP);
        if (threadIdx.x == 0) scratch[1] = nl ? atomicAdd(&cs[5], nl) : 0u;
        __syncthreads();
        uint64_t* gl = ws.clist + row * CS_LCAP;
        const uint32_t gb = scratch[1];
        for (uint32_t i = threadIdx.x; i < nl; i += CS_NT)
            if (gb + i < (uint32_t)CS_LCAP) gl[gb + i] = lst[i];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            last_wg = atomicAdd(&ws.carrive[row * RCS], 1u) == B - 1u ? 1u : 0u;
        }
        __syncthreads();
        if (!last_wg) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const uint32_t m = __hip_atomic_load(&cs[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool ok = m == cs[4] && m >= krem && krem >= 1u;          // every entry of the bin arrived
        const uint32_t mm = min(m, (uint32_t)CS_LCAP);
        for (uint32_t i = threadIdx.x; i < mm; i += CS_NT)
            lst[i] = __hip_atomic_load(&gl[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (threadIdx.x == 0) { scratch[0] = 0; scratch[1] = 0; scratch[2] = 0; scratch[3] = 0; }
        __syncthreads();
        // the entry of rank krem - 1 is the K-th: its key the threshold, its index the tie cut
        if (ok)
            for (uint32_t i = threadIdx.x; i < mm; i += CS_NT) {
                const uint64_t me = lst[i];
                uint32_t rank = 0;
                for (uint32_t j = 0; j < mm; ++j) rank += lst[j] > me ? 1u : 0u;
                if (rank == krem - 1u) { scratch[0] = (uint32_t)(me >> 32); scratch[1] = tie_pref((uint32_t)me, ws.tie_hi); }
            }
        __syncthreads();
        const uint32_t kth = scratch[0];
        if (ok)
            for (uint32_t i = threadIdx.x; i < mm; i += CS_NT) {
                const uint32_t key = (uint32_t)(lst[i] >> 32);
                if (key > kth) atomicAdd(&scratch[2], 1u);
                else if (key == kth) atomicAdd(&scratch[3], 1u);
            }
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicExch(&ws.carrive[row * RCS], 0u);
            if (!ok) {
                ws.flags[row] |= F_SHORT;                                // exact path
            } else {
                const uint32_t gt = scratch[2], eq = scratch[3];
                ws.thr[row] = kth;
                ws.krem[row] = krem - gt;                                // ties admitted
                if (gt + eq > krem) { ws.tiecut[row] = scratch[1]; ws.flags[row] |= F_TIES; }
            }
            cs[3] = 2u;
        }
        return;
    }
    for (int i = threadIdx.x; i < HBINS; i += CS_NT) h[i] = 0;
    __syncthreads();
    auto add = [&](float x) {
        const uint32_t dk = mag_key(x) - T;
        if (first) atomicAdd(&h[min(dk >> s1, (uint32_t)(HBINS - 1))], 1u);
        else if ((dk >> sh) == prefix) atomicAdd(&h[(dk >> s1) & mask], 1u);
    };
    const float* vals = ws.ent_val + row * ws.cap + b * segcap;          // 16 B aligned shards
    const float4* v4 = reinterpret_cast<const float4*>(vals);
    const uint32_t n4 = mycnt >> 2, q1 = n4;
    uint32_t i = threadIdx.x;
    for (; i + 3 * CS_NT < q1; i += 4 * CS_NT) {
        float4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = cs_ld(v4 + i + u * CS_NT);
#pragma unroll
        for (int u = 0; u < 4; ++u) { add(q[u].x); add(q[u].y); add(q[u].z); add(q[u].w); }
    }
    for (; i < q1; i += CS_NT) {
        const float4 q = cs_ld(v4 + i);
        add(q.x); add(q.y); add(q.z); add(q.w);
    }
    for (uint32_t t = n4 * 4 + threadIdx.x; t < mycnt; t += CS_NT) add(vals[t]);
    __syncthreads();
    uint32_t* gh = ws.hist + row * HBINS;
    for (int t = threadIdx.x; t < HBINS; t += CS_NT)
        if (h[t]) atomicAdd(gh + t, h[t]);
    // publish: every wave's adds complete, then one release + the arrival (the last arriver picks)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last_wg = atomicAdd(&ws.carrive[row * RCS], 1u) == B - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!last_wg) return;
    // the row's histogram read and cleared with memory-side atomics: current on any XCD
    for (int t = threadIdx.x; t < HBINS; t += CS_NT) h[t] = atomicExch(gh + t, 0u);
    __syncthreads();
    uint32_t bin, above;
    hist_find(h, krem, bin, above, scratch);
    const uint32_t last = h[bin];
    const uint32_t np = first ? bin : ((prefix << (sh - s1)) | bin);
    const uint32_t nk = krem - above;
    const bool clamp = first && bin == HBINS - 1;                        // K-th key in the clamp bin
    bool ties = !clamp && s1 == 0u && last > nk, tie_fail = ties && last > TIECAP;
    if (ties && !tie_fail) {
        // gather the indices of the entries with key == thr over all shards (4 threads per shard,
        // 8 float4 per thread in flight), then the nk-th smallest index is the cut
        static_assert(CS_NT == 4 * CS_SH, "tie gather: 4 threads per shard");
        __syncthreads();                                                 // h[bin] read by every thread
        uint32_t* tix = h;
        if (threadIdx.x == 0) scratch[0] = 0;
        __syncthreads();
        const uint32_t thr = T + np;
        const int k = threadIdx.x >> 2;
        const uint32_t sub = threadIdx.x & 3u, c = shc[k * RCS], c4 = c >> 2;
        const float* sv = ws.ent_val + row * ws.cap + k * segcap;
        const uint32_t* si = ws.ent_idx + row * ws.cap + k * segcap;
        const float4* s4 = reinterpret_cast<const float4*>(sv);
        auto test = [&](float x, uint32_t pos) {
            if (mag_key(x) == thr) {
                const uint32_t slot = atomicAdd(&scratch[0], 1u);
                if (slot < TIECAP) tix[slot] = si[pos];
            }
        };
        uint32_t j = sub;
        for (; j + 28u < c4; j += 32u) {
            float4 q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = cs_ld(s4 + j + 4u * u);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t p4 = (j + 4u * u) * 4u;
                test(q[u].x, p4); test(q[u].y, p4 + 1u); test(q[u].z, p4 + 2u); test(q[u].w, p4 + 3u);
            }
        }
        for (; j < c4; j += 4u) {
            const float4 q = cs_ld(s4 + j);
            test(q.x, j * 4u); test(q.y, j * 4u + 1u); test(q.z, j * 4u + 2u); test(q.w, j * 4u + 3u);
        }
        for (uint32_t t = c4 * 4u + sub; t < c; t += 4u) test(sv[t], t);
        __syncthreads();
        const uint32_t m = scratch[0];                                   // == last
        if (m != last) tie_fail = true;                                  // (uniform: scratch[0] in LDS)
        else
            for (uint32_t a = threadIdx.x; a < m; a += CS_NT) {
                const uint32_t ia = tix[a];
                uint32_t rank = 0;
                for (uint32_t bb = 0; bb < m; ++bb) rank += tie_pref(tix[bb], ws.tie_hi) > tie_pref(ia, ws.tie_hi) ? 1u : 0u;
                if (rank == nk - 1u) ws.tiecut[row] = ia;                // indices are distinct
            }
    }
    if (threadIdx.x == 0) {
        atomicExch(&ws.carrive[row * RCS], 0u);
        if (clamp) {
            ws.flags[row] |= F_SHORT;
            cs[3] = 2u;
        } else if (s1 == 0u) {
            if (tie_fail) ws.flags[row] |= F_SHORT;                      // > TIECAP ties: exact path
            else {
                ws.thr[row] = T + np;
                ws.krem[row] = nk;
                if (ties) ws.flags[row] |= F_TIES;
            }
            cs[3] = 2u;
        } else if (final_pass) {
            ws.flags[row] |= F_SHORT;                                    // digits left, no launch: exact path
            cs[3] = 2u;
        } else {
            cs[0] = s1; cs[1] = np; cs[2] = nk; cs[3] = 1u; cs[4] = last;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Radix passes over candidate lists (fast path) or full rows (exact path)
// ------------------------------------------------------------------------------------------
// Histogram of pass p over row data; grid-stride over (row, block of 64 K elements).
template <bool FULLROW>
__global__ __launch_bounds__(256) void k_radix_hist(RowSrc rows, int64_t n, int64_t d, int p, SelWs ws) {
    __shared__ uint32_t h[HBINS];
    constexpr int64_t BLK = 65536;
    const int64_t nrows = FULLROW ? (int64_t)(*ws.nwork) : n;
    const int64_t maxlen = FULLROW ? d : ws.cap;
    const int64_t bpr = (maxlen + BLK - 1) / BLK;
    const int64_t items = nrows * bpr;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t li = it / bpr;
        const int64_t row = FULLROW ? (int64_t)ws.worklist[li] : li;
        if (!FULLROW && ws.flags[row]) continue;
        const int64_t len = FULLROW ? d : (int64_t)ws.rowcnt[(row) * RCS];
        const int64_t b0 = (it % bpr) * BLK;
        if (b0 >= len) continue;
        const int64_t b1 = min(len, b0 + BLK);
        for (int i = threadIdx.x; i < HBINS; i += 256) h[i] = 0;
        __syncthreads();
        const uint32_t prefix = ws.prefix[row];
        const float* src = FULLROW ? rows.row(row) : (ws.ent_val + row * ws.cap);
        for (int64_t j = b0 + threadIdx.x; j < b1; j += 256) {
            const uint32_t k = mag_key(src[j]);
            if (key_in_prefix(k, p, prefix)) atomicAdd(&h[key_bin(k, p)], 1u);
        }
        __syncthreads();
        uint32_t* gh = ws.hist + row * HBINS;
        for (int i = threadIdx.x; i < HBINS; i += 256)
            if (h[i]) atomicAdd(&gh[i], h[i]);
        __syncthreads();
    }
}

// Select step of pass p: one workgroup per row.  After pass 2: thr = exact K-th key,
// krem = ties to admit.  Fast path: a short list (count < K) or ambiguous ties -> worklist.
template <bool FULLROW>
__global__ __launch_bounds__(256) void k_radix_select(int64_t n, int p, int64_t K, SelWs ws) {
    __shared__ uint32_t scratch[260];
    const int64_t nrows = FULLROW ? (int64_t)(*ws.nwork) : n;
    for (int64_t li = blockIdx.x; li < nrows; li += gridDim.x) {
        const int64_t row = FULLROW ? (int64_t)ws.worklist[li] : li;
        if (!FULLROW && ws.flags[row]) continue;
        uint32_t* gh = ws.hist + row * HBINS;
        if (!FULLROW && p == 0 && ws.rowcnt[(row) * RCS] < (uint32_t)K) {   // sample threshold too high
            for (int i = threadIdx.x; i < HBINS; i += 256) gh[i] = 0;
            if (threadIdx.x == 0) ws.flags[row] |= F_SHORT;
            continue;
        }
        const uint32_t k = (p == 0) ? (uint32_t)K : ws.krem[row];
        uint32_t bin, above;
        hist_find(gh, k, bin, above, scratch);
        const uint32_t ties_here = gh[bin];
        __syncthreads();
        for (int i = threadIdx.x; i < HBINS; i += 256) gh[i] = 0;    // ready for the next pass
        if (threadIdx.x == 0) {
            const uint32_t pre = (p == 0) ? 0u : ws.prefix[row];
            ws.prefix[row] = (pre << pass_bits(p)) | bin;
            ws.krem[row] = k - above;
            if (p == 2) {
                ws.thr[row] = ws.prefix[row];
                if (FULLROW) ws.tiecut[row] = ties_here;                  // the row's keys == thr (tie order)
                if (ties_here > k - above) ws.flags[row] |= (FULLROW ? F_TIES | F_EXACT : F_TIES);
                else if (FULLROW) ws.flags[row] |= F_EXACT;
            }
        }
        __syncthreads();
    }
}

// RowSrc that failed the fast path go on the worklist; their list state is reset.
__global__ void k_build_worklist(int64_t n, int64_t K, int64_t d, SelWs ws, int force_all) {
    // single block
    __shared__ uint32_t cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    for (int64_t row = threadIdx.x; row < n; row += blockDim.x) {
        uint32_t f = ws.flags[row];
        if (force_all || (f & (F_OVERFLOW | F_SHORT))) {   // ambiguous ties stay on the fast path
            uint32_t pos = atomicAdd(&cnt, 1u);
            ws.worklist[pos] = (uint32_t)row;
            ws.flags[row] = F_EXACT;
            ws.rowcnt[(row) * RCS] = 0;
            ws.prefix[row] = 0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *ws.nwork = cnt;
}

// Exact path of the fast path's rare failures, in ONE launch: a workgroup per row (grid-stride),
// rows without F_OVERFLOW / F_SHORT return at once.  A failed row gets the exact radix select over
// its full row (three 11/11/9-bit passes, LDS histogram), then its list is rewritten chunk by
// chunk in index order: key > thr, plus the first krem elements with key == thr (the lowest
// indices, the oracle's tie rule), tab[c][row] = (offset, count), flags = F_EXACT (the fold admits
// the whole list).  The same selection as the multi-launch path (k_build_worklist, k_radix_*,
// k_tie_*, k_topk_filter<true>) that dense-K rows take, without its ~10 launches per call when no
// row failed.

// One row's exact selection by one EX_NT-thread workgroup: three radix passes over the row, then the
// row's list rewritten with exactly its admitted entries in index order (ties: the lowest indices).
template <bool VEC, int NT = EX_NT>
__device__ void exact_row(RowSrc rows, int64_t n, int64_t row, int64_t d, int64_t K, SelWs ws, uint32_t* h,
                          uint32_t* scratch, uint32_t* wsum) {
    const int t = threadIdx.x;
    const int64_t C = nchunks(d);
    {
        const float* r = rows.row(row);
        uint32_t prefix = 0, krem = (uint32_t)K, ties_tot = 0;
        for (int p = 0; p < 3; ++p) {
            for (int i = t; i < HBINS; i += NT) h[i] = 0;
            __syncthreads();
            auto add = [&](uint32_t k) { if (key_in_prefix(k, p, prefix)) atomicAdd(&h[key_bin(k, p)], 1u); };
            int64_t j = 0;
            if (VEC) {
                const float4* r4 = reinterpret_cast<const float4*>(r);
                const int64_t g4 = d / 4;
                int64_t g = t;
                for (; g + (EX_U - 1) * NT < g4; g += EX_U * NT) {
                    float4 q[EX_U];
#pragma unroll
                    for (int u = 0; u < EX_U; ++u) q[u] = ld_row4(r4 + g + u * NT);
#pragma unroll
                    for (int u = 0; u < EX_U; ++u) {
                        add(mag_key(q[u].x)); add(mag_key(q[u].y)); add(mag_key(q[u].z)); add(mag_key(q[u].w));
                    }
                }
                for (; g < g4; g += NT) {
                    const float4 q = ld_row4(r4 + g);
                    add(mag_key(q.x)); add(mag_key(q.y)); add(mag_key(q.z)); add(mag_key(q.w));
                }
                j = g4 * 4;
            }
            for (int64_t jj = j + t; jj < d; jj += NT) add(mag_key(r[jj]));
            __syncthreads();
            uint32_t bin, above;
            hist_find(h, krem, bin, above, scratch);
            prefix = (prefix << pass_bits(p)) | bin;                   // p == 0: prefix is 0
            krem -= above;
            if (p == 2) ties_tot = h[bin];                              // the row's keys == thr
            __syncthreads();
        }
        const uint32_t thr = prefix;                                    // the K-th key; krem ties admitted
        // tie ranks admitted in index order: [0, krem) (lowest-index rule) or [tot - krem, tot)
        const uint32_t tie_from = ws.tie_hi ? ties_tot - krem : 0u, tie_to = ws.tie_hi ? ties_tot : krem;
        uint32_t* oi = ws.ent_idx + row * ws.cap;
        float* ov = ws.ent_val + row * ws.cap;
        // a chunk is CHUNK / (NT * 4) sub-blocks of NT * 4 columns (1 for NT = 1024, 2 / 4 for the
        // 512 / 256-thread selects), walked in index order with base and tie_run carried across them
        static_assert(CHUNK % (NT * 4) == 0, "exact_row: NT * 4 must divide CHUNK");
        constexpr int SUBS = CHUNK / (NT * 4);
        uint32_t base = 0, tie_run = 0, cbase = 0;
        for (int64_t cs = 0; cs < C * SUBS; ++cs) {
            const int64_t c = cs / SUBS;
            const int sb = (int)(cs % SUBS);
            if (sb == 0) cbase = base;
            const int64_t j0 = c * CHUNK + (int64_t)sb * (NT * 4) + (int64_t)t * 4;
            float v[4];
            if (VEC && j0 + 3 < d) {
                const float4 q = ld_row4(reinterpret_cast<const float4*>(r + j0));
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = (j0 + q < d) ? r[j0 + q] : 0.f;
            }
            bool gt[4], eq[4];
            uint32_t ne = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = j0 + q < d;
                const uint32_t k = mag_key(v[q]);
                gt[q] = in && k > thr;
                eq[q] = in && k == thr;
                ne += eq[q] ? 1u : 0u;
            }
            uint32_t etot;
            uint32_t erank = tie_run + ex_scan<NT>(ne, wsum, etot);        // ties before this thread's
            uint32_t na = 0;
            bool adm[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                adm[q] = gt[q] || (eq[q] && erank >= tie_from && erank < tie_to);
                erank += eq[q] ? 1u : 0u;
                na += adm[q] ? 1u : 0u;
            }
            uint32_t atot;
            uint32_t pos = base + ex_scan<NT>(na, wsum, atot);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (adm[q]) { oi[pos] = (uint32_t)(j0 + q); ov[pos] = v[q]; ++pos; }
            base += atot;
            tie_run += etot;
            if (sb == SUBS - 1 && t == 0) ws.tab[c * n + row] = make_uint2(cbase, base - cbase);
        }
        if (t == 0) {
            ws.thr[row] = thr;
            ws.krem[row] = krem;
            ws.rowcnt[row * RCS] = base;
            // the reason the fast path failed stays readable (flc_select_row_flags)
            ws.flags[row] = F_EXACT | (ws.flags[row] & (F_OVERFLOW | F_SHORT));
        }
        __syncthreads();
    }
}

template <bool VEC>
__global__ __launch_bounds__(EX_NT) void k_topk_exact_rows(RowSrc rows, int64_t n, int64_t r0, int64_t rn, int64_t d, int64_t K, SelWs ws) {
    __shared__ uint32_t h[HBINS];
    __shared__ uint32_t scratch[260];
    __shared__ uint32_t wsum[EX_NT / 64];
    for (int64_t row = r0 + blockIdx.x; row < r0 + rn; row += gridDim.x) {
        if (!(ws.flags[row] & (F_OVERFLOW | F_SHORT))) continue;       // row-uniform
        exact_row<VEC>(rows, n, row, d, K, ws, h, scratch, wsum);
    }
}

// The many-row candidate select with the exact fallback in the same workgroup: a row whose list
// overflowed in the filter, came up short, or whose K-th key the digits could not settle is
// selected exactly right here (exact_row with this workgroup's NT threads), so the group's
// select leaves every row final and no separate exact launch (a grid of 1024-thread workgroups
// that waited for whole CUs beside the next filter) follows it.
template <int NT, bool VEC>
__global__ __launch_bounds__(NT) void k_cand_select_x(RowSrc rows, int64_t n, int64_t r0, int64_t rn, int64_t d, int64_t K,
                                                      SelWs ws) {
    __shared__ uint32_t h[HBINS];
    __shared__ uint32_t scratch[260];
    __shared__ uint32_t wsum[NT / 64];
    __shared__ uint32_t failed;
    for (int64_t row = r0 + blockIdx.x; row < r0 + rn; row += gridDim.x) {
        cand_select_row<NT>(row, K, ws, h, scratch);
        __syncthreads();
        if (threadIdx.x == 0) failed = __atomic_load_n(&ws.flags[row], __ATOMIC_RELAXED) & (F_OVERFLOW | F_SHORT);
        __syncthreads();
        if (failed) exact_row<VEC, NT>(rows, n, row, d, K, ws, h, scratch, wsum);
        __syncthreads();
    }
}

// Exact path, ambiguous ties: per chunk count of key == thr, then the exclusive prefix over
// chunks (in index order) per row.  RowSrc without F_TIES get tieprefix = 0 (krem admits all ties).
__global__ __launch_bounds__(256) void k_tie_count(RowSrc rows, int64_t n, int64_t d, SelWs ws) {
    const int64_t C = nchunks(d);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nrows = *ws.nwork;
    const int64_t bpr = (C + 3) / 4;
    for (int64_t it = blockIdx.x; it < nrows * bpr; it += gridDim.x) {
        const int64_t row = ws.worklist[it / bpr];
        const int64_t c = (it % bpr) * 4 + wv;
        if (c >= C) continue;
        uint32_t cnt = 0;
        if (ws.flags[row] & F_TIES) {
            const uint32_t T = ws.thr[row];
            const float* r = rows.row(row);
            const int64_t j1 = min(d, (c + 1) * (int64_t)CHUNK);
            for (int64_t j = c * CHUNK + lane; j < j1; j += 64) cnt += (mag_key(r[j]) == T) ? 1u : 0u;
            cnt = wave_sum(cnt);
        }
        if (lane == 0) ws.tieprefix[c * n + row] = cnt;
    }
}

// Exclusive prefix of the per-chunk tie counts, in chunk (= index) order, for the exact-path
// worklist rows.
__global__ __launch_bounds__(256) void k_tie_scan(int64_t n, int64_t d, SelWs ws) {
    constexpr bool EXACT = true;
    __shared__ uint32_t part[256];
    const int64_t C = nchunks(d);
    const int64_t nrows = EXACT ? (int64_t)(*ws.nwork) : n;
    const int t = threadIdx.x;
    const int64_t per = (C + 255) / 256;           // chunks per thread (contiguous)
    for (int64_t li = blockIdx.x; li < nrows; li += gridDim.x) {
        const int64_t row = EXACT ? (int64_t)ws.worklist[li] : li;
        if (!EXACT && (ws.flags[row] & (F_TIES | F_EXACT)) != F_TIES) continue;
        const int64_t c0 = t * per, c1 = min(C, c0 + per);
        uint32_t sum = 0;
        for (int64_t c = c0; c < c1; ++c) sum += ws.tieprefix[c * n + row];
        part[t] = sum;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const uint32_t v = (t >= off) ? part[t - off] : 0u;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        uint32_t run = part[t] - sum;              // exclusive
        for (int64_t c = c0; c < c1; ++c) {
            const uint32_t v = ws.tieprefix[c * n + row];
            ws.tieprefix[c * n + row] = run;
            run += v;
        }
        __syncthreads();
    }
}

// A lone compressVector row on the fast path (its output zeroed by the filter): the exact fallback and
// the scatter in ONE launch.  A failed row (overflow / short list / ambiguous ties) is selected
// exactly by workgroup 0, which then scatters the rewritten list alone; otherwise every workgroup
// scatters its shards as k_assign_scatter does.
template <bool VEC>
__global__ __launch_bounds__(EX_NT) void k_assign_finish(RowSrc rows, int64_t d, int64_t K, SelWs ws, float* __restrict__ out) {
    __shared__ uint32_t h[HBINS];
    __shared__ uint32_t scratch[260];
    __shared__ uint32_t wsum[EX_NT / 64];
    if (ws.flags[0] & (F_OVERFLOW | F_SHORT)) {                          // uniform over the grid
        if (blockIdx.x != 0) return;
        exact_row<VEC>(rows, 1, 0, d, K, ws, h, scratch, wsum);
        __threadfence_block();
        const uint32_t cnt = ws.rowcnt[0];
        for (uint32_t e = threadIdx.x; e < cnt; e += EX_NT) out[ws.ent_idx[e]] = ws.ent_val[e];
        return;
    }
    const uint32_t T = ws.thr[0], f = ws.flags[0];
    const uint32_t cut = (f & F_TIES) ? tie_pref(ws.tiecut[0], ws.tie_hi) : 0u;
    const int64_t segcap = (ws.cap / CS_SH) & ~int64_t(3);
    for (int sh = (int)blockIdx.x; sh < CS_SH; sh += (int)gridDim.x) {
        const uint32_t cnt = ws.shcnt[sh * RCS];
        const int64_t o = sh * segcap;
        for (uint32_t e = threadIdx.x; e < cnt; e += EX_NT) {
            const uint32_t ix = ws.ent_idx[o + e];
            const float v = ws.ent_val[o + e];
            const uint32_t key = mag_key(v);
            if (key > T || (key == T && tie_pref(ix, ws.tie_hi) >= cut)) out[ix] = v;
        }
    }
}

// the candidate select of rows [r0, r0 + rn) on stream sx.  few rows (a lone compressVector): each
// list over 64 workgroups, one launch per digit (a finished row's workgroups exit at once); with
// list mode two launches settle a row whose first digit's bin holds <= CS_LCAP entries
// (~(4 sqrt(ks) + 8) D / 16 K spread over 256-512 bins: up to ~900 at D = 64 M), else 3 cover every
// shift; many rows: 512-thread workgroups (measured 0.289 -> 0.263 ms against 256 at C3)
void launch_select(const TkCall& c, int64_t r0, int64_t rn, bool last_of_many, hipStream_t sx) {
    const int64_t n = c.n, d = c.d, K = c.K;
    const SelWs& ws = c.ws;
    if (c.few) {
        const int np = (FLC_CS_LIST && d <= FLC_CS_TWO_MAXD) ? 2 : 3;
        for (int p = 0; p < np; ++p)
            hipLaunchKernelGGL(k_cs_pass, dim3((unsigned)CS_SH, (unsigned)n), dim3(CS_NT), 0, c.st, K, ws,
                               p == np - 1 ? 1 : 0);
    } else if (c.gfold) {
        // the select with the exact fallback in the same workgroup (every row final after it)
        const bool big = rn < 128 || last_of_many;
        const int nt = big ? 1024 : FLC_TK_SIDE_NT;
        const dim3 grid((unsigned)(big ? rn : grid_stride_blocks(rn, 8192)));
        with_vec(c.vec, [&](auto v) {
            constexpr bool V = decltype(v)::value;
            if (big) hipLaunchKernelGGL((k_cand_select_x<1024, V>), grid, dim3(nt), 0, sx, c.rows, n, r0, rn, d, K, ws);
            else if (FLC_TK_SIDE_NT == 256) hipLaunchKernelGGL((k_cand_select_x<256, V>), grid, dim3(nt), 0, sx, c.rows, n, r0, rn, d, K, ws);
            else hipLaunchKernelGGL((k_cand_select_x<512, V>), grid, dim3(nt), 0, sx, c.rows, n, r0, rn, d, K, ws);
        });
    } else if (rn < 128 || last_of_many)
        // few rows, or the last tail group (its select is exposed, nothing runs beside it):
        // 1024-thread workgroups, twice the loads in flight per row
        hipLaunchKernelGGL(k_cand_select<1024>, dim3((unsigned)rn), dim3(1024), 0, sx, r0, rn, K, ws);
    else if (FLC_TK_SIDE_NT == 256)
        // beside the next group's filter: one wave per SIMD (66 VGPRs) fits in the VGPRs the
        // filter's three waves per SIMD leave free, so the select co-resides with the
        // filter's blocks instead of displacing one (512-thread selects slowed the filter
        // they ran beside by ~8 %, round-4 trace)
        hipLaunchKernelGGL(k_cand_select<256>, dim3(grid_stride_blocks(rn, 8192)), dim3(256), 0, sx, r0, rn, K, ws);
    else hipLaunchKernelGGL(k_cand_select<512>, dim3(grid_stride_blocks(rn, 8192)), dim3(512), 0, sx, r0, rn, K, ws);
}

// the exact selection of every row the fast path failed: a workgroup per row, grid-stride, rows
// that did not fail return at once
int launch_exact_rows(const TkCall& c, hipStream_t sx) {
    ProfScope _ps("k_topk_exact_rows", sx);
    const int eb = grid_stride_blocks(c.n, FLC_TK_EXACT_WG);
    with_vec(c.vec, [&](auto v) {
        hipLaunchKernelGGL((k_topk_exact_rows<decltype(v)::value>), dim3(eb), dim3(EX_NT), 0, sx, c.rows, c.n, (int64_t)0, c.n, c.d, c.K, c.ws);
    });
    FLC_CHECK_LAUNCH("k_topk_exact_rows");
    return FLC_OK;
}

// dense K, after ws.hist and ws.flags are cleared: every row on the worklist, three radix hist /
// select pairs over the full rows, then the ties at the K-th key counted and scanned per chunk
int launch_radix_full(const TkCall& c) {
    const int64_t n = c.n, d = c.d, K = c.K;
    const SelWs& ws = c.ws;
    const hipStream_t st = c.st;
    const int64_t bpr = (host_chunks(d) + 3) / 4;
    hipLaunchKernelGGL(k_build_worklist, dim3(1), dim3(1024), 0, st, n, K, d, ws, 1);
    FLC_CHECK_LAUNCH("k_build_worklist");
    const int64_t hb = (d + 65535) / 65536;
    for (int p = 0; p < 3; ++p) {
        { ProfScope _ps("k_radix_hist_full", st);
        hipLaunchKernelGGL((k_radix_hist<true>), dim3(grid_stride_blocks(n * hb)), dim3(256), 0, st, c.rows, n, d, p, ws); }
        FLC_CHECK_LAUNCH("k_radix_hist(full)");
        hipLaunchKernelGGL((k_radix_select<true>), dim3(grid_stride_blocks(n, 1024)), dim3(256), 0, st, n, p, K, ws);
        FLC_CHECK_LAUNCH("k_radix_select(full)");
    }
    hipLaunchKernelGGL(k_tie_count, dim3(grid_stride_blocks(n * bpr, 4096)), dim3(256), 0, st, c.rows, n, d, ws);
    FLC_CHECK_LAUNCH("k_tie_count");
    hipLaunchKernelGGL(k_tie_scan, dim3(grid_stride_blocks(n, 1024)), dim3(256), 0, st, n, d, ws);
    FLC_CHECK_LAUNCH("k_tie_scan");
    return FLC_OK;
}

// a lone compressVector row on the few-row path (output zeros written by the filter): the exact
// fallback (if the row failed) + scatter
int launch_assign_finish(const TkCall& c) {
    ProfScope _ps("k_assign_finish", c.st);
    with_vec(c.vec, [&](auto v) {
        hipLaunchKernelGGL((k_assign_finish<decltype(v)::value>), dim3(CS_SH), dim3(EX_NT), 0, c.st, c.rows, c.d, c.K, c.ws, c.out);
    });
    FLC_CHECK_LAUNCH("k_assign_finish");
    return FLC_OK;
}

}  // namespace flc
