// The selection core's lone resident row: k_lone_resident with its grid rounds and repair, the
// library-owned control block, the serialisation of its launches and the test hook.  The gate that
// sends a call here is select.hip's.  Control-block layout and switches: select_impl.hpp.
#include "select_impl.hpp"

namespace flc {

// ------------------------------------------------------------------------------------------
// A lone compressVector row held in the chip's registers: the exact selection in ONE launch.
// The row (up to RS_U float4 a thread x 1024 threads x one workgroup per CU: 16.7 M elements on 256
// CUs, 64 MB of the chip's 128 MB of VGPRs) is read once into registers; the exact radix select
// (11/11/9-bit digits of the magnitude key, exact_row's digits) runs over it: per digit, each
// workgroup's LDS histogram is added into its group's replica (RS_NG groups: the atomics on one
// address come from G / RS_NG workgroups, not G — one global histogram's hot bins serialised 245
// deep), the workgroups arrive through a two-level counter tree, and the last to arrive sums the
// replicas, picks the digit (hist_find) and releases the others with the result in the release
// word.  After two digits the elements sharing the K-th key's 22-bit prefix (~70 on a Gaussian
// 10 M row, at most RS_CAP) are listed and ranked by the last workgroup to arrive (key, then tie
// order), which stores the kept ones; everyone else has written its dense output (x where the
// prefix is above, +0 elsewhere) and left.  Rows with more elements at that prefix take the third
// digit and a tie-rank exchange (workgroups publish their tie counts, tagged by the call's sequence
// number; one holding ties sums those before it).  No sample, no candidate lists, no fallback.
// The grid is meant to be co-resident: one 1024-thread workgroup per CU, G <= CUs, and the
// launches are serialised across the library's streams (lone_resident_launch).  Nothing outside
// the library is: another process's kernels, RCCL's, or a long kernel on a stream of the caller's
// can hold CUs while the grid starts.  So a wait never trusts stale data.  A wait past `spin`
// ticks of the 100 MHz clock (FLC_RS_SPIN, 0.1 s) ABORTS the call: it stores the call's sequence
// number in RS_GAVE, and every workgroup that waits (or later finds the word set) leaves without
// storing anything; a workgroup only stores output from a completed round, so every store made is
// a final value.  Every workgroup counts itself out on its group's RS_XGRP counter (after its last
// wait, before its stores; counters that run on across calls, the host passing the count before
// the launch).  The FIRST workgroup to abort instead waits for all the others to be out, then
// selects the row exactly on its own (rs_repair: three radix passes over the row in HBM and the
// dense output with the tie ranks, a few ms), rewrites the whole output, puts the control block
// back to zero and flags the row F_REPAIR.  Correct bits in every case; a clean call pays one
// non-returning counter atomic per workgroup.
// The control block is the library's own, zeroed once; a clean call leaves it clean
// (self-resetting barrier counters, replicas cleared by their merger), an aborted one is zeroed by
// its repair.
// ------------------------------------------------------------------------------------------
constexpr int RS_NT = 1024;

struct RsTree {
    uint32_t* ctl;
    uint32_t grp, gsz, ngr;             // this workgroup's group, its size, groups in use
};
// The release word (64 bits at RS_GEN): generation mod 8 | a 61-bit payload, the merger's result, so
// that the waiters get it with the release itself.  A digit's payload: bin | the count above it << 11
// (24 bits: < K <= 2^24) | the bin's count << 35 (25 bits).
__device__ inline uint64_t rs_digit(uint32_t bin, uint32_t above, uint32_t last) {
    return (uint64_t)bin | ((uint64_t)above << 11) | ((uint64_t)last << 35);
}
// Self-resetting two-level barrier (no per-call clearing): a group's counter is reset by its last
// arriver, the global one by the last group's; every workgroup reads the release word BEFORE
// arriving and waits for its generation to change (the merger bumps it after every arrival, so no
// workgroup can have read the new one).  rs_arrive returns true on the last workgroup to arrive (the
// merger), whose thread 0 has acquired every other workgroup's writes.
// (gen: the release word's generation, read by thread 0 before this workgroup's flush — any time
// after the previous release — so that its load is not one more round trip here)
__device__ inline uint32_t rs_gen(const RsTree& tr) {
    return (uint32_t)__hip_atomic_load(reinterpret_cast<const uint64_t*>(tr.ctl + RS_GEN), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 7u;
}
__device__ inline bool rs_arrive(const RsTree& tr, uint32_t* flag_s, uint32_t* gen_s, uint32_t gen) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                     // this wave's atomics performed
    __syncthreads();
    if (threadIdx.x == 0) {
        *gen_s = gen;
        if (FLC_RS_FENCE) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        uint32_t last = 0;
        uint32_t* gc = tr.ctl + RS_GRP + 32 * tr.grp;
#if FLC_RS_FENCE
        if (__hip_atomic_fetch_add(gc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tr.gsz - 1u) {
            // the group's members' writes (released before their arrivals) ordered before this
            // workgroup's release into the global counter: acquire, then release (transitivity)
            if (FLC_RS_GACQ) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(gc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            if (__hip_atomic_fetch_add(tr.ctl + RS_GLOB, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tr.ngr - 1u) {
                __hip_atomic_store(tr.ctl + RS_GLOB, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = 1;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
        }
#else
        // Write-through hand-off: every member drained its atomics before its add, so when an add
        // RETURNS the members counted before it have their bytes at the coherence point, and a
        // group's last add comes before that workgroup's global add (it waits for the value).
        // The counters are never stored to: an arrival is the last of its round when it takes the
        // count to a multiple of the group size, and that workgroup takes the group size back off
        // with an add — adds commute, so whenever that add lands (before or among the next
        // round's arrivals, which start only after this round's release) the next round's
        // arrivals still return every residue mod the size once, the last one gsz - 1.
        const uint32_t o = __hip_atomic_fetch_add(gc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((o + 1u) % tr.gsz == 0u) {
            __hip_atomic_fetch_add(gc, 0u - tr.gsz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t og = __hip_atomic_fetch_add(tr.ctl + RS_GLOB, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((og + 1u) % tr.ngr == 0u) {
                __hip_atomic_fetch_add(tr.ctl + RS_GLOB, 0u - tr.ngr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = 1;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");              // (compiler order only)
#endif
        *flag_s = last;
    }
    __syncthreads();
    return *flag_s != 0u;
}
// the merger, after its writes: the release word with its result
__device__ inline void rs_release(const RsTree& tr, const uint32_t* gen_s, uint64_t payload) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        // (the waiters read nothing but this word: its payload is the round's result)
        if (FLC_RS_FENCE) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_store(reinterpret_cast<uint64_t*>(tr.ctl + RS_GEN), (uint64_t)((*gen_s + 1u) & 7u) | (payload << 3),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// everyone else: the release word (thread 0 leaves its payload in res_s[0..1], low word first).
// false when the call is aborted — this wait passed `spin` ticks (it aborts the call; the first
// workgroup to abort, *rep_s = 1, repairs it) or another workgroup's did (RS_GAVE holds the
// call's sequence number): the caller leaves at once.
__device__ inline bool rs_wait(const RsTree& tr, const uint32_t* gen_s, uint32_t* res_s, uint32_t* ok_s,
                               uint32_t* rep_s, uint64_t spin, uint32_t seq, bool raw_bar = false) {
    if (threadIdx.x == 0) {
        const uint64_t* rw = reinterpret_cast<const uint64_t*>(tr.ctl + RS_GEN);
        uint32_t* ab = tr.ctl + RS_GAVE;
        const uint64_t t0 = (uint64_t)wall_clock64();
        uint64_t w;
        uint32_t ok = 1;
        for (uint32_t it = 0;; ++it) {
            // the abort word every FLC_RS_POLLAB-th poll (loaded beside the release word)
            w = __hip_atomic_load(rw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t a = (it % FLC_RS_POLLAB) == FLC_RS_POLLAB - 1
                                   ? __hip_atomic_load(ab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            if (((uint32_t)w & 7u) != *gen_s) break;
            if (a == seq) { ok = 0; break; }
            __builtin_amdgcn_s_sleep(1);
            if ((uint64_t)wall_clock64() - t0 > spin) {
                if (__hip_atomic_exchange(ab, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != seq) *rep_s = 1;
                ok = 0;
                break;
            }
        }
        if (FLC_RS_FENCE || !ok) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");      // (compiler order only)
        res_s[0] = (uint32_t)(w >> 3);
        res_s[1] = (uint32_t)(w >> 35);
        *ok_s = ok;
    }
    if (raw_bar) {                     // (the other waves' stores in flight stay in flight)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    } else {
        __syncthreads();
    }
    return *ok_s != 0u;
}

// The repair of an aborted call, by the last workgroup to leave (every other one has gone, none
// stores anything any more except final values): the control block back to zero, then the row
// selected exactly on its own — three radix passes (exact_row's 11/11/9-bit digits) over the row
// in HBM, the elements at the K-th key ranked in index order (tie rule `tie_hi`) — and the whole
// dense output written: the same function of the row as the resident selection, bit for bit.
// (32-bit indices: d * 4 < 2^31; the row state words st[0..3] = thr, krem, tiecut, flags.)
__device__ inline void rs_repair(const float* x, uint32_t d, uint32_t K, uint32_t tie_hi, uint32_t* st_thr,
                                 uint32_t* st_krem, uint32_t* st_tiecut, uint32_t* st_flags, float* out,
                                 uint32_t* ctl, uint32_t* h, uint32_t* scratch, uint32_t* wsum) {
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    constexpr uint32_t RU4 = 4;                                        // float4 loads in flight a thread
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < (uint32_t)RS_CTL; i += RS_NT)                 // (RS_XGRP runs on: the host's xbase)
        if (i < (uint32_t)RS_XGRP || i >= (uint32_t)(RS_XGRP + 32 * RS_NG_MAX))
            __hip_atomic_store(ctl + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), (short)0, (int)(d * 4u), 0x00020000);
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(out, (short)0, (int)(d * 4u), 0x00020000);
    const uint32_t d4 = (d + 3u) / 4u;
    uint32_t prefix = 0, krem = K, ties = 0;
    for (int p = 0; p < 3; ++p) {
        for (uint32_t i = t; i < (uint32_t)HBINS; i += RS_NT) h[i] = 0;
        __syncthreads();
        for (uint32_t f0 = t; f0 < d4; f0 += RU4 * RS_NT) {
            u4v q[RU4];
#pragma unroll
            for (uint32_t u = 0; u < RU4; ++u)                          // past the row: zeros, not counted
                q[u] = __builtin_amdgcn_raw_buffer_load_b128(rx, (f0 + u * RS_NT) * 16u, 0, 0);
#pragma unroll
            for (uint32_t u = 0; u < RU4; ++u)
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e) {
                    const uint32_t k = q[u][e] & 0x7FFFFFFFu;
                    if ((f0 + u * RS_NT) * 4u + e < d && key_in_prefix(k, p, prefix)) atomicAdd(&h[key_bin(k, p)], 1u);
                }
        }
        __syncthreads();
        uint32_t bin, above;
        hist_find(h, krem, bin, above, scratch);
        prefix = (prefix << pass_bits(p)) | bin;
        krem -= above;
        if (p == 2) ties = h[bin];                                     // the row's keys == the K-th
        __syncthreads();
    }
    const uint32_t thr = prefix;
    const bool cut = ties > krem;
    const uint32_t from = tie_hi ? ties - krem : 0u, to = tie_hi ? ties : krem;
    uint32_t run = 0;                                                  // ties in index order so far
    for (uint32_t b = 0; b < d4; b += RS_NT) {
        const uint32_t f = b + t;
        const u4v q = __builtin_amdgcn_raw_buffer_load_b128(rx, f * 16u, 0, 0);
        uint32_t ne = 0;
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) ne += (f * 4u + e < d && (q[e] & 0x7FFFFFFFu) == thr) ? 1u : 0u;
        uint32_t tot;
        uint32_t r = run + ex_scan<RS_NT>(ne, wsum, tot);
        u4v o;
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
            const uint32_t k = q[e] & 0x7FFFFFFFu;
            const bool eq = f * 4u + e < d && k == thr;
            const bool keep = k > thr || (eq && (!cut || (r >= from && r < to)));
            r += eq ? 1u : 0u;
            o[e] = keep ? q[e] : 0u;
        }
        if (f < d4) __builtin_amdgcn_raw_buffer_store_b128(o, ro, f * 16u, 0, 0);   // (range-checked: the row end)
        run += tot;
    }
    if (t == 0) {
        *st_thr = thr;
        *st_krem = krem;
        *st_tiecut = 0;
        *st_flags = F_RESIDENT | F_REPAIR | (cut ? F_TIES : 0u);
    }
}

#ifdef FLC_RS_PRINT                       // probe builds: phase stamps of workgroup 0 (printf)
#define RS_STAMP(i) do { if (threadIdx.x == 0) stamp[i] = (uint64_t)wall_clock64(); } while (0)
#else
#define RS_STAMP(i) do { } while (0)
#endif
template <int RU>
__global__ __launch_bounds__(RS_NT) void k_lone_resident(RowSrc rows, int64_t d, int64_t K, SelWs ws,
                                                          float* __restrict__ out, int e4, uint32_t* __restrict__ ctl,
                                                          uint32_t seq, uint64_t spin, uint32_t xbase) {
    __shared__ uint32_t h[HBINS];
    __shared__ uint32_t scratch[260];
    __shared__ uint32_t wsum[RS_NT / 64];
    __shared__ uint32_t flag_s, gen_s, ok_s, lcnt_s;
    __shared__ uint64_t lst[RS_CAP];                                     // this workgroup's listed elements
    const uint32_t G = gridDim.x, g = blockIdx.x, t = threadIdx.x;
#ifdef FLC_RS_PRINT
    uint64_t stamp[18] = {0};
    // every 16th call, workgroup 0 summarises the PREVIOUS call's per-workgroup timeline (complete:
    // that launch has ended), so that the stamps are of back-to-back calls, not of a cold launch
    if (g == 0 && t == 0 && (seq & 15u) == 0u && G <= 256u) {
        const uint64_t* pr = reinterpret_cast<const uint64_t*>(ctl + RS_PROBE);
        const int ks[7] = {FLC_RS_TLK};
        uint64_t s0 = ~0ull;
        for (uint32_t i = 0; i < G; ++i) { const uint64_t v = pr[i]; s0 = v < s0 ? v : s0; }
        uint32_t mg = 0;
        for (uint32_t i = 0; i < G; ++i) if (pr[7 * 256 + i]) mg = i;
        printf("rs_tl G=%u merger %u (x10ns from the first start): ", G, mg);
        for (int k = 0; k < 7; ++k) {
            uint64_t mn = ~0ull, mx = 0, sum = 0;
            for (uint32_t i = 0; i < G; ++i) {
                const uint64_t v = pr[k * 256 + i] - s0;
                mn = v < mn ? v : mn; mx = v > mx ? v : mx; sum += v;
            }
            printf("s%d %llu/%llu/%llu ", ks[k], mn, sum / G, mx);
        }
        printf("\n");
    }
#endif
    RS_STAMP(0);
    RsTree tr;
    tr.ctl = ctl;
    tr.grp = g % RS_NG;
    tr.ngr = min(G, (uint32_t)RS_NG);
    tr.gsz = (G - tr.grp + RS_NG - 1) / RS_NG;
    // Counted out after the workgroup's last wait and before its stores: one non-returning add to
    // its group's RS_XGRP counter (thread 0; one counter for the grid serialised ~245 atomics on one
    // address and held the kernel's end ~1 us).  The counters run over the library's launches on
    // this control block; the host passes xbase, the workgroups of its earlier launches, so the
    // repairer knows when this call's others are out (sum - xbase == G - 1) and a clean call needs
    // to know nothing.
    auto count_out = [&]() {
        // (after this lane's counter adds have landed: a repair zeroes the counters once all are out)
        if (t == 0 && !FLC_RS_FENCE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (t == 0 && !FLC_RS_PROBE_NOCOUNT)
            __hip_atomic_fetch_add(ctl + RS_XGRP + 32 * tr.grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // what an aborted workgroup needs at its exit, stashed in LDS at the start: kept in registers to
    // the end, these arguments spilled SGPRs all through the dense stores (820 spill slots, not 81)
    struct RsExit {
        const float* x;
        float* out;
        uint32_t* ctl;
        uint32_t *thr, *krem, *tiecut, *flags;
        uint32_t d, K, tie_hi, seq, G, xbase;
        uint64_t spin;
    };
    __shared__ RsExit ex_s;
    __shared__ uint32_t rep_s;                                          // 1: this workgroup repairs the call
    if (t == 0) {
        rep_s = 0;
        lcnt_s = 0;
        ex_s = RsExit{rows.row_s(0), out, ctl, ws.thr, ws.krem, ws.tiecut, ws.flags, (uint32_t)d, (uint32_t)K, ws.tie_hi, seq,
                      G, xbase, spin};
    }
    const uint32_t nb = (uint32_t)(d * 4);                               // d <= RS_U * 4096 * CUs
    // the output's descriptor, rebuilt where the stores are from the LDS copy of the arguments (one
    // kept from here to the end of the kernel was spilled and shuffled around every store)
    auto out_rsrc = [&]() {
        const uint64_t op = reinterpret_cast<uint64_t>(ex_s.out);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)op), hi = __builtin_amdgcn_readfirstlane((uint32_t)(op >> 32));
        const uint32_t nbx = __builtin_amdgcn_readfirstlane(ex_s.d * 4u);
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(((uint64_t)hi << 32) | lo), (short)0, (int)nbx, 0x00020000);
    };
    // float4 u of this thread: elements 4 (g e4 RS_NT + u RS_NT + t) + q, coalesced over the threads;
    // index order inside the workgroup is (u, t, q), workgroups in order (G = ceil(d / (4 e4 RS_NT))).
    // A thread's float4 u < uv lie (at least partly) inside the row; the rest are skipped.  The one
    // float4 that straddles the row end holds pad = (-d) mod 4 elements of +0 (the range-checked
    // load): padding at the END of the index order, taken out of the counts of key 0 (bin 0 while
    // the digits so far are 0; the tie count of the workgroup holding it when the K-th key is 0),
    // never stored.  (Whole padding float4 counted into bin 0 serialised ~40 K LDS atomics on one
    // address in the last workgroups: 40 us.)
    const uint32_t f0 = g * (uint32_t)e4 * RS_NT + t;                   // float4 index of u = 0
    const int64_t d4 = (d + 3) / 4;                                      // float4 touching the row
    const int uv = (int)min((int64_t)e4, max((int64_t)0, (d4 - (int64_t)f0 + RS_NT - 1) / RS_NT));
    const uint32_t pad = (uint32_t)((4 - (d & 3)) & 3);
    const uint32_t padg = (uint32_t)((d / 4) / ((int64_t)e4 * RS_NT));  // the workgroup holding it
    const uint32_t voff = f0 * 16u;
    // the speculative first digit (rows of >= 4 RS_SS elements): a fixed sample of RS_SS elements
    // (32 spread pieces of 256), the same in every workgroup, loaded BEFORE the row so that it lands
    // first (vmcnt retires in order) and its digit is picked while the row streams in
    const bool spec = FLC_RS_SPEC && d >= 4 * (int64_t)RS_SS;
    // the release word's generation for the first round, loaded before everything else (by every
    // thread, unconditionally): its wait then does not drain the row's loads (vmcnt is in order)
    // (raw: the generation is masked out where it is used, so nothing waits for this load early)
    const uint64_t gen_word = __hip_atomic_load(reinterpret_cast<const uint64_t*>(ctl + RS_GEN), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the sample's loads unconditionally (an empty descriptor when there is no speculation: zeros,
    // no memory access), so that no branch makes the compiler wait for them before the row's loads
    const int64_t spos = spec ? (int64_t)(t >> 5) * (d - 256) / 31 + (int64_t)(t & 31) * 8 : 0;
    const auto rsm = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rows.row_s(0)), (short)0, spec ? (int)nb : 0, 0x00020000);
    const auto sa = __builtin_amdgcn_raw_buffer_load_b128(rsm, (uint32_t)(spos * 4), 0, 0);
    const auto sb = __builtin_amdgcn_raw_buffer_load_b128(rsm, (uint32_t)(spos * 4 + 16), 0, 0);
    // the workgroup's part through a descriptor of its own extent: the loads past it (u >= e4, the
    // row end) return zeros without touching memory, so all RU are issued unconditionally and the
    // compiler's in-order vmcnt count stays exact (the sample's wait does not drain the row)
    const int64_t gb = (int64_t)g * e4 * RS_NT * 4;
    const auto rxg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rows.row_s(0)) + gb, (short)0,
                                                       (int)(min((int64_t)e4 * RS_NT * 4, d - gb) * 4), 0x00020000);
    float4 v[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
        const auto q = __builtin_amdgcn_raw_buffer_load_b128(rxg, t * 16u, u * RS_NT * 16, FLC_LOADPOL);
        v[u] = make_float4(__uint_as_float(q[0]), __uint_as_float(q[1]), __uint_as_float(q[2]), __uint_as_float(q[3]));
    }
#ifdef FLC_RS_PRINT
    if (t < 64) {                                                        // (probe: when wave 0's row has landed)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        RS_STAMP(4);
    }
#endif
#if defined(FLC_RS_EXIT) && FLC_RS_EXIT == 3                             // (cost probe: the loads, then the row stored)
    {
        typedef unsigned int u4v __attribute__((ext_vector_type(4)));
        const uint64_t op = reinterpret_cast<uint64_t>(out);
        const auto rq = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(op), (short)0, (int)nb, 0x00020000);
#pragma unroll
        for (int u = 0; u < RU; ++u)
            if (u < uv) {
                const u4v ov = {__float_as_uint(v[u].x), __float_as_uint(v[u].y), __float_as_uint(v[u].z), __float_as_uint(v[u].w)};
                __builtin_amdgcn_raw_buffer_store_b128(ov, rq, voff, u * RS_NT * 16, FLC_RS_STPOL);
            }
        return;
    }
#endif
#if defined(FLC_RS_EXIT) && FLC_RS_EXIT == 1                             // (cost probe: the loads only)
    {
        uint32_t a = 0;
#pragma unroll
        for (int u = 0; u < RU; ++u) a |= __float_as_uint(v[u].x);
        if (a == 0x7FFFFFFFu) out[0] = 1.f;
        return;
    }
#endif
    uint32_t prefix = 0, krem = (uint32_t)K, last = 0, bar = 0;
    bool cand = false;
    uint32_t bs = 0;
    int p0 = 0;
    // bit u: float4 u holds an element whose first digit is in the speculative window (bs +- 1);
    // the others were stored before the round's release when the guess hits (FLC_RS_SPECST)
    uint32_t winm = 0;
    bool sst = false;                                                    // (uniform) those stores made and final
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    if (spec) {
        __shared__ uint32_t h1[3 * HBINS];
        // the sample's first-digit histogram in RS_SR replicas, lane l adding to replica l mod
        // RS_SR (a padded stride: other banks) — the exponents crowd a Gaussian row's keys into a
        // few bins; but the conflicts are not on the path (8 replicas: 0.35 us slower a call)
        __shared__ uint32_t hs[RS_SR * (HBINS + 1)];
        const uint32_t gen = (uint32_t)gen_word & 7u;
        // (LDS-only barriers up to the row's histogram: the sample's digit is picked while the
        // row's loads are still in flight — a __syncthreads waits for them, ~7 us)
        for (int i = t; i < RS_SR * (HBINS + 1); i += RS_NT) hs[i] = 0;
        for (int i = t; i < 3 * HBINS; i += RS_NT) h1[i] = 0;
        lds_bar();
        {
            uint32_t* hr = hs + (t % RS_SR) * (HBINS + 1);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                atomicAdd(&hr[(sa[q] & 0x7FFFFFFFu) >> 20], 1u);
                atomicAdd(&hr[(sb[q] & 0x7FFFFFFFu) >> 20], 1u);
            }
        }
        lds_bar();
        for (int i = t; i < HBINS; i += RS_NT) {
            uint32_t c = 0;
#pragma unroll
            for (int r = 0; r < RS_SR; ++r) c += hs[r * (HBINS + 1) + i];
            h[i] = c;
        }
        lds_bar();
        RS_STAMP(5);
#if defined(FLC_RS_EXIT) && FLC_RS_EXIT == 2                             // (cost probe: loads + the sample's digit)
        if (h[t] == 0x7FFFFFFFu) out[0] = 1.f;
        return;
#endif
        uint32_t ab;
        const uint32_t rs = (uint32_t)min((int64_t)RS_SS, max((int64_t)1, (K * RS_SS + d / 2) / d));
        hist_find<true>(h, rs, bs, ab, scratch);                         // the sample's digit (uniform)
        lds_bar();
        RS_STAMP(6);
        // the second digit's histograms for the first digits bs - 1 .. bs + 1, and the count of keys
        // whose first digit is above them: with the K-th key's first digit among the three, that is
        // all the merger needs for both digits (the contended first-digit histogram — the exponents
        // crowd into few bins — is not built at all unless the guess misses)
        uint32_t km = 0x7FFFFFFFu;
        asm volatile("" : "+s"(km));
        // (per element: the key, its offset from the window's low end, one compare into the
        // histogram's exec mask, one into a ballot counted by the scalar unit — every VALU op a
        // row element costs is ~0.25 us of a launch with one 16-wave workgroup per CU)
        const uint32_t wlo = (bs - 1u) << 20, whi = (bs + 2u) << 20;   // the window: first digits bs-1 .. bs+1
        uint32_t abv = 0;                                                // keys above the window (wave total)
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            if (u < uv) {
                const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t k = __float_as_uint(e[q]) & km;
                    const uint32_t dd = k - wlo;                         // window bin = dd >> 9 (3 x 2048)
                    abv += (uint32_t)__popcll(__ballot(k >= whi));
                    if (dd < (3u << 20)) {
                        atomicAdd(&h1[dd >> 9], 1u);
                        winm |= 1u << u;
                    }
                }
            }
        }
        RS_STAMP(7);
        if (t == 0) scratch[0] = 0;
        __syncthreads();
        if ((t & 63) == 0 && abv) atomicAdd(&scratch[0], abv);
        __syncthreads();
        RS_STAMP(1);
#if defined(FLC_RS_EXIT) && FLC_RS_EXIT == 4                             // (cost probe: + the window histograms)
        if (scratch[0] == 0x7FFFFFFFu) out[0] = 1.f;
        return;
#endif
        // the float4 with no element in the window: final if the guess hits (first digit above the
        // window: kept, below: +0), stored while the round runs; a miss rewrites every float4 later
        auto spec_store = [&]() {
            if (!FLC_RS_SPECST) return;
            const auto ro = out_rsrc();
            // (opaque copies: the 16 per-float4 lane masks the compiler would otherwise compute
            // once and keep for the later store loops spilled SGPRs through the whole kernel)
            int uvx = uv;
            uint32_t wmx = winm;
            asm volatile("" : "+v"(uvx), "+v"(wmx));
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                if (u < uvx && !((wmx >> u) & 1u)) {
                    const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                    uint32_t o[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = (mag_key(e[q]) >> 20) > bs + 1u ? __float_as_uint(e[q]) : 0u;
                    const u4v ov = {o[0], o[1], o[2], o[3]};
                    // (the float4's offset in the VGPR operand: 16 scalar offsets kept live here
                    // spilled SGPRs through the whole kernel)
                    __builtin_amdgcn_raw_buffer_store_b128(ov, ro, voff + (uint32_t)(u * RS_NT * 16), 0, FLC_RS_STPOL);
                }
            }
        };
        uint32_t* gs = ctl + RS_HSPEC + tr.grp * 3 * HBINS;
        for (int i = t; i < 3 * HBINS; i += RS_NT)
            if (h1[i]) __hip_atomic_fetch_add(gs + i, h1[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == 0 && scratch[0]) __hip_atomic_fetch_add(ctl + RS_ABV + 32 * tr.grp, scratch[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++bar;
        // (the speculative stores: by the waves 1.. of the workgroups that wait, while they wait —
        // wave 0 polls, and a poll would queue behind stores of its own, so it stores all its
        // float4 at the end; the merger's after its release, its loads not queued behind them)
        if (FLC_RS_SPECST && t < 64) winm = 0xFFFFu;
        const bool mg_ = rs_arrive(tr, &flag_s, &gen_s, gen);
#if defined(FLC_RS_EXIT) && FLC_RS_EXIT == 5                             // (cost probe: + the flush and the arrival)
        return;
#endif
        if (mg_) {
            // the merger: the three second-digit histograms summed (all loads in flight at once) with
            // their totals; the first digit is the one of the three where the count from the top
            // reaches K (else the guess missed: the rounds start from the first digit), the second
            // from its histogram — both digits in ONE round
            RS_STAMP(2);
#ifdef FLC_RS_PRINT
            stamp[13] = 1;
#endif
            // every replica word loaded at once (RS_NG x 3 x HBINS / RS_NT a thread, one round trip),
            // then added into h1 (its own counts first cleared) by LDS atomics
            uint32_t* s0 = ctl + RS_HSPEC;
            constexpr int ML = RS_NG * 3 * HBINS / RS_NT;
            uint32_t mv[ML];
#pragma unroll
            for (int j = 0; j < ML; ++j) mv[j] = __hip_atomic_load(s0 + t + j * RS_NT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t ar = t < RS_NG ? __hip_atomic_load(ctl + RS_ABV + 32 * t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            for (int i = t; i < 3 * HBINS; i += RS_NT) h1[i] = 0;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < ML; ++j) {
                const int i = (t + j * RS_NT) % (3 * HBINS);
                if (mv[j]) atomicAdd(&h1[i], mv[j]);
            }
            if (t < 64) {
                const uint32_t a4 = wave_sum(ar);
                if (t == 0) scratch[259] = a4;
            }
            __syncthreads();
            if (t < 2) {                                                 // the padding: first digit 0, second 0
                if (bs + (uint32_t)t == 1u) h1[t * HBINS] -= pad;
            }
            __syncthreads();
            const uint32_t A = scratch[259];
            // the three windows in index order w 0, 1, 2 are first digits bs - 1, bs, bs + 1: from the
            // top, h1's 3 x 2048 bins descend through both digits at once — one search finds both
            uint32_t bb = 0, ab = 0;
            bool found = false;
            if (A < (uint32_t)K) hist_find_n<3 * HBINS>(h1, (uint32_t)K - A, bb, ab, found, scratch);   // (uniform)
            uint64_t pl = 0;                                             // miss: start from the first digit
            if (found) {
                const uint32_t w0 = bb / HBINS, b1 = bb % HBINS, b0 = bs - 1u + w0;
                // hit | 22-bit prefix << 1 | krem << 23 | the prefix's count (saturated) << 47
                pl = 1ull | ((uint64_t)((b0 << 11) | b1) << 1) | ((uint64_t)((uint32_t)K - A - ab) << 23) |
                     ((uint64_t)min(h1[bb], 16383u) << 47);
            }
            rs_release(tr, &gen_s, pl);
            if (t == 0) { scratch[0] = (uint32_t)pl; scratch[1] = (uint32_t)(pl >> 32); }
            RS_STAMP(3);
            spec_store();
            if (t < RS_NG) __hip_atomic_store(ctl + RS_ABV + 32 * t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int i = t; i < 3 * RS_NG * HBINS; i += RS_NT)           // clean for the next call
                __hip_atomic_store(s0 + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            RS_STAMP(2);
            spec_store();
            if (!rs_wait(tr, &gen_s, scratch, &ok_s, &rep_s, spin, seq, true)) goto leave;
        }
        // (raw barriers: a __syncthreads here would drain the speculative stores first)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const uint64_t pl = ((uint64_t)scratch[1] << 32) | scratch[0];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (pl & 1u) {
            prefix = (uint32_t)(pl >> 1) & 0x3FFFFFu;
            krem = (uint32_t)(pl >> 23) & 0xFFFFFFu;
            last = (uint32_t)(pl >> 47);
            p0 = 2;
            cand = last <= (uint32_t)RS_CAP;
            sst = FLC_RS_SPECST;
        }
#if defined(FLC_RS_EXIT) && FLC_RS_EXIT == 6                             // (cost probe: + the merger and the release)
        return;
#endif                                                                // (else p0 = 0: the full rounds)
        RS_STAMP(3);
    }
    for (int p = p0; p < 3 && !cand; ++p) {
        const uint32_t gen = (p == 0 && !spec) ? ((uint32_t)gen_word & 7u) : (t == 0 ? rs_gen(tr) : 0u);
        for (int i = t; i < HBINS; i += RS_NT) h[i] = 0;
        __syncthreads();
        // an opaque copy of the key mask per pass: keeps the compiler from hoisting the 4 RU keys out
        // of the pass loop into as many more VGPRs (spills at 128)
        uint32_t km = 0x7FFFFFFFu;
        asm volatile("" : "+s"(km));
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            if (u < uv) {
                const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t k = __float_as_uint(e[q]) & km;
                    if (key_in_prefix(k, p, prefix)) atomicAdd(&h[key_bin(k, p)], 1u);
                }
            }
        }
        __syncthreads();
        RS_STAMP(1 + 3 * p);
        uint32_t* gh = ctl + RS_HREP + (p * RS_NG + tr.grp) * HBINS;
        for (int i = t; i < HBINS; i += RS_NT)
            if (h[i]) __hip_atomic_fetch_add(gh + i, h[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++bar;
        if (rs_arrive(tr, &flag_s, &gen_s, gen)) {
            // the merger: the replicas summed, the digit picked, the result released with the
            // generation; the replicas cleared for the next call after that (off the critical path)
            RS_STAMP(2 + 3 * p);
            uint32_t* r0 = ctl + RS_HREP + p * RS_NG * HBINS;
            for (int i = t; i < HBINS; i += RS_NT) {
                uint32_t c = 0;
#pragma unroll
                for (int r = 0; r < RS_NG; ++r) c += __hip_atomic_load(r0 + r * HBINS + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                h[i] = (i == 0 && prefix == 0u) ? c - pad : c;
            }
            __syncthreads();
            uint32_t bin, above;
            hist_find(h, krem, bin, above, scratch);
            const uint64_t pl = rs_digit(bin, above, h[bin]);
            rs_release(tr, &gen_s, pl);
            if (t == 0) { scratch[0] = (uint32_t)pl; scratch[1] = (uint32_t)(pl >> 32); }
            for (int i = t; i < HBINS; i += RS_NT)
#pragma unroll
                for (int r = 0; r < RS_NG; ++r) __hip_atomic_store(r0 + r * HBINS + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            RS_STAMP(2 + 3 * p);
            if (!rs_wait(tr, &gen_s, scratch, &ok_s, &rep_s, spin, seq)) goto leave;
        }
        __syncthreads();
        const uint64_t pl = ((uint64_t)scratch[1] << 32) | scratch[0];
        const uint32_t bin = (uint32_t)pl & 0x7FFu, above = (uint32_t)(pl >> 11) & 0xFFFFFFu;
        last = (uint32_t)(pl >> 35);
        prefix = (prefix << pass_bits(p)) | bin;
        krem -= above;
        __syncthreads();
        RS_STAMP(3 + 3 * p);
        if (p == 1 && last <= (uint32_t)RS_CAP) { cand = true; break; }  // (uniform) the candidate finish
    }
    if (cand) {
        // Candidate finish (after two digits, the K-th key's 22-bit prefix P holding <= RS_CAP
        // elements): keys above P are kept, below dropped, and the elements AT P — the K-th and its
        // equals — are stored as +0 now and listed (value bits, index); the last workgroup to arrive
        // ranks the list by (key desc, tie order), stores the krem first and writes the row state.
        // The third digit's round and the tie counts' exchange are not needed; nobody waits for the
        // ranking.  (The padding of the straddling float4 is never listed.)
        const uint32_t P = prefix;
        const uint32_t plo = P << 9;                                     // keys at P: [plo, plo + 512)
        // the listed elements into this workgroup's LDS list at positions from an LDS counter
        // (~70 in a 10 M row: the rare atomics cost less than a counting pass and a scan over
        // every element), then wave 0 hands them over: the first RS_CS into this workgroup's own
        // slots (no shared counter on the path: 245 returning adds on one word serialised ~3 us),
        // any beyond them into the shared list at a reserved offset, the count into its count word
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            if (u < uv) {
                const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (mag_key(e[q]) - plo < 512u) {
                        const uint32_t j = (f0 + u * RS_NT) * 4u + (uint32_t)q;
                        if ((int64_t)j < d) {                            // (not the straddling float4's padding)
                            const uint32_t pp = atomicAdd(&lcnt_s, 1u);
                            if (pp < (uint32_t)RS_CAP) lst[pp] = ((uint64_t)__float_as_uint(e[q]) << 32) | j;
                        }
                    }
                }
            }
        }
        lds_bar();
        const uint32_t ctot = lcnt_s;                                    // (uniform)
        RS_STAMP(9);
        if (FLC_RS_DONE && t < 64 && ctot) {
            // (the workgroups without candidates — nearly all — store nothing here)
            uint64_t* cl = reinterpret_cast<uint64_t*>(ctl + RS_CLIST);
            uint32_t ob = 0;
            if (t == 0) ob = __hip_atomic_fetch_add(ctl + RS_CCNT, ctot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t obase = __shfl(ob, 0, 64);
            const uint32_t nl = min(ctot, (uint32_t)RS_CAP);
            for (uint32_t i = t; i < nl; i += 64)
                if (obase + i < (uint32_t)RS_CAP) __hip_atomic_store(cl + obase + i, lst[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (t == 0) __hip_atomic_fetch_add(ctl + RS_CDONE, ctot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!FLC_RS_DONE && t < 64) {
            uint64_t* cl = reinterpret_cast<uint64_t*>(ctl + RS_CLIST);
            uint64_t* cr = reinterpret_cast<uint64_t*>(ctl + RS_CREG) + (size_t)g * RS_CS;
            uint32_t ob = 0;
            if (ctot > (uint32_t)RS_CS && t == 0)
                ob = __hip_atomic_fetch_add(ctl + RS_CCNT, ctot - (uint32_t)RS_CS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t obase = __shfl(ob, 0, 64);
            const uint32_t nl = min(ctot, (uint32_t)RS_CAP);
            for (uint32_t i = t; i < nl; i += 64) {
                const uint64_t en = lst[i];
                if (i < (uint32_t)RS_CS) __hip_atomic_store(cr + i, en, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else if (obase + i - RS_CS < (uint32_t)RS_CAP)
                    __hip_atomic_store(cl + obase + i - RS_CS, en, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (t == 0) __hip_atomic_store(ctl + RS_CNUM + g, ctot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        // the dense output without the listed positions (the ranking workgroup writes those); with
        // the speculative stores made, only the float4 holding a window element are left
        auto dense = [&]() {
            const auto ro = out_rsrc();
            int uvx = uv;
            uint32_t wmx = sst ? winm : 0xFFFFu;
            asm volatile("" : "+v"(uvx), "+v"(wmx));
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                if (u < uvx && ((wmx >> u) & 1u)) {
                    const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                    uint32_t o[4];
                    bool at[4], any = false;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const uint32_t k = mag_key(e[q]);
                        o[q] = k >= plo + 512u ? __float_as_uint(e[q]) : 0u;
                        at[q] = k - plo < 512u;
                        any |= at[q];
                    }
                    if (!any) {
                        const u4v ov = {o[0], o[1], o[2], o[3]};
                        __builtin_amdgcn_raw_buffer_store_b128(ov, ro, voff, u * RS_NT * 16, FLC_RS_STPOL);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (!at[q]) __builtin_amdgcn_raw_buffer_store_b32(o[q], ro, voff + 4u * q, u * RS_NT * 16, FLC_RS_STPOL);
                    }
                }
            }
        };
        RS_STAMP(10);
        // the hand-over drained (wave 0), then the workgroup counts out (its last hand-off) and
        // every wave stores its dense output — except the ranking workgroup (the last one: its
        // slice of the row is the shortest), which stores its dense output, waits until the
        // others are out, then ranks the list
        if (g != G - 1u) {
            count_out();
            lds_bar();                                                   // (nothing stored before the count-out)
#if defined(FLC_RS_EXIT) && FLC_RS_EXIT == 7                             // (cost probe: all but the others' dense stores)
            return;
#endif
            dense();
        } else {
            if (!FLC_RS_RANKFIRST) dense();
            // (everything below from the LDS copy of the arguments: kept in registers across the
            // dense stores they spill SGPRs all through them)
            const RsExit ex = ex_s;
            if (t == 0) {
                const uint64_t t0 = (uint64_t)wall_clock64();
                uint32_t okw = 1;
                for (;;) {
                    if (FLC_RS_DONE) {
                        // (every candidate delivered; more than `last` would be a list that does
                        // not add up: the check below aborts it)
                        if (__hip_atomic_load(ex.ctl + RS_CDONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= last) break;
                    } else {
                        uint32_t out_n = 0;
#pragma unroll
                        for (int r = 0; r < RS_NG; ++r)
                            out_n += __hip_atomic_load(ex.ctl + RS_XGRP + 32 * r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (out_n - ex.xbase >= ex.G - 1u) break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                    if ((uint64_t)wall_clock64() - t0 > ex.spin) {                 // (never seen: all ran the round)
                        if (__hip_atomic_exchange(ex.ctl + RS_GAVE, ex.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ex.seq) rep_s = 1;
                        okw = 0;
                        break;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");          // (compiler order only)
                ok_s = okw;
            }
            __syncthreads();
            if (!ok_s) goto leave;
            // the list: every workgroup's count and slots (one thread each, all loads at once; slots
            // beyond a count are stale and unused), then the shared list's overflow entries — m
            // entries in all, every element at P (checked: a list that does not add up aborts the
            // call and the repair selects the row), ranked by (key desc, tie order)
            __shared__ uint64_t comp[RS_CAP];
            __shared__ uint64_t ent[RS_CAP];
            __shared__ uint64_t kth_s;
            uint32_t m, ns, ovn, mm;
            bool ok;
            if (FLC_RS_DONE) {
                // the shared list holds exactly the `last` candidates (delivered count and reserved
                // count agree), read in one pass
                if (t == 0) {
                    scratch[4] = __hip_atomic_load(ex.ctl + RS_CCNT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    scratch[5] = __hip_atomic_load(ex.ctl + RS_CDONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __syncthreads();
                m = scratch[4];
                ok = m == last && scratch[5] == last && m >= krem && krem >= 1u && m <= (uint32_t)RS_CAP;
                mm = ok ? m : 0u;
                for (uint32_t i = t; i < mm; i += RS_NT)
                    ent[i] = __hip_atomic_load(reinterpret_cast<const uint64_t*>(ex.ctl + RS_CLIST) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ovn = 1u;                                                // (the reserved count to reset below)
            } else {
            uint32_t c = 0;
            uint64_t sl[RS_CS];
            if (t < ex.G) {
                c = __hip_atomic_load(ex.ctl + RS_CNUM + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint64_t* ct = reinterpret_cast<const uint64_t*>(ex.ctl + RS_CREG) + (size_t)t * RS_CS;
#pragma unroll
                for (int k = 0; k < RS_CS; ++k) sl[k] = __hip_atomic_load(ct + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const uint32_t ov = t == 0 ? __hip_atomic_load(ex.ctl + RS_CCNT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            if (t == 0) scratch[4] = ov;
            const uint32_t cs = min(c, (uint32_t)RS_CS);
            (void)ex_scan<RS_NT>(c, wsum, m);                            // (also the barrier before scratch[4])
            const uint32_t sp = ex_scan<RS_NT>(cs, wsum, ns);
            ovn = scratch[4];
            ok = m == last && ovn == m - ns && m >= krem && krem >= 1u && m <= (uint32_t)RS_CAP;
            mm = ok ? m : 0u;
            if (ok) {
#pragma unroll
                for (int k = 0; k < RS_CS; ++k)
                    if ((uint32_t)k < cs) ent[sp + k] = sl[k];
                for (uint32_t i = t; i < ovn; i += RS_NT) ent[ns + i] = __hip_atomic_load(reinterpret_cast<const uint64_t*>(ex.ctl + RS_CLIST) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            }
            if (t == 0) { scratch[2] = 0; scratch[3] = 0; kth_s = ~0ull; }
            __syncthreads();
            for (uint32_t i = t; i < mm; i += RS_NT) {
                const uint64_t en = ent[i];
                comp[i] = ((uint64_t)((uint32_t)(en >> 32) & 0x7FFFFFFFu) << 32) | tie_pref((uint32_t)en, ex.tie_hi);
            }
            __syncthreads();
            for (uint32_t i = t; i < mm; i += RS_NT) {
                const uint64_t me = comp[i];
                uint32_t rank = 0;
                for (uint32_t jj = 0; jj < mm; ++jj) rank += comp[jj] > me ? 1u : 0u;
                if (rank == krem - 1u) kth_s = me;                       // entries are distinct
            }
            __syncthreads();
            const uint64_t kc = kth_s;
            const uint32_t kth = (uint32_t)(kc >> 32);
            for (uint32_t i = t; i < mm; i += RS_NT) {
                const uint64_t me = comp[i];
                const uint64_t en = ent[i];
                ex.out[(uint32_t)en] = me >= kc ? __uint_as_float((uint32_t)(en >> 32)) : 0.f;
                const uint32_t key = (uint32_t)(me >> 32);
                if (key > kth) atomicAdd(&scratch[2], 1u);
                else if (key == kth) atomicAdd(&scratch[3], 1u);
            }
            __syncthreads();
            if (t == 0) {
                if (ovn) __hip_atomic_store(ex.ctl + RS_CCNT, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // clean for the next call
                if (FLC_RS_DONE) __hip_atomic_store(ex.ctl + RS_CDONE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t gt = scratch[2], eq = scratch[3];
                *ex.thr = kth;
                *ex.krem = krem - gt;
                *ex.tiecut = tie_pref((uint32_t)kc, ex.tie_hi);
                *ex.flags = F_RESIDENT | (gt + eq > krem ? F_TIES : 0u);
                if (!ok && __hip_atomic_exchange(ex.ctl + RS_GAVE, ex.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ex.seq)
                    rep_s = 1;
            }
            if (!ok) goto leave;                                         // (uniform) aborted: repaired
            if (t == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_fetch_add(ex.ctl + RS_XGRP + 32 * (blockIdx.x % RS_NG), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (FLC_RS_RANKFIRST) dense();
        }
        RS_STAMP(11);
    } else {
    // thr = the K-th key; krem of the `last` elements equal to it are kept
    const uint32_t thr = prefix;
    const bool tie_cut = last > krem;                                    // uniform over the grid
    uint64_t tmask = 0;                                                  // kept ties: bit 4 u + q
    if (tie_cut) {
        // this workgroup's ties (its padding, at its end, is not one), published as (call seq << 32 |
        // count); a workgroup holding ties sums the counts of the workgroups before it (waiting for
        // each to be published: all publish right after the last digit, so no barrier round) and
        // ranks its own in (u, t, q) order; the others have nothing to rank
        uint32_t c = 0;
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            if (u < uv) {
                const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) c += mag_key(e[q]) == thr ? 1u : 0u;
            }
        }
        uint32_t tot;
        (void)ex_scan<RS_NT>(c, wsum, tot);
        if (thr == 0u && g == padg) tot -= pad;
        uint64_t* tc = reinterpret_cast<uint64_t*>(ctl + RS_TCNT);
        if (t == 0) __hip_atomic_store(tc + g, ((uint64_t)seq << 32) | tot, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (tot == 0u) goto store;                                       // (uniform) no tie here
        uint32_t part = 0, run = 0;
        int bail = 0;
        const uint64_t t0 = (uint64_t)wall_clock64();
        for (uint32_t i = t; i < g && !bail; i += RS_NT) {
            uint64_t w;
            for (;;) {
                w = __hip_atomic_load(tc + i, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t a = __hip_atomic_load(ctl + RS_GAVE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((uint32_t)(w >> 32) == seq) break;
                if (a == seq) { bail = 1; break; }                       // aborted elsewhere
                __builtin_amdgcn_s_sleep(1);
                if ((uint64_t)wall_clock64() - t0 > spin) {             // a workgroup before is not running
                    if (__hip_atomic_exchange(ctl + RS_GAVE, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != seq)
                        rep_s = 1;                                       // (one thread of the grid)
                    bail = 1;
                    break;
                }
            }
            part += (uint32_t)w;
        }
        if (__syncthreads_or(bail)) goto leave;                          // (uniform) the call is aborted
        (void)ex_scan<RS_NT>(part, wsum, run);                           // ties in the workgroups before
        const uint32_t tie_from = ws.tie_hi ? last - krem : 0u, tie_to = ws.tie_hi ? last : krem;
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            if (u < e4) {                                                // (uniform: ex_scan inside)
                const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                uint32_t ce = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) ce += (u < uv && mag_key(e[q]) == thr) ? 1u : 0u;
                uint32_t tu;
                uint32_t r = run + ex_scan<RS_NT>(ce, wsum, tu);
                run += tu;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (u < uv && mag_key(e[q]) == thr) {
                        if (r >= tie_from && r < tie_to) tmask |= 1ull << (4 * u + q);
                        ++r;
                    }
            }
        }
    }
store:
    RS_STAMP(10);
    // every wait of this workgroup is behind it: the row state (workgroup 0: released before it is
    // counted out, so that a repair's later state is the one that stays), counted out, then the
    // stores (final values)
    if (g == 0 && t == 0) {
#if FLC_RS_FENCE
        ws.thr[0] = thr;
        ws.krem[0] = krem;
        ws.tiecut[0] = 0;
        ws.flags[0] = F_RESIDENT | (tie_cut ? F_TIES : 0u);
        if (FLC_RS_G0REL) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#else
        // written through (agent-scope stores) and drained before the count-out, so that a
        // repair's later row state is the one that stays
        __hip_atomic_store(ws.thr, thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ws.krem, krem, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ws.tiecut, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ws.flags, F_RESIDENT | (tie_cut ? F_TIES : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    }
    count_out();
    // the dense output from the registers: x where kept, +0 elsewhere (range-checked: no padding);
    // with the speculative stores made, only the float4 holding a window element
    const auto ro = out_rsrc();
    int uvx = uv;
    uint32_t wmx = sst ? winm : 0xFFFFu;
    asm volatile("" : "+v"(uvx), "+v"(wmx));
#pragma unroll
    for (int u = 0; u < RU; ++u) {
        if (u < uvx && ((wmx >> u) & 1u)) {
            const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            uint32_t o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t k = mag_key(e[q]);
                const bool keep = k > thr || (k == thr && (!tie_cut || ((tmask >> (4 * u + q)) & 1ull)));
                o[q] = keep ? __float_as_uint(e[q]) : 0u;
            }
            const u4v ov = {o[0], o[1], o[2], o[3]};
            __builtin_amdgcn_raw_buffer_store_b128(ov, ro, voff, u * RS_NT * 16, FLC_RS_STPOL);
        }
    }
    RS_STAMP(11);
    (void)bar;
    }
    goto done;
leave:
    // An aborted workgroup (it left from a wait, or the ranking found the list inconsistent): its
    // control-block writes completed (release), then counted out — except the repairer (the first
    // to abort), which waits for every other workgroup of the call to be out, selects the row on
    // its own, rewrites the output and the row state, zeroes the control block, then counts out.
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    }
    if (!rep_s) count_out();
    __syncthreads();
    if (rep_s) {
        const RsExit ex = ex_s;
        if (t == 0) {
            // (bounded: every other workgroup leaves within its own waits' limit once it runs; a
            // grid that cannot drain at all after 64 of them is repaired anyway — its stragglers
            // never store anything but final values)
            const uint64_t t0 = (uint64_t)wall_clock64();
            for (;;) {
                uint32_t out_n = 0;
                for (int r = 0; r < RS_NG; ++r)
                    out_n += __hip_atomic_load(ex.ctl + RS_XGRP + 32 * r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (out_n - ex.xbase >= ex.G - 1u || (uint64_t)wall_clock64() - t0 >= 64 * ex.spin) break;
                __builtin_amdgcn_s_sleep(8);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        __syncthreads();
        rs_repair(ex.x, ex.d, ex.K, ex.tie_hi, ex.thr, ex.krem, ex.tiecut, ex.flags, ex.out, ex.ctl, h, scratch, wsum);
        __syncthreads();
        if (t == 0) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        count_out();
    }
done:;
#ifdef FLC_RS_PRINT
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    RS_STAMP(12);
    if (t == 0 && G <= 256u) {
        uint64_t* pr = reinterpret_cast<uint64_t*>(ex_s.ctl + RS_PROBE);
        const int ks[8] = {FLC_RS_TLK, 13};
        for (int k = 0; k < 8; ++k) __hip_atomic_store(pr + k * 256 + g, stamp[ks[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#endif
}

// k_lone_resident's control block (library-owned, one per device, zeroed once: the kernel leaves it
// clean) and the serialisation of its launches: two resident grids at once could each hold part of
// the chip and wait for the other forever, so a launch on another stream than the previous one
// waits for that one's completion event (one stream: stream order alone)
struct RsCtx {
    uint32_t* ctl = nullptr;
    uint32_t seq = 0;                   // launches so far (tags the tie counts of each call)
    uint32_t xcum = 0;                  // workgroups launched so far (the RS_XGRP counters' sum before a launch)
    hipStream_t last = nullptr;
    hipEvent_t done = nullptr;
};
static std::mutex g_rs_mu;
static std::map<int, RsCtx> g_rs_ctx;
// test hook (flc_debug_resident): the grid of the next resident launches x mult (workgroups that
// cannot all be resident: the abort + repair path, deterministically) and the waits' give-up time
static std::atomic<int> g_rs_dbg_mult{1};
static std::atomic<long long> g_rs_dbg_spin{0};
int rs_debug(int mult, int64_t spin_ticks) {
    if (mult < 1 || mult > 64 || spin_ticks < 0) { set_error("flc_debug_resident: mult 1..64, spin >= 0"); return FLC_ERR_ARG; }
    g_rs_dbg_mult.store(mult);
    g_rs_dbg_spin.store((long long)spin_ticks);
    return FLC_OK;
}
static int rs_cus() {              // compute units of the current device (one k_lone_resident workgroup each)
    static int cu[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (!cu[dev]) {
        int c = 0;
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        cu[dev] = c;
    }
    return cu[dev];
}

// k_lone_resident for a row of up to RS_U * 4096 elements per CU (any K): one launch.  *took = false,
// nothing launched, for a longer row: the list path takes it.
int lone_resident_launch(RowSrc rows, int64_t d, int64_t K, SelWs ws, float* out, hipStream_t st, bool* took) {
    const int64_t cus = rs_cus();
    const int mult = std::max(1, g_rs_dbg_mult.load());              // (test hook: > 1 forces an aborted call)
    const int64_t G = std::min<int64_t>(cus * mult, (d + RS_NT * 4 - 1) / (RS_NT * 4));
    const int64_t e4 = G > 0 ? (d + G * RS_NT * 4 - 1) / (G * RS_NT * 4) : RS_U + 1;
    if (!(e4 <= RS_U && d * 4 < ((int64_t)1 << 31))) return FLC_OK;
    const int64_t Gu = (d + e4 * RS_NT * 4 - 1) / (e4 * RS_NT * 4);   // no workgroup of padding only
    const long long dspin = g_rs_dbg_spin.load();
    const uint64_t spin = dspin > 0 ? (uint64_t)dspin : (uint64_t)FLC_RS_SPIN;
    ProfScope _ps("k_lone_resident", st);
    int dev = 0;
    FLC_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_rs_mu);
    RsCtx& rc = g_rs_ctx[dev];
    if (!rc.ctl) {
        FLC_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&rc.ctl), (size_t)RS_CTL * sizeof(uint32_t)));
        FLC_CHECK_HIP(hipMemsetAsync(rc.ctl, 0, (size_t)RS_CTL * sizeof(uint32_t), st));
        FLC_CHECK_HIP(hipEventCreateWithFlags(&rc.done, FLC_SYNC_EVENT_FLAGS));
    }
    if (rc.last && rc.last != st) {
        if (!FLC_RS_EVREC) FLC_CHECK_HIP(hipEventRecord(rc.done, rc.last));   // (probe builds)
        FLC_CHECK_HIP(hipStreamWaitEvent(st, rc.done, 0));
    }
    if (++rc.seq == 0u) rc.seq = 1u;                              // (0: no call; RS_GAVE's cleared value)
    const int e4i = (int)e4;
    if (FLC_RS_COOP) {
        RowSrc ra = rows;
        int64_t da = d, ka = K;
        SelWs wa = ws;
        float* oa = out;
        int ea = e4i;
        uint32_t* ca = rc.ctl;
        uint32_t sa = rc.seq;
        uint64_t pa = spin;
        uint32_t xa = rc.xcum;
        void* args[] = {&ra, &da, &ka, &wa, &oa, &ea, &ca, &sa, &pa, &xa};
        FLC_CHECK_HIP(hipLaunchCooperativeKernel(reinterpret_cast<const void*>(&k_lone_resident<RS_U>), dim3((unsigned)Gu),
                                                 dim3(RS_NT), args, 0, st));
    } else {
        hipLaunchKernelGGL((k_lone_resident<RS_U>), dim3((unsigned)Gu), dim3(RS_NT), 0, st, rows, d, K, ws, out, e4i,
                           rc.ctl, rc.seq, spin, rc.xcum);
    }
    FLC_CHECK_LAUNCH("k_lone_resident");
    rc.xcum += (uint32_t)Gu;                                      // (every workgroup counts out once)
    if (FLC_RS_EVREC) FLC_CHECK_HIP(hipEventRecord(rc.done, st));
    rc.last = st;
    *took = true;
    return FLC_OK;
}

}  // namespace flc
