// Private to the units of the selection core — select.hip (the host end), topk_filter.hip,
// topk_select.hip, lone_row.hip, randk.hip, chunk_accum.hip — and included by nothing else: the
// workspace structs, the block primitives, every FLC_* compile-time switch of those units (one
// definition for all of them, also under XFLAGS), TkCall and the host launchers that cross units.
// A kernel is defined in one unit together with every host function that launches it; only host
// functions cross.
//
// Sparsifying codecs: TopK (compressors.py:330-335) and RandK (240-245), dense single-vector
// encode and fused batch encode + reduce.
//
// Data flow of the batch path (N client rows x D, chunk = 4096 elements = one wave's tile):
//
//   TopK  sample   : one workgroup per row keys a spread sample (<= 16 K elements, LDS) and picks a
//                    conservative threshold T_lo with count(|x| >= T_lo) >= K w.h.p.
//         filter   : ONE pass over every row (the only full HBM read): entries with key >= T_lo
//                    are appended to the row's candidate list (idx, val), per chunk -> tab[c][row]
//         select   : exact K-th largest key among the candidates (3 radix passes, 11/11/9 bits)
//         fallback : rows whose list overflowed, came up short (sample unlucky), or whose K-th
//                    magnitude is tied ambiguously are redone exactly on the full row
//                    (3 radix passes + tie prefix + exact filter, ties -> lowest index first)
//   RandK device   : the device sampler (randk_tree.hpp) is generated chunk by chunk: per row the
//                    chunk counts (k_randk_counts, a hypergeometric tree), then one wave per chunk
//                    regenerates every row's members of its chunk, gathers (D/K) * x[j] and folds
//                    them in row order (k_randk_fold) — no index lists in memory; the only HBM
//                    traffic is the gathered 128-B lines and the [D] result
//   RandK compat   : the K numpy-stream indices of each row are bucketed by chunk in two coalesced
//                    levels — superchunks in one workgroup per row (LDS counts + multi-split),
//                    then chunks inside each superchunk (LDS counting sort) with the gather of
//                    (D/K) * x[j] in ascending order (k_randk_coarse / k_randk_fine)
//   accumulate     : one wave owns one chunk (or 1/2, 1/4 of it when the rows are short) as an
//                    fp32 LDS tile and folds the rows' admitted
//                    entries in row order -> (sum_i w_i C_i(x_i)) / w_total, bit-identical to the
//                    sequential reduction of the dense compressVector outputs (indices are
//                    distinct within a row, so every element sees its terms in row order).
//
// Keys: |x| bits with the sign cleared (uint32, monotone; NaN above inf like torch.topk).
#pragma once
#include <stdlib.h>

#include <atomic>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "chunks.hpp"
#include "randk_tree.hpp"

namespace flc {

constexpr uint32_t ALL = 0xFFFFFFFFu;
constexpr uint32_t F_OVERFLOW = 1u, F_SHORT = 2u, F_TIES = 4u, F_EXACT = 8u;
constexpr uint32_t F_RESIDENT = 16u;  // a lone row selected exactly in registers (k_lone_resident)
constexpr uint32_t F_REPAIR = 32u;    // ... whose grid was not co-resident: re-selected by its last workgroup
constexpr int SMAX = 16384;          // sample size kept in LDS
constexpr int HBINS = 2048;          // radix histogram bins (11 bits)
constexpr uint32_t TIECAP = HBINS;   // fast-path tie list (LDS); more ties at the K-th key -> exact path
constexpr int CS_SH = 64;            // few rows: shards of a row's candidate list (k_cs_pass workgroups)
constexpr int64_t CS_FEW = 16;       // rows: sharded lists + k_cs_pass up to here, else k_cand_select
constexpr int CS_ST = 8;             // words of a row's k_cs_pass state
constexpr int CS_LCAP = 2048;        // entries of the first digit's bin ranked directly (list mode)
constexpr int RS_U = 16;             // (<= 16: kept-tie mask of 64 bits) k_lone_resident: float4 of the row per thread at most (64 VGPRs)
constexpr int GCAP = 512;             // staged entries per group (4 chunks: 3.1 %, ~2.5x the mean at 1.2 %; more -> row overflow)
static_assert(GCAP % 64 == 0, "copy-out runs in whole wave slots");
constexpr int EX_NT = 1024;
constexpr int EX_U = 8;                      // float4 loads per thread in flight in the radix passes
constexpr int RK_SB = 256;                   // superchunks per row (max)
#ifndef FLC_RS_NG
#define FLC_RS_NG 4                   // k_lone_resident: workgroup groups (histogram replicas, barrier tree);
#endif                                // us a call at D = 10 M: 1 -> 57, 2 -> 53, 4 -> 52, 8 -> 54.6, 16 -> 60
constexpr int RS_NG = FLC_RS_NG;
constexpr int RS_NG_MAX = 16;
static_assert(RS_NG >= 1 && RS_NG <= RS_NG_MAX, "FLC_RS_NG: 1..16 groups");
// its control words: counters on lines of their own, per-group digit histograms, tie counts
// (RS_GAVE: the sequence number of a call that was aborted; RS_XGRP: workgroups that have left)
constexpr int RS_GLOB = 0, RS_GEN = 32, RS_GAVE = 64, RS_CCNT = 96, RS_CDONE = 112, RS_GRP = 128;
constexpr int RS_XGRP = RS_GRP + 32 * RS_NG_MAX;  // per group: workgroups counted out (runs on across calls)
constexpr int RS_ABV = RS_XGRP + 32 * RS_NG_MAX;   // per group: keys above the speculated first digits
constexpr int RS_CAP = 2048;          // candidates (22-bit prefix of the K-th key) ranked by the last workgroup
constexpr int RS_SS = 8192;           // the speculative first digit's sample (32 pieces of 256)
#ifndef FLC_RS_SR
#define FLC_RS_SR 1                   // replicas of the sample's histogram (LDS; 8 measured 0.35 us slower a call)
#endif
constexpr int RS_SR = FLC_RS_SR;
#ifndef FLC_RS_STPOL
#define FLC_RS_STPOL 2                // the dense output's stores: nontemporal (2) or default (0)
#endif
#ifndef FLC_RS_GACQ
#define FLC_RS_GACQ 1                 // k_lone_resident: a group's last arriver acquires before its release
#endif
#ifndef FLC_RS_POLLAB
#define FLC_RS_POLLAB 1               // k_lone_resident: a grid wait reads the abort word every n-th poll
#endif
#ifndef FLC_RS_DONE
// k_lone_resident's candidate hand-over: 1 = a workgroup holding candidates reserves their place in
// the shared list (one returning add), stores them and then adds their number to a delivered count;
// the ranking workgroup waits for that count to reach the candidates' total (known to all from the
// round's payload), not for every workgroup to count out, and reads the list in one pass.
// 0 = per-workgroup slots gathered after every workgroup counted out.
#define FLC_RS_DONE 1
#endif
#ifndef FLC_RS_RANKFIRST
#define FLC_RS_RANKFIRST 0            // 1: the ranking workgroup ranks before its own dense stores (measured 0.2 us slower)
#endif
#ifndef FLC_RS_PROBE_NOCOUNT
#define FLC_RS_PROBE_NOCOUNT 0        // (cost probes only: no exit count — an aborted call would not repair)
#endif
#ifndef FLC_RS_G0REL
#define FLC_RS_G0REL 1                // workgroup 0 releases the row state before it counts out
#endif
#ifndef FLC_RS_FENCE
// k_lone_resident's grid rounds: 1 = agent-scope release / acquire fences around the counters (an
// L2 write-back or L1 invalidate each, ~1.7 us; five on the last arriver's path); 0 = no fences —
// every byte handed over inside the launch is written by an agent-scope atomic (histogram adds,
// list entries, counters, the release word) and read by agent-scope (sc1) loads, every writing
// wave drains (vmcnt(0)) before its workgroup's one counter add, and the counters never need a
// reset store (see rs_arrive)
#define FLC_RS_FENCE 0
#endif
#ifndef FLC_RS_SPEC
#define FLC_RS_SPEC 1                 // k_lone_resident: speculative first digit (two digits in one round)
#endif
constexpr int RS_HREP = RS_ABV + 32 * RS_NG_MAX;
constexpr int RS_HSPEC = RS_HREP + 3 * RS_NG * HBINS;    // [RS_NG][3][HBINS] speculative second digit
constexpr int RS_CLIST = RS_HSPEC + 3 * RS_NG * HBINS;   // [RS_CAP] (value bits, index)
constexpr int RS_TCNT = RS_CLIST + 2 * RS_CAP;               // (tie counts: 64-bit (call << 32 | count) per workgroup)
constexpr int RS_GMAX = 1024;                                  // workgroups a launch may have (tie counts, list slots)
constexpr int RS_CS = 4;                                       // listed elements a workgroup keeps in slots of its own
constexpr int RS_CNUM = RS_TCNT + 2 * RS_GMAX;                 // [RS_GMAX] elements a workgroup listed (this call)
constexpr int RS_CREG = RS_CNUM + RS_GMAX;                     // [RS_GMAX][RS_CS] 64-bit (value bits, index)
#ifdef FLC_RS_PRINT
constexpr int RS_PROBE = RS_CREG + 2 * RS_CS * RS_GMAX;        // probe builds: per-workgroup phase stamps
constexpr int RS_CTL = RS_PROBE + 4096;
#else
constexpr int RS_CTL = RS_CREG + 2 * RS_CS * RS_GMAX;
#endif
#ifndef FLC_RS_SPECST
#define FLC_RS_SPECST 0               // 1: the dense output outside the speculative window stored during the round (slower: 42.5 vs 36.7 us, the writes delay the merger)
#endif
#ifndef FLC_CS_LIST
#define FLC_CS_LIST 1
#endif
#ifndef FLC_CS_TWO_MAXD
#define FLC_CS_TWO_MAXD (int64_t(64) << 20)   // rows up to this long: two k_cs_pass launches
#endif
// k_cand_select / k_cs_pass
// candidate values of a row, read twice per launch (measured: nt loads 0.335 -> 0.293 ms at C3)
#ifndef FLC_CS_NT
#define FLC_CS_NT 1
#endif
// the TopK filters and the row groups of the many-row path
#ifndef FLC_TK_STPOL
#define FLC_TK_STPOL 0               // A/B: the filter's list copy-out stores nontemporal (2) or default (0)
#endif
#ifndef FLC_TK_COPY4
#define FLC_TK_COPY4 1               // TopK filter copy-out: 16-B stores of whole quads
#endif
#ifndef FLC_TK_PROBE
#define FLC_TK_PROBE 0               // A/B cost probes (outputs NOT valid): 1 no staging writes, 2 no copy-out, 3 loads only,
                                     // 4 copy-out aimed at a small per-wave region that stays in the L2 (reservation and tab real)
#endif
#ifndef FLC_TK_RING
#define FLC_TK_RING 16               // loads in flight per wave (ring registers: 4 x RING VGPRs)
#endif
#ifndef FLC_TK_WPE
#define FLC_TK_WPE 1                 // unconstrained (143 VGPRs); 4 waves per SIMD spilled and ran slower
#endif
#ifndef FLC_TK_WG
#define FLC_TK_WG 1                   // many-row TopK filter: 1 workgroup items, 0 the per-wave groups of k_topk_filter_fast
#endif
#ifndef FLC_TK_WG_NL
#define FLC_TK_WG_NL 4                // loader waves (groups per item); the workgroup has one wave more (3: +0.02 ms at C3)
#endif
#ifndef FLC_TK_WG_RING
#define FLC_TK_WG_RING FLC_TK_RING    // loads in flight per loader wave (8: 73 VGPRs, four workgroups per CU, the same step time,
                                      // but the side stream's sample ran 1.19 instead of 0.14 ms beside it)
#endif
#ifndef FLC_TK_WG_STPOL
#define FLC_TK_WG_STPOL 17            // the writer's copy-out stores: sc0 sc1, written through the L2 at once: C3 -0.11 .. -0.18 ms
                                      // a step against k_topk_filter_fast, same allocation; 0 (default policy) -0.045, sc1 alone
                                      // as 17, sc0 -0.03, nt 0, sc1 nt / sc0 sc1 nt +0.12 (profiles/r07/wgfilter/)
#endif
#ifndef FLC_TK_WG_WPE
#define FLC_TK_WG_WPE 4               // 127 VGPRs: three 5-wave workgroups per CU (unconstrained: 129 VGPRs, two, +0.66 ms at C3)
#endif
#ifndef FLC_TK_SPLIT_SAMPLE
#define FLC_TK_SPLIT_SAMPLE 1         // TopK row groups: only group 0's sample before the first filter
#endif
#ifndef FLC_TK_LASTPCT
#define FLC_TK_LASTPCT 100            // size of the last TopK row group in % of the others (its tail is exposed)
#endif
static_assert(FLC_TK_LASTPCT >= 1 && FLC_TK_LASTPCT <= 100, "FLC_TK_LASTPCT: the last row group is 1..100 % of the others");
#ifndef FLC_TK_LAST_TS
#define FLC_TK_LAST_TS 4096           // the exposed last group fold's tile (columns per wave)
#endif
#ifndef FLC_TK_GFOLD
#define FLC_TK_GFOLD 1                // many-row TopK: fold each row group under the next group's filter
#endif
#ifndef FLC_TK_SIDE_NT
#define FLC_TK_SIDE_NT 512            // threads of the side-stream candidate selects (256 or 512)
#endif
#ifndef FLC_TK_EXACT_WG
#define FLC_TK_EXACT_WG 256           // workgroups of the one exact-rows launch (one per CU)
#endif
// the chunk-owner folds: k_chunk_accum (chunk_accum.hip), k_randk_fold (randk.hip)
#ifndef FLC_CA_PROBE
#define FLC_CA_PROBE 0               // A/B cost probe of k_chunk_accum (outputs NOT valid): 1 no tile update
#endif
#ifndef FLC_CA_AP1
#define FLC_CA_AP1 4                 // one-wave fold workgroups: rows in flight (<= 113 VGPRs: beside the TopK filter's 3 waves per SIMD)
#endif
#ifndef FLC_CA_WPB1
#define FLC_CA_WPB1 0                // k_chunk_accum over whole chunks: one-wave workgroups
#endif
#ifndef FLC_CA_AP
#define FLC_CA_AP 8
#endif
#ifndef FLC_RK_AP
#define FLC_RK_AP 8
#endif
// k_lone_resident's launch and the choice of the lone-row path
#ifndef FLC_RS_SPIN
#define FLC_RS_SPIN 10000000ull          // 0.1 s of the 100 MHz clock
#endif
#if defined(FLC_RS_PRINT) && !defined(FLC_RS_TLK)
#define FLC_RS_TLK 0, 4, 1, 2, 3, 10, 12   // the 7 stamps the timeline reports (13: the merger flag)
#endif
#ifndef FLC_LONE_PATH
#define FLC_LONE_PATH 2                // a lone compressVector row: 2 in registers (k_lone_resident, rows up to
#endif                                 // RS_U * 4096 per CU; longer: the list path), 0 the list path
#ifndef FLC_RS_EVREC
#define FLC_RS_EVREC 1                 // the completion event recorded after every resident launch (0: at a stream switch)
#endif
#ifndef FLC_RS_COOP
#define FLC_RS_COOP 0                  // 1: k_lone_resident launched cooperatively (HIP's launch: +22 us a call
#endif                                 // measured; residency holds anyway: G <= CUs, one workgroup per CU, launches serialised)

struct SelWs {            // carved from the caller workspace
    uint2* tab;           // [C][N] (offset, count) of each row's entries in chunk c
    uint32_t* ent_idx;    // [N][cap] element index within the row
    float* ent_val;       // [N][cap] entry value (already scaled for RandK)
    uint32_t* rowcnt;     // [N * RCS] entries used (one counter per 128 B line)
    uint32_t* flags;      // [N]
    uint32_t* thr;        // [N] admission key: entries with key >= thr are summed
    uint32_t* prefix;     // [N] radix-select state
    uint32_t* krem;       // [N]
    uint32_t* tieprefix;  // [C][N] ties (key == thr) in chunks before c   (exact path only)
    uint32_t* tiecut;     // [N] fast path, F_TIES: the last index admitted among key == thr (tie_pref order);
                          // rows selected by k_radix_select<FULLROW> (dense K): the count of keys == thr
    uint32_t* hist;       // [N][HBINS]
    uint32_t* worklist;   // [N] rows on the exact path
    uint32_t* nwork;      // [1]
    uint32_t* cursor;     // [C][N] RandK scatter cursors
    uint32_t* cstate;     // [N][CS_ST] few-row candidate select: shift, prefix, krem, stage, bin count, list fill (k_cs_pass)
    uint64_t* clist;      // [min(N, CS_FEW)][CS_LCAP] few rows: the first digit bin's entries (k_cs_pass list mode)
    uint32_t* carrive;    // [N * RCS] its per-row arrival counters
    uint32_t* shcnt;      // [N][CS_SH * RCS] few rows: the filter's reservation counters, one per shard
    uint32_t* zm;         // [C][CHUNK / 32] k_chunk_accum (one-wave blocks): a fold job's kept-column mask
    float* part;          // [D] TopK row-group folds: the running tiles carried from one group to the next
    int64_t cap;
    uint32_t tie_hi;      // TopK ties at the K-th key: 0 the lowest indices are kept (default), 1 the highest
};

// Tie order of TopK (flc_codec_params.tie): tie_pref(ix) is larger for the index kept first among
// equal magnitudes — ~ix for the lowest-index rule (the oracle's, torch.topk's CPU order on the
// reference's rows), ix for the highest-index rule.  A row's tie cut is the last kept tie's index:
// a tie is admitted iff tie_pref(ix) >= tie_pref(cut); tie_all(ws) is the cut that admits every tie.
__device__ __host__ inline uint32_t tie_pref(uint32_t ix, uint32_t hi) { return hi ? ix : ~ix; }
__device__ __host__ inline uint32_t tie_all(uint32_t hi) { return hi ? 0u : 0xFFFFFFFFu; }


// ------------------------------------------------------------------------------------------
// Block-level helpers
// ------------------------------------------------------------------------------------------
// Find, scanning a 2048-bin histogram from the TOP bin down, the bin b where the running count
// reaches k (1-based).  Returns b and the count strictly above b.  256 threads, 8 bins each.
// (t, own): the thread's index in the 256 that scan; every thread of the block takes the barriers.
// A workgroup barrier for LDS only: this wave's LDS operations done, then s_barrier — unlike
// __syncthreads it does not wait for the wave's global loads (vmcnt), so loads stay in flight.
__device__ inline void lds_bar() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
template <bool RAW>
__device__ inline void blk_bar() {
    if (RAW) lds_bar();
    else __syncthreads();
}
template <bool RAW = false>
__device__ inline void hist_find_at(const uint32_t* h, uint32_t k, uint32_t& bin, uint32_t& above,
                                    uint32_t* scratch /* LDS 256+2 */, int t, bool own) {
    // thread t owns bins [HBINS-8(t+1), HBINS-8t)  (top bins first)
    uint32_t local[8];
    uint32_t s = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) { local[q] = own ? h[HBINS - 1 - (t * 8 + q)] : 0u; s += local[q]; }
    if (t == 0) { scratch[256] = 0; scratch[257] = 0; }   // defined result even if k > total
    // inclusive scan over the 256 thread sums: inside each wave by shuffles, then the totals of the
    // waves before (one barrier instead of the 16 of a Hillis-Steele scan through LDS)
    const int lane = t & 63, w = t >> 6;
    uint32_t inc = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(inc, off, 64);
        inc += lane >= off ? v : 0u;
    }
    if (own && lane == 63) scratch[w] = inc;
    blk_bar<RAW>();
    uint32_t before = 0;
    if (own)
        for (int q = 0; q < w; ++q) before += scratch[q];
    uint32_t incl = own ? before + inc : 0u, excl = incl - s;
    if (own && excl < k && incl >= k) {
        uint32_t run = excl;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (run + local[q] >= k) {
                scratch[256] = (uint32_t)(HBINS - 1 - (t * 8 + q));
                scratch[257] = run;
                break;
            }
            run += local[q];
        }
    }
    blk_bar<RAW>();
    bin = scratch[256];
    above = scratch[257];
    blk_bar<RAW>();
}
// The same search over NB bins (NB / 256 a thread, threads 0..255 of a larger block; the rest only
// sync); found = false when the bins hold fewer than k in all.
template <int NB>
__device__ inline void hist_find_n(const uint32_t* h, uint32_t k, uint32_t& bin, uint32_t& above, bool& found,
                                   uint32_t* scratch /* LDS 256+3 */) {
    constexpr int PER = NB / 256;
    static_assert(NB % 256 == 0, "256 threads scan NB / 256 bins each");
    const int t = (int)threadIdx.x;
    const bool own = t < 256;
    uint32_t local[PER];
    uint32_t s = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) { local[q] = own ? h[NB - 1 - (t * PER + q)] : 0u; s += local[q]; }
    if (t == 0) { scratch[256] = 0; scratch[257] = 0; scratch[258] = 0; }
    const int lane = t & 63, w = t >> 6;
    uint32_t inc = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(inc, off, 64);
        inc += lane >= off ? v : 0u;
    }
    if (own && lane == 63) scratch[w] = inc;
    __syncthreads();
    uint32_t before = 0;
    if (own)
        for (int q = 0; q < w; ++q) before += scratch[q];
    const uint32_t incl = own ? before + inc : 0u, excl = incl - s;
    if (own && excl < k && incl >= k) {
        uint32_t run = excl;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            if (run + local[q] >= k) {
                scratch[256] = (uint32_t)(NB - 1 - (t * PER + q));
                scratch[257] = run;
                scratch[258] = 1;
                break;
            }
            run += local[q];
        }
    }
    __syncthreads();
    bin = scratch[256];
    above = scratch[257];
    found = scratch[258] != 0u;
    __syncthreads();
}
template <bool RAW = false>
__device__ inline void hist_find(const uint32_t* h, uint32_t k, uint32_t& bin, uint32_t& above,
                                 uint32_t* scratch /* LDS 256+2 */) {
    hist_find_at<RAW>(h, k, bin, above, scratch, (int)threadIdx.x, threadIdx.x < 256);   // larger blocks: the rest only sync
}
// Two searches side by side (blocks of >= 512 threads): threads 0-255 scan ha for ka, 256-511 hb for kb.
__device__ inline void hist_find2(const uint32_t* ha, uint32_t ka, uint32_t& bina, uint32_t& abovea, uint32_t* sa,
                                  const uint32_t* hb, uint32_t kb, uint32_t& binb, uint32_t& aboveb, uint32_t* sb) {
    const bool second = threadIdx.x >= 256;
    uint32_t bin, above;
    hist_find_at(second ? hb : ha, second ? kb : ka, bin, above, second ? sb : sa, (int)(threadIdx.x & 255u),
                 threadIdx.x < 512);
    bina = sa[256]; abovea = sa[257];
    binb = sb[256]; aboveb = sb[257];
    __syncthreads();
}

// pass p: 0 -> bits [30:20], 1 -> [19:9], 2 -> [8:0]
__device__ inline uint32_t pass_shift(int p) { return p == 0 ? 20u : (p == 1 ? 9u : 0u); }
__device__ inline uint32_t pass_bits(int p) { return p == 2 ? 9u : 11u; }
__device__ inline bool key_in_prefix(uint32_t key, int p, uint32_t prefix) {
    // prefix holds the bits above this pass's field
    if (p == 0) return true;
    uint32_t sh = pass_shift(p) + pass_bits(p);
    return (key >> sh) == prefix;
}
__device__ inline uint32_t key_bin(uint32_t key, int p) {
    return (key >> pass_shift(p)) & ((1u << pass_bits(p)) - 1u);
}

// exclusive prefix of v over the workgroup's threads (in thread order) and the total
template <int NT = EX_NT>
__device__ inline uint32_t ex_scan(uint32_t v, uint32_t* wsum /* LDS [NT / 64] */, uint32_t& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        inc += lane >= o ? t : 0u;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
        const uint32_t x = wsum[k];
        before += k < wv ? x : 0u;
        tot += x;
    }
    __syncthreads();
    total = tot;
    return before + inc - v;
}

struct RkdWs {
    uint32_t* cnt;     // [C][N]
    uint64_t* ckey;    // [N]
};

// ------------------------------------------------------------------------------------------
// Host side: what the units share, then the launchers that cross units
// ------------------------------------------------------------------------------------------
static inline int64_t host_chunks(int64_t d) { return (d + CHUNK - 1) / CHUNK; }
static inline int grid_stride_blocks(int64_t items, int64_t cap = 4096) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(items, cap));
}
// f(std::true_type / std::false_type) for a run-time vec: both instantiations of a <bool VEC> kernel
template <class F>
static inline void with_vec(bool vec, F f) {
    if (vec) f(std::true_type{});
    else f(std::false_type{});
}

// One sel_run call as its TopK regimes see it.  few: sharded candidate lists (k_topk_filter_fast) and
// the spread select (k_cs_pass); lone_assign: a lone compressVector row on the few-row path, its
// output zeroed by the filter and finished by k_assign_finish; gfold: many rows, each row group folded
// right after its select (tiles carried in ws.part), the last group's fold writing out.
struct TkCall {
    const flc_codec_params* prm;
    RowSrc rows;
    bool vec;
    int64_t n, d, K;
    bool assign;
    const float* w;
    float wt;
    float* out;
    SelWs ws;
    hipStream_t st;
    bool few, lone_assign, gfold;
};

// select.hip
int64_t sel_capacity(int codec, int64_t d, int64_t K);
SelWs carve_sel(void* base, int codec, int64_t n, int64_t d, int64_t K, size_t* bytes);
// topk_filter.hip: the sample of rows [a, b) on sx; the fast filter of rows [r0, r0 + rn) on c.st
// (2- or 4-chunk groups, per-wave or workgroup items); the exact filter of every row (dense K)
void launch_sample(const TkCall& c, int64_t a, int64_t b, hipStream_t sx);
void launch_filter_rows(const TkCall& c, int64_t r0, int64_t rn);
int launch_filter_exact(const TkCall& c);
// topk_select.hip: the candidate select of rows [r0, r0 + rn) on sx; the one exact-rows launch of the
// rows the fast path failed; dense K's worklist, radix passes and tie prefix over the full rows; a
// lone row's exact fallback + scatter
void launch_select(const TkCall& c, int64_t r0, int64_t rn, bool last_of_many, hipStream_t sx);
int launch_exact_rows(const TkCall& c, hipStream_t sx);
int launch_radix_full(const TkCall& c);
int launch_assign_finish(const TkCall& c);
// lone_row.hip: k_lone_resident for a row that fits the chip's registers (*took), serialised across streams
int lone_resident_launch(RowSrc rows, int64_t d, int64_t K, SelWs ws, float* out, hipStream_t st, bool* took);
// randk.hip: the compat bucketing of the rows' given indices into ws's lists; the device sampler's run
int randk_lists_launch(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, int64_t n, int64_t d, SelWs ws,
                       hipStream_t st);
int randk_device_run(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, int64_t n, int64_t d,
                     const float* w, float wt, float* out, void* wsp, size_t ws_bytes, hipStream_t st);
// chunk_accum.hip: the fold of the rows' lists (split by chunk count), of one TopK row group, of
// whole chunks whatever their number (the wire unpack), and a lone row's list scattered into out
int launch_chunk_accum(int64_t n, int64_t d, SelWs ws, bool assign, const float* w, float wt, float* out, hipStream_t st);
int launch_group_fold(int64_t n, int64_t d, SelWs ws, const float* w, float wt, float* out, int64_t r0, int64_t r1,
                      bool first, bool last, bool exposed, hipStream_t st);
int launch_chunk_accum_whole(int64_t n, int64_t d, SelWs ws, const float* w, float wt, float* out, hipStream_t st);
void launch_assign_scatter(SelWs ws, float* out, bool few, hipStream_t st);

}  // namespace flc
