// Sparse fused standard dithering / QSGD encode + reduce: device-RNG mode, p = 2 norm.
// fl_pytorch/utils/compressors.py:270-299 (the codec; qsgd = std dithering with p = 2, 95-101) and
// the serverGradient fold (algorithms.py:1748-1770), reading every client row from HBM ONCE.
//
// Why a sparse path: the encode needs the row's norm before any element, so the dense path reads
// every row twice (norm pass + encode pass, codecs.hip).  But QSGD's output is sparse: element j
// is nonzero only if y_j = |x_j| / ||x||_2 >= l1 (the first level, 1/s) or its draw goes up, so
//     E[nonzeros] <= sum_j min(1, y_j / l1) <= ||x||_1 / (l1 ||x||_2) <= s sqrt(D)
// for ANY row (2.0 % of the elements at s = 127, D = 25 M for Gaussian rows).  One streaming pass
// can therefore accumulate the norm AND decide almost every element, using BOUNDS n_lo <= n <=
// n_hi of the norm from a spread sample (checked once the norm is known; a row outside its bounds
// is folded dense):
//
//   sample  : per row, sum of squares (and 4th powers) of a spread 16 K-element sample -> n_lo,
//             n_hi, the candidate scale qc = 256 (1 + 2^-18) / (l1 n_lo), the classification
//             scales q0 = RU(1 / (l1 n_lo)), q1 = RD(1 / (l1 n_hi)), the device-RNG row key.
//   filter  : ONE pass over every row: float64 sum of squares per 8192-element item (fixed slots),
//             and every element passing  fma(|x|, qc, hi8) > 254.98  staged in LDS (hi8 = the top
//             byte of the element's draw, one group hash per 4 elements).  At the item's end each
//             staged candidate is classified with its full 32-bit draw h (the low hash computed
//             for the ~2 % staged only):
//               sure   — kept at level l1 for EVERY norm in [n_lo, n_hi]: a 2-byte entry
//                        (item-local index | sign) — its contribution is +-RN(l1 n) for any n;
//               drop   — zero for every norm >= n_lo: nothing written;
//               ambiguous (norm band, higher levels, 0-ish draws): the 8-byte (index | hi8, x).
//   final   : per row, norm = RN(sqrt(sum of the partials in a fixed order)); the row is folded
//             DENSE (every element re-read and encoded) if the norm is outside [n_lo, n_hi], not
//             finite, its weight not finite, or an item overflowed its staging.
//   resolve : the ambiguous entries encoded exactly with the norm (ds_encode = DitherOp::apply's
//             arithmetic), rewritten in place as (index, C(x)) when nonzero.
//   accum   : one wave owns a 2048-element half chunk as an fp32 LDS tile and folds the rows in
//             order: per row its sure entries (+-RN(l1 n)) and resolved entries (C(x)), times the
//             weight; untouched columns get the sign of zero the sequential fold of the all-zero
//             contributions gives (-0 only if every row gives -0).
//
// Exactness of the classification.  In the first level interval [0, l1] the encode keeps l1 iff
// h >= thr(n),  thr(n) = sat_u32(ceil(RN(RN(y - l1) / (-l1 2^-32)))),  y = RN(|x| / n).  Every
// step is monotone, so thr is nondecreasing in n; and |thr(n) - 2^32 (1 - |x| / (n l1))| <
// 2^32 2^-22.  Hence for n in [n_lo, n_hi] (and |x| q0 <= 1 - 2^-18, so y < l1 throughout):
//   h / 2^32 + |x| / (n_hi l1) >= 1 + 2^-22  =>  kept for every such n      (sure)
//   h / 2^32 + |x| / (n_lo l1) <  1 - 2^-22  =>  not kept for every such n  (drop)
// evaluated as fp32 fmas with q1 / q0 and floor / ceil of h / 2^32 at 2^-24 resolution against
// 1 +- 2^-20 (the fma's rounding is < 2^-24 there).  The candidate test itself is conservative (never
// drops a nonzero): for n >= n_lo a nonzero output has h >= p 2^32 with p >= 1 - y / l1 - 2^-23,
// so hi8 = h >> 24 > 255 - 256 |x| (1 + 2^-24) / (l1 n_lo) - 2^-15, and |x| qc + hi8 > 255 - 2^-15;
// the fp32 fma loses < 2^-14 there, so > 254.98 keeps every nonzero.  Elements in higher
// intervals (y >= l1) have |x| qc >= 256.
//
// Norms from elsewhere.  The argument above holds for ANY norm n in [n_lo, n_hi], whoever computed
// it, so the row's norm may also be GIVEN by the caller (the norm a server received) or be the
// reference's own fp32 value (FLC_NORMMODE_TORCH_CPU: torch.norm(x, 2) in torch's CPU reduction
// order, torch_norm.hip): k_ds_final then takes it from an array instead of sqrt(sum of partials)
// and checks it against the same bounds; a row whose norm lies outside is folded dense with that
// norm, like any other.  Such a norm is not the exactly rounded one, so for rows sampled whole
// (d <= DS_SMAX), whose bounds are otherwise norm (1 -+ 2^-20), these two modes give the bounds
// the sampled case's relative margin (FLC_DS_MARGIN on the sum of squares): the fp32 chain's norm
// is a few 1e-4 away at most there.  The wider band changes no result — the classification is
// exact for every norm inside the bounds — it only makes more candidates ambiguous (resolved with
// the norm) instead of sure.
// In the torch-order mode the filter also emits, per item, the float64 sum of squares PER TORCH
// LANE (an item is 1024 steps of each of torch's 8 accumulator lanes: one block of torch_norm.hip),
// which replace k_tn_sums' extra read of the rows; they are a prediction only — k_tn_walk checks
// every map against the real accumulator — so they cannot change a bit of the norm.
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "chunks.hpp"
#include "codec_ops.hpp"

namespace flc {

constexpr uint32_t DS_DENSE = 1u, DS_FAST = 4u;
constexpr int DS_FGS = 2;                  // chunks per filter work item (8192 elements)
constexpr int DS_NH = 2 * DS_FGS;          // fold tiles (half chunks) per item
constexpr int DS_GCAP = 512;               // staged candidates per item (6.25 %; more -> row overflow)
constexpr int DS_HCAP = DS_GCAP / DS_NH;    // entries per half chunk of an item (more -> row overflow)
constexpr int DS_MAXLEV = 15;              // entry level field: 4 bits (a higher level -> row dense)
#ifndef FLC_DS_SPLIT_SAMPLE
#define FLC_DS_SPLIT_SAMPLE 1         // QSGD row groups: only group 0's sample before the first filter
#endif
#ifndef FLC_DS_SMAX
#define FLC_DS_SMAX 65536
#endif
#ifndef FLC_DS_MARGIN
#define FLC_DS_MARGIN 0.02
#endif
constexpr int DS_SMAX = FLC_DS_SMAX;       // sample elements per row (256-element pieces)
constexpr int DS_SNT = 1024;               // sample threads per row
constexpr float DS_QT = 254.98f;
constexpr int DS_MAXS = 512;               // level table entries kept in LDS by the fold
constexpr uint32_t DS_OVF = 0xFFFFFFFFu;   // itm: the item overflowed its staging capacity
#ifndef FLC_DS_AP
#define FLC_DS_AP 16
#endif
constexpr int DS_AP = FLC_DS_AP;           // passed for k_ds_accum's AP
// rows per block of the filter's item order: 16 measured as fast as one block of all rows at C4
// (and 1, row-major, 1-2 % slower on the same box); a block never reads one row twice, so rows
// that alias (C5's replayed pool) are still read from HBM once per client
constexpr int64_t DS_RB = 16;
constexpr int DS_RINGC = 4;                // compat filter ring (x + u: 24 B per lane per step)
#ifndef FLC_DS_STPOL
// k_ds_filter's list copy-outs (sure and ambiguous entries) as nontemporal stores: bit-identical,
// C4 9.736 -> 9.615 ms per step on one allocation (profiles/r05/ab_list_stnt.txt; the same for
// the TopK filter's lists ran 7.618 -> 7.734 ms at C3, so FLC_TK_STPOL stays 0)
#define FLC_DS_STPOL 2
#endif
#ifndef FLC_DS_CU
#define FLC_DS_CU 2                  // k_ds_filter: candidate batches (of 64) classified per iteration
#endif
#ifndef FLC_DS_RW
#define FLC_DS_RW 8                  // k_ds_resolve: candidate windows (64 each) gathered up front
#endif

// One entry of the fold's lists (u16): half-chunk-local index (11 bits) | sign << 11 | level << 12;
// its contribution is copysign(levels[level], sign) * norm — C(x) exactly as the encode forms it.
struct DsWs {
    uint2* tabs;          // [Hp][N] (unused, count) of row's sure entries in half chunk h: the
                          // list of (h, row) is ent16[h][row][0 .. count + cntr)
    uint32_t* cntr;       // [Hp][N] resolved entries appended after them (k_ds_resolve)
    uint16_t* ent16;      // [Hp][N][DS_HCAP] entries, half-major: the fold of half h reads its
                          // rows' regions as one contiguous n * 256-byte run
    uint2* enta;          // [N][cap] ambiguous candidates (item-local index | hi8 << 13, x bits)
    uint32_t* itm;        // [G][N] ambiguous candidates of the item; DS_OVF: it overflowed
    uint32_t* flags;      // [N] DS_*
    float* qc;            // [N] candidate scale
    float* nlo;           // [N] norm bounds the classification assumes (checked by k_ds_final)
    float* nhi;
    float* q0;            // [N] RU(1 / (l1 n_lo))
    float* q1;            // [N] RD(1 / (l1 n_hi)); 0: no sure entries (n_hi unbounded)
    double* partial;      // [N][G] per-item sums of squares
    float* pn;            // [N] norm
    float* rpn;           // [N] RN(1 / norm)
    uint32_t* rk;         // [N] device-RNG row key
    float* part;          // [D] running sums carried between the row groups' folds
    float4* gtab;         // [DS_MAXS] level table (load_table) for the fold's dense rows, made by
                          // k_ds_sample: the fold keeps only its tile in LDS
    int64_t cap;          // per row: G * GCAP (each filter item owns a fixed region)
    int64_t G;            // filter items per row
    int64_t n;            // rows
    double* tsum;         // [N][G][8] torch-order mode: the item's sums of squares per torch lane
};

constexpr int HCHUNK = CHUNK / 2;          // the fold's tile: 2048 elements (8 KB of LDS per wave)
__host__ __device__ inline int64_t nhalves(int64_t d) { return (d + HCHUNK - 1) / HCHUNK; }

// top byte of element j's draw (common.hpp dev_draw)
__device__ inline uint32_t ds_hi8(uint32_t j, uint32_t rk) { return (grouphash(j >> 2, rk) >> (8u * (j & 3u))) & 0xFFu; }
__device__ inline float f32_up(double v) { float f = (float)v; return (double)f < v ? nextafterf(f, __builtin_huge_valf()) : f; }
__device__ inline float f32_down(double v) { float f = (float)v; return (double)f > v ? nextafterf(f, 0.f) : f; }

// The two-operand row source of the one-read shifted round (flc_dither_shift_reduce, DESIGN.md
// §8.04): row i is the fp32 difference a_i - b_i, formed wherever the one-operand kernels use x.
// k_ds_sample, k_ds_filter and k_ds_accum are templates on the source; everything after the filter
// (k_ds_final, k_ds_resolve) works on entries, which carry the value's bits: v's here.
struct DiffSrc {
    RowSrc a, b;
};
struct RowRef {
    const float* p;
    __device__ inline float operator[](int64_t i) const { return p[i]; }
};
struct DiffRef {
    const float* a;
    const float* b;
    __device__ inline float operator[](int64_t i) const { return a[i] - b[i]; }
};
__device__ inline RowRef row_ref(const RowSrc& s, int64_t i) { return RowRef{s.row(i)}; }
__device__ inline DiffRef row_ref(const DiffSrc& s, int64_t i) { return DiffRef{s.a.row(i), s.b.row(i)}; }
// the (first) operand's row through the scalar cache (RowSrc::row_s)
__device__ inline const float* row_a(const RowSrc& s, int64_t i) { return s.row_s(i); }
__device__ inline const float* row_a(const DiffSrc& s, int64_t i) { return s.a.row_s(i); }

// ------------------------------------------------------------------------------------------
// Sample: one workgroup per row.
// ------------------------------------------------------------------------------------------
template <class SRC>
__global__ __launch_bounds__(DS_SNT) void k_ds_sample(SRC rows, int64_t n, int64_t d, const float* __restrict__ levels,
                                                      int s, uint64_t seed, int64_t client0, DsWs ws, int64_t r_off, int wide) {
    constexpr int NW = DS_SNT / 64;
    __shared__ double r2[NW], r4[NW];
    const int64_t row = r_off + blockIdx.x;                               // (a launch may take a row range)
    if (row == 0) load_table(levels, s, ws.gtab);
    if (row >= n) return;
    const auto r = row_ref(rows, row);
    double a2 = 0.0, a4 = 0.0;
    int64_t S;
    if (d <= DS_SMAX) {
        S = d;
        for (int64_t i = threadIdx.x; i < d; i += DS_SNT) {
            const double v = (double)r[i] * (double)r[i];
            a2 += v;
            a4 += v * v;
        }
    } else {
        // P pieces of 256 contiguous elements spread evenly; the block's 4 quarters take every 4th
        // piece, thread t reading element t % 256 of 16 pieces per round trip
        constexpr int P = DS_SMAX / 256, Q = DS_SNT / 256, U = 16;
        static_assert(P % (Q * U) == 0, "sample pieces");
        S = DS_SMAX;
        const int e = threadIdx.x & 255, q = threadIdx.x >> 8;
        for (int p0 = q; p0 < P; p0 += Q * U) {
            float x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = r[((int64_t)(p0 + Q * u) * (d - 256)) / (P - 1) + e];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double v = (double)x[u] * (double)x[u];
                a2 += v;
                a4 += v * v;
            }
        }
    }
    a2 = wave_sum(a2);
    a4 = wave_sum(a4);
    if ((threadIdx.x & 63) == 0) { r2[threadIdx.x >> 6] = a2; r4[threadIdx.x >> 6] = a4; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a2 = 0.0;
        a4 = 0.0;
        for (int w = 0; w < NW; ++w) { a2 += r2[w]; a4 += r4[w]; }
        const float l0 = levels[0], l1 = levels[1];
        const bool bad = !(l0 == 0.f) || !(l1 > 0.f);   // the bounds need levels 0 < l1 < ...
        double nlo, nhi = __builtin_huge_val();
        if (S == d && wide) {
            nlo = sqrt(a2 * (1.0 - FLC_DS_MARGIN));        // the whole row, the norm not the exactly
            nhi = sqrt(a2 * (1.0 + FLC_DS_MARGIN));        // rounded one (given / torch's order)
        } else if (S == d) {
            nlo = sqrt(a2) * (1.0 - 0x1p-20);              // the whole row: the norm itself
            nhi = sqrt(a2) * (1.0 + 0x1p-20);
        } else {
            // estimate of the sum of squares, discounted by 6 sigma of the sample mean + a margin; the
            // upper bound only for light-tailed samples (heavy tails: n_hi unbounded, no sure entries)
            const double m = (double)S, mean2 = a2 / m;
            const double var = fmax(a4 / m - mean2 * mean2, 0.0);
            const double rel = sqrt(var / m) / mean2;      // NaN/inf when mean2 == 0 or overflow
            const double f = fmin(fmax(1.0 - 6.0 * rel - FLC_DS_MARGIN, 0.25), 0.97);
            nlo = sqrt(f * mean2 * (double)d);
            if (rel <= 0.05) nhi = sqrt((1.0 + 6.0 * rel + FLC_DS_MARGIN) * mean2 * (double)d);
        }
        float nlof = (float)nlo;
        if (!(nlof >= 0.f) || !(nlof <= 3.0e38f)) nlof = 0.f;
        float nhif = f32_up(nhi);
        if (!(nhif >= nlof) || !(nhif <= 3.0e38f)) nhif = __builtin_huge_valf();
        const double qcd = 256.0 * (1.0 + 0x1p-18) / ((double)l1 * (double)nlof);   // +inf for nlof 0
        float qc = (float)(qcd * (1.0 + 0x1p-22));         // rounded up past the conversion
        if (!(qc >= 0.f)) qc = __builtin_huge_valf();
        float q0 = f32_up(1.0 / ((double)l1 * (double)nlof));                       // +inf for nlof 0
        float q1 = f32_down(1.0 / ((double)l1 * (double)nhif));                     // 0 for nhi inf
        if (!(q0 >= 0.f)) q0 = __builtin_huge_valf();
        if (!(q1 >= 0.f) || !(q1 <= 3.0e38f)) q1 = 0.f;
        if (bad) { qc = 0.f; q1 = 0.f; }                   // row is folded dense anyway
        ws.qc[row] = qc;
        ws.nlo[row] = nlof;
        ws.nhi[row] = nhif;
        ws.q0[row] = q0;
        ws.q1[row] = q1;
        ws.flags[row] = bad ? DS_DENSE : 0u;
        ws.rk[row] = rowkey(client_key(seed, client0 + row));
    }
}

// ------------------------------------------------------------------------------------------
// Filter: a RING-deep buffer-load pipeline across chunks and items (topk_filter.hip's TopK filter
// structure), the dithering candidate test and the norm.  A work item is DS_FGS consecutive
// 4096-element chunks of one row; its candidates are compacted (ballot / mbcnt) into wave-private
// LDS, classified (sure / drop / ambiguous) and copied out coalesced into the item's FIXED regions
// of the row's lists (item * GCAP): no reservation atomic, so nothing returning sits in the
// in-order vmcnt queue of the load stream.  The tab gets the sure entries' (offset, count) per
// 2048-element half chunk (the fold's tile).
// ------------------------------------------------------------------------------------------
// PROBE (-DFLC_TUNING builds only, FLC_DS_PROBE in the environment; outputs NOT valid): 1 fp32
// norm; 2 no candidate staging; 3 loads + norm only; 4 the draw's group hash without its
// multiplies; 5 exec-narrowed staging without a branch; 6 staging without the classification
//
// COMPAT: the draws are the caller's float64 uniforms u (the reference's numpy stream, [n][uld]),
// read in the same single pass (12 B per element).  A lane then holds elements {2l, 2l+1, 128 + 2l,
// 128 + 2l + 1} of each 256-element step (one 512-B x load and one 1-KB u load per pair, both
// contiguous); the candidate test takes RN(u) * 256 for the top byte, and each staged candidate
// carries RD(u) (LDS) for its classification — the same bounds with h / 2^32 replaced by u, whose
// float brackets [RD(u), next float up] are tighter than the 24-bit h's.
struct CSlot {
    float2 xa, xb;       // elements 2l, 2l+1 | 128 + 2l, 128 + 2l + 1 of the step
    double2 ua, ub;      // their uniforms
};
__device__ inline CSlot load_c(__amdgpu_buffer_rsrc_t rx, __amdgpu_buffer_rsrc_t ru, int lane, int L) {
    CSlot s;
    const auto a = __builtin_amdgcn_raw_buffer_load_b64(rx, lane * 8, L * 1024, FLC_LOADPOL);
    const auto b = __builtin_amdgcn_raw_buffer_load_b64(rx, lane * 8 + 512, L * 1024, FLC_LOADPOL);
    const auto p = __builtin_amdgcn_raw_buffer_load_b128(ru, lane * 16, L * 2048, FLC_LOADPOL);
    const auto q = __builtin_amdgcn_raw_buffer_load_b128(ru, lane * 16 + 1024, L * 2048, FLC_LOADPOL);
    s.xa = make_float2(__uint_as_float(a[0]), __uint_as_float(a[1]));
    s.xb = make_float2(__uint_as_float(b[0]), __uint_as_float(b[1]));
    s.ua = make_double2(__hiloint2double((int)p[1], (int)p[0]), __hiloint2double((int)p[3], (int)p[2]));
    s.ub = make_double2(__hiloint2double((int)q[1], (int)q[0]), __hiloint2double((int)q[3], (int)q[2]));
    return s;
}
// descriptor of chunk c's uniforms (range-checked like chunk_rsrc: 0 past the row end)
__device__ inline __amdgpu_buffer_rsrc_t chunk_ursrc(const double* u, int64_t j0, int64_t d) {
    const int64_t len = max((int64_t)0, min((int64_t)CHUNK, d - j0));
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(u + j0), (short)0, (int)(len * 8), 0x00020000);
}
#ifndef FLC_DS_WPE
#define FLC_DS_WPE 6                 // 6 waves per SIMD (80 VGPRs): measured 9.19 -> 9.10 ms at C4 vs 5
#endif
#ifndef FLC_DS_WPEC
#define FLC_DS_WPEC 5                // compat: 5 (LDS: 32 KB of staging per block)
#endif
//
// TNS (the torch-order norm mode): instead of the item's one sum of squares (the partial of the
// exact norm, not needed there) the float64 sums PER TORCH LANE go to tsum[row][item][8] — element
// j of a row belongs to lane j % 8, i.e. lane 4 (t & 1) + q for thread t's q-th element of a
// device-RNG step (4 t + 256 L + q) and 2 (t & 3) + (q & 1) for the compat filter's.
//
// DIFF (SRC = DiffSrc, the one-read shifted round): the elements are v = a - b.  A ring slot holds
// both operands' float4 of a step, so the ring is 8 pairs deep where the one-operand ring holds 16
// float4 — the same 64 VGPRs and the same bytes in flight per wave — and the subtraction happens
// at consumption.  b's chunk descriptors are range-checked like a's (both return 0 past the row
// end: v = 0, dropped), and the item's fixed store sequence is unchanged.  Device draws and the
// exact norm only.
struct DSlot {
    float4 a, b;
};
__device__ inline DSlot load_d(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb, int lane, int L) {
    DSlot s;
    s.a = load_q(ra, lane, L);
    s.b = load_q(rb, lane, L);
    return s;
}
template <int RING, int GCAP, int PROBE = 0, bool COMPAT = false, bool TNS = false, class SRC = RowSrc>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(COMPAT ? FLC_DS_WPEC : FLC_DS_WPE))) void k_ds_filter(SRC rows, int64_t n, int64_t r0, int64_t rn, int64_t rb, int64_t d, DsWs ws, UniformSrc us) {
    constexpr int FGS = DS_FGS, NH = DS_NH;
    constexpr bool DIFF = std::is_same<SRC, DiffSrc>::value;
    static_assert(!DIFF || (!COMPAT && !TNS && PROBE == 0), "two-operand source: the device-RNG, exact-norm filter only");
    static_assert(16 % RING == 0, "ring must divide the 16 loads of a chunk");
    static_assert(GCAP % 512 == 0 && (GCAP & (GCAP - 1)) == 0, "copy-out in whole 16-B wave slots; wrap mask");
    static_assert(!COMPAT || PROBE == 0, "probes: device-RNG filter only");
    static_assert(!TNS || PROBE == 0, "probes: the exact-norm filter only");
    constexpr int NTA = TNS ? (COMPAT ? 2 : 4) : 1;        // TNS: a thread's torch lanes
    constexpr int DS_ITEM_STORES = 4 + GCAP / 128;   // partial, itm, tab, sure and ambiguous copy-outs
    // (entry word, x bits); 64 slots past GCAP take the writes of a wave-instruction that starts
    // at GCAP (its item has overflowed)
    __shared__ __attribute__((aligned(16))) uint2 stage[4][GCAP + 64];
    __shared__ __attribute__((aligned(16))) uint16_t stage16[4][GCAP];
    __shared__ float stagef[4][COMPAT ? GCAP + 64 : 1];     // compat: RD(u) of the staged
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t G = ws.G;
    const int64_t items = rn * G;                            // this launch's rows: [r0, r0 + rn)
    const int64_t stride = (int64_t)gridDim.x * 4;
    int64_t it = (int64_t)blockIdx.x * 4 + wv;
    if (it >= items) return;
    const uint32_t lphi = (uint32_t)lane * 0x9E3779B1u;    // group index g = c*1024 + 64 L + lane
    uint2* sg = stage[wv];
    uint16_t* s16 = stage16[wv];
    float* sgf = stagef[wv];
    // LDS byte address of the wave's staging buffer (wave-uniform)
    const uint32_t sla = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) uint2*)sg);
    typedef typename std::conditional<COMPAT, CSlot, typename std::conditional<DIFF, DSlot, float4>::type>::type Slot;
    Slot ring[RING];
    // item order: blocks of rb rows (the last one shorter), and inside a block (gi, row) with the
    // row fastest: the waves in flight at any time read the same item of the block's rows, spread
    // over rb rows rather than one row's neighbouring items, and each row is read once per launch
    // even when rows alias (a row read twice inside one block would be served from the caches)
    auto item_at = [&](int64_t t, int64_t& r, int64_t& g) {
        const int64_t blk = t / (rb * G), rem = t - blk * rb * G;
        const int64_t bn = min(rb, rn - blk * rb);            // rows in this block
        g = rem / bn;
        r = r0 + blk * rb + (rem - g * bn);
    };
    int64_t row, gi0;
    item_at(it, row, gi0);
    int64_t c = gi0 * FGS;
    auto rs = chunk_rsrc(row_a(rows, row), c * CHUNK, d);
    auto urow = [&](int64_t r) { return us.u + r * us.uld; };
    auto ru = rs;                                            // the second operand: compat u, DIFF b
    if constexpr (COMPAT) ru = chunk_ursrc(urow(row), c * CHUNK, d);
    if constexpr (DIFF) ru = chunk_rsrc(rows.b.row_s(row), c * CHUNK, d);
#pragma unroll
    for (int L = 0; L < RING - 1; ++L) {
        if constexpr (COMPAT) ring[L] = load_c(rs, ru, lane, L);
        else if constexpr (DIFF) ring[L] = load_d(rs, ru, lane, L);
        else ring[L] = load_q(rs, lane, L);
        __builtin_amdgcn_sched_barrier(0);
    }
    {
        // the stores an item ends with, dropped (num_records 0): the loop is entered with the same
        // vmcnt queue shape as it is re-entered
        const auto nd = __builtin_amdgcn_make_buffer_rsrc(ws.enta, (short)0, 0, 0x00020000);
#pragma unroll
        for (int k = 0; k < DS_ITEM_STORES; ++k) __builtin_amdgcn_raw_buffer_store_b32(0u, nd, lane * 4, k * 256, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    while (it < items) {
        const float qc = sload(ws.qc + row);
        const uint32_t rk = sload(ws.rk + row);
        const int64_t gi = c / FGS;
        const int64_t nit = it + stride;
        uint32_t cnt = 0;
        double a2 = 0.0;
        double ta[NTA];                                      // TNS: sums of squares per torch lane
#pragma unroll
        for (int u = 0; u < NTA; ++u) ta[u] = 0.0;
        int64_t nrow = row, nc = c;
#pragma unroll
        for (int sub = 0; sub < FGS; ++sub, ++c) {
            const int64_t j0 = c * CHUNK;
            __amdgpu_buffer_rsrc_t rsn, run = ru;
            if (sub + 1 < FGS) {
                rsn = chunk_rsrc(row_a(rows, row), j0 + CHUNK, d);
                if constexpr (COMPAT) run = chunk_ursrc(urow(row), j0 + CHUNK, d);
                if constexpr (DIFF) run = chunk_rsrc(rows.b.row_s(row), j0 + CHUNK, d);
            } else if (nit < items) {
                int64_t ngi;
                item_at(nit, nrow, ngi);
                nc = ngi * FGS;
                rsn = chunk_rsrc(row_a(rows, nrow), nc * CHUNK, d);
                if constexpr (COMPAT) run = chunk_ursrc(urow(nrow), nc * CHUNK, d);
                if constexpr (DIFF) run = chunk_rsrc(rows.b.row_s(nrow), nc * CHUNK, d);
            } else {
                    rsn = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row_a(rows, row)), (short)0, 0, 0x00020000);
                    if constexpr (COMPAT) run = chunk_ursrc(urow(row), 0, 0);
                    if constexpr (DIFF) run = chunk_rsrc(rows.b.row_s(row), 0, 0);   // no records: every load returns 0
                }
                if constexpr (COMPAT) {
                    // item-local index of (L, q): 4096 sub + 2 lane + 256 L + {0, 1, 128, 129}[q]
                    uint32_t jb = (uint32_t)lane * 2u + (uint32_t)sub * CHUNK;
                    asm volatile("" : "+v"(jb));
#pragma unroll
                    for (int L = 0; L < 16; ++L) {
                        const int P = L + RING - 1;
                        ring[P % RING] = P < 16 ? load_c(rs, ru, lane, P) : load_c(rsn, run, lane, P - 16);
                        const CSlot sl = ring[L % RING];
                        const float vq[4] = {sl.xa.x, sl.xa.y, sl.xb.x, sl.xb.y};
                        const double uq[4] = {sl.ua.x, sl.ua.y, sl.ub.x, sl.ub.y};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if constexpr (TNS) ta[q & 1] = fma((double)vq[q], (double)vq[q], ta[q & 1]);
                            else a2 = fma((double)vq[q], (double)vq[q], a2);
                            const float hf = (float)uq[q];                 // RN(u): |hf - u| <= 2^-25
                            const bool f = fmaf(fabsf(vq[q]), qc, hf * 256.f) > DS_QT;
                            const uint64_t m = __ballot(f);
                            if (f) {
                                const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                                const uint32_t slot = min(cnt, (uint32_t)GCAP) + pre;
                                sg[slot] = make_uint2(jb + (uint32_t)(L * 256 + (q & 1) + (q >> 1) * 128), __float_as_uint(vq[q]));
                                // RD(u) (u in [0, 1): hf > u implies hf > 0)
                                sgf[slot] = (double)hf > uq[q] ? __uint_as_float(__float_as_uint(hf) - 1u) : hf;
                            }
                            cnt += (uint32_t)__popcll(m);
                        }
                        if constexpr (TNS) {
#pragma unroll
                            for (int u = 0; u < NTA; ++u) asm volatile("" : "+v"(ta[u]));
                        } else {
                            asm volatile("" : "+v"(a2));
                        }
                    }
                } else {
                // item-local index of (L, q): 4096 sub + 4 lane + 256 L + q (opaque: keeps the 64
                // constants out of VGPRs); the draw's top byte is recomputed for the staged only
                uint32_t jb = (uint32_t)lane * 4u + (uint32_t)sub * CHUNK;
                asm volatile("" : "+v"(jb));
                const uint32_t gb = lphi + (uint32_t)(c * 1024) * 0x9E3779B1u + rk;   // hash input of L = 0
#pragma unroll
                for (int L = 0; L < 16; ++L) {
                    const int P = L + RING - 1;
                    float4 x;
                    if constexpr (DIFF) {
                        // both operands of step P go out; step L's pair is subtracted here
                        ring[P % RING] = P < 16 ? load_d(rs, ru, lane, P) : load_d(rsn, run, lane, P - 16);
                        const DSlot sl = ring[L % RING];
                        x = make_float4(sl.a.x - sl.b.x, sl.a.y - sl.b.y, sl.a.z - sl.b.z, sl.a.w - sl.b.w);
                    } else {
                        ring[P % RING] = P < 16 ? load_q(rs, lane, P) : load_q(rsn, lane, P - 16);
                        x = ring[L % RING];
                    }
                    uint32_t hg;
                    if (PROBE == 4) { hg = gb + (uint32_t)(L * 64) * 0x9E3779B1u; hg ^= hg >> 15; }   // cost probe only
                    else hg = gmix(gb + (uint32_t)(L * 64) * 0x9E3779B1u);
                    const float vq[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (PROBE == 1) a2 = (double)fmaf(vq[q], vq[q], (float)a2);
                        else if constexpr (TNS) ta[q] = fma((double)vq[q], (double)vq[q], ta[q]);
                        else a2 = fma((double)vq[q], (double)vq[q], a2);
                        if (PROBE == 3) continue;
                        const float hi = (float)((hg >> (8 * q)) & 0xFFu);
                        // no range test: past the row end the loads return 0, and a zero candidate
                        // is dropped; NaN from 0 * inf (qc = inf) is not a candidate
                        const bool f = fmaf(fabsf(vq[q]), qc, hi) > DS_QT;
                        const uint64_t m = __ballot(f);
                        // exec-masked store (a branch-free store of every element to a per-lane spill
                        // slot measured 9.2 -> 11.9 ms: the staging is LDS-issue sensitive)
                        if (PROBE == 5) {
                            // A/B: the staging store without a branch — exec narrowed to the
                            // candidates for the one ds_write2 (the loop runs with every lane active)
                            const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                            uint32_t sb = sla + min(cnt, (uint32_t)GCAP) * 8u;
                            asm volatile("" : "+s"(sb));
                            const uint32_t la = sb + pre * 8u;
                            uint64_t saved;
                            asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\ts_nop 1\n\t"
                                         "ds_write2_b32 %2, %3, %4 offset1:1\n\ts_mov_b64 exec, %0"
                                         : "=&s"(saved) : "s"(m), "v"(la), "v"(jb + (uint32_t)(L * 256 + q)), "v"(__float_as_uint(vq[q]))
                                         : "memory");
                        } else if (PROBE != 2 && f) {
                            // slot = min(cnt, GCAP) + candidates in lower lanes (< GCAP + 64): exact
                            // while the item fits; past GCAP the item overflows (its row is folded
                            // dense) and the writes land in the spare slots.  The scalar part is folded
                            // into the wave's LDS address in SALU (sla), the lane part is one mbcnt
                            // pair; index and x go out as one ds_write2_b32 (no register pair to
                            // assemble for a 64-bit store).
                            const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                            uint32_t sb = sla + min(cnt, (uint32_t)GCAP) * 8u;
                            asm volatile("" : "+s"(sb));             // stays a scalar term: one v_lshl_add
                            const uint32_t la = sb + pre * 8u;
                            asm volatile("ds_write2_b32 %0, %1, %2 offset1:1" ::"v"(la), "v"(jb + (uint32_t)(L * 256 + q)),
                                         "v"(__float_as_uint(vq[q])) : "memory");
                        }
                        cnt += (uint32_t)__popcll(m);
                    }
                    // keep the norm's fma chain here: left alone, the compiler sinks all 128 of an
                    // item's fmas to its end and holds the 128 x values live (218 VGPRs)
                    if constexpr (TNS) {
#pragma unroll
                        for (int u = 0; u < NTA; ++u) asm volatile("" : "+v"(ta[u]));
                    } else {
                        asm volatile("" : "+v"(a2));
                    }
                }
            }
            rs = rsn;
            ru = run;
        }
        if constexpr (TNS) {
            // threads of one torch-lane set (t & 1 / t & 3) summed by the butterfly's upper steps;
            // then wave lane l & 7 takes torch lane l & 7 from a thread that holds it
            constexpr int SETS = COMPAT ? 4 : 2;
            const int l7 = lane & 7;
            double tv = 0.0;
#pragma unroll
            for (int u = 0; u < NTA; ++u) {
                double v = ta[u];
#pragma unroll
                for (int o = 32; o >= SETS; o >>= 1) v += __shfl_xor(v, o, WAVE);
                v = __shfl(v, l7 / NTA, WAVE);
                tv = (l7 % NTA) == u ? v : tv;
            }
            a2 = tv;
        } else {
            a2 = wave_sum(a2);                               // fixed butterfly: deterministic
        }
        const bool fits = cnt <= GCAP;
        const uint32_t base = (uint32_t)gi * GCAP;
        // Classification of the staged candidates (LDS and ALU only: no vector-memory op between
        // the item's loads and its fixed store sequence).  Sure entries go to stage16, half h's at
        // h * DS_HCAP; ambiguous ones are compacted in place in sg (a batch reads its 64 slots
        // before it writes lower ones).
        uint32_t na = 0;
        uint32_t hs[NH];
#pragma unroll
        for (int u = 0; u < NH; ++u) hs[u] = 0;
        {
            const float q0 = sload(ws.q0 + row), q1 = sload(ws.q1 + row);
            const uint32_t rk2 = rk ^ 0x27D4EB2Fu;
            const uint32_t j0 = (uint32_t)(gi * (FGS * CHUNK));
            const uint32_t ncl = (fits && PROBE != 6) ? cnt : 0u;     // probe 6: no classification
            // CU batches of 64 per iteration: their LDS reads and draw hashes are independent, so
            // they overlap; only the compaction (ballot / mbcnt counters) runs batch after batch.
            // All CU batches are read before any in-place write (writes go below e0 + 64 CU).
            constexpr int CU = FLC_DS_CU;
            for (uint32_t e0 = 0; e0 < ncl; e0 += 64 * CU) {
                uint2 en[CU];
                float hf[CU], hfu[CU];
                uint32_t hi8[CU];
                bool vv[CU];
#pragma unroll
                for (int b = 0; b < CU; ++b) {
                    const uint32_t e = e0 + (uint32_t)(b * 64 + lane);
                    vv[b] = e < ncl;
                    en[b] = vv[b] ? sg[e] : make_uint2(0u, 0u);
                }
#pragma unroll
                for (int b = 0; b < CU; ++b) {
                    const uint32_t loc = en[b].x & 0x1FFFu;
                    hi8[b] = 0;
                    if constexpr (COMPAT) {
                        const uint32_t e = e0 + (uint32_t)(b * 64 + lane);
                        const float ud = vv[b] ? sgf[e] : 0.f;
                        hf[b] = ud;
                        hfu[b] = __uint_as_float(__float_as_uint(ud) + 1u);
                    } else {
                        hi8[b] = ds_hi8(j0 + loc, rk);
                        const uint32_t h24 = (hi8[b] << 16) | (fmix32(colbase(j0 + loc) + rk2) >> 16);   // h >> 8
                        hf[b] = (float)h24 * 0x1p-24f;                      // hf <= draw / 2^32 <= hfu
                        hfu[b] = (float)(h24 + 1u) * 0x1p-24f;
                    }
                }
#pragma unroll
                for (int b = 0; b < CU; ++b) {
                    if (e0 + (uint32_t)(b * 64) >= ncl) break;       // wave-uniform
                    const float x = __uint_as_float(en[b].y), ax = fabsf(x);
                    const uint32_t loc = en[b].x & 0x1FFFu;
                    const bool inl = ax * q0 <= 1.0f - 0x1p-18f;
                    const bool nz = vv[b] && !(x == 0.f);
                    const bool sure = nz && inl && fmaf(ax, q1, hf[b]) >= 1.0f + 0x1p-20f;
                    const bool drop = !nz || (inl && fmaf(ax, q0, hfu[b]) < 1.0f - 0x1p-20f);
                    const bool amb = !sure && !drop;
                    const uint32_t u = loc >> 11;
                    uint32_t pin = 0;
#pragma unroll
                    for (int h = 0; h < NH; ++h) {
                        const uint64_t mh = __ballot(sure && u == (uint32_t)h);
                        const uint32_t ph = __builtin_amdgcn_mbcnt_hi((uint32_t)(mh >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mh, hs[h]));
                        pin = u == (uint32_t)h ? ph : pin;
                        hs[h] += (uint32_t)__popcll(mh);
                    }
                    if (sure && pin < (uint32_t)DS_HCAP)
                        s16[u * DS_HCAP + pin] = (uint16_t)((loc & (HCHUNK - 1)) | ((en[b].y >> 31) << 11) | (1u << 12));
                    const uint64_t ma = __ballot(amb);
                    const uint32_t pa = __builtin_amdgcn_mbcnt_hi((uint32_t)(ma >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ma, na));
                    if (amb) sg[pa] = make_uint2(loc | (hi8[b] << 13), en[b].y);      // k_ds_resolve's entry
                    na += (uint32_t)__popcll(ma);
                }
            }
        }
        bool ovf = !fits;
#pragma unroll
        for (int u = 0; u < NH; ++u) ovf |= hs[u] > (uint32_t)DS_HCAP;
        // The item's stores: a FIXED sequence of DS_ITEM_STORES vector-memory ops with no exec
        // branch (every lane stores; duplicate lanes write equal values to equal addresses; the
        // copy-outs are range-checked by their buffer descriptors).  The stores sit in the
        // in-order vmcnt queue in front of the loads issued after them; with one fixed sequence on
        // every path (the prologue issues the same count of dropped stores) the compiler's static
        // vmcnt waits count them exactly instead of draining part of the ring.
        if constexpr (TNS) ws.tsum[(row * G + gi) * 8 + (lane & 7)] = a2;   // (8 lanes' values, each 8 times)
        else ws.partial[row * G + gi] = a2;
        ws.itm[gi * n + row] = ovf ? DS_OVF : na;
        {
            const uint32_t u = (uint32_t)lane & (NH - 1);
            uint32_t hc = 0;
#pragma unroll
            for (int v = 0; v < NH; ++v) hc = (uint32_t)v == u ? hs[v] : hc;
            // halves past the row end land in the tab's padding rows (G * NH >= H)
            ws.tabs[(gi * NH + u) * n + row] = make_uint2(0u, ovf ? 0u : hc);
        }
        {
            // sure entries: lane l holds entries 8 (l % 16) .. + 8 of half l / 16; slots past the
            // half's count are sent out of range (dropped) by their offset, not by an exec branch
            static_assert(DS_HCAP == 128 && GCAP == 512, "sure copy-out: 16 lanes x 16 B per half");
            const uint32_t u = (uint32_t)lane >> 4, k8 = ((uint32_t)lane & 15u) * 8u;
            uint32_t hc = 0;
#pragma unroll
            for (int v = 0; v < NH; ++v) hc = (uint32_t)v == u ? hs[v] : hc;
            const bool put = !ovf && k8 < hc;
            // half u's region of this row: ent16[gi * NH + u][row], n * DS_HCAP entries apart
            const uint32_t hstride = (uint32_t)n * (DS_HCAP * 2);               // bytes
            const auto od = __builtin_amdgcn_make_buffer_rsrc(ws.ent16 + ((int64_t)gi * NH * n + row) * DS_HCAP, (short)0,
                                                              (int)((NH - 1) * hstride + DS_HCAP * 2), 0x00020000);
            const uint4 v = reinterpret_cast<const uint4*>(s16)[lane];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned int, v), od,
                                                   put ? u * hstride + k8 * 2u : 0x7FFFFFF0u, 0, FLC_DS_STPOL);
        }
        {
            // ambiguous entries: two per lane per 16-B store; an odd count's last slot is stale
            const uint32_t nrec = ovf ? 0u : ((na + 1u) & ~1u) * 8u;
            const auto od = __builtin_amdgcn_make_buffer_rsrc(ws.enta + row * ws.cap + base, (short)0, (int)nrec, 0x00020000);
            const uint4* sq = reinterpret_cast<const uint4*>(sg);
#pragma unroll
            for (int k = 0; k < GCAP / 128; ++k) {
                const uint4 v = sq[k * 64 + lane];
                __builtin_amdgcn_raw_buffer_store_b128(
                    __builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned int, v), od, (k * 64 + lane) * 16, 0, FLC_DS_STPOL);
            }
        }
        // the copy-out reads precede the next item's staging writes in the wave's program order
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        it = nit;
        row = nrow;
        c = nc;
    }
}

// ------------------------------------------------------------------------------------------
// Norm and row mode: one wave per row.
// ------------------------------------------------------------------------------------------
// GIVEN: the row's norm comes from `given` (the caller's norms, or k_tn_walk's in the torch-order
// mode) instead of the filter's partials; everything else — the bounds, overflow and weight checks
// that send a row to the dense fold, DS_FAST, rpn, pnorm_out — is the same.
template <bool GIVEN>
__global__ __launch_bounds__(256) void k_ds_final(int64_t r0, int64_t rn, DsWs ws, const float* __restrict__ w,
                                                  float* __restrict__ pnorm_out, const float* given) {
    const int lane = threadIdx.x & 63;
    const int64_t row = r0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= r0 + rn) return;
    double a = 0.0;
    uint32_t ov = 0;
    int64_t k = lane;
    for (; k + 7 * 64 < ws.G; k += 8 * 64) {                 // 8 far loads per round trip, same order
        double v[8];
        uint32_t t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { v[u] = GIVEN ? 0.0 : ws.partial[row * ws.G + k + u * 64]; t[u] = ws.itm[(k + u * 64) * ws.n + row]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { a += v[u]; ov |= t[u] == DS_OVF; }
    }
    for (; k < ws.G; k += 64) { a += GIVEN ? 0.0 : ws.partial[row * ws.G + k]; ov |= ws.itm[k * ws.n + row] == DS_OVF; }
    a = wave_sum(a);
    ov = __ballot(ov != 0u) != 0ull;
    if (lane == 0) {
        const float nv = GIVEN ? given[row] : (float)sqrt(a);
        ws.pn[row] = nv;
        if (pnorm_out) pnorm_out[row] = nv;
        ws.rpn[row] = 1.0f / nv;
        uint32_t fl = ws.flags[row];
        const bool wbad = w && !(fabsf(w[row]) <= 3.4028235e38f);
        if (!(nv >= ws.nlo[row]) || !(nv <= ws.nhi[row]) || !(nv <= 3.4028235e38f) || ov || wbad) fl |= DS_DENSE;
        if (nv >= 0x1p-40f && nv <= 0x1p80f) fl |= DS_FAST;   // |x| / norm may use div_fast
        ws.flags[row] = fl;
    }
}

// Row state of the exact encode (wave-uniform).
struct DsRow {
    float n, rn;          // norm, RN(1 / norm)
    uint32_t rk2;         // row key of the low draw: rk ^ 0x27D4EB2F (common.hpp dev_draw)
    bool fast;            // norm inside the div_fast window
};

// The level C(x)_j of standard dithering (compressors.py:270-299) picks for one element, exactly as
// DitherOp::apply<false> (codec_ops.hpp) computes it: the draw's top byte comes with the entry
// (hi8), and the rare slow cases (|x| or a level gap outside the fast-division window, the
// interval guess off by one) are taken behind wave-level branches instead of being if-converted.
// Returns the level's value (0 outside every interval) and index (-1 there).
struct DsLev {
    float v;
    int idx;
};
// COMPAT: the draw is the caller's float64 uniform ud, against p = p2 * 2^-32 as DitherOp<.., true>.
template <bool COMPAT>
__device__ inline DsLev ds_level(float x, uint32_t j, uint32_t hi8, double ud, const DsRow& r, const float4* tab, int s,
                                 float sf) {
    const float ax = fabsf(x);
    FastDiv dn;
    dn.b = r.n; dn.rb = r.rn; dn.ok = true;
    float y = div_fast(ax, dn);                                   // |x| / pnorm
    const bool slow = !(r.fast && (ax >= 0x1p-80f || ax == 0.f) && ax <= 0x1p80f);
    if (__builtin_expect(__ballot(slow) != 0ull, 0)) {
        if (slow) y = ax / r.n;
    }
    int g = (int)(y * sf);                                        // y >= 0; NaN -> 0
    g = g > s - 1 ? s - 1 : g;
    float4 t = tab[g];
    const bool off = (y < t.x) | (y >= t.y);                      // on the upper level: the next interval's
    if (__builtin_expect(__ballot(off) != 0ull, 0)) {            // std levels RN(k/s): at most one off
        if (off) {
            g = (y < t.x) ? (g > 0 ? g - 1 : 0) : (g < s - 1 ? g + 1 : g);
            t = tab[g];
        }
    }
    const bool in = y <= t.y;                                     // y > 1 or NaN: no interval -> 0
    const float num = y - t.y;
    FastDiv dd;
    dd.b = t.z; dd.rb = t.w; dd.ok = true;
    float p2 = div_fast(num, dd);                                 // p * 2^32
    const bool gap_slow = t.w == 0.f;                             // gap outside the window (load_table)
    if (__builtin_expect(__ballot(gap_slow) != 0ull, 0)) {
        if (gap_slow) p2 = num / t.z;
    }
    bool down;
    if constexpr (COMPAT) {
        down = ud < (double)ldexpf(p2, -32);
    } else {
        uint32_t thr;
        asm("v_cvt_u32_f32 %0, %1" : "=v"(thr) : "v"(ceilf(p2)));   // saturating: thr32(p)
        // draw h = hi8 << 24 | lo24 against thr: the top byte decides unless it equals thr's (1 in
        // 256), so the low hash is computed only for those lanes
        const uint32_t th = thr >> 24;
        down = hi8 < th;
        const bool tie = hi8 == th;
        if (__builtin_expect(__ballot(tie) != 0ull, 0)) {
            if (tie) down = ((hi8 << 24) | (fmix32(colbase(j) + r.rk2) >> 8)) < thr;
        }
    }
    DsLev l;
    l.v = in ? (down ? t.x : t.y) : 0.f;
    l.idx = in ? (down ? g : g + 1) : -1;
    return l;
}

// C(x)_j: (lev * sign(x)) * pnorm
template <bool COMPAT>
__device__ inline float ds_encode(float x, uint32_t j, uint32_t hi8, double ud, const DsRow& r, const float4* tab, int s,
                                  float sf) {
    const DsLev l = ds_level<COMPAT>(x, j, hi8, ud, r, tab, s, sf);
    // the sign by compare and the zero times the norm, as DitherOp::apply
    return ((x == 0.f) ? 0.f : (x < 0.f ? -l.v : l.v)) * r.n;
}


// ------------------------------------------------------------------------------------------
// Resolve: one wave per 64 filter items — item gi of 64 consecutive rows, one lane each, so the
// per-item tables ([item][row]) are read and written coalesced; their ambiguous candidates,
// spread over the wave's lanes, encoded with their rows' norms; the nonzero ones appended as list
// entries after the sure entries of their half chunk (an LDS counter per (item, half): the order
// inside one row's list is free, its columns are distinct), the counts into cntr.  A level above
// DS_MAXLEV or a full half region turns the row dense.
// ------------------------------------------------------------------------------------------
template <bool COMPAT>
__global__ __launch_bounds__(256) void k_ds_resolve(int64_t n, int64_t r0, int64_t rn, DsWs ws,
                                                    const float* __restrict__ levels, int s, UniformSrc us) {
    constexpr int NH = DS_NH;
    __shared__ __attribute__((aligned(16))) float4 tab[DS_MAXS];
    __shared__ uint32_t pre[4][65], irow[4][64], igi[4][64], ikey[4][64], imode[4][64], cs[4][64][NH], cr[4][64][NH];
    __shared__ float ipn[4][64], irpn[4][64];
    __shared__ int own[4][64];
    load_table(levels, s, tab);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float sf = (float)s;
    const int64_t nrb = (rn + 63) / 64, groups = nrb * ws.G;
    for (int64_t grp = (int64_t)blockIdx.x * 4 + wv; grp < groups; grp += (int64_t)gridDim.x * 4) {
        const uint32_t gi = (uint32_t)(grp / nrb);
        const int64_t row = r0 + (grp - (int64_t)gi * nrb) * 64 + lane;
        const bool valid = row < r0 + rn;
        uint32_t na = 0, mode = DS_DENSE;
        if (valid) {
            mode = ws.flags[row];
            if (!(mode & DS_DENSE)) na = ws.itm[(int64_t)gi * n + row];
        }
        // exclusive prefix of na over the lanes
        uint32_t inc = na;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o, 64);
            inc += lane >= o ? t : 0u;
        }
        const uint32_t total = __shfl(inc, 63, 64);
        pre[wv][lane] = inc - na;
        if (lane == 0) pre[wv][64] = total;
        irow[wv][lane] = (uint32_t)row;
        igi[wv][lane] = gi;
        ikey[wv][lane] = (valid ? ws.rk[row] : 0u) ^ 0x27D4EB2Fu;
        imode[wv][lane] = mode;
        ipn[wv][lane] = valid ? ws.pn[row] : 1.f;
        irpn[wv][lane] = valid ? ws.rpn[row] : 1.f;
#pragma unroll
        for (int u = 0; u < NH; ++u) {
            cs[wv][lane][u] = (na > 0u) ? ws.tabs[((int64_t)gi * NH + u) * n + row].y : 0u;
            cr[wv][lane][u] = 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // The candidates of the 64 items, flattened: slot t belongs to the last lane k with
        // pre[k] <= t.  Per window of 64 slots the owners come from marks (lane k with candidates
        // writes its lane id at slot pre[k] - t0) and a max-scan over the lanes (owners rise with
        // the slot), slots before the window's first mark taking the previous window's last owner;
        // the next window's owners and candidate loads are issued before this window is encoded.
        const uint32_t mypre = inc - na;
        uint32_t carry = 0;
        auto owner = [&](uint32_t t0) -> uint32_t {
            own[wv][lane] = -1;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            if (na > 0u && mypre >= t0 && mypre < t0 + 64u) own[wv][mypre - t0] = lane;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            int v = own[wv][lane];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int w = __shfl_up(v, o, 64);
                v = (lane >= o && w > v) ? w : v;
            }
            const uint32_t k = v < 0 ? carry : (uint32_t)v;
            carry = __shfl(k, 63, 64);
            return k;
        };
        auto fetch = [&](uint32_t t0, uint32_t k) -> uint2 {
            const uint32_t t = t0 + (uint32_t)lane;
            const uint32_t e = t - pre[wv][k];
            const int64_t ei = t < total ? (int64_t)irow[wv][k] * ws.cap + (int64_t)igi[wv][k] * DS_GCAP + e : 0;
            const uint2 v = ws.enta[ei];                          // lanes past the total: entry 0 (ignored)
            return v;
        };
        // The first RW windows' owners and candidate loads are all issued before any is encoded
        // (their gathers from 64 rows' regions overlap instead of costing one round trip each);
        // windows past RW are fetched one ahead.
        constexpr int RW = FLC_DS_RW;
        uint32_t kw[RW];
        uint2 ew[RW];
#pragma unroll
        for (int w = 0; w < RW; ++w) {
            kw[w] = 0u;
            ew[w] = make_uint2(0u, 0u);
            if ((uint32_t)w * 64u < total) { kw[w] = owner((uint32_t)w * 64u); ew[w] = fetch((uint32_t)w * 64u, kw[w]); }
        }
        uint32_t kc = 0;
        uint2 enc = make_uint2(0u, 0u);
        if ((uint32_t)RW * 64u < total) { kc = owner((uint32_t)RW * 64u); enc = fetch((uint32_t)RW * 64u, kc); }
        for (uint32_t t0 = 0; t0 < total; t0 += 64) {
            const uint32_t t = t0 + (uint32_t)lane;
            const bool tv = t < total;
            const uint32_t wi = t0 >> 6;
            uint32_t k = kc;
            uint2 en = enc;
            if (wi < (uint32_t)RW) {
#pragma unroll
                for (int w = 0; w < RW; ++w)
                    if ((uint32_t)w == wi) { k = kw[w]; en = ew[w]; }
            } else if (t0 + 64u < total) {
                const uint32_t kn = owner(t0 + 64u);
                const uint2 nn = fetch(t0 + 64u, kn);
                k = kc; en = enc;
                kc = kn; enc = nn;
            }
            en = tv ? en : make_uint2(0u, 0u);
            const int64_t rk_ = irow[wv][k];
            const uint32_t gk = igi[wv][k];
            const float x = __uint_as_float(en.y);
            const uint32_t loc = en.x & 0x1FFFu;
            DsRow rr;
            rr.n = ipn[wv][k];
            rr.rn = irpn[wv][k];
            rr.rk2 = ikey[wv][k];
            rr.fast = (imode[wv][k] & DS_FAST) != 0u;
            const uint32_t j = gk * (uint32_t)(DS_FGS * CHUNK) + loc;
            double ud = 0.0;                                  // compat: the element's uniform
            if constexpr (COMPAT) ud = us.u[(tv ? rk_ : 0) * us.uld + (tv ? j : 0u)];
            const DsLev l = ds_level<COMPAT>(x, j, en.x >> 13, ud, rr, tab, s, sf);
            const bool keep = tv && !(x == 0.f) && l.idx > 0 && !(l.v == 0.f);
            if (keep) {
                const uint32_t u = loc >> 11;
                const uint32_t slot = atomicAdd(&cr[wv][k][u], 1u);
                const uint32_t pos = cs[wv][k][u] + slot;
                if (l.idx > DS_MAXLEV || pos >= (uint32_t)DS_HCAP) {
                    atomicOr(&ws.flags[rk_], DS_DENSE);
                } else {
                    ws.ent16[(((int64_t)gk * NH + u) * n + rk_) * DS_HCAP + pos] =
                        (uint16_t)((loc & (HCHUNK - 1)) | ((en.y >> 31) << 11) | ((uint32_t)l.idx << 12));
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (valid && na > 0u) {
#pragma unroll
            for (int u = 0; u < NH; ++u) ws.cntr[((int64_t)gi * NH + u) * n + row] = cr[wv][lane][u];
        } else if (valid) {
#pragma unroll
            for (int u = 0; u < NH; ++u) ws.cntr[((int64_t)gi * NH + u) * n + row] = 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

// ------------------------------------------------------------------------------------------
// Chunk-owner fold.  One wave per half chunk, fp32 LDS tile, rows in order; per row its list
// (sure + resolved entries: copysign(levels[level], sign) * norm) — the first 64 entries from a
// 64-row batch's list windows, brought into LDS a batch ahead, the rest read in place — or, for
// DENSE rows, the half chunk of x itself, encoded.  Contributions are W ? w_i * C(x)_j : C(x)_j.
// ------------------------------------------------------------------------------------------
struct DsMeta {
    uint32_t off, cnt;
    float pn, rpn, w;
    uint32_t rk, mode;
};

__device__ inline DsMeta ds_meta(const DsWs& ws, int64_t c, int64_t n, int64_t rend, int64_t r, const float* w) {
    DsMeta m;
    m.off = 0; m.cnt = 0;
    m.pn = 1.f; m.rpn = 1.f; m.w = 1.f; m.rk = 0; m.mode = 0;
    if (r < rend) {
        // every load issued at once (no flags -> tab dependency): a dense row's count is dropped below
        m.pn = ws.pn[r];
        m.rpn = ws.rpn[r];
        m.rk = ws.rk[r];
        m.mode = ws.flags[r];
        const uint32_t c0 = ws.tabs[c * n + r].y, c1 = ws.cntr[c * n + r];   // c: half-chunk index
        m.cnt = (m.mode & DS_DENSE) ? 0u : c0 + c1;
        if (w) m.w = w[r];
    }
    return m;
}

// ds_meta without anything computed from the loads: off = sure entries, cnt = resolved entries
// (their sum is the list length of a non-dense row), mode = the row's flags
__device__ inline DsMeta ds_meta_raw(const DsWs& ws, int64_t c, int64_t n, int64_t rend, int64_t r, const float* w) {
    DsMeta m;
    m.off = 0; m.cnt = 0;
    m.pn = 1.f; m.rpn = 1.f; m.w = 1.f; m.rk = 0; m.mode = 0;
    if (r < rend) {
        m.pn = ws.pn[r];
        m.rpn = ws.rpn[r];
        m.rk = ws.rk[r];
        m.mode = ws.flags[r];
        m.off = ws.tabs[c * n + r].y;
        m.cnt = ws.cntr[c * n + r];
        if (w) m.w = w[r];
    }
    return m;
}

#ifndef FLC_DS_AW
#define FLC_DS_AW 1                  // waves per fold workgroup (LDS: an 8 KB tile and 8 KB of list windows per wave)
#endif
constexpr int DS_AW = FLC_DS_AW;
// the compiler's occupancy model of the 16 KB of LDS per wave gives up on any waves-per-EU target
// (it then takes 400 registers): cap the registers explicitly (4 waves per SIMD: 128)
#define FLC_DS_ACCUM_ATTR __attribute__((amdgpu_num_vgpr(128)))

// Folds rows [r0, r0 + rn) into the running sums: the first group starts the tiles at -0, the others
// continue from `part` (the previous group's tiles); the last group resolves untouched columns
// over ALL n rows and writes out = sums / wt, the others write their tiles back to `part`.
// Small workgroups with only the tile and the list windows in LDS (the dense rows' level table is
// ws.gtab) for this latency-bound walk.
// SRC = DiffSrc (the one-read shifted round): every place that reads a row — a dense row's
// re-encode and the sign-of-zero pass over the -0 columns — reads a - b.
// AP is only a name now (once a register ring's depth): kept as part of the symbols the profiles and traces name.
template <bool W, int AP, bool COMPAT, class SRC = RowSrc>
__global__ __launch_bounds__(64 * DS_AW) FLC_DS_ACCUM_ATTR void k_ds_accum(SRC rows, int64_t n, int64_t r0, int64_t rn, int first, int last,
                                                  int64_t d, DsWs ws, const float* __restrict__ levels, int s,
                                                  const float* __restrict__ w, float wt, float* __restrict__ part,
                                                  float* __restrict__ out, UniformSrc us) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    __shared__ __attribute__((aligned(16))) float tile[DS_AW][HCHUNK];
    __shared__ __attribute__((aligned(16))) uint16_t dstg[DS_AW][8][512];   // a 64-row batch's list windows: 8 KB per wave
    __shared__ float lvl[DS_MAXLEV + 1];
    if (threadIdx.x <= (unsigned)DS_MAXLEV) lvl[threadIdx.x] = (int)threadIdx.x <= s ? levels[threadIdx.x] : 0.f;
    __syncthreads();
    const float4* tab = ws.gtab;
    const int lane = threadIdx.x & 63;
    const int wv = DS_AW == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t H = nhalves(d);
    float* tl = tile[wv];
    const int64_t rend = r0 + rn;
    const int64_t nb = (rn + 63) / 64;
    const float sf = (float)s;
    for (int64_t h = (int64_t)blockIdx.x * DS_AW + wv; h < H; h += (int64_t)gridDim.x * DS_AW) {
        // The tile starts at -0.0: (-0) + t == t for every nonzero t, and a column that received a
        // nonzero contribution never returns to -0 (x + y == -0 needs two -0 addends), so a final
        // -0 bit pattern marks exactly the untouched columns.  Zero contributions are not added.
        // Adds are read-modify-writes of the wave's own tile, in row order (one wave executes its
        // LDS operations in program order; the lanes of one instruction hit distinct columns), so
        // each column sees its rows' terms in row order.
        const uint32_t hbase = (uint32_t)(h * HCHUNK);
        const int64_t len = min((int64_t)HCHUNK, d - (int64_t)hbase);
        if (FLC_TILE_V4 && !first && len == HCHUNK) {
            // the carried tile with every load in flight at once (the loop of load -> LDS write
            // pairs below waits one memory latency per 64 columns: 32 per tile)
            const float4* p4 = reinterpret_cast<const float4*>(part + hbase);
            float4 v[HCHUNK / 256];
#pragma unroll
            for (int k = 0; k < HCHUNK / 256; ++k) v[k] = p4[k * 64 + lane];
#pragma unroll
            for (int k = 0; k < HCHUNK / 256; ++k) reinterpret_cast<float4*>(tl)[k * 64 + lane] = v[k];
        } else {
            for (int i = lane; i < HCHUNK; i += 64) tl[i] = (first || i >= len) ? -0.f : part[hbase + i];
        }
        DsMeta cur = ds_meta_raw(ws, h, n, rend, r0 + lane, w), nxt;
        // (LDS float atomic adds instead of the read-modify-write — one wave's LDS operations run
        // in issue order, so the row order would hold — measured 1.34 against 0.51 ms at C4)
        auto add = [&](uint32_t loc, float t) {
            if (!(t == 0.f)) tl[loc] = tl[loc] + t;
        };
        auto value = [&](uint32_t e, float pn) {            // copysign(levels[lev], sign) * pnorm
            const float lv = lvl[(e >> 12) & 15u];
            return __uint_as_float(__float_as_uint(lv) | ((e & 0x800u) << 20)) * pn;
        };
        auto row_state = [&](const DsMeta& m, int q, float& pn, float& wi) {
            pn = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(m.pn), q));
            wi = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(m.w), q));
        };
        // Wide batches through LDS DMA: a 64-row batch's list windows (the first 128 B of each row's
        // region, loaded whatever the row's count, rows clamped to the array's last row, and masked
        // with the count where the row is folded: the load address needs no row state) are 8 loads
        // of 16 B per lane straight into the wave's 8 KB staging (lane l: row l / 8 of its 8-row
        // slot, bytes 16 (l % 8) ..), issued a whole batch ahead.  The compiler waits for every
        // outstanding load before the first staging read (vmcnt(0): it does not track LDS DMA per
        // slot), so each batch reads all its 64 entries per lane first, then issues the next
        // batch's 8 loads and its row state, then folds the 64 rows: each batch's loads have a
        // whole batch of folding to arrive in.
        int64_t b = 0;
        auto dma = [&](int64_t row0, int sl) {
            const uint16_t* src = ws.ent16 + (h * n + min(row0 + (lane >> 3), n - 1)) * DS_HCAP + (lane & 7) * 8;
            __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)&dstg[wv][sl][0], 16, 0, 0);
        };
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) dma(r0 + 8 * sl, sl);
        for (; b < nb; ++b) {
            const int64_t i0 = r0 + b * 64;
            if (__ballot((cur.mode & DS_DENSE) != 0u) != 0ull) break;
            // rows with more than 64 entries in this half (~1e-4 of C4's): the batch takes the rolled
            // path below, which reads the rest of their lists directly
            const uint64_t lng = __ballot(cur.off + cur.cnt > 64u);
            if (__builtin_expect(lng == 0ull, 1)) {
                // the batch's 64 entries of this lane, two rows per register
                uint32_t ent2[32];
#pragma unroll
                for (int q = 0; q < 64; q += 2)
                    ent2[q >> 1] = (uint32_t)dstg[wv][q >> 3][(q & 7) * 64 + lane] |
                                   ((uint32_t)dstg[wv][(q + 1) >> 3][((q + 1) & 7) * 64 + lane] << 16);
                __builtin_amdgcn_s_waitcnt(0xC07F);                  // lgkmcnt(0): the slots are read
                // the next batch's row state, raw (nothing computed from it before the next batch: a
                // use here would wait for the loads behind it), then its list windows
                nxt = ds_meta_raw(ws, h, n, rend, i0 + 64 + lane, w);
#pragma unroll
                for (int sl = 0; sl < 8; ++sl) dma(i0 + 64 + 8 * sl, sl);
#pragma unroll
                for (int q = 0; q < 64; ++q) {
                    // rows in order; the scheduler does not hoist 64 rows' work (register pressure)
                    __builtin_amdgcn_sched_barrier(0);
                    float pn, wi;
                    row_state(cur, q, pn, wi);
                    // (no dense row in the batch: the count is the sure + resolved entries)
                    const uint32_t cnt = __builtin_amdgcn_readlane(cur.off, q) + __builtin_amdgcn_readlane(cur.cnt, q);
                    const uint32_t raw = (q & 1) ? (ent2[q >> 1] >> 16) : (ent2[q >> 1] & 0xFFFFu);
                    const uint32_t a = (uint32_t)lane < cnt ? raw : NONE;
                    const float e = value(a, pn);
                    if (a != NONE) add(a & (HCHUNK - 1), W ? wi * e : e);
                }
            } else {
#pragma unroll 1
                for (int q = 0; q < 64; ++q) {
                    float pn, wi;
                    row_state(cur, q, pn, wi);
                    const uint32_t cnt = __builtin_amdgcn_readlane(cur.off, q) + __builtin_amdgcn_readlane(cur.cnt, q);
                    const uint32_t raw = dstg[wv][q >> 3][(q & 7) * 64 + lane];
                    const uint32_t a = (uint32_t)lane < cnt ? raw : NONE;
                    const float e = value(a, pn);
                    if (a != NONE) add(a & (HCHUNK - 1), W ? wi * e : e);
                    const int64_t row = i0 + q;
                    for (uint32_t kk = 64u + lane; kk < cnt; kk += 64) {
                        const uint32_t en = ws.ent16[(h * n + row) * DS_HCAP + kk];
                        const float ev = value(en, pn);
                        add(en & (HCHUNK - 1), W ? wi * ev : ev);
                    }
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);                  // lgkmcnt(0): the slots are read
                nxt = ds_meta_raw(ws, h, n, rend, i0 + 64 + lane, w);
#pragma unroll
                for (int sl = 0; sl < 8; ++sl) dma(i0 + 64 + 8 * sl, sl);
            }
            cur = nxt;
        }
        // rows from the batch with a dense row on, one at a time (rare: a row outside its sample's
        // norm bounds, an overflowed item, a non-finite row or weight)
        for (int64_t row = r0 + b * 64; row < rend; ++row) {
            const uint32_t mode = ws.flags[row];
            const float pn = ws.pn[row], wi = W ? w[row] : 1.f;
            if (mode & DS_DENSE) {
                // dense row: every element of the half chunk, coalesced
                DsRow rr;
                rr.n = pn;
                rr.rn = ws.rpn[row];
                const uint32_t rk = ws.rk[row];
                rr.rk2 = rk ^ 0x27D4EB2Fu;
                rr.fast = (mode & DS_FAST) != 0u;
                const auto rp = row_ref(rows, row);
                for (int k = 0; k < HCHUNK / 64; ++k) {
                    const uint32_t e = (uint32_t)(k * 64 + lane);
                    if (e < (uint32_t)len) {
                        const uint32_t j = hbase + e;
                        const float xv = rp[(int64_t)hbase + e];
                        const float ev = COMPAT ? ds_encode<true>(xv, j, 0u, us.u[row * us.uld + j], rr, tab, s, sf)
                                                : ds_encode<false>(xv, j, ds_hi8(j, rk), 0.0, rr, tab, s, sf);
                        add(e, W ? wi * ev : ev);
                    }
                }
            } else {
                const uint32_t cnt = ws.tabs[h * n + row].y + ws.cntr[h * n + row];
                for (uint32_t k = lane; k < cnt; k += 64) {
                    const uint32_t en = ws.ent16[(h * n + row) * DS_HCAP + k];
                    const float ev = value(en, pn);
                    add(en & (HCHUNK - 1), W ? wi * ev : ev);
                }
            }
        }
        if (!last) {
            for (int64_t i = lane; i < len; i += 64) part[hbase + i] = tl[i];
            continue;
        }
        // untouched columns: every contribution was +-0; the sequential fold gives -0 only if all
        // are -0.  Sign of row i's zero: C(x) = copysign(0, x) * norm (+0 for x == 0), times w_i.
        for (int k = 0; k < HCHUNK / 64; ++k) {
            const int e = k * 64 + lane;
            bool neg = e < len && __float_as_uint(tl[e]) == 0x80000000u;
            if (__ballot(neg) == 0ull) continue;
            const bool mine = neg;
            for (int64_t i = 0; i < n && __ballot(neg) != 0ull; ++i) {
                if (neg) {
                    const float xv = row_ref(rows, i)[hbase + e];
                    const bool zs = (xv != 0.f) && (__float_as_uint(xv) >> 31);
                    const bool ws_ = W && (__float_as_uint(w[i]) >> 31);
                    neg = zs != ws_;
                }
            }
            if (mine) tl[e] = neg ? -0.f : 0.f;
        }
        for (int64_t i = lane; i < len; i += 64) out[hbase + i] = tl[i] / wt;
    }
}

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
// Filter grid.  The product build always takes the default; a -DFLC_TUNING build reads the
// A/B switches once per process (FLC_DS_GRID=res launches a resident-only grid; FLC_DS_GRIDPCT=p
// caps it at p % of the resident blocks when row groups run).
#ifndef FLC_DS_LDSPAD
#define FLC_DS_LDSPAD 5120           // row groups: extra LDS per filter block (bytes), room for the side tail
#endif
#ifndef FLC_DS_LASTPCT
#define FLC_DS_LASTPCT 100           // size of the last QSGD row group in % of the others (its tail is exposed)
#endif
static_assert(FLC_DS_LASTPCT >= 1 && FLC_DS_LASTPCT <= 100, "FLC_DS_LASTPCT: the last row group is 1..100 % of the others");
#ifndef FLC_DS_RESGRID
#define FLC_DS_RESGRID 0             // k_ds_filter: a resident grid (one round of blocks, grid-stride items)
#endif
#ifndef FLC_DS_SIDE_FOLD_WG
#define FLC_DS_SIDE_FOLD_WG 0        // a non-last row group's fold (beside the next filter): grid cap, 0 = one per half
#endif
#ifndef FLC_DS_SIDE_RES_WG
#define FLC_DS_SIDE_RES_WG 0         // a non-last row group's resolve: grid cap, 0 = one wave per 64 items
#endif
#ifndef FLC_DS_PROBE_SIDE
#define FLC_DS_PROBE_SIDE 0          // A/B probes: 1 skip the side resolve, 2 the side fold, 3 both (outputs NOT valid)
#endif
#ifndef FLC_DS_TNSUMS
// torch-order norm mode: 1 = the filter emits the torch lanes' sums (the rows are read twice:
// filter + k_tn_maps), 0 = the three-read composition (k_tn_sums reads them once more; the
// yardstick and the fallback).  Tuning builds: FLC_DS_TNSUMS=0|1 in the environment.
#define FLC_DS_TNSUMS 1
#endif
struct DsVariant { bool resident; int gridpct; int probe; int64_t rb; int cring; bool tnsums; };
static const DsVariant& ds_variant() {
    static const DsVariant v = [] {
        DsVariant r{false, 100, 0, DS_RB, DS_RINGC, FLC_DS_TNSUMS != 0};
        if (const char* e = tuning_env("FLC_DS_TNSUMS")) r.tnsums = atoi(e) != 0;
        if (const char* e = tuning_env("FLC_DS_CRING")) r.cring = atoi(e);
        if (const char* e = tuning_env("FLC_DS_RB")) r.rb = std::max<int64_t>(1, atoll(e));
        if (const char* e = tuning_env("FLC_DS_PROBE")) r.probe = atoi(e);
        if (const char* e = tuning_env("FLC_DS_GRIDPCT")) r.gridpct = std::max(10, std::min(100, atoi(e)));
        if (const char* e = tuning_env("FLC_DS_GRID")) r.resident = !strcmp(e, "res");
        return r;
    }();
    return v;
}

// The filter kernel of a call.  The product library carries five: device draws (ring 16) and the
// caller's uniforms (ring DS_RINGC), each with and without the torch lanes' sums, and the
// two-operand one.  The cost probes and the 8-deep compat ring are chosen by switches that only a
// -DFLC_TUNING build reads, so only that build instantiates them.
template <class SRC>
using DsFilterKernel = void (*)(SRC, int64_t, int64_t, int64_t, int64_t, int64_t, DsWs, UniformSrc);
template <class SRC>
static DsFilterKernel<SRC> ds_filter_kernel(const DsVariant& v, bool compat, bool tns) {
    if constexpr (std::is_same<SRC, DiffSrc>::value) {
        return k_ds_filter<8, DS_GCAP, 0, false, false, DiffSrc>;          // 8 pairs: the 16-float4 ring's bytes
    } else {
#ifdef FLC_TUNING
        if (compat && v.cring == 8) return tns ? k_ds_filter<8, DS_GCAP, 0, true, true> : k_ds_filter<8, DS_GCAP, 0, true>;
        if (!compat && !tns) {
            switch (v.probe) {
            case 1: return k_ds_filter<16, DS_GCAP, 1>;
            case 2: return k_ds_filter<16, DS_GCAP, 2>;
            case 3: return k_ds_filter<16, DS_GCAP, 3>;
            case 4: return k_ds_filter<16, DS_GCAP, 4>;
            case 5: return k_ds_filter<16, DS_GCAP, 5>;
            case 6: return k_ds_filter<16, DS_GCAP, 6>;
            }
        }
#endif
        if (compat) return tns ? k_ds_filter<DS_RINGC, DS_GCAP, 0, true, true> : k_ds_filter<DS_RINGC, DS_GCAP, 0, true>;
        return tns ? k_ds_filter<16, DS_GCAP, 0, false, true> : k_ds_filter<16, DS_GCAP>;
    }
}

// tn (the torch-order norm mode): the filter's per-lane sums and torch_norm.hip's workspace
// behind everything the exact mode carves (whose layout and size do not change)
static DsWs carve_ds(void* base, int64_t n, int64_t d, size_t* bytes, bool tn = false, void** tnws = nullptr) {
    Carver cv(base);
    const int64_t C = std::max<int64_t>(nchunks(d), 1), H = std::max<int64_t>(nhalves(d), 1);
    const int64_t nn = std::max<int64_t>(n, 1);
    DsWs w;
    w.G = (C + DS_FGS - 1) / DS_FGS;
    w.n = nn;
    w.cap = w.G * DS_GCAP;
    const size_t tabn = (size_t)std::max<int64_t>(H, w.G * DS_NH) * nn;         // + padding halves
    w.tabs = cv.take<uint2>(tabn);
    w.cntr = cv.take<uint32_t>(tabn);
    w.ent16 = cv.take<uint16_t>((size_t)nn * w.cap);
    w.enta = cv.take<uint2>((size_t)nn * w.cap);
    w.itm = cv.take<uint32_t>((size_t)nn * w.G);
    w.flags = cv.take<uint32_t>(nn);
    w.qc = cv.take<float>(nn);
    w.nlo = cv.take<float>(nn);
    w.nhi = cv.take<float>(nn);
    w.q0 = cv.take<float>(nn);
    w.q1 = cv.take<float>(nn);
    w.partial = cv.take<double>((size_t)nn * w.G);
    w.pn = cv.take<float>(nn);
    w.rpn = cv.take<float>(nn);
    w.rk = cv.take<uint32_t>(nn);
    w.part = cv.take<float>((size_t)std::max<int64_t>(d, 1));
    w.gtab = cv.take<float4>(DS_MAXS);
    w.tsum = nullptr;
    if (tn) {
        w.tsum = cv.take<double>((size_t)nn * w.G * 8);
        char* t = cv.take<char>(norm_torch_ws_bytes(nn, d));
        if (tnws) *tnws = t;
    }
    if (bytes) *bytes = cv.bytes();
    return w;
}

// Path choice: the sparse path pays when the expected candidate share (s / sqrt(D), the hi8
// slack) keeps a filter item well inside its staging capacity.  The caller's hint
// (flc_codec_params.flags & FLC_PATH_MASK: FLC_PATH_SPARSE / FLC_PATH_DENSE) forces one; both
// paths give the same bits.

bool ds_eligible(const flc_codec_params* prm, const flc_pattern* pat, int64_t n, int64_t d) {
    if (prm->codec != FLC_STD_DITHERING || prm->norm != FLC_NORM_L2) return false;
    if (prm->s < 1 || prm->s > DS_MAXS - 1 || !prm->d_levels || n < 1 || d < 1) return false;
    if (d >= (int64_t)0x7FFFFFFF) return false;
    const int m = prm->flags & FLC_PATH_MASK;
    if (m) return m == FLC_PATH_SPARSE;
    const double share = 1.1 * (double)prm->s / sqrt((double)d) + 0.003;
    return share * DS_FGS * CHUNK <= DS_GCAP / 1.4;
}

size_t ds_workspace(const flc_codec_params* prm, int64_t n, int64_t d, int norm_mode) {
    (void)prm;
    size_t b = 0;
    carve_ds(nullptr, n, d, &b, norm_mode == FLC_NORMMODE_TORCH_CPU);
    return b;
}

// Per-device side stream and events of the row-group pipeline (lazily created, mutex-guarded;
// enqueueing under the mutex keeps concurrent callers' event records and waits paired).
namespace {
struct DsCtx {
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ev;
};
std::mutex g_ds_mu;
std::map<int, DsCtx> g_ds_ctx;
}  // namespace

// Row groups of the pipeline: the caller's hint (FLC_ROW_GROUPS(g) in flags), else 2 for 128 rows
// or more.  Group g's norm, resolve and fold run on the side stream under group g + 1's filter,
// whose blocks reserve FLC_DS_LDSPAD bytes more LDS (5 instead of 6 per CU) so that the tail
// kernels find room beside them: C4 9.684 -> 9.554 ms per step, same allocation, two processes
// (round 4, profiles/r04); 3 groups ran 9.89 (one more filter launch boundary), and without the
// pad 2 groups ran 9.650 (round 3's version, the norm and resolve between the filters and no pad,
// was not faster than 1 group).
static int ds_groups(const flc_codec_params* prm, int64_t n) {
    const int g = (prm->flags >> 8) & 0xFF;
    return (int)std::max<int64_t>(1, std::min<int64_t>(g ? g : (n >= 128 ? 2 : 1), n));
}

// The pipeline in two parts, as topk_lists_build / topk_lists_fold split the TopK one: the lists
// (sample, filter, norm, resolve) and the fold (k_ds_accum).  The row-group pipeline interleaves the
// two — group g's fold runs under group g + 1's filter — so they are one function with the fold
// switched: fold == false issues every launch but k_ds_accum's and still joins the side stream back
// into `st`, after which the lists, norms and flags in the workspace are final.  ds_run is
// <RowSrc, fold>: its launches are what they were.  SRC = DiffSrc: device draws, the exact norm.
template <class SRC>
static int ds_run_t(const flc_codec_params* prm, const flc_pattern* pat, SRC rows, int64_t n, int64_t d, const float* w,
                    float wt, float* pnorm_out, float* out, void* wsp, size_t ws_bytes, hipStream_t st, const float* pnorm_in,
                    int norm_mode, bool fold) {
    constexpr bool DIFF = std::is_same<SRC, DiffSrc>::value;
    const DsVariant& v = ds_variant();
    // the rows' norms: the filter's partials (exact), the caller's, or torch's CPU order (tn)
    const bool tn = norm_mode == FLC_NORMMODE_TORCH_CPU && !pnorm_in;
    const bool tns = tn && v.tnsums;                        // the filter emits the torch lanes' sums
    size_t need = 0;
    carve_ds(nullptr, n, d, &need, tn);
    if (ws_bytes < need) { set_error("dithering (sparse): workspace %zu < %zu", ws_bytes, need); return FLC_ERR_WORKSPACE; }
    void* tnws = nullptr;
    DsWs ws = carve_ds(wsp, n, d, nullptr, tn, &tnws);
    const int64_t client0 = pat ? pat->client0 : 0;
    const int64_t H = nhalves(d);
    const int K = ds_groups(prm, n);
    // compat: the caller's float64 uniforms (the reference's numpy stream) instead of device draws
    const bool compat = pat && pat->d_uniforms;
    const UniformSrc us{compat ? pat->d_uniforms : nullptr, (pat && pat->uniforms_ld) ? pat->uniforms_ld : d};

    hipEvent_t filt_ev = nullptr;
    auto filter = [&](int64_t r0, int64_t rn, hipStream_t s2 = nullptr, bool beside = false) -> int {
        // s2: the row group's norm / resolve go to this stream (after an event on st), under the
        // next group's filter
        const auto kern = ds_filter_kernel<SRC>(v, compat, tns);
        int gw = (int)std::max<int64_t>(1, std::min<int64_t>((rn * ws.G + 3) / 4, 32768));
        // row groups (s2: the group's tail runs beside the next group's filter): the filter's
        // blocks reserve FLC_DS_LDSPAD more bytes of LDS, so one block fewer fits a CU and the
        // side stream's tail kernels find room without waiting for a filter block to retire
        const size_t pad = s2 ? (size_t)FLC_DS_LDSPAD : 0u;
        if (FLC_DS_RESGRID || v.resident || (K > 1 && v.gridpct < 100)) {
            // resident grid: exactly the blocks that fit the chip at once (the LDS pad counted),
            // each walking its items grid-stride, so no block retires before the end — no partial
            // last round of blocks, and the side stream's kernels get only the room left beside
            // the filter instead of every slot a retiring filter block frees
            int per = 0, dev = 0, cus = 0;
            if (hipGetDevice(&dev) == hipSuccess &&
                hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
                hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, 256, pad) == hipSuccess && per > 0)
                gw = std::min(gw, std::max(1, per * cus * (K > 1 ? v.gridpct : 100) / 100));
        }
        { ProfScope _ps("k_ds_filter", st);
        hipLaunchKernelGGL(kern, dim3(gw), dim3(256), pad, st, rows, n, r0, rn, std::min<int64_t>(v.rb, rn), d, ws, us); }
        FLC_CHECK_LAUNCH("k_ds_filter");
        hipStream_t sr = st;
        if (s2) {
            FLC_CHECK_HIP(hipEventRecord(filt_ev, st));
            FLC_CHECK_HIP(hipStreamWaitEvent(s2, filt_ev, 0));
            sr = s2;
        }
        if (tn) {
            // the group's norms in torch's order (k_tn_maps: the one extra read of its rows; with
            // k_tn_sums, the three-read composition, two), where the exact mode's k_ds_final
            // runs: under the next group's filter when there is one
            if constexpr (!DIFF)
                if (int rc = tn_run(rows, n, r0, rn, d, ws.pn, tnws, tns ? ws.tsum : nullptr, ws.G, sr)) return rc;
        }
        { ProfScope _ps("k_ds_final", sr);
        if (tn || pnorm_in)
            hipLaunchKernelGGL(k_ds_final<true>, dim3((unsigned)((rn + 3) / 4)), dim3(256), 0, sr, r0, rn, ws, w, pnorm_out,
                               tn ? ws.pn : pnorm_in);
        else
            hipLaunchKernelGGL(k_ds_final<false>, dim3((unsigned)((rn + 3) / 4)), dim3(256), 0, sr, r0, rn, ws, w, pnorm_out,
                               (const float*)nullptr); }
        FLC_CHECK_LAUNCH("k_ds_final");
        int rb = (int)std::max<int64_t>(1, std::min<int64_t>(((rn + 63) / 64 * ws.G + 3) / 4, 8192));
        // beside the next group's filter: a bounded grid (grid-stride), so the side kernel holds a
        // fixed share of the CUs instead of taking every slot a retiring filter block frees
        if (beside && FLC_DS_SIDE_RES_WG > 0) rb = std::min(rb, FLC_DS_SIDE_RES_WG);
        if (!(beside && (FLC_DS_PROBE_SIDE & 1)))             // probe builds only (outputs NOT valid)
        { ProfScope _ps("k_ds_resolve", sr);
        hipLaunchKernelGGL(compat ? k_ds_resolve<true> : k_ds_resolve<false>, dim3(rb), dim3(256), 0, sr, n, r0, rn, ws,
                           prm->d_levels, prm->s, us); }
        FLC_CHECK_LAUNCH("k_ds_resolve");
        return FLC_OK;
    };
    auto accum = [&](int64_t r0, int64_t rn, int first, int last, hipStream_t s2, bool beside = false) -> int {
        int ab = (int)std::max<int64_t>(1, std::min<int64_t>((H + DS_AW - 1) / DS_AW, 32768));
        if (!fold) return FLC_OK;                            // the lists only: the caller folds (or does not)
        if (beside && FLC_DS_SIDE_FOLD_WG > 0) ab = std::min(ab, FLC_DS_SIDE_FOLD_WG);
        ProfScope _ps("k_ds_accum", s2);
        auto kern = [&] {
            if constexpr (DIFF) {
                return w ? k_ds_accum<true, DS_AP, false, DiffSrc> : k_ds_accum<false, DS_AP, false, DiffSrc>;
            } else {
                return w ? (compat ? k_ds_accum<true, DS_AP, true> : k_ds_accum<true, DS_AP, false>)
                         : (compat ? k_ds_accum<false, DS_AP, true> : k_ds_accum<false, DS_AP, false>);
            }
        }();
        hipLaunchKernelGGL(kern, dim3(ab), dim3(64 * DS_AW), 0, s2, rows, n, r0, rn, first, last, d, ws, prm->d_levels, prm->s, w,
                           wt, ws.part, out, us);
        FLC_CHECK_LAUNCH("k_ds_accum");
        return FLC_OK;
    };

    auto sample = [&](int64_t a, int64_t b, hipStream_t sx) -> int {
        if (b <= a) return FLC_OK;
        ProfScope _ps("k_ds_sample", sx);
        hipLaunchKernelGGL(k_ds_sample<SRC>, dim3((unsigned)(b - a)), dim3(DS_SNT), 0, sx, rows, n, d, prm->d_levels, prm->s, prm->seed,
                           client0, ws, a, (tn || pnorm_in) ? 1 : 0);
        FLC_CHECK_LAUNCH("k_ds_sample");
        return FLC_OK;
    };
    // row groups (K >= 2): only group 0's sample before its filter; the other rows' samples run on
    // the side stream beside it and group 1's filter waits for them
    const bool split = FLC_DS_SPLIT_SAMPLE && K >= 2;
    if (!split)
        if (int rc = sample(0, n, st)) return rc;
    if (K == 1) {
        int rc = filter(0, n);
        if (rc) return rc;
        return accum(0, n, 1, 1, st);
    }
    // Row-group pipeline: the fold of group g (side stream, latency-bound) runs under the filter
    // of group g + 1 (caller stream, HBM-bound); the groups' folds continue one another's tiles
    // through `part`, in row order.
    int dev = 0;
    FLC_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_ds_mu);
    DsCtx& cx = g_ds_ctx[dev];
    if (!cx.side) {
        // the fold is latency-bound and short: it gets the dispatcher's priority over the filter
        int lo = 0, hi = 0;
        FLC_CHECK_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        FLC_CHECK_HIP(hipStreamCreateWithPriority(&cx.side, hipStreamNonBlocking, hi));
    }
    // events: [0, K) a group's filter, K the join, K + 2 and K + 3 the split sample
    // (a stream's events are reused in order: a record after the wait that consumed it)
    while ((int)cx.ev.size() < K + 4) {
        hipEvent_t e;
        FLC_CHECK_HIP(hipEventCreateWithFlags(&e, FLC_SYNC_EVENT_FLAGS));
        cx.ev.push_back(e);
    }
    const int EV_S0 = K + 2, EV_S1 = EV_S0 + 1;
    if (split) {
        const int64_t rs1 = group_row(n, K, 1, FLC_DS_LASTPCT);
        FLC_CHECK_HIP(hipEventRecord(cx.ev[EV_S0], st));                   // after the work queued before
        FLC_CHECK_HIP(hipStreamWaitEvent(cx.side, cx.ev[EV_S0], 0));
        if (int rc = sample(0, rs1, st)) return rc;
        if (int rc = sample(rs1, n, cx.side)) return rc;
        FLC_CHECK_HIP(hipEventRecord(cx.ev[EV_S1], cx.side));
    }
    for (int g = 0; g < K; ++g) {
        const int64_t r0 = group_row(n, K, g, FLC_DS_LASTPCT), r1 = group_row(n, K, g + 1, FLC_DS_LASTPCT);
        if (split && g == 1) FLC_CHECK_HIP(hipStreamWaitEvent(st, cx.ev[EV_S1], 0));
        // the group's whole tail (norm, resolve, fold) on the side stream, under the next
        // group's filter
        filt_ev = cx.ev[g];
        int rc = filter(r0, r1 - r0, cx.side, g < K - 1);
        if (rc) return rc;
        if (!(g < K - 1 && (FLC_DS_PROBE_SIDE & 2)))         // probe builds only (outputs NOT valid)
            rc = accum(r0, r1 - r0, g == 0, g == K - 1, cx.side, g < K - 1);
        if (rc) return rc;
    }
    FLC_CHECK_HIP(hipEventRecord(cx.ev[K], cx.side));
    FLC_CHECK_HIP(hipStreamWaitEvent(st, cx.ev[K], 0));
    return FLC_OK;
}

int ds_run(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, int64_t n, int64_t d, const float* w,
           float wt, float* pnorm_out, float* out, void* wsp, size_t ws_bytes, hipStream_t st, const float* pnorm_in,
           int norm_mode) {
    return ds_run_t<RowSrc>(prm, pat, rows, n, d, w, wt, pnorm_out, out, wsp, ws_bytes, st, pnorm_in, norm_mode, /*fold=*/true);
}

// ------------------------------------------------------------------------------------------
// The one-read shifted round's epilogues (flc_dither_shift_reduce, dither_shift.hip; DESIGN.md
// §8.04): after the lists of the differences v_i = a_i - b_i are final, the in-place operand is
// updated at the elements whose encoded value e is nonzero, and nowhere else:
//     shape A (DIANA)  b_i[j] = b_i[j] + alpha * e        shape B (EF21)  b_i[j] = b_i[j] + e * msg_scale
// each operation rounded separately, e exactly the value k_ds_accum folds.
// ------------------------------------------------------------------------------------------
struct DsShift {
    const float* a; int64_t lda;
    float* b;       int64_t ldb;      // the in-place operand: h_i (A) or g_prev_i (B)
    float ms;                         // msg_scale
    float alpha;                      // shift_alpha
};

__device__ inline float ds_shift_upd(int mode, float bv, float e, const DsShift& g) {
    return mode == SHAPE_A ? bv + g.alpha * e : bv + e * g.ms;
}

// Sparse rows.  One wave per (half chunk h, 64-row batch): per row its list ent16[h][row][0 .. sure +
// resolved), U rows' entry windows, then their gathers of b, then their stores in flight together.
// Rows flagged dense have count 0 here (ds_meta) and are k_ds_shift_dense_rows'.  A row's entries
// name distinct columns and every (h, row) list belongs to one wave, so the thread that gathered an
// element stores it; a column at or past d is never stored to.
template <int MODE>
__global__ __launch_bounds__(256) void k_ds_shift_lists(DsShift g, int64_t n, int64_t d, DsWs ws,
                                                        const float* __restrict__ levels, int s) {
    constexpr int U = 8;
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    __shared__ float lvl[DS_MAXLEV + 1];
    if (threadIdx.x <= (unsigned)DS_MAXLEV) lvl[threadIdx.x] = (int)threadIdx.x <= s ? levels[threadIdx.x] : 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t H = nhalves(d), nb = (n + 63) / 64;
    auto value = [&](uint32_t e, float pn) {                // k_ds_accum's: copysign(levels[lev], sign) * pnorm
        const float lv = lvl[(e >> 12) & 15u];
        return __uint_as_float(__float_as_uint(lv) | ((e & 0x800u) << 20)) * pn;
    };
    for (int64_t t = (int64_t)blockIdx.x * 4 + wv; t < H * nb; t += (int64_t)gridDim.x * 4) {
        const int64_t h = t / nb, r0 = (t - h * nb) * 64;
        const int64_t hbase = h * HCHUNK;
        const DsMeta m = ds_meta(ws, h, n, n, r0 + lane, nullptr);   // cnt: 0 for dense rows and past n
        const uint64_t any = __ballot(m.cnt != 0u);
        if (any == 0ull) continue;
#pragma unroll 1
        for (int q0 = 0; q0 < 64; q0 += U) {
            if (((any >> q0) & ((1ull << U) - 1ull)) == 0ull) continue;
            uint32_t en[U];
            float bv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t cnt = __builtin_amdgcn_readlane(m.cnt, q0 + u);
                const int64_t row = min(r0 + q0 + u, n - 1);
                en[u] = NONE;
                if ((uint32_t)lane < cnt) en[u] = ws.ent16[(h * n + row) * DS_HCAP + lane];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t row = min(r0 + q0 + u, n - 1);
                const int64_t j = hbase + (int64_t)(en[u] & (HCHUNK - 1));
                if (en[u] != NONE && j >= d) en[u] = NONE;
                bv[u] = 0.f;
                if (en[u] != NONE) bv[u] = g.b[row * g.ldb + j];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t row = min(r0 + q0 + u, n - 1);
                const float pn = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(m.pn), q0 + u));
                if (en[u] != NONE) {
                    const float e = value(en[u], pn);
                    const int64_t j = hbase + (int64_t)(en[u] & (HCHUNK - 1));
                    if (!(e == 0.f)) g.b[row * g.ldb + j] = ds_shift_upd(MODE, bv[u], e, g);
                }
            }
            // the rest of a list longer than one window (rare)
            for (int u = 0; u < U; ++u) {
                const uint32_t cnt = __builtin_amdgcn_readlane(m.cnt, q0 + u);
                if (cnt <= 64u) continue;
                const int64_t row = r0 + q0 + u;
                const float pn = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(m.pn), q0 + u));
                for (uint32_t k = 64u + (uint32_t)lane; k < cnt; k += 64u) {
                    const uint32_t ek = ws.ent16[(h * n + row) * DS_HCAP + k];
                    const int64_t j = hbase + (int64_t)(ek & (HCHUNK - 1));
                    const float e = value(ek, pn);
                    if (j < d && !(e == 0.f)) {
                        float* p = g.b + row * g.ldb + j;
                        *p = ds_shift_upd(MODE, *p, e, g);
                    }
                }
            }
        }
    }
}

// Dense rows.  The flags live on the device, so this is one launch whose workgroups leave at once
// for rows without DS_DENSE.  A flagged row is encoded element by element with its norm — ds_encode,
// k_ds_accum's dense re-encode — and the in-place element is stored where e is nonzero (NaN
// included): the same contract whichever path a row took.
template <int MODE>
__global__ __launch_bounds__(256) void k_ds_shift_dense_rows(DsShift g, int64_t n, int64_t d, DsWs ws, int s) {
    const int64_t row = blockIdx.y;
    if (row >= n) return;
    const uint32_t mode = ws.flags[row];
    if (!(mode & DS_DENSE)) return;
    DsRow rr;
    rr.n = ws.pn[row];
    rr.rn = ws.rpn[row];
    const uint32_t rk = ws.rk[row];
    rr.rk2 = rk ^ 0x27D4EB2Fu;
    rr.fast = (mode & DS_FAST) != 0u;
    const float4* tab = ws.gtab;
    const float sf = (float)s;
    const float* ap = g.a + row * g.lda;
    float* bp = g.b + row * g.ldb;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < d; j += (int64_t)gridDim.x * 256) {
        const float bv = bp[j];
        const float v = ap[j] - bv;
        const float e = ds_encode<false>(v, (uint32_t)j, ds_hi8((uint32_t)j, rk), 0.0, rr, tab, s, sf);
        if (!(e == 0.f)) bp[j] = ds_shift_upd(MODE, bv, e, g);
    }
}

const uint32_t* ds_flags_at(const void* wsp, int64_t n, int64_t d) { return carve_ds(const_cast<void*>(wsp), n, d, nullptr).flags; }

int ds_shift_run(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows& sr, int shape, int64_t n, int64_t d,
                 const float* w, float wt, float* pnorm_out, float* out, void* wsp, size_t ws_bytes, hipStream_t st) {
    const DiffSrc rows{RowSrc{sr.d_a, sr.lda, nullptr}, RowSrc{sr.d_b, sr.ldb, nullptr}};
    // A and D: the fold of the messages (k_ds_accum over a - b) completes before either epilogue writes
    // b — it re-reads a and b for dense rows and -0 columns — and ds_run_t returns with the row-group
    // pipeline joined into st.  B folds the updated rows afterwards instead.
    if (int rc = ds_run_t<DiffSrc>(prm, pat, rows, n, d, w, wt, pnorm_out, out, wsp, ws_bytes, st, nullptr, FLC_NORMMODE_EXACT,
                                   /*fold=*/shape != SHAPE_B))
        return rc;
    if (shape != SHAPE_A && shape != SHAPE_B) return FLC_OK;
    const DsWs ws = carve_ds(wsp, n, d, nullptr);
    const DsShift g{sr.d_a, sr.lda, const_cast<float*>(sr.d_b), sr.ldb, sr.msg_scale, sr.shift_alpha};
    {
        ProfScope _ps("k_ds_shift_lists", st);
        const int64_t waves = nhalves(d) * ((n + 63) / 64);
        const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, 65536)));
        if (shape == SHAPE_A) hipLaunchKernelGGL(k_ds_shift_lists<SHAPE_A>, grid, dim3(256), 0, st, g, n, d, ws, prm->d_levels, prm->s);
        else hipLaunchKernelGGL(k_ds_shift_lists<SHAPE_B>, grid, dim3(256), 0, st, g, n, d, ws, prm->d_levels, prm->s);
        FLC_CHECK_LAUNCH("k_ds_shift_lists");
    }
    {
        ProfScope _ps("k_ds_shift_dense_rows", st);
        const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((d + 2047) / 2048, 256)), (unsigned)n);
        if (shape == SHAPE_A) hipLaunchKernelGGL(k_ds_shift_dense_rows<SHAPE_A>, grid, dim3(256), 0, st, g, n, d, ws, prm->s);
        else hipLaunchKernelGGL(k_ds_shift_dense_rows<SHAPE_B>, grid, dim3(256), 0, st, g, n, d, ws, prm->s);
        FLC_CHECK_LAUNCH("k_ds_shift_dense_rows");
    }
    return shape == SHAPE_B ? fold_updated_rows(sr, n, d, w, wt, out, st) : FLC_OK;
}

}  // namespace flc
