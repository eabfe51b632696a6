// Rank-K server fold from the factor payloads (flc_unpack_reduce_factored): one fp32 MFMA GEMM over
// the messages as they lie, no dense rows.
//
// A Rank-K message body is the factor block of rank_k.hip: U'_i (B x K', column-major, ld B) at float
// 0 and (S V'^T)_i (K' x A, column-major, ld K') at float rk_uoff.  The fold of n messages
//     out (B x A column-major = the row-major A x B result)
//         = (1 / w_total) sum_i w_i U'_i (S V'^T)_i
//         = [U'_0 | U'_1 | ...] (B x nK')  [w_0 (SV)_0 ; w_1 (SV)_1 ; ...] (nK' x A) / w_total
// is ONE product with a contraction of length n K' whose operands are the bodies in place: 4 n K' (A +
// B) bytes of messages read (each tile re-reads its slabs through L2), 4 D written, 2 D n K' flops, no
// workspace.  flc_unpack_reduce's Rank-K path reconstructs n dense [D] rows with rocBLAS and folds
// them: about 8 n D + 4 D bytes and an n D-float workspace.
//
// k_rk_fold<T>: a 256-thread workgroup owns the T x T output tile (a0.., b0..), T = 128 when that grid
// fills the chip and 64 otherwise (rk_fold_large: a pure function of A and B).  Its four waves lie 2 x 2
// over the tile; a wave keeps its (T/2) x (T/2) corner as (T/64)^2 accumulators of
// v_mfma_f32_32x32x2f32 in registers for the whole contraction.  The instruction's M dimension runs
// along a and its N dimension along b, so an accumulator register of lanes 0-31 is 32 consecutive b
// of one a: a 128-byte run of `out`.
//   operand A (32 x 2): lane l holds w_i (SV)_i[k + l / 32][a + l % 32]
//   operand B (2 x 32): lane l holds U'_i[b + l % 32][k + l / 32]
//   result register v of lane l: a + 8 (v / 4) + 4 (l / 32) + v % 4,  b + l % 32
// Contraction order: a step is (row i, slab k0 = 0, KC, ... of that row's K' columns); rows in client
// order, k ascending, the same in every tile, no split over the contraction and no atomics — the
// result is the same bits from run to run and for strided rows and a pointer list.
// Staging: per step the U' slab (k, b) and the SV slab (k, a) go to LDS as [k][T + 32] floats, two
// buffers each; the next step's global loads are issued before the current step's MFMAs and written
// to the other buffer after them (one barrier per step).  U' is contiguous along b: 16-byte loads
// when B % 4 == 0 (every column start is then 16-byte aligned), a scalar path otherwise.  SV is
// contiguous along k in runs of K': thread order follows memory (k fastest), w_i is multiplied in on
// the way to LDS (no multiply without weights).  The operand reads are one float per lane at
// [k + l / 32][x + l % 32]: with the leading dimension = 32 (mod 64) the two half-waves fall on
// disjoint banks.  Rows k of a slab past K' (an odd K', the last slab) and columns past A or B are
// written as zeros; stores past A or B are predicated.
// Epilogue: acc / w_total (the fp32 division of the plain fold) straight to out; n == 0 stores zeros.
//
// Nothing is taken from the messages but their bodies: every index comes from (A, B, K') of the
// codec and d, so a kernel addresses only bytes below flc_payload_bytes of each message.  The header
// is the business of flc_payload_validate (host).
#include <algorithm>

#include "common.hpp"

namespace flc {

namespace {
constexpr int KC = 16;                       // slab depth: k columns staged per step
typedef float v16f __attribute__((ext_vector_type(16)));
template <class T>
using gptr = const __attribute__((address_space(1))) T*;

struct RkFold {
    const char* base;                        // strided messages (row i at base + i * ld) or
    int64_t ld;
    const char* const* ptrs;                 // a device array of message pointers
    int64_t n, A, B, uoff;
    int K;                                   // K' = min(K, A, B)
    const float* w;
    float wt;
    float* out;
};
}  // namespace

// the large tile when its grid gives every compute unit of the MI355X (256) a workgroup
static bool rk_fold_large(int64_t A, int64_t B) { return ((A + 127) / 128) * ((B + 127) / 128) >= 256; }

template <int T, bool W, bool VEC>
__global__ __launch_bounds__(256) void k_rk_fold(RkFold g) {
    constexpr int LD = T + 32;               // = 32 (mod 64): the half-waves' operand reads on disjoint banks
    constexpr int BM = T / 64;               // 32 x 32 blocks per wave and dimension
    constexpr int NSV = T * KC / 256;        // SV floats per thread and slab
    constexpr int NU = (VEC ? T / 4 : T) * KC / 256;   // U' float4 / floats per thread and slab
    __shared__ __attribute__((aligned(16))) float sU[2][KC * LD];
    __shared__ __attribute__((aligned(16))) float sS[2][KC * LD];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t tiles_b = (g.B + T - 1) / T;
    const int64_t a0 = (int64_t)(blockIdx.x / tiles_b) * T, b0 = (int64_t)(blockIdx.x % tiles_b) * T;
    const int K = g.K;
    const int kdp = (min(KC, K) + 1) & ~1;   // rows of a full slab, padded to the instruction's k = 2
    const int64_t steps = g.n * ((K + KC - 1) / KC);

    // SV: element e of the slab is (a = e / kdp, k = e % kdp), memory order when K' <= KC is even
    int sv[NSV];
#pragma unroll
    for (int j = 0; j < NSV; ++j) {
        const int e = t + 256 * j, a = e / kdp;
        sv[j] = e < T * kdp ? (a | (e - a * kdp) << 8) : -1;
    }
    float rs[NSV];
    float4 ru[VEC ? NU : 1];
    float ru1[VEC ? 1 : NU];
    float wn = 1.f;
    auto load = [&](int64_t i, int k0) {
        const char* p = g.base ? g.base + i * g.ld : sload(g.ptrs + i);
        gptr<float> body = (gptr<float>)(p + 16);
        gptr<float> ps = body + g.uoff + a0 * K + k0;
        if (W) wn = sload(g.w + i);
#pragma unroll
        for (int j = 0; j < NSV; ++j) {
            const int a = sv[j] & 255, k = sv[j] >> 8;
            rs[j] = (sv[j] >= 0 && a0 + a < g.A && k0 + k < K) ? ps[a * K + k] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int e = t + 256 * j;
            if (VEC) {
                const int k = e / (T / 4), b = 4 * (e % (T / 4));
                ru[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k0 + k < K && b0 + b < g.B) {      // (B % 4 == 0: the whole group is below B)
                    typedef float v4f __attribute__((ext_vector_type(4)));
                    const v4f v = *(gptr<v4f>)(body + (int64_t)(k0 + k) * g.B + b0 + b);
                    ru[j] = make_float4(v.x, v.y, v.z, v.w);
                }
            } else {
                const int k = e / T, b = e % T;
                ru1[j] = (k0 + k < K && b0 + b < g.B) ? body[(int64_t)(k0 + k) * g.B + b0 + b] : 0.f;
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < NSV; ++j)
            if (sv[j] >= 0) sS[buf][(sv[j] >> 8) * LD + (sv[j] & 255)] = W ? wn * rs[j] : rs[j];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int e = t + 256 * j;
            if (VEC) {
                const int k = e / (T / 4), b = 4 * (e % (T / 4));
                if (k < kdp) *reinterpret_cast<float4*>(&sU[buf][k * LD + b]) = ru[j];
            } else {
                const int k = e / T, b = e % T;
                if (k < kdp) sU[buf][k * LD + b] = ru1[j];
            }
        }
    };

    const int wa = (wv >> 1) * (T / 2), wb = (wv & 1) * (T / 2);
    v16f acc[BM][BM];
#pragma unroll
    for (int x = 0; x < BM; ++x)
#pragma unroll
        for (int y = 0; y < BM; ++y)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[x][y][v] = 0.f;
    const int opnd = (lane >> 5) * LD + (lane & 31);

    if (steps > 0) {
        load(0, 0);
        store(0);
    }
    __syncthreads();
    int64_t i = 0;
    int k0 = 0;
    for (int64_t s = 0; s < steps; ++s) {
        int kn = k0 + KC;
        int64_t in = i;
        if (kn >= K) { kn = 0; ++in; }
        const bool more = s + 1 < steps;
        if (more) load(in, kn);                                // in flight under this step's MFMAs
        const float* pa = sS[s & 1] + opnd + wa;
        const float* pb = sU[s & 1] + opnd + wb;
        const int kd2 = (min(KC, K - k0) + 1) & ~1;
        for (int kk = 0; kk < kd2; kk += 2) {
            float fa[BM], fb[BM];
#pragma unroll
            for (int x = 0; x < BM; ++x) {
                fa[x] = pa[kk * LD + 32 * x];
                fb[x] = pb[kk * LD + 32 * x];
            }
#pragma unroll
            for (int x = 0; x < BM; ++x)
#pragma unroll
                for (int y = 0; y < BM; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[x], fb[y], acc[x][y], 0, 0, 0);
        }
        if (more) store((s + 1) & 1);
        __syncthreads();
        i = in;
        k0 = kn;
    }

    const bool div = g.n > 0;
#pragma unroll
    for (int x = 0; x < BM; ++x)
#pragma unroll
        for (int y = 0; y < BM; ++y) {
            const int64_t b = b0 + wb + 32 * y + (lane & 31);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int64_t a = a0 + wa + 32 * x + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
                if (a < g.A && b < g.B) g.out[a * g.B + b] = div ? acc[x][y][v] / g.wt : acc[x][y][v];
            }
        }
}

template <int T>
static void rk_fold_launch(const RkFold& g, hipStream_t st) {
    const int64_t tiles = ((g.A + T - 1) / T) * ((g.B + T - 1) / T);
    const dim3 grid((unsigned)tiles), blk(256);
    const bool vec = g.B % 4 == 0;
    if (g.w) {
        if (vec) hipLaunchKernelGGL((k_rk_fold<T, true, true>), grid, blk, 0, st, g);
        else hipLaunchKernelGGL((k_rk_fold<T, true, false>), grid, blk, 0, st, g);
    } else {
        if (vec) hipLaunchKernelGGL((k_rk_fold<T, false, true>), grid, blk, 0, st, g);
        else hipLaunchKernelGGL((k_rk_fold<T, false, false>), grid, blk, 0, st, g);
    }
}

int rk_fold_run(const flc_codec_params* prm, const char* base, int64_t ld, const char* const* ptrs, int64_t n, int64_t d,
                const float* w, float wt, float* out, hipStream_t st) {
    const char* me = "flc_unpack_reduce_factored";
    if (prm->k < 1) { set_error("%s: K=%lld < 1", me, (long long)prm->k); return FLC_ERR_ARG; }
    if (d >= (int64_t)0x7FFFFFFF) { set_error("%s: D too large for a Rank-K message (32-bit sizes)", me); return FLC_ERR_ARG; }
    if (base && ((ld & 15) || ((uintptr_t)base & 15u))) { set_error("%s: payload rows must be 16-byte aligned", me); return FLC_ERR_ARG; }
    if (d == 0) return FLC_OK;
    RkFold g{base, ld, ptrs, n, 0, 0, 0, 0, w, wt, out};
    int64_t K = 0;
    rk_dims(prm, d, &g.A, &g.B, &K, &g.uoff);
    g.K = (int)K;
    ProfScope _ps("k_rk_fold", st);
    if (rk_fold_large(g.A, g.B)) rk_fold_launch<128>(g, st);
    else rk_fold_launch<64>(g, st);
    FLC_CHECK_LAUNCH("k_rk_fold");
    return FLC_OK;
}

}  // namespace flc
