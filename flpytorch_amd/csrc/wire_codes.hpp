// Wire-format constants and the per-element codes (wire.hip's layout; include/flcodec.h), shared by
// the pack / decode kernels of wire.hip and the fused encode -> code kernel of codecs.hip.
#pragma once
#include <type_traits>
#include <utility>

#include "common.hpp"

namespace flc {

enum { FMT_F32 = 1, FMT_Q8 = 2, FMT_Q16 = 3, FMT_NAT16 = 4, FMT_SPARSE = 5, FMT_RANKK = 6,
       FMT_LBITS = 7, FMT_NAT9 = 8,        // the bit-packed forms (wire_bits.hip)
       FMT_SEEDED = 9,                     // RandK values only, the set redrawn from the key (wire_seeded.hip)
       FMT_SLEV = 10 };                    // the nonzero Q8 codes as per-chunk lists (wire_slev.hip)
struct PayloadHeader {
    uint32_t fmt, count;
    float norm;
    uint32_t bad;          // elements whose code search failed (0 by construction)
};

__host__ __device__ inline int64_t a16(int64_t b) { return (b + 15) & ~int64_t(15); }

// ---- level codes ------------------------------------------------------------------------------
__device__ inline float lev_value(const float* lv, uint32_t idx, bool neg, float norm) {
    return copysignf(lv[idx], neg ? -1.f : 1.f) * norm;
}

__device__ inline uint32_t lev_code(float v, const float* lv, int s, float norm, uint32_t sbit, uint32_t* bad) {
    const uint32_t vb = __float_as_uint(v);
    if (vb == 0u) return 0u;                                   // +0 (x == 0)
    const bool neg = (vb >> 31) != 0u;
    if (v != v) return sbit;                                   // NaN: -0 * non-finite norm
    // the guess only has to land within one level: a product by 1 / norm, checked exactly below
    const float y = fabsf(v) * __builtin_amdgcn_rcpf(norm);
    int g = (int)rintf(y * (float)s);
    g = g < 0 ? 0 : (g > s ? s : g);
    for (int dlt = 0; dlt < 3; ++dlt) {
        const int c = dlt == 0 ? g : (dlt == 1 ? g - 1 : g + 1);
        if (c >= 0 && c <= s && __float_as_uint(lev_value(lv, (uint32_t)c, neg, norm)) == vb)
            return (neg ? sbit : 0u) | (uint32_t)c;
    }
    int lo = 0, hi = s;                                        // levels ascending: binary search on |v|
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const float m = fabsf(lev_value(lv, (uint32_t)mid, neg, norm));
        if (__float_as_uint(lev_value(lv, (uint32_t)mid, neg, norm)) == vb) return (neg ? sbit : 0u) | (uint32_t)mid;
        if (m < fabsf(v)) lo = mid + 1; else hi = mid - 1;
    }
    atomicAdd(bad, 1u);
    return neg ? sbit : 0u;
}

// a level index past s (only a malformed message has one) reads the top level, never past the table
__device__ inline float lev_decode(uint32_t code, const float* lv, int s, float norm, uint32_t sbit) {
    if (code == 0u) return 0.f;
    return lev_value(lv, min(code & (sbit - 1u), (uint32_t)s), (code & sbit) != 0u, norm);
}

// ---- natural codes ----------------------------------------------------------------------------
__device__ inline uint32_t nat_code(float v) {
    const uint32_t vb = __float_as_uint(v), sg = (vb >> 31) << 15;
    if ((vb & 0x7FFFFFFFu) == 0u) return sg;
    if (v != v) return 0x7FFFu;
    if (isinf(v)) return sg | 0x7FFEu;
    int e;
    (void)frexpf(v, &e);                                       // |v| = 0.5 * 2^e (a power of two)
    return sg | (uint32_t)(e - 1 + 16384);
}

__device__ inline float nat_decode(uint32_t c) {
    const float sg = (c & 0x8000u) ? -1.f : 1.f;
    const uint32_t m = c & 0x7FFFu;
    if (m == 0u) return copysignf(0.f, sg);
    if (m == 0x7FFFu) return __uint_as_float(0x7FC00000u);
    if (m == 0x7FFEu) return copysignf(__builtin_inff(), sg);
    return copysignf(ldexpf(1.f, (int)m - 16384), sg);
}

// ---- one 16-B body slice of a dense format (the tile owners of wire.hip and wire_shift.hip) ----
template <int FMT>
struct WireFmt {
    static constexpr int E = FMT == FMT_Q8 ? 16 : (FMT == FMT_F32 ? 4 : 8);
    static constexpr int BYTES = 16 / E;
};

template <int FMT>
__device__ inline float dec1(uint32_t c, const float* lv, int s, float norm) {
    if (FMT == FMT_Q8) return lev_decode(c, lv, s, norm, 0x80u);
    if (FMT == FMT_Q16) return lev_decode(c, lv, s, norm, 0x8000u);
    if (FMT == FMT_NAT16) return nat_decode(c);
    return __uint_as_float(c);
}

template <int FMT>
__device__ inline void dec16(uint4 v, const float* lv, int s, float norm, float* e) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    constexpr int E = WireFmt<FMT>::E;
#pragma unroll
    for (int q = 0; q < E; ++q) {
        uint32_t c;
        if (FMT == FMT_Q8) c = (w[q >> 2] >> (8 * (q & 3))) & 0xFFu;
        else if (FMT == FMT_F32) c = w[q];
        else c = (w[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
        e[q] = dec1<FMT>(c, lv, s, norm);
    }
}

// ---- bit-packed tiles (wire_bits.hip; FMT_LBITS / FMT_NAT9) ------------------------------------
// A tile is 2048 consecutive elements; lane l of the owning wave holds the 32 codes of elements
// 256 t + 4 l + q (code number i = 4 t + q), concatenated LSB-first into B words: code i at bits
// [i B, (i + 1) B).  Word k of lane l is the tile's word k * 64 + l.  Every index below is a
// constant after instantiation, so the words stay in registers.
constexpr int BT_TILE = 2048;

// codes 4 T .. 4 T + 3 of a lane (grp: 4 B bits, code q at bit q B) into its words
template <int B, int T>
__device__ inline void bt_put(uint32_t (&w)[B], uint64_t grp) {
    constexpr int P = 4 * B * T, k = P >> 5, sh = P & 31;
    static_assert(sh + 4 * B <= 64, "a group spans at most two words");
    w[k] |= (uint32_t)(grp << sh);
    if constexpr (sh + 4 * B > 32) w[k + 1] |= (uint32_t)(grp >> (32 - sh));
}

template <int B, int I>
__device__ inline uint32_t bt_get(const uint32_t (&w)[B]) {
    constexpr int P = B * I, k = P >> 5, sh = P & 31;
    uint32_t c = w[k] >> sh;
    if constexpr (sh + B > 32) c |= w[k + 1] << (32 - sh);
    return c & ((1u << B) - 1u);
}

template <class F, int... I>
__device__ inline void bt_each(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}

// A code's value.  NAT9: the code is the value's top nine bits.  Level codes: `lv` is
// |levels[min(lane, s)]|, so an element's magnitude is lane idx's register (one cross-lane read, no
// LDS table, no barrier) and an index past s reads the top level; then the sign and the norm exactly
// as lev_decode: (levels[idx] * sign) * norm, code 0 the exact +0.  Every lane of the wave must be
// active.
template <int B>
__device__ inline float bt_value(uint32_t c, float lv, float norm) {
    if constexpr (B == 9) {
        return __uint_as_float(c << 23);
    } else {
        const uint32_t idx = c & ((1u << (B - 1)) - 1u);
        const uint32_t mag = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(idx << 2), (int)__float_as_uint(lv));
        const float v = __uint_as_float(mag | ((c >> (B - 1)) << 31)) * norm;
        return c == 0u ? 0.f : v;
    }
}

// A lane's 32 values from its B words.
template <int B>
__device__ inline void bt_decode(const uint32_t (&w)[B], float lv, float norm, float* e) {
    bt_each([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        e[I] = bt_value<B>(bt_get<B, I>(w), lv, norm);
    }, std::make_integer_sequence<int, 32>{});
}

// Half a lane's tile: codes 16 H .. 16 H + 15 (steps t = 4 H .. 4 H + 3) lie in words K0 .. K0 + NW - 1
// of the lane (for odd B the middle word belongs to both halves).
template <int B, int H>
struct BtHalf {
    static constexpr int K0 = (16 * B * H) >> 5, NW = ((16 * B * (H + 1) + 31) >> 5) - K0;
};

template <int B, int H>
__device__ inline void bt_decode_half(const uint32_t (&w)[BtHalf<B, H>::NW], float lv, float norm, float* e) {
    bt_each([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        constexpr int P = B * (16 * H + I), k = (P >> 5) - BtHalf<B, H>::K0, sh = P & 31;
        uint32_t c = w[k] >> sh;
        if constexpr (sh + B > 32) c |= w[k + 1] << (32 - sh);
        e[I] = bt_value<B>(c & ((1u << B) - 1u), lv, norm);
    }, std::make_integer_sequence<int, 16>{});
}

// a lane's 32 values of a tile to the dense row: eight float4, or the elements below d
__device__ inline void bt_store(float* __restrict__ out, int64_t j0, int64_t d, const float* e) {
    const bool al = ((uintptr_t)out & 15u) == 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int64_t j = j0 + 256 * t;
        if (al && j + 3 < d) {
            *reinterpret_cast<float4*>(out + j) = make_float4(e[4 * t], e[4 * t + 1], e[4 * t + 2], e[4 * t + 3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (j + q < d) out[j + q] = e[4 * t + q];
        }
    }
}

// the base operand of the shifted-wire folds (wire_shift.hip, wire_shift_bits.hip): none, a row per
// payload, or ONE [d] vector for every row (ldbase == 0)
enum { UB_NONE = 0, UB_ROWS = 1, UB_SHARED = 2 };

}  // namespace flc
