// Sub-byte wire formats (flc_pack_bits / flc_unpack_bits / flc_unpack_reduce_bits): the dense level
// and natural messages at the bits the reference counts (last_need_to_send_advance,
// compressors.py:268, 367-368) instead of a byte or two per element.
//
//   LBITS (7 | b << 8)  standard dithering / QSGD / TernGrad with s <= 63: b = 1 + bit_length(s) bits,
//                       sign << (b - 1) | level index — Q8's code with the sign bit moved
//   NAT9  (8)           natural: the top nine bits of the fp32 value +-2^k (decode: code << 23)
//
// Header as wire.hip's (16 B: format word, count = d, norm, bad).  Body: tiles of 2048 elements, the
// last one padded with code 0, 256 b bytes each.  Inside a tile (wire_codes.hpp, bt_put / bt_get):
// element e = 256 t + 4 l + q is lane l's code i = 4 t + q; a lane's 32 codes are concatenated
// LSB-first into b words and word k of lane l is the tile's word k * 64 + l.  So a wave moves a
// tile with b fully coalesced 256-B word accesses, a lane's fp32 side is eight aligned float4, no
// code straddles lanes and every shift is a compile-time constant.
//
// Contract (tests/test_gpu_wire_bits.py): the payload is this layout applied to the codes flc_pack
// gives for the same row, parameters and pattern; flc_unpack_bits(flc_pack_bits(x)) ==
// flc_unpack(flc_pack(x)); flc_unpack_reduce_bits == flc_unpack_reduce of the byte payloads.
// No byte-format payload is ever written on the way: the pack kernel forms the dense value as
// k_ew_code does and packs it in registers.
#include <cstring>

#include "wire_bits.hpp"

namespace flc {

int bits_width(const flc_codec_params* prm) {
    if (prm->codec == FLC_NATURAL) return 9;
    if (prm->codec != FLC_STD_DITHERING || prm->s < 1 || prm->s > 63) return 0;
    int b = 1;                                    // the sign, then bit_length(s) bits of level index
    for (int v = prm->s; v; v >>= 1) ++b;
    return b;
}

int bits_format(const flc_codec_params* prm) {
    const int b = bits_width(prm);
    return b == 0 ? 0 : (b == 9 ? FMT_NAT9 : (FMT_LBITS | (b << 8)));
}

static int64_t bits_tiles(int64_t d) { return (d + BT_TILE - 1) / BT_TILE; }

int64_t bits_payload_bytes(const flc_codec_params* prm, int64_t d) {
    const int b = bits_width(prm);
    return b == 0 ? 0 : 16 + 256 * (int64_t)b * bits_tiles(d);
}

// ---- pack ----------------------------------------------------------------------------------------
// the whole header, before the code pass counts into `bad` (and the message of d == 0)
__global__ void k_bits_header(char* payload, uint32_t fmt, uint32_t count) {
    if (threadIdx.x == 0) {
        PayloadHeader* h = reinterpret_cast<PayloadHeader*>(payload);
        h->fmt = fmt;
        h->count = count;
        h->norm = 0.f;
        h->bad = 0u;
    }
}

// A wave owns whole tiles.  Per tile a lane walks its eight float4 of x (the next one loaded while
// the current one is encoded), forms each dense value and its code as k_ew_code does — the same
// functor, draws, lev_code and `bad` counter; apply4 on whole aligned groups, the element path on a
// misaligned row and on the group that crosses d — and ORs the four codes of step t into its B word
// registers at constant positions; then B coalesced dword stores.  Nothing at or past d is read;
// those elements are code 0.
template <class Op, int B, bool VEC>
__global__ __launch_bounds__(256) void k_ew_code_bits(const float* __restrict__ x, int64_t d, Op op,
                                                      const float* __restrict__ levels, int s, CodeArgs ca) {
    extern __shared__ __attribute__((aligned(16))) float4 smem_tab[];
    if (Op::TABLE) op.set_table_ok(load_table(levels, s, smem_tab));
    op.setup(0);
    PayloadHeader* h = reinterpret_cast<PayloadHeader*>(ca.payload);
    uint32_t* body = reinterpret_cast<uint32_t*>(ca.payload + 16);
    const float norm = ca.pn ? *ca.pn : 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        h->fmt = B == 9 ? (uint32_t)FMT_NAT9 : (uint32_t)(FMT_LBITS | (B << 8));
        h->count = (uint32_t)d;
        h->norm = norm;
    }
    auto code = [&](float v) -> uint32_t {
        if constexpr (B == 9) {
            const uint32_t vb = __float_as_uint(v);
            if (vb & 0x7FFFFFu) atomicAdd(&h->bad, 1u);     // a subnormal 2^k or a NaN: nine bits cannot carry it
            return vb >> 23;
        } else {
            return lev_code(v, ca.lv, ca.s, norm, 1u << (B - 1), &h->bad);
        }
    };
    auto ld4 = [&](int64_t j) -> float4 {
        if (VEC && j + 3 < d) return *reinterpret_cast<const float4*>(x + j);
        return make_float4(j < d ? x[j] : 0.f, j + 1 < d ? x[j + 1] : 0.f, j + 2 < d ? x[j + 2] : 0.f,
                           j + 3 < d ? x[j + 3] : 0.f);
    };
    const int lane = threadIdx.x & 63;
    const int64_t tiles = (d + BT_TILE - 1) / BT_TILE;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t j0 = tile * BT_TILE + 4 * lane;
        uint32_t w[B];
#pragma unroll
        for (int k = 0; k < B; ++k) w[k] = 0u;
        float4 nxt = ld4(j0);
#pragma unroll 1
        for (int t = 0; t < 8; ++t) {
            const int64_t j = j0 + 256 * t;
            const float4 v = nxt;
            if (t < 7) nxt = ld4(j + 256);
            uint32_t c[4] = {0u, 0u, 0u, 0u};
            if (VEC && j + 3 < d) {
                uint32_t cs[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) cs[q] = op.col(j + q);
                const float4 e = op.row_fast() ? apply4<true>(op, v, j, cs, smem_tab) : apply4<false>(op, v, j, cs, smem_tab);
                c[0] = code(e.x); c[1] = code(e.y); c[2] = code(e.z); c[3] = code(e.w);
            } else {
                const float xe[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (j + q < d) c[q] = code(op.template apply<false>(xe[q], j + q, op.col(j + q), smem_tab));
            }
            const uint64_t grp = (uint64_t)c[0] | ((uint64_t)c[1] << B) | ((uint64_t)c[2] << (2 * B)) | ((uint64_t)c[3] << (3 * B));
            switch (t) {                                     // wave-uniform: the word indices stay constants
                case 0: bt_put<B, 0>(w, grp); break;
                case 1: bt_put<B, 1>(w, grp); break;
                case 2: bt_put<B, 2>(w, grp); break;
                case 3: bt_put<B, 3>(w, grp); break;
                case 4: bt_put<B, 4>(w, grp); break;
                case 5: bt_put<B, 5>(w, grp); break;
                case 6: bt_put<B, 6>(w, grp); break;
                default: bt_put<B, 7>(w, grp); break;
            }
        }
        uint32_t* tw = body + tile * (64 * B) + lane;
#pragma unroll
        for (int k = 0; k < B; ++k) tw[k * 64] = w[k];
    }
}

template <class Op, int B>
static int launch_code_b(const float* x, int64_t d, Op op, const float* levels, int s, const CodeArgs& ca, hipStream_t st) {
    const bool vec = ((uintptr_t)x & 15u) == 0;
    const size_t lds = Op::TABLE ? (size_t)s * sizeof(float4) : 0;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((bits_tiles(d) + 3) / 4, 4096));
    ProfScope _ps("k_ew_code_bits", st);
    if (vec) hipLaunchKernelGGL((k_ew_code_bits<Op, B, true>), dim3(grid), dim3(256), lds, st, x, d, op, levels, s, ca);
    else hipLaunchKernelGGL((k_ew_code_bits<Op, B, false>), dim3(grid), dim3(256), lds, st, x, d, op, levels, s, ca);
    FLC_CHECK_LAUNCH("k_ew_code_bits");
    return FLC_OK;
}

template <class Op>
int launch_code_bits(const float* x, int64_t d, Op op, const float* levels, int s, const CodeArgs& ca, hipStream_t st) {
    if (d == 0) return FLC_OK;
    if constexpr (Op::TABLE) {
        switch (ca.bits) {
            case 2: return launch_code_b<Op, 2>(x, d, op, levels, s, ca, st);
            case 3: return launch_code_b<Op, 3>(x, d, op, levels, s, ca, st);
            case 4: return launch_code_b<Op, 4>(x, d, op, levels, s, ca, st);
            case 5: return launch_code_b<Op, 5>(x, d, op, levels, s, ca, st);
            case 6: return launch_code_b<Op, 6>(x, d, op, levels, s, ca, st);
            case 7: return launch_code_b<Op, 7>(x, d, op, levels, s, ca, st);
            default: break;
        }
    } else if (ca.bits == 9) {
        return launch_code_b<Op, 9>(x, d, op, levels, s, ca, st);
    }
    set_error("flc_pack_bits: no %d-bit form of this codec", ca.bits);
    return FLC_ERR_UNSUPPORTED;
}
template int launch_code_bits(const float*, int64_t, DitherOp<false, true>, const float*, int, const CodeArgs&, hipStream_t);
template int launch_code_bits(const float*, int64_t, DitherOp<false, false>, const float*, int, const CodeArgs&, hipStream_t);
template int launch_code_bits(const float*, int64_t, NaturalOp<true>, const float*, int, const CodeArgs&, hipStream_t);
template int launch_code_bits(const float*, int64_t, NaturalOp<false>, const float*, int, const CodeArgs&, hipStream_t);

// ---- decode ----------------------------------------------------------------------------------------
// One payload to a dense row: a wave per tile (the fold's ownership, no accumulation).  The format,
// b and s come from the codec, never from the message (flc_payload_validate_bits reports a header
// that lies), and the body is read within the bytes flc_payload_bits_bytes sized.
template <int B>
__global__ __launch_bounds__(256) void k_unpack_bits(const char* __restrict__ payload, int64_t d,
                                                     const float* __restrict__ levels, int s, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= (d + BT_TILE - 1) / BT_TILE) return;           // a whole wave leaves: the others stay complete
    const float lv = B == 9 ? 0.f : fabsf(levels[min(lane, s)]);
    const float norm = reinterpret_cast<const PayloadHeader*>(payload)->norm;
    const uint32_t* tw = reinterpret_cast<const uint32_t*>(payload + 16) + tile * (64 * B) + lane;
    uint32_t w[B];
#pragma unroll
    for (int k = 0; k < B; ++k) w[k] = tw[k * 64];
    float e[32];
    bt_decode<B>(w, lv, norm, e);
    bt_store(out, tile * BT_TILE + 4 * lane, d, e);
}

// Server fold, tile owner: a wave owns one tile for the whole fold, rows in order, so the fp32 sum
// is k_unpack_accum's sequential one (acc = t_0; acc = acc + t_i; out = acc / wt, t_i = w_i * dec_i).
// PF rows' B words per lane are in flight in a register ring; 32 accumulators per lane.  The level
// table is one register per lane for the whole kernel (bt_decode), so a row costs its B word loads,
// the scalar loads of its pointer, norm and weight, and no barrier.
template <int B, bool W, int PF>
__global__ __launch_bounds__(256) void k_unpack_bits_accum(const char* __restrict__ base, int64_t ld,
                                                           const char* const* __restrict__ ptrs, int64_t n, int64_t d,
                                                           const float* __restrict__ levels, int s,
                                                           const float* __restrict__ w, float wt, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= (d + BT_TILE - 1) / BT_TILE) return;
    const float lv = B == 9 ? 0.f : fabsf(levels[min(lane, s)]);
    auto row = [&](int64_t i) -> const char* { return base ? base + i * ld : sload(ptrs + i); };
    const int64_t off = 16 + (tile * (64 * B) + lane) * 4;
    uint32_t ring[PF][B];
#pragma unroll
    for (int p = 0; p < PF; ++p)
        if (p < n) {
            const uint32_t* tw = reinterpret_cast<const uint32_t*>(row(p) + off);
#pragma unroll
            for (int k = 0; k < B; ++k) ring[p][k] = tw[k * 64];
        }
    float acc[32];
    for (int64_t i0 = 0; i0 < n; i0 += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int64_t i = i0 + p;
            if (i < n) {
                const float norm = B == 9 ? 0.f : sload(reinterpret_cast<const float*>(row(i) + 8));
                const float wi = W ? sload(w + i) : 1.f;
                float e[32];
                bt_decode<B>(ring[p], lv, norm, e);
                if (i + PF < n) {
                    const uint32_t* tw = reinterpret_cast<const uint32_t*>(row(i + PF) + off);
#pragma unroll
                    for (int k = 0; k < B; ++k) ring[p][k] = tw[k * 64];
                }
#pragma unroll
                for (int q = 0; q < 32; ++q) {
                    const float t = W ? wi * e[q] : e[q];
                    acc[q] = (i == 0) ? t : acc[q] + t;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 32; ++q) acc[q] = acc[q] / wt;
    bt_store(out, tile * BT_TILE + 4 * lane, d, acc);
}

// ---- host ------------------------------------------------------------------------------------------
static int bits_refuse(const flc_codec_params* prm, const char* me) {
    if (bits_width(prm)) return FLC_OK;
    set_error("%s: codec %d%s has no bit-packed form (natural, or standard dithering with s <= 63)", me, prm->codec,
              prm->codec == FLC_STD_DITHERING ? " with s > 63" : "");
    return FLC_ERR_UNSUPPORTED;
}

struct BitsWs {
    float* pnorm;
    void* inner;
    size_t inner_bytes;
};
static BitsWs carve_bits(void* base, const flc_codec_params* prm, int64_t d, size_t* bytes) {
    Carver c(base);
    BitsWs w;
    w.pnorm = c.take<float>(1);
    w.inner_bytes = ew_workspace(prm, 1, d);
    w.inner = c.take<char>(w.inner_bytes);
    if (bytes) *bytes = c.bytes();
    return w;
}

size_t bits_pack_workspace(const flc_codec_params* prm, int64_t d) {
    if (!bits_width(prm)) return 0;
    size_t b = 0;
    carve_bits(nullptr, prm, d, &b);
    return b;
}

// flc_pack_bits (sh null: the row x) and flc_pack_shift_bits (the row x - sh->b, with the epilogues of
// *sh): everything refused before the header is written
static int bits_pack_go(const char* me, const flc_codec_params* prm, const flc_pattern* pat, const float* x,
                        const ShiftArgs* sh, int64_t d, char* payload, void* ws, size_t ws_bytes, hipStream_t st) {
    if (int rc = bits_refuse(prm, me)) return rc;
    const bool dither = prm->codec == FLC_STD_DITHERING;
    if (dither) if (int rc = check_dither(prm)) return rc;
    if (ws_bytes < bits_pack_workspace(prm, d)) { set_error("%s: workspace too small", me); return FLC_ERR_WORKSPACE; }
    if ((uintptr_t)payload & 15u) { set_error("%s: payload must be 16-byte aligned", me); return FLC_ERR_ARG; }
    BitsWs w = carve_bits(ws, prm, d, nullptr);
    hipLaunchKernelGGL(k_bits_header, dim3(1), dim3(64), 0, st, payload, (uint32_t)bits_format(prm), (uint32_t)d);
    FLC_CHECK_LAUNCH("k_bits_header");
    if (d == 0) return FLC_OK;
    // the norm pass (over x - b for a shifted step), then ONE pass to the packed words (codecs.hip
    // ew_run -> k_ew_code_bits, or wire_shift_bits.hip's k_ew_shift_code_bits)
    CodeArgs ca{0, payload, prm->d_levels, prm->s, dither ? w.pnorm : nullptr, bits_width(prm)};
    RowSrc src{x, d, nullptr};
    const bool vec = (((uintptr_t)x | (uintptr_t)(sh ? sh->b : nullptr)) & 15u) == 0;
    return ew_run(prm, pat, src, vec, 1, d, nullptr, dither ? w.pnorm : nullptr, /*dense=*/true, nullptr, nullptr, 1.f,
                  w.inner, w.inner_bytes, st, sh, &ca);
}

int bits_pack_run(const flc_codec_params* prm, const flc_pattern* pat, const float* x, int64_t d, char* payload, void* ws,
                  size_t ws_bytes, hipStream_t st) {
    return bits_pack_go("flc_pack_bits", prm, pat, x, nullptr, d, payload, ws, ws_bytes, st);
}

int bits_pack_shift_run(const flc_codec_params* prm, const flc_pattern* pat, const float* a, int64_t d, const ShiftArgs& sh,
                        char* payload, void* ws, size_t ws_bytes, hipStream_t st) {
    return bits_pack_go("flc_pack_shift_bits", prm, pat, a, &sh, d, payload, ws, ws_bytes, st);
}

int bits_decode_check(const flc_codec_params* prm, const char* me) {
    if (int rc = bits_refuse(prm, me)) return rc;
    if (prm->codec == FLC_STD_DITHERING && !prm->d_levels) { set_error("%s: dithering needs the level table", me); return FLC_ERR_ARG; }
    return FLC_OK;
}

int bits_unpack_run(const flc_codec_params* prm, const char* payload, int64_t d, float* out, hipStream_t st) {
    if (int rc = bits_decode_check(prm, "flc_unpack_bits")) return rc;
    if (d == 0) return FLC_OK;
    if ((uintptr_t)payload & 15u) { set_error("flc_unpack_bits: payload must be 16-byte aligned"); return FLC_ERR_ARG; }
    const int grid = (int)((bits_tiles(d) + 3) / 4);
#define CASE(BB) hipLaunchKernelGGL((k_unpack_bits<BB>), dim3(grid), dim3(256), 0, st, payload, d, prm->d_levels, prm->s, out);
    FLC_BITS_SWITCH(bits_width(prm), CASE)
#undef CASE
    FLC_CHECK_LAUNCH("k_unpack_bits");
    return FLC_OK;
}

#ifndef FLC_BITS_PF
#define FLC_BITS_PF 4
#endif
int bits_unpack_reduce_run(const flc_codec_params* prm, const char* base, int64_t ld, const char* const* ptrs, int64_t n,
                           int64_t d, const float* w, float wt, float* out, hipStream_t st) {
    if (int rc = bits_decode_check(prm, "flc_unpack_reduce_bits")) return rc;
    if (base && ((ld & 15) || ((uintptr_t)base & 15u))) { set_error("flc_unpack_reduce_bits: payload rows must be 16-byte aligned"); return FLC_ERR_ARG; }
    if (d == 0) return FLC_OK;
    if (n == 0) { FLC_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)d * sizeof(float), st)); return FLC_OK; }
    const int grid = (int)((bits_tiles(d) + 3) / 4);
    ProfScope _ps("k_unpack_bits_accum", st);
#define CASE(BB)                                                                                                        \
    if (w) hipLaunchKernelGGL((k_unpack_bits_accum<BB, true, FLC_BITS_PF>), dim3(grid), dim3(256), 0, st, base, ld, ptrs, n, d, \
                              prm->d_levels, prm->s, w, wt, out);                                                       \
    else hipLaunchKernelGGL((k_unpack_bits_accum<BB, false, FLC_BITS_PF>), dim3(grid), dim3(256), 0, st, base, ld, ptrs, n, d,  \
                            prm->d_levels, prm->s, w, wt, out);
    FLC_BITS_SWITCH(bits_width(prm), CASE)
#undef CASE
    FLC_CHECK_LAUNCH("k_unpack_bits_accum");
    return FLC_OK;
}

// Host check of one bit-packed message off the network (flc_payload_validate_bits): its size, the
// header's format word (b included), count and bad, and every level index of the d elements.
int bits_payload_validate(const flc_codec_params* prm, const uint8_t* p, int64_t nbytes, int64_t d) {
    if (int rc = bits_refuse(prm, "flc_payload_validate_bits")) return rc;
    const int64_t pb = bits_payload_bytes(prm, d);
    if (nbytes < pb) { set_error("payload: %lld bytes, the bit-packed message of d=%lld is %lld", (long long)nbytes, (long long)d, (long long)pb); return FLC_ERR_ARG; }
    if (d == 0) return FLC_OK;
    PayloadHeader h;
    std::memcpy(&h, p, sizeof h);
    const int b = bits_width(prm), fmt = bits_format(prm);
    if ((int)(h.fmt & 0xFFu) != (fmt & 0xFF)) { set_error("payload: header format %u, the codec's bit-packed format is %d", h.fmt & 0xFFu, fmt & 0xFF); return FLC_ERR_ARG; }
    if ((int)h.fmt != fmt) { set_error("payload: header says b=%u bits per code, the codec's is %d", h.fmt >> 8, fmt >> 8); return FLC_ERR_ARG; }
    if (h.count != (uint32_t)d) { set_error("payload: count %u != d", h.count); return FLC_ERR_ARG; }
    if (h.bad != 0u) { set_error("payload: %u elements flagged unrepresentable by the sender", h.bad); return FLC_ERR_ARG; }
    if (b == 9) return FLC_OK;
    const uint8_t* body = p + 16;
    const uint32_t mask = (1u << (b - 1)) - 1u;
    for (int64_t j = 0; j < d; ++j) {
        const int64_t tile = j / BT_TILE, e = j % BT_TILE;
        const int lane = (int)(e % 256) / 4, i = 4 * (int)(e / 256) + (int)(e % 4), pos = i * b, k = pos >> 5, sh = pos & 31;
        const uint8_t* tw = body + tile * 256 * b;
        uint32_t lo, hi = 0;
        std::memcpy(&lo, tw + (k * 64 + lane) * 4, 4);
        if (sh + b > 32) std::memcpy(&hi, tw + ((k + 1) * 64 + lane) * 4, 4);
        const uint32_t c = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
        if ((c & mask) > (uint32_t)prm->s) { set_error("payload: level code %u at %lld exceeds s=%d", c & mask, (long long)j, prm->s); return FLC_ERR_ARG; }
    }
    return FLC_OK;
}

}  // namespace flc
