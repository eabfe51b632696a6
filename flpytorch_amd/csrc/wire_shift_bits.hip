// Bit-packed shifted steps (flc_pack_shift_bits / flc_unpack_shift_reduce_bits): the messages of
// DIANA / EF21 / MARINA at the sub-byte widths of wire_bits.hip, with the shifted round's semantics
// of wire_shift.hip:
//     client   payload = bit-pack(e), e = C(a - b);  msg = base + e * scale;  h_out = h_in + alpha * e
//     server   msg_i = base_i + dec(payload_i) * scale;  out = (sum_i w_i msg_i) / wt
// The payload is flc_pack_bits' of the row a - b byte for byte; msg / h_out / out carry the bits of
// flc_pack_shift and flc_unpack_shift_reduce over the byte payloads of the same rows: the codes are
// the same and every op is rounded separately in the order of k_ew_shift_code / k_unpack_shift_accum.
//
// Both kernels keep wire_bits.hip's ownership — a wave owns a 2048-element tile (the server: half of
// one), a lane the float4 steps 256 t + 4 l of it — so every dense element is read and written by
// exactly one lane
// and the in-place forms (msg == b, h_out == b == h_in on the client; the EF21 mirror msg == base on
// the server) stay legal: a lane's loads of an element precede its store of it.
#include "wire_bits.hpp"

namespace flc {

// ---- client --------------------------------------------------------------------------------------
// k_ew_code_bits' tile walk over a - b with k_ew_shift_code's epilogues.  Per step a lane holds the
// float4 of a, b and (when asked) base and h_in; the NEXT step's are issued before the current step
// is encoded, so up to four 16-B loads per lane are in flight under the dither / code arithmetic.
// The four codes go into the B word registers at constant positions (bt_put), msg and h_out are
// stored from the same registers, and the tile ends with B coalesced dword stores.  No byte-format
// payload and no dense e row is written.  Nothing at or past d is read: those elements are code 0.
// VEC: every operand in use is 16-byte aligned (whole groups as float4, the group that crosses d by
// element); else element loads and stores, the same bits.
struct ShiftIn {
    float4 a, b, bs, h;
};

template <class Op, int B, bool VEC>
__global__ __launch_bounds__(256) void k_ew_shift_code_bits(const float* a, int64_t d, Op op,
                                                            const float* __restrict__ levels, int s, ShiftArgs sh,
                                                            CodeArgs ca) {
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
    const bool has_base = sh.msg && sh.base;
    auto ld4 = [&](const float* p, int64_t j) -> float4 {
        if (VEC && j + 3 < d) return *reinterpret_cast<const float4*>(p + j);
        return make_float4(j < d ? p[j] : 0.f, j + 1 < d ? p[j + 1] : 0.f, j + 2 < d ? p[j + 2] : 0.f,
                           j + 3 < d ? p[j + 3] : 0.f);
    };
    auto ld = [&](int64_t j) -> ShiftIn {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        ShiftIn v;
        v.a = ld4(a, j);
        v.b = ld4(sh.b, j);
        v.bs = has_base ? ld4(sh.base, j) : z;
        v.h = sh.hout ? ld4(sh.hin, j) : z;
        return v;
    };
    const int lane = threadIdx.x & 63;
    const int64_t tiles = (d + BT_TILE - 1) / BT_TILE;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t j0 = tile * BT_TILE + 4 * lane;
        uint32_t w[B];
#pragma unroll
        for (int k = 0; k < B; ++k) w[k] = 0u;
        ShiftIn nxt = ld(j0);
#pragma unroll 1
        for (int t = 0; t < 8; ++t) {
            const int64_t j = j0 + 256 * t;
            const ShiftIn in = nxt;
            if (t < 7) nxt = ld(j + 256);                    // the next step's loads, before this step's stores
            const float4 v = make_float4(in.a.x - in.b.x, in.a.y - in.b.y, in.a.z - in.b.z, in.a.w - in.b.w);
            const bool whole = VEC && j + 3 < d;
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            uint32_t c[4] = {0u, 0u, 0u, 0u};
            if (whole) {
                uint32_t cs[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) cs[q] = op.col(j + q);
                const float4 e4 = op.row_fast() ? apply4<true>(op, v, j, cs, smem_tab) : apply4<false>(op, v, j, cs, smem_tab);
                e[0] = e4.x; e[1] = e4.y; e[2] = e4.z; e[3] = e4.w;
#pragma unroll
                for (int q = 0; q < 4; ++q) c[q] = code(e[q]);
            } else {
                const float ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (j + q < d) {
                        e[q] = op.template apply<false>(ve[q], j + q, op.col(j + q), smem_tab);
                        c[q] = code(e[q]);
                    }
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
            // the epilogues, k_ew_shift_code's ops: t = e * scale; msg = base + t; h_out = h_in + alpha * e
            if (sh.msg) {
                const float bs[4] = {in.bs.x, in.bs.y, in.bs.z, in.bs.w};
                float m[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float ts = e[q] * sh.scale;
                    m[q] = sh.base ? bs[q] + ts : ts;
                }
                if (whole) {
                    *reinterpret_cast<float4*>(sh.msg + j) = make_float4(m[0], m[1], m[2], m[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (j + q < d) sh.msg[j + q] = m[q];
                }
            }
            if (sh.hout) {
                const float hv[4] = {in.h.x, in.h.y, in.h.z, in.h.w};
                float o[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = hv[q] + sh.alpha * e[q];
                if (whole) {
                    *reinterpret_cast<float4*>(sh.hout + j) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (j + q < d) sh.hout[j + q] = o[q];
                }
            }
        }
        uint32_t* tw = body + tile * (64 * B) + lane;
#pragma unroll
        for (int k = 0; k < B; ++k) tw[k * 64] = w[k];
    }
}

// the vector kernel needs every operand in use 16-byte aligned (the payload always is); one profile
// record per call
template <class Op, int B>
static int launch_shift_code_b(const float* a, int64_t d, Op op, const float* levels, int s, const ShiftArgs& sh,
                               const CodeArgs& ca, hipStream_t st) {
    const uintptr_t al = (uintptr_t)a | (uintptr_t)sh.b | (uintptr_t)sh.base | (uintptr_t)sh.msg |
                         (uintptr_t)sh.hin | (uintptr_t)sh.hout;
    const bool vec = (al & 15u) == 0;
    const size_t lds = Op::TABLE ? (size_t)s * sizeof(float4) : 0;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(((d + BT_TILE - 1) / BT_TILE + 3) / 4, 4096));
    ProfScope _ps("k_ew_shift_code_bits", st);
    if (vec) hipLaunchKernelGGL((k_ew_shift_code_bits<Op, B, true>), dim3(grid), dim3(256), lds, st, a, d, op, levels, s, sh, ca);
    else hipLaunchKernelGGL((k_ew_shift_code_bits<Op, B, false>), dim3(grid), dim3(256), lds, st, a, d, op, levels, s, sh, ca);
    FLC_CHECK_LAUNCH("k_ew_shift_code_bits");
    return FLC_OK;
}

template <class Op>
int launch_shift_code_bits(const float* a, int64_t d, Op op, const float* levels, int s, const ShiftArgs& sh,
                           const CodeArgs& ca, hipStream_t st) {
    if (d == 0) return FLC_OK;
    if constexpr (Op::TABLE) {
        switch (ca.bits) {
            case 2: return launch_shift_code_b<Op, 2>(a, d, op, levels, s, sh, ca, st);
            case 3: return launch_shift_code_b<Op, 3>(a, d, op, levels, s, sh, ca, st);
            case 4: return launch_shift_code_b<Op, 4>(a, d, op, levels, s, sh, ca, st);
            case 5: return launch_shift_code_b<Op, 5>(a, d, op, levels, s, sh, ca, st);
            case 6: return launch_shift_code_b<Op, 6>(a, d, op, levels, s, sh, ca, st);
            case 7: return launch_shift_code_b<Op, 7>(a, d, op, levels, s, sh, ca, st);
            default: break;
        }
    } else if (ca.bits == 9) {
        return launch_shift_code_b<Op, 9>(a, d, op, levels, s, sh, ca, st);
    }
    set_error("flc_pack_shift_bits: no %d-bit form of this codec", ca.bits);
    return FLC_ERR_UNSUPPORTED;
}
template int launch_shift_code_bits(const float*, int64_t, DitherOp<false, true>, const float*, int, const ShiftArgs&, const CodeArgs&, hipStream_t);
template int launch_shift_code_bits(const float*, int64_t, DitherOp<false, false>, const float*, int, const ShiftArgs&, const CodeArgs&, hipStream_t);
template int launch_shift_code_bits(const float*, int64_t, NaturalOp<true>, const float*, int, const ShiftArgs&, const CodeArgs&, hipStream_t);
template int launch_shift_code_bits(const float*, int64_t, NaturalOp<false>, const float*, int, const ShiftArgs&, const CodeArgs&, hipStream_t);

// ---- server --------------------------------------------------------------------------------------
// a lane's 16 elements of one dense row of its half tile: four float4, or the elements below d (0 past d)
template <bool VEC>
__device__ inline void bth_load(const float* br, int64_t j0, int64_t d, float* v) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t j = j0 + 256 * t;
        if (VEC && j + 3 < d) {
            const float4 b4 = *reinterpret_cast<const float4*>(br + j);
            v[4 * t] = b4.x; v[4 * t + 1] = b4.y; v[4 * t + 2] = b4.z; v[4 * t + 3] = b4.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[4 * t + q] = j + q < d ? br[j + q] : 0.f;
        }
    }
}

template <bool VEC>
__device__ inline void bth_store(float* br, int64_t j0, int64_t d, const float* v) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t j = j0 + 256 * t;
        if (VEC && j + 3 < d) {
            *reinterpret_cast<float4*>(br + j) = make_float4(v[4 * t], v[4 * t + 1], v[4 * t + 2], v[4 * t + 3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (j + q < d) br[j + q] = v[4 * t + q];
        }
    }
}

// Tile owner, k_unpack_bits_accum's ownership (a wave folds its elements for all n rows in client
// order, the level table one register per lane) with k_unpack_shift_accum's row step:
//     e = dec(code);  t = e * scale;  m = base_i + t (or t);  acc = first ? w_i m : acc + w_i m
// m stored to msg row i when asked, out = acc / wt.  The fold moves 8 n d bytes of mirror where the
// plain one moves none, so the loads are kept in flight by hand: PF rows' payload words per lane sit
// in a register ring, and the base float4 of row i + 1 are issued into the other half of a two-row
// register buffer BEFORE row i's arithmetic and stores (row i + 1's base is then never behind row
// i's msg stores in program order; the host refuses msg rows that overlap other base rows).  A
// shared base is loaded once, outside the row loop, into both halves of the buffer.
//
// A wave owns HALF a tile: steps t = 4 H .. 4 H + 3 of a lane, its codes 16 H .. 16 H + 15, which lie
// in words K0 .. K0 + NW - 1 of the lane (BtHalf; NW = ceil(B / 2), every word access still a whole
// coalesced 256 B of the wave).  With the whole tile per wave the ring, the two base rows, the
// decoded row and the accumulators are 36 + 64 + 32 + 32 live values and the compiler's report was
// 227-255 VGPRs with 32 more moved to AGPRs for B = 5..7, one or two waves per SIMD; the half is
// 16 accumulators, 2 x 16 base values and PF x NW words.  Every index is a constant after unrolling
// (PF even: row i's buffer half is i & 1 == p & 1), so nothing lives in scratch.
// VEC: base / msg 16-byte aligned with leading dimensions multiples of 4; else by element.
struct ShiftFoldArgs {
    const char* pbase; int64_t ld;
    const char* const* ptrs;
    int64_t n, d;
    float scale;
    const float* base; int64_t ldbase; int base_mode;
    float* msg; int64_t ldmsg;
    const float* w; float wt;
    float* out;
};

template <int B, bool W, int PF, bool VEC, int H>
__device__ inline void shift_fold_half(const ShiftFoldArgs& g, int64_t tile, int lane, float lv) {
    static_assert(PF % 2 == 0, "the base buffer's half is the ring slot's parity");
    constexpr int K0 = BtHalf<B, H>::K0, NW = BtHalf<B, H>::NW;
    const int64_t n = g.n, d = g.d;
    auto row = [&](int64_t i) -> const char* { return g.pbase ? g.pbase + i * g.ld : sload(g.ptrs + i); };
    const int64_t off = 16 + (tile * (64 * B) + K0 * 64 + lane) * 4;
    const int64_t j0 = tile * BT_TILE + 1024 * H + 4 * lane;
    uint32_t ring[PF][NW];
#pragma unroll
    for (int p = 0; p < PF; ++p)
        if (p < n) {
            const uint32_t* tw = reinterpret_cast<const uint32_t*>(row(p) + off);
#pragma unroll
            for (int k = 0; k < NW; ++k) ring[p][k] = tw[k * 64];
        }
    float bb[2][16];
    if (g.base_mode != UB_NONE) {                              // row 0's base, or the shared one for every row
        bth_load<VEC>(g.base, j0, d, bb[0]);
        if (g.base_mode == UB_SHARED) {
#pragma unroll
            for (int q = 0; q < 16; ++q) bb[1][q] = bb[0][q];
        }
    }
    float acc[16];
    for (int64_t i0 = 0; i0 < n; i0 += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int64_t i = i0 + p;
            if (i < n) {
                if (g.base_mode == UB_ROWS && i + 1 < n) bth_load<VEC>(g.base + (i + 1) * g.ldbase, j0, d, bb[(p + 1) & 1]);
                const float norm = B == 9 ? 0.f : sload(reinterpret_cast<const float*>(row(i) + 8));
                const float wi = W ? sload(g.w + i) : 1.f;
                float m[16];
                bt_decode_half<B, H>(ring[p], lv, norm, m);
                if (i + PF < n) {
                    const uint32_t* tw = reinterpret_cast<const uint32_t*>(row(i + PF) + off);
#pragma unroll
                    for (int k = 0; k < NW; ++k) ring[p][k] = tw[k * 64];
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float ts = m[q] * g.scale;
                    m[q] = g.base_mode != UB_NONE ? bb[p & 1][q] + ts : ts;
                    const float wm = W ? wi * m[q] : m[q];
                    acc[q] = (i == 0) ? wm : acc[q] + wm;
                }
                if (g.msg) bth_store<VEC>(g.msg + i * g.ldmsg, j0, d, m);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = acc[q] / g.wt;
    if (((uintptr_t)g.out & 15u) == 0) bth_store<true>(g.out, j0, d, acc);
    else bth_store<false>(g.out, j0, d, acc);
}

template <int B, bool W, int PF, bool VEC>
__global__ __launch_bounds__(256) void k_unpack_bits_shift_accum(ShiftFoldArgs g, const float* __restrict__ levels, int s) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // (tile, half), wave-uniform
    const int64_t tile = unit >> 1;
    if (tile * BT_TILE + 1024 * (unit & 1) >= g.d) return;     // a whole wave leaves: the others stay complete
    const float lv = B == 9 ? 0.f : fabsf(levels[min(lane, s)]);
    if (unit & 1) shift_fold_half<B, W, PF, VEC, 1>(g, tile, lane, lv);
    else shift_fold_half<B, W, PF, VEC, 0>(g, tile, lane, lv);
}

#ifndef FLC_SHIFT_BITS_PF
#define FLC_SHIFT_BITS_PF 4
#endif
int bits_unpack_shift_reduce_run(const flc_codec_params* prm, const flc_payload_rows& pr, int64_t n, int64_t d,
                                 const float* w, float wt, float* out, hipStream_t st) {
    if (int rc = bits_decode_check(prm, "flc_unpack_shift_reduce_bits")) return rc;
    if (d == 0) return FLC_OK;
    if (n == 0) { FLC_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)d * sizeof(float), st)); return FLC_OK; }
    const int grid = (int)((2 * ((d + BT_TILE - 1) / BT_TILE) + 3) / 4);      // a wave per half tile
    uintptr_t pal = 0;
    uint64_t lal = 0;
    if (pr.d_base) { pal |= (uintptr_t)pr.d_base; lal |= (uint64_t)pr.ldbase; }
    if (pr.d_msg) { pal |= (uintptr_t)pr.d_msg; lal |= (uint64_t)pr.ldmsg; }
    const bool vec = (pal & 15u) == 0 && (lal & 3u) == 0;
    const ShiftFoldArgs g{static_cast<const char*>(pr.d_payloads), pr.ld_bytes,
                          reinterpret_cast<const char* const*>(pr.d_payload_ptrs), n, d, pr.msg_scale,
                          pr.d_base, pr.ldbase, !pr.d_base ? UB_NONE : (pr.ldbase == 0 ? UB_SHARED : UB_ROWS),
                          pr.d_msg, pr.ldmsg, w, wt, out};
    ProfScope _ps("k_unpack_bits_shift_accum", st);
#define GO(BB, WW, VV)                                                                                               \
    hipLaunchKernelGGL((k_unpack_bits_shift_accum<BB, WW, FLC_SHIFT_BITS_PF, VV>), dim3(grid), dim3(256), 0, st, g,   \
                       prm->d_levels, prm->s);
#define CASE(BB)                                                    \
    if (w) { if (vec) GO(BB, true, true) else GO(BB, true, false) } \
    else { if (vec) GO(BB, false, true) else GO(BB, false, false) }
    FLC_BITS_SWITCH(bits_width(prm), CASE)
#undef CASE
#undef GO
    FLC_CHECK_LAUNCH("k_unpack_bits_shift_accum");
    return FLC_OK;
}

}  // namespace flc
