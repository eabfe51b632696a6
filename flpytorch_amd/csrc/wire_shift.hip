// Shifted steps on the wire: the client step e = C(a - b) of DIANA / EF21 / MARINA that emits its
// message (flc_pack_shift), and the server fold of n such messages with the shifted round's
// semantics (flc_unpack_shift_reduce):
//     client   payload = pack(e);  msg = base + e * scale;  h_out = h_in + alpha * e
//     server   msg_i = base_i + dec(payload_i) * scale;  out = (sum_i w_i msg_i) / wt
// n x flc_pack_shift followed by flc_unpack_shift_reduce leaves flc_encode_shift_reduce's d_out and
// d_msg rows bit for bit: dec(pack(e)) == e (wire.hip), and both sides round every op separately in
// the order of k_ew_shift_accum.
//
// Client, dense formats: the norm pass over a - b, then ONE pass (codecs.hip k_ew_shift_code).
// Client, SPARSE: a - b and the dense e in the workspace (shift.hip), the compaction of flc_pack
// (wire.hip k_pack_*), then the epilogue over the stored e — a constant number of launches.
// Server, dense formats: one tile-owner pass (k_unpack_shift_accum below).  Server, SPARSE: row by
// row through a dense workspace row (k_unpack_sparse_row, k_shift_epi, k_shift_fold), so the bits are
// the dense shifted round's.
#include "wire_codes.hpp"

namespace flc {

// ---- client --------------------------------------------------------------------------------------
struct PackShiftWs {
    float* pnorm;
    uint32_t* bc;
    void* inner;
    size_t inner_bytes;
};
static PackShiftWs carve_pack_shift(void* base, const flc_codec_params* prm, int64_t d, size_t* bytes) {
    Carver c(base);
    PackShiftWs w;
    const bool sparse = payload_format(prm) == FMT_SPARSE;
    w.pnorm = c.take<float>(1);
    w.bc = c.take<uint32_t>(sparse ? (size_t)pack_blocks(d) : 0);
    w.inner_bytes = shift_workspace(prm, d);
    w.inner = c.take<char>(w.inner_bytes);
    if (bytes) *bytes = c.bytes();
    return w;
}

size_t pack_shift_workspace(const flc_codec_params* prm, int64_t d) {
    size_t b = 0;
    carve_pack_shift(nullptr, prm, d, &b);
    return std::max(b, d == 0 ? pack_workspace(prm, 0) : (size_t)0);   // d == 0: flc_pack's empty header
}

// what the encode would refuse after the payload's header has been zeroed: refused here, before it
static int pack_shift_precheck(const flc_codec_params* prm, const flc_pattern* pat, int64_t d) {
    const int codec = prm->codec;
    if (codec == FLC_LAZY && !(pat && pat->d_lazy_u)) { set_error("lazy: pattern needs d_lazy_u"); return FLC_ERR_ARG; }
    if (codec == FLC_STD_DITHERING || codec == FLC_NAT_DITHERING)
        if (int rc = check_dither(prm)) return rc;
    if (codec == FLC_RANDK && !(pat && pat->d_randk_idx) && prm->k > d) { set_error("randk: K > D"); return FLC_ERR_ARG; }
    if ((codec == FLC_RANDK || codec == FLC_TOPK) && prm->k < 1) { set_error("flc_pack_shift: K < 1"); return FLC_ERR_ARG; }
    return FLC_OK;
}

int pack_shift_run(const flc_codec_params* prm, const flc_pattern* pat, const float* a, int64_t d, const ShiftArgs& sh,
                   char* payload, void* ws, size_t ws_bytes, hipStream_t st) {
    if (ws_bytes < pack_shift_workspace(prm, d)) { set_error("flc_pack_shift: workspace too small"); return FLC_ERR_WORKSPACE; }
    if (d == 0) return pack_run(prm, pat, nullptr, 0, payload, ws, ws_bytes, st);
    if (int rc = pack_shift_precheck(prm, pat, d)) return rc;
    const int fmt = payload_format(prm);
    PackShiftWs w = carve_pack_shift(ws, prm, d, nullptr);
    const int64_t pb = payload_bytes(prm, d);
    if (fmt == FMT_SPARSE) {
        float* e = nullptr;
        if (int rc = shift_encode_dense(prm, pat, a, sh.b, d, &e, w.inner, w.inner_bytes, st)) return rc;
        // the unused part of the list and the padding zeroed: a payload's bytes are a function of the row alone
        FLC_CHECK_HIP(hipMemsetAsync(payload, 0, (size_t)pb, st));
        if (int rc = pack_sparse_launch(e, d, std::max<int64_t>(1, std::min(prm->k, d)), w.bc, payload, st)) return rc;
        return (sh.msg || sh.hout) ? shift_epi_launch(e, d, sh, st) : FLC_OK;
    }
    // header (its `bad` word counts up from 0) and the body's last 16 bytes (the padding) zeroed
    FLC_CHECK_HIP(hipMemsetAsync(payload, 0, 16, st));
    FLC_CHECK_HIP(hipMemsetAsync(payload + pb - 16, 0, 16, st));
    const bool dither = fmt == FMT_Q8 || fmt == FMT_Q16;
    CodeArgs ca{fmt, payload, prm->d_levels, prm->s, dither ? w.pnorm : nullptr};
    RowSrc src{a, d, nullptr};
    const bool vec = (((uintptr_t)a | (uintptr_t)sh.b) & 15u) == 0;
    return ew_run(prm, pat, src, vec, 1, d, nullptr, dither ? w.pnorm : nullptr, /*dense=*/true, nullptr, nullptr, 1.f,
                  w.inner, w.inner_bytes, st, &sh, &ca);
}

// ---- server, dense formats -----------------------------------------------------------------------
// Tile owner, as k_unpack_accum: a thread owns the E elements of one 16-B body slice (16 Q8 codes,
// 8 Q16 / NAT16 codes, 4 floats) for all n rows, rows in order, PF rows' slices in flight.  Per row
//     e = dec(code);  t = e * scale;  m = base_i + t (or t);  acc = first ? w_i m : acc + w_i m
// each op rounded separately exactly as k_ew_shift_accum; m is stored to msg row i when asked (row i
// of base included: every element of a row is read and written by one thread, the base load before
// the store).  A shared base (MARINA's g_prev) is loaded once, outside the row loop.  VEC: base / msg
// rows as float4s (16-byte aligned, leading dimensions multiples of 4); else element loads and stores,
// the same bits.  The format and s come from the codec, never from the message.
enum { UB_NONE = 0, UB_ROWS = 1, UB_SHARED = 2 };

template <int FMT, bool W, int PF, bool VEC>
__global__ __launch_bounds__(256) void k_unpack_shift_accum(const char* __restrict__ pbase, int64_t ld,
                                                            const char* const* __restrict__ ptrs, int64_t n, int64_t d,
                                                            const float* __restrict__ levels, int s, float scale,
                                                            const float* base, int64_t ldbase, int base_mode,
                                                            float* msg, int64_t ldmsg, const float* __restrict__ w,
                                                            float wt, float* __restrict__ out) {
    constexpr int E = WireFmt<FMT>::E;
    __shared__ float lvs[128];
    const float* lv = levels;
    if (FMT == FMT_Q8) {
        for (int i = threadIdx.x; i <= s && i < 128; i += 256) lvs[i] = levels[i];
        __syncthreads();
        lv = lvs;
    }
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t j0 = g * E;
    const int64_t full = d / E;                       // complete 16-B slices
    auto row = [&](int64_t i) -> const char* { return pbase ? pbase + i * ld : sload(ptrs + i); };
    if (g < full) {
        uint4 ring[PF];
#pragma unroll
        for (int p = 0; p < PF; ++p)
            if (p < n) ring[p] = *reinterpret_cast<const uint4*>(row(p) + 16 + g * 16);
        float sb[E];                                   // the shared base's elements
        if (base_mode == UB_SHARED) {
            if (VEC) {
#pragma unroll
                for (int q = 0; q < E; q += 4) {
                    const float4 b4 = *reinterpret_cast<const float4*>(base + j0 + q);
                    sb[q] = b4.x; sb[q + 1] = b4.y; sb[q + 2] = b4.z; sb[q + 3] = b4.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < E; ++q) sb[q] = base[j0 + q];
            }
        }
        float acc[E];
        for (int64_t i0 = 0; i0 < n; i0 += PF) {
#pragma unroll
            for (int p = 0; p < PF; ++p) {
                const int64_t i = i0 + p;
                if (i < n) {
                    const char* r = row(i);
                    const float norm = (FMT == FMT_Q8 || FMT == FMT_Q16) ? sload(reinterpret_cast<const float*>(r + 8)) : 0.f;
                    const float wi = W ? w[i] : 1.f;
                    float bs[E];
                    if (base_mode == UB_ROWS) {        // the row's base before any store of the row
                        const float* br = base + i * ldbase + j0;
                        if (VEC) {
#pragma unroll
                            for (int q = 0; q < E; q += 4) {
                                const float4 b4 = *reinterpret_cast<const float4*>(br + q);
                                bs[q] = b4.x; bs[q + 1] = b4.y; bs[q + 2] = b4.z; bs[q + 3] = b4.w;
                            }
                        } else {
#pragma unroll
                            for (int q = 0; q < E; ++q) bs[q] = br[q];
                        }
                    } else if (base_mode == UB_SHARED) {
#pragma unroll
                        for (int q = 0; q < E; ++q) bs[q] = sb[q];
                    }
                    float e[E];
                    dec16<FMT>(ring[p], lv, s, norm, e);
                    if (i + PF < n) ring[p] = *reinterpret_cast<const uint4*>(row(i + PF) + 16 + g * 16);
                    float m[E];
#pragma unroll
                    for (int q = 0; q < E; ++q) {
                        const float t = e[q] * scale;
                        m[q] = base_mode != UB_NONE ? bs[q] + t : t;
                        const float wm = W ? wi * m[q] : m[q];
                        acc[q] = (i == 0) ? wm : acc[q] + wm;
                    }
                    if (msg) {
                        float* mr = msg + i * ldmsg + j0;
                        if (VEC) {
#pragma unroll
                            for (int q = 0; q < E; q += 4)
                                *reinterpret_cast<float4*>(mr + q) = make_float4(m[q], m[q + 1], m[q + 2], m[q + 3]);
                        } else {
#pragma unroll
                            for (int q = 0; q < E; ++q) mr[q] = m[q];
                        }
                    }
                }
            }
        }
        if (((uintptr_t)(out + j0) & 15u) == 0) {
            float4* o4 = reinterpret_cast<float4*>(out + j0);
#pragma unroll
            for (int q = 0; q < E; q += 4) o4[q / 4] = make_float4(acc[q] / wt, acc[q + 1] / wt, acc[q + 2] / wt, acc[q + 3] / wt);
        } else {
#pragma unroll
            for (int q = 0; q < E; ++q) out[j0 + q] = acc[q] / wt;
        }
        return;
    }
    if (g == full && full * E < d) {                   // the tail: fewer than E elements, element loads
        const int mt = (int)(d - full * E);
        float acc[E];
        for (int64_t i = 0; i < n; ++i) {
            const char* r = row(i);
            const float norm = (FMT == FMT_Q8 || FMT == FMT_Q16) ? reinterpret_cast<const float*>(r + 8)[0] : 0.f;
            const float wi = W ? w[i] : 1.f;
            for (int q = 0; q < mt; ++q) {
                const int64_t j = full * E + q;
                uint32_t c;
                if (FMT == FMT_Q8) c = reinterpret_cast<const uint8_t*>(r + 16)[j];
                else if (FMT == FMT_F32) c = reinterpret_cast<const uint32_t*>(r + 16)[j];
                else c = reinterpret_cast<const uint16_t*>(r + 16)[j];
                const float t = dec1<FMT>(c, lv, s, norm) * scale;
                const float m = base_mode != UB_NONE ? base[i * ldbase + j] + t : t;
                const float wm = W ? wi * m : m;
                acc[q] = (i == 0) ? wm : acc[q] + wm;
                if (msg) msg[i * ldmsg + j] = m;
            }
        }
        for (int q = 0; q < mt; ++q) out[full * E + q] = acc[q] / wt;
    }
}

// ---- server, SPARSE ------------------------------------------------------------------------------
// wire.hip's k_unpack_sparse over payload i of the strided rows or the device pointer list: the
// entries into a zeroed dense row; an index past the row is never written, a count past K is cut
__global__ __launch_bounds__(256) void k_unpack_sparse_row(const char* __restrict__ pbase, int64_t ld,
                                                           const char* const* __restrict__ ptrs, int64_t i, int64_t cap,
                                                           int64_t d, float* __restrict__ out) {
    const char* payload = pbase ? pbase + i * ld : sload(ptrs + i);
    const PayloadHeader h = *reinterpret_cast<const PayloadHeader*>(payload);
    const uint32_t* idx = reinterpret_cast<const uint32_t*>(payload + 16);
    const float* val = reinterpret_cast<const float*>(payload + 16 + a16(4 * cap));
    const int64_t cnt = min<int64_t>(h.count, cap);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cnt; e += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t j = idx[e];
        if (j < (uint64_t)d) out[j] = val[e];
    }
}

// ---- server, host --------------------------------------------------------------------------------
struct UnpackShiftWs {
    float* e;
    float* mrow;
};
static UnpackShiftWs carve_unpack_shift(void* base, const flc_codec_params* prm, int64_t d, size_t* bytes) {
    Carver c(base);
    UnpackShiftWs w{nullptr, nullptr};
    if (payload_format(prm) == FMT_SPARSE) {
        w.e = c.take<float>((size_t)d);
        w.mrow = c.take<float>((size_t)d);
    }
    if (bytes) *bytes = c.bytes();
    return w;
}

size_t unpack_shift_reduce_workspace(const flc_codec_params* prm, int64_t n, int64_t d) {
    (void)n;
    size_t b = 0;
    carve_unpack_shift(nullptr, prm, d, &b);
    return b;
}

int unpack_shift_reduce_run(const flc_codec_params* prm, const flc_payload_rows& pr, int64_t n, int64_t d,
                            const float* w, float wt, float* out, void* ws, size_t ws_bytes, hipStream_t st) {
    if (d == 0) return FLC_OK;
    if (ws_bytes < unpack_shift_reduce_workspace(prm, n, d)) { set_error("flc_unpack_shift_reduce: workspace too small"); return FLC_ERR_WORKSPACE; }
    if (n == 0) { FLC_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)d * sizeof(float), st)); return FLC_OK; }
    const int fmt = payload_format(prm);
    const char* pbase = static_cast<const char*>(pr.d_payloads);
    const char* const* ptrs = reinterpret_cast<const char* const*>(pr.d_payload_ptrs);
    if (fmt == FMT_SPARSE) {
        // row by row: payload i into a zeroed dense row (its address taken on the device: a pointer
        // list is never read back), the epilogue into msg row i or the workspace's, one fold step
        UnpackShiftWs u = carve_unpack_shift(ws, prm, d, nullptr);
        const int64_t cap = std::max<int64_t>(1, std::min(prm->k, d));
        const int sg = (int)std::max<int64_t>(1, std::min<int64_t>((cap + 255) / 256, 4096));
        for (int64_t i = 0; i < n; ++i) {
            FLC_CHECK_HIP(hipMemsetAsync(u.e, 0, (size_t)d * sizeof(float), st));
            hipLaunchKernelGGL(k_unpack_sparse_row, dim3(sg), dim3(256), 0, st, pbase, pr.ld_bytes, ptrs, i, cap, d, u.e);
            FLC_CHECK_LAUNCH("k_unpack_sparse_row");
            float* m = pr.d_msg ? pr.d_msg + i * pr.ldmsg : u.mrow;
            ShiftArgs sh{nullptr, pr.msg_scale, pr.d_base ? pr.d_base + i * pr.ldbase : nullptr, m, 0.f, nullptr, nullptr};
            if (int rc = shift_epi_launch(u.e, d, sh, st)) return rc;
            if (int rc = shift_fold_launch(m, d, w, i, i == n - 1, wt, out, st)) return rc;
        }
        return FLC_OK;
    }
    if (fmt == FMT_Q8 && prm->s > 127) { set_error("flc_unpack_shift_reduce: Q8 with s > 127"); return FLC_ERR_ARG; }
    const int E = fmt == FMT_Q8 ? 16 : (fmt == FMT_F32 ? 4 : 8);
    const int64_t groups = d / E + 1;
    const int grid = (int)((groups + 255) / 256);
    const int base_mode = !pr.d_base ? UB_NONE : (pr.ldbase == 0 ? UB_SHARED : UB_ROWS);
    uintptr_t pal = 0;
    uint64_t lal = 0;
    if (pr.d_base) { pal |= (uintptr_t)pr.d_base; lal |= (uint64_t)pr.ldbase; }
    if (pr.d_msg) { pal |= (uintptr_t)pr.d_msg; lal |= (uint64_t)pr.ldmsg; }
    const bool vec = (pal & 15u) == 0 && (lal & 3u) == 0;
#define UNPACK_SHIFT_GO(F, WW, VV)                                                                              \
    hipLaunchKernelGGL((k_unpack_shift_accum<F, WW, 4, VV>), dim3(grid), dim3(256), 0, st, pbase, pr.ld_bytes,  \
                       ptrs, n, d, prm->d_levels, prm->s, pr.msg_scale, pr.d_base, pr.ldbase, base_mode,        \
                       pr.d_msg, pr.ldmsg, w, wt, out)
#define UNPACK_SHIFT_CASE(F)                                                       \
    if (w) { if (vec) UNPACK_SHIFT_GO(F, true, true); else UNPACK_SHIFT_GO(F, true, false); }     \
    else { if (vec) UNPACK_SHIFT_GO(F, false, true); else UNPACK_SHIFT_GO(F, false, false); }
    { ProfScope _ps("k_unpack_shift_accum", st);
    if (fmt == FMT_Q8) { UNPACK_SHIFT_CASE(FMT_Q8) }
    else if (fmt == FMT_Q16) { UNPACK_SHIFT_CASE(FMT_Q16) }
    else if (fmt == FMT_NAT16) { UNPACK_SHIFT_CASE(FMT_NAT16) }
    else { UNPACK_SHIFT_CASE(FMT_F32) } }
#undef UNPACK_SHIFT_CASE
#undef UNPACK_SHIFT_GO
    FLC_CHECK_LAUNCH("k_unpack_shift_accum");
    return FLC_OK;
}

}  // namespace flc
