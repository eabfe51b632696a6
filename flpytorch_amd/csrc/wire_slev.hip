// Sparse level messages (flc_pack_slev / flc_unpack_slev / flc_unpack_reduce_slev): the Q8 message
// of standard dithering / QSGD / TernGrad (s <= 127) as lists of its nonzero codes.  An element is
// nonzero only when it reaches level 1 or its draw goes up, so E[nonzeros] <= s sqrt(d): at s = 127,
// d = 25 M at most 2.5 % of the row, where FMT_Q8 ships a byte for every element.
//
//   SLEV (10)  header  16 B   {10, count = d, norm, bad}                      C = ceil(d / 4096)
//              tab     a16(4 (C + 1)) B  u32 exclusive offsets of the chunks' entries, tab[C] = nnz
//              idx     a16(2 nnz) B      u16 chunk-local index (0..4095), ascending inside a chunk
//              code    a16(nnz) B        u8  FMT_Q8's code of that element (sign << 7 | level index)
//
// Listed: the elements whose encoded value is neither +0 nor -0.  The sign of an unlisted zero does
// not travel (about half of a dense QSGD row is -0: one bit per element, more than the rest of the
// message), so every contract below is on canon(a) = bits(a + 0.0f): flc_unpack_slev(flc_pack_slev(x))
// and flc_unpack(flc_pack(x)) have equal canon, and so do the two folds.  The code plane's offset
// depends on nnz: a reader takes tab[C] first.  Capacity (what a caller provides): the size at
// nnz = d.
//
// Pack: the norm pass, then k_slev_stage (a wave per chunk: encode as k_ew_code does, compact the
// listed elements into wave-private LDS in index order, copy the runs to fixed workspace regions),
// k_slev_scan (one workgroup: the counts' exclusive scan straight into tab, the padding bytes) and
// k_slev_gather (the staged runs to their offsets).  No dense message row is written.
// Fold: a one-wave workgroup owns chunk c as a 4096-float LDS tile, walks the rows in order and adds
// each row's entries by read-modify-write (indices inside one row's chunk are distinct, rows are
// serialized in the wave: no LDS atomics), so every nonzero sum carries the dense fold's bits.
// Whatever the bytes, a decode kernel never indexes outside its tile, the level table or, for a
// message in a capacity-sized buffer, the message: idx & 4095, a table of 128 clamped levels, entry
// ranges clamped to [0, min(tab[C], d)].
#include <algorithm>
#include <cmath>
#include <cstring>

#include "wire_slev.hpp"

namespace flc {

bool slev_ok(const flc_codec_params* prm) { return prm->codec == FLC_STD_DITHERING && prm->s >= 1 && prm->s <= 127; }

static int64_t slev_chunks(int64_t d) { return (d + CHUNK - 1) / CHUNK; }
static int64_t slev_idx_off(int64_t d) { return 16 + a16(4 * (slev_chunks(d) + 1)); }

int64_t slev_used_bytes(int64_t d, int64_t nnz) { return slev_idx_off(d) + a16(2 * nnz) + a16(nnz); }

typedef uint32_t __attribute__((may_alias)) u32a;
// a message's planes as global-memory pointers: a pointer rebuilt from two registers is generic to
// the compiler, and a flat load counts in the LDS counter the tile updates wait on
template <class T>
using gptr = const __attribute__((address_space(1))) T*;

// ---- pack ------------------------------------------------------------------------------------------
// the whole header before the stage pass counts into `bad`; the message of d == 0 is complete here
// (tab[0] = 0 and its padding)
__global__ void k_slev_header(char* payload, uint32_t count) {
    if (threadIdx.x == 0) {
        PayloadHeader* h = reinterpret_cast<PayloadHeader*>(payload);
        h->fmt = FMT_SLEV;
        h->count = count;
        h->norm = 0.f;
        h->bad = 0u;
        if (count == 0u) *reinterpret_cast<uint4*>(payload + 16) = make_uint4(0u, 0u, 0u, 0u);
    }
}

// A wave owns whole chunks.  Per chunk a lane walks its 16 float4 of x (element 256 t + 4 l + q, the
// next group loaded while the current one is encoded) and forms each dense value as k_ew_code does:
// the same functor and draws, apply4 on whole aligned groups, the element path on a misaligned row
// and on the group that crosses d; nothing at or past d is read.  The listed elements of step t get
// their places from four ballots (one per q): the entries of lower lanes, then the lane's own lower
// q, behind the chunk's running fill — ascending index order.  lev_code (and its `bad` counter) runs
// for listed elements only: it returns 0 for +0 and sign | 0 for -0 without counting.  Then the
// chunk's count and its two staged runs go to the workspace, coalesced 32-bit words.
template <class Op, bool VEC>
__global__ __launch_bounds__(256) void k_slev_stage(const float* __restrict__ x, int64_t d, Op op,
                                                    const float* __restrict__ levels, int s, CodeArgs ca) {
    extern __shared__ __attribute__((aligned(16))) float4 smem_tab[];
    __shared__ uint32_t st_idx[4][CHUNK / 2];          // u16 entries
    __shared__ uint32_t st_code[4][CHUNK / 4];         // u8 entries
    if (Op::TABLE) op.set_table_ok(load_table(levels, s, smem_tab));
    op.setup(0);
    PayloadHeader* h = reinterpret_cast<PayloadHeader*>(ca.payload);
    const float norm = ca.pn ? *ca.pn : 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) h->norm = norm;
    auto ld4 = [&](int64_t j) -> float4 {
        if (VEC && j + 3 < d) return *reinterpret_cast<const float4*>(x + j);
        return make_float4(j < d ? x[j] : 0.f, j + 1 < d ? x[j + 1] : 0.f, j + 2 < d ? x[j + 2] : 0.f,
                           j + 3 < d ? x[j + 3] : 0.f);
    };
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint16_t* si = reinterpret_cast<uint16_t*>(st_idx[wv]);
    uint8_t* sc = reinterpret_cast<uint8_t*>(st_code[wv]);
    const int64_t C = (d + CHUNK - 1) / CHUNK;
    for (int64_t c = (int64_t)blockIdx.x * 4 + wv; c < C; c += (int64_t)gridDim.x * 4) {
        const int64_t j0 = c * CHUNK + 4 * lane;
        uint32_t fill = 0;                              // wave-uniform: entries staged so far
        float4 nxt = ld4(j0);
#pragma unroll 1
        for (int t = 0; t < CHUNK / 256; ++t) {
            const int64_t j = j0 + 256 * t;
            const float4 v = nxt;
            if (t < CHUNK / 256 - 1) nxt = ld4(j + 256);
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            if (VEC && j + 3 < d) {
                uint32_t cs[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) cs[q] = op.col(j + q);
                const float4 r = op.row_fast() ? apply4<true>(op, v, j, cs, smem_tab) : apply4<false>(op, v, j, cs, smem_tab);
                e[0] = r.x; e[1] = r.y; e[2] = r.z; e[3] = r.w;
            } else {
                const float xe[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (j + q < d) e[q] = op.template apply<false>(xe[q], j + q, op.col(j + q), smem_tab);
            }
            uint32_t pos = fill;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t m = __ballot((__float_as_uint(e[q]) << 1) != 0u);
                pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                fill += (uint32_t)__builtin_popcountll(m);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if ((__float_as_uint(e[q]) << 1) != 0u) {
                    si[pos] = (uint16_t)(256 * t + 4 * lane + q);
                    sc[pos] = (uint8_t)lev_code(e[q], ca.lv, ca.s, norm, 0x80u, &h->bad);
                    ++pos;
                }
        }
        wave_lds_fence();
        if (lane == 0) ca.sl_cnt[c] = fill;
        u32a* gi = reinterpret_cast<u32a*>(ca.sl_idx + c * CHUNK);
        u32a* gc = reinterpret_cast<u32a*>(ca.sl_code + c * CHUNK);
        const u32a* li = reinterpret_cast<const u32a*>(st_idx[wv]);
        const u32a* lc = reinterpret_cast<const u32a*>(st_code[wv]);
        for (uint32_t i = lane; i < (fill + 1) / 2; i += 64) gi[i] = li[i];
        for (uint32_t i = lane; i < (fill + 3) / 4; i += 64) gc[i] = lc[i];
        wave_lds_fence();
    }
}

template <class Op>
int launch_code_slev(const float* x, int64_t d, Op op, const float* levels, int s, const CodeArgs& ca, hipStream_t st) {
    if (d == 0) return FLC_OK;
    const bool vec = ((uintptr_t)x & 15u) == 0;
    const size_t lds = (size_t)s * sizeof(float4);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((slev_chunks(d) + 3) / 4, 4096));
    ProfScope _ps("k_slev_stage", st);
    if (vec) hipLaunchKernelGGL((k_slev_stage<Op, true>), dim3(grid), dim3(256), lds, st, x, d, op, levels, s, ca);
    else hipLaunchKernelGGL((k_slev_stage<Op, false>), dim3(grid), dim3(256), lds, st, x, d, op, levels, s, ca);
    FLC_CHECK_LAUNCH("k_slev_stage");
    return FLC_OK;
}
template int launch_code_slev(const float*, int64_t, DitherOp<false, true>, const float*, int, const CodeArgs&, hipStream_t);
template int launch_code_slev(const float*, int64_t, DitherOp<false, false>, const float*, int, const CodeArgs&, hipStream_t);

// One workgroup: the exclusive scan of cnt[0..C) straight into the message's tab (tab[C] = nnz),
// then the zero padding of the three blocks, whose places only nnz settles.
__global__ __launch_bounds__(1024) void k_slev_scan(const uint32_t* __restrict__ cnt, int64_t C, char* __restrict__ payload) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t total;
    uint32_t* tab = reinterpret_cast<uint32_t*>(payload + 16);
    const int tid = threadIdx.x;
    const int64_t per = (C + 1023) / 1024, q0 = min<int64_t>(C, tid * per), q1 = min<int64_t>(C, q0 + per);
    uint32_t loc = 0;
    for (int64_t q = q0; q < q1; ++q) loc += cnt[q];
    uint32_t incl = loc;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o, WAVE);
        if ((tid & 63) >= o) incl += u;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    uint32_t run = incl - loc;
    for (int w = 0; w < (tid >> 6); ++w) run += wsum[w];
    for (int64_t q = q0; q < q1; ++q) { tab[q] = run; run += cnt[q]; }
    if (tid == 1023) { tab[C] = run; total = run; }
    __syncthreads();
    const int64_t nnz = total, tb = 4 * (C + 1), io = 16 + a16(tb), co = io + a16(2 * nnz);
    if (tid < 4 && tb + 4 * tid < a16(tb)) tab[C + 1 + tid] = 0u;
    if (tid >= 64 && tid < 72 && 2 * nnz + 2 * (tid - 64) < a16(2 * nnz))
        reinterpret_cast<uint16_t*>(payload + io)[nnz + (tid - 64)] = 0;
    if (tid >= 128 && tid < 144 && nnz + (tid - 128) < a16(nnz))
        reinterpret_cast<uint8_t*>(payload + co)[nnz + (tid - 128)] = 0;
}

// Every chunk's staged run to idx + tab[c] / code + tab[c]: the offsets have arbitrary 2-byte /
// 1-byte alignment, so plain element stores, coalesced across the lanes of the chunk's wave.
__global__ __launch_bounds__(256) void k_slev_gather(const uint32_t* __restrict__ cnt, const uint16_t* __restrict__ sidx,
                                                     const uint8_t* __restrict__ scode, int64_t C, char* __restrict__ payload) {
    const uint32_t* tab = reinterpret_cast<const uint32_t*>(payload + 16);
    const int lane = threadIdx.x & 63;
    const int64_t nnz = tab[C], io = 16 + a16(4 * (C + 1));
    uint16_t* idx = reinterpret_cast<uint16_t*>(payload + io);
    uint8_t* code = reinterpret_cast<uint8_t*>(payload + io + a16(2 * nnz));
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < C; c += (int64_t)gridDim.x * 4) {
        const uint32_t m = min(cnt[c], (uint32_t)CHUNK);
        const int64_t off = tab[c];
        for (uint32_t e = lane; e < m; e += 64) {
            idx[off + e] = sidx[c * CHUNK + e];
            code[off + e] = scode[c * CHUNK + e];
        }
    }
}

// ---- decode ----------------------------------------------------------------------------------------
// What the decode kernels take from one message for chunk c, clamped so that nothing outside the
// message's capacity is addressed: its entries are [lo, lo + cnt) of the idx / code planes, the code
// plane at byte coff.  tab words out of order, or past nnz, give an empty or shortened range.
struct SlevRow {
    uint32_t lo, cnt;
    int64_t coff;
};
__device__ inline SlevRow slev_row(uint32_t t0, uint32_t t1, uint32_t tC, int64_t d, int64_t io) {
    const uint32_t nn = (uint32_t)min<int64_t>(tC, d);
    SlevRow r;
    r.lo = min(t0, nn);
    r.cnt = min(max(t1, r.lo), nn) - r.lo;
    r.coff = io + a16(2 * (int64_t)nn);
    return r;
}

// the level table as 128 floats, entry i = levels[min(i, s)]: any 7-bit level index is inside it and
// one past s (only a malformed message has one) reads the top level, as lev_decode's clamp does
__device__ inline void slev_levels(const float* __restrict__ levels, int s, float* lvs) {
    for (int i = threadIdx.x; i < 128; i += blockDim.x) lvs[i] = levels[min(i, s)];
}

__device__ inline void slev_tile_zero(float* tile, int lane) {
#pragma unroll
    for (int k = 0; k < CHUNK / 256; ++k) reinterpret_cast<float4*>(tile)[k * 64 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// the tile to the row: tile / wt (DIV), float4 stores, the elements below d only in the last chunk
template <bool DIV>
__device__ inline void slev_tile_out(const float* tile, float* __restrict__ out, int64_t c, int64_t d, float wt, int lane) {
    const int64_t j0 = c * CHUNK;
    if (j0 + CHUNK <= d && ((uintptr_t)out & 15u) == 0) {
#pragma unroll 4
        for (int k = 0; k < CHUNK / 256; ++k) {
            float4 v = reinterpret_cast<const float4*>(tile)[k * 64 + lane];
            if (DIV) v = make_float4(v.x / wt, v.y / wt, v.z / wt, v.w / wt);
            reinterpret_cast<float4*>(out + j0)[k * 64 + lane] = v;
        }
    } else {
        const int64_t len = min<int64_t>(CHUNK, d - j0);
        for (int64_t i = lane; i < len; i += 64) out[j0 + i] = DIV ? tile[i] / wt : tile[i];
    }
}

// One message to a dense row: a one-wave workgroup per chunk writes the chunk's +0 background and
// its entries into an LDS tile, then the tile.  The format and s come from the codec, never from
// the message (flc_payload_validate_slev reports a header that lies).
__global__ __launch_bounds__(64) void k_unpack_slev(const char* __restrict__ payload, int64_t d,
                                                    const float* __restrict__ levels, int s, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[CHUNK];
    __shared__ float lvs[128];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x, C = (d + CHUNK - 1) / CHUNK, io = 16 + a16(4 * (C + 1));
    slev_levels(levels, s, lvs);
    slev_tile_zero(tile, lane);
    const uint32_t* tab = reinterpret_cast<const uint32_t*>(payload + 16);
    const SlevRow r = slev_row(sload(tab + c), sload(tab + c + 1), sload(tab + C), d, io);
    const float norm = sload(reinterpret_cast<const float*>(payload + 8));
    const uint16_t* idx = reinterpret_cast<const uint16_t*>(payload + io) + r.lo;
    const uint8_t* code = reinterpret_cast<const uint8_t*>(payload + r.coff) + r.lo;
    wave_lds_fence();
    for (uint32_t e = lane; e < r.cnt; e += 64)
        tile[idx[e] & (CHUNK - 1)] = lev_decode(code[e], lvs, 127, norm, 0x80u);
    wave_lds_fence();
    slev_tile_out<false>(tile, out, c, d, 1.f, lane);
}

// Server fold, chunk owner (k_chunk_accum's shape): a one-wave workgroup owns chunk c as a 4096-float
// LDS tile started at +0 (16.5 KB with the level table: nine workgroups on a CU) and walks the rows
// in order.  Rows come in batches of 64: lane r of the wave loads row r's pointer, its three tab
// words, norm and weight one batch ahead, and the row loop takes them with v_readlane.  The first
// 128 entries of PF rows (u16 idx, u8 code per lane, two halves) are in flight in a register ring;
// a longer list folds its tail in place.  Per entry: v = lev_decode(code), t = w_q * v,
// tile[idx] = tile[idx] + t.  The per-element order is the sequential fold's, so a nonzero sum has
// the dense fold's bits; an element no row lists stays +0 (the dense fold: the sum of its signed
// zeros).  n == 0 stores zeros.
struct SlevMeta {                    // lane r: row i0 + r of the batch
    uint32_t plo, phi, lo, cnt, clo, chi;
    float norm, w;
};

template <bool W, int PF>
__global__ __launch_bounds__(64) void k_unpack_slev_accum(const char* __restrict__ base, int64_t ld,
                                                          const char* const* __restrict__ ptrs, int64_t n, int64_t d,
                                                          const float* __restrict__ levels, int s,
                                                          const float* __restrict__ w, float wt, float* __restrict__ out) {
    static_assert(64 % PF == 0, "the ring divides a batch");
    __shared__ __attribute__((aligned(16))) float tile[CHUNK];
    __shared__ float lvs[128];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x, C = (d + CHUNK - 1) / CHUNK, io = 16 + a16(4 * (C + 1));
    slev_levels(levels, s, lvs);
    slev_tile_zero(tile, lane);
    wave_lds_fence();
    auto meta = [&](int64_t row) -> SlevMeta {
        SlevMeta m{0u, 0u, 0u, 0u, 0u, 0u, 0.f, 1.f};
        if (row < n) {
            const char* p = base ? base + row * ld : ptrs[row];
            gptr<uint32_t> tab = (gptr<uint32_t>)(p + 16);
            const SlevRow r = slev_row(tab[c], tab[c + 1], tab[C], d, io);
            m.plo = (uint32_t)(uintptr_t)p; m.phi = (uint32_t)((uintptr_t)p >> 32);
            m.lo = r.lo; m.cnt = r.cnt;
            m.clo = (uint32_t)r.coff; m.chi = (uint32_t)((uint64_t)r.coff >> 32);
            m.norm = ((gptr<float>)(p + 8))[0];
            if (W) m.w = w[row];
        }
        return m;
    };
    auto bc = [](uint32_t v, int q) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)v, q); };
    struct Planes { gptr<uint16_t> idx; gptr<uint8_t> code; uint32_t cnt; };
    auto planes = [&](const SlevMeta& m, int q) -> Planes {
        const char* p = reinterpret_cast<const char*>(((uintptr_t)bc(m.phi, q) << 32) | bc(m.plo, q));
        const int64_t coff = (int64_t)(((uint64_t)bc(m.chi, q) << 32) | bc(m.clo, q));
        const uint32_t lo = bc(m.lo, q);
        return Planes{(gptr<uint16_t>)(p + io) + lo, (gptr<uint8_t>)(p + coff) + lo, bc(m.cnt, q)};
    };
    uint32_t ri[PF][2], rc[PF][2];
    auto fetch = [&](const SlevMeta& m, int q, int slot) {
        const Planes pl = planes(m, q);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t e = (uint32_t)lane + 64u * h;
            ri[slot][h] = e < pl.cnt ? (uint32_t)pl.idx[e] : 0u;
            rc[slot][h] = e < pl.cnt ? (uint32_t)pl.code[e] : 0u;
        }
    };
    auto add = [&](uint32_t ix, uint32_t cd, float norm, float wi) {
        const float v = lev_decode(cd, lvs, 127, norm, 0x80u);
        const uint32_t loc = ix & (CHUNK - 1);
        tile[loc] = tile[loc] + (W ? wi * v : v);
    };
    SlevMeta cur = meta(lane), nxt;
#pragma unroll
    for (int p = 0; p < PF; ++p) fetch(cur, p, p);
    for (int64_t i0 = 0; i0 < n; i0 += 64) {
        nxt = meta(i0 + 64 + lane);
        const int rows = (int)min<int64_t>(64, n - i0);
        for (int q0 = 0; q0 < rows; q0 += PF) {
#pragma unroll
            for (int p = 0; p < PF; ++p) {
                const int q = q0 + p;
                const uint32_t cnt = bc(cur.cnt, q);
                const float norm = __uint_as_float(bc(__float_as_uint(cur.norm), q));
                const float wi = W ? __uint_as_float(bc(__float_as_uint(cur.w), q)) : 1.f;
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    if ((uint32_t)lane + 64u * h < cnt) add(ri[p][h], rc[p][h], norm, wi);
                if (cnt > 128u) {                          // a list past the ring slot: its tail in place
                    const Planes pl = planes(cur, q);
                    for (uint32_t e = 128u + lane; e < cnt; e += 64) add(pl.idx[e], pl.code[e], norm, wi);
                }
                wave_lds_fence();
                if (q + PF < 64) fetch(cur, q + PF, p);
                else fetch(nxt, q + PF - 64, p);           // past n: empty lists
            }
        }
        cur = nxt;
    }
    wave_lds_fence();
    if (n == 0) slev_tile_out<false>(tile, out, c, d, 1.f, lane);
    else slev_tile_out<true>(tile, out, c, d, wt, lane);
}

// ---- host ------------------------------------------------------------------------------------------
static int slev_refuse(const flc_codec_params* prm, const char* me) {
    if (slev_ok(prm)) return FLC_OK;
    set_error("%s: codec %d%s has no sparse level form (standard dithering / qsgd / terngrad with s <= 127)", me,
              prm->codec, prm->codec == FLC_STD_DITHERING ? " with s > 127" : "");
    return FLC_ERR_UNSUPPORTED;
}

static int slev_dim(int64_t d, const char* me) {
    if (d <= 0xFFFFFFFFll) return FLC_OK;
    set_error("%s: d=%lld does not fit the header's 32-bit count", me, (long long)d);
    return FLC_ERR_ARG;
}

struct SlevWs {
    float* pnorm;
    uint32_t* cnt;
    uint16_t* sidx;
    uint8_t* scode;
    void* inner;
    size_t inner_bytes;
};
static SlevWs carve_slev(void* base, const flc_codec_params* prm, int64_t d, size_t* bytes) {
    Carver c(base);
    SlevWs w;
    const size_t C = (size_t)std::max<int64_t>(slev_chunks(d), 1);
    w.pnorm = c.take<float>(1);
    w.cnt = c.take<uint32_t>(C);
    w.sidx = c.take<uint16_t>(C * CHUNK);
    w.scode = c.take<uint8_t>(C * CHUNK);
    w.inner_bytes = ew_workspace(prm, 1, d);
    w.inner = c.take<char>(w.inner_bytes);
    if (bytes) *bytes = c.bytes();
    return w;
}

size_t slev_pack_workspace(const flc_codec_params* prm, int64_t d) {
    if (!slev_ok(prm)) return 0;
    size_t b = 0;
    carve_slev(nullptr, prm, d, &b);
    return b;
}

int slev_pack_run(const flc_codec_params* prm, const flc_pattern* pat, const float* x, int64_t d, char* payload, void* ws,
                  size_t ws_bytes, hipStream_t st) {
    const char* me = "flc_pack_slev";
    if (int rc = slev_refuse(prm, me)) return rc;
    if (int rc = check_dither(prm)) return rc;
    if (int rc = slev_dim(d, me)) return rc;
    if (ws_bytes < slev_pack_workspace(prm, d)) { set_error("%s: workspace too small", me); return FLC_ERR_WORKSPACE; }
    if ((uintptr_t)payload & 15u) { set_error("%s: payload must be 16-byte aligned", me); return FLC_ERR_ARG; }
    SlevWs w = carve_slev(ws, prm, d, nullptr);
    hipLaunchKernelGGL(k_slev_header, dim3(1), dim3(64), 0, st, payload, (uint32_t)d);
    FLC_CHECK_LAUNCH("k_slev_header");
    if (d == 0) return FLC_OK;
    // the norm pass, then ONE pass from x to the staged lists (codecs.hip ew_run -> k_slev_stage)
    CodeArgs ca{0, payload, prm->d_levels, prm->s, w.pnorm, 0, w.cnt, w.sidx, w.scode};
    RowSrc src{x, d, nullptr};
    if (int rc = ew_run(prm, pat, src, ((uintptr_t)x & 15u) == 0, 1, d, nullptr, w.pnorm, /*dense=*/true, nullptr, nullptr,
                        1.f, w.inner, w.inner_bytes, st, nullptr, &ca))
        return rc;
    const int64_t C = slev_chunks(d);
    hipLaunchKernelGGL(k_slev_scan, dim3(1), dim3(1024), 0, st, w.cnt, C, payload);
    FLC_CHECK_LAUNCH("k_slev_scan");
    const int grid = (int)std::min<int64_t>((C + 3) / 4, 4096);
    hipLaunchKernelGGL(k_slev_gather, dim3(grid), dim3(256), 0, st, w.cnt, w.sidx, w.scode, C, payload);
    FLC_CHECK_LAUNCH("k_slev_gather");
    return FLC_OK;
}

static int slev_decode_check(const flc_codec_params* prm, int64_t d, const char* me) {
    if (int rc = slev_refuse(prm, me)) return rc;
    if (!prm->d_levels) { set_error("%s: dithering needs the level table", me); return FLC_ERR_ARG; }
    return slev_dim(d, me);
}

int slev_unpack_run(const flc_codec_params* prm, const char* payload, int64_t d, float* out, hipStream_t st) {
    const char* me = "flc_unpack_slev";
    if (int rc = slev_decode_check(prm, d, me)) return rc;
    if (d == 0) return FLC_OK;
    if ((uintptr_t)payload & 15u) { set_error("%s: payload must be 16-byte aligned", me); return FLC_ERR_ARG; }
    hipLaunchKernelGGL(k_unpack_slev, dim3((unsigned)slev_chunks(d)), dim3(64), 0, st, payload, d, prm->d_levels, prm->s, out);
    FLC_CHECK_LAUNCH("k_unpack_slev");
    return FLC_OK;
}

#ifndef FLC_SLEV_PF
#define FLC_SLEV_PF 4
#endif
int slev_unpack_reduce_run(const flc_codec_params* prm, const char* base, int64_t ld, const char* const* ptrs, int64_t n,
                           int64_t d, const float* w, float wt, float* out, hipStream_t st) {
    const char* me = "flc_unpack_reduce_slev";
    if (int rc = slev_decode_check(prm, d, me)) return rc;
    if (base && ((ld & 15) || ((uintptr_t)base & 15u))) { set_error("%s: payload rows must be 16-byte aligned", me); return FLC_ERR_ARG; }
    if (d == 0) return FLC_OK;
    const unsigned grid = (unsigned)slev_chunks(d);
    ProfScope _ps("k_unpack_slev_accum", st);
    if (w) hipLaunchKernelGGL((k_unpack_slev_accum<true, FLC_SLEV_PF>), dim3(grid), dim3(64), 0, st, base, ld, ptrs, n, d,
                              prm->d_levels, prm->s, w, wt, out);
    else hipLaunchKernelGGL((k_unpack_slev_accum<false, FLC_SLEV_PF>), dim3(grid), dim3(64), 0, st, base, ld, ptrs, n, d,
                            prm->d_levels, prm->s, w, wt, out);
    FLC_CHECK_LAUNCH("k_unpack_slev_accum");
    return FLC_OK;
}

// The used size of a host message from tab[C] alone (flc_payload_slev_used); 0 when nbytes does not
// reach tab[C] or tab[C] > d.
int64_t slev_payload_used(const uint8_t* p, int64_t nbytes, int64_t d) {
    const int64_t C = slev_chunks(d);
    if (!p || nbytes < 16 + 4 * (C + 1)) return 0;
    uint32_t nnz;
    std::memcpy(&nnz, p + 16 + 4 * C, 4);
    return (int64_t)nnz > d ? 0 : slev_used_bytes(d, nnz);
}

// Host check of one sparse level message off the network (flc_payload_validate_slev): everything
// the decode kernels take from the message itself.
int slev_payload_validate(const flc_codec_params* prm, const uint8_t* p, int64_t nbytes, int64_t d) {
    if (int rc = slev_refuse(prm, "flc_payload_validate_slev")) return rc;
    if (int rc = slev_dim(d, "flc_payload_validate_slev")) return rc;
    const int64_t C = slev_chunks(d), io = slev_idx_off(d);
    if (nbytes < io) { set_error("payload: %lld bytes, header and chunk table of d=%lld are %lld", (long long)nbytes, (long long)d, (long long)io); return FLC_ERR_ARG; }
    PayloadHeader h;
    std::memcpy(&h, p, sizeof h);
    if (h.fmt != (uint32_t)FMT_SLEV) { set_error("payload: header format %u, the sparse level format is %d", h.fmt, FMT_SLEV); return FLC_ERR_ARG; }
    if (h.count != (uint32_t)d) { set_error("payload: count %u != d", h.count); return FLC_ERR_ARG; }
    if (h.bad != 0u) { set_error("payload: %u elements flagged unrepresentable by the sender", h.bad); return FLC_ERR_ARG; }
    auto tab = [&](int64_t c) { uint32_t v; std::memcpy(&v, p + 16 + 4 * c, 4); return v; };
    const int64_t nnz = tab(C);
    if (nnz > d) { set_error("payload: %lld entries, d=%lld", (long long)nnz, (long long)d); return FLC_ERR_ARG; }
    const int64_t used = slev_used_bytes(d, nnz);
    if (nbytes < used) { set_error("payload: %lld bytes, the message of %lld entries is %lld", (long long)nbytes, (long long)nnz, (long long)used); return FLC_ERR_ARG; }
    if (tab(0) != 0u) { set_error("payload: tab[0] = %u", tab(0)); return FLC_ERR_ARG; }
    const uint8_t* idx = p + io;
    const uint8_t* code = idx + a16(2 * nnz);
    const bool finite = std::isfinite(h.norm);
    for (int64_t c = 0; c < C; ++c) {                  // the whole table first: the planes' places hang on it
        const int64_t t0 = tab(c), t1 = tab(c + 1), len = std::min<int64_t>(CHUNK, d - c * CHUNK);
        if (t1 < t0 || t1 - t0 > len) { set_error("payload: chunk %lld holds entries [%lld, %lld), its length is %lld", (long long)c, (long long)t0, (long long)t1, (long long)len); return FLC_ERR_ARG; }
    }
    for (int64_t c = 0; c < C; ++c) {
        const int64_t t0 = tab(c), t1 = tab(c + 1), len = std::min<int64_t>(CHUNK, d - c * CHUNK);
        int64_t prev = -1;
        for (int64_t e = t0; e < t1; ++e) {
            uint16_t j;
            std::memcpy(&j, idx + 2 * e, 2);
            if ((int64_t)j >= len || (int64_t)j <= prev) { set_error("payload: entry %lld index %u not ascending in [0, %lld)", (long long)e, j, (long long)len); return FLC_ERR_ARG; }
            prev = j;
            const uint32_t lev = code[e] & 0x7Fu;
            if (lev > (uint32_t)prm->s || (lev == 0u && finite)) { set_error("payload: entry %lld level index %u outside 1..s=%d", (long long)e, lev, prm->s); return FLC_ERR_ARG; }
        }
    }
    auto zeros = [&](int64_t a, int64_t b) { for (int64_t i = a; i < b; ++i) if (p[i]) return false; return true; };
    if (!zeros(16 + 4 * (C + 1), io) || !zeros(io + 2 * nnz, io + a16(2 * nnz)) ||
        !zeros(io + a16(2 * nnz) + nnz, used)) { set_error("payload: padding bytes are not zero"); return FLC_ERR_ARG; }
    return FLC_OK;
}

}  // namespace flc
