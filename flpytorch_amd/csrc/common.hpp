// Device/host helpers shared by the flcodec translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/flcodec.h"

namespace flc {

constexpr int WAVE = 64;          // CDNA wavefront
constexpr int CHUNK = 4096;       // elements per selection chunk (one wave's tile, 16 KB fp32)
constexpr int CHUNK_SHIFT = 12;

// ------------------------------------------------------------------------------------------
// error plumbing (thread-local message, status codes of flcodec.h)
// ------------------------------------------------------------------------------------------
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define FLC_CHECK_HIP(expr)                                          \
    do {                                                             \
        hipError_t _e = (expr);                                      \
        if (_e != hipSuccess) return ::flc::hip_fail(_e, #expr);     \
    } while (0)
#define FLC_CHECK_LAUNCH(what)                                       \
    do {                                                             \
        hipError_t _e = hipGetLastError();                           \
        if (_e != hipSuccess) return ::flc::hip_fail(_e, what);      \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Layout / probe switches for A/B tuning runs.  Only a build with -DFLC_TUNING (tools/ab_build.sh
// --tuning) reads them from the environment; the product library ignores the environment, so a
// stray variable can never change a result.
// Events that only order one device's streams (hipStreamWaitEvent; never inspected by the host):
// device-scope release, no system-scope cache writeback at each record
#ifndef FLC_SYNC_EVENT_FLAGS
#define FLC_SYNC_EVENT_FLAGS (hipEventDisableTiming | hipEventDisableSystemFence)
#endif

inline const char* tuning_env(const char* name) {
#ifdef FLC_TUNING
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// Kernel timing (flc_profile_enable): a scope records a hipEvent pair around one launch.
extern bool g_prof_on;
void prof_record(const char* name, hipStream_t st, bool begin);
struct ProfScope {
    const char* name;
    hipStream_t st;
    ProfScope(const char* n, hipStream_t s) : name(n), st(s) { if (g_prof_on) prof_record(name, st, true); }
    ~ProfScope() { if (g_prof_on) prof_record(name, st, false); }
};

// Workspace carving: every sub-buffer 256-byte aligned.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base(static_cast<char*>(b)) {}
    template <class T>
    T* take(size_t count) {
        off = align_up(off, 256);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return align_up(off, 256); }
};

// Row addressing shared by every kernel: a strided matrix (row i at base + i*ld) or a device
// array of row pointers (base == nullptr).
// Scalar (constant address space) load of a wave-uniform address: the data must not change
// during the kernel (written by earlier launches only).
template <class T>
__device__ inline T sload(const T* p) {
    return *(const __attribute__((address_space(4))) T*)p;
}

#ifndef FLC_ROWNT
#define FLC_ROWNT 1
#endif
// One float4 of a client row in a streaming pass (read once per launch): a nontemporal load
// (measured: the serverGradient fold 2-4 % faster, the dense norm pass 10 %; -DFLC_ROWNT=0 for A/B)
__device__ inline float4 ld_row4(const float4* p) {
#if FLC_ROWNT
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}

struct RowSrc {
    const float* base;
    int64_t ld;
    const float* const* ptrs;
    __device__ inline const float* row(int64_t i) const { return base ? base + i * ld : ptrs[i]; }
    // wave-uniform i: the pointer table is read through the scalar cache (s_load, lgkmcnt), so it
    // does not join the vector-memory queue of a streaming pipeline
    __device__ inline const float* row_s(int64_t i) const {
        return base ? base + i * ld : sload(ptrs + i);
    }
};

// Partial participation (the _sampled entries, flc_row_map): participant i of a round is client
// ids[i] of n_total resident ones.  The kernels of the shifted rounds take the mapping as a template
// argument: MapNone is the contiguous round (participant i is row i and client client0 + i, nothing
// is loaded), MapIds reads the id.  id_s / at_s: a wave-uniform i, read through the scalar cache like
// RowSrc::row_s; at / at_s: the row of an operand whose FLC_IDX_ bit is `bit`.
struct MapNone {
    static constexpr bool ON = false;
    __device__ inline bool has(uint32_t) const { return false; }
    __device__ inline int64_t id(int64_t i) const { return i; }
    __device__ inline int64_t id_s(int64_t i) const { return i; }
    __device__ inline int32_t raw_s(int64_t i) const { return (int32_t)i; }
    __device__ inline int64_t at(int64_t i, uint32_t) const { return i; }
    __device__ inline int64_t at_s(int64_t i, uint32_t) const { return i; }
};
struct MapIds {
    static constexpr bool ON = true;
    const int32_t* ids;
    uint32_t indexed;
    __device__ inline bool has(uint32_t bit) const { return (indexed & bit) != 0; }
    __device__ inline int64_t id(int64_t i) const { return ids[i]; }
    __device__ inline int64_t id_s(int64_t i) const { return sload(ids + i); }
    __device__ inline int32_t raw_s(int64_t i) const { return sload(ids + i); }
    __device__ inline int64_t at(int64_t i, uint32_t bit) const { return (indexed & bit) ? (int64_t)ids[i] : i; }
    __device__ inline int64_t at_s(int64_t i, uint32_t bit) const { return (indexed & bit) ? (int64_t)sload(ids + i) : i; }
};
inline MapIds map_ids(const flc_row_map* map) { return MapIds{map->d_ids, map->indexed}; }
inline bool map_has(const flc_row_map* map, uint32_t bit) { return map && (map->indexed & bit); }
// device array tab[i] = base + at(i) * ld (the rows of an indexed operand as a RowSrc pointer table)
int row_ptrs_launch(const float* base, int64_t ld, const flc_row_map* map, int64_t n, const float** tab, hipStream_t st);

// Internal entry points of the codec families (reduce.hip, codecs.hip, the selection core:
// select.hip with topk_filter.hip, topk_select.hip, lone_row.hip, randk.hip and chunk_accum.hip).
int reduce_impl(RowSrc src, bool rows_vec_ok, int64_t n, int64_t d, const float* x, const float* w, float wt,
                int mode, float* out, hipStream_t st);
// norms_given / norm_mode: flc_encode_reduce_ex's selectors (0, FLC_NORMMODE_EXACT: flc_encode_reduce)
size_t ew_workspace(const flc_codec_params* prm, int64_t n, int64_t d, bool norms_given = false,
                    int norm_mode = FLC_NORMMODE_EXACT);
// The shift codecs' epilogue (flc_encode_shift): b is subtracted from the input row before the
// codec; msg = base + C * scale, hout = hin + alpha * C (null msg / hout: not written).
struct ShiftArgs {
    const float* b;
    float scale;
    const float* base;
    float* msg;
    float alpha;
    const float* hin;
    float* hout;
};
// flc_pack's fused encode -> code form (Q8 / Q16 / NAT16): payload header + body written directly.
// Together with ShiftArgs (flc_pack_shift, k_ew_shift_code) the F32 format is taken too: e itself.
struct CodeArgs {
    int fmt;
    char* payload;
    const float* lv;     // the level table (dithering)
    int s;
    const float* pn;     // device norm the codes are relative to (dithering)
};
int ew_run(const flc_codec_params* prm, const flc_pattern* pat, RowSrc src, bool vec, int64_t n, int64_t d,
           const float* pnorm_in, float* pnorm_out, bool dense, float* out, const float* w, float wt, void* ws,
           size_t ws_bytes, hipStream_t st, const ShiftArgs* sh = nullptr, const CodeArgs* ca = nullptr,
           int norm_mode = FLC_NORMMODE_EXACT, const flc_shift_rows* sr = nullptr, const flc_row_map* map = nullptr);
// the dithering codecs' parameter check (s, levels, p-norm), before any launch
int check_dither(const flc_codec_params* prm);
size_t ew_shift_reduce_workspace(const flc_codec_params* prm, int64_t n, int64_t d);
size_t shift_workspace(const flc_codec_params* prm, int64_t d);
// the shifted fold over n rows (flc_encode_shift_reduce): the elementwise codecs in one tile-owner
// pass (codecs.hip k_ew_shift_accum), RandK / TopK / Rank-K row by row (shift.hip)
size_t shift_reduce_workspace(const flc_codec_params* prm, int64_t n, int64_t d);
int shift_reduce_run(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows& sr, int64_t n, int64_t d,
                     const float* w, float wt, float* pnorms_out, float* out, void* ws, size_t ws_bytes, hipStream_t st,
                     const flc_row_map* map = nullptr);
// FRECON's two-message round (flc_frecon_reduce, codecs.hip k_ew_frecon_accum): elementwise codecs
// only; frecon_precheck is the codec's host-side parameter / pattern check, before any launch
bool frecon_elementwise(int codec);
size_t frecon_workspace(const flc_codec_params* prm, int64_t n, int64_t d);
int frecon_precheck(const flc_codec_params* prm, const flc_pattern* pat);
int frecon_run(const flc_codec_params* prm, const flc_pattern* pat, const flc_frecon_rows& fr, int64_t n, int64_t d,
               const float* w, float wt, float* pnorms_u_out, float* pnorms_q_out, float* u_out, float* q_out,
               const flc_frecon_server* srv, void* ws, size_t ws_bytes, hipStream_t st);
int encode_row(const flc_codec_params* prm, const flc_pattern* pat, const float* d_x, int64_t d,
               const float* d_pnorm_in, float* d_pnorm_out, float* d_out, void* d_ws, size_t ws_bytes, hipStream_t st);
size_t encode_row_workspace(const flc_codec_params* prm, int64_t d);
int sel_unpack_reduce(const flc_codec_params* prm, const void* base, int64_t ld_bytes, const void* const* ptrs,
                      int64_t n, int64_t d, const float* w, float wt, float* out, void* wsp, size_t ws_bytes,
                      hipStream_t st);
size_t sel_unpack_workspace(const flc_codec_params* prm, int64_t n, int64_t d);
int64_t payload_bytes(const flc_codec_params* prm, int64_t d);
int64_t rk_payload_floats(const flc_codec_params* prm, int64_t d);
int64_t rk_rank(const flc_codec_params* prm, int64_t d);
int rk_pack(const flc_codec_params* prm, const float* x, int64_t d, float* body, void* wsp, size_t ws_bytes,
            hipStream_t st);
size_t rk_unpack_workspace(const flc_codec_params* prm, int64_t n, int64_t d);
int rk_unpack1(const flc_codec_params* prm, const float* body, int64_t d, float* out, hipStream_t st);
int rk_unpack_reduce(const flc_codec_params* prm, const char* base, int64_t ld, const char* const* ptrs, int64_t n,
                     int64_t d, const float* w, float wt, float* out, bool reduce, void* wsp, size_t ws_bytes,
                     hipStream_t st);
int payload_format(const flc_codec_params* prm);
int payload_validate(const flc_codec_params* prm, const uint8_t* p, int64_t nbytes, int64_t d);
size_t pack_workspace(const flc_codec_params* prm, int64_t d);
int pack_run(const flc_codec_params* prm, const flc_pattern* pat, const float* x, int64_t d, char* payload, void* ws,
             size_t ws_bytes, hipStream_t st);
int unpack_run(const flc_codec_params* prm, const char* payload, int64_t d, float* out, hipStream_t st);
size_t unpack_reduce_workspace(const flc_codec_params* prm, int64_t n, int64_t d);
int unpack_reduce_run(const flc_codec_params* prm, const char* base, int64_t ld, const char* const* ptrs, int64_t n,
                      int64_t d, const float* w, float wt, float* out, void* ws, size_t ws_bytes, hipStream_t st);
int shift_run(const flc_codec_params* prm, const flc_pattern* pat, const float* a, int64_t d, const ShiftArgs& sh,
              float* pnorm_out, void* ws, size_t ws_bytes, hipStream_t st);
// RandK / TopK / Rank-K: the dense row e = C(a - b) formed in the workspace (shift_workspace bytes),
// the first half of shift_run; then its epilogue over a stored e and one step of the row-order fold
int shift_encode_dense(const flc_codec_params* prm, const flc_pattern* pat, const float* a, const float* b, int64_t d,
                       float** e_out, void* ws, size_t ws_bytes, hipStream_t st);
int shift_epi_launch(const float* e, int64_t d, const ShiftArgs& sh, hipStream_t st);
int shift_fold_launch(const float* m, int64_t d, const float* w, int64_t i, bool last, float wt, float* acc,
                      hipStream_t st);
// What the sparse rounds (flc_randk / topk / dither_shift_reduce) share on the host (shift.hip).
// shift_shape: the accepted shape of a round (the table in flcodec.h), recognised by pointer and
// leading dimension, or -1 with the reason set under the entry's name `me`; sr is api.hip's
// normalised copy.  The values are template arguments of the rounds' kernels.
enum { SHAPE_D = 0, SHAPE_A = 1, SHAPE_C = 2, SHAPE_B = 3 };
int shift_shape(const flc_shift_rows& sr, const char* me);
// the in-place shapes (A, B) store into the b rows: they must not overlap
int inplace_rows_check(const char* me, int shape, const flc_shift_rows& sr, int64_t n, int64_t d);
// the sampled rounds' extra workspace (the pointer table of shape B's fold over the mapped rows)
size_t sampled_tab_bytes(int64_t n);
// a round over (index, value) lists: K in [1, D], D within 32-bit entry indices, then inplace_rows_check
int sparse_round_precheck(const char* me, int shape, const flc_shift_rows& sr, int64_t n, int64_t d, int64_t K);
// shape B's tail: the dense fold of the rows the round has just updated in place
// (map with FLC_IDX_B: over the participants' rows, through the pointer table tab[n] built here)
int fold_updated_rows(const flc_shift_rows& sr, int64_t n, int64_t d, const float* w, float wt, float* out, hipStream_t st,
                      const flc_row_map* map = nullptr, const float** tab = nullptr);
// the SPARSE payload of a dense row (wire.hip k_pack_count / scan / write): bc holds pack_blocks(d)
// counters, the payload is zeroed by the caller
int64_t pack_blocks(int64_t d);
int pack_sparse_launch(const float* dense, int64_t d, int64_t cap, uint32_t* bc, char* payload, hipStream_t st);
// shifted steps on the wire (wire_shift.hip): flc_pack_shift / flc_unpack_shift_reduce
size_t pack_shift_workspace(const flc_codec_params* prm, int64_t d);
int pack_shift_run(const flc_codec_params* prm, const flc_pattern* pat, const float* a, int64_t d, const ShiftArgs& sh,
                   char* payload, void* ws, size_t ws_bytes, hipStream_t st);
size_t unpack_shift_reduce_workspace(const flc_codec_params* prm, int64_t n, int64_t d);
int unpack_shift_reduce_run(const flc_codec_params* prm, const flc_payload_rows& pr, int64_t n, int64_t d,
                            const float* w, float wt, float* out, void* ws, size_t ws_bytes, hipStream_t st);
// Row g's boundary of G row groups whose last group is `lastpct` % of the others' size (the last
// group's tail is the exposed one): rows [group_row(n, G, g), group_row(n, G, g + 1)).
// lastpct is clamped to [1, 100]: 0 or less would leave the last group (the one whose fold writes
// the output) empty, above 100 is the even split.
inline int64_t group_row(int64_t n, int G, int g, int lastpct) {
    lastpct = lastpct < 1 ? 1 : lastpct;
    if (G <= 1 || lastpct >= 100) return n * g / G;
    const int64_t unit = 100 * (int64_t)(G - 1) + lastpct;     // group sizes 100, ..., 100, lastpct
    const int64_t cum = g <= G - 1 ? 100 * (int64_t)g : unit;
    return n * cum / unit;
}
int norm_torch_run(const float* x, int64_t ld, int64_t n, int64_t d, float* out, hipStream_t st);
size_t norm_torch_ws_bytes(int64_t n, int64_t d);
int norm_torch_ws_run(const float* x, int64_t ld, int64_t n, int64_t d, float* out, void* wsp, size_t ws_bytes,
                      hipStream_t st);
int tn_run(RowSrc rows, int64_t n, int64_t r0, int64_t rn, int64_t d, float* out, void* wsp, const double* item_sums,
           int64_t G, hipStream_t st);
size_t sel_workspace(const flc_codec_params* prm, int64_t n, int64_t d);
int sel_run(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, bool vec, int64_t n, int64_t d,
            bool assign, const float* w, float wt, float* out, void* wsp, size_t ws_bytes, hipStream_t st);
int rs_debug(int mult, int64_t spin_ticks);
int sel_row_flags(const flc_codec_params* prm, int64_t n, int64_t d, const void* wsp, size_t ws_bytes,
                  uint32_t* flags, hipStream_t st);
bool ds_eligible(const flc_codec_params* prm, const flc_pattern* pat, int64_t n, int64_t d);
size_t ds_workspace(const flc_codec_params* prm, int64_t n, int64_t d, int norm_mode = FLC_NORMMODE_EXACT);
int ds_run(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, int64_t n, int64_t d, const float* w,
           float wt, float* pnorm_out, float* out, void* wsp, size_t ws_bytes, hipStream_t st,
           const float* pnorm_in = nullptr, int norm_mode = FLC_NORMMODE_EXACT);
size_t rk_workspace(const flc_codec_params* prm, int64_t n, int64_t d, bool reduce);
int rk_run(const flc_codec_params* prm, RowSrc rows, int64_t n, int64_t d, bool reduce, const float* w, float wt,
           float* out, void* wsp, size_t ws_bytes, hipStream_t st);
size_t randk_device_workspace(int64_t n, int64_t d);
int randk_device_counts(uint64_t seed, int64_t client0, int64_t n, int64_t d, int64_t k, uint32_t* cnt, void* ws,
                        size_t ws_bytes, hipStream_t st);
// chunk counts [C][n] (the pattern's d_randk_counts or computed) and client keys [n] of a device-draw
// fold; wsp: randk_device_workspace(n, d) bytes
int randk_device_prepare(const flc_codec_params* prm, const flc_pattern* pat, int64_t n, int64_t d, void* wsp,
                         const uint32_t** cnt, const uint64_t** ckey, hipStream_t st, const flc_row_map* map = nullptr);
// The compat RandK lists by themselves: row r's entries of chunk c are idx / val[r * cap + tab[c * n + r].x + t],
// t < tab[c * n + r].y (element index within the row; randk_scale * rows[r][idx]).  A caller may
// rewrite val before randk_lists_fold (k_chunk_accum) folds the lists into out.
struct RkLists {
    const uint2* tab;
    const uint32_t* idx;
    float* val;
    int64_t cap;
};
size_t randk_lists_workspace(int64_t n, int64_t d, int64_t K);
int randk_lists_build(const flc_codec_params* prm, const flc_pattern* pat, RowSrc rows, int64_t n, int64_t d, void* wsp,
                      RkLists* lists, hipStream_t st);
int randk_lists_fold(int64_t n, int64_t d, int64_t K, void* wsp, const float* w, float wt, float* out, hipStream_t st);
// the sparse in-place RandK shifted round (flc_randk_shift_reduce, randk_shift.hip)
size_t randk_shift_workspace(const flc_codec_params* prm, bool compat, int64_t n, int64_t d, bool sampled = false);
int randk_shift_run(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows& sr, int64_t n, int64_t d,
                    const float* w, float wt, float* out, void* ws, size_t ws_bytes, hipStream_t st,
                    const flc_row_map* map = nullptr);
// shape C's fold of base + t over lists in the RkLists layout (k_randk_shift_lfold)
int randk_shift_lfold_launch(const float* base, int64_t n, int64_t d, RkLists lists, const float* w, float wt, float* out,
                             hipStream_t st);
// The many-row TopK selection by itself (select.hip's dispatcher up to the lists): after topk_lists_build row r's entries of chunk
// c are ent_idx / ent_val[r * cap + tab[c * n + r].x + t], t < tab[c * n + r].y, and an entry is
// admitted iff (mag_key(val), idx ^ txm) >= (T, cut) with T, cut taken from thr / flags / tiecut as
// k_chunk_accum's load_meta takes them (flag TK_F_EXACT: every entry; TK_F_TIES: the tie cut).  A
// caller may rewrite the entries and the admission state before topk_lists_fold (k_chunk_accum).
// wsp: sel_workspace(prm, n, d) bytes, the carve of flc_encode_reduce.
constexpr uint32_t TK_F_TIES = 4u, TK_F_EXACT = 8u;
struct TkLists {
    const uint2* tab;
    uint32_t* ent_idx;
    float* ent_val;
    int64_t cap;
    uint32_t* thr;
    uint32_t* flags;
    const uint32_t* tiecut;
    uint32_t tie_hi;
};
int topk_lists_build(const flc_codec_params* prm, RowSrc rows, bool vec, int64_t n, int64_t d, void* wsp, size_t ws_bytes,
                     TkLists* lists, hipStream_t st);
int topk_lists_fold(const flc_codec_params* prm, int64_t n, int64_t d, void* wsp, const float* w, float wt, float* out,
                    hipStream_t st);
// the batched TopK shifted round (flc_topk_shift_reduce, topk_shift.hip)
size_t topk_shift_workspace(const flc_codec_params* prm, int64_t n, int64_t d, bool sampled = false);
int topk_shift_run(const flc_codec_params* prm, const flc_shift_rows& sr, int64_t n, int64_t d, const float* w, float wt,
                   float* out, void* ws, size_t ws_bytes, hipStream_t st, const flc_row_map* map = nullptr);
// the one-read QSGD shifted round (flc_dither_shift_reduce): dither_shift.hip decides on the host,
// before any launch, whether the call is taken (else the refusal with its reason) and runs it;
// dither_sparse.hip's ds_shift_run is the sparse pipeline over a - b with the in-place epilogues
// (shape: SHAPE_A / SHAPE_B / SHAPE_D), ds_flags_at the DsWs.flags of a workspace
size_t dither_shift_workspace(const flc_codec_params* prm, int64_t n, int64_t d);
int dither_shift_run(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows& sr, int64_t n, int64_t d,
                     const float* w, float wt, float* pnorms_out, float* out, void* ws, size_t ws_bytes, hipStream_t st);
int dither_row_flags(int64_t n, int64_t d, const void* ws, size_t ws_bytes, uint32_t* flags, hipStream_t st);
int ds_shift_run(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows& sr, int shape, int64_t n,
                 int64_t d, const float* w, float wt, float* pnorm_out, float* out, void* wsp, size_t ws_bytes,
                 hipStream_t st);
const uint32_t* ds_flags_at(const void* wsp, int64_t n, int64_t d);
int randk_dense(const flc_codec_params* prm, const flc_pattern* pat, const float* x, int64_t d, float* out, void* ws,
                size_t ws_bytes,
                hipStream_t st);

// ------------------------------------------------------------------------------------------
// Device-RNG mode: counter-based generator, SplitMix64 finaliser over a keyed Weyl sequence.
// uniform(seed, client, j) = (mix(seed, client, j) >> 11) * 2^-53 — a 53-bit double like
// numpy's random_sample, so compat and device modes share every downstream comparison.
// ------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__host__ __device__ inline uint64_t client_key(uint64_t seed, int64_t client) {
    return mix64(seed ^ mix64(0x9E3779B97F4A7C15ull * (uint64_t)(client + 1)));
}
__host__ __device__ inline double uniform53(uint64_t ckey, int64_t j) {
    uint64_t z = mix64(ckey + 0x9E3779B97F4A7C15ull * (uint64_t)j);
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// Per-element device draw used by the dithering / natural kernels: a 32-bit uniform
// u = fmix32(j * m_c + o_c) * 2^-32, with (m_c odd, o_c) taken from the client key — one Weyl
// sequence per client through the MurmurHash3 finaliser (a bijection with full avalanche).
// 32-bit multiplies only: the 64-bit mix above costs ~3x the VALU time per element.
__host__ __device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
// u(client, j) = hi8 << 24 | lo24 from two hashes keyed by the row key rk (a 32-bit fold of the
// client key):
//   lo24 = fmix32(colbase(j) + (rk ^ 0x27D4EB2F)) >> 8,  colbase(j) = j * 0x85EBCA77 (computed
//          once per column by the tile-owner kernels, outside the client loop);
//   hi8  = byte (j & 3) of grouphash(j >> 2, rk) = gmix((j >> 2) * 0x9E3779B1 + rk) — one hash
//          serves 4 consecutive elements.
// The split lets a streaming pass decide `u >= t` for a small t from the top byte alone, at a
// quarter hash per element (the sparse QSGD candidate filter, dither_sparse.hip).  gmix is two
// rounds of xorshift + 24-bit multiply (v_mul_u32_u24, full rate; the top byte the multiply ignores
// is xored back in), instead of the MurmurHash3 finaliser's two quarter-rate 32-bit multiplies:
// same-box A/B 0.1-0.2 ms off the C4 filter; statistically checked like fmix32 (bit bias, bit-pair
// correlations at lags 0-1024, 4-byte joint, adjacent groups: tests/test_host.py).
__host__ __device__ inline uint32_t colbase(uint32_t j) { return j * 0x85EBCA77u; }
__host__ __device__ inline uint32_t rowkey(uint64_t ckey) { return (uint32_t)(ckey >> 32) ^ (uint32_t)ckey; }
#ifndef FLC_GHASH
#define FLC_GHASH 1
#endif
__host__ __device__ inline uint32_t mul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
// FLC_GHASH (A/B builds only; the draws are part of the device-RNG definition and oracle/devrng.py
// states variant 1): 0 = fmix32, 1 = the 24-bit mixer, 2 = a 32x32->64 multiply folded lo ^ hi
__host__ __device__ inline uint32_t gmix(uint32_t v) {
#if FLC_GHASH == 1
    uint32_t h = v ^ (v >> 16);
    h = mul24(h, 0xB5297Bu) ^ (h >> 24);
    h ^= h >> 16;
    h = mul24(h, 0x68E31Du) ^ (h >> 24);
    return h ^ (h >> 16);
#elif FLC_GHASH == 2
    const uint64_t p = (uint64_t)v * (uint64_t)(v ^ 0x2D358DCCu);
    return (uint32_t)p ^ (uint32_t)(p >> 32);
#else
    return fmix32(v);
#endif
}
__host__ __device__ inline uint32_t grouphash(uint32_t g, uint32_t rk) { return gmix(g * 0x9E3779B1u + rk); }
__host__ __device__ inline uint32_t draw_join(uint32_t hg, uint32_t q, uint32_t lo) {
    return ((hg >> (8u * q)) << 24) | (lo >> 8);
}
__host__ __device__ inline uint32_t dev_draw(uint32_t cs, uint32_t hg, uint32_t j, uint32_t rk) {
    return draw_join(hg, j & 3u, fmix32(cs + (rk ^ 0x27D4EB2Fu)));
}
__host__ __device__ inline uint32_t dev_u32(uint64_t ckey, uint32_t j) {
    const uint32_t rk = rowkey(ckey);
    return dev_draw(colbase(j), grouphash(j >> 2, rk), j, rk);
}
// Decision for a draw h (u = h * 2^-32) against an fp32 probability p:  h < sat_u32(ceil(p*2^32)).
// Equals (u < p) exactly for p in [0, 1); p >= 1 admits every h but 0xFFFFFFFF (prob. 2^-32), and
// p <= 0 or NaN admits none.  ldexp / ceil / saturating convert are exact single instructions.
__host__ __device__ inline uint32_t thr32(float p) {
    const float t = ceilf(ldexpf(p, 32));
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;   // v_cvt_u32_f32 saturates: < 0 -> 0, >= 2^32 -> 0xFFFFFFFF, NaN -> 0
    asm("v_cvt_u32_f32 %0, %1" : "=v"(r) : "v"(t));
    return r;
#else
    if (!(t > 0.f)) return 0u;                    // p <= 0 or NaN
    if (t >= 4294967295.f) return 0xFFFFFFFFu;
    return (uint32_t)t;
#endif
}
__host__ __device__ inline bool below32(uint32_t h, float p) { return h < thr32(p); }

// ------------------------------------------------------------------------------------------
// Wave helpers
// ------------------------------------------------------------------------------------------
__device__ inline int lane_id() { return __lane_id(); }

template <class T>
__device__ inline T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// |x| ordering key for TopK: sign cleared; NaN (0x7F8..1-0x7FF..F) above +inf, like torch.topk.
__device__ inline uint32_t mag_key(float x) { return __float_as_uint(x) & 0x7FFFFFFFu; }

// torch.sign semantics: -1 / 0 / +1 (NaN -> 0 is irrelevant: a NaN row's norm is NaN).
__device__ inline float tsign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

}  // namespace flc
