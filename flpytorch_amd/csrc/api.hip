// C ABI entry points of libflcodec.so (declared in include/flcodec.h): argument checking,
// workspace sizing and dispatch to the codec families.
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"

namespace flc {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return FLC_ERR_HIP;
}

// ---- kernel timing ------------------------------------------------------------------------
bool g_prof_on = false;
namespace {
std::mutex g_prof_mu;
std::vector<hipEvent_t> g_ev_free;
std::map<std::string, std::vector<std::pair<hipEvent_t, hipEvent_t>>> g_prof;
std::map<std::string, hipEvent_t> g_open;
hipEvent_t take_event() {
    if (!g_ev_free.empty()) { hipEvent_t e = g_ev_free.back(); g_ev_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}
}  // namespace

void prof_record(const char* name, hipStream_t st, bool begin) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    hipEvent_t e = take_event();
    if (!e) return;
    (void)hipEventRecord(e, st);
    if (begin) {
        g_open[name] = e;
    } else {
        auto it = g_open.find(name);
        if (it == g_open.end()) { g_ev_free.push_back(e); return; }
        g_prof[name].emplace_back(it->second, e);
        g_open.erase(it);
    }
}

static bool is_sel(int codec) { return codec == FLC_TOPK || codec == FLC_RANDK; }
static bool known(int codec) { return codec >= FLC_IDENT && codec <= FLC_RANK_K; }
// host-side check of the fields that choose WHAT is computed (before any device argument)
static int bad_params(const flc_codec_params* prm, const char* what) {
    if (prm->codec == FLC_TOPK && prm->tie != FLC_TIE_LOWEST && prm->tie != FLC_TIE_HIGHEST) {
        set_error("%s: unknown TopK tie rule %d (FLC_TIE_LOWEST / FLC_TIE_HIGHEST)", what, (int)prm->tie);
        return FLC_ERR_ARG;
    }
    return FLC_OK;
}

// ---- argument checks shared by the shifted entries ------------------------------------------------
static int too_many(const char* me, int64_t n, const char* what, int rc) {   // kernels index rows by blockIdx.y
    set_error("%s: n=%lld %s, at most %d per call (fold larger rounds as partials)", me, (long long)n, what, FLC_MAX_ROWS);
    return rc;
}

static int orphan_shift_out(const char* me, const float* shift_in, const float* shift_out) {
    if (shift_out && !shift_in) { set_error("%s: shift_out without shift_in", me); return FLC_ERR_ARG; }
    return FLC_OK;
}

// One row (flc_encode_shift, flc_pack_shift): the operands and what may be absent.  need_output: a
// call that writes neither msg nor shift_out is refused (the wire entry always writes its payload).
static int shift_row_check(const char* me, const float* a, const float* b, int64_t d, const float* base, const float* msg,
                           const float* shift_in, const float* shift_out, bool need_output) {
    if (d > 0 && (!a || !b)) { set_error("%s: need a and b", me); return FLC_ERR_ARG; }
    if (need_output && d > 0 && !msg && !shift_out) { set_error("%s: nothing to write (msg and shift_out null)", me); return FLC_ERR_ARG; }
    if (int rc = orphan_shift_out(me, shift_in, shift_out)) return rc;
    if (base && !msg) { set_error("%s: base without msg", me); return FLC_ERR_ARG; }
    return FLC_OK;
}

// The n-row entries over flc_shift_rows (flc_encode / randk / topk / dither _shift_reduce): the sizes,
// the empty call (*empty: return FLC_OK, nothing else is looked at), the operands every shape needs,
// and *sr, the copy the round hosts work on: a shift nobody stores is not read, and the leading
// dimensions of absent operands are zero.  late_tie: TopK parameters whose tie rule is checked
// here, after the operands (the entry that checks it first passes null).
static int shift_rows_prepare(const char* me, const flc_codec_params* late_tie, const flc_shift_rows* rows, int64_t n,
                              int64_t d, const float* d_out, flc_shift_rows* sr, bool* empty) {
    *empty = false;
    if (n < 0 || d < 0) { set_error("%s: n=%lld d=%lld", me, (long long)n, (long long)d); return FLC_ERR_ARG; }
    if (n > FLC_MAX_ROWS) return too_many(me, n, "rows", FLC_ERR_ARG);
    if (n == 0 || d == 0) { *empty = true; return FLC_OK; }
    if (!rows || !rows->d_a || !rows->d_b || !d_out) { set_error("%s: need rows, a, b and out", me); return FLC_ERR_ARG; }
    if (late_tie)
        if (int rc = bad_params(late_tie, me)) return rc;
    *sr = *rows;
    if (int rc = orphan_shift_out(me, sr->d_shift_in, sr->d_shift_out)) return rc;
    if (!sr->d_shift_out) { sr->d_shift_in = nullptr; sr->ldin = sr->ldout = 0; }
    if (!sr->d_base) sr->ldbase = 0;
    if (!sr->d_msg) sr->ldmsg = 0;
    return FLC_OK;
}

// the element range [lo, hi) that n rows of d elements at p + i * ld cover
static void row_span(const float* p, int64_t ld, int64_t n, int64_t d, uintptr_t* lo, uintptr_t* hi) {
    const int64_t last = (n - 1) * ld;
    const float* a = p + std::min<int64_t>(0, last);
    const float* b = p + std::max<int64_t>(0, last) + d;
    *lo = (uintptr_t)a;
    *hi = (uintptr_t)b;
}

// Output matrices of an n-row round (absent: p null): the rows of one must not overlap each other,
// and with ONE base vector for every row (ldbase == 0) no output may lie over it: a store there
// would change the base under the later rows.
struct OutRows { const char* name; const char* ldname; const float* p; int64_t ld; };
static int outputs_overlap(const char* me, std::initializer_list<OutRows> outs, const float* base, int64_t ldbase,
                           int64_t n, int64_t d) {
    if (n <= 1) return FLC_OK;
    for (const OutRows& o : outs)
        if (o.p && (o.ld < 0 ? -o.ld : o.ld) < d) {
            set_error("%s: the %s rows overlap (|%s| < d)", me, o.name, o.ldname);
            return FLC_ERR_ARG;
        }
    if (!base || ldbase != 0) return FLC_OK;
    const uintptr_t b0 = (uintptr_t)base, b1 = (uintptr_t)(base + d);
    for (const OutRows& o : outs) {
        if (!o.p) continue;
        uintptr_t lo, hi;
        row_span(o.p, o.ld, n, d, &lo, &hi);
        if (lo < b1 && b0 < hi) { set_error("%s: %s overlaps the shared base", me, o.name); return FLC_ERR_ARG; }
    }
    return FLC_OK;
}

// The row map of a _sampled entry against the round's normalised operands sr (shift_rows_prepare),
// everything decided on the host before any launch.  *m: the copy the round hosts work on, the bits
// of absent operands (and of a shift_in nobody stores from) cleared.
static int row_map_check(const char* me, const flc_row_map* map, const flc_shift_rows& sr, int64_t n, int64_t d,
                         flc_row_map* m) {
    if (!map || !map->h_ids || !map->d_ids) { set_error("%s: need map, h_ids and d_ids", me); return FLC_ERR_ARG; }
    *m = *map;
    const uint32_t all = FLC_IDX_B | FLC_IDX_BASE | FLC_IDX_MSG | FLC_IDX_SHIFT_IN | FLC_IDX_SHIFT_OUT;
    if (m->indexed & ~all) { set_error("%s: unknown bits 0x%x in map->indexed", me, (unsigned)(m->indexed & ~all)); return FLC_ERR_ARG; }
    if (m->n_total < 1 || m->n_total > (int64_t)INT32_MAX) { set_error("%s: n_total=%lld", me, (long long)m->n_total); return FLC_ERR_ARG; }
    if ((m->indexed & FLC_IDX_BASE) && sr.d_base && sr.ldbase == 0) {
        set_error("%s: FLC_IDX_BASE with a shared base (ldbase == 0)", me);
        return FLC_ERR_ARG;
    }
    if (!sr.d_base) m->indexed &= ~(uint32_t)FLC_IDX_BASE;
    if (!sr.d_msg) m->indexed &= ~(uint32_t)FLC_IDX_MSG;
    if (!sr.d_shift_out) m->indexed &= ~(uint32_t)(FLC_IDX_SHIFT_IN | FLC_IDX_SHIFT_OUT);
    for (int64_t i = 0; i < n; ++i)
        if (m->h_ids[i] < 0 || (int64_t)m->h_ids[i] >= m->n_total) {
            set_error("%s: ids[%lld]=%d outside [0, n_total=%lld)", me, (long long)i, (int)m->h_ids[i], (long long)m->n_total);
            return FLC_ERR_ARG;
        }
    struct Op { const char* name; const float* p; int64_t ld; uint32_t bit; };
    const Op outs[2] = {{"d_msg", sr.d_msg, sr.ldmsg, FLC_IDX_MSG}, {"d_shift_out", sr.d_shift_out, sr.ldout, FLC_IDX_SHIFT_OUT}};
    const Op ins[3] = {{"d_b", sr.d_b, sr.ldb, FLC_IDX_B}, {"d_base", sr.d_base, sr.ldbase, FLC_IDX_BASE},
                       {"d_shift_in", sr.d_shift_in, sr.ldin, FLC_IDX_SHIFT_IN}};
    if (m->indexed & (FLC_IDX_MSG | FLC_IDX_SHIFT_OUT)) {       // two participants would store into one row
        std::vector<int32_t> s(m->h_ids, m->h_ids + n);
        std::sort(s.begin(), s.end());
        for (int64_t i = 1; i < n; ++i)
            if (s[i] == s[i - 1]) { set_error("%s: id %d twice with an indexed output", me, (int)s[i]); return FLC_ERR_ARG; }
    }
    for (const Op& o : outs) {
        if (!o.p) continue;
        if ((m->indexed & o.bit) && m->n_total > 1 && (o.ld < 0 ? -o.ld : o.ld) < d) {
            set_error("%s: the indexed %s rows overlap (|ld| < d)", me, o.name);
            return FLC_ERR_ARG;
        }
        for (const Op& in : ins)
            if (in.p == o.p && in.ld == o.ld && !(m->indexed & in.bit) != !(m->indexed & o.bit)) {
                set_error("%s: %s is %s in place, but only one of them is indexed", me, o.name, in.name);
                return FLC_ERR_ARG;
            }
    }
    return FLC_OK;
}

// an output matrix's row count for the overlap checks: n_total where it is indexed
static int sampled_outputs_overlap(const char* me, const flc_shift_rows& sr, const flc_row_map& m, int64_t n, int64_t d) {
    if (int rc = outputs_overlap(me, {{"d_msg", "ldmsg", sr.d_msg, sr.ldmsg}}, sr.d_base, sr.ldbase,
                                 (m.indexed & FLC_IDX_MSG) ? m.n_total : n, d))
        return rc;
    return outputs_overlap(me, {{"d_shift_out", "ldout", sr.d_shift_out, sr.ldout}}, sr.d_base, sr.ldbase,
                           (m.indexed & FLC_IDX_SHIFT_OUT) ? m.n_total : n, d);
}

}  // namespace flc

using namespace flc;

extern "C" int flc_version(void) { return 104; }   // 1.04: flc_rows_alloc / free (1.03: flc_norm2_torch_cpu_ws; 1.02: flc_debug_resident; 1.01: tie, flc_norm2_torch_cpu)

#ifndef FLC_SRC_HASH
#define FLC_SRC_HASH "unknown"
#endif
extern "C" const char* flc_build_id(void) { return FLC_SRC_HASH; }

extern "C" int flc_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
    return FLC_OK;
}

extern "C" int flc_profile_collect(const char* kernel, double* h_total_ms, int64_t* h_launches) {
    if (!kernel || !h_total_ms || !h_launches) { set_error("flc_profile_collect: null argument"); return FLC_ERR_ARG; }
    std::vector<std::pair<hipEvent_t, hipEvent_t>> recs;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        auto it = g_prof.find(kernel);
        if (it != g_prof.end()) { recs.swap(it->second); g_prof.erase(it); }
    }
    double total = 0.0;
    for (auto& r : recs) {
        FLC_CHECK_HIP(hipEventSynchronize(r.second));
        float ms = 0.f;
        FLC_CHECK_HIP(hipEventElapsedTime(&ms, r.first, r.second));
        total += ms;
    }
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        for (auto& r : recs) { g_ev_free.push_back(r.first); g_ev_free.push_back(r.second); }
    }
    *h_total_ms = total;
    *h_launches = (int64_t)recs.size();
    return FLC_OK;
}

extern "C" const char* flc_last_error_string(void) { return g_err; }

extern "C" int flc_select_row_flags(const flc_codec_params* prm, int64_t n, int64_t d, const void* d_workspace,
                                    size_t ws_bytes, uint32_t* d_flags, void* stream) {
    if (!prm || (n > 0 && (!d_workspace || !d_flags))) { set_error("flc_select_row_flags: null argument"); return FLC_ERR_ARG; }
    return sel_row_flags(prm, n, d, d_workspace, ws_bytes, d_flags, (hipStream_t)stream);
}

// Host helper (no compute): the resident client-update matrix in PHYSICALLY CONTIGUOUS HBM
// (hipDeviceMallocContiguous).  A default allocation of tens of GB is stitched from fragments and
// some of its rows read 6-10 % slower, with more address-translation misses (profiles/r06/
// regions_pmc.jsonl); contiguous memory maps with the largest page fragments: C4's 51.2 GB shard
// read 8.04 vs 8.48 ms, its step 9.09 vs 9.57 ms, same process (profiles/r06/contig.jsonl).
extern "C" int flc_rows_alloc(size_t bytes, int contiguous, void** d_ptr) {
    if (!d_ptr || bytes == 0) { set_error("flc_rows_alloc: bad args"); return FLC_ERR_ARG; }
    *d_ptr = nullptr;
    const hipError_t e = contiguous ? hipExtMallocWithFlags(d_ptr, bytes, hipDeviceMallocContiguous) : hipMalloc(d_ptr, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *d_ptr = nullptr;
        set_error("flc_rows_alloc: %s of %zu bytes failed: %s", contiguous ? "contiguous allocation" : "hipMalloc", bytes,
                  hipGetErrorString(e));
        return FLC_ERR_HIP;
    }
    return FLC_OK;
}

extern "C" int flc_rows_free(void* d_ptr) {
    if (d_ptr && hipFree(d_ptr) != hipSuccess) { set_error("flc_rows_free: hipFree failed"); return FLC_ERR_HIP; }
    return FLC_OK;
}

extern "C" size_t flc_norm2_torch_cpu_workspace_size(int64_t n, int64_t d) {
    return (n <= 0 || d < 0) ? 0 : norm_torch_ws_bytes(n, d);
}

extern "C" int flc_norm2_torch_cpu_ws(const float* d_rows, int64_t ld, int64_t n, int64_t d, float* d_out, void* d_ws,
                                      size_t ws_bytes, void* stream) {
    if (n < 0 || d < 0 || (n > 1 && ld < d) || (n > 0 && (!d_rows || !d_out || !d_ws))) {
        set_error("flc_norm2_torch_cpu_ws: bad args (n=%lld d=%lld ld=%lld)", (long long)n, (long long)d, (long long)ld);
        return FLC_ERR_ARG;
    }
    if (n == 0) return FLC_OK;
    return norm_torch_ws_run(d_rows, ld, n, d, d_out, d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int flc_debug_resident(int grid_mult, int64_t spin_ticks) { return rs_debug(grid_mult, spin_ticks); }

extern "C" int flc_norm2_torch_cpu(const float* d_rows, int64_t ld, int64_t n, int64_t d, float* d_out, void* stream) {
    if (n < 0 || d < 0 || (n > 1 && ld < d) || (n > 0 && (!d_rows || !d_out))) {
        set_error("flc_norm2_torch_cpu: bad args (n=%lld d=%lld ld=%lld)", (long long)n, (long long)d, (long long)ld);
        return FLC_ERR_ARG;
    }
    if (n == 0) return FLC_OK;
    return norm_torch_run(d_rows, ld, n, d, d_out, (hipStream_t)stream);
}

namespace flc {
int selftest_division(const float* d_b, int nb, unsigned long long* d_bad, hipStream_t st);
}
extern "C" int flc_selftest_division(const float* d_divisors, int n, unsigned long long* d_mismatches,
                                     void* stream) {
    if (n < 0 || (n > 0 && (!d_divisors || !d_mismatches))) { set_error("flc_selftest_division: bad args"); return FLC_ERR_ARG; }
    if (n == 0) return FLC_OK;
    return selftest_division(d_divisors, n, d_mismatches, (hipStream_t)stream);
}

namespace flc {
size_t encode_row_workspace(const flc_codec_params* prm, int64_t d) {
    if (prm->codec == FLC_TOPK) return sel_workspace(prm, 1, d);
    if (prm->codec == FLC_RANK_K) return rk_workspace(prm, 1, d, false);
    if (prm->codec == FLC_RANDK) return randk_device_workspace(1, d);
    return ew_workspace(prm, 1, d);
}
}  // namespace flc

extern "C" size_t flc_encode_workspace_size(const flc_codec_params* prm, int64_t d) {
    if (!prm || !known(prm->codec)) return 0;
    if (prm->codec == FLC_TOPK) return sel_workspace(prm, 1, d);
    if (prm->codec == FLC_RANK_K) return rk_workspace(prm, 1, d, false);
    if (prm->codec == FLC_RANDK) return randk_device_workspace(1, d);
    return ew_workspace(prm, 1, d);
}

extern "C" size_t flc_encode_reduce_ex_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d, int norms_given,
                                                      int norm_mode) {
    if (!prm || !known(prm->codec)) return 0;
    if (is_sel(prm->codec)) return sel_workspace(prm, n, d);
    if (prm->codec == FLC_RANK_K) return rk_workspace(prm, n, d, true);
    return ew_workspace(prm, n, d, norms_given != 0, norm_mode);
}

extern "C" size_t flc_encode_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d) {
    return flc_encode_reduce_ex_workspace_size(prm, n, d, 0, FLC_NORMMODE_EXACT);
}

namespace flc {
// one row, dense output (flc_encode; also the first stage of flc_pack)
int encode_row(const flc_codec_params* prm, const flc_pattern* pat, const float* d_x, int64_t d,
               const float* d_pnorm_in, float* d_pnorm_out, float* d_out, void* d_ws, size_t ws_bytes, hipStream_t st) {
    const bool vec = (((uintptr_t)d_x | (uintptr_t)d_out) & 15u) == 0;
    switch (prm->codec) {
        case FLC_RANDK:
            if (!(pat && pat->d_randk_idx) && prm->k > d) { set_error("randk: K > D"); return FLC_ERR_ARG; }
            return randk_dense(prm, pat, d_x, d, d_out, d_ws, ws_bytes, st);
        case FLC_RANK_K: {
            RowSrc r{d_x, d, nullptr};
            return rk_run(prm, r, 1, d, /*reduce=*/false, nullptr, 1.f, d_out, d_ws, ws_bytes, st);
        }
        case FLC_TOPK: {
            RowSrc r{d_x, d, nullptr};
            return sel_run(prm, pat, r, vec, 1, d, /*assign=*/true, nullptr, 1.f, d_out, d_ws, ws_bytes, st);
        }
        default: {
            RowSrc s{d_x, d, nullptr};
            return ew_run(prm, pat, s, vec, 1, d, d_pnorm_in, d_pnorm_out, /*dense=*/true, d_out, nullptr, 1.f, d_ws,
                          ws_bytes, st);
        }
    }
}
}  // namespace flc

extern "C" int flc_encode(const flc_codec_params* prm, const flc_pattern* pat, const float* d_x, int64_t d,
                          const float* d_pnorm_in, float* d_pnorm_out, float* d_out, void* d_ws, size_t ws_bytes,
                          void* stream) {
    if (!prm || !known(prm->codec)) { set_error("flc_encode: unknown codec"); return FLC_ERR_UNSUPPORTED; }
    if (int rc = bad_params(prm, "flc_encode")) return rc;
    if (d < 0 || (d > 0 && (!d_x || !d_out))) { set_error("flc_encode: bad x/out/d"); return FLC_ERR_ARG; }
    return encode_row(prm, pat, d_x, d, d_pnorm_in, d_pnorm_out, d_out, d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" size_t flc_encode_shift_workspace_size(const flc_codec_params* prm, int64_t d) {
    if (!prm || !known(prm->codec) || d < 0) return 0;
    return shift_workspace(prm, d);
}

extern "C" int flc_encode_shift(const flc_codec_params* prm, const flc_pattern* pat, const float* d_a,
                                const float* d_b, int64_t d, float msg_scale, const float* d_base, float* d_msg,
                                float shift_alpha, const float* d_shift_in, float* d_shift_out, float* d_pnorm_out,
                                void* d_ws, size_t ws_bytes, void* stream) {
    const char* me = "flc_encode_shift";
    if (!prm || !known(prm->codec)) { set_error("%s: unknown codec", me); return FLC_ERR_UNSUPPORTED; }
    if (int rc = bad_params(prm, me)) return rc;
    if (d < 0) { set_error("%s: d < 0", me); return FLC_ERR_ARG; }
    if (int rc = shift_row_check(me, d_a, d_b, d, d_base, d_msg, d_shift_in, d_shift_out, /*need_output=*/true)) return rc;
    ShiftArgs sh{d_b, msg_scale, d_base, d_msg, shift_alpha, d_shift_in, d_shift_out};
    return shift_run(prm, pat, d_a, d, sh, d_pnorm_out, d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" size_t flc_encode_shift_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d) {
    if (!prm || !known(prm->codec) || n < 0 || d < 0) return 0;
    return shift_reduce_workspace(prm, n, d);
}

extern "C" int flc_encode_shift_reduce(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows* rows,
                                       int64_t n, int64_t d, const float* d_w, float w_total, float* d_pnorms_out,
                                       float* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    const char* me = "flc_encode_shift_reduce";
    if (!prm || !known(prm->codec)) { set_error("%s: unknown codec", me); return FLC_ERR_UNSUPPORTED; }
    if (int rc = bad_params(prm, me)) return rc;
    flc_shift_rows sr;
    bool empty;
    if (int rc = shift_rows_prepare(me, nullptr, rows, n, d, d_out, &sr, &empty)) return rc;
    if (empty) return FLC_OK;
    if (int rc = outputs_overlap(me, {{"d_msg", "ldmsg", sr.d_msg, sr.ldmsg}, {"d_shift_out", "ldout", sr.d_shift_out, sr.ldout}},
                                 sr.d_base, sr.ldbase, n, d))
        return rc;
    return shift_reduce_run(prm, pat, sr, n, d, d_w, w_total, d_pnorms_out, d_out, d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" size_t flc_frecon_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d) {
    if (!prm || !frecon_elementwise(prm->codec) || n < 0 || d < 0) return 0;
    return frecon_workspace(prm, n, d);
}

extern "C" int flc_frecon_reduce(const flc_codec_params* prm, const flc_pattern* pat, const flc_frecon_rows* rows, int64_t n,
                                 int64_t d, const float* d_w, float w_total, float* d_pnorms_u_out, float* d_pnorms_q_out,
                                 float* d_u_out, float* d_q_out, const flc_frecon_server* srv, void* d_ws, size_t ws_bytes,
                                 void* stream) {
    const char* me = "flc_frecon_reduce";
    if (!prm || !known(prm->codec)) { set_error("%s: unknown codec", me); return FLC_ERR_UNSUPPORTED; }
    if (!frecon_elementwise(prm->codec)) {
        set_error("%s: only the elementwise codecs have a two-message round (compose RandK / TopK / Rank-K from flc_encode_shift_reduce)", me);
        return FLC_ERR_UNSUPPORTED;
    }
    // the u message is the in-place DIANA round over (a, h): the shifted entries' shared checks see it as such
    flc_shift_rows as_diana, sr;
    memset(&as_diana, 0, sizeof(as_diana));
    if (rows) {
        as_diana.d_a = rows->d_a; as_diana.lda = rows->lda;
        as_diana.d_b = as_diana.d_shift_in = as_diana.d_shift_out = rows->d_h;
        as_diana.ldb = as_diana.ldin = as_diana.ldout = rows->ldh;
    }
    const float* some_out = srv ? srv->d_result : d_u_out;
    bool empty;
    if (int rc = shift_rows_prepare(me, nullptr, rows ? &as_diana : nullptr, n, d, some_out, &sr, &empty)) return rc;
    if (empty) return FLC_OK;
    if (!rows->d_p) { set_error("%s: need the p rows", me); return FLC_ERR_ARG; }
    if (!srv && (!d_u_out || !d_q_out)) { set_error("%s: d_u_out and d_q_out are required without a server tail", me); return FLC_ERR_ARG; }
    if (srv && (!srv->d_g_server_prev || !srv->d_h_prev || !srv->d_result)) {
        set_error("%s: the server tail needs g_server_prev, h_prev and result", me);
        return FLC_ERR_ARG;
    }
    if (int rc = outputs_overlap(me, {{"d_h", "ldh", rows->d_h, rows->ldh}}, nullptr, 0, n, d)) return rc;
    if (srv) {
        const OutRows ops[3] = {{"d_a", "lda", rows->d_a, rows->lda}, {"d_h", "ldh", rows->d_h, rows->ldh},
                                {"d_p", "ldp", rows->d_p, rows->ldp}};
        const OutRows outs[2] = {{"d_result", "", srv->d_result, 0}, {"d_h_prev_out", "", srv->d_h_prev_out, 0}};
        for (const OutRows& o : outs) {
            if (!o.p) continue;
            const uintptr_t o0 = (uintptr_t)o.p, o1 = (uintptr_t)(o.p + d);
            for (const OutRows& r : ops) {
                uintptr_t lo, hi;
                row_span(r.p, r.ld, n, d, &lo, &hi);
                if (lo < o1 && o0 < hi) { set_error("%s: %s overlaps the %s rows", me, o.name, r.name); return FLC_ERR_ARG; }
            }
        }
    }
    if (int rc = frecon_precheck(prm, pat)) return rc;
    if (ws_bytes < frecon_workspace(prm, n, d)) { set_error("%s: workspace too small", me); return FLC_ERR_WORKSPACE; }
    if (frecon_workspace(prm, n, d) > 0 && !d_ws) { set_error("%s: null workspace", me); return FLC_ERR_ARG; }
    return frecon_run(prm, pat, *rows, n, d, d_w, w_total, d_pnorms_u_out, d_pnorms_q_out, d_u_out, d_q_out, srv, d_ws,
                      ws_bytes, (hipStream_t)stream);
}

extern "C" size_t flc_randk_shift_reduce_workspace_size(const flc_codec_params* prm, const flc_pattern* pat, int64_t n,
                                                        int64_t d) {
    if (!prm || prm->codec != FLC_RANDK || n < 0 || d < 0) return 0;
    return randk_shift_workspace(prm, pat && pat->d_randk_idx, n, d);
}

extern "C" int flc_randk_shift_reduce(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows* rows,
                                      int64_t n, int64_t d, const float* d_w, float w_total, float* d_out, void* d_ws,
                                      size_t ws_bytes, void* stream) {
    const char* me = "flc_randk_shift_reduce";
    if (!prm || prm->codec != FLC_RANDK) {
        set_error("%s: only FLC_RANDK has a sparse shifted round (use flc_encode_shift_reduce)", me);
        return FLC_ERR_UNSUPPORTED;
    }
    flc_shift_rows sr;
    bool empty;
    if (int rc = shift_rows_prepare(me, nullptr, rows, n, d, d_out, &sr, &empty)) return rc;
    if (empty) return FLC_OK;
    return randk_shift_run(prm, pat, sr, n, d, d_w, w_total, d_out, d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" size_t flc_topk_shift_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d) {
    if (!prm || prm->codec != FLC_TOPK || n < 0 || d < 0) return 0;
    return topk_shift_workspace(prm, n, d);
}

extern "C" int flc_topk_shift_reduce(const flc_codec_params* prm, const flc_shift_rows* rows, int64_t n, int64_t d,
                                     const float* d_w, float w_total, float* d_out, void* d_ws, size_t ws_bytes,
                                     void* stream) {
    const char* me = "flc_topk_shift_reduce";
    if (!prm || prm->codec != FLC_TOPK) {
        set_error("%s: only FLC_TOPK has a batched shifted round (use flc_encode_shift_reduce)", me);
        return FLC_ERR_UNSUPPORTED;
    }
    flc_shift_rows sr;
    bool empty;
    if (int rc = shift_rows_prepare(me, prm, rows, n, d, d_out, &sr, &empty)) return rc;
    if (empty) return FLC_OK;
    return topk_shift_run(prm, sr, n, d, d_w, w_total, d_out, d_ws, ws_bytes, (hipStream_t)stream);
}

// ---- partial participation: the three rounds over sampled client rows (flc_row_map) ----------------
extern "C" size_t flc_encode_shift_reduce_sampled_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d) {
    if (!prm || !known(prm->codec) || n < 0 || d < 0) return 0;
    return shift_reduce_workspace(prm, n, d);       // the ids are the caller's: nothing is added
}

extern "C" int flc_encode_shift_reduce_sampled(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows* rows,
                                               const flc_row_map* map, int64_t n, int64_t d, const float* d_w, float w_total,
                                               float* d_pnorms_out, float* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    const char* me = "flc_encode_shift_reduce_sampled";
    if (!prm || !known(prm->codec)) { set_error("%s: unknown codec", me); return FLC_ERR_UNSUPPORTED; }
    if (int rc = bad_params(prm, me)) return rc;
    flc_shift_rows sr;
    bool empty;
    if (int rc = shift_rows_prepare(me, nullptr, rows, n, d, d_out, &sr, &empty)) return rc;
    if (empty) return FLC_OK;
    flc_row_map m;
    if (int rc = row_map_check(me, map, sr, n, d, &m)) return rc;
    if (int rc = sampled_outputs_overlap(me, sr, m, n, d)) return rc;
    return shift_reduce_run(prm, pat, sr, n, d, d_w, w_total, d_pnorms_out, d_out, d_ws, ws_bytes, (hipStream_t)stream, &m);
}

extern "C" size_t flc_randk_shift_reduce_sampled_workspace_size(const flc_codec_params* prm, const flc_pattern* pat, int64_t n,
                                                                int64_t d) {
    if (!prm || prm->codec != FLC_RANDK || n < 0 || d < 0) return 0;
    return randk_shift_workspace(prm, pat && pat->d_randk_idx, n, d, /*sampled=*/true);
}

extern "C" int flc_randk_shift_reduce_sampled(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows* rows,
                                              const flc_row_map* map, int64_t n, int64_t d, const float* d_w, float w_total,
                                              float* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    const char* me = "flc_randk_shift_reduce_sampled";
    if (!prm || prm->codec != FLC_RANDK) {
        set_error("%s: only FLC_RANDK has a sparse shifted round (use flc_encode_shift_reduce_sampled)", me);
        return FLC_ERR_UNSUPPORTED;
    }
    flc_shift_rows sr;
    bool empty;
    if (int rc = shift_rows_prepare(me, nullptr, rows, n, d, d_out, &sr, &empty)) return rc;
    if (empty) return FLC_OK;
    flc_row_map m;
    if (int rc = row_map_check(me, map, sr, n, d, &m)) return rc;
    if (pat && pat->d_randk_counts) {
        set_error("%s: d_randk_counts are keyed by position, not by client id (the entry computes its counts)", me);
        return FLC_ERR_ARG;
    }
    return randk_shift_run(prm, pat, sr, n, d, d_w, w_total, d_out, d_ws, ws_bytes, (hipStream_t)stream, &m);
}

extern "C" size_t flc_topk_shift_reduce_sampled_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d) {
    if (!prm || prm->codec != FLC_TOPK || n < 0 || d < 0) return 0;
    return topk_shift_workspace(prm, n, d, /*sampled=*/true);
}

extern "C" int flc_topk_shift_reduce_sampled(const flc_codec_params* prm, const flc_shift_rows* rows, const flc_row_map* map,
                                             int64_t n, int64_t d, const float* d_w, float w_total, float* d_out,
                                             void* d_ws, size_t ws_bytes, void* stream) {
    const char* me = "flc_topk_shift_reduce_sampled";
    if (!prm || prm->codec != FLC_TOPK) {
        set_error("%s: only FLC_TOPK has a batched shifted round (use flc_encode_shift_reduce_sampled)", me);
        return FLC_ERR_UNSUPPORTED;
    }
    flc_shift_rows sr;
    bool empty;
    if (int rc = shift_rows_prepare(me, prm, rows, n, d, d_out, &sr, &empty)) return rc;
    if (empty) return FLC_OK;
    flc_row_map m;
    if (int rc = row_map_check(me, map, sr, n, d, &m)) return rc;
    return topk_shift_run(prm, sr, n, d, d_w, w_total, d_out, d_ws, ws_bytes, (hipStream_t)stream, &m);
}

extern "C" size_t flc_dither_shift_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d) {
    if (!prm || n < 0 || d < 0) return 0;
    return dither_shift_workspace(prm, n, d);
}

extern "C" int flc_dither_shift_reduce(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows* rows,
                                       int64_t n, int64_t d, const float* d_w, float w_total, float* d_pnorms_out,
                                       float* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    const char* me = "flc_dither_shift_reduce";
    if (!prm || prm->codec != FLC_STD_DITHERING || prm->norm != FLC_NORM_L2) {
        set_error("%s: only FLC_STD_DITHERING with FLC_NORM_L2 (QSGD) has a one-read shifted round (use flc_encode_shift_reduce)", me);
        return FLC_ERR_UNSUPPORTED;
    }
    flc_shift_rows sr;
    bool empty;
    if (int rc = shift_rows_prepare(me, nullptr, rows, n, d, d_out, &sr, &empty)) return rc;
    if (empty) return FLC_OK;
    return dither_shift_run(prm, pat, sr, n, d, d_w, w_total, d_pnorms_out, d_out, d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int flc_dither_row_flags(int64_t n, int64_t d, const void* d_ws, size_t ws_bytes, uint32_t* d_flags, void* stream) {
    if (n < 0 || d < 0) { set_error("flc_dither_row_flags: n=%lld d=%lld", (long long)n, (long long)d); return FLC_ERR_ARG; }
    if (n > 0 && d > 0 && (!d_ws || !d_flags)) { set_error("flc_dither_row_flags: null argument"); return FLC_ERR_ARG; }
    return dither_row_flags(n, d, d_ws, ws_bytes, d_flags, (hipStream_t)stream);
}

extern "C" int64_t flc_payload_bytes(const flc_codec_params* prm, int64_t d) {
    if (!prm || !known(prm->codec) || d < 0) return 0;
    return payload_bytes(prm, d);
}

extern "C" int flc_payload_format(const flc_codec_params* prm) {
    if (!prm || !known(prm->codec)) return 0;
    return payload_format(prm);
}

extern "C" int flc_payload_validate(const flc_codec_params* prm, const void* h_payload, int64_t nbytes, int64_t d) {
    if (!prm || !known(prm->codec)) { set_error("flc_payload_validate: unknown codec"); return FLC_ERR_UNSUPPORTED; }
    if (d < 0 || nbytes < 0 || (nbytes > 0 && !h_payload)) { set_error("flc_payload_validate: bad payload/nbytes/d"); return FLC_ERR_ARG; }
    return payload_validate(prm, (const uint8_t*)h_payload, nbytes, d);
}

extern "C" size_t flc_pack_workspace_size(const flc_codec_params* prm, int64_t d) {
    if (!prm || !known(prm->codec) || d < 0) return 0;
    return pack_workspace(prm, d);
}

extern "C" int flc_pack(const flc_codec_params* prm, const flc_pattern* pat, const float* d_x, int64_t d,
                        void* d_payload, void* d_ws, size_t ws_bytes, void* stream) {
    if (!prm || !known(prm->codec)) { set_error("flc_pack: unknown codec"); return FLC_ERR_UNSUPPORTED; }
    if (int rc = bad_params(prm, "flc_pack")) return rc;
    if (d < 0 || !d_payload || (d > 0 && !d_x)) { set_error("flc_pack: bad x/payload/d"); return FLC_ERR_ARG; }
    return pack_run(prm, pat, d_x, d, (char*)d_payload, d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int flc_unpack(const flc_codec_params* prm, const void* d_payload, int64_t d, float* d_out, void* stream) {
    if (!prm || !known(prm->codec)) { set_error("flc_unpack: unknown codec"); return FLC_ERR_UNSUPPORTED; }
    if (d < 0 || (d > 0 && (!d_payload || !d_out))) { set_error("flc_unpack: bad payload/out/d"); return FLC_ERR_ARG; }
    return unpack_run(prm, (const char*)d_payload, d, d_out, (hipStream_t)stream);
}

extern "C" size_t flc_unpack_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d) {
    if (!prm || !known(prm->codec) || n < 0 || d < 0) return 0;
    return unpack_reduce_workspace(prm, n, d);
}

extern "C" int flc_unpack_reduce(const flc_codec_params* prm, const void* d_payloads, int64_t ld_bytes,
                                 const void* const* d_payload_ptrs, int64_t n, int64_t d, const float* d_w,
                                 float w_total, float* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    if (!prm || !known(prm->codec)) { set_error("flc_unpack_reduce: unknown codec"); return FLC_ERR_UNSUPPORTED; }
    if (n < 0 || d < 0 || (d > 0 && !d_out)) { set_error("flc_unpack_reduce: bad n/d/out"); return FLC_ERR_ARG; }
    if (n > FLC_MAX_ROWS) {
        set_error("flc_unpack_reduce: n=%lld payloads, at most %d per call", (long long)n, FLC_MAX_ROWS);
        return FLC_ERR_UNSUPPORTED;
    }
    if (n > 0 && d > 0 && !d_payloads && !d_payload_ptrs) { set_error("flc_unpack_reduce: no payloads"); return FLC_ERR_ARG; }
    if (d_payloads && ld_bytes < payload_bytes(prm, d)) { set_error("flc_unpack_reduce: ld_bytes < payload size"); return FLC_ERR_ARG; }
    return unpack_reduce_run(prm, (const char*)d_payloads, ld_bytes, (const char* const*)d_payload_ptrs, n, d, d_w,
                             w_total, d_out, d_ws, ws_bytes, (hipStream_t)stream);
}

// ---- shifted steps on the wire (wire_shift.hip) ----------------------------------------------------
extern "C" size_t flc_pack_shift_workspace_size(const flc_codec_params* prm, int64_t d) {
    if (!prm || !known(prm->codec) || prm->codec == FLC_RANK_K || d < 0) return 0;
    return pack_shift_workspace(prm, d);
}

extern "C" int flc_pack_shift(const flc_codec_params* prm, const flc_pattern* pat, const float* d_a, const float* d_b,
                              int64_t d, float msg_scale, const float* d_base, float* d_msg, float shift_alpha,
                              const float* d_shift_in, float* d_shift_out, void* d_payload, void* d_ws, size_t ws_bytes,
                              void* stream) {
    const char* me = "flc_pack_shift";
    if (!prm || !known(prm->codec)) { set_error("%s: unknown codec", me); return FLC_ERR_UNSUPPORTED; }
    if (prm->codec == FLC_RANK_K) { set_error("%s: Rank-K payloads are not carried by shifted steps", me); return FLC_ERR_UNSUPPORTED; }
    if (int rc = bad_params(prm, me)) return rc;
    if (d < 0) { set_error("%s: d < 0", me); return FLC_ERR_ARG; }
    if (!d_payload) { set_error("%s: need a payload", me); return FLC_ERR_ARG; }
    if ((uintptr_t)d_payload & 15u) { set_error("%s: payload must be 16-byte aligned", me); return FLC_ERR_ARG; }
    if (int rc = shift_row_check(me, d_a, d_b, d, d_base, d_msg, d_shift_in, d_shift_out, /*need_output=*/false)) return rc;
    ShiftArgs sh{d_b, msg_scale, d_base, d_msg, shift_alpha, d_shift_out ? d_shift_in : nullptr, d_shift_out};
    return pack_shift_run(prm, pat, d_a, d, sh, (char*)d_payload, d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" size_t flc_unpack_shift_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d) {
    if (!prm || !known(prm->codec) || prm->codec == FLC_RANK_K || n < 0 || d < 0) return 0;
    return unpack_shift_reduce_workspace(prm, n, d);
}

extern "C" int flc_unpack_shift_reduce(const flc_codec_params* prm, const flc_payload_rows* rows, int64_t n, int64_t d,
                                       const float* d_w, float w_total, float* d_out, void* d_ws, size_t ws_bytes,
                                       void* stream) {
    const char* me = "flc_unpack_shift_reduce";
    if (!prm || !known(prm->codec)) { set_error("%s: unknown codec", me); return FLC_ERR_UNSUPPORTED; }
    if (prm->codec == FLC_RANK_K) { set_error("%s: Rank-K payloads are not carried by shifted steps", me); return FLC_ERR_UNSUPPORTED; }
    if (n < 0 || d < 0) { set_error("%s: n=%lld d=%lld", me, (long long)n, (long long)d); return FLC_ERR_ARG; }
    if (n > FLC_MAX_ROWS) return too_many(me, n, "payloads", FLC_ERR_UNSUPPORTED);
    if (d == 0) return FLC_OK;
    if (!d_out) { set_error("%s: need out", me); return FLC_ERR_ARG; }
    flc_payload_rows pr;
    memset(&pr, 0, sizeof(pr));
    pr.msg_scale = 1.f;
    if (n > 0) {
        if (!rows || (!rows->d_payloads && !rows->d_payload_ptrs)) { set_error("%s: no payloads", me); return FLC_ERR_ARG; }
        pr = *rows;
        if (pr.d_payloads) {
            pr.d_payload_ptrs = nullptr;
            if ((uintptr_t)pr.d_payloads & 15u) { set_error("%s: payload rows must be 16-byte aligned", me); return FLC_ERR_ARG; }
            if (pr.ld_bytes < payload_bytes(prm, d) || (pr.ld_bytes & 15)) {
                set_error("%s: ld_bytes=%lld, at least the payload's %lld bytes and a multiple of 16", me,
                          (long long)pr.ld_bytes, (long long)payload_bytes(prm, d));
                return FLC_ERR_ARG;
            }
        }
        if (!pr.d_base) pr.ldbase = 0;
        if (!pr.d_msg) pr.ldmsg = 0;
        if (int rc = outputs_overlap(me, {{"d_msg", "ldmsg", pr.d_msg, pr.ldmsg}}, pr.d_base, pr.ldbase, n, d)) return rc;
    }
    return unpack_shift_reduce_run(prm, pr, n, d, d_w, w_total, d_out, d_ws, ws_bytes, (hipStream_t)stream);
}

namespace flc {
// the torch-order mode restates p = 2 of the dithering codecs; p = inf: a maximum, exact in any order
static bool dithering(int codec) { return codec == FLC_STD_DITHERING || codec == FLC_NAT_DITHERING; }
}  // namespace flc

extern "C" int flc_encode_reduce_ex(const flc_codec_params* prm, const flc_pattern* pat, const float* d_rows, int64_t ld,
                                    const float* const* d_row_ptrs, int64_t n, int64_t d, const float* d_w, float w_total,
                                    const float* d_pnorms_in, int norm_mode, float* d_pnorms_out, float* d_out, void* d_ws,
                                    size_t ws_bytes, void* stream) {
    if (!prm || !known(prm->codec)) { set_error("flc_encode_reduce: unknown codec"); return FLC_ERR_UNSUPPORTED; }
    if (int rc = bad_params(prm, "flc_encode_reduce")) return rc;
    if (norm_mode != FLC_NORMMODE_EXACT && norm_mode != FLC_NORMMODE_TORCH_CPU) {
        set_error("flc_encode_reduce_ex: unknown norm_mode %d", norm_mode);
        return FLC_ERR_ARG;
    }
    if (d_pnorms_in && norm_mode != FLC_NORMMODE_EXACT) {
        set_error("flc_encode_reduce_ex: d_pnorms_in and a norm_mode are two sources for one norm");
        return FLC_ERR_ARG;
    }
    if (!dithering(prm->codec)) { d_pnorms_in = nullptr; norm_mode = FLC_NORMMODE_EXACT; }
    if (norm_mode == FLC_NORMMODE_TORCH_CPU) {
        if (prm->norm == FLC_NORM_L1) {
            set_error("flc_encode_reduce_ex: FLC_NORMMODE_TORCH_CPU restates torch's p = 2 reduction only (p = 1 asked)");
            return FLC_ERR_UNSUPPORTED;
        }
        if (prm->norm != FLC_NORM_L2) norm_mode = FLC_NORMMODE_EXACT;
    }
    if (n < 0 || d < 0 || (d > 0 && !d_out)) { set_error("flc_encode_reduce: bad n/d/out"); return FLC_ERR_ARG; }
    if (n > FLC_MAX_ROWS) return too_many("flc_encode_reduce", n, "rows", FLC_ERR_UNSUPPORTED);
    if (n > 0 && d > 0 && !d_rows && !d_row_ptrs) { set_error("flc_encode_reduce: no rows"); return FLC_ERR_ARG; }
    if (d_rows && ld < d) { set_error("flc_encode_reduce: ld < d"); return FLC_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    if (d == 0) return FLC_OK;
    if (n == 0) {
        FLC_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)d * sizeof(float), st));
        return FLC_OK;
    }
    // vector path: matrix rows 16-byte aligned with ld % 4 == 0; pointer rows are required aligned
    const bool vec = d_rows ? ((((uintptr_t)d_rows & 15u) == 0) && (ld % 4 == 0)) : true;
    if (prm->codec == FLC_IDENT) {
        RowSrc s{d_rows, ld, d_row_ptrs};
        return reduce_impl(s, vec, n, d, nullptr, d_w, w_total, FLC_REDUCE_PLAIN, d_out, st);
    }
    if (prm->codec == FLC_RANK_K) {
        RowSrc r{d_rows, ld, d_row_ptrs};
        return rk_run(prm, r, n, d, /*reduce=*/true, d_w, w_total, d_out, d_ws, ws_bytes, st);
    }
    if (is_sel(prm->codec)) {
        RowSrc r{d_rows, ld, d_row_ptrs};
        return sel_run(prm, pat, r, vec, n, d, false, d_w, w_total, d_out, d_ws, ws_bytes, st);
    }
    RowSrc s{d_rows, ld, d_row_ptrs};
    return ew_run(prm, pat, s, vec, n, d, d_pnorms_in, d_pnorms_out, false, d_out, d_w, w_total, d_ws, ws_bytes, st, nullptr,
                  nullptr, norm_mode);
}

extern "C" int flc_encode_reduce(const flc_codec_params* prm, const flc_pattern* pat, const float* d_rows, int64_t ld,
                                 const float* const* d_row_ptrs, int64_t n, int64_t d, const float* d_w, float w_total,
                                 float* d_pnorms_out, float* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    return flc_encode_reduce_ex(prm, pat, d_rows, ld, d_row_ptrs, n, d, d_w, w_total, nullptr, FLC_NORMMODE_EXACT, d_pnorms_out,
                                d_out, d_ws, ws_bytes, stream);
}

extern "C" size_t flc_device_randk_counts_workspace_size(int64_t n, int64_t d) {
    if (n < 1 || d < 1) return 0;
    return randk_device_workspace(n, d);
}

extern "C" int flc_device_randk_counts(uint64_t seed, int64_t client0, int64_t n, int64_t d, int64_t k,
                                       uint32_t* d_counts, void* d_ws, size_t ws_bytes, void* stream) {
    if (n < 1 || d < 1 || k < 1 || k > d || d >= (int64_t)0xFFFFFFFF || !d_counts) {
        set_error("flc_device_randk_counts: bad arguments");
        return FLC_ERR_ARG;
    }
    if (n > FLC_MAX_ROWS) {   // k_randk_counts indexes rows by blockIdx.y
        set_error("flc_device_randk_counts: n=%lld rows, at most %d per call", (long long)n, FLC_MAX_ROWS);
        return FLC_ERR_UNSUPPORTED;
    }
    return randk_device_counts(seed, client0, n, d, k, d_counts, d_ws, ws_bytes, (hipStream_t)stream);
}
