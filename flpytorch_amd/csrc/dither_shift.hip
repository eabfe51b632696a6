// The one-read QSGD shifted round (flc_dither_shift_reduce).
//
// A DIANA / EF21 round with standard dithering, p = 2 (qsgd:s), device draws,
//     v = a_i[j] - b_i[j];  e = C_i(v);  t = e * msg_scale;  m = base ? base[j] + t : t;
//     h' = shift_in[j] + shift_alpha * e
// through the sparse QSGD pipeline of the DCGD uplink (dither_sparse.hip) with a two-operand row
// source: a and b are read ONCE — the filter takes the norm of a - b and the candidates in the same
// pass — instead of the general entry's norm pass plus encode pass, and because C(v) is sparse the
// in-place operand is written at the nonzero elements only:
//   ds_run_t<DiffSrc>        k_ds_sample, k_ds_filter, k_ds_final, k_ds_resolve over a - b, and (A, D)
//                            k_ds_accum, the fold of the messages
//   k_ds_shift_lists         the sparse epilogue: every list entry's in-place update (A, B)
//   k_ds_shift_dense_rows    the same for rows the pipeline flagged dense (A, B)
//   reduce_impl              B: the dense fold of the updated rows
// This file is the host side: which calls are taken (decided before any launch, so that a refused
// call writes nothing), the workspace, and the flags hook.  The kernels live with the pipeline they
// extend, in dither_sparse.hip.
//
// Shapes: the table in flcodec.h.  A and D fold e itself, so msg_scale must be 1 there; C (MARINA's one
// shared base) is refused: its fold needs the (index, value) list form.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace flc {

static const char* const DSH_ME = "flc_dither_shift_reduce";

static bool dsh_codec(const flc_codec_params* prm) { return prm && prm->codec == FLC_STD_DITHERING && prm->norm == FLC_NORM_L2; }

size_t dither_shift_workspace(const flc_codec_params* prm, int64_t n, int64_t d) {
    if (!dsh_codec(prm) || n <= 0 || d <= 0) return 0;
    return ds_workspace(prm, n, d);                         // carve_ds's layout at the workspace base, nothing else
}

int dither_shift_run(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows& sr, int64_t n, int64_t d,
                     const float* w, float wt, float* pnorms_out, float* out, void* ws, size_t ws_bytes, hipStream_t st) {
    const char* me = DSH_ME;
    if (pat && pat->d_uniforms) {
        set_error("%s: compat draws (d_uniforms) are not taken by the one-read round (use flc_encode_shift_reduce)", me);
        return FLC_ERR_UNSUPPORTED;
    }
    if (d >= (int64_t)0x7FFFFFFF) { set_error("%s: D too large for the sparse pipeline's 32-bit offsets", me); return FLC_ERR_ARG; }
    if (!ds_eligible(prm, pat, n, d)) {
        set_error("%s: the sparse QSGD path does not take (s=%d, n=%lld, d=%lld, path hint %d): FLC_PATH_DENSE, a candidate "
                  "share past the staging capacity, or no level table (use flc_encode_shift_reduce)", me, (int)prm->s,
                  (long long)n, (long long)d, (int)(prm->flags & FLC_PATH_MASK));
        return FLC_ERR_UNSUPPORTED;
    }
    const int shape = shift_shape(sr, me);
    if (shape < 0) return FLC_ERR_UNSUPPORTED;
    if (shape == SHAPE_C) {
        set_error("%s: a shared base (MARINA) is not taken yet: its fold needs the (index, value) list form "
                  "(use flc_encode_shift_reduce)", me);
        return FLC_ERR_UNSUPPORTED;
    }
    if (shape != SHAPE_B && sr.msg_scale != 1.0f) {
        set_error("%s: msg_scale must be 1 when the messages themselves are folded (got %g)", me, (double)sr.msg_scale);
        return FLC_ERR_UNSUPPORTED;
    }
    if (int rc = inplace_rows_check(me, shape, sr, n, d)) return rc;
    if (ws_bytes < dither_shift_workspace(prm, n, d)) { set_error("%s: workspace too small", me); return FLC_ERR_WORKSPACE; }
    return ds_shift_run(prm, pat, sr, shape, n, d, w, wt, pnorms_out, out, ws, ws_bytes, st);
}

// Test hook: DsWs.flags of the workspace the entry left (bit 1: the row was folded dense; bit 4: its
// norm lies in the fast-division window), copied on `st`.
int dither_row_flags(int64_t n, int64_t d, const void* ws, size_t ws_bytes, uint32_t* flags, hipStream_t st) {
    if (n <= 0 || d <= 0) return FLC_OK;
    if (ws_bytes < ds_workspace(nullptr, n, d)) { set_error("flc_dither_row_flags: workspace too small"); return FLC_ERR_WORKSPACE; }
    FLC_CHECK_HIP(hipMemcpyAsync(flags, ds_flags_at(ws, n, d), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    return FLC_OK;
}

}  // namespace flc
