/*
 * flcodec — MI355X (gfx950) gradient codecs + N-way reduction: the C ABI.
 *
 * The drop-in boundary for FL_PyTorch's simulated-uplink hot path.  The reference is pure
 * Python; the Python layer in flpytorch_amd/aggregation binds these entry points with ctypes
 * (INTEGRATION.md shows the binding) and keeps the reference's object protocol on top:
 *   - Compressor.generateCompressPattern / compressVector   fl_pytorch/utils/compressors.py:196-371
 *   - <Algorithm>.serverGradient                           fl_pytorch/utils/algorithms.py:1748-1770,
 *                                                          1810-1832 (+ the identical cores listed
 *                                                          in SURVEY.md §8a row a14)
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory (caller-owned; the library never frees it);
 *     h_* is host memory.  fp32 data only (other dtypes: FLC_ERR_DTYPE).
 *   - every compute call is asynchronous on `stream` (a hipStream_t, passed as void*), never
 *     synchronises the device, never allocates: scratch comes from a caller workspace sized by
 *     the matching *_workspace_size query.  Calls are reentrant across host threads that use
 *     distinct streams and distinct workspaces.
 *   - return 0 (FLC_OK) or an flc_status; flc_last_error_string() gives the detail for the
 *     calling thread.
 */
#ifndef FLCODEC_H
#define FLCODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    FLC_OK = 0,
    FLC_ERR_ARG = 1,        /* bad size / null pointer / misaligned where alignment is required */
    FLC_ERR_DTYPE = 2,      /* not fp32 */
    FLC_ERR_HIP = 3,        /* a HIP runtime call failed (launch, memset) */
    FLC_ERR_WORKSPACE = 4,  /* workspace smaller than *_workspace_size() */
    FLC_ERR_UNSUPPORTED = 5 /* codec / mode not supported (e.g. a p-norm other than 1, 2, inf) */
} flc_status;

/* Codec ids = the reference's CompressorType values (compressors.py:11-19). */
typedef enum {
    FLC_IDENT = 1,
    FLC_LAZY = 2,
    FLC_RANDK = 3,
    FLC_NATURAL = 4,
    FLC_STD_DITHERING = 5,
    FLC_NAT_DITHERING = 6,
    FLC_TOPK = 7,
    FLC_RANK_K = 8          /* k = K; rank-K truncated SVD of the A x B view (compressors.py:336-364):
                               rocSOLVER / rocBLAS, parity to a stated tolerance */
} flc_codec;

/* p-norm used by the dithering codecs (Compressor.p, compressors.py:91, 123). */
#define FLC_NORM_L1 1
#define FLC_NORM_L2 2
#define FLC_NORM_LINF 0

/* Execution hints (flc_codec_params.flags).  They choose HOW a result is computed, never WHAT:
 * every combination gives the same bits.  0 = the library's choice.
 *   bits 0-1  standard dithering with p = 2: FLC_PATH_SPARSE (one-read candidate filter + exact
 *             fold) or FLC_PATH_DENSE (norm pass, then encode pass); flc_encode of one row takes
 *             the sparse pass only when FLC_PATH_SPARSE is set
 *   bits 8-15 fused encode+reduce (QSGD sparse path, TopK): number of row groups whose tails are
 *             pipelined under the next group's streaming pass (FLC_ROW_GROUPS(g), g in 1..255) */
#define FLC_PATH_AUTO 0
#define FLC_PATH_SPARSE 1
#define FLC_PATH_DENSE 2
#define FLC_PATH_MASK 3
#define FLC_ROW_GROUPS(g) (((g) & 0xFF) << 8)

/* Codec configuration — the constants Compressor.make* sets (compressors.py:64-178). */
typedef struct {
    int32_t codec;          /* flc_codec */
    int32_t s;              /* dithering: number of level intervals (levels has s+1 entries) */
    int32_t norm;           /* dithering: FLC_NORM_* */
    int32_t flags;          /* execution hints (FLC_PATH_*, FLC_ROW_GROUPS), 0 = library default */
    int64_t k;              /* randk / topk: K */
    float lazy_p;           /* lazy: P */
    float randk_scale;      /* randk: (float)(D / K) as the reference's fp32 scalar multiply */
    const float* d_levels;  /* dithering: s+1 fp32 levels (Compressor.levelsValues) on device */
    uint64_t seed;          /* device-RNG mode: experiment key of the counter-based generator */
    int32_t tie;            /* topk: which of the entries tied at the K-th magnitude are kept when
                               fewer places are left than ties (compressors.py:332 leaves it to
                               torch.topk): FLC_TIE_LOWEST (0, the lowest indices: torch.topk's CPU
                               order on the reference's rows, the oracle's rule) or FLC_TIE_HIGHEST.
                               A result, not a hint: the two rules give different sets on tied rows. */
} flc_codec_params;

#define FLC_TIE_LOWEST 0
#define FLC_TIE_HIGHEST 1

/* Patterns: where the randomness of one call comes from (generateCompressPattern, 196-216).
 * Compat mode reproduces the reference's numpy stream bit for bit (host-drawn, uploaded);
 * device mode draws from a counter-based generator keyed by (seed, client id, element). */
typedef struct {
    const int64_t* d_randk_idx; /* randk compat: [n][k] int64 indices (numpy choice(D,K)) or NULL */
    const double* d_uniforms;   /* natural / dithering compat: [n][d] float64 (numpy rand(D)) or NULL */
    const double* d_lazy_u;     /* lazy: [n] float64 draws (numpy random()) on device — required */
    int64_t client0;            /* device mode: id of row 0 (row r is client client0 + r) */
    int64_t uniforms_ld;        /* leading dimension of d_uniforms (elements); 0 = d */
    int64_t idx_ld;             /* leading dimension of d_randk_idx (elements); 0 = k */
    const uint32_t* d_randk_counts; /* randk device mode: the rows' chunk counts [ceil(d/4096)][n]
                                   * from flc_device_randk_counts with the same seed, client0, n, d,
                                   * k (e.g. computed on another stream, beside other work), or
                                   * NULL: computed inside the call */
} flc_pattern;

/* ----------------------------------------------------------------------------------------
 * Library info / errors
 * -------------------------------------------------------------------------------------- */
int flc_version(void);                    /* ABI version (major*100 + minor) */
/* Build provenance: the first 16 hex digits of sha256 over the library's sources (csrc: .hip,
 * .hpp and .cpp files in name order, then csrc/Makefile and this header), fixed at build time; "+x" is
 * appended when extra compile flags (XFLAGS) were given.  flpytorch_amd._lib.source_hash()
 * computes the same digest from a tree, so a stale .so is detected before it is measured. */
const char* flc_build_id(void);
const char* flc_last_error_string(void);  /* thread-local detail of the last failure */

/* ----------------------------------------------------------------------------------------
 * N-way reduction — the serverGradient core (algorithms.py:1753-1768).
 *
 *   mode FLC_REDUCE_REL_X : out = (sum_i w_i * (x - row_i)) / w_total      (client models in)
 *   mode FLC_REDUCE_PLAIN : out = (sum_i w_i * row_i) / w_total            (client updates in)
 *
 * Summed per element strictly in row order with fp32 rounding after every operation, i.e.
 * bit-identical to the reference's sequential loop (gs = w0*g0; gs += wi*gi; gs / w_total).
 * d_w: n fp32 weights (the reference's python-float weights as fp32), or NULL for all 1.0.
 * w_total: the python-float sum of the weights, as the fp32 divisor.
 * Rows come either as a device array of n row pointers (flc_reduce_rows; every row pointer,
 * d_x and d_out 16-byte aligned) or as one strided matrix (flc_reduce_matrix, row i at
 * d_rows + i*ld; any alignment, the vector path needs 16-byte rows and ld % 4 == 0).
 * -------------------------------------------------------------------------------------- */
#define FLC_REDUCE_PLAIN 0
#define FLC_REDUCE_REL_X 1
int flc_reduce_rows(const float* const* d_row_ptrs, int64_t n, int64_t d, const float* d_x,
                    const float* d_w, float w_total, int mode, float* d_out, void* stream);
int flc_reduce_matrix(const float* d_rows, int64_t ld, int64_t n, int64_t d, const float* d_x,
                      const float* d_w, float w_total, int mode, float* d_out, void* stream);

/* ----------------------------------------------------------------------------------------
 * Single-vector encode — Compressor.compressVector(x) (compressors.py:218-371): dense fp32
 * output `d_out[d]` (zeros where the codec sends nothing).  `row` selects pattern row 0.
 *   d_pnorm_in : dithering only — device fp32 norm to use instead of computing one (the norm
 *                the server receives on the wire), or NULL.  A NaN element under a finite given
 *                norm encodes to +0, the reference's bits (torch.sign(NaN) is 0), whatever the
 *                NaN's sign; an element above the norm (y > 1) lies in no interval: +-0.  Under
 *                an inf or NaN norm every element is NaN, zeros included (0 * 0 * pnorm)
 *   d_pnorm_out: dithering only — device fp32 where the norm used is written, or NULL
 * -------------------------------------------------------------------------------------- */
size_t flc_encode_workspace_size(const flc_codec_params* prm, int64_t d);
int flc_encode(const flc_codec_params* prm, const flc_pattern* pat, const float* d_x, int64_t d,
               const float* d_pnorm_in, float* d_pnorm_out, float* d_out, void* d_ws,
               size_t ws_bytes, void* stream);

/* Rows per flc_encode_reduce / flc_unpack_reduce call (larger rounds: fold the row blocks as
 * partials with w_total = 1 and combine them, as the multi-GPU path does). */
#define FLC_MAX_ROWS 65535

/* ----------------------------------------------------------------------------------------
 * Fused batch encode + reduce — the simulated uplink of one round in one call:
 *     out = (sum_i w_i * C_i(row_i)) / w_total
 * with C_i the codec applied to client row i under its own pattern, summed in row order
 * (bit-identical to reducing the dense compressVector outputs sequentially).  Rows are the
 * strided matrix d_rows (row i at d_rows + i*ld, ld % 4 == 0 and 16-byte alignment for the
 * vector path) — or, with d_rows == NULL, the device pointer array d_row_ptrs (every row
 * 16-byte aligned).
 * d_pnorms_out: optional [n] fp32 norms used (dithering).
 * -------------------------------------------------------------------------------------- */
size_t flc_encode_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d);
int flc_encode_reduce(const flc_codec_params* prm, const flc_pattern* pat, const float* d_rows,
                      int64_t ld, const float* const* d_row_ptrs, int64_t n, int64_t d,
                      const float* d_w, float w_total, float* d_pnorms_out, float* d_out,
                      void* d_ws, size_t ws_bytes, void* stream);

/* The same call with the dithering codecs' norms chosen by the caller (ABI 1.04, additive):
 *   d_pnorms_in : [n] device fp32 norms to use instead of computing any — the norms a server
 *                 receives on the wire (flc_encode's d_pnorm_in, per row) — or NULL: compute.
 *                 Dithering codecs only; ignored by the others.
 *   norm_mode   : FLC_NORMMODE_EXACT      the correctly rounded norm (flc_encode_reduce)
 *                 FLC_NORMMODE_TORCH_CPU  p = 2 of standard / natural dithering as the reference
 *                                         computes it: torch.norm(x, p=2) on a CPU fp32 tensor
 *                                         (compressors.py:272 / 303), in torch's reduction order,
 *                                         bit for bit (flc_norm2_torch_cpu_ws per row).  p = inf:
 *                                         the same as EXACT (a maximum has no order); p = 1:
 *                                         FLC_ERR_UNSUPPORTED before any launch.
 * Both selectors at once: FLC_ERR_ARG.  d_pnorms_out reports the norms used in every mode.
 * The workspace size depends on the selectors (norms given: yes / no, and the mode); a smaller
 * workspace is FLC_ERR_WORKSPACE before any launch.  flc_encode_reduce is this call with
 * (NULL, FLC_NORMMODE_EXACT); its results and its workspace size are the same as before.
 * A row whose given norm is outside the bounds the sparse QSGD path sampled is encoded by the
 * dense fold: every norm gives the bits of flc_encode with that d_pnorm_in, reduced in order. */
#define FLC_NORMMODE_EXACT 0
#define FLC_NORMMODE_TORCH_CPU 1
size_t flc_encode_reduce_ex_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d,
                                           int norms_given, int norm_mode);
int flc_encode_reduce_ex(const flc_codec_params* prm, const flc_pattern* pat, const float* d_rows,
                         int64_t ld, const float* const* d_row_ptrs, int64_t n, int64_t d,
                         const float* d_w, float w_total, const float* d_pnorms_in, int norm_mode,
                         float* d_pnorms_out, float* d_out, void* d_ws, size_t ws_bytes,
                         void* stream);

/* ----------------------------------------------------------------------------------------
 * Shift codecs — the client-side update of the compressed algorithms,
 * one client row, with e = C(a - b) never stored for the elementwise codecs:
 *     d_msg       = d_base + e * msg_scale        (e * msg_scale when d_base == NULL)
 *     d_shift_out = d_shift_in + shift_alpha * e
 * each op rounded separately in fp32, like the torch expressions it replaces:
 *   DIANA  m = C(g - h); h = h + alpha * m              algorithms.py:1383-1391
 *          -> a=g, b=h, msg_scale=1, msg=m, shift_in=h, shift_out=h', alpha=(float)alpha
 *   EF21   g_next = g_prev + C(g - g_prev) * mult      algorithms.py:1506-1517
 *          -> a=g, b=g_prev, base=g_prev, msg_scale=(float)mult, msg=g_next
 *   MARINA g_next = g_prev + C(g - g_prev_x)           algorithms.py:537, 691
 *   FRECON / COFIG u = C(g - h); h = h + alpha * u     algorithms.py:1104-1110, 1265-1269
 * C follows prm / pat exactly as in flc_encode (same patterns, same draws).  d_msg or
 * d_shift_out may be NULL (not written), not both; outputs may alias any input (every element
 * is read before it is written, by the same thread).  d_pnorm_out: optional norm of a - b
 * (dithering).
 * -------------------------------------------------------------------------------------- */
size_t flc_encode_shift_workspace_size(const flc_codec_params* prm, int64_t d);
int flc_encode_shift(const flc_codec_params* prm, const flc_pattern* pat, const float* d_a,
                     const float* d_b, int64_t d, float msg_scale, const float* d_base, float* d_msg,
                     float shift_alpha, const float* d_shift_in, float* d_shift_out,
                     float* d_pnorm_out, void* d_ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------
 * Fused shifted uplink — a DIANA / EF21 / MARINA / FRECON / COFIG round of n resident clients in
 * one call (additive: flc_version() stays 104, detect the entry by its symbol):
 *     msg_i  = base_i + C_i(a_i - b_i) * msg_scale          (without a base: C_i(a_i - b_i) * msg_scale)
 *     h_i'   = shift_in_i + shift_alpha * C_i(a_i - b_i)    (when d_shift_out is given)
 *     d_out  = (sum_i w_i * msg_i) / w_total
 * Row i of an operand is at ptr + i * ld (elements).  msg_i and h_i' are exactly the bits
 * flc_encode_shift gives for (a_i, b_i, base_i, shift_in_i) under pattern row i (d_uniforms +
 * i * uniforms_ld, d_randk_idx + i * idx_ld, d_lazy_u[i]) and client client0 + i; d_out is folded
 * in row order with fp32 rounding per operation, the first term assigned, d_w == NULL meaning no
 * multiply: flc_reduce_matrix(FLC_REDUCE_PLAIN) over the stored messages, without storing them.
 * Dithering uses the exactly rounded norm of a_i - b_i, as flc_encode_shift does (no
 * FLC_NORMMODE_TORCH_CPU for shifted steps); d_pnorms_out: optional [n] norms used.
 *   DIANA  a = g, b = shift_in = shift_out = h rows (in place), msg_scale 1, no base, no d_msg
 *   EF21   a = g, b = base = d_msg = g_prev rows (in place), msg_scale = mult
 *   MARINA a = g_cur, b = previous gradients, base = g_prev: ONE shared [d] vector (ldbase == 0)
 * Aliasing: row i of d_msg / d_shift_out may be row i of d_b, d_base or d_shift_in (same pointer and
 * leading dimension); any other overlap of an output with an operand is the caller's error.
 *
 * Elementwise codecs (ident, lazy, natural, standard / natural dithering): ONE pass — a_i and b_i
 * read once (after the norm pass over a_i - b_i for dithering), h_i' / msg_i written once, the sum
 * kept in registers: 12 n d bytes for an in-place DIANA round (20 n d with the norm pass) against
 * 20 / 28 n d for n flc_encode_shift calls and a fold of their stored messages.  The vector path
 * needs every operand 16-byte aligned with ld % 4 == 0; anything else runs the scalar kernel
 * (same bits).
 * RandK / TopK / Rank-K select or factor the whole difference: their rows run in order through
 * flc_encode_shift's path into a workspace row (or d_msg row i), each followed by a fold step into
 * d_out.  Correct and bounded in workspace (one message row + flc_encode_shift's own), NOT a fast
 * path: n selection passes and 2 n small launches.  d_randk_counts is ignored there.  RandK rounds
 * that store nothing or update in place have a sparse entry, flc_randk_shift_reduce below, and TopK
 * rounds of the same shapes a batched one, flc_topk_shift_reduce.
 *
 * Checked before any launch — FLC_ERR_ARG: null rows / d_a / d_b / d_out with n * d > 0,
 * n > FLC_MAX_ROWS, d_shift_out without d_shift_in, an output operand whose rows overlap
 * (|ld| < d, n > 1), d_msg or d_shift_out overlapping a shared base (the fold always consumes a
 * base, so "base without a consumer" cannot occur here); FLC_ERR_WORKSPACE: ws_bytes below
 * flc_encode_shift_reduce_workspace_size; FLC_ERR_UNSUPPORTED: unknown codec.  n == 0 or d == 0:
 * FLC_OK, the device is not touched (no clients: d_out is the caller's to zero).
 * -------------------------------------------------------------------------------------- */
typedef struct {
    const float* d_a;    int64_t lda;     /* [n] rows a_i (local gradients) */
    const float* d_b;    int64_t ldb;     /* [n] rows b_i (shift h_i / g_prev_i / previous gradient) */
    const float* d_base; int64_t ldbase;  /* NULL; or [n] rows; or ldbase == 0: ONE shared [d] vector (MARINA's g_prev) */
    float msg_scale;
    float* d_msg;        int64_t ldmsg;   /* NULL: messages are not stored; else [n] rows (EF21's g_next, may be d_b/d_base rows) */
    float shift_alpha;
    const float* d_shift_in; int64_t ldin;   /* NULL or [n] rows */
    float* d_shift_out;      int64_t ldout;  /* NULL or [n] rows (may be the d_shift_in / d_b rows: in place) */
} flc_shift_rows;

size_t flc_encode_shift_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d);
int flc_encode_shift_reduce(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows* rows,
                            int64_t n, int64_t d, const float* d_w, float w_total, float* d_pnorms_out,
                            float* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------
 * Sparse in-place RandK round (additive: flc_version() stays 104, detect the entry by its symbol).
 * RandK's index set does not depend on the data, so of a shifted round only the K selected
 * elements of a row are ever needed.  This entry computes flc_encode_shift_reduce's round for
 * FLC_RANDK with work proportional to n K (plus the 128-B line granularity of the gathers), not
 * n d, and writes an in-place operand at the selected elements only.  Arithmetic, each operation
 * rounded separately, in this order:
 *     v = a_i[j] - b_i[j];  e = randk_scale * v;  t = e * msg_scale;  m = base ? base[j] + t : t;
 *     h' = shift_in[j] + shift_alpha * e
 * d_out is folded in row order, the first term assigned, d_w == NULL meaning no multiply, one
 * division by w_total at the end.  Draws as for flc_encode_shift_reduce: d_randk_idx (+ idx_ld)
 * int64 rows of K indices, distinct and below d (the caller's contract, numpy's choice without
 * replacement; an index >= d is never stored to), or device draws from (seed, client0 + i), with
 * d_randk_counts ([ceil(d / 4096)][n], flc_device_randk_counts) honoured when given.
 *
 * THE SHAPE TABLE of the sparse rounds (this entry, flc_topk_shift_reduce and
 * flc_dither_shift_reduce; stated here once).  Accepted shapes, recognised by pointer and leading
 * dimension:
 *   A  DIANA / FRECON / COFIG in place: no base, no d_msg, d_shift_in == d_shift_out == d_b with
 *      equal leading dimensions.  Only row i's K selected elements of h_i are read and written;
 *      d_out is the fold of the sparse messages.
 *   B  EF21 in place: d_base == d_msg == d_b with equal leading dimensions, no shift.  Only the K
 *      selected elements of g_prev_i are written; d_out is then the dense fold of the updated rows
 *      (flc_reduce_matrix's pass on the same stream: 4 n d bytes read).
 *   C  MARINA: ONE shared [d] base (ldbase == 0), no d_msg, no shift.  d_out is the fold of
 *      base + t_i; a row that did not select column j contributes exactly
 *      w_i * (base[j] + 0.0f * msg_scale) (evaluated, not skipped).  No row is read outside its set.
 *   D  the plain fold of C_i(a_i - b_i) * msg_scale: no base, no d_msg, no shift.
 *
 * THE CONTRACT that makes this an entry of its own: elements of an in-place operand (h_i in A,
 * g_prev_i in B) OUTSIDE row i's index set are NOT WRITTEN.  flc_encode_shift_reduce stores
 * x + (+0) there, which is x for every float except -0, which becomes +0.  Therefore
 *   - every element of h_i' / g_next_i that row i selected has exactly flc_encode_shift's bits;
 *   - every other element keeps its stored bits;
 *   - if the in-place operand holds no -0 at an unselected place, the rows and d_out are
 *     bit-identical to flc_encode_shift_reduce's.  That is the case whenever the operand started
 *     as +0 and was only ever updated by these steps (a sum is -0 only when both operands are);
 *   - if it does hold one, the row differs from the dense step only in that zero's sign, and in
 *     shape B d_out can differ only in the sign of a zero;
 *   - shapes C and D have no in-place operand: bit-identical to flc_encode_shift_reduce without
 *     condition, the -0 columns of the fold included.
 *
 * FLC_ERR_UNSUPPORTED before any launch (the caller then uses flc_encode_shift_reduce): a codec
 * other than FLC_RANDK; any other operand shape (a dense output matrix, a per-row base that is not
 * d_msg == d_b, a shift not in place over d_b); msg_scale, or shift_alpha with a shift, that is not
 * finite and > 0 (a negative scale would turn the unselected +0 into -0).  FLC_ERR_ARG: null rows /
 * d_a / d_b / d_out with n * d > 0, n > FLC_MAX_ROWS, negative n or d, K < 1 or K > d, in-place rows
 * that overlap (|ldb| < d, n > 1).  FLC_ERR_WORKSPACE: ws_bytes below the size query.  n == 0 or
 * d == 0: FLC_OK, the device is not touched.  A refused call writes nothing.
 *
 * Workspace: no [d]-sized row.  Device draws: the chunk counts [ceil(d / 4096)][n] and the client
 * keys.  Compat: the chunk-bucketed (index, value) lists, n * K entries, and their tables.  `pat` in
 * the size query only tells the two apart (d_randk_idx != NULL: compat; NULL pat: device draws).
 * -------------------------------------------------------------------------------------- */
size_t flc_randk_shift_reduce_workspace_size(const flc_codec_params* prm, const flc_pattern* pat, int64_t n, int64_t d);
int flc_randk_shift_reduce(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows* rows,
                           int64_t n, int64_t d, const float* d_w, float w_total, float* d_out,
                           void* d_ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------
 * Batched TopK shifted round (additive: flc_version() stays 104, detect the entry by its symbol).
 * flc_encode_shift_reduce runs FLC_TOPK row by row: n lone selections, each with a dense encoded
 * row, an epilogue and a fold step (about 48 n d bytes and 6 n launches in series).  This entry
 * computes the same round for all n rows in a constant number of launches: the n differences are
 * formed once into a workspace matrix (k_shift_sub_rows), the many-row TopK selection of
 * flc_encode_reduce runs over that matrix, a sparse epilogue (k_topk_shift_lists) turns every
 * selected entry into its message and in-place update, and the lists are folded: about
 * 16 n d + 4 d bytes for an in-place DIANA round.  No flc_pattern: TopK draws nothing.
 * Arithmetic, each operation rounded separately, in this order:
 *     v = a_i[j] - b_i[j]
 *     S_i = the K indices of largest |v| (key = the bits of |v|, NaN above inf), ties at the K-th
 *           magnitude by prm->tie: exactly the set flc_encode_shift selects for that row
 *     for j in S_i:  e = v;  t = e * msg_scale;  m = base ? base[j] + t : t;
 *                    h' = shift_in[j] + shift_alpha * e
 * d_out is folded in row order, the first term assigned, d_w == NULL meaning no multiply, one
 * division by w_total at the end.
 *
 * Accepted shapes: A, B, C and D of flc_randk_shift_reduce's shape table, with S_i as the row's
 * index set, and THE CONTRACT stated there: elements of an in-place operand outside S_i are NOT
 * WRITTEN, with the same consequences for the bits of the rows and of d_out.
 *
 * FLC_ERR_UNSUPPORTED before any launch (the caller then uses flc_encode_shift_reduce): a codec
 * other than FLC_TOPK (the size query then returns 0); any other operand shape (a dense output
 * matrix, a per-row base that is not d_msg == d_b, a shift not in place over d_b); msg_scale, or
 * shift_alpha with a shift, that is not finite and > 0 (a negative scale would turn the unselected
 * +0 into -0).  FLC_ERR_ARG: null rows / d_a / d_b / d_out with n * d > 0, n > FLC_MAX_ROWS,
 * negative n or d, K < 1 or K > d, d >= 0xFFFFFFFF, an unknown tie rule, in-place rows that overlap
 * (|ldb| < d, n > 1).  FLC_ERR_WORKSPACE: ws_bytes below the size query.  n == 0 or d == 0: FLC_OK,
 * the device is not touched.  A refused call writes nothing.
 *
 * Workspace, in this order: first the selection state exactly as flc_encode_reduce carves it for
 * (FLC_TOPK, n, d, K) at the workspace base — flc_select_row_flags(prm, n, d, d_ws, ...) reports
 * the rows' paths after this call as it does after the fused uplink (bits 1, 2 and 8; the
 * epilogue consumes bit 4) — then the difference matrix [n][ldd], ldd = (d + 3) & ~3, 16-byte
 * aligned.  Size <= flc_encode_reduce_workspace_size(prm, n, d) + 4 n ldd + 1 KiB.
 * -------------------------------------------------------------------------------------- */
size_t flc_topk_shift_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d);
int flc_topk_shift_reduce(const flc_codec_params* prm, const flc_shift_rows* rows, int64_t n, int64_t d,
                          const float* d_w, float w_total, float* d_out,
                          void* d_ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------
 * Partial participation: the three shifted rounds above over SAMPLED client rows (additive:
 * flc_version() stays 104, detect the entries by their symbols).  Of n_total resident clients n take
 * part in a round (the reference's --num-clients-per-round; EF21-PP, PP-MARINA): participant
 * i = 0..n-1, in this order, is client ids[i].  Each _sampled entry is its contiguous sibling with a
 * row map after `rows`; apart from addresses and keys nothing changes:
 *   - a_i is always at d_a + i * lda (this round's gradients);
 *   - an operand whose FLC_IDX_ bit is set in `indexed` is a state matrix of n_total rows addressed
 *     by id: its row for participant i is at ptr + ids[i] * ld.  An operand whose bit is clear is at
 *     ptr + i * ld as in the sibling (MARINA's previous-gradient rows are fresh per round and stay
 *     unindexed).  A shared base (ldbase == 0) is never indexed.  Bits of absent operands are ignored;
 *   - draws and row keys are those of client pat->client0 + ids[i], so a client's device draws do not
 *     depend on the company it keeps in a round;
 *   - compat pattern rows (d_uniforms, d_randk_idx, d_lazy_u), d_w and d_pnorms_out stay in
 *     participant order i;
 *   - the fold runs in participant order, the first term assigned, one division at the end.
 * Row ids[i] of an indexed output and d_out carry exactly the bits flc_encode_shift gives for
 * (a_i, b_{ids[i]}, ...) under client client0 + ids[i], followed by the sequential fold.  Rows of an
 * indexed operand that are not named in ids are neither read nor written.  The sparse and the batched
 * entry keep the shape table (A - D) and THE CONTRACT on untouched elements of
 * flc_randk_shift_reduce word for word.  "In place" now means same pointer, same leading dimension
 * and the same `indexed` bit.
 *
 * Elementwise codecs run the sibling's kernels in their row-mapped instantiations (the id is
 * wave-uniform and read through the scalar cache): an in-place DIANA round moves 12 n d bytes (20 n d
 * with dithering's norm pass) where gathering the state rows, running the contiguous round and
 * scattering them back moves 16 n d more.  RandK / TopK / Rank-K of the general entry run row by row
 * from h_ids (correct, not a fast path).
 *
 * Checked before any launch, a refused call writes nothing — FLC_ERR_ARG: a null map, h_ids or d_ids
 * with n * d > 0; n_total < 1 or above 2^31 - 1; an unknown bit in `indexed`; an id outside
 * [0, n_total); duplicate ids when an output operand is indexed; an indexed output whose rows overlap
 * (|ld| < d, n_total > 1); an output with the pointer and leading dimension of an operand whose
 * `indexed` bit differs from its own; FLC_IDX_BASE with a shared base (ldbase == 0); d_randk_counts
 * given to flc_randk_shift_reduce_sampled (there is no id-keyed form of flc_device_randk_counts; the
 * entry computes its counts itself).  Every check of the contiguous sibling applies unchanged
 * (FLC_ERR_UNSUPPORTED and FLC_ERR_WORKSPACE included, the latter against the _sampled size query).
 * n == 0 or d == 0: FLC_OK, the device is not touched.  h_ids is read only during the call; d_ids by
 * the kernels, on `stream`.
 * -------------------------------------------------------------------------------------- */
#define FLC_IDX_B 1
#define FLC_IDX_BASE 2
#define FLC_IDX_MSG 4
#define FLC_IDX_SHIFT_IN 8
#define FLC_IDX_SHIFT_OUT 16
typedef struct {
    const int32_t* h_ids;  /* host [n]: checked before any launch; drives the row-at-a-time paths */
    const int32_t* d_ids;  /* device [n]: the same values, read by the kernels */
    int64_t n_total;       /* rows of every indexed operand; every id in [0, n_total) */
    uint32_t indexed;      /* which per-row operands are state matrices addressed by id */
} flc_row_map;

size_t flc_encode_shift_reduce_sampled_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d);
int flc_encode_shift_reduce_sampled(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows* rows,
                                    const flc_row_map* map, int64_t n, int64_t d, const float* d_w, float w_total,
                                    float* d_pnorms_out, float* d_out, void* d_ws, size_t ws_bytes, void* stream);
size_t flc_randk_shift_reduce_sampled_workspace_size(const flc_codec_params* prm, const flc_pattern* pat, int64_t n,
                                                     int64_t d);
int flc_randk_shift_reduce_sampled(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows* rows,
                                   const flc_row_map* map, int64_t n, int64_t d, const float* d_w, float w_total,
                                   float* d_out, void* d_ws, size_t ws_bytes, void* stream);
size_t flc_topk_shift_reduce_sampled_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d);
int flc_topk_shift_reduce_sampled(const flc_codec_params* prm, const flc_shift_rows* rows, const flc_row_map* map,
                                  int64_t n, int64_t d, const float* d_w, float w_total, float* d_out,
                                  void* d_ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------
 * One-read QSGD shifted round (additive: flc_version() stays 104, detect the entry by its symbol).
 * flc_encode_shift_reduce runs FLC_STD_DITHERING in two full reads: the norms of the n differences
 * (8 n d bytes), then the encode, which also stores every element of an in-place operand (12 n d
 * bytes for DIANA in place).  This entry runs the round through the sparse QSGD pipeline of
 * flc_encode_reduce with the difference a_i - b_i as its row: a and b are read once (norm and
 * candidates in the same pass), and because C(v) is sparse the in-place operand is gathered and
 * written at the nonzero elements only: 8 n d + 4 d bytes algorithmically for DIANA in place.
 * Semantics are flc_encode_shift_reduce's for FLC_STD_DITHERING, FLC_NORM_L2, device draws, each
 * operation rounded separately, in this order:
 *     v = a_i[j] - b_i[j];  e = C_i(v);  t = e * msg_scale;  m = base ? base[j] + t : t;
 *     h' = shift_in[j] + shift_alpha * e
 * with the draws and row key of (prm->seed, pat->client0 + i) and the exactly rounded norm (the
 * float64 sum of squares of v in a fixed order, rounded once; d_pnorms_out[n] receives it when not
 * NULL).  d_out is folded in row order, the first term assigned, d_w == NULL meaning no multiply,
 * one division by w_total at the end.
 *
 * Accepted shapes: A, B and D of flc_randk_shift_reduce's shape table, with msg_scale == 1.0f in A
 * and D (the messages themselves are folded; B takes any finite msg_scale > 0).  C, MARINA's one
 * shared base, is refused: its fold needs the (index, value) list form.
 *
 * THE CONTRACT is flc_randk_shift_reduce's with "selected" read as "e is nonzero": an element of
 * the in-place operand whose encoded value is +-0 is NOT WRITTEN (flc_encode_shift_reduce stores
 * x + 0 there: x for every float except -0); every written element has exactly flc_encode_shift's
 * bits; if the operand holds no -0 where e is zero, the rows and d_out are bit-identical to
 * flc_encode_shift_reduce's; shape D is identical without condition.
 *
 * FLC_ERR_UNSUPPORTED, decided on the host before any launch (the call writes nothing; the caller
 * uses flc_encode_shift_reduce): a codec other than FLC_STD_DITHERING or a norm other than
 * FLC_NORM_L2 (the size query then returns 0); pat->d_uniforms given (compat draws); the sparse
 * path not taken for (prm, n, d) — FLC_PATH_DENSE, or no path hint and a candidate share
 * 1.1 s / sqrt(d) + 0.003 past the staging capacity (FLC_PATH_SPARSE forces the path); shape C or
 * any other operand shape; msg_scale != 1 in A or D; msg_scale, or shift_alpha with a shift, that
 * is not finite and > 0.  FLC_ERR_ARG: null rows / d_a / d_b / d_out with n * d > 0, negative n or
 * d, n > FLC_MAX_ROWS, d >= 0x7FFFFFFF, d_shift_out without d_shift_in, in-place rows that overlap
 * (|ldb| < d, n > 1).  FLC_ERR_WORKSPACE: ws_bytes below the size query.  n == 0 or d == 0: FLC_OK,
 * the device is not touched.
 *
 * Workspace: the sparse pipeline's state exactly as flc_encode_reduce carves it for (n, d), at the
 * workspace base; no [n][d] matrix and no [d] message row.  A row whose norm falls outside its
 * sampled bounds, or whose candidates overflow an item's staging, is flagged dense and takes the
 * dense forms of the fold and of the epilogue: same bits, same contract.
 * flc_dither_row_flags (test hook, no compute) copies the per-row flag words this entry left in
 * d_ws — called with the same n and d — into d_flags[n] (device, on `stream`): bit 1 the row was
 * folded dense, bit 4 its norm lies in the fast-division window.
 * -------------------------------------------------------------------------------------- */
size_t flc_dither_shift_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d);
int flc_dither_shift_reduce(const flc_codec_params* prm, const flc_pattern* pat, const flc_shift_rows* rows,
                            int64_t n, int64_t d, const float* d_w, float w_total, float* d_pnorms_out,
                            float* d_out, void* d_ws, size_t ws_bytes, void* stream);
int flc_dither_row_flags(int64_t n, int64_t d, const void* d_ws, size_t ws_bytes, uint32_t* d_flags, void* stream);

/* ----------------------------------------------------------------------------------------
 * FRECON's two-message uplink — a FRECON round of n resident clients in one call (additive:
 * flc_version() stays 104, detect the entry by its symbol).  The FRECON client sends two messages
 * made from the same gradient under the same pattern (algorithms.py:1104-1119), the server folds
 * both and combines them (1124-1176).  Per row i, under pattern row i and client client0 + i, every
 * operation rounded separately in fp32:
 *     u_i  = C_i(a_i - h_i);   q_i = C_i(a_i - p_i)   (the SAME draws: one generateCompressPattern)
 *     h_i' = h_i + shift_alpha * u_i                   (in place over the h rows)
 *     u_avg = (sum_i w_i * u_i) / w_total;   q_avg = (sum_i w_i * q_i) / w_total
 * Both sums are folded in row order, the first term assigned, d_w == NULL meaning no multiply, one
 * division by w_total at the end.  With a server tail (srv != NULL), in the reference's op order:
 *     t1 = one_minus_lambda * g_server_prev;  t2 = q_avg + t1;  t3 = u_avg + h_prev;
 *     t4 = lambda * t3;  d_result = t2 + t4;  d_h_prev_out = h_prev + alpha_update * u_avg
 * (h_prev' from the OLD h_prev; d_h_prev_out may be d_h_prev, or NULL).  d_u_out / d_q_out receive
 * the two averages: required without srv, optional (NULL) with it.
 *
 * The bits are the library's own: the h rows, u_avg, q_avg and both norm vectors are bit-identical
 * to two flc_encode_shift_reduce calls with the same prm and pat — the in-place DIANA round over
 * (a, h), then the plain fold (no base, no message, no shift) over (a, p).  Dithering encodes each
 * message with the exactly rounded norm of its own difference; d_pnorms_u_out / d_pnorms_q_out:
 * optional [n] norms used (dithering codecs only).
 *
 * One kernel reads a_i, h_i and p_i once per pass and keeps both sums in registers: 16 n d bytes
 * (28 n d with dithering's norm pass, which reads the three operands once for both norm sets)
 * against 20 n d + 16 n d (12 n d + 8 n d without norms) for the two calls.  The vector path needs
 * every operand in use 16-byte aligned with ld % 4 == 0; anything else runs the scalar kernel
 * (same bits).  Compat uniforms (d_uniforms) and device draws are both accepted.
 *
 * FLC_ERR_UNSUPPORTED before any launch: FLC_RANDK, FLC_TOPK, FLC_RANK_K (the caller composes the
 * round from flc_encode_shift_reduce and its sparse / batched siblings) or an unknown codec; the
 * size query then returns 0.  FLC_ERR_ARG: null prm-independent operands (rows, d_a, d_h, d_p, the
 * outputs required above, any of srv's d_g_server_prev / d_h_prev / d_result) with n * d > 0,
 * negative n or d, n > FLC_MAX_ROWS, h rows that overlap (|ldh| < d, n > 1), d_result or
 * d_h_prev_out overlapping any row operand (a, h, p).  FLC_ERR_WORKSPACE: ws_bytes below the size
 * query.  n == 0 or d == 0: FLC_OK, the device is not touched.  A refused call writes nothing.
 * -------------------------------------------------------------------------------------- */
typedef struct {
    const float* d_a; int64_t lda;   /* [n] rows g_i */
    float*       d_h; int64_t ldh;   /* [n] rows h_i, updated IN PLACE: h_i + shift_alpha * u_i */
    const float* d_p; int64_t ldp;   /* [n] rows: the gradient at x_prev */
    float shift_alpha;
} flc_frecon_rows;

typedef struct {                      /* optional server tail, all [d] */
    const float* d_g_server_prev; const float* d_h_prev;
    float lambda, one_minus_lambda;   /* (float)lambda_ and (float)(1.0 - lambda_), the double difference cast once */
    float* d_result;                  /* q_avg + one_minus_lambda * g_server_prev + lambda * (u_avg + h_prev) */
    float alpha_update; float* d_h_prev_out;   /* NULL, or h_prev + alpha_update * u_avg; may be d_h_prev */
} flc_frecon_server;

size_t flc_frecon_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d);
int flc_frecon_reduce(const flc_codec_params* prm, const flc_pattern* pat, const flc_frecon_rows* rows, int64_t n,
                      int64_t d, const float* d_w, float w_total, float* d_pnorms_u_out, float* d_pnorms_q_out,
                      float* d_u_out, float* d_q_out, const flc_frecon_server* srv, void* d_ws, size_t ws_bytes,
                      void* stream);

/* ----------------------------------------------------------------------------------------
 * Wire format: the message a client sends, and the server's decode +
 * reduce straight from the N messages.  The reference counts these bits
 * (last_need_to_send_advance, compressors.py:223-224, 367-368) but moves the dense decoded
 * tensor (comm_socket.py:16-82 pickles it).  One row's payload = 16-B header
 * {u32 format, u32 count, f32 norm, u32 bad} + body, padded to 16 B:
 *   1 F32    ident, lazy, natural dithering                f32[d]
 *   2 Q8     std dithering / qsgd / terngrad, s <= 127     u8[d]: bit 7 sign, bits 0-6 level index
 *   3 Q16    std dithering, s > 127                        u16[d]: bit 15 sign, bits 0-14 level index
 *   4 NAT16  natural                                       u16[d]: bit 15 sign; 0 zero, 0x7FFE inf,
 *                                                          0x7FFF NaN, else k + 16384 for 2^k
 *   5 SPARSE randk, topk                                   u32 idx[K] then f32 val[K] (count used,
 *                                                          ascending idx, the elements not +0)
 *   6 RANKK  rank_k                                        the rank-K' expansion, f32: U'_K (B x K')
 *                                                          then (S V'^T)_K' (K' x A), each 16-B
 *                                                          padded — K' (A + B) values, count = K'
 *                                                          (decoded by the encode's own GEMM)
 * Level code 0 is +0; otherwise value = (levels[idx] * sign) * norm (compressors.py:294-296).
 * flc_unpack(flc_pack(x)) == flc_encode(x) bit for bit at every element that is not a NaN; a NaN
 * element of flc_encode(x) decodes to a NaN (NAT16 and the level codes carry "a NaN", not its
 * bits: 0x7FFF decodes to 0x7FC00000, and a level code's NaN is -0 * norm of a non-finite norm).
 * flc_unpack_reduce(payloads) == flc_encode_reduce(rows) in the same sense.  flc_pack runs the
 * encode (same patterns and draws as flc_encode) and derives the codes from its output (an
 * element x == 0 under an inf or NaN norm is a NaN there, 0 * norm, not code 0).
 * Payloads are 16-byte aligned; strided payload rows
 * (d_payloads + i * ld_bytes, ld_bytes >= flc_payload_bytes, a multiple of 16) or a device
 * array of payload pointers.
 * -------------------------------------------------------------------------------------- */
int64_t flc_payload_bytes(const flc_codec_params* prm, int64_t d);
int flc_payload_format(const flc_codec_params* prm);
size_t flc_pack_workspace_size(const flc_codec_params* prm, int64_t d);
int flc_pack(const flc_codec_params* prm, const flc_pattern* pat, const float* d_x, int64_t d,
             void* d_payload, void* d_ws, size_t ws_bytes, void* stream);
int flc_unpack(const flc_codec_params* prm, const void* d_payload, int64_t d, float* d_out,
               void* stream);
/* Host-side check of a message received from a peer, before it goes to the device: nbytes >=
 * flc_payload_bytes, header format = the codec's, bad = 0, count = d (dense formats) / <= K with
 * strictly ascending indices < d (SPARSE) / the codec's rank (RANKK), level codes <= s (Q8 / Q16).
 * FLC_OK or FLC_ERR_ARG with the reason in flc_last_error_string.  Host memory only; no device work.
 * (The decode kernels also never index outside the row or the level table, whatever the bytes.)
 * Replaces the trust the reference's transport places in pickle.loads of the peer's reply
 * (model_funcs.py:445-452, comm_socket.py:59-82). */
int flc_payload_validate(const flc_codec_params* prm, const void* h_payload, int64_t nbytes, int64_t d);
size_t flc_unpack_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d);
int flc_unpack_reduce(const flc_codec_params* prm, const void* d_payloads, int64_t ld_bytes,
                      const void* const* d_payload_ptrs, int64_t n, int64_t d, const float* d_w,
                      float w_total, float* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------
 * Shifted steps on the wire (additive to ABI 1.04: detect by symbol): the shift codecs' client
 * step e = C(a - b) that EMITS its message, and the server fold of n such messages with the
 * shifted round's semantics.
 *
 * flc_pack_shift — one client row.  v = a - b and e = C(v) exactly as flc_encode_shift forms them
 * (same pattern row, same draws, the exactly rounded norm of a - b for dithering).  d_payload
 * receives exactly the bytes flc_pack writes for the fp32 row x = a - b under the same prm / pat
 * (header with the norm and bad = 0, the codes or the ascending (idx, val) list, zeroed padding):
 * flc_unpack(payload) == e bit for bit.  d_msg = d_base + e * msg_scale (e * msg_scale without a
 * base) and d_shift_out = d_shift_in + shift_alpha * e, each op rounded separately, flc_encode_shift's
 * bits; both are optional (MARINA's client needs the payload only).  d_msg / d_shift_out may alias
 * a, b, base and shift_in as in flc_encode_shift; the payload (16-byte aligned, flc_payload_bytes)
 * must not overlap any operand.  Dense formats (F32 / Q8 / Q16 / NAT16): one pass after the norm
 * pass (k_ew_shift_code: a, b [, base, shift_in] read once; codes, msg, shift_out written once —
 * QSGD with in-place DIANA moves 8 d + 8 d + 4 d + 1 d = 21 d bytes).  SPARSE (RandK / TopK): a - b
 * and the dense e in the workspace, the compaction of flc_pack, then the epilogue — a constant
 * number of launches, not a fast path.  d == 0 writes the empty header, as flc_pack.
 *
 * flc_unpack_shift_reduce — the server.  msg_i = base_i + dec(payload_i) * msg_scale (dec * msg_scale
 * without a base), stored to d_msg row i when given; d_out = (sum_i w_i * msg_i) / w_total folded in
 * row order (first term assigned, d_w == NULL: no multiply, one division at the end).  Row i of
 * d_msg may be row i of d_base (same pointer and leading dimension: EF21's server mirror updated in
 * place); ldbase == 0 is ONE shared [d] base (MARINA's g_prev).  Without base and d_msg and with
 * msg_scale == 1 it is flc_unpack_reduce's fold.  Dense formats: one tile-owner pass
 * (k_unpack_shift_accum; an in-place EF21 mirror with Q8 moves (1 + 4 + 4) n d + 4 d bytes); SPARSE:
 * row by row through a dense workspace row, so the bits are the dense shifted round's.
 *
 * The identity: for any flc_shift_rows round in which nothing is written through a shift operand,
 * flc_pack_shift of each row into payload i followed by flc_unpack_shift_reduce over the n payloads
 * with the same base, msg_scale, d_msg and weights leaves the d_out and the d_msg rows of
 * flc_encode_shift_reduce, bit for bit (compat and device draws, -0 columns included).
 *
 * Checked before any launch; a refused call writes nothing.  FLC_ERR_ARG: null a / b / payload /
 * out with work to do, d < 0 or n < 0, a payload that is not 16-byte aligned, ld_bytes <
 * flc_payload_bytes or ld_bytes % 16 != 0, d_shift_out without d_shift_in, d_base without d_msg
 * (client entry), d_msg rows that overlap (|ldmsg| < d with n > 1), d_msg overlapping a shared base.
 * FLC_ERR_UNSUPPORTED (reason in flc_last_error_string): an unknown codec, FLC_RANK_K (its factors
 * are not carried by shifted steps), n > FLC_MAX_ROWS.  FLC_ERR_WORKSPACE: ws_bytes below the size
 * query (0 for an unknown codec, a negative size or Rank-K).  Server: d == 0 returns FLC_OK without
 * touching the device; n == 0 with d > 0 zero-fills d_out.
 * -------------------------------------------------------------------------------------- */
size_t flc_pack_shift_workspace_size(const flc_codec_params* prm, int64_t d);
int flc_pack_shift(const flc_codec_params* prm, const flc_pattern* pat,
                   const float* d_a, const float* d_b, int64_t d,
                   float msg_scale, const float* d_base, float* d_msg,
                   float shift_alpha, const float* d_shift_in, float* d_shift_out,
                   void* d_payload, void* d_ws, size_t ws_bytes, void* stream);

typedef struct {
    const void* d_payloads; int64_t ld_bytes;   /* strided payload rows, or NULL with ...          */
    const void* const* d_payload_ptrs;          /* ... a device array of n payload pointers         */
    float msg_scale;
    const float* d_base; int64_t ldbase;        /* NULL; [n] rows; or ldbase == 0: ONE shared [d]   */
    float* d_msg;        int64_t ldmsg;         /* NULL, or [n] rows (may be the d_base rows)       */
} flc_payload_rows;
size_t flc_unpack_shift_reduce_workspace_size(const flc_codec_params* prm, int64_t n, int64_t d);
int flc_unpack_shift_reduce(const flc_codec_params* prm, const flc_payload_rows* rows,
                            int64_t n, int64_t d, const float* d_w, float w_total,
                            float* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------
 * Multi-GPU combine on a caller-owned RCCL communicator (rccl_comm: an ncclComm_t, passed as
 * void* so no RCCL type crosses the boundary).  Each rank's d_partial holds the client-order
 * partial sum of its client block (flc_encode_reduce / flc_unpack_reduce with w_total = 1.0);
 * on return every rank holds the global result:
 *   FLC_COMBINE_ALLREDUCE  in-place all-reduce(sum), then / w_total (RCCL's summation order)
 *   FLC_COMBINE_ORDERED    all-gather into d_ws, fixed rank-order fold, / w_total
 *                          (bit-reproducible; d_ws of flc_combine_workspace_size bytes)
 * Replaces the reference's per-client .to(device) gathering into one master thread
 * (thread_pool.py:59, algorithms.py:1756-1763).  Enqueued on stream; no host synchronisation.
 * -------------------------------------------------------------------------------------- */
enum { FLC_COMBINE_ALLREDUCE = 0, FLC_COMBINE_ORDERED = 1 };
size_t flc_combine_workspace_size(void* rccl_comm, int64_t d, int mode);
int flc_combine_partials(void* rccl_comm, float* d_partial, int64_t d, float w_total, int mode,
                         void* d_ws, size_t ws_bytes, void* stream);

/* G-invariant combine (SURVEY §8e "combine the 8 block partials in fixed order"): the round's
 * clients fall into fixed contiguous blocks (8 in flpytorch_amd.sharding), split evenly over the
 * ranks in rank order; d_blocks holds this rank's nb_local exact block partials (rows ld floats
 * apart, block order).  On return every rank's d_out = (((B_0 + B_1) + ...) + B_last) / w_total
 * over ALL blocks — the same bits for any rank count.  All-to-all of column slices (grouped
 * ncclSend/ncclRecv), a block-order fold of the rank's slice, ncclAllGather: per rank
 * ~2 (G-1)/G x 4 D bytes with one block per rank.  Every rank must pass the same nb_local and d.
 * Replaces the same reference code as flc_combine_partials. */
size_t flc_combine_blocks_workspace_size(void* rccl_comm, int64_t nb_local, int64_t d);
int flc_combine_blocks(void* rccl_comm, const float* d_blocks, int64_t ld, int64_t nb_local, int64_t d,
                       float w_total, float* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------
 * Host side of compat mode: the numpy legacy MT19937 stream (what the reference's
 * rndgen.choice / rand / random / randint draw, compressors.py:204-212, algorithms.py:2055),
 * advanced in place on a caller-held state (key[624], pos — numpy's get_state() layout).
 * Each call consumes exactly the draws numpy would, so the caller can hand the state back
 * to its RandomState (set_state) and the experiment stream stays identical.
 * h_scratch for choice: n int64 (the Fisher-Yates array).
 * -------------------------------------------------------------------------------------- */
int flc_mt_choice(uint32_t* h_key, int32_t* h_pos, int64_t n, int64_t k, int64_t* h_out,
                  int64_t* h_scratch);
int flc_mt_rand(uint32_t* h_key, int32_t* h_pos, int64_t n, double* h_out);
int flc_mt_randint31(uint32_t* h_key, int32_t* h_pos, int64_t count, int64_t* h_out);

/* Device-RNG mode, host mirror: the uniform (a multiple of 2^-32) / the RandK index set the
 * kernels draw for (seed, client, element). */
double flc_device_uniform(uint64_t seed, int64_t client, int64_t j);
int flc_device_randk_indices(uint64_t seed, int64_t client, int64_t d, int64_t k, int64_t* h_out);
/* The device sampler's per-chunk member counts of clients client0 .. client0 + n - 1, computed by
 * the kernel the fused RandK path runs (k_randk_counts), into d_counts[C][n] (C = ceil(d / 4096),
 * uint32, chunk-major): the GPU-side check of the sampler against its host mirror and the numpy
 * restatement.  Workspace of flc_device_randk_counts_workspace_size bytes; enqueued on stream. */
size_t flc_device_randk_counts_workspace_size(int64_t n, int64_t d);
int flc_device_randk_counts(uint64_t seed, int64_t client0, int64_t n, int64_t d, int64_t k, uint32_t* d_counts,
                            void* d_ws, size_t ws_bytes, void* stream);

/* The fp32 2-norm of each of n rows (row i at d_rows + i*ld) in torch's CPU reduction order —
 * the norm the reference computes, compressors.py:272 `torch.norm(x, p=2)` on a CPU fp32
 * tensor, bit for bit ON AN x86 HOST WITH AVX2 (torch 2.10's AVX2 Vectorized<float> of 8 lanes —
 * the norm kernel has no AVX512 registration, so AVX512 hosts run it too: 8 lane accumulators of
 * fused multiply-adds summed left to right, the D % 8 tail added in order, then the correctly
 * rounded sqrt; oracle/torch_norm.c, pinned by tests/golden/rows.json at D = 25 M and against
 * torch on an AVX512 host by tests/test_host.py).  A torch without AVX2 kernels (DEFAULT
 * capability, non-x86) sums in another lane count: parity there is unpinned.  Not exactly rounded (14 616 ulp below
 * the exact norm at D = 25 M); hand it to flc_encode's d_pnorm_in to get the reference's dithering
 * bits (standard and natural dithering, compressors.py:272 / 303).  Each row is D / 8 dependent
 * fmas per lane: latency-bound (a parity mode; bench.py --dropin --norm-mode torch_cpu prices it). */
int flc_norm2_torch_cpu(const float* d_rows, int64_t ld, int64_t n, int64_t d, float* d_out, void* stream);

/* The same norms, bit for bit, without the chain (ABI 1.03): while a lane's accumulator stays in
 * one binade its rounding grid is fixed, so each step is A -> A + D(A mod 2) on that grid (two
 * integers; the parity carries ties-to-even) and runs of steps compose associatively; the steps
 * that cross a binade are taken as real fmas (torch_norm.hip).  Three launches, a workspace of
 * flc_norm2_torch_cpu_workspace_size(n, d) bytes (per row ~24 bytes per 4096 elements); n <= 65535. */
size_t flc_norm2_torch_cpu_workspace_size(int64_t n, int64_t d);
int flc_norm2_torch_cpu_ws(const float* d_rows, int64_t ld, int64_t n, int64_t d, float* d_out, void* d_ws,
                           size_t ws_bytes, void* stream);

/* Self-test of the exact fast fp32 division the dithering kernels use: for each of the n
 * device divisors, every float numerator in [2^-80, 2^80] is divided both ways and the
 * mismatches are written to d_mismatches[n] (device).  Must be all zero. */
int flc_selftest_division(const float* d_divisors, int n, unsigned long long* d_mismatches, void* stream);

/* ----------------------------------------------------------------------------------------
 * Kernel timing (off by default).  While enabled, every launch of the named hot kernels is
 * bracketed by hipEvents recorded on the launch stream; flc_profile_collect() waits for them
 * and returns the summed duration and launch count for one kernel name, then forgets them.
 * Names: k_topk_filter, k_topk_sample, k_radix_hist, k_chunk_accum, k_ew_accum_vec,
 * k_norm_partials, k_reduce_vec, k_randk_scatter, k_ew_shift (flc_encode_shift's elementwise pass),
 * k_ew_shift_accum (flc_encode_shift_reduce's: one record per call), k_randk_shift (flc_randk_shift_reduce
 * with device draws: one record per call), k_randk_shift_lists (its compat epilogue, one per call),
 * k_shift_sub_rows and k_topk_shift_lists (flc_topk_shift_reduce's difference pass and sparse epilogue:
 * one record each per call), k_ds_sample / k_ds_filter / k_ds_final / k_ds_resolve / k_ds_accum (the sparse QSGD
 * pipeline, one record per launch), k_ds_shift_lists and k_ds_shift_dense_rows (flc_dither_shift_reduce's
 * sparse and dense-row epilogues: one record each per call in shapes A and B), k_ew_shift_code
 * (flc_pack_shift's one pass over a dense format: one record per call) and k_unpack_shift_accum
 * (flc_unpack_shift_reduce's tile-owner pass over a dense format: one record per call);
 * the TopK filter's variant is recorded too
 * (k_topk_filter_g4: 4-chunk work items, the many-row path of large launches; k_topk_filter_g2:
 * 2-chunk items), so a test can assert which one ran.
 * -------------------------------------------------------------------------------------- */
int flc_profile_enable(int on);
int flc_profile_collect(const char* kernel, double* h_total_ms, int64_t* h_launches);

/* Path report of the last TopK selection (test hook, no compute): copies the per-row state
 * words the previous flc_encode_reduce / flc_encode (TopK) left in d_workspace — called with the
 * same params, n and d — into d_flags[n] (device, on `stream`).  Bits: 1 the candidate list
 * overflowed, 2 it came up short, 4 ambiguous ties at the K-th key resolved on the fast path,
 * 8 the row was selected by the exact path (the fast path failed — bits 1 / 2 then say why — or
 * K > D/16), 16 a lone compressVector row (flc_encode, n = 1) selected exactly in registers in one
 * launch (rows up to 16 float4 x 4096 x the device's CUs; 4 then marks a tie cut), 32 (with 16)
 * that launch's grid was not co-resident — a grid wait gave up, the call was aborted and its last
 * workgroup re-selected the row exactly (same result).  Rows that stayed on the fast path read 0
 * or 4.  (Replaces nothing in the reference: compressors.py:330-335 has one path.) */
int flc_select_row_flags(const flc_codec_params* prm, int64_t n, int64_t d, const void* d_workspace,
                         size_t ws_bytes, uint32_t* d_flags, void* stream);

/* Host helper (no compute; the compute entries still never allocate): storage for the resident
 * client-update matrix.  contiguous != 0: physically contiguous HBM (hipDeviceMallocContiguous) —
 * a default allocation of tens of GB is stitched from fragments and some of its rows read 6-10 %
 * slower with more address-translation misses; contiguous memory maps with the largest fragments
 * (C4's shard: plain read 8.04 vs 8.48 ms, encode+reduce step 9.09 vs 9.57 ms, one process).
 * FLC_ERR_HIP when the allocation fails (e.g. no contiguous range that large is free): the caller
 * may fall back to contiguous = 0.  Free with flc_rows_free.  (The reference keeps its N client
 * tensors wherever torch puts them, model_funcs.py:367-386.) */
int flc_rows_alloc(size_t bytes, int contiguous, void** d_ptr);
int flc_rows_free(void* d_ptr);

/* Test hook of the lone-TopK resident selection (no compute): the next resident launches of this
 * process use grid_mult x their grid (grid_mult > 1: more 1024-thread workgroups than can be
 * resident at once, so the call's grid waits give up and its abort + exact repair path runs) and
 * give up a grid wait after spin_ticks of the 100 MHz clock (0: the default, 0.1 s).
 * flc_debug_resident(1, 0) restores the defaults.  FLC_ERR_ARG outside grid_mult 1..64,
 * spin_ticks >= 0.  (Replaces nothing in the reference.) */
int flc_debug_resident(int grid_mult, int64_t spin_ticks);

#ifdef __cplusplus
}
#endif
#endif /* FLCODEC_H */
