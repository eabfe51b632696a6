/* Host side of flc_unpack_shift_reduce_sparse from C: every refusal is decided before any launch, so
 * made-up device addresses are enough.  Built and run by tests/test_sparse_shift_wire_host.py; its
 * own main, so the host-side argument checking can also be run under a sanitizer build. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "flcodec.h"

#define D 4099
#define CHECK(expr, want) if ((expr) != (want)) { printf("line %d: %s is not %s\n", __LINE__, #expr, #want); return 1; }

static int call(const flc_codec_params* prm, const flc_payload_rows* r, const flc_row_map* map, int64_t n, size_t ws) {
    return flc_unpack_shift_reduce_sparse(prm, r, map, n, D, NULL, 1.f, (float*)0x50000000, (void*)0x60000000, ws, NULL);
}

int main(void) {
    float* const base = (float*)0x30000000;
    const size_t big = (size_t)1 << 40;
    const float scales[4] = {0.f, -1.f, INFINITY, NAN};
    flc_codec_params prm, dense;
    flc_payload_rows ok, r;
    memset(&prm, 0, sizeof(prm));
    memset(&ok, 0, sizeof(ok));
    prm.codec = FLC_TOPK;
    prm.k = 10;
    dense = prm;
    dense.codec = FLC_NATURAL;
    ok.d_payloads = (void*)0x78000000;
    ok.ld_bytes = flc_payload_bytes(&prm, D);
    ok.msg_scale = 1.f;
    CHECK(flc_unpack_shift_reduce_sparse_workspace_size(&prm, 2, D), 256)
    CHECK(flc_unpack_shift_reduce_sparse_workspace_size(&dense, 2, D), 0)
    CHECK(call(&dense, &ok, NULL, 2, big), FLC_ERR_UNSUPPORTED)
    r = ok;
    r.d_base = base; r.ldbase = D; r.d_msg = base + 0x1000000; r.ldmsg = D;   /* a separate dense d_msg */
    CHECK(call(&prm, &r, NULL, 2, big), FLC_ERR_UNSUPPORTED)
    for (int i = 0; i < 4; ++i) {
        r = ok;
        r.msg_scale = scales[i];
        CHECK(call(&prm, &r, NULL, 2, big), FLC_ERR_UNSUPPORTED)
    }
    r = ok;
    r.ld_bytes -= 16;
    CHECK(call(&prm, &r, NULL, 2, big), FLC_ERR_ARG)
    CHECK(call(&prm, NULL, NULL, 2, big), FLC_ERR_ARG)
    CHECK(call(&prm, &ok, NULL, 65536, big), FLC_ERR_ARG)
    r = ok;
    r.d_base = base; r.ldbase = D - 1; r.d_msg = base; r.ldmsg = D - 1;       /* the mirror rows overlap */
    CHECK(call(&prm, &r, NULL, 2, big), FLC_ERR_ARG)
    r.ldbase = r.ldmsg = D;                                                   /* shape B, up to the last check */
    CHECK(call(&prm, &r, NULL, 2, 0), FLC_ERR_WORKSPACE)
    /* the row map: the checks of the _sampled entries */
    int32_t ids[2] = {5, 0};
    flc_row_map map;
    memset(&map, 0, sizeof(map));
    map.h_ids = ids; map.d_ids = (const int32_t*)0x7C000000; map.n_total = 7; map.indexed = FLC_IDX_BASE | FLC_IDX_MSG;
    CHECK(call(&prm, &r, &map, 2, 0), FLC_ERR_WORKSPACE)
    map.indexed = FLC_IDX_MSG;                                                /* in place, one of the two indexed */
    CHECK(call(&prm, &r, &map, 2, 0), FLC_ERR_ARG)
    map.indexed = FLC_IDX_BASE | FLC_IDX_MSG;
    ids[1] = 7;                                                               /* outside [0, n_total) */
    CHECK(call(&prm, &r, &map, 2, 0), FLC_ERR_ARG)
    ids[1] = 5;                                                               /* twice */
    CHECK(call(&prm, &r, &map, 2, 0), FLC_ERR_ARG)
    ids[1] = 0;
    map.d_ids = NULL;
    CHECK(call(&prm, &r, &map, 2, 0), FLC_ERR_ARG)
    CHECK(flc_unpack_shift_reduce_sparse(&prm, &ok, NULL, 5, 0, NULL, 1.f, NULL, NULL, 0, NULL), FLC_OK)
    printf("sparse shifted-wire refusals OK\n");
    return 0;
}
