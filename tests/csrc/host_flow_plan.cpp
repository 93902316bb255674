// TEST INFRASTRUCTURE: csrc/flow_plan.h compiled for the HOST (tests/test_flow_plan.py replays recorded calls through it).  Not part of
// librnf_hip.so.
#include "../../rotationnormflow_amd/csrc/flow_plan.h"

using namespace rnf;

static void put_key(int64_t *row, const KernelKey &k) {
    const int64_t f[9] = {k.dir, k.kt_inv, k.nw, k.pipe, k.prec, k.ext, k.lean, k.fused, k.rows};
    for (int i = 0; i < 9; ++i) row[i] = f[i];
}

extern "C" {
enum { ROW = 16, MEMSET = 0, PROJECTION = 1, STACK = 2, FINALIZE = 3 };

// call: dir, n, n_layers, segments, feature_dim, feature_div, feature, side, states, sum_out, workspace, workspace_bytes, in_place
// switches: wide, staging_dma, guard, lean, fused, fair, rf_first
// rows [max_rows][ROW]: what, fallback, key[9] (projection: kernel id in key[0]), block, grid, dynamic LDS bytes, chunk, governor offset
// summary: family, ext, rows, prec, fb_prec, guarded, pipe, fused, ws_need, kt_inv, rf_first4, n_slots
// -> number of launches in the order rnf_flow_pass issues them, -1 with `err` filled when the call is refused
int fp_plan(const int32_t *desc, const int64_t *call, int cus, const int32_t *switches, int64_t *rows, int max_rows, int64_t *summary, char *err,
            int err_len) {
    static float something[16];
    static FlowPlan p;
    RnfFlowPass o = {};
    o.struct_bytes = sizeof(o);
    o.dir = (int32_t)call[0]; o.n = call[1]; o.n_layers = (int32_t)call[2]; o.segments = (int32_t)call[3];
    o.feature_dim = (int32_t)call[4]; o.feature_div = call[5];
    o.rotation = something; o.blob = something; o.desc = desc; o.ldj_out = something;
    o.feature = call[6] ? something : nullptr;
    o.side = call[7] ? something : nullptr;
    o.states = call[8] ? something : nullptr;
    o.sum_out = call[9] ? reinterpret_cast<double *>(something) : nullptr;
    o.workspace = call[10] ? something : nullptr;
    o.workspace_bytes = (size_t)call[11];
    o.rotation_out = call[12] ? something : something + 1;
    Switches sw;
    sw.wide = switches[0]; sw.staging_dma = switches[1]; sw.guard = switches[2]; sw.lean = switches[3]; sw.fused = switches[4];
    sw.fair = switches[5]; sw.rf_first = switches[6];
    if (!plan_flow(o, cus, sw, p, err, (size_t)err_len)) return -1;
    int count = 0;
    auto add = [&](int what, bool fb, int chunk, int block, int grid, size_t lds) -> int64_t * {
        if (count >= max_rows) return nullptr;
        int64_t *r = rows + (size_t)count++ * ROW;
        for (int i = 0; i < ROW; ++i) r[i] = 0;
        r[0] = what; r[1] = fb; r[11] = block; r[12] = grid; r[13] = (int64_t)lds; r[14] = chunk; r[15] = -1;
        return r;
    };
    if (p.empty) {
        if (o.sum_out) add(FINALIZE, false, 0, 256, 1, 0);
        for (int i = 0; i < 12; ++i) summary[i] = 0;
        return count;
    }
    const int64_t s[12] = {p.family, p.ext, p.rows, p.prec, p.fb_prec, p.guarded, p.pipe, p.fused, (int64_t)p.ws_need, p.kt_inv, p.rf_first4, p.n_slots};
    for (int i = 0; i < 12; ++i) summary[i] = s[i];
    for_each_launch(p, cus, o.n, o.sum_out != nullptr, [&](const Launch &l) -> int {
        const int chunk = (int)(l.base / p.chunk_cap);
        if (l.kind == LAUNCH_GUARD_RESET) add(MEMSET, false, chunk, 0, 0, 0);
        if (l.kind == LAUNCH_FINALIZE) add(FINALIZE, false, chunk, 256, 1, 0);
        if (l.kind == LAUNCH_PROJECTION) {
            const ProjPlan j = plan_projection(p, cus, l.cn, l.fb);
            if (int64_t *r = add(PROJECTION, l.fb, chunk, j.block, j.grid, j.lds_bytes)) r[2] = j.kernel;
        }
        if (l.kind == LAUNCH_STACK) {
            const KernelKey k = l.fb ? fallback_key(p) : stack_key(p, l.chunk);
            if (int64_t *r = add(STACK, l.fb, chunk, k.nw * 64, l.fb ? l.chunk.grid_fb : l.chunk.grid, l.fb ? p.lds_fb : p.lds_bytes)) {
                put_key(r + 2, k);
                r[15] = l.fb ? -1 : l.chunk.fair_off;
                if (key_index(k) < 0) r[0] = -1;          // a key the dispatcher would refuse
            }
        }
        return 0;
    });
    return count;
}

// the dispatcher's list (flow_plan.h BUILT), [count][9]
int fp_built_keys(int64_t *out) {
    for (int i = 0; i < N_BUILT; ++i) {
        if (key_index(BUILT.k[i]) != i) return -1;        // a key listed twice
        put_key(out + 9 * (size_t)i, BUILT.k[i]);
    }
    return N_BUILT;
}
}
