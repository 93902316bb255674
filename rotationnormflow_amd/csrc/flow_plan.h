// flow_plan.h -- what rnf_flow_pass launches, decided on the host from the descriptor and the call alone (no HIP runtime call in here:
// tests/csrc/host_flow_plan.cpp compiles this header for the CPU and tests/test_flow_plan.py pins the decision against a kernel trace).
//
//   plan_flow(pass, cus, switches)  -> FlowPlan: everything that is the same for every chunk of the call
//   plan_chunk(plan, cus, cn)       -> ChunkPlan: waves per workgroup and grids of a chunk of cn rotations
//   plan_projection(plan, cus, fb)  -> ProjPlan: the feature-projection launch in front of a stack launch
//   for_each_launch(plan, ...)      -> the launches of the call in order (rnf_api.hip issues them, the test lists them)
//   stack_key / fallback_key        -> KernelKey: the instantiation of flow_stack_kernel a launch runs
//   BUILT / key_index(key)          -> THE list of instantiations librnf_hip.so holds (rnf_api.hip builds its kernel table from it)
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/rnf_hip.h"
#include "layout.h"

namespace rnf {

constexpr int NW = 8;                                   // waves per workgroup (2 per SIMD): exact-fp32 and inverse kernels, featproj
constexpr int NW_FWD_H = 8;                             // forward split-precision kernel small launches
constexpr int NW_FWD_NARROW = 4;                        // same kernel, 1 wave per SIMD: launches that leave half of the CUs empty at 8 waves (small
                                                        // batches, training: forward latency 0.41 -> 0.34 ms at 1024 rotations)
constexpr int NW_FWD_WIDE = 16;                         // same kernel, 4 waves per SIMD (fits in 128 VGPRs): launches that fill every CU with
                                                        // 512-rotation workgroups; +12 % over 8 waves (profiles/r1/nw_sweep.txt)
#ifndef RNF_NW_FP
#define RNF_NW_FP 8
#endif
constexpr int NW_INV_BIG = 4;                           // inverse with 64 < K <= 128: one wave per SIMD
constexpr int NW_FP = RNF_NW_FP;                        // waves per workgroup of the feature projection (workgroups per CU: 8 / NW_FP)
#ifndef RNF_NW_FUSED
#define RNF_NW_FUSED 8
#endif
constexpr int NW_FUSED = RNF_NW_FUSED;                  // the FUSED instantiation (projection inside the stack kernel)
#ifndef RNF_CHUNK_LOG2
#define RNF_CHUNK_LOG2 18           // (17 / 16 measured and not better: profiles/r6/ab_chunk_C4.jsonl)
#endif
constexpr long long CHUNK_SAMPLES = 1LL << RNF_CHUNK_LOG2;   // samples per launch when a feature projection scratch is needed
// head of the workspace: [0, 2048) block partials of the primary launch, [2048, 4095) partials of the exact-fp32 re-run, double 4095 =
// two int32: {guard of the current chunk, sticky "a re-run happened in this call"} (flow_kernels.h FlowArgs::guard)
constexpr size_t PARTIALS_BYTES = 4096 * sizeof(double);
constexpr int PARTIALS_FB_AT = 2048, GUARD_AT = 4095;

// Limits and LDS sizes of the kernel headers (which need the device headers), restated; rnf_api.hip asserts that they agree.
namespace klim {
constexpr int MAX_LAYERS = 400, MAX_SLOTS = 224, FP_KCHUNK = 256, FUSED_MAX_F = 256;
constexpr int FUSED_PA_FLOATS = FUSED_MAX_F / 16 * 512 + 32;
constexpr int B3_REGION_FLOATS = 4 * Lay<2>::LAST_TILE_FLOATS;                  // one ring region of the bf16x3 kernels
constexpr size_t FP2_LDS_BYTES = sizeof(float) * (2 * 2 * (FP_KCHUNK / 16) * 512 + 2 * 4 * 64 * 16);
}  // namespace klim

// The environment switches (rnf_api.hip reads each once) and rnf_set_fused, as plain values.
struct Switches {
    bool wide = true;          // RNF_WIDE=0 keeps the forward kernel at 8 waves per workgroup (measurement switch)
    bool staging_dma = true;   // LDS-DMA double-phase prefetch (needs segments <= 64) unless RNF_STAGING=sync
    bool guard = true;         // RNF_GUARD=0: no range guard / fp32 re-run behind split-precision calls (measurement switch)
    bool lean = true;          // RNF_LEAN=0 keeps unconditional Moebius / affine stacks on the general instantiation (measurement switch)
    bool fused = false;        // RNF_FUSED=1 / rnf_set_fused(1), see plan_flow
    bool fair = true;          // RNF_FAIR=0 switches the SIMD fairness governor off
    int rf_first = 0;          // RNF_RF_FIRST=3|4 forces the order of the inverse root finder's first pass; 0: the flow's own
};

// One instantiation flow_stack_kernel<DIR, KT_INV, NW, PIPE, PREC, EXT, LEAN, FUSED, ROWS>.
struct KernelKey {
    int dir, kt_inv, nw;
    bool pipe;
    int prec;
    bool ext;
    int lean;
    bool fused, rows;
};

// THE LIST of instantiations the library holds: 22 forward + 58 inverse = 80 (DESIGN.md section 3.1 explains each family).  rnf_api.hip
// instantiates exactly these, in this order -- which is also the order the kernels are emitted in, and the compiler's register
// allocation of some of them depends on that: append, do not reorder (tools/kernel_resources.py shows the effect).
constexpr int N_BUILT = 80;
struct BuiltKeys {
    KernelKey k[N_BUILT] = {};
    int n = 0;
    constexpr void add(int dir, int kt, int nw, bool pipe, int prec, bool ext, int lean = 0, bool fused = false, bool rows = false) {
        k[n++] = KernelKey{dir, kt, nw, pipe, prec, ext, lean, fused, rows};
    }
};
constexpr BuiltKeys built_keys() {
    BuiltKeys b;
    b.add(0, 0, NW_FUSED, true, 1, false, 2, true);                             // FUSED: projection inside the kernel (opt-in)
    const int kts[5] = {0, 1, 2, 4, 8};                                          // forward, then the inverse with 1, 2, 4, 8 tiles in registers
    for (int kt : kts) {
        const int dir = kt ? 1 : 0;
        b.add(dir, kt, NW, false, 2, true);                                      // bf16x3 stages synchronously (ring)
        b.add(dir, kt, NW, false, 2, false);
        // the fast path (split precision, DMA staging, no extended layer kind) has the narrow / wide workgroups and the families:
        // shared feature rows -- forward on the conditional-lean family only, 4 / 8 / 16 waves; inverse 4 / 8 waves
        if (!dir) b.add(0, 0, NW_FWD_WIDE, true, 1, false, 2, false, true), b.add(0, 0, NW_FWD_H, true, 1, false, 2, false, true);
        b.add(dir, kt, NW_FWD_NARROW, true, 1, false, dir ? 0 : 2, false, true);
        if (dir) b.add(1, kt, NW, true, 1, false, 0, false, true);
        b.add(dir, kt, NW, true, 1, true);                                       // extended layer kinds: 8 waves, every staging and arithmetic
        b.add(dir, kt, NW, true, 0, true);
        b.add(dir, kt, NW, false, 1, true);
        b.add(dir, kt, NW, false, 0, true);
        for (int lean = 2; !dir && lean >= 1; --lean) {                          // conditional-lean (2) and lean (1) forward families
            b.add(0, 0, NW_FWD_WIDE, true, 1, false, lean);
            b.add(0, 0, NW_FWD_H, true, 1, false, lean);
            b.add(0, 0, NW_FWD_NARROW, true, 1, false, lean);
        }
        if (!dir) b.add(0, 0, NW_FWD_WIDE, true, 1, false);                      // general family: 16 / 4 / 8 waves forward, 4 / 8 inverse
        b.add(dir, kt, NW_FWD_NARROW, true, 1, false);
        b.add(dir, kt, NW, true, 1, false);
        b.add(dir, kt, NW, true, 0, false);                                      // 8 waves for every other staging and arithmetic
        b.add(dir, kt, NW, false, 1, false);
        b.add(dir, kt, NW, false, 0, false);
    }
    b.add(1, 16, NW_INV_BIG, false, 2, true);                                    // 64 < K: 4 waves with the whole register file, synchronous
    b.add(1, 16, NW_INV_BIG, false, 2, false);
    b.add(1, 16, NW_INV_BIG, false, 1, true);
    b.add(1, 16, NW_INV_BIG, false, 0, true);
    b.add(1, 16, NW_INV_BIG, false, 1, false);
    b.add(1, 16, NW_INV_BIG, false, 0, false);
    return b;
}
constexpr BuiltKeys BUILT = built_keys();
static_assert(BUILT.n == N_BUILT, "the list of instantiations and its length disagree");
constexpr int key_index(const KernelKey &q) {            // position in BUILT, -1: no such instantiation
    for (int i = 0; i < N_BUILT; ++i) {
        const KernelKey &k = BUILT.k[i];
        if (k.dir == q.dir && k.kt_inv == q.kt_inv && k.nw == q.nw && k.pipe == q.pipe && k.prec == q.prec && k.ext == q.ext && k.lean == q.lean &&
            k.fused == q.fused && k.rows == q.rows)
            return i;
    }
    return -1;
}

struct LayerEntry { int x, y; };                         // FlowArgs::layers

struct FlowPlan {
    bool empty;                              // n == 0: nothing to launch but the finalize of sum_out
    int dir, n_layers, n_slots, K, KT, kt_inv, F;
    LayerEntry layers[klim::MAX_LAYERS];     // x = kind | perm_row << 4 | (cond_slot + 1) << 8 | (position of the next MLP layer + 1) << 16
    int param_fb[klim::MAX_LAYERS];          // y of the exact-fp32 / bf16x3 fallback records of the MLP layers
    int feat_off[klim::MAX_SLOTS], feat_off_fb[klim::MAX_SLOTS];
    int prec, fb_prec;                       // arithmetic of the primary launch and of the guard's re-run
    bool any_mlp, shared, guarded, pipe, ext, ext_fb, rows, fused, wide_ok, rf_first4;
    int family;                              // 0 general, 1 lean, 2 conditional-lean
    int fair_off, tab_off, tab_off_fb, pa_off, feat_stride;
    size_t lds_bytes, lds_fb;                // dynamic LDS of the primary (FUSED: incl. its projection buffer) and of the fallback launch
    size_t ws_need, stash_at;                // workspace the call needs; the K > 128 inverse stash starts at stash_at when ws_need > stash_at
    long long chunk_cap, feat_rows;
};

struct ChunkPlan {
    int nw, fair_off;                        // waves per workgroup of the primary launch; its governor offset (-1: off)
    long long groups;                        // 32-sample groups per cond slot in the projection scratch
    int grid, grid_fb;                       // workgroups of the primary and of the fallback launch
};

enum ProjKernel { PROJ_F16X2_KSPLIT, PROJ_F16X2_KCHUNKS, PROJ_F16X2, PROJ_FP32 };
struct ProjPlan { ProjKernel kernel; int grid, block; size_t lds_bytes; long long rows; };

// cond slots and "has a conditioner MLP" of a descriptor table, validated or not (rnf_flow_pass_workspace_bytes takes any)
inline void desc_slots(const int32_t *desc, int n_layers, int *n_slots, bool *any_mlp) {
    *n_slots = 0;
    *any_mlp = false;
    for (int l = 0; desc && l < n_layers && l < klim::MAX_LAYERS; ++l) {
        const int32_t *d = desc + (size_t)l * D_STRIDE;
        if (d[D_SLOT] + 1 > *n_slots) *n_slots = d[D_SLOT] + 1;
        *any_mlp = *any_mlp || kind_has_mlp(d[D_KIND]);
    }
}
inline bool needs_stash(const RnfFlowPass &p, bool any_mlp) { return p.dir == 1 && any_mlp && (p.segments + 7) / 8 > 16; }

inline size_t conditioner_workspace(long long n, int n_cond_layers) {       // rnf_workspace_bytes
    size_t bytes = PARTIALS_BYTES;
    if (n_cond_layers > 0) {
        long long chunk = n < CHUNK_SAMPLES ? n : CHUNK_SAMPLES;
        long long groups = (chunk + 255) / 256 * 8;     // whole workgroup tiles, for either workgroup size
        const long long g16 = (chunk + 32 * NW_FWD_WIDE - 1) / (32 * NW_FWD_WIDE) * NW_FWD_WIDE;
        if (g16 > groups) groups = g16;
        bytes += (size_t)n_cond_layers * groups * G_FLOATS_PER_GROUP * sizeof(float);
    }
    return bytes;
}

// The workspace rnf_flow_pass requires: the partials block, the feature-projection scratch of n_slots conditional slots -- one 64-float
// record per (slot, feature row) with shared feature rows -- and behind them, from *stash_at on, the per-wave stash of an inverse pass
// with K > 128 (the parameters of 64 segments per lane stay in registers, flow_kernels.h mobius_inv_tiles); `cus` is read for that only.
inline size_t flow_workspace(const RnfFlowPass &p, int n_slots, bool any_mlp, int cus, size_t *stash_at) {
    const bool shared = p.feature_div > 0 && n_slots > 0;
    size_t bytes = shared ? PARTIALS_BYTES + (size_t)n_slots * (size_t)((p.n + p.feature_div - 1) / p.feature_div) * 64 * sizeof(float)
                          : conditioner_workspace(p.n, n_slots);
    *stash_at = bytes;
    if (needs_stash(p, any_mlp)) bytes += (size_t)cus * NW_INV_BIG * (size_t)(4 * ((p.segments + 7) / 8 - 16)) * 64 * 4 * sizeof(float);
    return bytes;
}

// the refusal of a call: its message into `err`, false
inline bool plan_fail(char *err, size_t err_len, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(err, err_len, fmt, ap);
    va_end(ap);
    return false;
}

// Validates the call and its descriptor and decides the launches.  false: `err` holds the message (the caller's rnf_last_error text).
inline bool plan_flow(const RnfFlowPass &o, int cus, const Switches &sw, FlowPlan &p, char *err, size_t err_len) {
    const int32_t *desc = o.desc;
    const long long n = o.n;
    const int F = o.feature_dim, n_layers = o.n_layers, K = o.segments;
    if (n < 0) return plan_fail(err, err_len, "n=%lld is negative", n);
    if (n_layers <= 0 || n_layers > klim::MAX_LAYERS) return plan_fail(err, err_len, "n_layers=%d outside [1,%d]", n_layers, klim::MAX_LAYERS);
    if (K <= 0) return plan_fail(err, err_len, "segments=%d must be positive", K);
    if (!o.blob || !desc || (n > 0 && !o.rotation)) return plan_fail(err, err_len, "null rotation / blob / desc pointer");
    if (o.fisher_A && (o.fisher_B <= 0 || n % o.fisher_B))
        return plan_fail(err, err_len, "n=%lld not divisible by fisher rows B=%lld (utils/fisher.py:226)", n, (long long)o.fisher_B);

    // exact-fp32 images of the same layers in the same blob (desc columns D_PARAM_FB / D_FEAT_FB): a split-precision call is guarded and
    // re-run on them, on the device, when a sample comes out non-finite (an fp16 operand overflowed)
    bool have_fb = !o.states;
    int min_tiles = 1;                       // fc_last tiles the largest non-Moebius record needs resident in LDS
    bool ext_layers = false;                 // the flow contains a layer kind only the extended kernel instantiation carries
    bool all_mlp_cond = true;                // every MLP layer consumes the feature vector (what the FUSED instantiation handles)
    int prec = -1, fb_prec = -1, rf_code = 0;
    bool lean = sw.lean && !o.states;        // Moebius + constant 4x4 affine layers only, nothing conditional, no saved states
    bool lean2 = sw.lean && !o.states;       // the conditional counterpart: + Condition16Trans, every MLP layer conditional (checked below)
    for (int sl = 0; sl < klim::MAX_SLOTS; ++sl) p.feat_off[sl] = 0, p.feat_off_fb[sl] = -1;
    for (int l = 0; l < n_layers; ++l) {
        const int32_t *d = desc + (size_t)l * D_STRIDE;
        const int kind = d[D_KIND], perm = d[D_PERM], slot = d[D_SLOT];
        if (kind < RNF_KIND_MOBIUS || kind > RNF_KIND_LAST) return plan_fail(err, err_len, "layer %d: unknown kind %d", l, kind);
        if (perm < 0 || perm > 5) return plan_fail(err, err_len, "layer %d: perm_row %d outside [0,5]", l, perm);
        if (d[D_PARAM] < 0 || (d[D_PARAM] % 4 && !kind_is_side(kind))) return plan_fail(err, err_len, "layer %d: param offset %d must be a non-negative multiple of 4", l, d[D_PARAM]);
        if ((kind == RNF_KIND_COND16 || kind_is_cond9(kind) || kind == RNF_KIND_COND36) && slot < 0)
            return plan_fail(err, err_len, "layer %d: a conditional affine layer needs a cond_slot", l);
        if (kind_is_cond9(kind) || kind == RNF_KIND_COND36 || kind_is_side(kind)) ext_layers = true;
        if (kind_is_side(kind) && !o.side) return plan_fail(err, err_len, "layer %d takes per-sample matrices: RnfFlowPass.side is null", l);
        if ((kind != RNF_KIND_MOBIUS && kind != RNF_KIND_AFFINE16) || slot >= 0) lean = false;
        if (kind != RNF_KIND_MOBIUS && kind != RNF_KIND_AFFINE16 && kind != RNF_KIND_COND16) lean2 = false;
        if (kind == RNF_KIND_COND36) min_tiles = 2;
        if (slot >= 0) {
            if (slot >= klim::MAX_SLOTS) return plan_fail(err, err_len, "layer %d: cond_slot %d >= %d", l, slot, klim::MAX_SLOTS);
            if (d[D_FEAT] < 0 || d[D_FEAT] % 4) return plan_fail(err, err_len, "layer %d: feat offset %d invalid", l, d[D_FEAT]);
            p.feat_off[slot] = d[D_FEAT];
        }
        p.param_fb[l] = -1;
        if (kind_has_mlp(kind)) {
            if (slot < 0) all_mlp_cond = false;
            if (d[D_PARAM_FB] < 0 || d[D_PARAM_FB] % 4 || (slot >= 0 && (d[D_FEAT_FB] < 0 || d[D_FEAT_FB] % 4))) have_fb = false;
            p.param_fb[l] = d[D_PARAM_FB];
            if (slot >= 0) p.feat_off_fb[slot] = d[D_FEAT_FB];
            const int pr = d[D_PREC] & 255, pfb = (d[D_PREC] >> 8) & 255;     // bits 8..15: arithmetic of the fallback records (0: fp32, 2: bf16x3)
            if (kind == RNF_KIND_MOBIUS) {                                    // bits 16..17: first-pass order of the inverse root finder
                const int rc = (d[D_PREC] >> 16) & 3;
                if (rc == 3) return plan_fail(err, err_len, "layer %d: root-finder order code 3 is reserved", l);
                if (rc > rf_code) rf_code = rc;
            }
            if (pr != RNF_PREC_FP32 && pr != RNF_PREC_F16X2 && pr != RNF_PREC_BF16X3) return plan_fail(err, err_len, "layer %d: unknown precision %d", l, pr);
            if (pfb != RNF_PREC_FP32 && pfb != RNF_PREC_BF16X3) return plan_fail(err, err_len, "layer %d: fallback records must be RNF_PREC_FP32 or RNF_PREC_BF16X3, got %d", l, pfb);
            if (fb_prec >= 0 && pfb != fb_prec) return plan_fail(err, err_len, "layer %d: all fallback records of a flow must share one precision", l);
            fb_prec = pfb;
            if (prec >= 0 && pr != prec) return plan_fail(err, err_len, "layer %d: all MLP layers of a flow must be packed with the same precision", l);
            prec = pr;
        }
        p.layers[l] = LayerEntry{kind | (perm << 4) | ((slot + 1) << 8), d[D_PARAM]};
    }
    if (prec < 0) prec = 0;
    if (fb_prec < 0) fb_prec = 0;
    {   // bits 16..25 of x: iteration position + 1 of the next layer with an MLP image behind this one (0 = none), in the order the
        // pass walks the layers -- saves the kernel a dependent chain of scalar loads per layer
        int nxt = 0;
        for (int pos = n_layers - 1; pos >= 0; --pos) {
            const int l = o.dir ? n_layers - 1 - pos : pos;
            p.layers[l].x |= nxt << 16;
            if (kind_has_mlp(p.layers[l].x & 15)) nxt = pos + 1;
        }
    }
    int n_slots;
    bool any_mlp;
    desc_slots(desc, n_layers, &n_slots, &any_mlp);
    if (n_slots > 0) {
        if (!o.feature) return plan_fail(err, err_len, "this flow consumes a feature vector but feature pointer is null (flow/mobiusflow.py:48-49)");
        if (F <= 0 || F % 8) return plan_fail(err, err_len, "feature_dim=%d must be a positive multiple of 8 (pad on the host)", F);
    }
    p.empty = n == 0;
    p.dir = o.dir; p.n_layers = n_layers; p.n_slots = n_slots; p.K = K; p.F = F;
    p.prec = prec; p.fb_prec = fb_prec; p.any_mlp = any_mlp;
    if (p.empty) return true;

    const bool shared = o.feature_div > 0 && n_slots > 0;
    if (shared && n % o.feature_div) return plan_fail(err, err_len, "n=%lld not divisible by feature_div=%lld", n, (long long)o.feature_div);
    p.ws_need = flow_workspace(o, n_slots, any_mlp, cus, &p.stash_at);
    const bool stash = p.ws_need > p.stash_at;           // overflow stash of the K > 128 inverse, behind everything else
    if (stash && shared) return plan_fail(err, err_len, "inverse pass with segments > 128 is not built for shared feature rows; got %d", K);
    if (n_slots > 0 || o.sum_out || stash) {
        if (!o.workspace) return plan_fail(err, err_len, "workspace pointer is null");
        if (o.workspace_bytes < p.ws_need)
            return plan_fail(err, err_len, "workspace of %zu bytes is smaller than the %zu needed (rnf_flow_pass_workspace_bytes)", o.workspace_bytes, p.ws_need);
    }

    const int KT = (K + 7) / 8;
    // inverse: the segment parameters of a layer stay in registers through the root finder; instantiations hold 1, 2, 4, 8 tiles
    // (8-wave workgroups) or 16 (K <= 128: 4-wave workgroups with the whole register file, fc_last staged in two halves; more segments
    // go through the stash).  Round 4: also for conditional 3x3 / 6x6 layers, side layers and shared feature rows -- flow/mobiusflow.py:7-14
    // takes any `segments` with any `rot` -- on the extended build of the 4-wave instantiation.
    p.KT = KT;
    p.kt_inv = KT <= 1 ? 1 : (KT <= 2 ? 2 : (KT <= 4 ? 4 : (KT <= 8 ? 8 : 16)));
    const int max_tiles = prec == 2 ? Lay<2>::MAX_TILES_IN_LDS : MOB_MAX_TILES_IN_LDS;
    int tiles_in_lds = any_mlp ? (KT < max_tiles ? KT : max_tiles) : 0;
    if (any_mlp && tiles_in_lds < min_tiles) tiles_in_lds = min_tiles;
    size_t lds = !any_mlp ? 0 : sizeof(float) * (prec == 2 ? (size_t)3 * klim::B3_REGION_FLOATS      // three ring regions (flow_kernels.h RING)
                                                           : MOB_HEAD_FLOATS + (size_t)tiles_in_lds * MOB_LAST_TILE_FLOATS);
    if (lds < NW_FWD_WIDE * sizeof(double) * 2) lds = NW_FWD_WIDE * sizeof(double) * 2;
    p.fair_off = -1;                                     // SIMD fairness governor (flow_kernels.h struct Fair): forward split-precision kernel
    if (sw.fair && any_mlp && o.dir == 0 && prec == 1) {
        p.fair_off = (int)(lds / sizeof(float));
        lds += 64;
    }
    // Root finder of the inverse pass: order of its FIRST pass (flow_kernels.h mobius_inv_finish).  Third order (Halley) unless the flow
    // asks for the fourth-order first pass -- bits 16..17 of desc column 5 on its Moebius layers (1: third, 2: fourth; 0: this default).
    // The fourth order pays on sharply peaked conditioner outputs (a trained p(R | image): the third-order iteration then needs a third
    // pass for most waves; trained_c4 10.02 -> 9.66 ms) and costs mild weights its four extra instructions per segment pair (BASELINE's
    // synthetic C5q +4 %, C5 +0.9 %: profiles/r6/ab_centre.jsonl), so it is a property of the FLOW its owner sets (Flow.set_rootfinder_order,
    // the checkpoint sidecar) -- one value per flow, never per launch.  RNF_RF_FIRST=3|4 forces one.
    p.rf_first4 = sw.rf_first ? (sw.rf_first == 4) : (rf_code == 2);
    const bool pipe = sw.staging_dma && KT <= MOB_MAX_TILES_IN_LDS && prec != 2;    // bf16x3: a K = 64 layer image is 171 KiB (layout.h Lay<2>): synchronous staging
    p.tab_off = -1;
    if ((pipe || prec == 2) && any_mlp) {                // two LDS buffers for the blocks of constant-affine layers (flow_kernels.h stage_table)
        lds = (lds + 15) / 16 * 16;
        p.tab_off = (int)(lds / sizeof(float));
        lds += sizeof(float) * 2 * AFF_TABLE_LDS_STRIDE;
    }
    // guarded split-precision call: every chunk is followed by the exact-fp32 kernels, which return at once unless the chunk's guard fired
    // (an in-place call -- rotation_out == rotation -- cannot be re-run from its own overwritten input: it runs unguarded, on the kernel
    // instantiations whose softplus is overflow-safe on its own; include/rnf_hip.h "aliasing")
    const bool guarded = prec == 1 && any_mlp && have_fb && o.workspace && o.workspace_bytes >= PARTIALS_BYTES && sw.guard &&
                         !(o.rotation_out && o.rotation_out == o.rotation);
    // FUSED: forward pass of a conditional flow whose every MLP layer is conditional, F <= 256, projection records equally spaced in the
    // blob (both packers lay them out that way) -- the feature projection runs inside the stack kernel, no scratch round trip (HBM traffic
    // = the algorithmic bytes).  Guarded launches only: the instantiation uses the one-piece softplus.  OFF by default: measured on C4 it is
    // SLOWER (12.2 ms against 8.7 ms, profiles/r3/fused_c4.md): the features take 128 of the 256 registers an 8-wave workgroup has per
    // lane, the rest of the layer does not fit beside them, and its projection phases run in lockstep between workgroup barriers.
    bool fused = sw.fused && lean2 && o.dir == 0 && prec == 1 && pipe && any_mlp && n_slots > 0 && all_mlp_cond && !shared && !ext_layers && !o.states &&
                 F <= klim::FUSED_MAX_F && guarded && p.tab_off >= 0;
    p.feat_stride = (int)((featproj_packed_floats(F) + 3) / 4 * 4);
    if (fused && n_slots > 1) p.feat_stride = p.feat_off[1] - p.feat_off[0];
    for (int sl = 0; fused && sl < n_slots; ++sl)
        if (p.feat_off[sl] != p.feat_off[0] + sl * p.feat_stride) fused = false;
    p.lds_fb = lds;                                      // the fallback shares the primary's layout (without the FUSED buffer) ...
    p.tab_off_fb = p.tab_off;
    p.pa_off = 0;
    if (fused) {
        const size_t at = (lds + 15) / 16 * 16;
        if (at + sizeof(float) * klim::FUSED_PA_FLOATS > 160 * 1024) fused = false;
        else { p.pa_off = (int)(at / sizeof(float)); lds = at + sizeof(float) * klim::FUSED_PA_FLOATS; }
    }
    p.lds_bytes = lds;
    if (fb_prec == 2) {
        // ... unless its records are bf16x3 (round 6: the guard's re-run target on host-packed flows -- 1.8x the guarded time instead of the
        // 3.3x of the exact-fp32 MFMA): the ring-staged kernels with their own LDS layout (three regions + the affine blocks)
        p.lds_fb = sizeof(float) * (size_t)3 * klim::B3_REGION_FLOATS;
        p.tab_off_fb = (int)(p.lds_fb / sizeof(float));
        p.lds_fb += sizeof(float) * 2 * AFF_TABLE_LDS_STRIDE;
    }
    // Shared feature rows on the fast kernels (round 5; pose estimation: agent.py:238-263 evaluates number_queries rotations per image
    // feature): rows of >= 32 rotations, guarded split-precision call with DMA staging, and either a forward pass of the conditional-lean
    // structure (SYMSOL-I: Condition16Trans + conditional Moebius + constant affine) or an inverse pass with K <= 64 segments of a flow
    // without extended layers.  Decided by the flow and the call's row length, never by the batch size.  Everything else with shared rows
    // stays on the extended instantiation.
    // GUARDED calls only, in both directions: the row records enter x0 through a matrix step (flow_kernels.h GFragRows), where a non-finite
    // record of one image would also poison the rotations of the NEXT image that share its wave (NaN x 0 = NaN); the guard sees that and the
    // exact-fp32 re-run, which reads the records per lane, restores per-image semantics.  Unguarded calls keep the extended instantiation.
    const long long feat_rows = shared ? n / o.feature_div : 0;
    const bool rows_lean2 = lean2 && all_mlp_cond && guarded && p.tab_off >= 0;
    const bool rows = shared && !ext_layers && prec == 1 && pipe && any_mlp && o.feature_div >= 32 && n < (1LL << 31) &&
                      feat_rows < (1LL << 24) && !o.states && guarded && (o.dir == 0 ? rows_lean2 : (KT <= 8));
    const bool ext = ext_layers || (shared && !rows);
    // The kernel FAMILY -- 1: Moebius + constant-affine layers only (BASELINE C1 / C2 / C3), 2: the conditional counterpart (Moebius +
    // constant-affine + Condition16Trans, every MLP conditional: C4), 0: the general kernel -- comes from the flow's structure and from
    // whether the call runs guarded, NEVER from the batch size: the families differ in arithmetic (one-piece softplus of the lean kernels,
    // so3_math.h), the workgroup widths of one family do not, so a rotation's result does not depend on the size of the launch (or chunk,
    // or shard) it travels in.
    p.family = (guarded && p.tab_off >= 0 && o.dir == 0 && prec == 1 && pipe && !ext)
                   ? (lean ? 1 : (lean2 && all_mlp_cond && n_slots > 0 && (!shared || rows) ? 2 : 0)) : 0;
    p.shared = shared; p.guarded = guarded; p.pipe = pipe; p.ext = ext; p.rows = rows; p.fused = fused; p.wide_ok = sw.wide;
    p.ext_fb = ext_layers || shared;                     // shared rows: the exact-fp32 re-run reads them on the extended instantiation
    p.chunk_cap = (n_slots && !shared) ? CHUNK_SAMPLES : n;      // shared feature rows: the projection scratch is tiny
    p.feat_rows = feat_rows;
    return true;
}

inline ChunkPlan plan_chunk(const FlowPlan &p, int cus, long long cn) {
    ChunkPlan c;
    // waves per workgroup of the stack kernel: the forward split-precision kernel goes 16 wide once 8-wave workgroups would no longer fit
    // the CUs in one round, and 4 narrow -- like the inverse one (round 5: a launch that leaves half of the CUs empty at 8 waves is a
    // latency chain per wave; 2^15 rotations: 0.73 -> 0.57 ms) -- while 4-wave workgroups still fit; same arithmetic, bit-equal rows
    const bool fast = p.prec == 1 && p.pipe && !p.ext && p.wide_ok;
    const bool wide = !p.fused && p.dir == 0 && fast && cn > (long long)cus * NW_FWD_H * 32;
    const bool narrow = !p.fused && p.dir == 0 && fast && cn <= (long long)cus * NW_FWD_NARROW * 32;
    const bool big_inv = p.dir == 1 && p.any_mlp && p.KT > 8;                  // 4-wave instantiation (512 registers per lane)
    const bool narrow_inv = p.dir == 1 && fast && p.any_mlp && p.KT <= 8 && cn <= (long long)cus * NW_FWD_NARROW * 32;
    c.nw = p.fused ? NW_FUSED : (big_inv ? NW_INV_BIG : (wide ? NW_FWD_WIDE : ((narrow || narrow_inv) ? NW_FWD_NARROW : ((p.dir == 0 && p.prec == 1) ? NW_FWD_H : NW))));
    c.fair_off = (wide || narrow || p.family || (p.fused && NW_FUSED != 8)) ? -1 : p.fair_off;     // the governor pairs two waves per SIMD (general 8-wave kernel)
    const long long ntiles = (cn + c.nw * 32 - 1) / (c.nw * 32);
    const long long ntiles_fp = (cn + NW_FP * 32 - 1) / (NW_FP * 32);
    const int nw_fb = big_inv ? NW_INV_BIG : NW;                               // the exact-fp32 re-run uses NW-wave workgroups
    const long long ntiles_fb = (cn + nw_fb * 32 - 1) / (nw_fb * 32);
    c.groups = (ntiles * c.nw > ntiles_fp * NW_FP) ? ntiles * c.nw : ntiles_fp * NW_FP;
    if (p.guarded && ntiles_fb * nw_fb > c.groups) c.groups = ntiles_fb * nw_fb;
    if ((cn + 127) / 128 * 4 > c.groups) c.groups = (cn + 127) / 128 * 4;
    c.grid = (int)(ntiles < cus ? ntiles : cus);
    c.grid_fb = p.guarded ? (int)(ntiles_fb < cus ? ntiles_fb : cus) : 0;
    return c;
}

// The instantiation of the primary launch of a chunk.  (kt_inv 16 exists with NW_INV_BIG waves only, whatever sized the grid.)
inline KernelKey stack_key(const FlowPlan &p, const ChunkPlan &c) {
    if (p.fused) return KernelKey{0, 0, NW_FUSED, true, 1, false, 2, true, false};
    const int kt = p.dir ? p.kt_inv : 0;
    return KernelKey{p.dir, kt, kt == 16 ? NW_INV_BIG : c.nw, p.pipe && kt != 16, p.prec, p.ext, p.family, false, p.rows};
}
// ... and of the guard's re-run: the strict kernels have no lean family, shared rows there stay on the extended kernels
inline KernelKey fallback_key(const FlowPlan &p) {
    const int kt = p.dir ? p.kt_inv : 0;
    return KernelKey{p.dir, kt, kt == 16 ? NW_INV_BIG : NW, p.pipe && kt != 16 && p.fb_prec != 2, p.fb_prec, p.ext_fb, 0, false, false};
}

// Feature projection of `rows` feature rows of F columns in arithmetic `prec` (0 exact fp32, 1 split precision)
inline ProjPlan plan_projection_rows(long long rows, int F, int prec, int cus) {
    ProjPlan j;
    j.rows = rows;
    const long long tiles = (rows + NW_FP * 32 - 1) / (NW_FP * 32);
    const int cus_fp = cus * (8 / NW_FP), kchunk = F < klim::FP_KCHUNK ? F : klim::FP_KCHUNK;
    j.grid = (int)(tiles < cus_fp ? tiles : cus_fp);
    j.block = NW_FP * 64;
    j.lds_bytes = sizeof(float) * (prec ? (size_t)2 * (klim::FP_KCHUNK / 16) * 512 : (size_t)kchunk / 8 * 256);   // f16x2: two DMA buffers
    j.kernel = !prec ? PROJ_FP32 : (F > klim::FP_KCHUNK ? PROJ_F16X2_KCHUNKS : PROJ_F16X2);      // F > 512: K-chunks whose partial sums pass through the scratch
    if (prec && F > klim::FP_KCHUNK && F <= 2 * klim::FP_KCHUNK) {     // K split over wave pairs: no partial sums through the scratch (featproj_kernel.h)
        const long long tiles2 = (rows + 127) / 128;
        j = ProjPlan{PROJ_F16X2_KSPLIT, (int)(tiles2 < cus ? tiles2 : cus), 8 * 64, klim::FP2_LDS_BYTES, rows};
    }
    return j;
}
// ... in front of a stack launch: of the chunk's cn rotations, or -- shared rows -- of the feature rows (ONE projection before the first
// chunk); `fb`: the exact-fp32 projection of a guarded call, which runs only if the guard fired (every chunk, also with shared rows).
// bf16x3 flows project in exact fp32 too (their records hold the fp32 image).
inline ProjPlan plan_projection(const FlowPlan &p, int cus, long long cn, bool fb) {
    return plan_projection_rows(p.shared ? p.feat_rows : cn, p.F, (fb || p.prec == 2) ? 0 : p.prec, cus);
}

// The launches of a call, in the order rnf_flow_pass issues them.  `visit(Launch)` returns non-zero to stop (the value is passed on).
enum LaunchKind {
    LAUNCH_GUARD_RESET,        // hipMemsetAsync of the guard: both ints before the first chunk, the chunk's int before each later one
    LAUNCH_PROJECTION,         // feature projection (fb: of the fallback records, runs only if the guard fired)
    LAUNCH_STACK,              // the stack kernel (fb: the guard's re-run)
    LAUNCH_FINALIZE            // nll_finalize_kernel of the chunk's partial sums
};
struct Launch {
    LaunchKind kind;
    bool fb;
    long long base, cn;        // the chunk: first rotation and count
    ChunkPlan chunk;
};
template <class Visit>
inline int for_each_launch(const FlowPlan &p, int cus, long long n, bool sum_out, Visit &&visit) {
    for (long long base = 0; base < n; base += p.chunk_cap) {
        const long long cn = (n - base) < p.chunk_cap ? (n - base) : p.chunk_cap;
        const ChunkPlan c = plan_chunk(p, cus, cn);
        if (p.guarded)
            if (int rc = visit(Launch{LAUNCH_GUARD_RESET, false, base, cn, c})) return rc;
        if (p.n_slots && !p.fused && (!p.shared || base == 0))         // shared rows: ONE projection, before the first chunk
            if (int rc = visit(Launch{LAUNCH_PROJECTION, false, base, cn, c})) return rc;
        if (int rc = visit(Launch{LAUNCH_STACK, false, base, cn, c})) return rc;
        if (p.guarded) {             // the same chunk on the exact-fp32 kernels, skipped on the device unless the guard fired
            if (p.n_slots)
                if (int rc = visit(Launch{LAUNCH_PROJECTION, true, base, cn, c})) return rc;
            if (int rc = visit(Launch{LAUNCH_STACK, true, base, cn, c})) return rc;
        }
        if (sum_out)
            if (int rc = visit(Launch{LAUNCH_FINALIZE, false, base, cn, c})) return rc;
    }
    return 0;
}

}  // namespace rnf
