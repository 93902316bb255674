// rnf_api.hip -- C ABI of librnf_hip.so (include/rnf_hip.h): host-side parameter packing + kernel launchers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rnf_hip.h"
#include "featproj_kernel.h"
#include "flow_kernels.h"
#include "flow_plan.h"
#include "train_kernels.h"
#include "train_block16.h"
#include "pack_device.h"
#include "sampler_kernel.h"
#include "fisher_math.h"
#include "fisher_exact.h"
#include "fisher_fit.h"
#include "fisher_mixture.h"
#include "layout.h"
#include "equalize.h"
#include "svd4_lapack.h"
#include "grid_modes.h"
#include "so3_grid.h"
#include "grid_beam.h"
#include "grid_credible.h"
#include "grid_locate.h"
#include "grid_sample.h"
#include "so3_kernel_sum.h"
#include "so3_kernel_moments.h"
#include "so3_angle_cdf.h"
#include "so3_set_angle_cdf.h"
#include "so3_grid_local.h"
#include "so3_harmonics.h"

using namespace rnf;

static_assert(RNF_LAYER_MOBIUS == RNF_KIND_MOBIUS && RNF_LAYER_AFFINE16 == RNF_KIND_AFFINE16 &&
                  RNF_LAYER_AFFINE16_COND == RNF_KIND_COND16 && RNF_DESC_STRIDE == D_STRIDE && RNF_HIDDEN == HID &&
                  RNF_LAYER_SIDE16 == RNF_KIND_SIDE16 && RNF_LAYER_SIDE16_ROT == RNF_KIND_SIDE16_ROT && RNF_LAYER_SIDE9 == RNF_KIND_SIDE9,
              "include/rnf_hip.h and csrc/layout.h disagree");

// ------------------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}
#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail("%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// The checks that every struct entry repeats; `who` is the struct's name.  Each returns 0, or 1 with the message set.
template <class P>
static int check_struct(const P *p, const char *who) {
    if (!p || p->struct_bytes != sizeof(P)) return fail("%s.struct_bytes does not match the library's %zu", who, sizeof(P));
    return 0;
}

// p->workspace holds `need` bytes (as `fn`, the entry's *_workspace_bytes, computes) and, with align > 0, is aligned to it
template <class P>
static int check_workspace(const P *p, const char *who, size_t need, const char *fn, unsigned align) {
    if (!p->workspace || p->workspace_bytes < need)
        return fail("%s.workspace of %zu bytes is smaller than the %zu needed (%s)", who, (size_t)p->workspace_bytes, need, fn);
    if (align && reinterpret_cast<uintptr_t>(p->workspace) % align) return fail("%s.workspace must be %u-byte aligned", who, align);
    return 0;
}

// `what` names the one or two pointers after the struct's name (null: aligned)
static int check_aligned16(const void *a, const void *b, const char *who, const char *what) {
    if (reinterpret_cast<uintptr_t>(a) % 16 || reinterpret_cast<uintptr_t>(b) % 16) return fail("%s%s must be 16-byte aligned", who, what);
    return 0;
}

// The 0/1 switches of the environment: on unless the value starts with '0' (default on), or off unless it starts with '1'.  Each is read
// once per process (flow_switches, equalise_allowed); flow_plan.h struct Switches says what each one does.
static bool env_flag(const char *name, bool dflt) {
    const char *e = std::getenv(name);
    return (e && e[0] == (dflt ? '0' : '1')) ? !dflt : dflt;
}

extern "C" int rnf_abi_version(void) { return RNF_ABI_VERSION; }
extern "C" const char *rnf_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------------------
// packing (pure host code)
// ------------------------------------------------------------------------------------------------------------
extern "C" int64_t rnf_mobius_packed_floats(int32_t K) { return K > 0 ? mobius_packed_floats(K) : -1; }
extern "C" int64_t rnf_mobius_packed_floats_prec(int32_t K, int32_t prec) { return (K > 0 && prec >= 0 && prec <= 2) ? mobius_packed_floats_p(K, prec) : -1; }
extern "C" int64_t rnf_cond_packed_floats_prec(int32_t n_out, int32_t prec) { return (prec >= 0 && prec <= 2) ? cond_packed_floats_p(n_out == 36 ? 2 : 1, prec) : -1; }
extern "C" int64_t rnf_affine16_packed_floats(void) { return AFF_FLOATS; }
extern "C" int64_t rnf_cond16_packed_floats(void) { return COND16_FLOATS; }
extern "C" int64_t rnf_featproj_packed_floats(int32_t F) { return (F >= 0 && F % 8 == 0) ? featproj_packed_floats(F) : -1; }

// [OUT=32*n_ot][64] row-major weight rows `rowmap(ot, i)` -> image [ot][tg][lane] float4
template <typename RowFn>
static void pack_w64(float *img, int n_ot, RowFn row_of /* (ot, i) -> const float* row of 64 or nullptr */) {
    for (int ot = 0; ot < n_ot; ++ot)
        for (int tg = 0; tg < 8; ++tg)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5;
                const float *row = row_of(ot, i);
                float *dst = img + (((size_t)ot * 8 + tg) * 64 + lane) * 4;
                for (int c = 0; c < 4; ++c) dst[c] = row ? row[8 * tg + 4 * h + c] : 0.f;
            }
}

// split-precision image of the same rows: [ot][s (4)][hi, lo][lane] 8 x fp16, element j of lane (i, h) of k-step
// s = 2t + s' is W[row][32t + 16s' + 8(j>>2) + 4h + (j&3)] as hi = fp16(w), lo = fp16(w - hi) (unscaled, flow_kernels.h; the feature
// projection images keep lo scaled by 2^12, layout.h)
static thread_local bool g_half_overflow = false;     // per calling thread: ctypes releases the GIL and two flows may be packed at once
template <typename RowFn>
static void pack_w64_h(float *img, int n_ot, RowFn row_of) {
    _Float16 *out = reinterpret_cast<_Float16 *>(img);
    for (int ot = 0; ot < n_ot; ++ot)
        for (int s = 0; s < 4; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5;
                const float *row = row_of(ot, i);
                _Float16 *hi = out + ((((size_t)ot * 4 + s) * 2 + 0) * 64 + lane) * 8;
                _Float16 *lo = out + ((((size_t)ot * 4 + s) * 2 + 1) * 64 + lane) * 8;
                for (int j = 0; j < 8; ++j) {
                    const float w = row ? row[16 * s + 8 * (j >> 2) + 4 * h + (j & 3)] : 0.f;
                    if (!(std::fabs(w) < 65504.0f)) g_half_overflow = true;      // also catches NaN / inf
                    const _Float16 wh = (_Float16)w;
                    hi[j] = wh;
                    lo[j] = (_Float16)((w - (float)wh) * W_LO_SCALE);
                }
            }
}

// bf16x3 image of the same rows (layout.h Lay<2>): [ot][s (4)][hi, mid, lo][lane] 8 x bf16, element j of lane (i, h) of k-step s as in the
// fp16 image; the three terms are the TRUNCATED splits the kernels use for the activations (top 16 bits of w, of w - hi, of the rest):
// hi + mid + lo reproduces w to 2^-24 |w|, nothing to overflow or underflow short of fp32 itself.
static inline uint16_t bf16_trunc(float x) { uint32_t u; std::memcpy(&u, &x, 4); return (uint16_t)(u >> 16); }
static inline float bf16_float(uint16_t b) { uint32_t u = (uint32_t)b << 16; float x; std::memcpy(&x, &u, 4); return x; }
template <typename RowFn>
static void pack_w64_b3(float *img, int n_ot, RowFn row_of) {
    uint16_t *out = reinterpret_cast<uint16_t *>(img);
    for (int ot = 0; ot < n_ot; ++ot)
        for (int s = 0; s < 4; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5;
                const float *row = row_of(ot, i);
                uint16_t *dst[3];
                for (int t = 0; t < 3; ++t) dst[t] = out + ((((size_t)ot * 4 + s) * 3 + t) * 64 + lane) * 8;
                for (int j = 0; j < 8; ++j) {
                    const float w = row ? row[16 * s + 8 * (j >> 2) + 4 * h + (j & 3)] : 0.f;
                    const uint16_t wh = bf16_trunc(w);
                    const float r1 = w - bf16_float(wh);
                    const uint16_t wm = bf16_trunc(r1);
                    const float r2 = r1 - bf16_float(wm);
                    dst[0][j] = wh; dst[1][j] = wm; dst[2][j] = bf16_trunc(r2);
                }
            }
}

// bias image [ot][h][16]: b[32*ot + rho(r,h)] (or the mapped row's bias)
template <typename BiasFn>
static void pack_bias(float *img, int n_ot, BiasFn bias_of /* (ot, row_in_tile) -> float */) {
    for (int ot = 0; ot < n_ot; ++ot)
        for (int h = 0; h < 2; ++h)
            for (int r = 0; r < 16; ++r) img[(ot * 2 + h) * 16 + r] = bias_of(ot, rho(r, h));
}

static void pack_hidden(float *out, const float *const w[3], const float *const b[3], int prec) {
    const int w_tile = prec == 2 ? Lay<2>::W_TILE : Lay<0>::W_TILE, hb = prec == 2 ? Lay<2>::HB : MOB_HB;
    for (int L = 0; L < 3; ++L) {
        const float *W = w[L];
        auto row_of = [&](int ot, int i) { return W + (size_t)(32 * ot + i) * 64; };
        float *dst = out + MOB_HID + (size_t)L * 2 * w_tile;
        if (prec == 2) pack_w64_b3(dst, 2, row_of);
        else if (prec) pack_w64_h(dst, 2, row_of);
        else pack_w64(dst, 2, row_of);
        const float *B = b[L];
        pack_bias(out + hb + L * 2 * 2 * 16, 2, [&](int ot, int row) { return B[32 * ot + row]; });
    }
}

// feature projection record: weights Wf [64][ldw] starting at column col0, F columns; bias b0 [64]
static void pack_featproj_h(float *out, const float *W, int ldw, int col0, int F, const float *b0) {
    const int ns = (F + 15) / 16;
    _Float16 *o16 = reinterpret_cast<_Float16 *>(out);
    for (int ot = 0; ot < 2; ++ot)
        for (int s = 0; s < ns; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5;
                _Float16 *hi = o16 + ((((size_t)ot * ns + s) * 2 + 0) * 64 + lane) * 8;
                _Float16 *lo = o16 + ((((size_t)ot * ns + s) * 2 + 1) * 64 + lane) * 8;
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * s + 8 * h + j;
                    const float w = k < F ? W[(size_t)(32 * ot + i) * ldw + col0 + k] : 0.f;
                    if (!(std::fabs(w) < 65504.0f)) g_half_overflow = true;
                    const _Float16 wh = (_Float16)w;
                    hi[j] = wh;
                    lo[j] = (_Float16)((w - (float)wh) * FEAT_LO_SCALE);
                }
            }
    // bias image: zeros since round 5 -- b0 rides in the bias slot of the stack kernel's fc_first image (pack_first_bias), where it costs
    // nothing (that matrix step exists anyway); the projection kernels start every accumulator at zero (no bias loads, 16 fewer live registers)
    (void)b0;
    pack_bias(out + (size_t)2 * ns * 512, 2, [&](int, int) { return 0.f; });
}

static void pack_featproj(float *out, const float *W, int ldw, int col0, int F, const float *b0) {
    const int ng = F / 8;
    for (int ot = 0; ot < 2; ++ot)
        for (int tg = 0; tg < ng; ++tg)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5;
                float *dst = out + (((size_t)ot * ng + tg) * 64 + lane) * 4;
                for (int c = 0; c < 4; ++c) dst[c] = W[(size_t)(32 * ot + i) * ldw + col0 + 8 * tg + 4 * h + c];
            }
    (void)b0;                                              // see pack_featproj_h: the bias lives in the fc_first image
    pack_bias(out + (size_t)2 * ng * 256, 2, [&](int, int) { return 0.f; });
}


// ---- the conditioner MLP on the canonical point of its ReLU-rescaling orbit (equalize.h): what the f16x2 images are split from ----
struct ScaledMlp {
    int ni = 0, yo = 0, n_out = 0;
    std::vector<float> W0, b0, hw[3], hb[3], WL;     // W0 [64][ni], hw[l] [64][64], WL [n_out][64]
    EqExponents eq;
};

// RNF_EQUALIZE=0 / rnf_set_equalize(0): split the weights as given (measurement / test switch: what the audit and the range guard
// catch without the equalisation)
static int g_equalize = -1;
static bool equalise_allowed() {
    if (g_equalize < 0) g_equalize = env_flag("RNF_EQUALIZE", true) ? 1 : 0;
    return g_equalize == 1;
}
extern "C" int rnf_set_equalize(int on) {
    const int old = equalise_allowed() ? 1 : 0;
    g_equalize = on ? 1 : 0;
    return old;
}
// the audit's refusal can be switched off separately (tests of the run-time guard need an unequalised, unaudited image)
static int g_audit = 1;
extern "C" int rnf_set_pack_audit(int on) {
    const int old = g_audit;
    g_audit = on ? 1 : 0;
    return old;
}

// mean square of a feature entry assumed by the equalisation of the packers called from this thread (equalize.h); default 1
static thread_local double g_feature_ms = 1.0;
extern "C" double rnf_set_feature_ms(double ms) {
    const double old = g_feature_ms;
    g_feature_ms = (ms > 1.0e-20 && ms < 1.0e20) ? ms : 1.0;
    return old;
}

static void scale_mlp(const float *fc_first_w, int ni, int yo, const float *fc_first_b, const float *const hw[3], const float *const hb[3],
                      const float *fc_last_w, int n_out, bool equalise, ScaledMlp &m) {
    m.ni = ni; m.yo = yo; m.n_out = n_out;
    if (equalise && equalise_allowed()) eq_exponents_host(fc_first_w, ni, yo, fc_first_b, hw, hb, g_feature_ms, m.eq);
    else std::memset(&m.eq, 0, sizeof(m.eq));
    const int *e0 = m.eq.e[0], *e1 = m.eq.e[1], *e2 = m.eq.e[2];
    m.W0.resize((size_t)64 * ni);
    m.b0.resize(64);
    for (int o = 0; o < 64; ++o) {
        for (int c = 0; c < ni; ++c) m.W0[(size_t)o * ni + c] = std::ldexp(fc_first_w[(size_t)o * ni + c], e0[o]);
        m.b0[o] = std::ldexp(fc_first_b[o], e0[o]);
    }
    const int *eo[3] = {e1, e2, e0}, *ei[3] = {e0, e1, e2};      // x1 = W1 relu(x0), x2 = W3 relu(x1), x3 = W5 relu(x2) (flow/condition.py:24-29)
    for (int l = 0; l < 3; ++l) {
        m.hw[l].resize(4096);
        m.hb[l].resize(64);
        for (int o = 0; o < 64; ++o) {
            for (int j = 0; j < 64; ++j) m.hw[l][o * 64 + j] = std::ldexp(hw[l][o * 64 + j], eo[l][o] - ei[l][j]);
            m.hb[l][o] = std::ldexp(hb[l][o], eo[l][o]);
        }
    }
    m.WL.resize((size_t)n_out * 64);
    for (int o = 0; o < n_out; ++o)
        for (int j = 0; j < 64; ++j) m.WL[(size_t)o * 64 + j] = std::ldexp(fc_last_w[(size_t)o * 64 + j], -e0[j]);
}

// Pack-time AUDIT of the split-precision images: the packed network (scaled weights and every activation rounded to fp16 hi + lo pairs
// exactly as the kernels hold them, three products per term, accumulation in double so that only the REPRESENTATION error shows) against the
// exact network (the weights as given, double) on probe inputs: unit vectors y, feature rows N(0, 1) and N(0, 1/64) from a fixed
// generator.  Returns max_o |out_packed - out_exact| / max(1, sum_j |Wl_oj t_j| + |bl_o|).  A layer that the equalisation could not bring into the regime
// where the pairs carry ~22 bits (estimates far off, a degenerate checkpoint) is refused like a weight outside the fp16 range, and the
// flow runs on the exact-fp32 kernels.
static inline void split_h(float v, float lo_scale, double &hi, double &lo) {
    const _Float16 h = (_Float16)v;
    hi = (double)(float)h;
    lo = (double)(float)(_Float16)((v - (float)h) * lo_scale) / lo_scale;
}
static double audit_mlp(const ScaledMlp &m, const float *fc_first_w, const float *fc_first_b, const float *const hw[3], const float *const hb[3],
                        const float *fc_last_w, const float *fc_last_b) {
    const int ni = m.ni, yo = m.yo, n_out = m.n_out, F = ni - yo;
    constexpr int PROBES = 6;
    unsigned long long rng = 0x9E3779B97F4A7C15ull;
    auto uni = [&]() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (double)((rng >> 11) & ((1ull << 53) - 1)) / (double)(1ull << 53); };
    auto gauss = [&]() { double s = 0.0; for (int i = 0; i < 12; ++i) s += uni(); return s - 6.0; };
    std::vector<double> whi((size_t)3 * 4096), wlo((size_t)3 * 4096), lhi((size_t)n_out * 64), llo((size_t)n_out * 64);
    for (int l = 0; l < 3; ++l)
        for (int i = 0; i < 4096; ++i) split_h(m.hw[l][i], W_LO_SCALE, whi[l * 4096 + i], wlo[l * 4096 + i]);
    for (size_t i = 0; i < (size_t)n_out * 64; ++i) split_h(m.WL[i], W_LO_SCALE, lhi[i], llo[i]);
    std::vector<double> fhi((size_t)64 * (F > 0 ? F : 1)), flo(fhi.size());
    for (int o = 0; o < 64; ++o)
        for (int k = 0; k < F; ++k) split_h(m.W0[(size_t)o * ni + yo + k], FEAT_LO_SCALE, fhi[(size_t)o * F + k], flo[(size_t)o * F + k]);
    double worst = 0.0;
    std::vector<float> in(ni > 0 ? ni : 1);
    for (int p = 0; p < PROBES; ++p) {
        double y[3] = {gauss(), gauss(), gauss()};
        const double yn = std::sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]) + 1e-30;
        for (int c = 0; c < yo; ++c) in[c] = (float)(y[c] / yn);
        const double fs = ((p & 1) ? 0.125 : 1.0) * std::sqrt(g_feature_ms);
        for (int k = 0; k < F; ++k) in[yo + k] = (float)(fs * gauss());
        // exact
        double x0[64], a[64], b[64], x3[64];
        for (int o = 0; o < 64; ++o) {
            double s = fc_first_b[o];
            for (int c = 0; c < ni; ++c) s += (double)fc_first_w[(size_t)o * ni + c] * in[c];
            x0[o] = s;
            a[o] = s > 0 ? s : 0;
        }
        for (int l = 0; l < 3; ++l) {
            for (int o = 0; o < 64; ++o) {
                double s = hb[l][o];
                for (int j = 0; j < 64; ++j) s += (double)hw[l][o * 64 + j] * a[j];
                b[o] = s;
            }
            for (int o = 0; o < 64; ++o) { x3[o] = b[o]; a[o] = b[o] > 0 ? b[o] : 0; }
        }
        double t[64];
        for (int o = 0; o < 64; ++o) { const double v = x0[o] + x3[o]; t[o] = v > 0 ? v : 0; }
        // packed arithmetic
        float px0[64], pa[64], pb[64];
        std::vector<double> ph(F > 0 ? F : 1), pl(ph.size());
        for (int k = 0; k < F; ++k) split_h(in[yo + k], FEAT_LO_SCALE, ph[k], pl[k]);
        for (int o = 0; o < 64; ++o) {
            double s = m.b0[o];
            for (int c = 0; c < yo; ++c) s += (double)m.W0[(size_t)o * ni + c] * in[c];
            for (int k = 0; k < F; ++k) s += fhi[(size_t)o * F + k] * ph[k] + fhi[(size_t)o * F + k] * pl[k] + flo[(size_t)o * F + k] * ph[k];
            px0[o] = (float)s;
            pa[o] = px0[o] > 0 ? px0[o] : 0.f;
        }
        for (int l = 0; l < 3; ++l) {
            double ah[64], al[64];
            for (int j = 0; j < 64; ++j) split_h(pa[j], W_LO_SCALE, ah[j], al[j]);
            for (int o = 0; o < 64; ++o) {
                double s = m.hb[l][o];
                const double *wh = &whi[l * 4096 + o * 64], *wl = &wlo[l * 4096 + o * 64];
                for (int j = 0; j < 64; ++j) s += wh[j] * ah[j] + wh[j] * al[j] + wl[j] * ah[j];
                pb[o] = (float)s;
            }
            for (int o = 0; o < 64; ++o) pa[o] = pb[o] > 0 ? pb[o] : 0.f;
        }
        double th[64], tl[64];
        for (int j = 0; j < 64; ++j) { const float v = px0[j] + pb[j]; split_h(v > 0 ? v : 0.f, W_LO_SCALE, th[j], tl[j]); }
        for (int o = 0; o < n_out; ++o) {
            double se = fc_last_b[o], sp = fc_last_b[o], mag = std::fabs((double)fc_last_b[o]);
            for (int j = 0; j < 64; ++j) {
                se += (double)fc_last_w[(size_t)o * 64 + j] * t[j];
                mag += std::fabs((double)fc_last_w[(size_t)o * 64 + j] * t[j]);
                sp += lhi[(size_t)o * 64 + j] * th[j] + lhi[(size_t)o * 64 + j] * tl[j] + llo[(size_t)o * 64 + j] * th[j];
            }
            const double err = std::fabs(sp - se) / std::fmax(1.0, mag);       // relative to the un-cancelled magnitude of the output's sum
            if (!(err <= worst)) worst = err;          // NaN lands here too
        }
    }
    return worst;
}
// largest audited error a split-precision layer may show (conditioner outputs, relative above 1); a balanced layer sits at ~2e-7
constexpr double AUDIT_MAX_ERR = 4.0e-6;
static thread_local double g_last_audit = 0.0;     // per calling thread, like g_half_overflow
extern "C" double rnf_last_pack_audit(void) { return g_last_audit; }

extern "C" int rnf_pack_mobius(const float *fc_first_w, const float *fc_first_b, const float *l1_w, const float *l1_b,
                               const float *l3_w, const float *l3_b, const float *l5_w, const float *l5_b,
                               const float *fc_last_w, const float *fc_last_b, int32_t K, int32_t F, int32_t prec,
                               float *out, float *out_feat) {
    if (K <= 0) return fail("rnf_pack_mobius: segments=%d must be positive", K);
    if (prec != RNF_PREC_FP32 && prec != RNF_PREC_F16X2 && prec != RNF_PREC_BF16X3) return fail("rnf_pack_mobius: unknown precision %d", prec);
    g_half_overflow = false;
    g_last_audit = 0.0;
    if (F < 0 || F % 8) return fail("rnf_pack_mobius: feature_dim=%d must be a multiple of 8 (pad on the host)", F);
    const int ni = 3 + F;
    const float *hw[3] = {l1_w, l3_w, l5_w};
    const float *hb[3] = {l1_b, l3_b, l5_b};
    // split precision: the layer is first moved to the canonical point of its ReLU-rescaling orbit (equalize.h); exact fp32: packed as given
    ScaledMlp m;
    scale_mlp(fc_first_w, ni, 3, fc_first_b, hw, hb, fc_last_w, 4 * K, prec == RNF_PREC_F16X2, m);
    // fc_first: float2 per lane = (W0[o][h], h ? b0[o] : W0[o][2]); round 5: conditional layers too (the projection record has no bias)
    for (int ot = 0; ot < 2; ++ot)
        for (int lane = 0; lane < 64; ++lane) {
            const int o = 32 * ot + (lane & 31), h = lane >> 5;
            float *dst = out + MOB_FIRST + (ot * 64 + lane) * 2;
            dst[0] = m.W0[(size_t)o * ni + h];
            dst[1] = h ? m.b0[o] : m.W0[(size_t)o * ni + 2];
        }
    const float *shw[3] = {m.hw[0].data(), m.hw[1].data(), m.hw[2].data()};
    const float *shb[3] = {m.hb[0].data(), m.hb[1].data(), m.hb[2].data()};
    pack_hidden(out, shw, shb, prec);
    // fc_last: packed row P = 32*tau + 8g + 4h + c  <->  segment k = 8*tau + 2g + h, component c
    // (K % 8 != 0: the last tile is padded with zero rows for segments k >= K; the kernels give those segments weight 0)
    auto src_row = [&](int tau, int row) {
        const int g = row >> 3, h = (row >> 2) & 1, c = row & 3;
        const int k = 8 * tau + 2 * g + h;
        if (k >= K) return -1;
        return c == 0 ? k : K + 3 * k + (c - 1);
    };
    // the rows that produce the segment weights' pre-activations (reference rows 0 .. K-1) are packed times log2 e (layout.h S_PRESCALE)
    for (size_t i = 0; i < (size_t)K * 64; ++i) m.WL[i] *= S_PRESCALE;
    const bool b3 = prec == RNF_PREC_BF16X3;
    for (int tau = 0; tau < (K + 7) / 8; ++tau) {
        float *rec = out + (b3 ? Lay<2>::LAST + (size_t)tau * Lay<2>::LAST_TILE_FLOATS : MOB_LAST + (size_t)tau * MOB_LAST_TILE_FLOATS);
        auto row_of = [&](int, int i) {
            const int r = src_row(tau, i);
            return r < 0 ? (const float *)nullptr : m.WL.data() + (size_t)r * 64;
        };
        if (b3) pack_w64_b3(rec, 1, row_of); else if (prec) pack_w64_h(rec, 1, row_of); else pack_w64(rec, 1, row_of);
        pack_bias(rec + (b3 ? Lay<2>::LAST_TILE_BIAS : MOB_LAST_TILE_BIAS), 1, [&](int, int row) {
            const int r = src_row(tau, row);
            return r < 0 ? 0.f : (r < K ? fc_last_b[r] * S_PRESCALE : fc_last_b[r]);
        });
    }
    // bf16x3 flows project their features with the exact-fp32 projection kernels (the fp16 projection images are the ones that need the
    // equalisation's feature scale)
    if (F) { if (prec == RNF_PREC_F16X2) pack_featproj_h(out_feat, m.W0.data(), ni, 3, F, m.b0.data()); else pack_featproj(out_feat, m.W0.data(), ni, 3, F, m.b0.data()); }
    if (b3) return 0;                                   // nothing to audit: 24-bit operands, fp32's range
    if (prec && g_half_overflow) return fail("rnf_pack_mobius: a weight is outside the fp16 range; use RNF_PREC_FP32") + 1;
    if (prec) {
        for (size_t i = 0; i < (size_t)K * 64; ++i) m.WL[i] = std::ldexp(fc_last_w[i], -m.eq.e[0][i & 63]);      // the audit compares unscaled outputs
        g_last_audit = audit_mlp(m, fc_first_w, fc_first_b, hw, hb, fc_last_w, fc_last_b);
        if (g_audit && !(g_last_audit <= AUDIT_MAX_ERR))
            return fail("rnf_pack_mobius: the split-precision image of this layer is off by %.2e on the probe inputs (limit %.1e): its scales "
                        "are outside what fp16 pairs resolve; use RNF_PREC_FP32", g_last_audit, AUDIT_MAX_ERR) + 1;
    }
    return 0;
}

static int pack_cond(const float *fc_first_w, const float *fc_first_b, const float *l1_w, const float *l1_b, const float *l3_w,
                     const float *l3_b, const float *l5_w, const float *l5_b, const float *fc_last_w, const float *fc_last_b, int32_t F,
                     int32_t prec, int32_t n_out, float *out, float *out_feat);

extern "C" int rnf_pack_cond16(const float *fc_first_w, const float *fc_first_b, const float *l1_w, const float *l1_b,
                               const float *l3_w, const float *l3_b, const float *l5_w, const float *l5_b,
                               const float *fc_last_w, const float *fc_last_b, int32_t F, int32_t prec, float *out,
                               float *out_feat) {
    return pack_cond(fc_first_w, fc_first_b, l1_w, l1_b, l3_w, l3_b, l5_w, l5_b, fc_last_w, fc_last_b, F, prec, 16, out, out_feat);
}

// Condition9Trans / Condition9RotL / Condition9RotR / Condition9RotRSmith (flow/squeezetrans.py:234-247, flow/rottrans.py:108-181): the
// same record with a 9-row fc_last; output i sits where output i of Condition16Trans sits, so the kernels gather both the same way.
extern "C" int rnf_pack_cond9(const float *fc_first_w, const float *fc_first_b, const float *l1_w, const float *l1_b,
                              const float *l3_w, const float *l3_b, const float *l5_w, const float *l5_b,
                              const float *fc_last_w, const float *fc_last_b, int32_t F, int32_t prec, float *out,
                              float *out_feat) {
    return pack_cond(fc_first_w, fc_first_b, l1_w, l1_b, l3_w, l3_b, l5_w, l5_b, fc_last_w, fc_last_b, F, prec, 9, out, out_feat);
}

// Condition36Trans (flow/squeezetrans.py:334-347): two fc_last tiles, packed row P of tile 0 = output P, rows 0..3 of tile 1 = outputs 32..35
extern "C" int rnf_pack_cond36(const float *fc_first_w, const float *fc_first_b, const float *l1_w, const float *l1_b,
                               const float *l3_w, const float *l3_b, const float *l5_w, const float *l5_b,
                               const float *fc_last_w, const float *fc_last_b, int32_t F, int32_t prec, float *out,
                               float *out_feat) {
    return pack_cond(fc_first_w, fc_first_b, l1_w, l1_b, l3_w, l3_b, l5_w, l5_b, fc_last_w, fc_last_b, F, prec, 36, out, out_feat);
}
extern "C" int64_t rnf_cond36_packed_floats(void) { return COND36_FLOATS; }

static int pack_cond(const float *fc_first_w, const float *fc_first_b, const float *l1_w, const float *l1_b, const float *l3_w,
                     const float *l3_b, const float *l5_w, const float *l5_b, const float *fc_last_w, const float *fc_last_b, int32_t F,
                     int32_t prec, int32_t n_out, float *out, float *out_feat) {
    if (F <= 0 || F % 8) return fail("rnf_pack_cond16: feature_dim=%d must be a positive multiple of 8", F);
    if (prec != RNF_PREC_FP32 && prec != RNF_PREC_F16X2 && prec != RNF_PREC_BF16X3) return fail("rnf_pack_cond16: unknown precision %d", prec);
    g_half_overflow = false;
    g_last_audit = 0.0;
    std::memset(out, 0, sizeof(float) * cond_packed_floats_p(n_out == 36 ? 2 : 1, prec));   // zero fc_first image: x0 comes from the projection
    const float *hw[3] = {l1_w, l3_w, l5_w};
    const float *hb[3] = {l1_b, l3_b, l5_b};
    ScaledMlp m;                                       // equalize.h: canonical scaling before the fp16 split (split precision only)
    scale_mlp(fc_first_w, F, 0, fc_first_b, hw, hb, fc_last_w, n_out, prec == RNF_PREC_F16X2, m);
    const float *shw[3] = {m.hw[0].data(), m.hw[1].data(), m.hw[2].data()};
    const float *shb[3] = {m.hb[0].data(), m.hb[1].data(), m.hb[2].data()};
    // fc_first image: no rotation inputs (zero weights); the bias slot (element 1 of lane-half 1, multiplied by the constant 1 of the second
    // matrix step) carries b0 -- the projection G = W0 f has no bias of its own (round 5)
    for (int ot = 0; ot < 2; ++ot)
        for (int lane = 32; lane < 64; ++lane) out[MOB_FIRST + (ot * 64 + lane) * 2 + 1] = m.b0[32 * ot + (lane & 31)];
    pack_hidden(out, shw, shb, prec);
    // one fc_last tile: packed row 8g + 4h + c (g = 0,1) <-> output 4*(2g+h) + c (= M[2g + h][c] of the 4x4); rows >= 16 and outputs
    // >= n_out are zero
    auto src_row = [&](int row) {
        if (row >= 16) return -1;
        const int g = row >> 3, h = (row >> 2) & 1, c = row & 3;
        const int o = 4 * (2 * g + h) + c;
        return o < n_out ? o : -1;
    };
    for (int tau = 0; tau < (n_out == 36 ? 2 : 1); ++tau) {
        auto src = [&](int row) { return n_out == 36 ? (tau == 0 ? row : (row < 4 ? 32 + row : -1)) : src_row(row); };
        const bool b3 = prec == RNF_PREC_BF16X3;
        float *rec = out + (b3 ? Lay<2>::LAST + (size_t)tau * Lay<2>::LAST_TILE_FLOATS : MOB_LAST + (size_t)tau * MOB_LAST_TILE_FLOATS);
        auto row_of = [&](int, int i) { int s = src(i); return s < 0 ? (const float *)nullptr : m.WL.data() + (size_t)s * 64; };
        if (b3) pack_w64_b3(rec, 1, row_of); else if (prec) pack_w64_h(rec, 1, row_of); else pack_w64(rec, 1, row_of);
        pack_bias(rec + (b3 ? Lay<2>::LAST_TILE_BIAS : MOB_LAST_TILE_BIAS), 1, [&](int, int row) { int s = src(row); return s < 0 ? 0.f : fc_last_b[s]; });
    }
    if (prec == RNF_PREC_F16X2) pack_featproj_h(out_feat, m.W0.data(), F, 0, F, m.b0.data()); else pack_featproj(out_feat, m.W0.data(), F, 0, F, m.b0.data());
    if (prec == RNF_PREC_BF16X3) return 0;
    if (prec && g_half_overflow) return fail("rnf_pack_cond16: a weight is outside the fp16 range; use RNF_PREC_FP32") + 1;
    if (prec) {
        g_last_audit = audit_mlp(m, fc_first_w, fc_first_b, hw, hb, fc_last_w, fc_last_b);
        if (g_audit && !(g_last_audit <= AUDIT_MAX_ERR))
            return fail("rnf_pack_cond16: the split-precision image of this layer is off by %.2e on the probe inputs (limit %.1e): its scales "
                        "are outside what fp16 pairs resolve; use RNF_PREC_FP32", g_last_audit, AUDIT_MAX_ERR) + 1;
    }
    return 0;
}

// 4x4 inverse / determinant in double (Gauss-Jordan with partial pivoting)
static bool inv4_double(const double *m, double *inv, double *det) {
    double a[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { a[i][j] = m[4 * i + j]; a[i][4 + j] = (i == j); }
    double d = 1.0;
    for (int c = 0; c < 4; ++c) {
        int p = c;
        for (int r = c + 1; r < 4; ++r) if (std::fabs(a[r][c]) > std::fabs(a[p][c])) p = r;
        if (a[p][c] == 0.0) return false;
        if (p != c) { for (int j = 0; j < 8; ++j) std::swap(a[p][j], a[c][j]); d = -d; }
        d *= a[c][c];
        double ip = 1.0 / a[c][c];
        for (int j = 0; j < 8; ++j) a[c][j] *= ip;
        for (int r = 0; r < 4; ++r) if (r != c) {
            double f = a[r][c];
            for (int j = 0; j < 8; ++j) a[r][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) inv[4 * i + j] = a[i][4 + j];
    *det = d;
    return true;
}

extern "C" int rnf_pack_affine16(const float *mat16, float *out) {
    double m[16], inv[16], det;
    for (int i = 0; i < 16; ++i) m[i] = mat16[i];
    if (!inv4_double(m, inv, &det)) return fail("rnf_pack_affine16: singular 4x4 matrix");
    for (int i = 0; i < 16; ++i) { out[i] = mat16[i]; out[17 + i] = (float)inv[i]; }
    out[16] = (float)std::log(std::fabs(det));
    out[33] = (float)(-std::log(std::fabs(det)));
    out[34] = out[35] = 0.f;
    affine16_table(m, out[16], false, out + AFF_TABLE_FWD);
    affine16_table(inv, out[33], false, out + AFF_TABLE_INV);
    return 0;
}

// n x n inverse in double (Gauss-Jordan with partial pivoting), n <= 6
static bool invn_double(const double *m, int n, double *inv) {
    double a[6][12];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) { a[i][j] = m[n * i + j]; a[i][n + j] = (i == j); }
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r) if (std::fabs(a[r][c]) > std::fabs(a[p][c])) p = r;
        if (a[p][c] == 0.0) return false;
        if (p != c) for (int j = 0; j < 2 * n; ++j) std::swap(a[p][j], a[c][j]);
        const double ip = 1.0 / a[c][c];
        for (int j = 0; j < 2 * n; ++j) a[c][j] *= ip;
        for (int r = 0; r < n; ++r) if (r != c) {
            const double f = a[r][c];
            for (int j = 0; j < 2 * n; ++j) a[r][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) inv[n * i + j] = a[i][n + j];
    return true;
}

// Uncondition9Trans / Uncondition36Trans (flow/squeezetrans.py:250-261, 350-361): [M | M^-1], n = 3 or 6
extern "C" int rnf_pack_gs(const float *mat, int32_t n, float *out) {
    if (n != 3 && n != 6) return fail("rnf_pack_gs: n=%d must be 3 or 6", n);
    if (!mat || !out) return fail("rnf_pack_gs: null pointer");
    double m[36], inv[36];
    for (int i = 0; i < n * n; ++i) m[i] = mat[i];
    if (!invn_double(m, n, inv)) return fail("rnf_pack_gs: singular %dx%d matrix", n, n);
    const int total = n == 3 ? GS9_FLOATS : GS36_FLOATS;
    for (int i = 0; i < total; ++i) out[i] = 0.f;
    for (int i = 0; i < n * n; ++i) { out[i] = mat[i]; out[n * n + i] = (float)inv[i]; }
    return 0;
}

extern "C" int64_t rnf_gs_packed_floats(int32_t n) { return n == 3 ? GS9_FLOATS : (n == 6 ? GS36_FLOATS : -1); }

extern "C" int rnf_pack_rot16(const float *mat16, float *out) {
    // orthogonality check in double: M M^T = I within fp32 rounding of a product of SVD factors
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double d = 0.0;
            for (int k = 0; k < 4; ++k) d += (double)mat16[4 * i + k] * mat16[4 * j + k];
            if (std::fabs(d - (i == j)) > 1e-4) return fail("rnf_pack_rot16: matrix is not orthogonal (|M M^T - I| = %g)", std::fabs(d - (i == j)));
        }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { out[4 * i + j] = mat16[4 * i + j]; out[17 + 4 * i + j] = mat16[4 * j + i]; }
    out[16] = 0.f;
    out[33] = 0.f;
    out[34] = 1.f;
    out[35] = 0.f;
    double m[16], mt[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { m[4 * i + j] = mat16[4 * i + j]; mt[4 * i + j] = mat16[4 * j + i]; }
    affine16_table(m, 0.f, true, out + AFF_TABLE_FWD);
    affine16_table(mt, 0.f, true, out + AFF_TABLE_INV);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------------------
static_assert(klim::MAX_LAYERS == MAX_LAYERS && klim::MAX_SLOTS == MAX_SLOTS && klim::FP_KCHUNK == FP_KCHUNK && klim::FUSED_MAX_F == FUSED_MAX_F &&
                  klim::FUSED_PA_FLOATS == FUSED_PA_FLOATS && klim::B3_REGION_FLOATS == Mlp<2>::REGION_FLOATS && klim::FP2_LDS_BYTES == FP2_LDS_BYTES &&
                  sizeof(LayerEntry) == sizeof(int2),
              "csrc/flow_plan.h and the kernel headers disagree");

// Compute units of the CALLING THREAD'S CURRENT DEVICE (grids of the persistent kernels are sized by it).  Cached per device ordinal: one
// process may drive several GPUs (nn.DataParallel, agent.py:22; round 5 cached the first device's count for the whole process -- VERDICT r5 #7).
static int device_cus() {
    constexpr int MAX_DEV = 64;
    static std::atomic<int> cus[MAX_DEV];                  // zero-initialised
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return 256;
    int c = cus[dev].load(std::memory_order_relaxed);
    if (c == 0) {
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
        cus[dev].store(c, std::memory_order_relaxed);
    }
    return c;
}

extern "C" size_t rnf_workspace_bytes(int64_t n, int32_t n_cond_layers) { return conditioner_workspace(n, n_cond_layers); }

// One kernel launch: raise the kernel's dynamic-LDS limit to what this launch asks for, launch, check.
template <typename... P, typename... A>
static int launch(void (*kernel)(P...), int grid, int block, size_t lds_bytes, hipStream_t stream, const A &...args) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_bytes, stream, args...);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int g_fused = -1;                                // RNF_FUSED, read at its first use; rnf_set_fused overrides it
static bool fused_allowed() {
    if (g_fused < 0) g_fused = env_flag("RNF_FUSED", false) ? 1 : 0;
    return g_fused == 1;
}
static Switches flow_switches() {                       // the others: read at the first flow pass
    static const Switches env = [] {
        Switches s;
        s.wide = env_flag("RNF_WIDE", true);
        const char *staging = std::getenv("RNF_STAGING"), *rf = std::getenv("RNF_RF_FIRST");
        s.staging_dma = !(staging && std::strcmp(staging, "sync") == 0);
        s.guard = env_flag("RNF_GUARD", true);
        s.lean = env_flag("RNF_LEAN", true);
#ifdef RNF_NO_GUARD
        s.guard = false;
#endif
#ifdef RNF_NO_LEAN
        s.lean = false;
#endif
        s.fair = env_flag("RNF_FAIR", true);
        s.rf_first = rf ? (rf[0] == '4' ? 4 : (rf[0] == '3' ? 3 : 0)) : 0;
        return s;
    }();
    Switches s = env;
    s.fused = fused_allowed();
    return s;
}
extern "C" int rnf_set_fused(int on) {
    const int old = fused_allowed() ? 1 : 0;
    g_fused = on ? 1 : 0;
    return old;
}

// Block size of the training backward sweep: 0 = by batch size (default), 16 / 64 = force (RNF_TRAIN_BLOCK in the environment).
constexpr int64_t kTrainBlock64From = 6144;     // batches from this size on use the 64-rotation kernel (measured crossover: profiles/README.md)
static int g_train_block = -1;
static int train_block() {
    if (g_train_block < 0) {
        const char *e = std::getenv("RNF_TRAIN_BLOCK");
        const int v = e ? std::atoi(e) : 0;
        g_train_block = (v == 16 || v == 64) ? v : 0;
    }
    return g_train_block;
}
// Layers per launch of the device packer and of the backward sweep (their layer tables are kernel arguments): the table capacity, or fewer
// with RNF_LAYER_CHUNK=<n> in the environment -- a test switch: a chunked sweep must reproduce the single launch (tests/test_gpu_grad.py).
static int layer_chunk(int capacity) {
    const char *e = std::getenv("RNF_LAYER_CHUNK");
    const int v = e ? std::atoi(e) : 0;
    return (v >= 1 && v < capacity) ? v : capacity;
}
extern "C" int rnf_set_train_block(int rotations) {
    const int prev = train_block();
    g_train_block = (rotations == 16 || rotations == 64) ? rotations : 0;
    return prev;
}

static int launch_projection(const ProjPlan &j, const FeatProjArgs &fp, hipStream_t stream) {
    void (*const kernels[])(FeatProjArgs) = {featproj_ksplit_kernel, featproj_kernel<NW_FP, 1, true>, featproj_kernel<NW_FP, 1>, featproj_kernel<NW_FP, 0>};   // (ProjKernel order)
    return launch(kernels[j.kernel], j.grid, j.block, j.lds_bytes, stream, fp);
}

// The kernel of a key: the table of the instantiations flow_plan.h BUILT lists -- nothing else is instantiated.
using StackKernel = void (*)(FlowArgs);
template <size_t... I>
static StackKernel stack_kernel(int index, std::index_sequence<I...>) {
    static const StackKernel table[] = {flow_stack_kernel<BUILT.k[I].dir, BUILT.k[I].kt_inv, BUILT.k[I].nw, BUILT.k[I].pipe, BUILT.k[I].prec, BUILT.k[I].ext,
                                                          BUILT.k[I].lean, BUILT.k[I].fused, BUILT.k[I].rows>...};
    return index < 0 ? nullptr : table[index];
}
static int launch_stack(const KernelKey &key, const FlowArgs &a, int grid, size_t lds_bytes, hipStream_t stream) {
    const StackKernel kernel = stack_kernel(key_index(key), std::make_index_sequence<N_BUILT>());
    if (!kernel) return fail("internal: no %d-wave instantiation of this stack kernel", key.nw);
    return launch(kernel, grid, key.nw * 64, lds_bytes, stream, a);
}

static int run_flow(const RnfFlowPass &o) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(o.stream);
    const int cus = device_cus();
    FlowPlan p;
    char err[sizeof(g_err)];
    if (!plan_flow(o, cus, flow_switches(), p, err, sizeof(err))) return fail("%s", err);
    if (p.empty) {
        if (o.sum_out) { hipLaunchKernelGGL(nll_finalize_kernel, dim3(1), dim3(256), 0, stream, (const double *)nullptr, 0, 0.0, o.sum_out, 0); }
        return 0;
    }
    const int64_t n = o.n;
    char *ws = reinterpret_cast<char *>(o.workspace);
    double *partials = reinterpret_cast<double *>(ws);
    float *G = p.n_slots ? reinterpret_cast<float *>(ws + PARTIALS_BYTES) : nullptr;
    int *guard = p.guarded ? reinterpret_cast<int *>(partials + GUARD_AT) : nullptr;

    FlowArgs a;
    std::memset(&a, 0, sizeof(a));
    std::memcpy(a.layers, p.layers, sizeof(LayerEntry) * p.n_layers);
    a.blob = o.blob;
#ifdef RNF_STAMPS
    {   // diagnostic build: RNF_STAMPS_PTR=<device address of 8 zeroed uint64> (set by tools/phase_stamps.py)
        const char *sp = std::getenv("RNF_STAMPS_PTR");
        a.stamps = sp ? reinterpret_cast<unsigned long long *>(std::strtoull(sp, nullptr, 0)) : nullptr;
    }
#endif
    a.n_layers = p.n_layers;
    a.KT = p.KT;
    a.K = p.K;
    a.min_wsum = kMinWeightSum * (float)p.K;
    a.rf_first4 = p.rf_first4;
    a.tab_off = p.tab_off;
    a.g_div = p.shared ? o.feature_div : 0;
    a.g_rows = p.feat_rows;
    a.G = G;
    a.side = o.side;
    a.side_n = n;
    a.states = o.states;
    a.states_n = n;
    a.fisher_A = o.fisher_A;
    a.fisher_c = o.fisher_c;
    a.fisher_div = o.fisher_A ? n / o.fisher_B : 1;
    a.guard = guard;
    a.guard_mode = p.guarded ? 1 : 0;
    if (p.ws_need > p.stash_at) a.inv_stash = reinterpret_cast<float4 *>(ws + p.stash_at);
    if (p.fused) {
        a.pa_off = p.pa_off;
        a.feat_F = p.F;
        a.feat_base = p.feat_off[0];
        a.feat_stride = p.feat_stride;
    }
    FlowArgs b;                                            // the same call on the fallback records (guarded calls)
    if (p.guarded) {
        b = a;
        for (int l = 0; l < p.n_layers; ++l)
            if (kind_has_mlp(b.layers[l].x & 15)) b.layers[l].y = p.param_fb[l];
        b.tab_off = p.tab_off_fb;
        b.guard_mode = 2;
        b.fair_off = -1;
    }
    if (p.fused) a.stash = G;                              // grid * 8 waves * 8 KB <= the projection scratch the workspace is sized for
    FeatProjArgs fp;
    std::memset(&fp, 0, sizeof(fp));
    fp.blob = o.blob;
    fp.G = G;
    fp.F = p.F;
    fp.n_slots = p.n_slots;
    fp.row_mode = p.shared ? 1 : 0;
    return for_each_launch(p, cus, n, o.sum_out != nullptr, [&](const Launch &l) -> int {
        const ChunkPlan &c = l.chunk;
        switch (l.kind) {
        case LAUNCH_GUARD_RESET:                           // guard[1] (a re-run happened in this call) stays across the chunks
            HIP_TRY(hipMemsetAsync(guard, 0, (l.base ? 1 : 2) * sizeof(int), stream));
            return 0;
        case LAUNCH_PROJECTION: {
            const ProjPlan j = plan_projection(p, cus, l.cn, l.fb);
            fp.feat = p.shared ? o.feature : o.feature + l.base * p.F;
            fp.n = j.rows;
            fp.g_groups = c.groups;
            fp.only_if = l.fb ? guard : nullptr;
            std::memcpy(fp.feat_off, l.fb ? p.feat_off_fb : p.feat_off, sizeof(int) * p.n_slots);
            return launch_projection(j, fp, stream);
        }
        case LAUNCH_STACK: {
            FlowArgs &x = l.fb ? b : a;
            x.rot_in = o.rotation + l.base * 9;
            x.rot_out = o.rotation_out ? o.rotation_out + l.base * 9 : nullptr;
            x.ldj_out = o.ldj_out ? o.ldj_out + l.base : nullptr;
            x.logp_out = o.logp_out ? o.logp_out + l.base : nullptr;
            x.partials = o.sum_out ? partials + (l.fb ? PARTIALS_FB_AT : 0) : nullptr;
            x.n = l.cn;
            x.sample_base = l.base;
            x.g_groups = c.groups;
            if (l.fb) return launch_stack(fallback_key(p), b, c.grid_fb, p.lds_fb, stream);
            a.feat = p.fused ? o.feature + l.base * p.F : nullptr;
            a.fair_off = c.fair_off;
            return launch_stack(stack_key(p, c), a, c.grid, p.lds_bytes, stream);
        }
        case LAUNCH_FINALIZE:
            hipLaunchKernelGGL(nll_finalize_kernel, dim3(1), dim3(256), 0, stream, (const double *)partials, c.grid, (double)l.cn, o.sum_out, l.base == 0 ? 0 : 1,
                               (const double *)(partials + PARTIALS_FB_AT), c.grid_fb, (const int *)guard);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        return 0;
    });
}

extern "C" int rnf_flow_pass(const RnfFlowPass *p) {
    if (!p) return fail("RnfFlowPass pointer is null");
    if (p->struct_bytes != sizeof(RnfFlowPass))
        return fail("RnfFlowPass.struct_bytes=%zu, the library's is %zu: header and library differ", p->struct_bytes, sizeof(RnfFlowPass));
    if (p->dir != 0 && p->dir != 1) return fail("RnfFlowPass.dir=%d must be 0 (Flow.forward) or 1 (Flow.inverse)", (int)p->dir);
    if ((p->fisher_A == nullptr) != (p->fisher_c == nullptr)) return fail("RnfFlowPass.fisher_A and fisher_c must both be given or both be null");
    if (p->feature_div < 0) return fail("RnfFlowPass.feature_div=%lld is negative", (long long)p->feature_div);
    const bool logp = p->fisher_A || p->logp_out || p->sum_out;
    if (logp && p->dir) return fail("RnfFlowPass: fisher_A / logp_out / sum_out (log p) need dir 0");
    if (p->states && (p->feature_div > 0 || logp)) return fail("RnfFlowPass.states (training pass) takes neither feature_div nor fisher_A / logp_out / sum_out");
    if (p->side && p->feature_div > 0) return fail("RnfFlowPass.side with feature_div > 0 is not built: expand the shared feature rows");
    if (p->states && p->n > 0 && !p->rotation_out) return fail("RnfFlowPass.states needs rotation_out (the backward sweep reads the pass's output)");
    return run_flow(*p);
}

extern "C" size_t rnf_flow_pass_workspace_bytes(const RnfFlowPass *p) {
    if (check_struct(p, "RnfFlowPass")) return 0;
    int n_slots;
    bool any_mlp;
    desc_slots(p->desc, p->n_layers, &n_slots, &any_mlp);
    size_t stash_at;
    return flow_workspace(*p, n_slots, any_mlp, needs_stash(*p, any_mlp) ? device_cus() : 0, &stash_at);
}

// ------------------------------------------------------------------------------------------------------------
// training: forward that saves per-layer states, and the reverse sweep (train_kernels.h)
// ------------------------------------------------------------------------------------------------------------
// ConditionalTransform(F, <= 16 outputs)(feature) alone (flow/condition.py:24-30): the nets of ConditionRot (flow/rottrans.py:40) and
// ConditionLU (flow/squeezetrans.py:117-119), whose outputs the reference post-processes with batched torch ops.  Records from
// rnf_pack_cond16 (rows beyond the net's outputs zero); out [n][16], output o of the net in column o.
// bf16x3 (PREC 2) images in the LDS of the standalone kernels: the two head units of Mlp<2>::head_ring back to back -- Ha = [fc_first | hidden
// tiles 0..2 | hidden biases], Hb = [hidden tiles 3..5 | hidden biases] -- then the fc_last tile(s); 22,176 floats (87 KiB) with one tile
struct B3Head {
    static constexpr int HA = 0, HB = Mlp<2>::HA_FLOATS, LAST = HB + Mlp<2>::HB_FLOATS;
    static constexpr int HEAD_TILE_FLOATS = LAST + Lay<2>::LAST_TILE_FLOATS;
    // the head of a Lay<2> record (hidden biases once, behind tile 5) -> Ha, Hb; Hb is one contiguous piece of the record
    static __device__ __forceinline__ void stage(float *lds, const float *rec, int tid, int nthreads) {
        stage_floats(lds + HA, rec, Mlp<2>::HA_BIAS, tid, nthreads);
        stage_floats(lds + HA + Mlp<2>::HA_BIAS, rec + Lay<2>::HB, MOB_HB_FLOATS, tid, nthreads);
        stage_floats(lds + HB, rec + Mlp<2>::HA_BIAS, Mlp<2>::HB_FLOATS, tid, nthreads);
    }
    // head_ring's unit control: both units are already resident
    struct Units {
        const float *lds;
        int next = 0;
        __device__ __forceinline__ const float *begin_unit() { return lds + (next++ ? HB : HA); }
    };
};
static_assert(Mlp<2>::HA_BIAS + MOB_HB_FLOATS == Mlp<2>::HA_FLOATS && Mlp<2>::HA_BIAS + Mlp<2>::HB_FLOATS == Lay<2>::HEAD_FLOATS,
              "B3Head: Hb is the record's head from hidden tile 3 on");

template <int NWc, int PREC>
__global__ __launch_bounds__(NWc * 64) void cond_mlp_kernel(const float *G, long long g_groups, long long n, const float *layer, float *out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const long long ntiles = (n + NWc * 32 - 1) / (NWc * 32);
    if constexpr (PREC == 2) {
        B3Head::stage(lds, layer, tid, NWc * 64);
        stage_floats(lds + B3Head::LAST, layer + Lay<2>::LAST, Lay<2>::LAST_TILE_FLOATS, tid, NWc * 64);
    } else {
        stage_floats(lds, layer, MOB_HEAD_FLOATS + MOB_LAST_TILE_FLOATS, tid, NWc * 64);
    }
    __syncthreads();
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long group = tile * NWc + wave;
        const long long sample = group * 32 + j;
        typename Mlp<PREC>::Act tt;
        bool bad = false;
        GFrag<false> g{G + (size_t)group * G_FLOATS_PER_GROUP, false};
        f32x16 o;
        if constexpr (PREC == 2) {
            B3Head::Units units{lds};
            Mlp<2>::head_ring<GFrag<false>, false>(units, lane, h, 0.f, 0.f, 0.f, g, tt, bad);
            o = Mlp<2>::last(lds + B3Head::LAST, lane, h, tt);
        } else {
            Fair nofair{lds, wave, -1, 0};
            Mlp<PREC>::head(lds, lane, h, 0.f, 0.f, 0.f, g, tt, nofair, bad);
            o = Mlp<PREC>::last(lds + MOB_LAST, lane, h, tt);
        }
        if (sample < n) {
#pragma unroll
            for (int gq = 0; gq < 2; ++gq) {              // packed row 8g + 4h + c  <->  output 4 (2g + h) + c (rnf_pack_cond16)
                float4 v = make_float4(o[4 * gq], o[4 * gq + 1], o[4 * gq + 2], o[4 * gq + 3]);
                if (bad) v = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
                reinterpret_cast<float4 *>(out + sample * 16)[2 * gq + h] = v;
            }
        }
    }
}

extern "C" int rnf_cond_mlp_forward(const float *feat, int64_t n, int32_t F, const float *blob, int32_t layer_off, int32_t feat_off,
                                    int32_t prec, float *out, void *ws, size_t ws_bytes, void *stream_v) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    if (n < 0) return fail("n=%lld is negative", (long long)n);
    if (F <= 0 || F % 8) return fail("feature_dim=%d must be a positive multiple of 8 (pad on the host)", F);
    if (prec != RNF_PREC_FP32 && prec != RNF_PREC_F16X2 && prec != RNF_PREC_BF16X3) return fail("unknown precision %d", prec);
    if (layer_off < 0 || layer_off % 4 || feat_off < 0 || feat_off % 4) return fail("record offsets must be non-negative multiples of 4");
    if (n == 0) return 0;
    if (!feat || !blob || !out || !ws) return fail("rnf_cond_mlp_forward: null pointer");
    if (ws_bytes < rnf_workspace_bytes(n, 1)) return fail("workspace of %zu bytes is smaller than the %zu needed", ws_bytes, rnf_workspace_bytes(n, 1));
    float *G = reinterpret_cast<float *>(reinterpret_cast<char *>(ws) + PARTIALS_BYTES);
    const int cus = device_cus();
    const size_t lds_bytes = sizeof(float) * (prec == RNF_PREC_BF16X3 ? B3Head::HEAD_TILE_FLOATS : MOB_HEAD_FLOATS + MOB_LAST_TILE_FLOATS);
    for (long long base = 0; base < n; base += CHUNK_SAMPLES) {
        const long long cn = (n - base) < CHUNK_SAMPLES ? (n - base) : CHUNK_SAMPLES;
        const long long ntiles = (cn + NW * 32 - 1) / (NW * 32), ntiles_fp = (cn + NW_FP * 32 - 1) / (NW_FP * 32);
        const long long groups = (ntiles * NW > ntiles_fp * NW_FP) ? ntiles * NW : ntiles_fp * NW_FP;
        FeatProjArgs fp;
        std::memset(&fp, 0, sizeof(fp));
        fp.feat = feat + base * F; fp.blob = blob; fp.G = G; fp.n = cn; fp.g_groups = groups; fp.F = F; fp.n_slots = 1; fp.row_mode = 0;
        fp.feat_off[0] = feat_off;
        const int grid = (int)(ntiles < cus ? ntiles : cus);
        // exact fp32 and bf16x3: the exact-fp32 projection (as the flow pass projects)
        if (int rc = launch_projection(plan_projection_rows(cn, F, prec == RNF_PREC_F16X2 ? 1 : 0, cus), fp, stream)) return rc;
        auto kern = prec == RNF_PREC_BF16X3 ? cond_mlp_kernel<NW, 2> : (prec ? cond_mlp_kernel<NW, 1> : cond_mlp_kernel<NW, 0>);
        if (int rc = launch(kern, grid, NW * 64, lds_bytes, stream, (const float *)G, groups, cn, blob + layer_off, out + base * 16)) return rc;
    }
    return 0;
}

// ConditionRot (flow/rottrans.py:37-66): rot = U^T V of svd(I + reshape(net(feature), 4, 4)) per sample, with the SIGN CONVENTIONS of the
// reference's torch.svd (LAPACK sgesdd; svd4_lapack.h restates that path for 4x4).  mlp_out [n][16] = the conditioner's outputs (row-major
// 4x4 per sample), rot_out [n][16] = the orthogonal matrix the RNF_LAYER_SIDE16_ROT layer applies to the quaternion.  One thread per sample.
// usv != nullptr: also U [n][16] (row-major), the singular values [n][4] and V^T [n][16], for the analytic backward of U^T V (rottrans.py).
__global__ void condrot_utv_kernel(const float *mlp_out, long long n, float *rot_out, float *u_out, float *s_out, float *vt_out, int *fail_flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float A[16], U[16], sv[4], VT[16];
    for (int k = 0; k < 16; ++k) A[k] = mlp_out[i * 16 + k] + ((k % 5 == 0) ? 1.0f : 0.0f);
    if (!svd4::svd(A, U, sv, VT) && fail_flag) atomicOr(fail_flag, 1);
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {                                   // rot = U^T V: rot[r][c] = u_r . v_c
            float a = 0.f;
            for (int k = 0; k < 4; ++k) a += U[4 * k + r] * VT[4 * c + k];
            rot_out[i * 16 + 4 * r + c] = a;
        }
    if (u_out) {
        for (int k = 0; k < 16; ++k) { u_out[i * 16 + k] = U[k]; vt_out[i * 16 + k] = VT[k]; }
        for (int k = 0; k < 4; ++k) s_out[i * 4 + k] = sv[k];
    }
}
static int condrot_launch(const float *mlp_out, int64_t n, float *rot_out, float *u, float *sv, float *vt, int32_t *fail_flag, void *stream) {
    if (n < 0) return fail("rnf_condrot: n=%lld", (long long)n);
    if (n == 0) return 0;
    if (!mlp_out || !rot_out) return fail("rnf_condrot: null pointer");
    hipLaunchKernelGGL(condrot_utv_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), mlp_out, (long long)n,
                       rot_out, u, sv, vt, reinterpret_cast<int *>(fail_flag));
    HIP_TRY(hipGetLastError());
    return 0;
}
extern "C" int rnf_condrot_matrices(const float *mlp_out, int64_t n, float *rot_out, int32_t *fail_flag, void *stream) {
    return condrot_launch(mlp_out, n, rot_out, nullptr, nullptr, nullptr, fail_flag, stream);
}
extern "C" int rnf_condrot_svd(const float *mlp_out, int64_t n, float *rot_out, float *u_out, float *s_out, float *vt_out, int32_t *fail_flag,
                               void *stream) {
    if (n > 0 && (!u_out || !s_out || !vt_out)) return fail("rnf_condrot_svd: null factor pointer");
    return condrot_launch(mlp_out, n, rot_out, u_out, s_out, vt_out, fail_flag, stream);
}

// ConditionLU (flow/squeezetrans.py:94-131) on the device (round 6; until round 5 the host ran the reference's einsum / torch.diag on the GPU):
//     weight[n] = w_p . (reshape(wl[n], C, C) * l_mask + l_eye) . (reshape(wu[n], C, C) * u_mask + dvec),   dvec[d] = s_sign[d] exp(ws[d][d])
// `torch.diag` of the 2-D [N, C] tensor s_sign * exp(ws) (squeezetrans.py:126-127) is its DIAGONAL ACROSS THE BATCH -- entry d of row d,
// d < C -- and the resulting C-vector is broadcast over the last axis of every sample's upper factor: it is added to EVERY row c of
// column d, and the weight of sample n depends on batch rows 0 .. C-1.  Reproduced as defined, a batch of ONE row included: torch.diag of
// a [1, C] tensor is the one-entry vector s_sign[0] exp(ws[0][0]), which broadcasts to every column (dvec[d] = that entry for all d, its
// gradient the sum over the columns); 2 .. C-1 rows have a diagonal of the wrong length and fail in the reference, and here.  consts = w_p [C*C] | l_mask [C*C] |
// u_mask [C*C] | l_eye [C*C] | s_sign [C] (the module's buffers, as loaded from the checkpoint).  One thread per sample; out [n][16]:
// the C x C matrix row-major in the first C*C floats (+ identity when add_identity: Condition9TransLU, squeezetrans.py:269-271), rest 0.
template <int C>
__global__ void condlu_assemble_kernel(const float *wl, const float *wu, const float *ws, int sl, int su, int ss, long long n, const float *consts,
                                       int add_identity, float *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int CC = C * C;
    const float *wp = consts, *lm = consts + CC, *um = consts + 2 * CC, *le = consts + 3 * CC, *sg = consts + 4 * CC;
    float dvec[C], Lm[CC], Um[CC], PL[CC];
#pragma unroll
    for (int d = 0; d < C; ++d) dvec[d] = n == 1 ? sg[0] * expf(ws[0]) : sg[d] * expf(ws[(long long)d * ss + d]);       // rows 0 .. C-1 of the BATCH
#pragma unroll
    for (int k = 0; k < CC; ++k) {
        Lm[k] = wl[i * sl + k] * lm[k] + le[k];
        Um[k] = wu[i * su + k] * um[k] + dvec[k % C];
    }
#pragma unroll
    for (int a = 0; a < C; ++a)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float t = 0.f;
#pragma unroll
            for (int b = 0; b < C; ++b) t = fmaf(wp[a * C + b], Lm[b * C + c], t);
            PL[a * C + c] = t;
        }
    float o[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) o[k] = 0.f;
#pragma unroll
    for (int a = 0; a < C; ++a)
#pragma unroll
        for (int d = 0; d < C; ++d) {
            float t = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) t = fmaf(PL[a * C + c], Um[c * C + d], t);
            o[a * C + d] = t + ((add_identity && a == d) ? 1.0f : 0.0f);
        }
    float4 *dst = reinterpret_cast<float4 *>(out + i * 16);
    dst[0] = make_float4(o[0], o[1], o[2], o[3]); dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    dst[2] = make_float4(o[8], o[9], o[10], o[11]); dst[3] = make_float4(o[12], o[13], o[14], o[15]);
}

// Backward of the assembly: g [n][16] = dL/d(weight).  dL/dL = P^T G U^T, dL/dU = (P L)^T G; g_wl = dL/dL * l_mask, g_wu = dL/dU * u_mask
// (row stride gstride), and the batch-coupled diagonal collects  g_dvec[d] = sum_n sum_c dL/dU[n][c][d]  (wave sums, then one float atomic
// per wave and column into dsum [C], zeroed by the launcher).  condlu_diag_kernel then writes g_ws: zero everywhere except
// g_ws[d][d] = g_dvec[d] * dvec[d]  (d dvec[d] / d ws[d][d] = dvec[d]).
template <int C>
__global__ void condlu_backward_kernel(const float *wl, const float *wu, const float *ws, int sl, int su, int ss, long long n, const float *consts,
                                       const float *g, float *g_wl, float *g_wu, int gsl, int gsu, float *dsum) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int CC = C * C;
    const float *wp = consts, *lm = consts + CC, *um = consts + 2 * CC, *le = consts + 3 * CC, *sg = consts + 4 * CC;
    float dcol[C];
#pragma unroll
    for (int d = 0; d < C; ++d) dcol[d] = 0.f;
    if (i < n) {
        float dvec[C], Lm[CC], Um[CC], PL[CC], PtG[CC], G[CC];
#pragma unroll
        for (int d = 0; d < C; ++d) dvec[d] = n == 1 ? sg[0] * expf(ws[0]) : sg[d] * expf(ws[(long long)d * ss + d]);
#pragma unroll
        for (int k = 0; k < CC; ++k) {
            Lm[k] = wl[i * sl + k] * lm[k] + le[k];
            Um[k] = wu[i * su + k] * um[k] + dvec[k % C];
            G[k] = g[i * 16 + k];
        }
#pragma unroll
        for (int a = 0; a < C; ++a)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float t = 0.f, u = 0.f;
#pragma unroll
                for (int b = 0; b < C; ++b) {
                    t = fmaf(wp[a * C + b], Lm[b * C + c], t);            // (P L)[a][c]
                    u = fmaf(wp[b * C + a], G[b * C + c], u);             // (P^T G)[a][c]
                }
                PL[a * C + c] = t;
                PtG[a * C + c] = u;
            }
#pragma unroll
        for (int b = 0; b < C; ++b)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float gl = 0.f, gu = 0.f;
#pragma unroll
                for (int d = 0; d < C; ++d) {
                    gl = fmaf(PtG[b * C + d], Um[c * C + d], gl);         // dL/dL[b][c] = sum_d (P^T G)[b][d] U[c][d]
                    gu = fmaf(PL[d * C + b], G[d * C + c], gu);           // dL/dU[b][c] = sum_a (P L)[a][b] G[a][c]
                }
                g_wl[i * gsl + b * C + c] = gl * lm[b * C + c];
                g_wu[i * gsu + b * C + c] = gu * um[b * C + c];
                dcol[c] += gu;
            }
    }
#pragma unroll
    for (int d = 0; d < C; ++d) {
        float v = dcol[d];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v != 0.f) atomicAdd(dsum + d, v);
    }
}
template <int C>
__global__ void condlu_diag_kernel(const float *ws, int ss, long long n, const float *consts, const float *dsum, float *g_ws, int gss) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *sg = consts + 4 * C * C;
#pragma unroll
    for (int d = 0; d < C; ++d) g_ws[i * gss + d] = (i == d) ? dsum[d] * sg[d] * expf(ws[(long long)d * ss + d]) : 0.f;
    if (n == 1) {                                   // the one-entry diagonal feeds every column: its gradient collects all of them
        float t = 0.f;
#pragma unroll
        for (int d = 0; d < C; ++d) t += dsum[d];
        g_ws[0] = t * sg[0] * expf(ws[0]);
    }
}
extern "C" int rnf_condlu_matrices(const float *wl, const float *wu, const float *ws, int32_t stride_wl, int32_t stride_wu, int32_t stride_ws, int64_t n,
                                   int32_t C, const float *consts, int32_t add_identity, float *side_out, void *stream) {
    if (C != 3 && C != 4) return fail("rnf_condlu_matrices: in_channel %d (3 or 4)", C);
    if (n < 0 || stride_wl < C * C || stride_wu < C * C || stride_ws < C) return fail("rnf_condlu_matrices: n=%lld row strides %d %d %d", (long long)n, stride_wl, stride_wu, stride_ws);
    if (n == 0) return 0;
    // the reference broadcasts the vector torch.diag(...) of an [n, C] tensor (length min(n, C)) against [n, C, C]: 2 .. C-1 rows fail there,
    // one row broadcasts its single entry
    if (n > 1 && n < C) return fail("rnf_condlu_matrices: a batch of %lld rows has no %d-entry batch diagonal (flow/squeezetrans.py:126-127 fails to broadcast)", (long long)n, C);
    if (!wl || !wu || !ws || !consts || !side_out) return fail("rnf_condlu_matrices: null pointer");
    const dim3 grid((unsigned)((n + 127) / 128)), block(128);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (C == 4) hipLaunchKernelGGL(condlu_assemble_kernel<4>, grid, block, 0, st, wl, wu, ws, stride_wl, stride_wu, stride_ws, (long long)n, consts, add_identity, side_out);
    else hipLaunchKernelGGL(condlu_assemble_kernel<3>, grid, block, 0, st, wl, wu, ws, stride_wl, stride_wu, stride_ws, (long long)n, consts, add_identity, side_out);
    HIP_TRY(hipGetLastError());
    return 0;
}
extern "C" int rnf_condlu_backward(const float *wl, const float *wu, const float *ws, int32_t stride_wl, int32_t stride_wu, int32_t stride_ws, int64_t n,
                                   int32_t C, const float *consts, const float *g_side, float *g_wl, float *g_wu, float *g_ws, float *scratch, void *stream) {
    if (C != 3 && C != 4) return fail("rnf_condlu_backward: in_channel %d (3 or 4)", C);
    if (n < 1 || (n > 1 && n < C) || stride_wl < C * C || stride_wu < C * C || stride_ws < C) return fail("rnf_condlu_backward: n=%lld row strides %d %d %d", (long long)n, stride_wl, stride_wu, stride_ws);
    if (!wl || !wu || !ws || !consts || !g_side || !g_wl || !g_wu || !g_ws || !scratch) return fail("rnf_condlu_backward: null pointer");
    const dim3 grid((unsigned)((n + 127) / 128)), block(128);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(scratch, 0, sizeof(float) * 4, st));
    if (C == 4) {
        hipLaunchKernelGGL(condlu_backward_kernel<4>, grid, block, 0, st, wl, wu, ws, stride_wl, stride_wu, stride_ws, (long long)n, consts, g_side, g_wl, g_wu, C * C, C * C, scratch);
        hipLaunchKernelGGL(condlu_diag_kernel<4>, grid, block, 0, st, ws, stride_ws, (long long)n, consts, scratch, g_ws, C);
    } else {
        hipLaunchKernelGGL(condlu_backward_kernel<3>, grid, block, 0, st, wl, wu, ws, stride_wl, stride_wu, stride_ws, (long long)n, consts, g_side, g_wl, g_wu, C * C, C * C, scratch);
        hipLaunchKernelGGL(condlu_diag_kernel<3>, grid, block, 0, st, ws, stride_ws, (long long)n, consts, scratch, g_ws, C);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// Training forward from the plain blob on 16-rotation workgroups (train_block16.h: flow_train_forward16_kernel): no packed blob, exact fp32.
// Built for the layer kinds of the reference's training recipes (Moebius, Uncondition16Trans / UnconditionRot, Condition16Trans) in the
// forward direction, at most TR_MAX_LAYERS layers; the caller keeps every other flow on rnf_flow_pass with states.
// Floats of the activation buffer the training forward can leave for the backward sweep: one slot of (256 + 4K rounded up to 16) x 16 floats
// per conditioner layer and 16-rotation block (train_block16.h).
static int act_rows_for(int32_t K) { return b16::ACT_HEAD_ROWS + (4 * K + 15) / 16 * 16; }
extern "C" size_t rnf_train_acts_floats(int64_t n, int32_t n_conditioner_layers, int32_t segments) {
    if (n <= 0 || n_conditioner_layers <= 0 || segments <= 0) return 0;
    return (size_t)n_conditioner_layers * (size_t)((n + b16::SB - 1) / b16::SB) * (size_t)act_rows_for(segments) * 16;
}

extern "C" int rnf_flow_forward_train_plain(const float *rot, const float *feat, int64_t n, int32_t F, const float *plain, const int32_t *tdesc,
                                            int32_t n_layers, int32_t K, float *rot_out, float *ldj_out, float *states, float *acts,
                                            void *stream_v) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    if (n < 0) return fail("n=%lld is negative", (long long)n);
    if (n_layers < 1 || n_layers > TR_MAX_LAYERS) return fail("rnf_flow_forward_train_plain: n_layers=%d outside [1,%d]", n_layers, TR_MAX_LAYERS);
    if (K < 1 || K > 512) return fail("rnf_flow_forward_train_plain: 1..512 segments, got %d", K);
    if (F < 0) return fail("feature_dim %d is negative", F);
    if (n == 0) return 0;
    if (!rot || !plain || !tdesc || !rot_out || !ldj_out || !states) return fail("null pointer argument");
    b16::FwdArgs a;
    std::memset(&a, 0, sizeof(a));
    bool any_feature = false;
    for (int l = 0; l < n_layers; ++l) {
        const int32_t *d = tdesc + (size_t)l * 3;
        const int kind = d[0] & 15, orth = (d[0] >> 8) & 1;
        if ((d[0] & ~(15 | 256)) || (kind != RNF_KIND_MOBIUS && kind != RNF_KIND_AFFINE16 && kind != RNF_KIND_COND16))
            return fail("rnf_flow_forward_train_plain: layer %d (kind %d) is not built here; use rnf_flow_pass with states", l, d[0]);
        if (d[1] < 0 || d[1] > 5) return fail("layer %d: perm_row %d outside [0,5]", l, d[1]);
        if (d[2] < 0) return fail("layer %d: negative plain offset", l);
        if (kind == RNF_KIND_COND16 && F == 0) return fail("layer %d: a conditional affine layer needs a feature", l);
        any_feature = any_feature || (kind != RNF_KIND_AFFINE16 && F > 0);
        a.layers[l] = make_int2(kind | (d[1] << 4) | (orth << 8), d[2]);
    }
    if (any_feature && !feat) return fail("conditional layers but feature pointer is null");
    a.rot = rot; a.feature = F ? feat : nullptr; a.plain = plain; a.rot_out = rot_out; a.ldj_out = ldj_out; a.states = states;
    a.n = n; a.n_layers = n_layers; a.K = K; a.F = F;
    a.acts = acts; a.act_rows = act_rows_for(K);
    const size_t rows = (4 * (size_t)K + 63) / 64 * 64;
    const size_t lds_bytes = sizeof(float) * (b16::HEAD_FLOATS + rows * b16::LR);
    const long long nblocks = (n + b16::SB - 1) / b16::SB;
    const long long cap = (long long)device_cus() * 4;
    const dim3 grid((unsigned)(nblocks < cap ? nblocks : cap)), block(b16::WAVES * 64);
    return launch(F ? b16::flow_train_forward16_kernel<true> : b16::flow_train_forward16_kernel<false>, (int)grid.x, (int)block.x, lds_bytes, stream, a);
}

extern "C" int rnf_pack_flow_device(const float *plain, const int32_t *pdesc, int32_t n_layers, int32_t K, int32_t F, int32_t prec,
                                    float *blob, int32_t *flags, void *stream_v) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    if (n_layers < 0 || n_layers > MAX_LAYERS) return fail("n_layers=%d outside [0,%d] (device packer)", n_layers, MAX_LAYERS);
    if (K <= 0) return fail("segments=%d must be positive", K);
    if (F < 0) return fail("feature_dim %d is negative", F);
    if (prec != RNF_PREC_FP32 && prec != RNF_PREC_F16X2 && prec != RNF_PREC_BF16X3) return fail("unknown precision %d", prec);
    if (n_layers == 0) return 0;
    if (!plain || !pdesc || !blob || !flags) return fail("null pointer argument");
    PackArgs a;
    std::memset(&a, 0, sizeof(a));
    a.plain = plain; a.blob = blob; a.flags = flags;
    a.n_layers = n_layers; a.K = K; a.F = F; a.Fp = (F + 7) / 8 * 8; a.prec = prec;
    a.equalise = (prec == RNF_PREC_F16X2 && equalise_allowed()) ? 1 : 0;
    a.feat_ms = g_feature_ms;
    for (int l = 0; l < n_layers; ++l) {
        const int32_t *d = pdesc + (size_t)l * 4;
        const int kind = d[0] & 15;
        if ((d[0] & ~(15 | 256)) || (kind != RNF_KIND_MOBIUS && kind != RNF_KIND_AFFINE16 && kind != RNF_KIND_COND16 && kind != RNF_KIND_GS9 &&
                                     kind != RNF_KIND_GS36 && kind != RNF_KIND_COND36 && !kind_is_cond9(kind) && !kind_is_side(kind)))
            return fail("layer %d: unknown kind %d", l, d[0]);
        if (d[1] < 0 || d[2] < 0 || d[2] % 4 || (d[3] >= 0 && d[3] % 4)) return fail("layer %d: bad offsets", l);
        if ((kind == RNF_KIND_COND16 || kind == RNF_KIND_COND36 || kind_is_cond9(kind)) && F == 0) return fail("layer %d: a conditional affine layer needs a feature", l);
        if (kind_has_mlp(kind) && (F > 0) != (d[3] >= 0)) return fail("layer %d: feature record offset does not match feature_dim", l);
    }
    const int pk_chunk = layer_chunk(PK_MAX_LAYERS);
    for (int base = 0; base < n_layers; base += pk_chunk) {            // the layer table travels as a kernel argument: PK_MAX_LAYERS per launch
        const int cnt = n_layers - base < pk_chunk ? n_layers - base : pk_chunk;
        for (int l = 0; l < cnt; ++l) {
            const int32_t *d = pdesc + (size_t)(base + l) * 4;
            a.layers[l] = PackLayer{d[0], d[1], d[2], d[3]};
        }
        a.n_layers = cnt;
        if (prec == RNF_PREC_BF16X3) hipLaunchKernelGGL(pack_flow_kernel<true>, dim3(8, cnt), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(pack_flow_kernel<false>, dim3(8, cnt), dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" size_t rnf_plain_layer_floats(int32_t kind, int32_t segments, int32_t feature_dim) {
    if (kind == RNF_KIND_AFFINE16) return 16;
    if (kind == RNF_KIND_GS9) return 12;
    if (kind == RNF_KIND_GS36) return 36;
    if (kind_is_side(kind)) return 0;
    const size_t ni = (kind == RNF_KIND_MOBIUS ? 3 : 0) + (size_t)feature_dim,
                 no = kind == RNF_KIND_MOBIUS ? 4 * (size_t)segments : (kind_is_cond9(kind) ? 9 : (kind == RNF_KIND_COND36 ? 36 : 16));
    return 64 * ni + 64 + 3 * (4096 + 64) + no * 64 + no;
}

// g_out_ext: dL/d(outputs) [n][NO] of an RNF_KIND_MLP_ONLY table (rnf_cond_mlp_backward)
static int run_backward(const RnfFlowBackward &x, const float *g_out_ext = nullptr) {
    const float *states = x.states, *feat = x.feature, *g_rot_out = x.g_rotation_out, *g_ldj = x.g_ldj;
    const float *rot_final = x.dir ? x.rotation_out : nullptr;
    static const float dummy = 0.f;                      // side-layer flows may have no plain parameters at all
    const float *plain = x.plain ? x.plain : (x.side ? &dummy : nullptr);
    const int32_t *tdesc = x.train_desc;
    const int64_t n = x.n;
    const int32_t F = x.feature_dim, n_layers = x.n_layers, K = x.segments;
    float *grads = x.grads, *g_rot_in = x.g_rotation_in, *g_feature = x.g_feature, *g_ldj_sum = x.layer_scratch;
    hipStream_t stream = reinterpret_cast<hipStream_t>(x.stream);
    if (n < 0) return fail("n=%lld is negative", (long long)n);
    if (n_layers < 0 || n_layers > MAX_LAYERS) return fail("n_layers=%d outside [0,%d] (training path)", n_layers, MAX_LAYERS);
    if (K < 1 || K > 512) return fail("training path supports 1..512 segments, got %d", K);
    if (F < 0) return fail("feature_dim %d is negative", F);
    if (n == 0) return 0;
    const bool mlp_only = n_layers == 1 && (tdesc[0] & 15) == RNF_KIND_MLP_ONLY;
    if (!plain || !tdesc || !g_ldj_sum) return fail("null pointer argument");
    if (!mlp_only && (!states || !g_ldj || !g_rot_in)) return fail("null pointer argument");
    TrainArgs a;
    std::memset(&a, 0, sizeof(a));
    bool rare = false;        // side / Gram-Schmidt / conditional 3x3 layers present: the instantiation that carries them (train_block16.h)
    std::vector<int2> table((size_t)n_layers);
    for (int l = 0; l < n_layers; ++l) {
        const int32_t *d = tdesc + (size_t)l * 3;
        const int kind = d[0] & 15, orth = (d[0] >> 8) & 1, aux = (d[0] >> 16) & 255;
        rare = rare || kind_is_side(kind) || kind == RNF_KIND_GS9 || kind == RNF_KIND_GS36 || kind == RNF_KIND_COND36 || kind_is_cond9(kind);
        if ((d[0] & ~(15 | 256 | (255 << 16))) ||
            (kind != RNF_KIND_MOBIUS && kind != RNF_KIND_AFFINE16 && kind != RNF_KIND_COND16 && kind != RNF_KIND_GS9 && kind != RNF_KIND_GS36 &&
             kind != RNF_KIND_COND36 && !kind_is_cond9(kind) && !kind_is_side(kind) && !(kind == RNF_KIND_MLP_ONLY && mlp_only)))
            return fail("layer %d: kind %d has no backward kernel", l, d[0]);
        if (kind_is_side(kind) && (!x.side || !x.side_grad)) return fail("layer %d is a side layer: RnfFlowBackward.side / side_grad are needed", l);
        if (kind == RNF_KIND_MLP_ONLY && (aux < 1 || aux > 64 || !g_out_ext || F <= 0)) return fail("rnf_cond_mlp_backward: 1..64 outputs, a feature and dL/d(outputs) are needed");
        if (x.acts && kind != RNF_KIND_MOBIUS && kind != RNF_KIND_AFFINE16 && kind != RNF_KIND_COND16)
            return fail("RnfFlowBackward.acts: layer %d (kind %d) has no saved activations (rnf_flow_forward_train_plain does not run it)", l, kind);
        if (d[1] < 0 || d[1] > 5) return fail("layer %d: perm_row %d outside [0,5]", l, d[1]);
        if (kind_has_mlp(kind) && F > 0 && !feat) return fail("conditional layer %d but feature pointer is null", l);
        if ((kind == RNF_KIND_COND16 || kind == RNF_KIND_COND36 || kind_is_cond9(kind)) && F == 0) return fail("layer %d: a conditional affine layer needs a feature", l);
        if (d[2] < 0) return fail("layer %d: negative plain offset", l);
        table[l] = make_int2(kind | (d[1] << 4) | (orth << 8) | (aux << 16), d[2]);
    }
    a.side = x.side; a.side_grad = x.side_grad; a.g_out_ext = g_out_ext;
    a.feature = F ? feat : nullptr; a.plain = plain; a.grads = grads; a.g_ldj = g_ldj;
    a.g_rot_in = g_rot_in; a.g_feature = F ? g_feature : nullptr;
    a.n = n; a.K = K; a.F = F;
    a.dir = x.dir;
#ifdef RNF_STAMPS
    {   // diagnostic build: RNF_TRAIN_STAMPS_PTR=<device address of 10 zeroed uint64> (tools/phase_stamps_train.py)
        const char *sp = std::getenv("RNF_TRAIN_STAMPS_PTR");
        a.stamps = sp ? reinterpret_cast<unsigned long long *>(std::strtoull(sp, nullptr, 0)) : nullptr;
    }
#endif
    const size_t rows = (4 * (size_t)K + 63) / 64 * 64;      // conditioner-output rows, padded to whole 64-row slabs (train_kernels.h)
    // Block size of the sweep: 16-rotation workgroups (train_block16.h: a quarter of the dependent matrix chain per workgroup, four times
    // as many workgroups, K up to 512) or 64-rotation ones (train_kernels.h: a quarter of the weight traffic and gradient atomics, K <= 64).
    const int blk_sel = train_block();
    const bool block16 = blk_sel == 16 || K > 64 || (blk_sel == 0 && n < kTrainBlock64From);
    if (blk_sel == 64 && K > 64) return fail("RNF_TRAIN_BLOCK=64: the 64-rotation backward kernel holds at most 64 segments, got %d", K);
    // The layer table travels as a kernel argument, TR_MAX_LAYERS entries per launch: a deeper stack is swept in chunks from the top, each
    // chunk starting from the rotation gradient the previous one left in g_rot_in (read at the start of a block, written at its end, by the
    // same workgroup) and reading its own slice of the saved states; dL/dldj is the same per-rotation value for every layer.
    const int tr_chunk = layer_chunk(TR_MAX_LAYERS);
    for (int hi = n_layers; hi > 0 || n_layers == 0; ) {
        const int lo = hi > tr_chunk ? hi - tr_chunk : 0;
        for (int l = lo; l < hi; ++l) a.layers[l - lo] = table[l];
        a.n_layers = hi - lo;
        a.states = states ? states + (size_t)lo * (size_t)n * 9 : nullptr;
        a.rot_final = hi == n_layers ? rot_final : states + (size_t)hi * (size_t)n * 9;      // (dir = 1: the output of the chunk's last position)
        a.g_rot_out = hi == n_layers ? g_rot_out : g_rot_in;
        a.g_ldj_sum = g_ldj_sum + lo;
        a.acts = block16 ? x.acts : nullptr;
        a.act_rows = act_rows_for(K);
        a.mlp_base = 0;
        for (int l = 0; l < lo; ++l) a.mlp_base += ((table[l].x & 15) == RNF_KIND_MOBIUS || (table[l].x & 15) == RNF_KIND_COND16) ? 1 : 0;
        if (block16) {
            const size_t lds_bytes = sizeof(float) * (b16::HEAD_FLOATS + rows * b16::LR);
            const long long nblocks = (n + b16::SB - 1) / b16::SB;
            const long long cap = (long long)device_cus() * 4;
            const dim3 grid((unsigned)(nblocks < cap ? nblocks : cap)), block(b16::WAVES * 64);
            auto kern = F ? (rare ? b16::flow_train_backward16_kernel<true, true> : b16::flow_train_backward16_kernel<true, false>)
                          : (rare ? b16::flow_train_backward16_kernel<false, true> : b16::flow_train_backward16_kernel<false, false>);
            if (int rc = launch(kern, (int)grid.x, (int)block.x, lds_bytes, stream, a)) return rc;
        } else {
            const size_t lds_bytes = sizeof(float) * (TR_LDS_HEAD_FLOATS + rows * LROW);
            const long long nblocks = (n + 63) / 64;
            const int cap = device_cus() * 4;
            const dim3 grid((unsigned)(nblocks < cap ? nblocks : cap)), block(TR_WAVES * 64);
            if (int rc = launch(F ? flow_train_backward_kernel<true> : flow_train_backward_kernel<false>, (int)grid.x, (int)block.x, lds_bytes, stream, a)) return rc;
        }
        if (a.n_layers) {
            hipLaunchKernelGGL(affine_logdet_grad_kernel, dim3((a.n_layers + 63) / 64), dim3(64), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
        hi = lo;
        if (n_layers == 0) break;
    }
    return 0;
}

extern "C" int rnf_flow_backward_pass(const RnfFlowBackward *p) {
    if (!p) return fail("RnfFlowBackward pointer is null");
    if (p->struct_bytes != sizeof(RnfFlowBackward))
        return fail("RnfFlowBackward.struct_bytes=%zu, the library's is %zu: header and library differ", p->struct_bytes, sizeof(RnfFlowBackward));
    if (p->dir != 0 && p->dir != 1) return fail("RnfFlowBackward.dir=%d must be 0 (Flow.forward) or 1 (Flow.inverse)", (int)p->dir);
    if (p->dir == 1 && p->n > 0 && !p->rotation_out)
        return fail("RnfFlowBackward.rotation_out is needed for dir 1: the output rotations of the inverse pass carry the roots");
    if (p->acts && p->dir) return fail("RnfFlowBackward.acts needs dir 0 (rnf_flow_forward_train_plain runs Flow.forward)");
    return run_backward(*p);
}

// Backward of ONE ConditionalTransform(feature_dim -> n_out) evaluated on its own (rnf_cond_mlp_forward; flow/condition.py:24-30): plain =
// its parameters in reference order (fc_first.weight [64][F], .bias, layers.{1,3,5}.weight/.bias, fc_last.weight [n_out][64], .bias),
// g_out [n][n_out] -> grads (same layout as plain, ACCUMULATED into; nullptr: feature gradient only) and g_feature [n][F] (ACCUMULATED
// into, or nullptr).  One launch of the training backward kernel with the layer math replaced by the caller's dL/d(outputs).
extern "C" int rnf_cond_mlp_backward(const float *feat, int64_t n, int32_t F, const float *plain, int32_t n_out, const float *g_out, float *grads,
                                     float *g_feature, float *scratch1, void *stream_v) {
    if (!feat || !plain || !g_out || !scratch1) return fail("rnf_cond_mlp_backward: null pointer");
    if (n_out < 1 || n_out > 64) return fail("rnf_cond_mlp_backward: n_out=%d outside [1,64]", (int)n_out);
    const int32_t tdesc[3] = {RNF_KIND_MLP_ONLY | (n_out << 16), 0, 0};
    RnfFlowBackward x{};
    x.struct_bytes = sizeof(x);
    x.feature = feat; x.n = n; x.feature_dim = F; x.plain = plain; x.train_desc = tdesc; x.n_layers = 1; x.segments = 8;
    x.grads = grads; x.g_feature = g_feature; x.layer_scratch = scratch1; x.stream = stream_v;
    return run_backward(x, g_out);
}

// ------------------------------------------------------------------------------------------------------------
// small standalone kernels
// ------------------------------------------------------------------------------------------------------------
__global__ void fisher_log_prob_kernel(const float *rot, long long n, const float *A, const float *c, long long div, float *out) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const long long row = i / div;
        float tr = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) tr = fmaf(rot[i * 9 + k], A[row * 9 + k], tr);
        out[i] = tr - c[row];
    }
}

extern "C" int rnf_fisher_log_prob(const float *rot, int64_t n, const float *A, const float *c, int64_t B, float *out, void *stream) {
    if (!rot || !A || !c || !out) return fail("rnf_fisher_log_prob: null pointer");
    if (B <= 0 || n % B) return fail("n=%lld not divisible by fisher rows B=%lld (utils/fisher.py:226)", (long long)n, (long long)B);
    if (n == 0) return 0;
    long long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(fisher_log_prob_kernel, dim3((int)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rot, (long long)n, A, c, (long long)(n / B), out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// eval_acc epilogue (agent.py:266-283, utils/utils.py:231-235): geodesic angle between an estimate and the closest of its K ground-truth
// rotations (K > 1: symmetric objects): acos(clip((max_k tr(E^T G_k) - 1) / 2, -1, 1)), one thread per estimate
__global__ void min_geodesic_kernel(const float *est, const float *gt, long long n, int k, float *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float e[9];
    for (int c = 0; c < 9; ++c) e[c] = est[i * 9 + c];
    float best = -4.0f;
    for (int q = 0; q < k; ++q) {
        const float *g = gt + ((size_t)i * k + q) * 9;
        float tr = 0.f;
        for (int c = 0; c < 9; ++c) tr = fmaf(e[c], g[c], tr);
        best = fmaxf(best, tr);
    }
    out[i] = acosf(fminf(fmaxf((best - 1.0f) * 0.5f, -1.0f), 1.0f));
}

extern "C" int rnf_min_geodesic(const float *est, const float *gt, int64_t n, int32_t k, float *out, void *stream) {
    if (n < 0 || k <= 0) return fail("rnf_min_geodesic: n=%lld k=%d", (long long)n, k);
    if (n == 0) return 0;
    if (!est || !gt || !out) return fail("rnf_min_geodesic: null pointer");
    hipLaunchKernelGGL(min_geodesic_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), est, gt, (long long)n, k, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Equivolumetric SO(3) grid of the grid-search pose estimate and its hierarchy: csrc/so3_grid.h.
extern "C" int rnf_so3_healpix_grid(int32_t level, const float *offset, float *out, void *stream) {
    if (level < 0 || level > 8) return fail("rnf_so3_healpix_grid: level=%d outside 0..8 (72 * 8^level rotations)", level);
    if (!out) return fail("rnf_so3_healpix_grid: null output pointer");
    const long long rows = 72LL << (3 * level);
    long long blocks = (rows + 255) / 256;
    if (blocks > (1LL << 20)) blocks = 1LL << 20;
    hipLaunchKernelGGL(so3g::so3_healpix_grid_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (int)level, rows,
                       offset, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int rnf_so3_grid_children(const RnfGridChildren *p) {
    if (check_struct(p, "RnfGridChildren")) return 1;
    if (p->level < 0 || p->level >= so3g::MAX_LEVEL)
        return fail("RnfGridChildren.level=%d outside 0..%d (children at level + 1 <= %d)", p->level, so3g::MAX_LEVEL - 1, so3g::MAX_LEVEL);
    if (p->n < 0 || p->n > (1LL << 36)) return fail("RnfGridChildren.n=%lld outside 0..2^36", (long long)p->n);
    if (p->n == 0) return 0;
    if (!p->parents || !p->rows_out) return fail("RnfGridChildren: null parents or rows_out");
    const long long total = p->n * 12;
    long long blocks = (total + 255) / 256;
    if (blocks > (1LL << 20)) blocks = 1LL << 20;
    hipLaunchKernelGGL(so3g::so3_grid_children_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(p->stream),
                       (int)p->level, (long long)p->n, (const long long *)p->parents, p->offset, (long long *)p->rows_out, p->rot_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Beam selection (csrc/grid_beam.h): passes of one-chunk-per-block sorts until one chunk per image remains.
static int grid_beam_check(const RnfGridBeamSelect *p) {
    if (check_struct(p, "RnfGridBeamSelect")) return 1;
    if (p->g < 1 || p->g > 65535) return fail("RnfGridBeamSelect.g=%d outside 1..65535", p->g);
    if (p->M < 1 || p->M > gb::ROW_MAX + 1) return fail("RnfGridBeamSelect.M=%lld outside 1..2^31 - 1", (long long)p->M);
    if (p->beam < 1 || p->beam > gb::MAX_BEAM) return fail("RnfGridBeamSelect.beam=%d outside 1..%d", p->beam, gb::MAX_BEAM);
    return 0;
}

extern "C" size_t rnf_grid_beam_select_workspace_bytes(const RnfGridBeamSelect *p) {
    if (grid_beam_check(p)) return 0;
    const long long nb = gb::blocks_for(p->M);
    // two ping-pong buffers of the first pass's keys; 8 bytes when a single pass suffices (never 0, which means an error)
    return nb > 1 ? 2 * (size_t)p->g * (size_t)nb * (size_t)p->beam * sizeof(unsigned long long) : 8;
}

extern "C" int rnf_grid_beam_select(const RnfGridBeamSelect *p) {
    if (grid_beam_check(p)) return 1;
    if (!p->logp || !p->rows_out || !p->logp_out) return fail("RnfGridBeamSelect: null logp or output pointer");
    const size_t need = rnf_grid_beam_select_workspace_bytes(p);
    if (check_workspace(p, "RnfGridBeamSelect", need, "rnf_grid_beam_select_workspace_bytes", 0)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    const int dedup = p->rows != nullptr;
    unsigned long long *ws = (unsigned long long *)p->workspace;
    unsigned long long *half = ws + (size_t)p->g * (size_t)gb::blocks_for(p->M) * (size_t)p->beam;
    const unsigned long long *in = nullptr;
    long long n = p->M;
    for (int pass = 0;; ++pass) {
        const long long nb = gb::blocks_for(n);
        unsigned long long *out = nb > 1 ? (pass & 1 ? half : ws) : nullptr;
        hipLaunchKernelGGL(gb::beam_select_kernel, dim3((unsigned)nb, (unsigned)p->g), dim3(gb::THREADS), 0, s, p->logp,
                           (const long long *)p->rows, in, n, dedup, (int)p->beam, out, (long long *)p->rows_out, p->logp_out);
        HIP_TRY(hipGetLastError());
        if (nb == 1) return 0;
        in = out;
        n = nb * p->beam;
    }
}

// Top-k pose modes on the grid (csrc/grid_modes.h): k arg-max passes and one mass pass, each followed by its per-image finalise.
static int grid_modes_check(const RnfGridModes *p) {
    if (check_struct(p, "RnfGridModes")) return 1;
    if (p->g < 1 || p->g > 65535) return fail("RnfGridModes.g=%d outside 1..65535", p->g);
    if (p->Q < 1) return fail("RnfGridModes.Q=%lld must be >= 1", (long long)p->Q);
    if (p->top_k < 1 || p->top_k > gm::MAX_K) return fail("RnfGridModes.top_k=%d outside 1..%d", p->top_k, gm::MAX_K);
    return 0;
}

extern "C" size_t rnf_grid_modes_workspace_bytes(const RnfGridModes *p) {
    if (grid_modes_check(p)) return 0;
    return (size_t)p->g * (size_t)gm::blocks_for(p->Q) * sizeof(double) * (size_t)(p->top_k + 2);
}

extern "C" int rnf_grid_modes(const RnfGridModes *p) {
    if (grid_modes_check(p)) return 1;
    if (!(p->separation_rad > 0.0 && p->separation_rad <= M_PI))
        return fail("RnfGridModes.separation_rad=%g outside (0, pi]", p->separation_rad);
    if (!p->logp || !p->grid || !p->index_out || !p->logp_out || !p->mass_out || !p->log_norm_out)
        return fail("RnfGridModes: null logp, grid or output pointer");
    if (check_aligned16(p->grid, nullptr, "RnfGridModes", ".grid")) return 1;
    if (p->gt && (p->n_gt < 1 || p->n_gt > gm::MAX_GT)) return fail("RnfGridModes.n_gt=%d outside 1..%d", p->n_gt, gm::MAX_GT);
    if (p->gt && !p->spread_out) return fail("RnfGridModes.gt needs spread_out");
    const size_t need = rnf_grid_modes_workspace_bytes(p);
    if (check_workspace(p, "RnfGridModes", need, "rnf_grid_modes_workspace_bytes", 0)) return 1;
    const float thr = p->separation_rad >= M_PI ? -INFINITY : (float)(1.0 + 2.0 * cos(p->separation_rad));
    const int nb = (int)gm::blocks_for(p->Q), k = p->top_k;
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    for (int j = 0; j < k; ++j) {
        hipLaunchKernelGGL(gm::grid_modes_argmax_kernel, dim3(nb, p->g), dim3(gm::THREADS), 0, s, p->logp, p->grid, (long long)p->Q, k, j, thr,
                           (const long long *)p->index_out, (const float *)p->logp_out, (gm::ArgPart *)p->workspace);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(gm::grid_modes_argmax_final_kernel, dim3(p->g), dim3(gm::THREADS), 0, s, (const gm::ArgPart *)p->workspace, nb, k, j,
                           (long long *)p->index_out, p->logp_out);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(gm::grid_modes_mass_kernel, dim3(nb, p->g), dim3(gm::THREADS), 0, s, p->logp, p->grid, (long long)p->Q, k, thr,
                       p->gt, p->gt ? p->n_gt : 0, (const long long *)p->index_out, (const float *)p->logp_out, (double *)p->workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gm::grid_modes_mass_final_kernel, dim3(p->g), dim3(gm::THREADS), 0, s, (const double *)p->workspace, nb, (long long)p->Q,
                       k, p->gt ? 1 : 0, (const long long *)p->index_out, (const float *)p->logp_out, p->mass_out, p->log_norm_out,
                       p->spread_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The row maximum of g images of Q log-densities -> max_index[g], max_value[g]: grid_modes.h's arg-max pass for one mode (k = 1, no grid,
// no separation) and its finalise.  The prologue of the credible sets, the histogram fit and the draws.
static int launch_row_max(const float *logp, long long Q, int g, gm::ArgPart *max_part, long long *max_index, float *max_value, hipStream_t s) {
    const int nbm = (int)gm::blocks_for(Q);
    hipLaunchKernelGGL(gm::grid_modes_argmax_kernel, dim3(nbm, g), dim3(gm::THREADS), 0, s, logp, (const float *)nullptr, Q, 1, 0, 0.0f,
                       (const long long *)max_index, (const float *)max_value, max_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gm::grid_modes_argmax_final_kernel, dim3(g), dim3(gm::THREADS), 0, s, (const gm::ArgPart *)max_part, nbm, 1, 0, max_index,
                       max_value);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Credible sets on the grid (csrc/grid_credible.h): the row maximum by grid_modes.h's arg-max pass, then 4 histogram passes of the radix
// select, each followed by its finalise.
static int grid_credible_check(const RnfGridCredible *p) {
    if (check_struct(p, "RnfGridCredible")) return 1;
    if (p->g < 1 || p->g > 65535) return fail("RnfGridCredible.g=%d outside 1..65535", p->g);
    if (p->Q < 1 || p->Q > gc::MAX_Q) return fail("RnfGridCredible.Q=%lld outside 1..2^26", (long long)p->Q);
    if (p->n_levels < 1 || p->n_levels > gc::MAX_LEVELS)
        return fail("RnfGridCredible.n_levels=%d outside 1..%d", p->n_levels, gc::MAX_LEVELS);
    if (p->n_queries < 0 || p->n_queries > gc::MAX_QUERIES)
        return fail("RnfGridCredible.n_queries=%d outside 0..%d", p->n_queries, gc::MAX_QUERIES);
    return 0;
}

extern "C" size_t rnf_grid_credible_workspace_bytes(const RnfGridCredible *p) {
    if (grid_credible_check(p)) return 0;
    return gc::carve(nullptr, p->Q, p->g, p->n_levels, p->n_queries).bytes;
}

extern "C" int rnf_grid_credible(const RnfGridCredible *p) {
    if (grid_credible_check(p)) return 1;
    if (!p->levels) return fail("RnfGridCredible: null levels");
    gc::Levels levels = {};
    for (int j = 0; j < p->n_levels; ++j) {
        if (!(p->levels[j] > 0.0 && p->levels[j] < 1.0)) return fail("RnfGridCredible.levels[%d]=%g outside (0, 1)", j, p->levels[j]);
        levels.a[j] = p->levels[j];
    }
    if (!p->logp || !p->threshold_out || !p->count_out || !p->mass_out || !p->log_norm_out)
        return fail("RnfGridCredible: null logp or output pointer");
    const int J = p->n_levels, G = p->n_queries;
    if (G > 0 && (!p->queries || !p->query_mass_out || !p->query_count_out))
        return fail("RnfGridCredible: null queries, query_mass_out or query_count_out with n_queries=%d", G);
    const size_t need = rnf_grid_credible_workspace_bytes(p);
    if (check_workspace(p, "RnfGridCredible", need, "rnf_grid_credible_workspace_bytes", 8)) return 1;
    const gc::Workspace w = gc::carve(p->workspace, p->Q, p->g, J, G);
    const long long Q = p->Q;
    const int nb = (int)gc::blocks_for(Q), S = gc::fixed_point_shift(Q);
    const double scale = ldexp(1.0, S);
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    if (launch_row_max(p->logp, Q, p->g, w.max_part, w.max_index, w.max_value, s)) return 1;
    for (int pass = 0; pass < gc::PASSES; ++pass) {
        const gc::State *prev = pass ? w.state + (size_t)(pass - 1) * p->g * J : nullptr;
        gc::State *next = w.state + (size_t)pass * p->g * J;
        if (pass == 0) {
            auto first = gc::grid_credible_first_kernel<gc::MAX_QUERIES>;
            switch (gc::query_slots(G)) {
                case 0: first = gc::grid_credible_first_kernel<0>; break;
                case 1: first = gc::grid_credible_first_kernel<1>; break;
                case 4: first = gc::grid_credible_first_kernel<4>; break;
            }
            hipLaunchKernelGGL(first, dim3(nb, p->g), dim3(gc::THREADS), 0, s, p->logp, Q, J, p->queries, G, scale,
                               (const float *)w.max_value, w.hist_mass, w.hist_count, w.query_mass, w.query_count);
        } else {
            hipLaunchKernelGGL(gc::grid_credible_pass_kernel, dim3(nb, p->g), dim3(gc::THREADS), 0, s, p->logp, Q, J, pass, scale,
                               (const float *)w.max_value, prev, w.hist_mass, w.hist_count);
        }
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(gc::grid_credible_final_kernel, dim3(J, p->g), dim3(gc::FINAL_THREADS), 0, s, Q, J, G, pass, nb, S, levels, p->queries,
                           (const float *)w.max_value, (const gc::u64 *)w.hist_mass, (const unsigned *)w.hist_count,
                           (const gc::u64 *)w.query_mass, (const unsigned *)w.query_count, prev, next, w.total, p->threshold_out,
                           (long long *)p->count_out, p->mass_out, p->log_norm_out, p->query_mass_out, (long long *)p->query_count_out);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// The cell of a rotation and the histogram over the cells (csrc/grid_locate.h): one thread per rotation.
extern "C" int rnf_so3_grid_locate(const RnfGridLocate *p) {
    if (check_struct(p, "RnfGridLocate")) return 1;
    if (p->level < 0 || p->level > so3g::MAX_LEVEL) return fail("RnfGridLocate.level=%d outside 0..%d", p->level, so3g::MAX_LEVEL);
    if (p->g < 1 || p->g > 65535) return fail("RnfGridLocate.g=%d outside 1..65535", p->g);
    if (p->n < 0 || p->n > (1LL << 36)) return fail("RnfGridLocate.n=%lld outside 0..2^36", (long long)p->n);
    if (!p->rows_out && !p->counts) return fail("RnfGridLocate: null rows_out and counts (at least one output)");
    if (p->counts && (72LL << (3 * p->level)) > gl::MAX_Q)
        return fail("RnfGridLocate.counts: Q=%lld rows of level %d exceed 2^26", 72LL << (3 * p->level), p->level);
    if (p->n == 0) return 0;
    if (!p->rotations) return fail("RnfGridLocate: null rotations");
    const long long total = (long long)p->g * p->n;
    long long blocks = (total + gl::THREADS - 1) / gl::THREADS;
    if (blocks > (1LL << 20)) blocks = 1LL << 20;
    hipLaunchKernelGGL(gl::so3_grid_locate_kernel, dim3((unsigned)blocks), dim3(gl::THREADS), 0, reinterpret_cast<hipStream_t>(p->stream),
                       (int)p->level, (long long)p->n, total, p->rotations, p->offset, (long long *)p->rows_out, (int *)p->counts);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The fit of a histogram against a grid density (csrc/grid_locate.h): the row maximum by grid_modes.h's arg-max pass, one pass, its finalise.
static int grid_fit_check(const RnfGridFit *p) {
    if (check_struct(p, "RnfGridFit")) return 1;
    if (p->g < 1 || p->g > 65535) return fail("RnfGridFit.g=%d outside 1..65535", p->g);
    if (p->Q < 1 || p->Q > gl::MAX_Q) return fail("RnfGridFit.Q=%lld outside 1..2^26", (long long)p->Q);
    return 0;
}

extern "C" size_t rnf_grid_fit_workspace_bytes(const RnfGridFit *p) {
    if (grid_fit_check(p)) return 0;
    return gl::carve(nullptr, p->Q, p->g).bytes;
}

extern "C" int rnf_grid_fit(const RnfGridFit *p) {
    if (grid_fit_check(p)) return 1;
    if (!p->logp || !p->counts || !p->stats_out) return fail("RnfGridFit: null logp, counts or stats_out");
    const size_t need = rnf_grid_fit_workspace_bytes(p);
    if (check_workspace(p, "RnfGridFit", need, "rnf_grid_fit_workspace_bytes", 8)) return 1;
    static_assert(gl::N_STATS == RNF_GRID_FIT_STATS, "csrc/grid_locate.h and include/rnf_hip.h disagree on the statistics");
    const gl::Workspace w = gl::carve(p->workspace, p->Q, p->g);
    const long long Q = p->Q;
    const int nb = (int)gl::blocks_for(Q);
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    if (launch_row_max(p->logp, Q, p->g, w.max_part, w.max_index, w.max_value, s)) return 1;
    hipLaunchKernelGGL(gl::grid_fit_kernel, dim3(nb, p->g), dim3(gl::THREADS), 0, s, p->logp, (const int *)p->counts, Q,
                       (const float *)w.max_value, w.part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gl::grid_fit_final_kernel, dim3(p->g), dim3(gl::THREADS), 0, s, (const gl::FitPart *)w.part, nb, Q,
                       (const float *)w.max_value, p->stats_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The chart of a grid cell (csrc/grid_sample.h): one thread per point.
extern "C" int rnf_so3_grid_cell_points(const RnfGridCellPoints *p) {
    if (check_struct(p, "RnfGridCellPoints")) return 1;
    if (p->level < 0 || p->level > gsa::MAX_LEVEL) return fail("RnfGridCellPoints.level=%d outside 0..%d", p->level, gsa::MAX_LEVEL);
    if (p->n < 0 || p->n > (1LL << 36)) return fail("RnfGridCellPoints.n=%lld outside 0..2^36", (long long)p->n);
    if (p->n == 0) return 0;
    if (!p->rows || !p->u || !p->rot_out) return fail("RnfGridCellPoints: null rows, u or rot_out");
    long long blocks = (p->n + gsa::THREADS - 1) / gsa::THREADS;
    if (blocks > (1LL << 20)) blocks = 1LL << 20;
    hipLaunchKernelGGL(gsa::so3_grid_cell_points_kernel, dim3((unsigned)blocks), dim3(gsa::THREADS), 0, reinterpret_cast<hipStream_t>(p->stream),
                       (int)p->level, (long long)p->n, (const long long *)p->rows, p->u, p->offset, p->rot_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Draws from grid posteriors (csrc/grid_sample.h): the row maximum by grid_modes.h's arg-max pass, the chunk sums, their scan, the draws.
static int grid_sample_check(const RnfGridSample *p) {
    if (check_struct(p, "RnfGridSample")) return 1;
    if (p->g < 1 || p->g > 65535) return fail("RnfGridSample.g=%d outside 1..65535", p->g);
    if (p->Q < 1 || p->Q > gsa::MAX_Q) return fail("RnfGridSample.Q=%lld outside 1..2^26", (long long)p->Q);
    return 0;
}

extern "C" size_t rnf_grid_sample_workspace_bytes(const RnfGridSample *p) {
    if (grid_sample_check(p)) return 0;
    return gsa::carve(nullptr, p->Q, p->g, gm::blocks_for(p->Q)).bytes;
}

extern "C" int rnf_grid_sample(const RnfGridSample *p) {
    if (grid_sample_check(p)) return 1;
    static_assert(sizeof(gm::ArgPart) == 16, "csrc/grid_sample.h carves 16 bytes per arg-max partial");
    static_assert(gsa::MULTINOMIAL == RNF_GRID_SAMPLE_MULTINOMIAL && gsa::SYSTEMATIC == RNF_GRID_SAMPLE_SYSTEMATIC,
                  "csrc/grid_sample.h and include/rnf_hip.h disagree on the methods");
    if (p->level < -1 || p->level > gsa::MAX_LEVEL) return fail("RnfGridSample.level=%d outside -1..%d", p->level, gsa::MAX_LEVEL);
    if (p->level >= 0 && p->Q != (72LL << (3 * p->level)))
        return fail("RnfGridSample.Q=%lld is not the %lld rows of level %d", (long long)p->Q, 72LL << (3 * p->level), p->level);
    if (p->rot_out && p->level < 0) return fail("RnfGridSample.rot_out needs a grid level (level=-1 draws rows only)");
    if (p->method != RNF_GRID_SAMPLE_MULTINOMIAL && p->method != RNF_GRID_SAMPLE_SYSTEMATIC)
        return fail("RnfGridSample.method=%d is neither RNF_GRID_SAMPLE_MULTINOMIAL nor RNF_GRID_SAMPLE_SYSTEMATIC", p->method);
    if (p->draws_total < 1 || p->draws_total > gsa::MAX_DRAWS)
        return fail("RnfGridSample.draws_total=%lld outside 1..2^30", (long long)p->draws_total);
    if (p->draws < 0 || p->draw_base < 0 || p->draws > p->draws_total || p->draw_base > p->draws_total - p->draws)
        return fail("RnfGridSample: draws %lld..%lld outside the draws_total=%lld", (long long)p->draw_base,
                    (long long)p->draw_base + (long long)p->draws, (long long)p->draws_total);
    if (p->image_base < 0 || p->image_base > (1LL << 62)) return fail("RnfGridSample.image_base=%lld outside 0..2^62", (long long)p->image_base);
    if (!p->logp) return fail("RnfGridSample: null logp");
    if (p->draws > 0 && !p->index_out) return fail("RnfGridSample: null index_out");
    const size_t need = rnf_grid_sample_workspace_bytes(p);
    if (check_workspace(p, "RnfGridSample", need, "rnf_grid_sample_workspace_bytes", 8)) return 1;
    const long long Q = p->Q, nc = gsa::chunks_for(Q);
    const int nbm = (int)gm::blocks_for(Q), nbs = (int)gsa::sum_blocks_for(Q);
    const gsa::Workspace w = gsa::carve(p->workspace, Q, p->g, nbm);
    const double scale = ldexp(1.0, gc::fixed_point_shift(Q));
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    if (launch_row_max(p->logp, Q, p->g, (gm::ArgPart *)w.max_part, w.max_index, w.max_value, s)) return 1;
    hipLaunchKernelGGL(gsa::grid_sample_sum_kernel, dim3(nbs, p->g), dim3(gsa::THREADS), 0, s, p->logp, Q, nc, scale, (const float *)w.max_value,
                       w.prefix);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gsa::grid_sample_scan_kernel, dim3(p->g), dim3(gsa::SCAN_THREADS), 0, s, nc, (const float *)w.max_value, w.prefix, w.total);
    HIP_TRY(hipGetLastError());
    if (p->draws == 0 && !p->total_out) return 0;
    long long blocks = (p->draws + gsa::THREADS - 1) / gsa::THREADS;
    blocks = blocks < 1 ? 1 : blocks > (1LL << 22) ? (1LL << 22) : blocks;
    hipLaunchKernelGGL(gsa::grid_sample_draw_kernel, dim3((unsigned)blocks, p->g), dim3(gsa::THREADS), 0, s, p->logp, Q, nc, scale, (int)p->level,
                       (long long)p->draws, (long long)p->draw_base, (long long)p->draws_total, (long long)p->image_base, (int)p->method,
                       (int)(p->jitter != 0), (gsa::u64)p->seed, p->offset, (const float *)w.max_value, (const gsa::u64 *)w.prefix,
                       (const gsa::u64 *)w.total, (long long *)p->index_out, (gsa::u64 *)p->target_out, (gsa::u64 *)p->total_out, p->rot_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// log Z of G rows of log-weights over n centres -> log_z[G]: so3_kernel_sum.h's weights pass and its finalise.  The prologue of the kernel
// sums, the kernel moments, the two angle distributions and the Fourier coefficients.
static int launch_log_z(const float *centres, const float *log_weights, int n, int G, ks::WeightPart *wpart, double *log_z, hipStream_t s) {
    const int nchunk = (int)ks::chunks_for(n);
    hipLaunchKernelGGL(ks::so3_kernel_weights_kernel, dim3(nchunk, G), dim3(ks::THREADS), 0, s, centres, log_weights, n, wpart);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ks::so3_kernel_weights_final_kernel, dim3(G), dim3(64), 0, s, (const ks::WeightPart *)wpart, nchunk, log_z);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Pairwise matrix-Fisher kernel sums (csrc/so3_kernel_sum.h): the weights pass and its finalise, the pairwise pass, its finalise.
static int so3_kernel_sum_check(const RnfSo3KernelSum *p) {
    if (check_struct(p, "RnfSo3KernelSum")) return 1;
    if (p->J < 1 || p->J > ks::MAX_J) return fail("RnfSo3KernelSum.J=%d outside 1..%d", p->J, ks::MAX_J);
    if (p->G < 1 || p->G > ks::MAX_G) return fail("RnfSo3KernelSum.G=%d outside 1..65535", p->G);
    if (p->n < 1 || p->n > ks::MAX_N) return fail("RnfSo3KernelSum.n=%lld outside 1..2^24", (long long)p->n);
    if (p->m < 0 || p->m > ks::MAX_M) return fail("RnfSo3KernelSum.m=%lld outside 0..2^31-1", (long long)p->m);
    if (ks::carve(nullptr, p->n, p->m, p->G, p->J).bytes == 0)
        return fail("RnfSo3KernelSum: the workspace of G=%d, J=%d, n=%lld, m=%lld does not fit; tile the queries", p->G, p->J, (long long)p->n,
                    (long long)p->m);
    return 0;
}

extern "C" size_t rnf_so3_kernel_sum_workspace_bytes(const RnfSo3KernelSum *p) {
    if (so3_kernel_sum_check(p)) return 0;
    return ks::carve(nullptr, p->n, p->m, p->G, p->J).bytes;
}

template <int J, int GB, bool LOO>
static void so3_kernel_sum_launch(const RnfSo3KernelSum *p, const float *Q, const ks::Scales &sc, const ks::Workspace &w, hipStream_t s) {
    const dim3 grid((unsigned)((p->m + ks::THREADS - 1) / ks::THREADS), (unsigned)ks::chunks_for(p->n), (unsigned)((p->G + GB - 1) / GB));
    hipLaunchKernelGGL((ks::so3_kernel_sum_kernel<J, GB, LOO>), grid, dim3(ks::THREADS), 0, s, p->centres, Q, p->log_weights, (int)p->n, (int)p->m,
                       (int)p->G, sc, w.pmax, w.psum);
}

extern "C" int rnf_so3_kernel_sum(const RnfSo3KernelSum *p) {
    if (so3_kernel_sum_check(p)) return 1;
    if (!p->kappas) return fail("RnfSo3KernelSum: null kappas");
    for (int a = 0; a < p->J; ++a)
        if (!(p->kappas[a] >= 0.0 && p->kappas[a] <= ks::MAX_KAPPA))
            return fail("RnfSo3KernelSum.kappas[%d]=%g outside 0..1e6", a, p->kappas[a]);
    if (check_aligned16(p->centres, p->queries, "RnfSo3KernelSum", ": centres and queries")) return 1;
    const bool loo = p->leave_one_out != 0;
    if (loo && (p->m != p->n || (p->queries && p->queries != p->centres)))
        return fail("RnfSo3KernelSum.leave_one_out: the queries must be the centres (queries NULL or == centres, m == n)");
    if (!p->queries && p->m != p->n) return fail("RnfSo3KernelSum: null queries stand for the centres, but m=%lld and n=%lld", (long long)p->m, (long long)p->n);
    if (p->m == 0) return 0;
    if (!p->centres || !p->out) return fail("RnfSo3KernelSum: null centres or out");
    const size_t need = ks::carve(nullptr, p->n, p->m, p->G, p->J).bytes;
    if (check_workspace(p, "RnfSo3KernelSum", need, "rnf_so3_kernel_sum_workspace_bytes", 8)) return 1;
    const ks::Workspace w = ks::carve(p->workspace, p->n, p->m, p->G, p->J);
    ks::Scales sc;
    ks::Normalisers nm;
    ks::scales_of(p->kappas, p->J, sc, nm);
    const float *Q = p->queries ? p->queries : p->centres;
    const int nchunk = (int)ks::chunks_for(p->n);
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    if (launch_log_z(p->centres, p->log_weights, (int)p->n, p->G, w.wpart, w.log_z, s)) return 1;
#define RNF_KS_CASE(J)                                                                 \
    case J:                                                                            \
        if (loo) so3_kernel_sum_launch<J, 1, true>(p, Q, sc, w, s);                    \
        else so3_kernel_sum_launch<J, 1, false>(p, Q, sc, w, s);                       \
        break;
    if (p->J == 1 && !loo && p->G > 1) {           // several groups share one d2
        so3_kernel_sum_launch<1, ks::GROUPS_PER_THREAD, false>(p, Q, sc, w, s);
    } else {
        switch (p->J) {
            RNF_KS_CASE(1) RNF_KS_CASE(2) RNF_KS_CASE(3) RNF_KS_CASE(4) RNF_KS_CASE(5) RNF_KS_CASE(6) RNF_KS_CASE(7) RNF_KS_CASE(8)
        }
    }
#undef RNF_KS_CASE
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ks::so3_kernel_sum_final_kernel, dim3((unsigned)((p->m + ks::THREADS - 1) / ks::THREADS), p->J, p->G), dim3(ks::THREADS), 0, s,
                       (const float *)w.pmax, (const double *)w.psum, (const double *)w.log_z, p->log_weights, (int)p->n, (int)p->m, nchunk, nm,
                       (int)loo, p->out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Moments of the same kernel sum (csrc/so3_kernel_moments.h): the weights pass and its finalise, the chunk flags, the pairwise pass, its
// finalise.
static int so3_kernel_moments_check(const RnfSo3KernelMoments *p) {
    if (check_struct(p, "RnfSo3KernelMoments")) return 1;
    if (p->G < 1 || p->G > ks::MAX_G) return fail("RnfSo3KernelMoments.G=%d outside 1..65535", p->G);
    if (p->n < 1 || p->n > ks::MAX_N) return fail("RnfSo3KernelMoments.n=%lld outside 1..2^24", (long long)p->n);
    if (p->m < 0 || p->m > ks::MAX_M) return fail("RnfSo3KernelMoments.m=%lld outside 0..2^31-1", (long long)p->m);
    if (km::carve(nullptr, p->n, p->m, p->G).bytes == 0)
        return fail("RnfSo3KernelMoments: the workspace of G=%d, n=%lld, m=%lld does not fit; tile the queries", p->G, (long long)p->n,
                    (long long)p->m);
    return 0;
}

extern "C" size_t rnf_so3_kernel_moments_workspace_bytes(const RnfSo3KernelMoments *p) {
    if (so3_kernel_moments_check(p)) return 0;
    return km::carve(nullptr, p->n, p->m, p->G).bytes;
}

extern "C" int rnf_so3_kernel_moments(const RnfSo3KernelMoments *p) {
    if (so3_kernel_moments_check(p)) return 1;
    if (!(p->kappa >= 0.0 && p->kappa <= ks::MAX_KAPPA)) return fail("RnfSo3KernelMoments.kappa=%g outside 0..1e6", p->kappa);
    if (check_aligned16(p->centres, p->queries, "RnfSo3KernelMoments", ": centres and queries")) return 1;
    if (p->step && !p->rotation) return fail("RnfSo3KernelMoments.step requires rotation");
    if (p->dlog_normaliser) *p->dlog_normaliser = km::dlog_normaliser(p->kappa);
    if (p->m == 0) return 0;
    if (!p->centres || !p->queries) return fail("RnfSo3KernelMoments: null centres or queries");
    const size_t need = km::carve(nullptr, p->n, p->m, p->G).bytes;
    if (check_workspace(p, "RnfSo3KernelMoments", need, "rnf_so3_kernel_moments_workspace_bytes", 8)) return 1;
    const km::Workspace w = km::carve(p->workspace, p->n, p->m, p->G);
    ks::Scales sc;
    ks::Normalisers nm;
    ks::scales_of(&p->kappa, 1, sc, nm);
    const int nchunk = (int)ks::chunks_for(p->n);
    const unsigned blocks = (unsigned)((p->m + ks::THREADS - 1) / ks::THREADS);
    const long long q_group = p->group_queries ? 9 * (long long)p->m : 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    if (launch_log_z(p->centres, p->log_weights, (int)p->n, p->G, w.wpart, w.log_z, s)) return 1;
    hipLaunchKernelGGL(km::so3_kernel_moments_flags_kernel, dim3(nchunk), dim3(ks::THREADS), 0, s, p->centres, (int)p->n, w.flags);
    HIP_TRY(hipGetLastError());
    const int block = km::block_for(p->m, nchunk, p->G);
    hipLaunchKernelGGL(km::so3_kernel_moments_kernel, dim3((unsigned)((p->m + block - 1) / block), nchunk, p->G), dim3(block), 0, s, p->centres,
                       p->queries, p->log_weights,
                       (int)p->n, (int)p->m, q_group, sc, (const int *)w.flags, w.pmax, w.psum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(km::so3_kernel_moments_final_kernel, dim3(blocks, p->G), dim3(ks::THREADS), 0, s, (const float *)w.pmax,
                       (const double *)w.psum, (const double *)w.log_z, p->queries, q_group, (int)p->m, nchunk, nm.l[0], p->log_density, p->mean,
                       p->msd, p->rotation, p->step);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The distribution function of the geodesic angle to a query (csrc/so3_angle_cdf.h) and to the nearest member of a set
// (csrc/so3_set_angle_cdf.h): one computation, a query being a set of one member.  launch_log_z, the normalised weights, the pairwise
// pass of the entry (so3_angle_cdf_launch), the finalise for sets of K.  What differs between the two structs is here:
template <class P>
struct So3AngleCdfEntry;
template <>
struct So3AngleCdfEntry<RnfSo3AngleCdf> {
    static constexpr bool sets = false;
    static constexpr const char *who = "RnfSo3AngleCdf", *noun = "queries", *workspace_fn = "rnf_so3_angle_cdf_workspace_bytes";
    static int K(const RnfSo3AngleCdf *) { return 1; }
};
template <>
struct So3AngleCdfEntry<RnfSo3SetAngleCdf> {
    static constexpr bool sets = true;
    static constexpr const char *who = "RnfSo3SetAngleCdf", *noun = "sets", *workspace_fn = "rnf_so3_set_angle_cdf_workspace_bytes";
    static int K(const RnfSo3SetAngleCdf *p) { return p->K; }
};

template <class P>
static int so3_angle_cdf_slots(const P *p) { return (p->mass ? p->T : 0) + (p->mean_angle || p->mean_sq_angle ? 2 : 0); }

template <class P>
static int so3_angle_cdf_check(const P *p) {
    using E = So3AngleCdfEntry<P>;
    if (check_struct(p, E::who)) return 1;
    if (p->T < 0 || p->T > ac::MAX_T) return fail("%s.T=%d outside 0..%d", E::who, p->T, ac::MAX_T);
    if (p->G < 1 || p->G > ks::MAX_G) return fail("%s.G=%d outside 1..65535", E::who, p->G);
    if (E::sets && (E::K(p) < 1 || E::K(p) > sac::MAX_K)) return fail("%s.K=%d outside 1..%d", E::who, E::K(p), sac::MAX_K);
    if (p->n < 1 || p->n > ks::MAX_N) return fail("%s.n=%lld outside 1..2^24", E::who, (long long)p->n);
    if (p->m < 0 || p->m > ks::MAX_M) return fail("%s.m=%lld outside 0..2^31-1", E::who, (long long)p->m);
    if (ac::carve(nullptr, p->n, p->m, p->G, so3_angle_cdf_slots(p)).bytes == 0)
        return fail("%s: the workspace of G=%d, T=%d, n=%lld, m=%lld does not fit; tile the %s", E::who, p->G, p->T, (long long)p->n,
                    (long long)p->m, E::noun);
    return 0;
}

template <class P>
static size_t so3_angle_cdf_workspace_bytes(const P *p) {
    if (so3_angle_cdf_check(p)) return 0;
    return ac::carve(nullptr, p->n, p->m, p->G, so3_angle_cdf_slots(p)).bytes;
}

template <int TT, bool MOM>
static void so3_angle_cdf_launch(const RnfSo3AngleCdf *p, int T, const ac::Taus &taus, const ac::Workspace &w, hipStream_t s) {
    const int nchunk = (int)ks::chunks_for(p->n);
    const long long q_group = p->group_queries ? 9 * (long long)p->m : 0;
    const bool perq = T > 0 && p->query_tau;
    const int gb = !perq && !p->group_queries && p->G > 1 ? ac::GROUPS_PER_THREAD : 1;      // shared queries and thresholds: groups share d2
    const unsigned zblocks = (unsigned)((p->G + gb - 1) / gb);
    const int block = ac::block_for(p->m, nchunk, zblocks);
    const dim3 grid((unsigned)((p->m + block - 1) / block), nchunk, zblocks);
#define RNF_AC_LAUNCH(GB, PERQ)                                                                                                              \
    hipLaunchKernelGGL((ac::so3_angle_cdf_kernel<TT, MOM, GB, PERQ>), grid, dim3(block), 0, s, p->centres, p->queries, (const float *)w.wn, \
                       (int)p->n, (int)p->m, (int)p->G, q_group, taus, p->query_tau, T, w.psum)
    if (perq) RNF_AC_LAUNCH(1, true);
    else if (gb > 1) RNF_AC_LAUNCH(ac::GROUPS_PER_THREAD, false);
    else RNF_AC_LAUNCH(1, false);
#undef RNF_AC_LAUNCH
}

template <int TT, bool MOM>
static void so3_angle_cdf_launch(const RnfSo3SetAngleCdf *p, int T, const ac::Taus &taus, const ac::Workspace &w, hipStream_t s) {
    constexpr int GBS = sac::groups_for(TT + (MOM ? 2 : 0));
    const int nchunk = (int)ks::chunks_for(p->n);
    const long long q_group = p->group_queries ? 9 * (long long)p->m * p->K : 0;
    const bool perq = T > 0 && p->query_tau;
    if (sac::wave_per_set(p->m, nchunk, p->G, p->K)) {                                       // few sets: a wave per (group, set, chunk)
        const dim3 waves((unsigned)p->m, nchunk, p->G);
        if (perq)
            hipLaunchKernelGGL((sac::so3_set_angle_cdf_wave_kernel<TT, MOM, true>), waves, dim3(64), 0, s, p->centres, p->queries, (const float *)w.wn,
                               (int)p->n, (int)p->m, (int)p->K, q_group, taus, p->query_tau, T, w.psum);
        else
            hipLaunchKernelGGL((sac::so3_set_angle_cdf_wave_kernel<TT, MOM, false>), waves, dim3(64), 0, s, p->centres, p->queries, (const float *)w.wn,
                               (int)p->n, (int)p->m, (int)p->K, q_group, taus, p->query_tau, T, w.psum);
        return;
    }
    const int gb = !perq && !p->group_queries && p->G > 1 ? GBS : 1;                        // shared sets and thresholds: groups share the minima
    const unsigned zblocks = (unsigned)((p->G + gb - 1) / gb);
    const int block = ac::block_for(p->m, nchunk, zblocks);
    const dim3 grid((unsigned)((p->m + block - 1) / block), nchunk, zblocks);
#define RNF_SAC_LAUNCH(GB, PERQ)                                                                                                                 \
    hipLaunchKernelGGL((sac::so3_set_angle_cdf_kernel<TT, MOM, GB, PERQ>), grid, dim3(block), 0, s, p->centres, p->queries, (const float *)w.wn, \
                       (int)p->n, (int)p->m, (int)p->K, (int)p->G, q_group, taus, p->query_tau, T, w.psum)
    if (perq) RNF_SAC_LAUNCH(1, true);
    else if (gb > 1) RNF_SAC_LAUNCH(GBS, false);
    else RNF_SAC_LAUNCH(1, false);
#undef RNF_SAC_LAUNCH
}

template <class P>
static int so3_angle_cdf_run(const P *p) {
    using E = So3AngleCdfEntry<P>;
    if (so3_angle_cdf_check(p)) return 1;
    if (check_aligned16(p->centres, p->queries, E::who, ": centres and queries")) return 1;
    const bool mom = p->mean_angle || p->mean_sq_angle;
    if (p->T == 0 && !mom) return fail("%s.T=0 requires mean_angle or mean_sq_angle", E::who);
    if (p->T == 0 && (p->thresholds || p->query_tau)) return fail("%s.T=0 with thresholds or query_tau", E::who);
    if (p->T > 0 && p->thresholds && p->query_tau) return fail("%s: both thresholds and query_tau are given; exactly one of the two", E::who);
    if (p->T > 0 && !p->thresholds && !p->query_tau) return fail("%s: neither thresholds nor query_tau is given for T=%d", E::who, p->T);
    ac::Taus taus;
    for (int t = 0; t < ac::MAX_T; ++t) taus.t[t] = -1.f;
    if (p->T > 0 && p->thresholds)
        for (int t = 0; t < p->T; ++t) {
            if (!(p->thresholds[t] >= 0.0 && p->thresholds[t] <= ac::PI))
                return fail("%s.thresholds[%d]=%g outside 0..pi", E::who, t, p->thresholds[t]);
            taus.t[t] = ac::tau_of(p->thresholds[t]);
        }
    if (p->m == 0) return 0;
    if (!p->centres || !p->queries) return fail("%s: null centres or queries", E::who);
    const int T = p->mass ? p->T : 0;              // masses nobody takes are not computed
    if (T == 0 && !mom) return 0;
    const size_t need = ac::carve(nullptr, p->n, p->m, p->G, so3_angle_cdf_slots(p)).bytes;
    if (check_workspace(p, E::who, need, E::workspace_fn, 8)) return 1;
    const ac::Workspace w = ac::carve(p->workspace, p->n, p->m, p->G, so3_angle_cdf_slots(p));
    const int nchunk = (int)ks::chunks_for(p->n), K = E::K(p);
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    if (launch_log_z(p->centres, p->log_weights, (int)p->n, p->G, w.wpart, w.log_z, s)) return 1;
    hipLaunchKernelGGL(ac::so3_angle_cdf_weights_kernel, dim3((unsigned)((p->n + ks::THREADS - 1) / ks::THREADS), p->G), dim3(ks::THREADS), 0, s,
                       p->log_weights, (const double *)w.log_z, (int)p->n, w.wn);
    HIP_TRY(hipGetLastError());
#define RNF_AC_CASE(TT)                                                    \
    case TT:                                                               \
        if (mom) so3_angle_cdf_launch<TT, true>(p, T, taus, w, s);         \
        else so3_angle_cdf_launch<TT, false>(p, T, taus, w, s);            \
        break;
    switch (ac::slots_for(T)) {
        case 0: so3_angle_cdf_launch<0, true>(p, T, taus, w, s); break;
        RNF_AC_CASE(1) RNF_AC_CASE(2) RNF_AC_CASE(4) RNF_AC_CASE(8)
    }
#undef RNF_AC_CASE
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sac::so3_set_angle_cdf_final_kernel, dim3((unsigned)((p->m + ks::THREADS - 1) / ks::THREADS), p->G), dim3(ks::THREADS), 0, s,
                       (const double *)w.psum, p->queries, p->group_queries ? 9 * (long long)p->m * K : 0LL, (int)p->m, K, nchunk, T, (int)mom, taus,
                       T > 0 ? p->query_tau : (const float *)nullptr, p->mass, p->mean_angle, p->mean_sq_angle);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" size_t rnf_so3_angle_cdf_workspace_bytes(const RnfSo3AngleCdf *p) { return so3_angle_cdf_workspace_bytes(p); }
extern "C" int rnf_so3_angle_cdf(const RnfSo3AngleCdf *p) { return so3_angle_cdf_run(p); }
extern "C" size_t rnf_so3_set_angle_cdf_workspace_bytes(const RnfSo3SetAngleCdf *p) { return so3_angle_cdf_workspace_bytes(p); }
extern "C" int rnf_so3_set_angle_cdf(const RnfSo3SetAngleCdf *p) { return so3_angle_cdf_run(p); }

// Harmonic analysis on SO(3) (csrc/so3_harmonics.h).  Every entry first writes the entry records into its workspace.
static int so3_harmonics_records(int L, float *records, hipStream_t s) {
    hipLaunchKernelGGL(sh::so3_harmonics_records_kernel, dim3((unsigned)((sh::entry_count(L) + sh::THREADS - 1) / sh::THREADS)), dim3(sh::THREADS), 0,
                       s, L, records);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int so3_wigner_check(const RnfSo3Wigner *p) {
    if (check_struct(p, "RnfSo3Wigner")) return 1;
    if (p->lmax < 0 || p->lmax > sh::MAX_DEGREE) return fail("RnfSo3Wigner.lmax=%d outside 0..%d", p->lmax, sh::MAX_DEGREE);
    if (p->n < 0 || p->n > sh::MAX_N) return fail("RnfSo3Wigner.n=%lld outside 0..2^24", (long long)p->n);
    return 0;
}

extern "C" size_t rnf_so3_wigner_workspace_bytes(const RnfSo3Wigner *p) { return so3_wigner_check(p) ? 0 : sh::records_bytes(p->lmax); }

extern "C" int rnf_so3_wigner(const RnfSo3Wigner *p) {
    if (so3_wigner_check(p)) return 1;
    if (p->n == 0) return 0;
    if (!p->rotations || !p->out) return fail("RnfSo3Wigner: null rotations or out");
    const size_t need = sh::records_bytes(p->lmax);
    if (check_workspace(p, "RnfSo3Wigner", need, "rnf_so3_wigner_workspace_bytes", 16)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    float *records = static_cast<float *>(p->workspace);
    if (so3_harmonics_records(p->lmax, records, s)) return 1;
    hipLaunchKernelGGL(sh::so3_wigner_kernel, dim3((unsigned)((p->n + sh::THREADS - 1) / sh::THREADS)), dim3(sh::THREADS), 0, s, p->rotations,
                       (long long)p->n, (int)p->lmax, (const float *)records, p->out);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int so3_fourier_check(const RnfSo3Fourier *p) {
    if (check_struct(p, "RnfSo3Fourier")) return 1;
    if (p->lmax < 0 || p->lmax > sh::MAX_DEGREE) return fail("RnfSo3Fourier.lmax=%d outside 0..%d", p->lmax, sh::MAX_DEGREE);
    if (p->G < 1 || p->G > ks::MAX_G) return fail("RnfSo3Fourier.G=%d outside 1..65535", p->G);
    if (p->n < 1 || p->n > sh::MAX_N) return fail("RnfSo3Fourier.n=%lld outside 1..2^24", (long long)p->n);
    return 0;
}

extern "C" size_t rnf_so3_fourier_workspace_bytes(const RnfSo3Fourier *p) {
    return so3_fourier_check(p) ? 0 : sh::carve(nullptr, p->n, p->G, p->lmax).bytes;
}

extern "C" int rnf_so3_fourier(const RnfSo3Fourier *p) {
    if (so3_fourier_check(p)) return 1;
    if (!p->centres || !p->out) return fail("RnfSo3Fourier: null centres or out");
    const size_t need = sh::carve(nullptr, p->n, p->G, p->lmax).bytes;
    if (check_workspace(p, "RnfSo3Fourier", need, "rnf_so3_fourier_workspace_bytes", 16)) return 1;
    const sh::Workspace w = sh::carve(p->workspace, p->n, p->G, p->lmax);
    const int nchunk = (int)ks::chunks_for(p->n), L = p->lmax, n = (int)p->n, G = p->G, CL = sh::coefficient_count(L);
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    if (so3_harmonics_records(L, w.records, s)) return 1;
    if (launch_log_z(p->centres, p->log_weights, n, G, w.wpart, w.log_z, s)) return 1;
    hipLaunchKernelGGL(ac::so3_angle_cdf_weights_kernel, dim3((unsigned)((n + ks::THREADS - 1) / ks::THREADS), G), dim3(ks::THREADS), 0, s,
                       p->log_weights, (const double *)w.log_z, n, w.wn);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sh::so3_fourier_table_kernel, dim3((unsigned)((n + sh::THREADS - 1) / sh::THREADS)), dim3(sh::THREADS), 0, s, p->centres, n, L,
                       w.tab);
    HIP_TRY(hipGetLastError());
    const int gb = sh::groups_per_thread(L);
    const dim3 grid((unsigned)((sh::entry_count(L) + sh::THREADS - 1) / sh::THREADS), nchunk, (unsigned)((G + gb - 1) / gb));
    if (L <= 8)
        hipLaunchKernelGGL((sh::so3_fourier_kernel<8, 4>), grid, dim3(sh::THREADS), 0, s, (const float *)w.tab, (const float *)w.wn,
                           (const float *)w.records, n, L, G, w.psum);
    else
        hipLaunchKernelGGL((sh::so3_fourier_kernel<16, 2>), grid, dim3(sh::THREADS), 0, s, (const float *)w.tab, (const float *)w.wn,
                           (const float *)w.records, n, L, G, w.psum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sh::so3_fourier_final_kernel, dim3((unsigned)((CL + sh::THREADS - 1) / sh::THREADS), G), dim3(sh::THREADS), 0, s,
                       (const double *)w.psum, nchunk, CL, p->out);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int so3_fourier_eval_check(const RnfSo3FourierEval *p) {
    if (check_struct(p, "RnfSo3FourierEval")) return 1;
    if (p->lmax < 0 || p->lmax > sh::MAX_DEGREE) return fail("RnfSo3FourierEval.lmax=%d outside 0..%d", p->lmax, sh::MAX_DEGREE);
    if (p->G < 1 || p->G > ks::MAX_G) return fail("RnfSo3FourierEval.G=%d outside 1..65535", p->G);
    if (p->m < 0 || p->m > sh::MAX_M) return fail("RnfSo3FourierEval.m=%lld outside 0..2^31-1", (long long)p->m);
    return 0;
}

extern "C" size_t rnf_so3_fourier_eval_workspace_bytes(const RnfSo3FourierEval *p) {
    return so3_fourier_eval_check(p) ? 0 : sh::records_bytes(p->lmax);
}

extern "C" int rnf_so3_fourier_eval(const RnfSo3FourierEval *p) {
    if (so3_fourier_eval_check(p)) return 1;
    if (p->m == 0) return 0;
    if (!p->coeffs || !p->queries || !p->out) return fail("RnfSo3FourierEval: null coeffs, queries or out");
    const size_t need = sh::records_bytes(p->lmax);
    if (check_workspace(p, "RnfSo3FourierEval", need, "rnf_so3_fourier_eval_workspace_bytes", 16)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    float *records = static_cast<float *>(p->workspace);
    if (so3_harmonics_records(p->lmax, records, s)) return 1;
    const int gb = !p->group_queries && p->G > 1 ? ks::GROUPS_PER_THREAD : 1;                // shared queries: the groups share the entries
    const unsigned yblocks = (unsigned)((p->G + gb - 1) / gb);
    const int block = (p->m + sh::THREADS - 1) / sh::THREADS * yblocks < ac::FEW_BLOCKS ? ac::SMALL_BLOCK : sh::THREADS;
    const dim3 grid((unsigned)((p->m + block - 1) / block), yblocks);
    const long long q_group = p->group_queries ? 9 * (long long)p->m : 0;
    if (gb > 1)
        hipLaunchKernelGGL((sh::so3_fourier_eval_kernel<ks::GROUPS_PER_THREAD>), grid, dim3(block), 0, s, p->queries, p->coeffs,
                           (const float *)records, (long long)p->m, (int)p->lmax, (int)p->G, q_group, p->out);
    else
        hipLaunchKernelGGL((sh::so3_fourier_eval_kernel<1>), grid, dim3(block), 0, s, p->queries, p->coeffs, (const float *)records, (long long)p->m,
                           (int)p->lmax, (int)p->G, q_group, p->out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Neighbour-limited kernel sums over the rows of the SO(3) grid (csrc/so3_grid_local.h): one launch, no workspace.
template <int GB, bool W>
static void so3_grid_local_launch(const RnfSo3GridLocalSum *p, const sgl::Geometry &ge, const float *Q, double l_kappa, hipStream_t s) {
    const dim3 grid((unsigned)((p->m + sgl::THREADS - 1) / sgl::THREADS), (unsigned)((p->G + GB - 1) / GB));
    hipLaunchKernelGGL((sgl::so3_grid_local_kernel<GB, W>), grid, dim3(sgl::THREADS), 0, s, ge, p->offset, p->grid, Q, p->log_weights,
                       sgl::rows_of(p->level), (int)p->m, (int)p->G, l_kappa, p->out, p->count);
}

// the refusals rnf_so3_grid_local_sum and rnf_so3_grid_local_max share; 1: refused, -1: nothing to do (m = 0), 0: go on
template <class P>
static int so3_grid_local_check(const P *p, const char *who, const void *arg, const char *arg_name) {
    if (p->level < 0 || p->level > sgl::MAX_LEVEL) return fail("%s.level=%d outside 0..%d", who, p->level, sgl::MAX_LEVEL);
    if (p->G < 1 || p->G > sgl::MAX_G) return fail("%s.G=%d outside 1..65535", who, p->G);
    if (p->m < 0 || p->m > sgl::MAX_M) return fail("%s.m=%lld outside 0..2^31-1", who, (long long)p->m);
    if constexpr (!std::is_same<P, RnfSo3GridLocalFisher>::value) {                          // the anisotropic entry checks its K itself
        if (!(p->kappa >= 0.0 && p->kappa <= ks::MAX_KAPPA)) return fail("%s.kappa=%g outside 0..1e6", who, p->kappa);
    }
    if (!(p->d2_cut >= 0.0 && p->d2_cut <= sgl::MAX_D2)) return fail("%s.d2_cut=%g outside 0..8", who, p->d2_cut);
    if (check_aligned16(p->grid, p->queries, who, ": grid and queries")) return 1;
    if (reinterpret_cast<uintptr_t>(p->offset) % 4 || reinterpret_cast<uintptr_t>(p->log_weights) % 4 || reinterpret_cast<uintptr_t>(p->out) % 4 ||
        reinterpret_cast<uintptr_t>(arg) % 4 || reinterpret_cast<uintptr_t>(p->count) % 4)
        return fail("%s: offset, log_weights, out%s and count must be 4-byte aligned", who, arg_name);
    const long long Q = sgl::rows_of(p->level);
    if (!p->queries && p->m != Q)
        return fail("%s: null queries stand for the grid rows, but m=%lld and level %d has %lld", who, (long long)p->m, p->level, Q);
    return p->m == 0 ? -1 : 0;
}

extern "C" int rnf_so3_grid_local_sum(const RnfSo3GridLocalSum *p) {
    if (check_struct(p, "RnfSo3GridLocalSum")) return 1;
    if (const int r = so3_grid_local_check(p, "RnfSo3GridLocalSum", nullptr, "")) return r > 0;
    if (!p->grid || !p->out) return fail("RnfSo3GridLocalSum: null grid or out");
    const sgl::Geometry ge = sgl::geometry_of(p->level, p->kappa, p->d2_cut);
    const double l_kappa = ks::log_normaliser(p->kappa);
    const float *queries = p->queries ? p->queries : p->grid;
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    if (!p->log_weights)
        so3_grid_local_launch<1, false>(p, ge, queries, l_kappa, s);
    else if (p->G == 1)
        so3_grid_local_launch<1, true>(p, ge, queries, l_kappa, s);
    else
        so3_grid_local_launch<sgl::GROUPS_PER_THREAD, true>(p, ge, queries, l_kappa, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The max-plus pass over the same neighbourhoods (csrc/so3_grid_local.h, SWEEP_ARGMAX): one launch of the sum's shape, no workspace.
template <int GB, bool W>
static void so3_grid_local_max_launch(const RnfSo3GridLocalMax *p, const sgl::Geometry &ge, const float *Q, double l_kappa, hipStream_t s) {
    const dim3 grid((unsigned)((p->m + sgl::THREADS - 1) / sgl::THREADS), (unsigned)((p->G + GB - 1) / GB));
    hipLaunchKernelGGL((sgl::so3_grid_local_max_kernel<GB, W>), grid, dim3(sgl::THREADS), 0, s, ge, p->offset, p->grid, Q, p->log_weights,
                       sgl::rows_of(p->level), (int)p->m, (int)p->G, l_kappa, p->out, p->arg, p->count);
}

extern "C" int rnf_so3_grid_local_max(const RnfSo3GridLocalMax *p) {
    if (check_struct(p, "RnfSo3GridLocalMax")) return 1;
    if (const int r = so3_grid_local_check(p, "RnfSo3GridLocalMax", p->arg, ", arg")) return r > 0;
    if (!p->grid || !p->out || !p->arg) return fail("RnfSo3GridLocalMax: null grid, out or arg");
    const sgl::Geometry ge = sgl::geometry_of(p->level, p->kappa, p->d2_cut);
    const double l_kappa = ks::log_normaliser(p->kappa);
    const float *queries = p->queries ? p->queries : p->grid;
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    if (!p->log_weights)
        so3_grid_local_max_launch<1, false>(p, ge, queries, l_kappa, s);
    else if (p->G == 1)
        so3_grid_local_max_launch<1, true>(p, ge, queries, l_kappa, s);
    else
        so3_grid_local_max_launch<sgl::GROUPS_PER_THREAD, true>(p, ge, queries, l_kappa, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The anisotropic term on the same two passes (csrc/so3_grid_local.h, F): arg selects the max-plus pass.  One launch, no workspace.
template <int GB, bool W, bool MAX>
static void so3_grid_local_fisher_launch(const RnfSo3GridLocalFisher *p, const sgl::Geometry &ge, const sgl::Quad &kq, const float *Q, double l_k,
                                         hipStream_t s) {
    const dim3 grid((unsigned)((p->m + sgl::THREADS - 1) / sgl::THREADS), (unsigned)((p->G + GB - 1) / GB));
    hipLaunchKernelGGL((sgl::so3_grid_local_fisher_kernel<GB, W, MAX>), grid, dim3(sgl::THREADS), 0, s, ge, kq, p->offset, p->grid, Q,
                       p->log_weights, sgl::rows_of(p->level), (int)p->m, (int)p->G, l_k, p->out, p->arg, p->count);
}

template <bool MAX>
static void so3_grid_local_fisher_pick(const RnfSo3GridLocalFisher *p, const sgl::Geometry &ge, const sgl::Quad &kq, const float *Q, double l_k,
                                       hipStream_t s) {
    if (!p->log_weights)
        so3_grid_local_fisher_launch<1, false, MAX>(p, ge, kq, Q, l_k, s);
    else if (p->G == 1)
        so3_grid_local_fisher_launch<1, true, MAX>(p, ge, kq, Q, l_k, s);
    else
        so3_grid_local_fisher_launch<sgl::GROUPS_PER_THREAD, true, MAX>(p, ge, kq, Q, l_k, s);
}

extern "C" int rnf_so3_grid_local_fisher(const RnfSo3GridLocalFisher *p) {
    const char *who = "RnfSo3GridLocalFisher";
    if (check_struct(p, who)) return 1;
    switch (sgl::concentration_defect(p->concentration)) {
        case 1: return fail("%s.concentration holds a non-finite entry", who);
        case 2: return fail("%s.concentration is not symmetric to 1e-9 of its norm", who);
        case 3: return fail("%s.concentration has two eigenvalues with a negative sum: not the symmetric factor of a proper SVD", who);
        case 4: return fail("%s.concentration has an eigenvalue beyond 3e4 in magnitude", who);
        default: break;
    }
    if (const int r = so3_grid_local_check(p, who, p->arg, ", arg")) return r > 0;
    if (!p->grid || !p->out) return fail("%s: null grid or out", who);
    const sgl::Geometry ge = sgl::geometry_of(p->level, 0.0, p->d2_cut);
    const sgl::Quad kq = sgl::quad_of(p->concentration);
    const double l_k = sgl::log_normaliser_fisher(p->concentration);
    const float *queries = p->queries ? p->queries : p->grid;
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    if (p->arg)
        so3_grid_local_fisher_pick<true>(p, ge, kq, queries, l_k, s);
    else
        so3_grid_local_fisher_pick<false>(p, ge, kq, queries, l_k, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// log-constants of MatrixFisherN(A, norm_type) (utils/fisher.py:67-76,79-97): c = s0 + s1 + s2 + log norm with the PROPER singular values
// of A (fisher_math.h).  One thread per matrix, fp64, so that a per-sample A coming out of a network never goes through a host SVD and a
// device->host sync.  scratch (doubles): [0] = Q = sum_b |A_b|_F^2 (norm_type 0 is batch-coupled through it), [1] = W, [2 + 10 b ..] =
// per-row gradient accumulators of the backward pass.
__global__ void fisher_frobenius_kernel(const float *A, long long B, double *q) {
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < B * 9; i += (long long)gridDim.x * blockDim.x) acc += (double)A[i] * (double)A[i];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(q, acc);
}

__global__ void fisher_log_const_kernel(const float *A, long long B, int norm_type, const double *q, float *c_out) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double a[9];
    for (int k = 0; k < 9; ++k) a[k] = A[b * 9 + k];
    c_out[b] = (float)fisher_log_const(a, norm_type, norm_type == 0 ? q[0] : 0.0, nullptr);
}

static int fisher_const_launch(const float *A, int64_t B, int32_t norm_type, double *scratch, float *c_out, hipStream_t st) {
    if (norm_type == 0) {
        HIP_TRY(hipMemsetAsync(scratch, 0, 2 * sizeof(double), st));
        long long blocks = (B * 9 + 255) / 256;
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(fisher_frobenius_kernel, dim3((int)blocks), dim3(256), 0, st, A, (long long)B, scratch);
    }
    if (c_out) hipLaunchKernelGGL(fisher_log_const_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, A, (long long)B, norm_type, scratch, c_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Proper SVD of every parameter matrix on the device (utils/fisher.py:53-76 proper_svd / proper_svd_N): U, V in SO(3) (vectors as columns,
// row-major), s with the smallest value signed by det A, and the Bingham parameters of the sampler lam = (0, 2(s1+s2), 2(s0+s2), 2(s0+s1))
// (utils/fisher.py:151-158).  fp64 Jacobi, one thread per matrix (fisher_math.h proper_svd3): MatrixFisherN._sample of a network-predicted
// A no longer goes through host LAPACK and a device->host copy per call.
__global__ void fisher_proper_svd_kernel(const float *A, long long B, float *U_out, float *V_out, float *s_out, float *lam_out) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double a[9], U[9], s[3], V[9];
    for (int k = 0; k < 9; ++k) a[k] = A[b * 9 + k];
    proper_svd3(a, U, s, V);
    for (int k = 0; k < 9; ++k) {
        if (U_out) U_out[b * 9 + k] = (float)U[k];
        if (V_out) V_out[b * 9 + k] = (float)V[k];
    }
    if (s_out) { s_out[b * 3] = (float)s[0]; s_out[b * 3 + 1] = (float)s[1]; s_out[b * 3 + 2] = (float)s[2]; }
    if (lam_out) {
        lam_out[b * 4] = 0.f;
        lam_out[b * 4 + 1] = (float)(2.0 * (s[1] + s[2]));
        lam_out[b * 4 + 2] = (float)(2.0 * (s[0] + s[2]));
        lam_out[b * 4 + 3] = (float)(2.0 * (s[0] + s[1]));
    }
}
extern "C" int rnf_fisher_proper_svd(const float *A, int64_t B, float *U_out, float *V_out, float *s_out, float *lam_out, void *stream) {
    if (B < 0) return fail("rnf_fisher_proper_svd: B=%lld", (long long)B);
    if (B == 0) return 0;
    if (!A) return fail("rnf_fisher_proper_svd: null pointer");
    hipLaunchKernelGGL(fisher_proper_svd_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), A, (long long)B,
                       U_out, V_out, s_out, lam_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int rnf_fisher_log_const(const float *A, int64_t B, float *c_out, void *stream) {
    if (!A || !c_out) return fail("rnf_fisher_log_const: null pointer");
    if (B <= 0) return fail("rnf_fisher_log_const: B=%lld", (long long)B);
    return fisher_const_launch(A, B, 1, nullptr, c_out, reinterpret_cast<hipStream_t>(stream));
}

// The exact log-normaliser (fisher_exact.h): c = sum s + log int f, its derivative dc/dA = E[R] and the entropy, by a fixed 224-node rule.
// ONE WAVE PER MATRIX, four matrices per workgroup: every lane of the wave runs the (wave-uniform) proper SVD of its matrix once, lane l
// sums nodes l, l + 64, .. (two scaled-Bessel pairs and one exp per node), and the xor butterfly leaves the five sums in every lane in one
// fixed order -- a row's result depends on nothing but the row: not on B, the row's position or the launch shape.  Lanes 0..8 write the
// entries of E[R]; with grad_acc (the fp64 sums T_b, G_b of fisher_grad_accum_kernel) they also finish d log p / dA = T - G dc/dA.
__global__ __launch_bounds__(256) void fisher_exact_kernel(const float *A, long long B, float *c_out, float *mean_out, float *entropy_out,
                                                           const double *grad_acc, float *g_A) {
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;                                                  // wave-uniform
    double a[9], U[9], s[3], V[9], acc[5], dc[9], m[3], c, h;
    for (int k = 0; k < 9; ++k) a[k] = A[b * 9 + k];
    proper_svd3(a, U, s, V);
    fisher_exact_lane(s, lane, acc);
#pragma unroll
    for (int k = 0; k < 5; ++k)
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    fisher_exact_finish(s, acc, c, m, h);
    fisher_exact_mean(U, m, V, dc);
    double mine = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) mine = lane == k ? dc[k] : mine;
    if (lane < 9) {
        if (mean_out) mean_out[b * 9 + lane] = (float)mine;
        if (g_A) g_A[b * 9 + lane] = (float)(grad_acc[10 * b + lane] - grad_acc[10 * b + 9] * mine);
    }
    if (lane == 0) {
        if (c_out) c_out[b] = (float)c;
        if (entropy_out) entropy_out[b] = (float)h;
    }
}

static int fisher_exact_launch(const char *who, const float *A, int64_t B, float *c_out, float *mean_out, float *entropy_out, const double *grad_acc,
                               float *g_A, hipStream_t st) {
    const long long blocks = ((long long)B + 3) / 4;
    if (blocks > 0x7fffffffLL) return fail("%s: B=%lld is more than one launch serves", who, (long long)B);
    hipLaunchKernelGGL(fisher_exact_kernel, dim3((unsigned)blocks), dim3(256), 0, st, A, (long long)B, c_out, mean_out, entropy_out, grad_acc, g_A);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int rnf_fisher_exact(const float *A, int64_t B, float *c_out, float *mean_out, void *stream) {
    if (B < 0) return fail("rnf_fisher_exact: B=%lld", (long long)B);
    if (!c_out && !mean_out) return fail("rnf_fisher_exact: c_out_dev and mean_out_dev are both null");
    if (B == 0) return 0;
    if (!A) return fail("rnf_fisher_exact: null pointer");
    return fisher_exact_launch("rnf_fisher_exact", A, B, c_out, mean_out, nullptr, nullptr, nullptr, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int rnf_fisher_entropy(const float *A, int64_t B, float *entropy_out, void *stream) {
    if (B < 0) return fail("rnf_fisher_entropy: B=%lld", (long long)B);
    if (B == 0) return 0;
    if (!A || !entropy_out) return fail("rnf_fisher_entropy: null pointer");
    return fisher_exact_launch("rnf_fisher_entropy", A, B, nullptr, nullptr, entropy_out, nullptr, nullptr, reinterpret_cast<hipStream_t>(stream));
}

// The maximum-likelihood matrix-Fisher parameter of B moment matrices (fisher_fit.h): ONE WAVE PER MATRIX, four per workgroup, as
// fisher_exact_kernel.  Every lane runs the same (wave-uniform) Newton iteration on the same s; an evaluation of the 14 integrals is a
// lane sum over nodes l, l + 64, .. and the xor butterfly, which leaves identical sums in every lane -- so the iteration count, the
// backtracking and the result of a row depend on nothing but the row.
struct FisherFitWaveEval {
    int lane;
    __device__ void operator()(const double s[3], double acc[kFisherFitSums]) const {
        fisher_fit_lane(s, lane, acc);
#pragma unroll
        for (int k = 0; k < kFisherFitSums; ++k)
            for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    }
};

__global__ __launch_bounds__(256) void fisher_fit_kernel(const double *moments, long long B, double cap, int max_iter, float *A_out, double *s_out,
                                                         double *H_out, int *iter_out, int *status_out) {
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;                                                  // wave-uniform
    double m[9], A[9], s[3], H[6];
    int iters, status;
    for (int k = 0; k < 9; ++k) m[k] = moments[b * 9 + k];
    fisher_fit_matrix(m, cap, max_iter, FisherFitWaveEval{lane}, A, s, H, iters, status);
    double a = 0.0, sv = 0.0, hv = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) a = lane == k ? A[k] : a;
#pragma unroll
    for (int k = 0; k < 3; ++k) sv = lane == k ? s[k] : sv;
#pragma unroll
    for (int k = 0; k < 6; ++k) hv = lane == k ? H[k] : hv;
    if (lane < 9) A_out[b * 9 + lane] = (float)a;
    if (s_out && lane < 3) s_out[b * 3 + lane] = sv;
    if (H_out && lane < 6) H_out[b * 6 + lane] = hv;
    if (lane == 0) {
        if (iter_out) iter_out[b] = iters;
        if (status_out) status_out[b] = status;
    }
}

extern "C" int rnf_fisher_fit(const RnfFisherFit *p) {
    if (check_struct(p, "RnfFisherFit")) return 1;
    if (p->B < 0) return fail("RnfFisherFit.B=%lld", (long long)p->B);
    if (!(p->max_concentration > 0.0 && p->max_concentration <= 3e4))
        return fail("RnfFisherFit.max_concentration=%g outside (0, 3e4]", p->max_concentration);
    if (p->max_iterations < 0 || p->max_iterations > kFisherFitMaxIter)
        return fail("RnfFisherFit.max_iterations=%d outside 0..%d (0: %d)", p->max_iterations, kFisherFitMaxIter, kFisherFitMaxIter);
    if (p->B == 0) return 0;
    if (!p->moments || !p->A_out) return fail("RnfFisherFit: null moments or A_out");
    const long long blocks = ((long long)p->B + 3) / 4;
    if (blocks > 0x7fffffffLL) return fail("RnfFisherFit.B=%lld is more than one launch serves", (long long)p->B);
    hipLaunchKernelGGL(fisher_fit_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(p->stream), p->moments, (long long)p->B,
                       p->max_concentration, p->max_iterations > 0 ? (int)p->max_iterations : kFisherFitMaxIter, p->A_out, p->s_out, p->hessian_out,
                       p->iterations_out, p->status_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Weighted moments M_g = sum_i w_gi R_gi of G groups of n rotations, in fp64 and in ONE fixed order: a group is cut into chunks of 4096 rows
// (a function of n alone), a 256-thread workgroup per (group, chunk) stages tiles of 256 rows through LDS (dwordx4 loads where the tile is
// 16-byte aligned, dword loads otherwise -- the same values either way), thread t adds rows t, t + 256, .. of its chunk in that order,
// the wave's xor butterfly and then waves 0, 1, 2, 3 in turn combine them, and one wave per group adds the chunk partials c, c + 64, ..
// and its butterfly.  Nothing depends on G, on the group's position or on the launch, and there are no atomics: a group's moment is
// bit-identical however it is batched.  With log-weights w = exp(lw - max lw) / sum (fp64 exp; the maximum is exact in any order);
// workspace per (group, chunk): 10 partial sums (9 entries, the weight) and the chunk's maximum.
namespace rmom {
constexpr int THREADS = 256, TILE = 256, CHUNK = 4096, SLOTS = 11;
static inline long long chunks_for(long long n) { return (n + CHUNK - 1) / CHUNK; }

__device__ inline float block_max(float m, float *smax) {
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
}

__global__ __launch_bounds__(THREADS) void rotation_moments_max_kernel(const float *lw, long long n, long long G, long long nchunk, double *ws) {
    __shared__ float smax[4];
    const long long g = blockIdx.x % G, ch = blockIdx.x / G;
    const long long lo = ch * CHUNK, hi = lo + CHUNK < n ? lo + CHUNK : n;
    float m = -INFINITY;
    for (long long i = lo + threadIdx.x; i < hi; i += THREADS) m = fmaxf(m, lw[g * n + i]);
    m = block_max(m, smax);
    if (threadIdx.x == 0) ws[(g * nchunk + ch) * SLOTS + 10] = (double)m;
}

__global__ __launch_bounds__(THREADS) void rotation_moments_kernel(const float *rot, long long group_stride, const float *lw, long long n, long long G,
                                                                   long long nchunk, double *ws) {
    __shared__ __attribute__((aligned(16))) float tile[TILE * 9];
    __shared__ float smax[4];
    __shared__ double red[4][10];
    const int tid = threadIdx.x;
    const long long g = blockIdx.x % G, ch = blockIdx.x / G;
    const long long lo = ch * CHUNK, hi = lo + CHUNK < n ? lo + CHUNK : n;
    double gmax = 0.0;
    if (lw) {
        float m = -INFINITY;
        for (long long c = tid; c < nchunk; c += THREADS) m = fmaxf(m, (float)ws[(g * nchunk + c) * SLOTS + 10]);
        gmax = (double)block_max(m, smax);
    }
    double acc[10];
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    for (long long t0 = lo; t0 < hi; t0 += TILE) {
        const int rows = (int)(hi - t0 < TILE ? hi - t0 : TILE), nelem = rows * 9;
        const float *src = rot + g * group_stride + t0 * 9;
        __syncthreads();                                                 // the previous tile has been read
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const int nq = nelem >> 2;
            for (int q = tid; q < nq; q += THREADS) reinterpret_cast<float4 *>(tile)[q] = reinterpret_cast<const float4 *>(src)[q];
            for (int e = 4 * nq + tid; e < nelem; e += THREADS) tile[e] = src[e];
        } else {
            for (int e = tid; e < nelem; e += THREADS) tile[e] = src[e];
        }
        __syncthreads();
        if (tid < rows) {
            const double w = lw ? exp((double)lw[g * n + t0 + tid] - gmax) : 1.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[k] += w * (double)tile[tid * 9 + k];     // stride 9: conflict-free
            acc[9] += w;
        }
    }
#pragma unroll
    for (int k = 0; k < 10; ++k)
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    if ((tid & 63) == 0)
        for (int k = 0; k < 10; ++k) red[tid >> 6][k] = acc[k];
    __syncthreads();
    if (tid < 10) ws[(g * nchunk + ch) * SLOTS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(64) void rotation_moments_final_kernel(const double *ws, long long nchunk, double *out) {
    const long long g = blockIdx.x;
    const int lane = threadIdx.x;
    double acc[10];
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    for (long long c = lane; c < nchunk; c += 64)
        for (int k = 0; k < 10; ++k) acc[k] += ws[(g * nchunk + c) * SLOTS + k];
#pragma unroll
    for (int k = 0; k < 10; ++k)
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    double mine = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) mine = lane == k ? acc[k] : mine;
    if (lane < 9) out[g * 9 + lane] = mine / acc[9];
}
}  // namespace rmom

static int rotation_moments_check(const RnfRotationMoments *p) {
    if (check_struct(p, "RnfRotationMoments")) return 1;
    if (p->G < 1) return fail("RnfRotationMoments.G=%lld must be >= 1", (long long)p->G);
    if (p->n < 1 || p->n > (1LL << 40)) return fail("RnfRotationMoments.n=%lld outside 1..2^40", (long long)p->n);
    if ((double)p->G * (double)rmom::chunks_for(p->n) > 2147483647.0)
        return fail("RnfRotationMoments: G=%lld groups of %lld chunks are more than one launch serves", (long long)p->G, rmom::chunks_for(p->n));
    return 0;
}

extern "C" size_t rnf_rotation_moments_workspace_bytes(const RnfRotationMoments *p) {
    if (rotation_moments_check(p)) return 0;
    return (size_t)p->G * (size_t)rmom::chunks_for(p->n) * rmom::SLOTS * sizeof(double);
}

extern "C" int rnf_rotation_moments(const RnfRotationMoments *p) {
    if (rotation_moments_check(p)) return 1;
    if (!p->rotations || !p->moments_out) return fail("RnfRotationMoments: null rotations or moments_out");
    if (p->shared_rotations && !p->log_weights) return fail("RnfRotationMoments.shared_rotations needs log_weights (every group would get the same moment)");
    const size_t need = rnf_rotation_moments_workspace_bytes(p);
    if (check_workspace(p, "RnfRotationMoments", need, "rnf_rotation_moments_workspace_bytes", 8)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(p->stream);
    const long long nchunk = rmom::chunks_for(p->n);
    const unsigned blocks = (unsigned)(p->G * nchunk);
    double *ws = (double *)p->workspace;
    if (p->log_weights) {
        hipLaunchKernelGGL(rmom::rotation_moments_max_kernel, dim3(blocks), dim3(rmom::THREADS), 0, s, p->log_weights, (long long)p->n, (long long)p->G,
                           nchunk, ws);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(rmom::rotation_moments_kernel, dim3(blocks), dim3(rmom::THREADS), 0, s, p->rotations,
                       p->shared_rotations ? 0LL : (long long)p->n * 9, p->log_weights, (long long)p->n, (long long)p->G, nchunk, ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rmom::rotation_moments_final_kernel, dim3((unsigned)p->G), dim3(64), 0, s, (const double *)ws, nchunk, p->moments_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// EM for mixtures of matrix-Fishers (fisher_mixture.h).  Per iteration two launches: mixture_accumulate_kernel, one 256-thread workgroup
// per (group, chunk) with the K parameter sets in LDS, adds the 10 K + 3 sums of its chunk in the order of rotation_moments_kernel
// (same tiles, same loads, same butterfly) into the workspace; mixture_finalise_kernel, one workgroup per group and one wave per
// component, adds the chunk partials as rotation_moments_final_kernel does and runs the M-step of its component on fisher_fit_matrix
// with the wave evaluator.  The state is A_out (fp32) and log_pi_out (fp64) themselves; c_k and the group's finished flag live in the
// workspace.  Workgroups of a finished group return at once (workgroup-uniform: the flag is read before the barrier that precedes
// any write of it).  No atomics, no host synchronisation; the launches depend on `iterations` alone.
namespace rmix {
constexpr int THREADS = 256, TILE = 256;

// c of one rounded fp32 parameter matrix by a whole wave, as fisher_exact_kernel computes it
__device__ __forceinline__ double wave_c(const float *A32, int lane) {
    double a[9], s[3], acc[5], m[3], c, h;
#pragma unroll
    for (int k = 0; k < 9; ++k) a[k] = (double)A32[k];
    proper_singular_values3(a, s);
    fisher_exact_lane(s, lane, acc);
#pragma unroll
    for (int k = 0; k < 5; ++k)
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    fisher_exact_finish(s, acc, c, m, h);
    return c;
}

// one workgroup per group, wave k = component k: the state copied to the outputs, c_k, and every output that a later kernel only
// writes in part
__global__ __launch_bounds__(64 * kMixMaxK) void mixture_prepare_kernel(const float *A_init, const double *log_pi_init, int K, int iterations,
                                                                        float *A_out, double *log_pi_out, double *s_out, double *loglik_out,
                                                                        double *went_out, int *status_out, int *iter_out, double *c_ws,
                                                                        int *flag_ws) {
    const long long g = blockIdx.x;
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long row = g * K + k;
    float a[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] = A_init[row * 9 + j];
    const double lp = log_pi_init ? log_pi_init[row] : -log((double)K);
    const double c = wave_c(a, lane);
    float mine = 0.f;
#pragma unroll
    for (int j = 0; j < 9; ++j) mine = lane == j ? a[j] : mine;
    if (lane < 9) A_out[row * 9 + lane] = mine;
    if (s_out && lane < 3) s_out[row * 3 + lane] = NAN;
    if (lane == 0) {
        log_pi_out[row] = lp;
        c_ws[row] = c;
        status_out[row] = lp == -INFINITY ? kMixEmpty : 0;
    }
    for (int t = threadIdx.x; t <= iterations; t += blockDim.x) loglik_out[g * (iterations + 1) + t] = NAN;
    if (threadIdx.x == 0) {
        if (went_out) went_out[g] = NAN;
        iter_out[g] = 0;
        flag_ws[g] = 0;
    }
}

template <int K>
__global__ __launch_bounds__(THREADS) void mixture_accumulate_kernel(const float *rot, long long group_stride, const float *lw, long long n, long long G,
                                                                     long long nchunk, const float *A, const double *log_pi, const double *c_ws,
                                                                     const int *flag_ws, int ignore_finished, const double *max_ws, double *part_ws,
                                                                     float *log_resp) {
    constexpr int S = mix_slots(K);
    __shared__ __attribute__((aligned(16))) float tile[TILE * 9];
    __shared__ float smax[4];
    __shared__ double pA[9 * K], pl[K], pc[K];
    __shared__ double red[4][S];
    const int tid = threadIdx.x;
    const long long g = blockIdx.x % G, ch = blockIdx.x / G;
    if (!ignore_finished && flag_ws[g]) return;                           // workgroup-uniform
    const long long lo = ch * kMixChunk, hi = lo + kMixChunk < n ? lo + kMixChunk : n;
    if (tid < 9 * K) pA[tid] = (double)A[g * 9 * K + tid];
    if (tid < K) {
        pl[tid] = log_pi[g * K + tid];
        pc[tid] = c_ws[g * K + tid];
    }
    double gmax = 0.0;
    if (lw) {
        float m = -INFINITY;
        for (long long c = tid; c < nchunk; c += THREADS) m = fmaxf(m, (float)max_ws[(g * nchunk + c) * rmom::SLOTS + 10]);
        gmax = (double)rmom::block_max(m, smax);
    }
    double acc[S];
#pragma unroll
    for (int q = 0; q < S; ++q) acc[q] = 0.0;
    for (long long t0 = lo; t0 < hi; t0 += TILE) {
        const int rows = (int)(hi - t0 < TILE ? hi - t0 : TILE), nelem = rows * 9;
        const float *src = rot + g * group_stride + t0 * 9;
        __syncthreads();                                                 // the previous tile has been read; the parameters are in LDS
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const int nq = nelem >> 2;
            for (int q = tid; q < nq; q += THREADS) reinterpret_cast<float4 *>(tile)[q] = reinterpret_cast<const float4 *>(src)[q];
            for (int e = 4 * nq + tid; e < nelem; e += THREADS) tile[e] = src[e];
        } else {
            for (int e = tid; e < nelem; e += THREADS) tile[e] = src[e];
        }
        __syncthreads();
        if (tid < rows) {
            const double d = lw ? (double)lw[g * n + t0 + tid] - gmax : 0.0, u = lw ? exp(d) : 1.0, e = u > 0.0 ? u * d : 0.0;
            fisher_mixture_add_row<K>(tile + tid * 9, u, e, pA, pl, pc, acc, log_resp ? log_resp + g * K * n + t0 + tid : nullptr, n);
        }
    }
#pragma unroll
    for (int q = 0; q < S; ++q)
        for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_xor(acc[q], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < S; ++q) red[tid >> 6][q] = acc[q];
    }
    __syncthreads();
    if (tid < S) part_ws[(g * nchunk + ch) * S + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(64 * kMixMaxK) void mixture_finalise_kernel(int K, int t, int iterations, int last, double tol, double cap, int weighted,
                                                                         long long nchunk, const double *part_ws, double *c_ws, int *flag_ws,
                                                                         float *A_out, double *log_pi_out, double *s_out, double *loglik_out,
                                                                         double *went_out, int *status_out, int *iter_out, float *log_resp,
                                                                         long long n) {
    const long long g = blockIdx.x;
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63, S = mix_slots(K);
    const long long row = g * K + k;
    const int finished = flag_ws[g];
    __syncthreads();                                                     // every wave has read the flag before wave 0 may set it
    if (finished) return;
    double acc[13];                                                      // the component's ten sums, then Z, sum u lse, sum u (lw - max)
#pragma unroll
    for (int q = 0; q < 13; ++q) acc[q] = 0.0;
    for (long long c = lane; c < nchunk; c += 64) {
        const double *p = part_ws + (g * nchunk + c) * S;
#pragma unroll
        for (int q = 0; q < 10; ++q) acc[q] += p[10 * k + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[10 + q] += p[10 * K + q];
    }
#pragma unroll
    for (int q = 0; q < 13; ++q)
        for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_xor(acc[q], o, 64);
    double L, went;
    double *ll = loglik_out + g * (iterations + 1);
    if (!fisher_mixture_group(acc[10], acc[11], acc[12], weighted != 0, L, went)) {        // a NaN group: NaN throughout, status INPUT
        if (lane < 9) A_out[row * 9 + lane] = NAN;
        if (s_out && lane < 3) s_out[row * 3 + lane] = NAN;
        if (lane == 0) {
            log_pi_out[row] = NAN;
            status_out[row] = kFisherFitInput;
        }
        if (log_resp)                                                   // the last pass: what the accumulate launch before it wrote
            for (long long i = lane; i < n; i += 64) log_resp[row * n + i] = NAN;
        if (k == 0) {
            for (int q = lane; q <= iterations; q += 64) ll[q] = NAN;
            if (lane == 0) {
                if (went_out) went_out[g] = NAN;
                iter_out[g] = t;
                flag_ws[g] = 1;
            }
        }
        return;
    }
    const double prev = t > 0 ? ll[t - 1] : 0.0;
    if (k == 0 && lane == 0) {
        ll[t] = L;
        if (went_out) went_out[g] = went;
        iter_out[g] = t;
    }
    if (last) return;
    if (t > 0 && tol > 0.0 && L - prev >= 0.0 && L - prev <= tol) {
        if (k == 0 && lane == 0) flag_ws[g] = 1;
        return;
    }
    bool live = log_pi_out[row] != -INFINITY;                           // wave-uniform from here on
    double lp = 0.0, s[3];
    float A32[9];
    int status = 0;
    if (live) live = fisher_mixture_mstep(acc, acc[10], cap, FisherFitWaveEval{lane}, lp, A32, s, status);
    if (!live) {
        if (lane == 0) {
            log_pi_out[row] = -INFINITY;
            status_out[row] = kMixEmpty;
        }
        return;
    }
    const double c = wave_c(A32, lane);
    float a = 0.f;
    double sv = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) a = lane == j ? A32[j] : a;
#pragma unroll
    for (int j = 0; j < 3; ++j) sv = lane == j ? s[j] : sv;
    if (lane < 9) A_out[row * 9 + lane] = a;
    if (s_out && lane < 3) s_out[row * 3 + lane] = sv;
    if (lane == 0) {
        log_pi_out[row] = lp;
        c_ws[row] = c;
        status_out[row] = status;
    }
}

// log p and the log-responsibilities of n rotations under one mixture: the row function of the E-step.  Every workgroup computes the K
// normalisers itself (waves k, k + 4, ..), so no workspace is needed.
template <int K>
__global__ __launch_bounds__(THREADS) void mixture_log_prob_kernel(const float *A, const double *log_pi, const float *rot, long long n, float *logp,
                                                                   float *log_resp) {
    __shared__ double pA[9 * K], pl[K], pc[K];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int k = wave; k < K; k += 4) {
        const double c = wave_c(A + 9 * k, lane);
        if (lane == 0) pc[k] = c;
    }
    if (tid < 9 * K) pA[tid] = (double)A[tid];
    if (tid < K) pl[tid] = log_pi[tid];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * THREADS + tid; i < n; i += (long long)gridDim.x * THREADS) {
        float R[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = rot[i * 9 + j];
        double l[K], lse;
        fisher_mixture_row<K>(R, pA, pl, pc, l, lse);
        logp[i] = (float)lse;
        if (log_resp) {
#pragma unroll
            for (int k = 0; k < K; ++k) log_resp[k * n + i] = (float)(l[k] - lse);
        }
    }
}

static inline long long chunks_for(long long n) { return (n + kMixChunk - 1) / kMixChunk; }
}  // namespace rmix

#define RNF_MIX_DISPATCH(K, ...)                                                                                                  \
    switch (K) {                                                                                                                    \
        case 1: { constexpr int KK = 1; __VA_ARGS__; } break;                                                                              \
        case 2: { constexpr int KK = 2; __VA_ARGS__; } break;                                                                              \
        case 3: { constexpr int KK = 3; __VA_ARGS__; } break;                                                                              \
        case 4: { constexpr int KK = 4; __VA_ARGS__; } break;                                                                              \
        case 5: { constexpr int KK = 5; __VA_ARGS__; } break;                                                                              \
        case 6: { constexpr int KK = 6; __VA_ARGS__; } break;                                                                              \
        case 7: { constexpr int KK = 7; __VA_ARGS__; } break;                                                                              \
        default: { constexpr int KK = 8; __VA_ARGS__; } break;                                                                             \
    }

static int fisher_mixture_check(const RnfFisherMixtureFit *p) {
    if (check_struct(p, "RnfFisherMixtureFit")) return 1;
    if (p->G < 1 || p->G > 0x7fffffffLL) return fail("RnfFisherMixtureFit.G=%lld outside 1..2^31-1", (long long)p->G);
    if (p->n < 1 || p->n > (1LL << 40)) return fail("RnfFisherMixtureFit.n=%lld outside 1..2^40", (long long)p->n);
    if (p->K < 1 || p->K > kMixMaxK) return fail("RnfFisherMixtureFit.K=%d outside 1..%d", (int)p->K, kMixMaxK);
    if (p->iterations < 1 || p->iterations > kMixMaxIterations)
        return fail("RnfFisherMixtureFit.iterations=%d outside 1..%d", (int)p->iterations, kMixMaxIterations);
    if ((double)p->G * (double)rmix::chunks_for(p->n) > 2147483647.0)
        return fail("RnfFisherMixtureFit: G=%lld groups of %lld chunks are more than one launch serves", (long long)p->G, rmix::chunks_for(p->n));
    return 0;
}

// workspace, in doubles: chunk partials [G][nchunk][10 K + 3] | chunk maxima in the layout of rotation_moments_max_kernel [G][nchunk][11] |
// c [G][K] | finished flags [G] (int32, one per 8 bytes)
extern "C" size_t rnf_fisher_mixture_fit_workspace_bytes(const RnfFisherMixtureFit *p) {
    if (fisher_mixture_check(p)) return 0;
    const size_t cells = (size_t)p->G * (size_t)rmix::chunks_for(p->n);
    return (cells * (size_t)(mix_slots(p->K) + rmom::SLOTS) + (size_t)p->G * (size_t)p->K + (size_t)p->G) * sizeof(double);
}

extern "C" int rnf_fisher_mixture_fit(const RnfFisherMixtureFit *p) {
    if (fisher_mixture_check(p)) return 1;
    if (!p->rotations || !p->A_init || !p->A_out || !p->log_pi_out || !p->loglik_out || !p->status_out || !p->iterations_out)
        return fail("RnfFisherMixtureFit: null rotations, A_init, A_out, log_pi_out, loglik_out, status_out or iterations_out");
    if (p->shared_rotations && !p->log_weights) return fail("RnfFisherMixtureFit.shared_rotations needs log_weights (every group would be the same)");
    if (!(p->tol >= 0.0)) return fail("RnfFisherMixtureFit.tol=%g must be >= 0", p->tol);
    if (!(p->max_concentration > 0.0 && p->max_concentration <= 3e4))
        return fail("RnfFisherMixtureFit.max_concentration=%g outside (0, 3e4]", p->max_concentration);
    const size_t need = rnf_fisher_mixture_fit_workspace_bytes(p);
    if (check_workspace(p, "RnfFisherMixtureFit", need, "rnf_fisher_mixture_fit_workspace_bytes", 8)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(p->stream);
    const int K = p->K, T = p->iterations;
    const long long G = p->G, n = p->n, nchunk = rmix::chunks_for(n);
    const size_t cells = (size_t)G * (size_t)nchunk;
    double *part_ws = (double *)p->workspace, *max_ws = part_ws + cells * mix_slots(K), *c_ws = max_ws + cells * rmom::SLOTS;
    int *flag_ws = reinterpret_cast<int *>(c_ws + (size_t)G * K);
    const unsigned blocks = (unsigned)cells;
    const long long stride = p->shared_rotations ? 0LL : n * 9;
    if (p->log_weights) {
        hipLaunchKernelGGL(rmom::rotation_moments_max_kernel, dim3(blocks), dim3(rmom::THREADS), 0, st, p->log_weights, n, G, nchunk, max_ws);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(rmix::mixture_prepare_kernel, dim3((unsigned)G), dim3(64 * K), 0, st, p->A_init, p->log_pi_init, K, T, p->A_out, p->log_pi_out,
                       p->s_out, p->loglik_out, p->weight_entropy_out, p->status_out, p->iterations_out, c_ws, flag_ws);
    HIP_TRY(hipGetLastError());
    for (int t = 0; t <= T; ++t) {
        const int last = t == T;
        RNF_MIX_DISPATCH(K, hipLaunchKernelGGL(rmix::mixture_accumulate_kernel<KK>, dim3(blocks), dim3(rmix::THREADS), 0, st, p->rotations, stride,
                                               p->log_weights, n, G, nchunk, (const float *)p->A_out, (const double *)p->log_pi_out,
                                               (const double *)c_ws, (const int *)flag_ws, last, (const double *)max_ws, part_ws,
                                               last ? p->log_resp_out : (float *)nullptr));
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(rmix::mixture_finalise_kernel, dim3((unsigned)G), dim3(64 * K), 0, st, K, t, T, last, p->tol, p->max_concentration,
                           p->log_weights ? 1 : 0, nchunk, (const double *)part_ws, c_ws, flag_ws, p->A_out, p->log_pi_out, p->s_out, p->loglik_out,
                           p->weight_entropy_out, p->status_out, p->iterations_out, last ? p->log_resp_out : (float *)nullptr, n);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int rnf_fisher_mixture_log_prob(const float *A, const double *log_pi, int32_t K, const float *rotations, int64_t n, float *logp_out,
                                           float *log_resp_out, void *stream) {
    if (K < 1 || K > kMixMaxK) return fail("rnf_fisher_mixture_log_prob: K=%d outside 1..%d", (int)K, kMixMaxK);
    if (n < 0) return fail("rnf_fisher_mixture_log_prob: n=%lld", (long long)n);
    if (n == 0) return 0;
    if (!A || !log_pi || !rotations || !logp_out) return fail("rnf_fisher_mixture_log_prob: null pointer");
    long long blocks = ((long long)n + rmix::THREADS - 1) / rmix::THREADS;
    if (blocks > 1024) blocks = 1024;
    RNF_MIX_DISPATCH(K, hipLaunchKernelGGL(rmix::mixture_log_prob_kernel<KK>, dim3((unsigned)blocks), dim3(rmix::THREADS), 0,
                                           reinterpret_cast<hipStream_t>(stream), A, log_pi, rotations, (long long)n, logp_out, log_resp_out));
    HIP_TRY(hipGetLastError());
    return 0;
}

// pytorch3d.transforms.matrix_to_quaternion (published 0.7.5 rule; call sites flow/squeezetrans.py:34, utils/fisher.py:243): real part first,
// the candidate with the largest |q_i|, denominators floored at 0.1 (so3_math.h rot_to_quat).  rot [n][9] row-major -> quat [n][4].
__global__ void matrix_to_quaternion_kernel(const float *rot, long long n, float *quat) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float *r = rot + i * 9;
        Rot R;
        R.c0 = v3f{r[0], r[3], r[6]}; R.c1 = v3f{r[1], r[4], r[7]}; R.c2 = v3f{r[2], r[5], r[8]};
        float q[4];
        rot_to_quat(R, q);
        quat[i * 4] = q[0]; quat[i * 4 + 1] = q[1]; quat[i * 4 + 2] = q[2]; quat[i * 4 + 3] = q[3];
    }
}
extern "C" int rnf_matrix_to_quaternion(const float *rot, int64_t n, float *quat, void *stream) {
    if (n < 0) return fail("rnf_matrix_to_quaternion: n=%lld", (long long)n);
    if (n == 0) return 0;
    if (!rot || !quat) return fail("rnf_matrix_to_quaternion: null pointer");
    long long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(matrix_to_quaternion_kernel, dim3((int)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rot, (long long)n, quat);
    HIP_TRY(hipGetLastError());
    return 0;
}

// norm_type 2 (utils/fisher.py:98-101): Monte-Carlo estimate of the normaliser over `approx_num` uniform rotations -- norm = mean_k
// exp(tr(R_k^T A) - sum S), hence c = sum S + log norm.  The reference broadcasts [approx_num,3,3] * [N,3,3], i.e. it serves ONE matrix
// (N = 1).  Uniform rotations from normalised Gaussian quaternions on the counter-based Philox stream of the sampler (the reference uses
// pytorch3d.transforms.random_rotations on torch's generator: parity is statistical, error ~ 1/sqrt(approx_num)).
__global__ void fisher_mc_accum_kernel(const float *A, long long n_mc, unsigned long long seed, double *acc /* [0] = sum exp(tr - sumS) */) {
    double a[9], U[9], s[3], V[9];
    for (int k = 0; k < 9; ++k) a[k] = A[k];
    proper_svd3(a, U, s, V);
    const float sumS = (float)(s[0] + s[1] + s[2]);
    float af[9];
    for (int k = 0; k < 9; ++k) af[k] = A[k];
    const Philox rng{(unsigned)seed, (unsigned)(seed >> 32)};
    double part = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_mc; i += (long long)gridDim.x * blockDim.x) {
        unsigned c0[4] = {(unsigned)i, (unsigned)(i >> 32), 0x4d43u, 0u};
        rng(c0);
        const float r0 = sqrtf(-2.0f * logf(u01(c0[0]))), r1 = sqrtf(-2.0f * logf(u01(c0[2])));
        float s0, k0, s1, k1;
        sincosf(kTwoPi * u01(c0[1]), &s0, &k0);
        sincosf(kTwoPi * u01(c0[3]), &s1, &k1);
        const float q[4] = {r0 * k0, r0 * s0, r1 * k1, r1 * s1};
        Rot R;
        quat_to_rot(q, q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3], R);
        const float tr = R.c0.x * af[0] + R.c1.x * af[1] + R.c2.x * af[2] + R.c0.y * af[3] + R.c1.y * af[4] + R.c2.y * af[5] + R.c0.z * af[6] +
                         R.c1.z * af[7] + R.c2.z * af[8];
        part += (double)expf(tr - sumS);
    }
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(acc, part);
}
__global__ void fisher_mc_final_kernel(const float *A, long long n_mc, const double *acc, float *c_out) {
    double a[9], U[9], s[3], V[9];
    for (int k = 0; k < 9; ++k) a[k] = A[k];
    proper_svd3(a, U, s, V);
    c_out[0] = (float)(s[0] + s[1] + s[2] + log(acc[0] / (double)n_mc));
}
extern "C" int rnf_fisher_log_const_mc(const float *A, int64_t B, int64_t approx_num, uint64_t seed, void *scratch, size_t scratch_bytes, float *c_out,
                                       void *stream) {
    if (!A || !c_out || !scratch) return fail("rnf_fisher_log_const_mc: null pointer");
    if (B != 1) return fail("rnf_fisher_log_const_mc: the reference's norm_type 2 broadcasts its random rotations against ONE matrix (got B=%lld)", (long long)B);
    if (approx_num <= 0) return fail("rnf_fisher_log_const_mc: approx_num=%lld must be positive", (long long)approx_num);
    if (scratch_bytes < sizeof(double)) return fail("rnf_fisher_log_const_mc: 8 bytes of scratch are needed");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(scratch, 0, sizeof(double), st));
    long long blocks = (approx_num + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(fisher_mc_accum_kernel, dim3((int)blocks), dim3(256), 0, st, A, (long long)approx_num, (unsigned long long)seed, static_cast<double *>(scratch));
    hipLaunchKernelGGL(fisher_mc_final_kernel, dim3(1), dim3(1), 0, st, A, (long long)approx_num, static_cast<const double *>(scratch), c_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" size_t rnf_fisher_scratch_bytes(int64_t B) { return (size_t)(2 + 10 * (B > 0 ? B : 0)) * sizeof(double); }

extern "C" int rnf_fisher_log_const_nt(const float *A, int64_t B, int32_t norm_type, void *scratch, size_t scratch_bytes, float *c_out, void *stream) {
    if (!A || !c_out) return fail("rnf_fisher_log_const_nt: null pointer");
    if (B <= 0) return fail("rnf_fisher_log_const_nt: B=%lld", (long long)B);
    if (norm_type == RNF_FISHER_NORM_EXACT)
        return fisher_exact_launch("rnf_fisher_log_const_nt", A, B, c_out, nullptr, nullptr, nullptr, nullptr, reinterpret_cast<hipStream_t>(stream));
    if (norm_type != 0 && norm_type != 1)
        return fail("rnf_fisher_log_const_nt: norm_type=%d -- the closed-form approximations 0 and 1 (utils/fisher.py:88-97) and the exact integral "
                    "RNF_FISHER_NORM_EXACT are built", (int)norm_type);
    if (norm_type == 0 && (!scratch || scratch_bytes < 2 * sizeof(double))) return fail("rnf_fisher_log_const_nt: norm_type 0 needs 16 bytes of scratch");
    return fisher_const_launch(A, B, norm_type, static_cast<double *>(scratch), c_out, reinterpret_cast<hipStream_t>(stream));
}

// d log p / dA (agent.py:57-65 keeps a predicted A in the graph):  g_A[b] = sum_{i in row b} g_i R_i  -  (sum_{i in row b} g_i) dc_b/dA_b
// (+ the batch coupling of norm_type 0 through Q).  Pass 1 accumulates T_b = sum g_i R_i and G_b = sum g_i in fp64: 256 consecutive
// samples per block step; a step inside one row reduces in the block and issues 10 atomics, a step that spans rows lets every sample
// add to its own row.
__global__ void fisher_grad_accum_kernel(const float *g, const float *rot, long long n, long long div, double *acc) {
    __shared__ double red[4][10];
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
        const long long i = base + threadIdx.x;
        const long long last = base + 255 < n ? base + 255 : n - 1;
        const bool one_row = base / div == last / div;                   // block uniform
        double v[10];
        const float gi = i < n ? g[i] : 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = i < n ? (double)gi * (double)rot[i * 9 + k] : 0.0;
        v[9] = gi;
        if (one_row) {
#pragma unroll
            for (int k = 0; k < 10; ++k)
                for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
            if ((threadIdx.x & 63) == 0)
                for (int k = 0; k < 10; ++k) red[threadIdx.x >> 6][k] = v[k];
            __syncthreads();
            if (threadIdx.x < 10) atomicAdd(acc + 10 * (base / div) + threadIdx.x, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
            __syncthreads();
        } else if (i < n) {
            double *dst = acc + 10 * (i / div);
#pragma unroll
            for (int k = 0; k < 10; ++k) atomicAdd(dst + k, v[k]);
        }
    }
}

// norm_type 0: W = sum_b G_b / D_b, D_b = 1 + Q/6 + det(A_b)/6  (the weight of dQ/dA_b' = 2 A_b' in every row's gradient)
__global__ void fisher_grad_w_kernel(const float *A, long long B, double *scratch) {
    double w = 0.0;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (long long)gridDim.x * blockDim.x) {
        double a[9];
        for (int k = 0; k < 9; ++k) a[k] = A[b * 9 + k];
        w += scratch[2 + 10 * b + 9] / (1.0 + scratch[0] / 6.0 + det3d(a) / 6.0);
    }
    for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(scratch + 1, w);
}

__global__ void fisher_grad_final_kernel(const float *A, long long B, int norm_type, const double *scratch, float *g_A) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double a[9], dc[9];
    for (int k = 0; k < 9; ++k) a[k] = A[b * 9 + k];
    fisher_log_const(a, norm_type, norm_type == 0 ? scratch[0] : 0.0, dc);
    const double *acc = scratch + 2 + 10 * b;
    for (int k = 0; k < 9; ++k) {
        double v = acc[k] - acc[9] * dc[k];
        if (norm_type == 0) v -= scratch[1] * a[k] / 3.0;
        g_A[b * 9 + k] = (float)v;
    }
}

extern "C" int rnf_fisher_log_prob_backward_param(const float *g_logp, const float *rot, int64_t n, const float *A, int64_t B, int32_t norm_type,
                                              void *scratch, size_t scratch_bytes, float *g_A, void *stream) {
    if (!g_logp || !rot || !A || !g_A || !scratch) return fail("rnf_fisher_log_prob_backward_param: null pointer");
    if (B <= 0 || n % B) return fail("n=%lld not divisible by fisher rows B=%lld (utils/fisher.py:226)", (long long)n, (long long)B);
    if (norm_type != 0 && norm_type != 1 && norm_type != RNF_FISHER_NORM_EXACT)
        return fail("rnf_fisher_log_prob_backward_param: norm_type=%d is not built", (int)norm_type);
    if (scratch_bytes < rnf_fisher_scratch_bytes(B)) return fail("rnf_fisher_log_prob_backward_param: scratch of %zu bytes, need %zu", scratch_bytes, rnf_fisher_scratch_bytes(B));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double *sc = static_cast<double *>(scratch);
    HIP_TRY(hipMemsetAsync(sc, 0, rnf_fisher_scratch_bytes(B), st));
    if (norm_type == 0) {
        long long blocks = (B * 9 + 255) / 256;
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(fisher_frobenius_kernel, dim3((int)blocks), dim3(256), 0, st, A, (long long)B, sc);
    }
    if (n > 0) {
        long long blocks = (n + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(fisher_grad_accum_kernel, dim3((int)blocks), dim3(256), 0, st, g_logp, rot, (long long)n, (long long)(n / B), sc + 2);
    }
    if (norm_type == 0) {
        long long blocks = (B + 255) / 256;
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(fisher_grad_w_kernel, dim3((int)blocks), dim3(256), 0, st, A, (long long)B, sc);
    }
    // the exact normaliser finishes in its own wave-per-matrix kernel: the quadrature never runs serially in a thread-per-matrix kernel
    if (norm_type == RNF_FISHER_NORM_EXACT) return fisher_exact_launch("rnf_fisher_log_prob_backward_param", A, B, nullptr, nullptr, nullptr, sc + 2, g_A, st);
    hipLaunchKernelGGL(fisher_grad_final_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, A, (long long)B, norm_type, sc, g_A);
    HIP_TRY(hipGetLastError());
    return 0;
}

// d(tr(A^T R) - c)/dR = A: g_rot[i] = g_logp[i] * A[row(i)]
__global__ void fisher_log_prob_backward_kernel(const float *g_logp, long long n, const float *A, long long div, float *g_rot) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const long long row = i / div;
        const float g = g_logp[i];
#pragma unroll
        for (int k = 0; k < 9; ++k) g_rot[i * 9 + k] = g * A[row * 9 + k];
    }
}

extern "C" int rnf_fisher_log_prob_backward(const float *g_logp, int64_t n, const float *A, int64_t B, float *g_rot, void *stream) {
    if (!g_logp || !A || !g_rot) return fail("rnf_fisher_log_prob_backward: null pointer");
    if (B <= 0 || n % B) return fail("n=%lld not divisible by fisher rows B=%lld (utils/fisher.py:226)", (long long)n, (long long)B);
    if (n == 0) return 0;
    long long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(fisher_log_prob_backward_kernel, dim3((int)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g_logp, (long long)n, A,
                       (long long)(n / B), g_rot);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int rnf_fisher_sample(const float *U, const float *V, const float *lam, int64_t B, int64_t n, uint64_t seed, float *out,
                                 int32_t *fail_flag_dev, void *stream) {
    if (!U || !V || !lam || !out) return fail("rnf_fisher_sample: null pointer");
    if (B <= 0 || n < 0) return fail("rnf_fisher_sample: B=%lld, n=%lld", (long long)B, (long long)n);
    if (n == 0) return 0;
    long long blocks = (B * n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(fisher_sample_kernel, dim3((int)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), U, V, lam,
                       (long long)B, (long long)n, (unsigned long long)seed, out, fail_flag_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ConditionalTransform alone: y [n,3] -> [n,4K] in the reference's row order (bring-up / unit test of the MFMA chain)
template <int NWc, int PREC>
__global__ __launch_bounds__(NWc * 64) void conditioner_kernel(const float *y, long long n, const float *layer, int KT, int K, float *out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const long long ntiles = (n + NWc * 32 - 1) / (NWc * 32);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long sample = (tile * NWc + wave) * 32 + j;
        const bool valid = sample < n;
        float y0 = 0.f, y1 = 0.f, y2 = 0.f;
        if (valid) { y0 = y[sample * 3]; y1 = y[sample * 3 + 1]; y2 = y[sample * 3 + 2]; }
        __syncthreads();
        if constexpr (PREC == 2) B3Head::stage(lds, layer, tid, NWc * 64);
        else stage_floats(lds, layer, MOB_HEAD_FLOATS, tid, NWc * 64);
        __syncthreads();
        typename Mlp<PREC>::Act tt;
        bool bad = false;
        if constexpr (PREC == 2) {
            B3Head::Units units{lds};
            Mlp<2>::head_ring<GFrag<false>, false>(units, lane, h, y0, y1, y2, GFrag<false>{nullptr, false}, tt, bad);
        } else {
            Fair nofair{lds, wave, -1, 0};
            Mlp<PREC>::head(lds, lane, h, y0, y1, y2, GFrag<false>{nullptr, false}, tt, nofair, bad);
        }
        // fc_last: one tile at a time (bf16x3: the head and one tile are 87 KiB)
        constexpr int T_LDS = PREC == 2 ? B3Head::LAST : MOB_LAST;
        for (int tau = 0; tau < KT; ++tau) {
            __syncthreads();
            stage_floats(lds + T_LDS, layer + Lay<PREC>::LAST + (size_t)tau * Lay<PREC>::LAST_TILE_FLOATS, Lay<PREC>::LAST_TILE_FLOATS, tid, NWc * 64);
            __syncthreads();
            f32x16 o = Mlp<PREC>::last(lds + T_LDS, lane, h, tt);
            if (valid) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int k = 8 * tau + 2 * g + h;
                        const int row = c == 0 ? k : K + 3 * k + (c - 1);
                        if (k < K) out[sample * 4 * K + row] = c == 0 ? S_UNSCALE * o[4 * g] : o[4 * g + c];   // (k >= K: pad rows; s: layout.h S_PRESCALE)
                    }
            }
        }
    }
}

extern "C" int rnf_conditioner_forward(const float *y, int64_t n, const float *layer, int32_t K, int32_t prec, float *out,
                                       void *stream) {
    if (K <= 0) return fail("segments=%d must be positive", K);
    if (prec != RNF_PREC_FP32 && prec != RNF_PREC_F16X2 && prec != RNF_PREC_BF16X3) return fail("unknown precision %d", prec);
    if (!y || !layer || !out) return fail("rnf_conditioner_forward: null pointer");
    if (n == 0) return 0;
    const size_t lds_bytes = sizeof(float) * (prec == RNF_PREC_BF16X3 ? B3Head::HEAD_TILE_FLOATS : MOB_HEAD_FLOATS + MOB_LAST_TILE_FLOATS);
    long long ntiles = (n + NW * 32 - 1) / (NW * 32);
    int grid = (int)(ntiles < device_cus() ? ntiles : device_cus());
    auto kern = prec == RNF_PREC_BF16X3 ? conditioner_kernel<NW, 2> : (prec ? conditioner_kernel<NW, 1> : conditioner_kernel<NW, 0>);
    return launch(kern, grid, NW * 64, lds_bytes, reinterpret_cast<hipStream_t>(stream), y, (long long)n, layer, (K + 7) / 8, K, out);
}
