// TEST INFRASTRUCTURE: the per-sample 4x4 layer of csrc/so3_math.h (cond16_apply, forward and inverse pass) and its reverse step
// (csrc/so3_grad.h cond16_backward) compiled for the HOST, one matrix per call of the headers' own definitions, so that every sample can be
// judged against fp64 on a CPU (tests/test_aff16_host.py).  Not part of librnf_hip.so.
#include "../../rotationnormflow_amd/csrc/so3_grad.h"

using namespace rnf;

static Rot load_rot(const float *s) {
    Rot R;
    R.c0 = v3f{s[0], s[3], s[6]}; R.c1 = v3f{s[1], s[4], s[7]}; R.c2 = v3f{s[2], s[5], s[8]};
    return R;
}
static void store_rot(const Rot &R, float *d) {
    d[0] = R.c0.x; d[1] = R.c1.x; d[2] = R.c2.x; d[3] = R.c0.y; d[4] = R.c1.y; d[5] = R.c2.y; d[6] = R.c0.z; d[7] = R.c1.z; d[8] = R.c2.z;
}

extern "C" {
// (Rout [n][9] row-major, ldj [n]) = cond16_apply(M [n][16], inverse, Rin [n][9] row-major), ldj starting from 0
void ha_cond16(const float *M, const float *Rin, int inverse, int n, float *Rout, float *ldj) {
    for (int i = 0; i < n; ++i) {
        float m[16];
        for (int k = 0; k < 16; ++k) m[k] = M[16 * i + k];
        Rot R = load_rot(Rin + 9 * i);
        float l = 0.f;
        cond16_apply(m, inverse != 0, R, l);
        store_rot(R, Rout + 9 * i);
        ldj[i] = l;
    }
}
// (dL/dM [n][16], dL/dRin [n][9]) = cond16_backward(M [n][16], inverse, Rin, cotangents of R' and ldj)
void ha_cond16_backward(const float *M, const float *Rin, int inverse, const float *gRout, const float *g_ldj, int n, float *gM, float *gRin) {
    for (int i = 0; i < n; ++i) {
        float m[16], gm[16];
        for (int k = 0; k < 16; ++k) m[k] = M[16 * i + k];
        Rot gi;
        cond16_backward(m, inverse != 0, load_rot(Rin + 9 * i), load_rot(gRout + 9 * i), g_ldj[i], gm, gi);
        for (int k = 0; k < 16; ++k) gM[16 * i + k] = gm[k];
        store_rot(gi, gRin + 9 * i);
    }
}
// M^-1 and det M by inv4, the form the other callers of the 4x4 inverse use
void ha_inv4(const float *M, int n, float *Mi, float *det) {
    for (int i = 0; i < n; ++i) {
        float m[16], o[16];
        for (int k = 0; k < 16; ++k) m[k] = M[16 * i + k];
        det[i] = inv4(m, o);
        for (int k = 0; k < 16; ++k) Mi[16 * i + k] = o[k];
    }
}
}
