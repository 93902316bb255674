// TEST INFRASTRUCTURE: the per-sample 6x6 layer of csrc/so3_math.h (cond_gs36_apply, forward and inverse pass) and its reverse step
// (csrc/so3_grad.h cond_gs36_backward) compiled for the HOST, one matrix per call of the header's own definition -- exactly what
// cond36_finish (flow_kernels.h) and rare_gs36 (train_kernels.h) call -- so that every sample can be judged against fp64 on a CPU
// (tests/test_gs36_host.py).  Not part of librnf_hip.so.
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
// (Rout [n][9] row-major, ldj [n]) = cond_gs36_apply(M [n][36], inverse, Rin [n][9] row-major), ldj starting from 0
void h36_apply(const float *M, const float *Rin, int inverse, int n, float *Rout, float *ldj) {
    for (int i = 0; i < n; ++i) {
        float m[36];
        for (int k = 0; k < 36; ++k) m[k] = M[36 * i + k];
        Rot R = load_rot(Rin + 9 * i);
        float l = 0.f;
        cond_gs36_apply(m, inverse != 0, R, l);
        store_rot(R, Rout + 9 * i);
        ldj[i] = l;
    }
}
// (gM [n][36], gRin [n][9] row-major) = cond_gs36_backward(M [n][36], inverse, Rin, gRout [n][9] row-major, g_ldj [n])
void h36_backward(const float *M, const float *Rin, const float *gRout, const float *g_ldj, int inverse, int n, float *gM, float *gRin) {
    for (int i = 0; i < n; ++i) {
        float m[36], gm[36];
        for (int k = 0; k < 36; ++k) m[k] = M[36 * i + k];
        Rot gi;
        cond_gs36_backward(m, inverse != 0, load_rot(Rin + 9 * i), load_rot(gRout + 9 * i), g_ldj[i], gm, gi);
        for (int k = 0; k < 36; ++k) gM[36 * i + k] = gm[k];
        store_rot(gi, gRin + 9 * i);
    }
}
}
