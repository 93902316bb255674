// TEST INFRASTRUCTURE: the per-sample 3x3 Gram-Schmidt routines of csrc/so3_math.h (smith3; cond_gs9_apply, forward and inverse pass)
// compiled for the HOST, one matrix per call of the header's own definition, so that every sample can be judged against fp64 on a CPU
// (tests/test_gs3_host.py).  The reverse step goes through hg_cond9 of host_grad.cpp.  Not part of librnf_hip.so.
#include "../../rotationnormflow_amd/csrc/so3_math.h"

using namespace rnf;

extern "C" {
// Q [n][9] row-major (columns q0, q1, q2) = smith3(M [n][9])
void hs_smith3(const float *M, float *Q, int n) {
    for (int i = 0; i < n; ++i) {
        float m[9];
        for (int k = 0; k < 9; ++k) m[k] = M[9 * i + k];
        v3f q0, q1, q2;
        smith3(m, q0, q1, q2);
        float *q = Q + 9 * i;
        q[0] = q0.x; q[1] = q1.x; q[2] = q2.x; q[3] = q0.y; q[4] = q1.y; q[5] = q2.y; q[6] = q0.z; q[7] = q1.z; q[8] = q2.z;
    }
}
// (Rout [n][9] row-major, ldj [n]) = cond_gs9_apply(M [n][9], inverse, Rin [n][9] row-major), ldj starting from 0
void hs_gs9(const float *M, const float *Rin, int inverse, int n, float *Rout, float *ldj) {
    for (int i = 0; i < n; ++i) {
        float m[9];
        for (int k = 0; k < 9; ++k) m[k] = M[9 * i + k];
        const float *s = Rin + 9 * i;
        Rot R;
        R.c0 = v3f{s[0], s[3], s[6]}; R.c1 = v3f{s[1], s[4], s[7]}; R.c2 = v3f{s[2], s[5], s[8]};
        float l = 0.f;
        cond_gs9_apply(m, inverse != 0, R, l);
        float *d = Rout + 9 * i;
        d[0] = R.c0.x; d[1] = R.c1.x; d[2] = R.c2.x; d[3] = R.c0.y; d[4] = R.c1.y; d[5] = R.c2.y; d[6] = R.c0.z; d[7] = R.c1.z; d[8] = R.c2.z;
        ldj[i] = l;
    }
}
}
