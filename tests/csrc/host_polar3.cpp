// TEST INFRASTRUCTURE: polar3 (csrc/so3_math.h) and polar3_backward (csrc/so3_grad.h) compiled for the HOST, one matrix per call of the
// header's own definition, so that every sample can be judged against fp64 on a CPU (tests/test_polar3_host.py).  The whole layer goes
// through hg_cond9 of host_grad.cpp.  Not part of librnf_hip.so.
#include "../../rotationnormflow_amd/csrc/so3_grad.h"

using namespace rnf;

extern "C" {
// Q [n][9] row-major = polar3(M [n][9])
void hp_polar3(const float *M, float *Q, int n) {
    for (int i = 0; i < n; ++i) {
        float m[9];
        for (int k = 0; k < 9; ++k) m[k] = M[9 * i + k];
        v3f p0, p1, p2;
        polar3(m, p0, p1, p2);
        float *q = Q + 9 * i;
        q[0] = p0.x; q[1] = p0.y; q[2] = p0.z; q[3] = p1.x; q[4] = p1.y; q[5] = p1.z; q[6] = p2.x; q[7] = p2.y; q[8] = p2.z;
    }
}
// gM [n][9] = dL/dM for dL/dQ = gQ [n][9]: polar3, then polar3_backward on its result, as cond9_backward runs them
void hp_polar3_backward(const float *M, const float *gQ, float *gM, int n) {
    for (int i = 0; i < n; ++i) {
        float m[9], g[9], o[9];
        for (int k = 0; k < 9; ++k) { m[k] = M[9 * i + k]; g[k] = gQ[9 * i + k]; }
        v3f p0, p1, p2;
        polar3(m, p0, p1, p2);
        polar3_backward(m, p0, p1, p2, g, o);
        for (int k = 0; k < 9; ++k) gM[9 * i + k] = o[k];
    }
}
}
