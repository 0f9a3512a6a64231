// lane_math_shim.cpp -- TEST HARNESS ONLY.  Exposes two functions of ik_amd/csrc/device/lane_math.hpp on the CPU: the 6 x 6 solve of
// the DLS step (ldlt_solve<6>) and the log6 / Jlog6 front end of the hot chain program (log6_and_jlog6_hot), so that
// tests/test_ldlt_solve_host.py and tests/test_log6_scalars_host.py can hold them to extended-precision and oracle results in the
// GPU-less build container.  Compiled by those tests with g++ into its own shared object; libikgpu.so neither contains nor calls it.
#include <cstdint>

#include "device/lane_math.hpp"

extern "C" {

// n systems G x = b: G [n][36] row-major (the lower triangle is read), b [n][6]; out x [n][6].
void lane_math_solve6(int64_t n, const double *G, const double *b, double *x) {
    for (int64_t s = 0; s < n; ++s) {
        double g[36], rhs[6], sol[6];
        for (int k = 0; k < 36; ++k) g[k] = G[36 * s + k];
        for (int k = 0; k < 6; ++k) rhs[k] = b[6 * s + k];
        ikdev::ldlt_solve<6>(g, rhs, sol);
        for (int k = 0; k < 6; ++k) x[6 * s + k] = sol[k];
    }
}

// n placements fMt = (Re [n][9] row-major, pe [n][3]); out e [n][6] = log6(fMt), A [n][9] and C [n][9] with
// Jlog6(tMf) = [A  C A; 0  A] (the form the hot chain program takes: WITH_BM = false), Bm [n][9] = C A as the other form returns it.
void lane_math_log6(int64_t n, const double *Re, const double *pe, double *e, double *A, double *Cm, double *Bm) {
    for (int64_t s = 0; s < n; ++s) {
        double R[9], p[3], Cout[9];
        for (int k = 0; k < 9; ++k) R[k] = Re[9 * s + k];
        for (int k = 0; k < 3; ++k) p[k] = pe[3 * s + k];
        ikdev::LogAndJlog o, o2;
        ikdev::log6_and_jlog6_hot<false, true>(R, p, o, &Cout);
        ikdev::log6_and_jlog6_hot<true, true>(R, p, o2);
        for (int k = 0; k < 6; ++k) e[6 * s + k] = o.e[k];
        for (int k = 0; k < 9; ++k) { A[9 * s + k] = o.A[k]; Cm[9 * s + k] = Cout[k]; Bm[9 * s + k] = o2.Bm[k]; }
    }
}

}  // extern "C"
