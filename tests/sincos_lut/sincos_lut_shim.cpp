// sincos_lut_shim.cpp -- TEST HARNESS ONLY.  dsincos_lut (ik_amd/csrc/device/lane_math.hpp) on the CPU, statement for statement
// what the hot chain kernels run, on the literals of device/sincos_lut_table.hpp.  Compiled by tests/test_sincos_lut_host.py with g++
// into its own shared object; libikgpu.so neither contains nor calls it.
#include <cstdint>

#include "device/lane_math.hpp"

extern "C" {

int sincos_lut_size(void) { return IKD_SINCOS_LUT_SIZE; }

// the table as the host build reads it: 2 * size doubles, {sin, cos} interleaved
void sincos_lut_table(double *out) {
    for (int k = 0; k < 2 * IKD_SINCOS_LUT_SIZE; ++k) out[k] = ikdev::kSinCosLutHost[k];
}

// the step of the table as the reduction takes it (one word of 2 pi over the size)
double sincos_lut_step(void) { return ikdev::kSinCosLutStepHi; }

// s, c: dsincos_lut(x); idx, r: what its reduction found
void sincos_lut_run(int64_t n, const double *x, double *s, double *c, int *idx, double *r) {
    for (int64_t i = 0; i < n; ++i) {
        ikdev::dsincos_lut(x[i], s[i], c[i]);
        ikdev::dsincos_lut_reduce(x[i], r[i], idx[i]);
    }
}

}  // extern "C"
