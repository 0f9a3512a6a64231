// lane_probe.hip -- runs ONE lane primitive per launch on the device (tests/lane_math/lane_probe_ops.hpp has the wrappers and the
// table).  A stand-alone program: tests/test_gpu_lane_probe.py starts it as a fresh child process and never loads it into Python.
// Built three times, with the flags of the product's three translation-unit recipes (tests/lane_probe_common.py reads them from
// ik_amd/csrc/Makefile and ik_amd/csrc/rtc.cpp).
//
//   lane_probe --list                                   the table: one line "name n_in n_out" per operation
//   lane_probe <op> <n> <in.f64> <out.f64> [<op> <n> <in> <out> ...]     one launch per group of four arguments, in order
//
// Files are raw little-endian doubles, structure-of-arrays: [n_in][n] in, [n_out][n] out.  One __global__ per operation, 64-thread
// workgroups as the product launches; lane i reads and writes column i only and returns at i >= n (the table routine stages its LDS
// table with the whole wave first, as the hot kernels do).  The device buffers are padded to whole workgroups plus one, the output is
// filled with NaNs before the launch, and the columns from n on must come back untouched: exit status 3 otherwise.  Any HIP error
// is printed and ends the program with status 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lane_probe_ops.hpp"

namespace {

using ikdev::HotTableLds;   // (IKD_HOT_LUT_DECLARE names them unqualified)
using ikdev::SinCosPair;

#define HIP_CHECK(expr)                                                                                          \
    do {                                                                                                         \
        const hipError_t err_ = (expr);                                                                          \
        if (err_ != hipSuccess) {                                                                                \
            std::fprintf(stderr, "lane_probe: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(err_), __FILE__, __LINE__); \
            std::exit(1);                                                                                        \
        }                                                                                                        \
    } while (0)

#define LANE_PROBE_KERNEL(name, ni, no)                                                                          \
    __global__ __launch_bounds__(64) void k_##name(long n, long stride, const double *in, double *out) {         \
        const long i = static_cast<long>(blockIdx.x) * 64 + threadIdx.x;                                         \
        if (i >= n) return;                                                                                      \
        double a[ni], o[no];                                                                                     \
        _Pragma("unroll") for (int k = 0; k < ni; ++k) a[k] = in[k * stride + i];                                \
        lane_probe::op_##name(a, o);                                                                             \
        _Pragma("unroll") for (int k = 0; k < no; ++k) out[k * stride + i] = o[k];                               \
    }                                                                                                            \
    void launch_##name(long n, long stride, const double *in, double *out) {                                     \
        k_##name<<<dim3(static_cast<unsigned>((n + 63) / 64)), dim3(64)>>>(n, stride, in, out);                  \
    }
LANE_PROBE_OPS(LANE_PROBE_KERNEL)

#define LANE_PROBE_LUT_KERNEL(name, nj)                                                                          \
    __global__ __launch_bounds__(64) void k_##name(long n, long stride, const double *in, double *out) {         \
        IKD_HOT_LUT_DECLARE(tv);                                                                                 \
        const auto stage = ikdev::hot_lut_issue(tv);                                                             \
        ikdev::hot_lut_commit(tv, stage);                                                                        \
        const long i = static_cast<long>(blockIdx.x) * 64 + threadIdx.x;                                         \
        if (i >= n) return;                                                                                      \
        double a[nj], o[4 * nj];                                                                                 \
        _Pragma("unroll") for (int k = 0; k < nj; ++k) a[k] = in[k * stride + i];                                \
        lane_probe::op_sincos_lut<nj>(tv, a, o);                                                                 \
        _Pragma("unroll") for (int k = 0; k < 4 * nj; ++k) out[k * stride + i] = o[k];                           \
    }                                                                                                            \
    void launch_##name(long n, long stride, const double *in, double *out) {                                     \
        k_##name<<<dim3(static_cast<unsigned>((n + 63) / 64)), dim3(64)>>>(n, stride, in, out);                  \
    }
LANE_PROBE_LUT_OPS(LANE_PROBE_LUT_KERNEL)

typedef void (*Launch)(long, long, const double *, double *);
#define LANE_PROBE_LAUNCH(name, a, b) launch_##name,
#define LANE_PROBE_LUT_LAUNCH(name, nj) launch_##name,
const Launch kLaunch[] = {LANE_PROBE_OPS(LANE_PROBE_LAUNCH) LANE_PROBE_LUT_OPS(LANE_PROBE_LUT_LAUNCH)};
static_assert(sizeof(kLaunch) / sizeof(kLaunch[0]) == lane_probe::kNumOps, "one launcher per row of the table");

int run_one(const char *op, const char *n_text, const char *in_path, const char *out_path) {
    int which = -1;
    for (int k = 0; k < lane_probe::kNumOps; ++k)
        if (std::strcmp(op, lane_probe::kOps[k].name) == 0) which = k;
    if (which < 0) {
        std::fprintf(stderr, "lane_probe: no operation '%s'\n", op);
        return 2;
    }
    const long n = std::atol(n_text);
    if (n < 1 || n > (1L << 22)) {
        std::fprintf(stderr, "lane_probe: n = %ld out of range\n", n);
        return 2;
    }
    const int ni = lane_probe::kOps[which].n_in, no = lane_probe::kOps[which].n_out;
    const long stride = (n + 63) / 64 * 64 + 64;   // every launched lane has a column of its own, read or written or not
    std::vector<double> hin(static_cast<size_t>(ni) * stride, 0.0), hout(static_cast<size_t>(no) * stride);
    std::FILE *f = std::fopen(in_path, "rb");
    if (!f) {
        std::fprintf(stderr, "lane_probe: cannot open %s\n", in_path);
        return 2;
    }
    for (int k = 0; k < ni; ++k)
        if (std::fread(hin.data() + static_cast<size_t>(k) * stride, sizeof(double), n, f) != static_cast<size_t>(n)) {
            std::fprintf(stderr, "lane_probe: %s is shorter than [%d][%ld] doubles\n", in_path, ni, n);
            std::fclose(f);
            return 2;
        }
    std::fclose(f);
    double *din = nullptr, *dout = nullptr;
    HIP_CHECK(hipMalloc(&din, hin.size() * sizeof(double)));
    HIP_CHECK(hipMalloc(&dout, hout.size() * sizeof(double)));
    HIP_CHECK(hipMemcpy(din, hin.data(), hin.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(dout, 0xff, hout.size() * sizeof(double)));   // all bits set: a NaN no arithmetic produces
    kLaunch[which](n, stride, din, dout);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(hout.data(), dout, hout.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(hipFree(din));
    HIP_CHECK(hipFree(dout));
    for (int k = 0; k < no; ++k)
        for (long i = n; i < stride; ++i) {
            unsigned long long bits;
            std::memcpy(&bits, &hout[static_cast<size_t>(k) * stride + i], 8);
            if (bits != ~0ull) {
                std::fprintf(stderr, "lane_probe: %s wrote column %ld of output %d, past n = %ld\n", op, i, k, n);
                return 3;
            }
        }
    f = std::fopen(out_path, "wb");
    if (!f) {
        std::fprintf(stderr, "lane_probe: cannot write %s\n", out_path);
        return 2;
    }
    for (int k = 0; k < no; ++k)
        if (std::fwrite(hout.data() + static_cast<size_t>(k) * stride, sizeof(double), n, f) != static_cast<size_t>(n)) {
            std::fprintf(stderr, "lane_probe: short write to %s\n", out_path);
            return 2;
        }
    if (std::fclose(f) != 0) return 2;
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && std::strcmp(argv[1], "--list") == 0) {
        for (int k = 0; k < lane_probe::kNumOps; ++k)
            std::printf("%s %d %d\n", lane_probe::kOps[k].name, lane_probe::kOps[k].n_in, lane_probe::kOps[k].n_out);
        return 0;
    }
    if (argc < 5 || (argc - 1) % 4 != 0) {
        std::fprintf(stderr, "usage: lane_probe --list | lane_probe <op> <n> <in.f64> <out.f64> [...]\n");
        return 2;
    }
    for (int a = 1; a + 3 < argc; a += 4) {
        const int rc = run_one(argv[a], argv[a + 1], argv[a + 2], argv[a + 3]);
        if (rc != 0) return rc;
    }
    return 0;
}
