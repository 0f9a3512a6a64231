// lane_probe_host.cpp -- the operations of tests/lane_math/lane_probe_ops.hpp under g++ (the HOST arms of lane_math.hpp), behind
// the same table as the device program tests/lane_math/lane_probe.hip.  Structure-of-arrays: in [n_in][n], out [n_out][n].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "lane_probe_ops.hpp"

namespace {

#define LANE_PROBE_HOST(name, ni, no)                                            \
    void run_##name(int64_t n, const double *in, double *out) {                 \
        for (int64_t i = 0; i < n; ++i) {                                        \
            double a[ni], o[no];                                                 \
            for (int k = 0; k < ni; ++k) a[k] = in[k * n + i];                   \
            lane_probe::op_##name(a, o);                                         \
            for (int k = 0; k < no; ++k) out[k * n + i] = o[k];                  \
        }                                                                        \
    }
LANE_PROBE_OPS(LANE_PROBE_HOST)

#define LANE_PROBE_LUT_HOST(name, nj)                                            \
    void run_##name(int64_t n, const double *in, double *out) {                 \
        const ikdev::HotTable tv{};                                              \
        for (int64_t i = 0; i < n; ++i) {                                        \
            double a[nj], o[4 * nj];                                             \
            for (int k = 0; k < nj; ++k) a[k] = in[k * n + i];                   \
            lane_probe::op_sincos_lut<nj>(tv, a, o);                             \
            for (int k = 0; k < 4 * nj; ++k) out[k * n + i] = o[k];              \
        }                                                                        \
    }
LANE_PROBE_LUT_OPS(LANE_PROBE_LUT_HOST)

typedef void (*Run)(int64_t, const double *, double *);
#define LANE_PROBE_RUN(name, a, b) run_##name,
#define LANE_PROBE_LUT_RUN(name, nj) run_##name,
const Run kRun[] = {LANE_PROBE_OPS(LANE_PROBE_RUN) LANE_PROBE_LUT_OPS(LANE_PROBE_LUT_RUN)};
static_assert(sizeof(kRun) / sizeof(kRun[0]) == lane_probe::kNumOps, "one runner per row of the table");

}  // namespace

// 0, or -1 when the table has no such operation
extern "C" int run(const char *op, int64_t n, const double *in, double *out) {
    for (int k = 0; k < lane_probe::kNumOps; ++k)
        if (std::strcmp(op, lane_probe::kOps[k].name) == 0) {
            kRun[k](n, in, out);
            return 0;
        }
    return -1;
}

// the text `lane_probe --list` prints
extern "C" const char *list() {
    static std::string text;
    text.clear();
    for (int k = 0; k < lane_probe::kNumOps; ++k) {
        char line[96];
        std::snprintf(line, sizeof line, "%s %d %d\n", lane_probe::kOps[k].name, lane_probe::kOps[k].n_in, lane_probe::kOps[k].n_out);
        text += line;
    }
    return text.c_str();
}
