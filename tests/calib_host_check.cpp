// Host-only check of csrc/calib_core.h (the bin rule of the score histograms): prints the column of every value at which the rule can
// go wrong -- every edge k / bins, its two fp32 neighbours, 0.0, -0.0, 1.0, a denormal, a negative, 1.5, +inf, NaN, the largest finite
// float -- for bins = 16, 1024, 4096, eligible and not, as "bins:bits:eligible -> column".  tests/test_calibration_cpu.py builds it
// with ASan + UBSan (a float outside the int range converted to int is what UBSan would catch) and compares the columns with the
// PyTorch restatement.  g++ only: no HIP header, no library, no device.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "calib_core.h"
#include "select_core.h"

int main() {
    using namespace vlsat;
    for (int bins : {16, 1024, 4096}) {
        if (!calib_bins_ok(bins) || calib_bins_ok(bins + 1) || calib_bins_ok(bins * 3)) return 1;
        std::vector<float> v;
        for (int k = 0; k < bins; ++k) {
            const float edge = (float)k / (float)bins;
            v.push_back(edge);
            v.push_back(std::nextafterf(edge, 2.f));
            v.push_back(std::nextafterf(edge, -1.f));
        }
        for (float x : {0.f, -0.f, 1.f, 1e-42f, -0.3f, 1.5f, std::numeric_limits<float>::infinity(), std::nanf(""),
                        std::numeric_limits<float>::max(), -std::numeric_limits<float>::infinity()})
            v.push_back(x);
        for (float x : v)
            for (int eligible = 0; eligible < 2; ++eligible)
                std::printf("%d:%08x:%d -> %d\n", bins, (unsigned)f32_bits(x), eligible, calib_bin(x, bins, eligible != 0));
    }
    if (calib_bins_ok(8) || calib_bins_ok(8192) || calib_bins_ok(0) || calib_bins_ok(-16)) return 1;
    return 0;
}
