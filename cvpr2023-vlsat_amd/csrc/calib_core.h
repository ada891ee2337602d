// The bin rule of the score histograms (include/vlsat_calib.h), for the kernels of calibration.hip and for the host
// (tests/calib_host_check.cpp): one function, so that both sides cannot drift apart.
//   bins is a power of two in 16..4096, so p * bins is exact in fp32 for every finite p >= 0 that does not overflow:
//   floor(p * bins) >= k  <=>  p >= k / bins.  The histogram therefore holds the decode's `p >= threshold` for every threshold
//   k / bins at once, exactly.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VLSAT_CALIB_HD __host__ __device__ __forceinline__
#else
#define VLSAT_CALIB_HD inline
#endif

namespace vlsat {

constexpr int CALIB_MIN_BINS = 16, CALIB_MAX_BINS = 4096;

VLSAT_CALIB_HD bool calib_bins_ok(int bins) { return bins >= CALIB_MIN_BINS && bins <= CALIB_MAX_BINS && (bins & (bins - 1)) == 0; }

// the column of a cell: 0..bins-1 for an eligible cell with p >= 0 (-0 included; +inf and p > 1 in the last bin), otherwise the
// "never asserted" column `bins` (NaN, p < 0, not eligible).  The comparison with bins comes before the conversion: no float
// outside the int range is ever converted.
VLSAT_CALIB_HD int calib_bin(float p, int bins, bool eligible) {
    if (!(eligible && p >= 0.f)) return bins;
    const float x = p * (float)bins;               // one fp32 multiply by a power of two
    return x >= (float)bins ? bins - 1 : (int)x;   // (x >= 0: truncation is floor)
}

}  // namespace vlsat
