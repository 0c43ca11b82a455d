// The two pure helpers of the dF/F baseline (include/dcunet.h, "dF/F traces"; csrc/dff.hip): the rank a percentile names in a
// window of n samples, and the midpoint of two int64 bounds that may lie 2^63 - 2 apart.  Plain C++ like series_math.h, so the
// same inline functions compile for the device and into a stand-alone host program (tests/native/dff_math_check.cpp, run under
// the address / undefined-behaviour sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_DFF_HD __host__ __device__ inline
#else
#define DC_DFF_HD inline
#endif

// k = (q * (n - 1)) / 100 in integers: the 0-based rank of integer percentile q in [0, 100] among n >= 1 samples.  (Not numpy's
// float rule: floor(0.29 * 100) is 28, this gives 29.)  n <= 4095 here; the product is formed in int64 anyway.
DC_DFF_HD int dc_dff_rank(int q, int n) { return (int)(((int64_t)q * (int64_t)(n - 1)) / 100); }

// floor((lo + hi) / 2) for lo <= hi without forming lo + hi or hi - lo in int64: the distance is taken in uint64, where it is
// exact for every pair (at most 2^64 - 1), halved, and added back; lo + half <= hi, so the sum cannot overflow either.
DC_DFF_HD int64_t dc_dff_midpoint(int64_t lo, int64_t hi) { return lo + (int64_t)(((uint64_t)hi - (uint64_t)lo) >> 1); }
