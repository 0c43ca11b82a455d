// The argument checks of an (R, T) matrix of float or double traces with row stride ld, as the entry points of deconv.hip and
// trace_dyn.hip take one: the one definition of each code and message.  Host only.  In pieces, because the entry points do not
// check in the same order, and the code an argument vector returns is part of their interface.
#pragma once
#include "common.h"

// the pointer, the element type, the counts and the stride
static inline int dc_trace_check_counts(const char* who, const void* y, int is_f64, long ld, int R, long T) {
  DC_REQUIRE(y, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(is_f64 == 0 || is_f64 == 1, DC_EINVAL, "%s: is_f64 = %d is neither 0 nor 1", who, is_f64);
  DC_REQUIRE(R >= 0 && T >= 0, DC_EINVAL, "%s: negative count (R %d, T %ld)", who, R, T);
  DC_REQUIRE(ld >= T, DC_EINVAL, "%s: ld = %ld is below T = %ld", who, ld, T);
  return DC_OK;
}

// y holds whole elements; the caller words the refusal ("%s: misaligned buffer") together with its other buffers
static inline bool dc_trace_aligned(const void* y, int is_f64) { return dc_aligned(is_f64 ? 7 : 3, y); }

// the frames of a trace and the samples of the matrix
static inline int dc_trace_check_limits(const char* who, int R, long T) {
  DC_REQUIRE(T <= DC_TRACE_DECONV_MAX_FRAMES, DC_EUNSUP, "%s: T = %ld is over the limit of %ld frames", who, T, DC_TRACE_DECONV_MAX_FRAMES);
  DC_REQUIRE((long)R * T <= DC_TRACE_DECONV_MAX_SAMPLES, DC_EUNSUP, "%s: R * T = %ld is over the limit of %ld samples", who, (long)R * T,
             DC_TRACE_DECONV_MAX_SAMPLES);
  return DC_OK;
}
