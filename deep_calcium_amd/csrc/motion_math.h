// The tie rule of rigid motion correction (motion.hip, dc_motion_pick): among the candidate shifts (dy, dx) of one frame the picked
// one minimises the tuple (score, dy^2 + dx^2, dy, dx) lexicographically -- the smallest sum of squared differences, then the
// smallest displacement, then the smaller dy, then the smaller dx.  Two candidates with different (dy, dx) never compare equal, so
// the minimum is unique and does not depend on the order in which candidates are compared.  Plain C++ on purpose -- no HIP header,
// no intrinsic -- so the same inline functions compile for the device and into a stand-alone host program
// (tests/native/motion_math_check.cpp, run under the address / undefined-behaviour sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_MOTION_HD __host__ __device__ inline
#else
#define DC_MOTION_HD inline
#endif

struct DcShiftCand {
  int64_t score;
  int dy, dx;
};

// |dy|, |dx| <= 16 in dc_motion_pick; any int32 pair is ordered correctly (each square is <= 2^62, their sum fits 64 unsigned bits)
DC_MOTION_HD uint64_t dc_motion_dist2(int dy, int dx) { return (uint64_t)((int64_t)dy * dy) + (uint64_t)((int64_t)dx * dx); }

// true when a comes strictly before b in the order above
DC_MOTION_HD bool dc_motion_before(const DcShiftCand a, const DcShiftCand b) {
  if (a.score != b.score) return a.score < b.score;
  const uint64_t da = dc_motion_dist2(a.dy, a.dx), db = dc_motion_dist2(b.dy, b.dx);
  if (da != db) return da < db;
  if (a.dy != b.dy) return a.dy < b.dy;
  return a.dx < b.dx;
}

// candidate i of the [2S+1][2S+1] score table of one frame (dy the slow axis, index dy + S)
DC_MOTION_HD DcShiftCand dc_motion_cand(const int64_t* scores, int S, int i) {
  const int nd = 2 * S + 1;
  DcShiftCand c;
  c.score = scores[i];
  c.dy = i / nd - S;
  c.dx = i % nd - S;
  return c;
}

// the picked shift of one frame: a serial scan (what the kernel's strided scan + wave reduction must equal)
DC_MOTION_HD DcShiftCand dc_motion_pick_serial(const int64_t* scores, int S) {
  const int nd = 2 * S + 1;
  DcShiftCand best = dc_motion_cand(scores, S, 0);
  for (int i = 1; i < nd * nd; ++i) {
    const DcShiftCand c = dc_motion_cand(scores, S, i);
    if (dc_motion_before(c, best)) best = c;
  }
  return best;
}
