// Rigid motion correction on the device: every frame of a recording (T, H, W) of 16-bit frames is compared with a template at every
// whole-pixel shift (dy, dx) in [-S, S]^2 (dc_motion_ssd: the sum of squared differences over the template's interior), the best
// shift is picked under a total order (dc_motion_pick, motion_math.h) and the frame is moved (dc_motion_apply).  Integer arithmetic
// only: a score is the exact int64 sum, so the chunking of a recording never changes a bit and numpy is an exact oracle.
// Sign convention: out[y][x] = frame[y + dy][x + dx]; a frame cut from a scene at offset (+a, +b) relative to the template is found
// as (dy, dx) = (-a, -b).
// Piecewise-rigid on top of it: per block of a By x Bx grid the rigid shift plus a residual within +-D (dc_motion_block_ssd,
// dc_motion_block_pick), blended into one whole-pixel shift per pixel (dc_motion_warp).
// Sub-pixel on top of both: every pick refined to a sixteenth of a pixel from the scores next to it (dc_motion_refine,
// dc_motion_block_refine) and the frames interpolated bilinearly with integer weights (dc_motion_apply_sub, dc_motion_warp_sub).
// Wide search beside the exhaustive one, for shifts up to 128: frames and template binned c x c (dc_motion_bin), the coarse pick by
// dc_motion_ssd + dc_motion_pick on the binned pair, then the full-resolution scores within +-c of c times that pick
// (dc_motion_ssd_around) and the pick over total shifts (dc_motion_pick_around).
// In front of all of it, the bidirectional scan-phase correction: the odd lines of every frame scored against their even neighbours
// at every horizontal offset within +-P (dc_bidi_scores: bidi_scores_kernel, built from the same tile pieces) and moved by the one
// offset the host picks for the recording (dc_bidi_apply: bidi_apply_kernel, the whole-pixel mover with a shift per row parity).
// Every piece exists once.  The exhaustive entry points are the window ones at centre 0: motion_ssd_kernel scores the shifts within
// +-D of a centre per frame (dc_motion_ssd: D = S, no centres) and motion_pick_kernel picks over centre + residual.  The two score
// kernels (frame-wide tiles, tiles of a block) are built from the same four tile_* pieces around ssd_rows; the movers
// motion_apply_kernel<SUB> and motion_warp_kernel<SUB> end in the same put8 / put1 (whole-pixel move or interpolation).
#include "common.h"
#include "motion_math.h"

namespace {

const int kThreads = 256;
const int kWave = 64;
const int kWaves = kThreads / kWave;
const int kPix = 8;                    // consecutive interior pixels of one row a lane owns
const int kTileW = kWave * kPix;       // interior columns of one workgroup's tile: 512
const int kZeroBlocks = 1024;

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__global__ __launch_bounds__(kThreads) void motion_zero_kernel(unsigned long long* __restrict__ scores, long n) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) scores[i] = 0;
}

// elements of one LDS row of the frame tile: the tile's 512 interior columns + the 2S halo, rounded up so that every row
// starts 16-byte aligned (the lanes read their windows as 16-byte pieces)
__host__ __device__ inline int ssd_stride(int S) { return kTileW + ((2 * S + 7) & ~7); }

// The rows of one dy for one wave: R template rows (registers) against R frame rows (LDS), all nd shifts along x.
//   acc[k] += (t[j][p] - f[j + m][p + k])^2,  k = dx + S.
// Every term is < 2^32 (|difference| <= 65535) and a lane adds at most R * kPix <= 64 of them per (m, k): < 2^38, kept in 64 bits
// from the first add on -- there is no 32-bit partial sum anywhere.  RAG: some lane of the wave owns fewer than kPix interior
// pixels (the tile's last, ragged lane); its other differences are masked to 0.
template <int SMAX, int R, bool RAG>
__device__ __forceinline__ void ssd_rows(const uint16_t* __restrict__ ft, int stride, int S, int nd, int nr, int row0, int lane,
                                        const unsigned (&t2)[R][kPix / 2], const unsigned (&mk)[kPix],
                                        unsigned long long (&acc)[2 * SMAX + 1]) {
  constexpr int NK = 2 * SMAX + 1, FW = kPix + 2 * SMAX;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    if (j < nr) {                                        // wave-uniform in motion_ssd_kernel; per 16 lanes in the block kernel
    const uint4* src = reinterpret_cast<const uint4*>(ft + (long)(row0 + j) * stride + kPix * lane);
    unsigned w[FW / 2];
#pragma unroll
    for (int q = 0; q < FW / 8; ++q) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (q * 8 < kPix + 2 * S) v = src[q];              // wave-uniform: the window is kPix + 2S values long
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
    int fw[FW], t[kPix];
#pragma unroll
    for (int i = 0; i < FW; ++i) fw[i] = (int)((w[i / 2] >> (16 * (i & 1))) & 0xffffu);
#pragma unroll
    for (int p = 0; p < kPix; ++p) t[p] = (int)((t2[j][p / 2] >> (16 * (p & 1))) & 0xffffu);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if (k < nd) {                                      // wave-uniform
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
          unsigned d = (unsigned)(t[p] - fw[p + k]);     // 17 bits and a sign
          if (RAG) d &= mk[p];
          acc[k] += (unsigned long long)(d * d);         // unsigned: d^2 < 2^32 is exact modulo 2^32 (a signed product would overflow)
        }
      }
    }
    }
  }
}

// ---- the pieces of one score tile, shared by motion_ssd_kernel and motion_block_ssd_kernel ----------------------------------------
// LDS of a score launch: the frame tile of th interior rows with its D-wide halo, then the (2D+1)^2 totals of the workgroup
__host__ __device__ inline size_t tile_bytes(int th, int stride, int D) { return (size_t)(th + 2 * D) * stride * sizeof(uint16_t); }
inline int ssd_lds(int th, int stride, int D) { return (int)tile_bytes(th, stride, D) + (2 * D + 1) * (2 * D + 1) * (int)sizeof(long long); }

// the mask of a lane that owns np of its kPix pixels; true where some lane of the wave is ragged (0 < np < kPix)
__device__ __forceinline__ bool tile_mask(int np, unsigned (&mk)[kPix]) {
#pragma unroll
  for (int p = 0; p < kPix; ++p) mk[p] = p < np ? 0xffffffffu : 0u;
  return __ballot(np > 0 && np < kPix) != 0;
}

// the lane's template pixels, nr rows of np from t0 on (the sign bit flipped for int16), packed in pairs; 0 beyond nr and np
template <int R>
__device__ __forceinline__ void tile_tmpl(const uint16_t* __restrict__ t0, int W, int nr, int np, unsigned flip, unsigned (&t2)[R][kPix / 2]) {
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const uint16_t* trow = t0 + (long)j * W;
#pragma unroll
    for (int q = 0; q < kPix / 2; ++q) {
      const unsigned lo = (j < nr && 2 * q < np) ? (trow[2 * q] ^ flip) : 0u;
      const unsigned hi = (j < nr && 2 * q + 1 < np) ? (trow[2 * q + 1] ^ flip) : 0u;
      t2[j][q] = lo | (hi << 16);
    }
  }
}

// the frame window of rows x cols values whose LDS (0, 0) is frame (oy, ox), values with the sign bit flipped for int16 (both
// operands move by 32768, the difference does not); 0 outside the frame, which the callers' origins make unreachable for a pixel
// that counts: what is not found inside the frame is read by lanes without pixels only, or masked
__device__ __forceinline__ void tile_stage(uint16_t* __restrict__ ft, int stride, const uint16_t* __restrict__ fr, int H, int W, int oy, int ox,
                                           int rows, int cols, unsigned flip, int wave, int lane) {
  for (int r = wave; r < rows; r += kWaves) {
    const int gy = oy + r;
    for (int c = lane; c < cols; c += kWave) {
      const int gx = ox + c;
      ft[r * stride + c] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? (uint16_t)(fr[(long)gy * W + gx] ^ flip) : (uint16_t)0;
    }
  }
}

// One staged window scored at all nd^2 residuals: per ey the lane (column col of its row group, rows row0 ..) keeps one 64-bit sum
// per ex, the wave adds them by shuffles -- EVERY lane of the wave takes part, whether it owns pixels or not --, lane k takes the
// total of ex = k - D and adds it to the workgroup's totals sc in LDS (an integer atomic).  sc is the caller's to zero and flush.
template <int RMAX, int R>
__device__ __forceinline__ void tile_score(const uint16_t* __restrict__ ft, int stride, int D, int nr, int np, bool ragged, int row0, int col,
                                           int lane, const unsigned (&t2)[R][kPix / 2], const unsigned (&mk)[kPix],
                                           unsigned long long* __restrict__ sc) {
  constexpr int NK = 2 * RMAX + 1;
  const int nd = 2 * D + 1;
  for (int m = 0; m < nd; ++m) {
    unsigned long long acc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] = 0;
    if (np > 0 && nr > 0) {
      if (ragged) ssd_rows<RMAX, R, true>(ft, stride, D, nd, nr, row0 + m, col, t2, mk, acc);
      else ssd_rows<RMAX, R, false>(ft, stride, D, nd, nr, row0 + m, col, t2, mk, acc);
    }
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if (k < nd) {
        const unsigned long long s = wave_sum64(acc[k]);
        if (lane == k) mine = s;
      }
    }
    if (lane < nd) atomicAdd(&sc[m * nd + lane], mine);
  }
}

// The scores of the (2D+1)^2 shifts within +-D of a centre (cy, cx) per frame, summed over the radius-S interior.  One workgroup
// per tile of that INTERIOR (kWaves * R rows x 512 columns) and frame.  The frame tile with its D-wide halo is staged in LDS once
// and reused for all nd^2 shifts; a lane owns kPix consecutive interior pixels of R rows, whose template values stay in registers.
// The workgroup's nd^2 totals meet in LDS (tile_score) before ONE 64-bit atomic per shift and workgroup goes to memory (integer
// addition: the order does not matter, the result is bit-reproducible).
// centres == nullptr (dc_motion_ssd, with D = S): centre 0, the exhaustive table; LDS (0, 0) is then frame (j0, i0).  Otherwise
// (dc_motion_ssd_around) the centre is clamp(mult * centres[f], S - D), formed HERE: LDS (0, 0) is frame (S + j0 + cy - D,
// S + i0 + cx - D), and because |cy| <= S - D the window's first row is >= 0 and its last, S + (H - 2S - 1) + cy + D, is
// <= H - 1, likewise the columns -- whatever the table holds, nothing outside the frame is read for a pixel that counts.
template <int RMAX, int R>
__global__ __launch_bounds__(kThreads) void motion_ssd_kernel(const uint16_t* __restrict__ frames, unsigned flip, int tc,
                                                             const uint16_t* __restrict__ tmpl, int H, int W, int S, int D,
                                                             const int* __restrict__ centres, int mult,
                                                             unsigned long long* __restrict__ scores, int tilesX) {
  constexpr int TH = kWaves * R;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nd = 2 * D + 1, stride = ssd_stride(D), rows = TH + 2 * D;
  uint16_t* ft = reinterpret_cast<uint16_t*>(smem);
  unsigned long long* sc = reinterpret_cast<unsigned long long*>(smem + tile_bytes(TH, stride, D));
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int tx = blockIdx.x % tilesX, ty = blockIdx.x / tilesX;
  const int i0 = tx * kTileW, j0 = ty * TH;              // the tile's first pixel, counted from the interior's corner (S, S)
  const int IW = W - 2 * S, IH = H - 2 * S;
  const int left = IW - i0 - kPix * lane, down = IH - j0 - wave * R;
  const int np = left < 0 ? 0 : (left < kPix ? left : kPix);      // interior pixels of this lane
  const int nr = down < 0 ? 0 : (down < R ? down : R);            // interior rows of this wave
  unsigned mk[kPix], t2[R][kPix / 2];
  const bool ragged = tile_mask(np, mk);
  tile_tmpl<R>(tmpl + (long)(S + j0 + wave * R) * W + S + i0 + kPix * lane, W, nr, np, flip, t2);
  for (int f = blockIdx.y; f < tc; f += gridDim.y) {
    const int cy = centres ? dc_motion_centre(mult, centres[2 * f], S - D) : 0;
    const int cx = centres ? dc_motion_centre(mult, centres[2 * f + 1], S - D) : 0;
    __syncthreads();                                     // the readers of the previous frame's tile and totals are done
    tile_stage(ft, stride, frames + (long)f * H * W, H, W, S + j0 + cy - D, S + i0 + cx - D, rows, stride, flip, wave, lane);
    for (int i = threadIdx.x; i < nd * nd; i += kThreads) sc[i] = 0;
    __syncthreads();
    if (nr > 0) tile_score<RMAX, R>(ft, stride, D, nr, np, ragged, wave * R, lane, lane, t2, mk, sc);        // wave-uniform
    __syncthreads();
    unsigned long long* dst = scores + (long)f * nd * nd;
    for (int i = threadIdx.x; i < nd * nd; i += kThreads) {
      const unsigned long long v = sc[i];
      if (v) atomicAdd(dst + i, v);
    }
  }
}

// One wave per score table: every lane scans the candidates lane, lane + 64, ... and the wave folds its 64 partial minima; the
// order of motion_math.h is total, so the result is the unique minimum whatever the order of the comparisons.  Every lane returns it.
// (cy, cx): the centre of a window table (motion_pick_kernel: the candidates are ordered as total shifts); the block pick orders
// residuals and leaves it at (0, 0).
__device__ __forceinline__ DcShiftCand pick_wave(const int64_t* __restrict__ sc, int S, int lane, int cy = 0, int cx = 0) {
  const int n = (2 * S + 1) * (2 * S + 1);
  DcShiftCand b = dc_motion_cand_around(sc, S, lane < n ? lane : 0, cy, cx);
  for (int i = lane + kWave; i < n; i += kWave) {
    const DcShiftCand c = dc_motion_cand_around(sc, S, i, cy, cx);
    if (dc_motion_before(c, b)) b = c;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    DcShiftCand c;
    c.score = (int64_t)__shfl_xor((unsigned long long)b.score, o, kWave);
    c.dy = __shfl_xor(b.dy, o, kWave);
    c.dx = __shfl_xor(b.dx, o, kWave);
    if (dc_motion_before(c, b)) b = c;
  }
  return b;
}

// One wave per frame: the total shift centre + (ey, ex) under the order of motion_math.h over TOTAL shifts, and (fine non-null) its
// refinement within the window table at the picked residual -- 0 on an axis where the residual lies on the window's border.
// centres == nullptr (dc_motion_pick, with D = S): centre 0, the pick of an exhaustive table.
__global__ __launch_bounds__(kWave) void motion_pick_kernel(const int64_t* __restrict__ wscores, const int* __restrict__ centres, int mult,
                                                           int tc, int S, int D, int* __restrict__ shifts, int64_t* __restrict__ best,
                                                           int* __restrict__ fine) {
  const int n = (2 * D + 1) * (2 * D + 1), lane = threadIdx.x;
  for (int f = blockIdx.x; f < tc; f += gridDim.x) {
    const int cy = centres ? dc_motion_centre(mult, centres[2 * f], S - D) : 0;
    const int cx = centres ? dc_motion_centre(mult, centres[2 * f + 1], S - D) : 0;
    const int64_t* sc = wscores + (long)f * n;
    const DcShiftCand b = pick_wave(sc, D, lane, cy, cx);
    if (lane == 0) {
      shifts[2 * f] = b.dy;
      shifts[2 * f + 1] = b.dx;
      if (best) best[f] = b.score;
      if (fine) {
        const DcSubShift q = dc_motion_refine_entry(sc, D, b.dy - cy, b.dx - cx);
        fine[2 * f] = dc_motion_fine(b.dy, q.qy);
        fine[2 * f + 1] = dc_motion_fine(b.dx, q.qx);
      }
    }
  }
}

// ---- the movers' last step: 8 values of a row by one 16-byte store, or one value; whole pixels or (sub-pixel) interpolated ---------
// 8 (nine: 9) consecutive values from any 2-byte address p, out of the 4 or 5 aligned dwords that hold them, funnel-shifted:
// n[0 .. 3] = values 0 .. 7 in pairs, the low half of n[4] = value 8.  The fifth dword is read only where it holds one of the
// values asked for (an aligned dword that holds one value of the buffer lies inside the buffer's pages).
__device__ __forceinline__ void run9(const uint16_t* __restrict__ p, bool nine, unsigned (&n)[5]) {
  const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
  const unsigned* q = reinterpret_cast<const unsigned*>(addr & ~(uintptr_t)3);
  const unsigned w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
  if (addr & 2) {
    const unsigned w4 = q[4];
    n[0] = (w0 >> 16) | (w1 << 16); n[1] = (w1 >> 16) | (w2 << 16); n[2] = (w2 >> 16) | (w3 << 16); n[3] = (w3 >> 16) | (w4 << 16);
    n[4] = w4 >> 16;
  } else {
    n[0] = w0; n[1] = w1; n[2] = w2; n[3] = w3;
    n[4] = nine ? q[4] : 0u;
  }
}

// 8 output values of one row that share a shift, o 16-byte aligned: one store of the 8 source values at (sy, sx .. sx + 7) of the
// frame f (a run that starts at any 2-byte address: run9), or of fill where all 8 lie outside it.  false (nothing stored) where
// the run straddles the frame's edge.
__device__ __forceinline__ bool move8(const uint16_t* __restrict__ f, long sy, long sx, int H, int W, unsigned fill2, uint16_t* __restrict__ o) {
  uint4 v;
  if (sy < 0 || sy >= H || sx + 8 <= 0 || sx >= W) {
    v = make_uint4(fill2, fill2, fill2, fill2);
  } else if (sx >= 0 && sx + 8 <= W) {
    unsigned n[5];
    run9(f + sy * W + sx, false, n);
    v = make_uint4(n[0], n[1], n[2], n[3]);
  } else {
    return false;
  }
  *reinterpret_cast<uint4*>(o) = v;
  return true;
}

// One output value at the split fine shift: source (sy, sx) = (y + iy, x + ix), weights (fy, fx).  flip: 0x8000 for int16 (the
// interpolation commutes with adding 32768 to every tap).
__device__ __forceinline__ uint16_t sub1(const uint16_t* __restrict__ f, long sy, long sx, int fy, int fx, int H, int W, unsigned flip,
                                         unsigned fill) {
  if (sy < 0 || sx < 0 || sy + (fy > 0) >= H || sx + (fx > 0) >= W) return (uint16_t)fill;
  const uint16_t* p = f + sy * W + sx;
  const int a00 = (int)(p[0] ^ flip), a01 = fx ? (int)(p[1] ^ flip) : 0;
  const int a10 = fy ? (int)(p[W] ^ flip) : 0, a11 = (fy && fx) ? (int)(p[W + 1] ^ flip) : 0;
  return (uint16_t)((unsigned)dc_motion_interp(a00, a01, a10, a11, fy, fx) ^ flip);
}

// 8 output values of one row that share a split fine shift, o 16-byte aligned: one store of the 8 interpolations between the source
// rows sy and (fy > 0) sy + 1, columns sx .. sx + 7 and (fx > 0) sx + 8 -- or of fill where all 8 use a tap outside the frame.  The
// rows' runs start at any 2-byte address each (run9).  false (nothing stored) where the runs straddle the frame's left or right edge.
__device__ __forceinline__ bool sub8(const uint16_t* __restrict__ f, long sy, long sx, int fy, int fx, int H, int W, unsigned flip,
                                     unsigned fill2, uint16_t* __restrict__ o) {
  const int ny = fy > 0, nx = fx > 0;
  uint4 v;
  if (sy < 0 || sy + ny >= H || sx + 8 <= 0 || sx + nx >= W) {
    v = make_uint4(fill2, fill2, fill2, fill2);
  } else if (sx >= 0 && sx + 8 + nx <= W) {
    const unsigned flip2 = flip | (flip << 16);
    unsigned r0[5], r1[5] = {0u, 0u, 0u, 0u, 0u};
    run9(f + sy * W + sx, nx, r0);
    if (ny) run9(f + (sy + 1) * W + sx, nx, r1);           // uniform over the frame
    int a[9], b[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      a[i] = (int)(((r0[i / 2] ^ flip2) >> (16 * (i & 1))) & 0xffffu);
      b[i] = (int)(((r1[i / 2] ^ flip2) >> (16 * (i & 1))) & 0xffffu);
    }
    unsigned r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned lo = (unsigned)dc_motion_interp(a[2 * i], a[2 * i + 1], b[2 * i], b[2 * i + 1], fy, fx);
      const unsigned hi = (unsigned)dc_motion_interp(a[2 * i + 1], a[2 * i + 2], b[2 * i + 1], b[2 * i + 2], fy, fx);
      r[i] = (lo | (hi << 16)) ^ flip2;
    }
    v = make_uint4(r[0], r[1], r[2], r[3]);
  } else {
    return false;
  }
  *reinterpret_cast<uint4*>(o) = v;
  return true;
}

// The group of 8 at (y, x .. x + 7) / the one value at (y, x) of the output, all at the shift (s0, s1): whole pixels, or (SUB) a
// fine shift, which is split here (iy = floor(s0 / 16), weight fy = s0 - 16 iy; every fine shift the callers form fits an int32).
// put8: false where nothing was stored (move8, sub8).  flip is unused without SUB.
template <bool SUB>
__device__ __forceinline__ bool put8(const uint16_t* __restrict__ f, long y, long x, long s0, long s1, int H, int W, unsigned flip, unsigned fill,
                                     uint16_t* __restrict__ o) {
  const long sy = y + (SUB ? dc_motion_floor16((int)s0) : s0), sx = x + (SUB ? dc_motion_floor16((int)s1) : s1);
  if constexpr (SUB) return sub8(f, sy, sx, dc_motion_frac16((int)s0), dc_motion_frac16((int)s1), H, W, flip, fill | (fill << 16), o);
  else return move8(f, sy, sx, H, W, fill | (fill << 16), o);
}
template <bool SUB>
__device__ __forceinline__ uint16_t put1(const uint16_t* __restrict__ f, long y, long x, long s0, long s1, int H, int W, unsigned flip,
                                         unsigned fill) {
  const long sy = y + (SUB ? dc_motion_floor16((int)s0) : s0), sx = x + (SUB ? dc_motion_floor16((int)s1) : s1);
  if constexpr (SUB) return sub1(f, sy, sx, dc_motion_frac16((int)s0), dc_motion_frac16((int)s1), H, W, flip, fill);
  else return (sy >= 0 && sy < H && sx >= 0 && sx < W) ? f[sy * W + sx] : (uint16_t)fill;
}

// out[t][y][x] = frames[t][y + dy][x + dx] inside the frame, fill outside; SUB (dc_motion_apply_sub): the bilinear interpolation of
// frames[t] at the fine shift shifts[t] (include/dcunet.h), fill where a used tap lies outside the frame.  A thread produces 8
// consecutive output values; the groups are cut at multiples of 8 elements of the WHOLE output (not of the frame), so a group that
// lies in one row is one aligned 16-byte store (put8: its source is one run of 8 values, or SUB two runs of 9, one per source row;
// the split and the weights are uniform over the frame).  Groups that cross a row, a frame or the edge of the source go value by
// value (put1).
template <bool SUB>
__global__ __launch_bounds__(kThreads) void motion_apply_kernel(const uint16_t* __restrict__ frames, unsigned flip, int tc,
                                                               const int* __restrict__ shifts, int H, int W, unsigned fill,
                                                               uint16_t* __restrict__ out, int wide) {
  const int HW = H * W;
  for (int t = blockIdx.y; t < tc; t += gridDim.y) {
    const long s0 = shifts[2 * t], s1 = shifts[2 * t + 1];
    const long base = (long)t * HW;
    const int off = (int)(base & 7);
    const int groups = (HW + off + 7) / 8;
    const uint16_t* f = frames + base;
    uint16_t* o = out + base;
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
      const int e0 = g * 8 - off;
      const int a = e0 < 0 ? 0 : e0, b = e0 + 8 < HW ? e0 + 8 : HW;
      int y = a / W, x = a - y * W;
      if (wide && b - a == 8 && x + 8 <= W && put8<SUB>(f, y, x, s0, s1, H, W, flip, fill, o + a)) continue;
      for (int e = a; e < b; ++e) {
        o[e] = put1<SUB>(f, y, x, s0, s1, H, W, flip, fill);
        if (++x == W) { x = 0; ++y; }
      }
    }
  }
}

// ---- sub-pixel: refine (the definitions are in include/dcunet.h, the arithmetic in motion_math.h; the interpolation is above) -----
// One thread per frame: the pick's neighbours on both axes, five scores of a table the pick kernel has just read.
__global__ __launch_bounds__(kThreads) void motion_refine_kernel(const int64_t* __restrict__ scores, const int* __restrict__ shifts, int tc,
                                                                int S, int* __restrict__ fine) {
  const long n = (2 * S + 1) * (2 * S + 1);
  for (long f = (long)blockIdx.x * kThreads + threadIdx.x; f < tc; f += (long)gridDim.x * kThreads) {
    const int dy = shifts[2 * f], dx = shifts[2 * f + 1];
    const DcSubShift q = dc_motion_refine_entry(scores + f * n, S, dy, dx);
    fine[2 * f] = dc_motion_fine(dy, q.qy);
    fine[2 * f + 1] = dc_motion_fine(dx, q.qx);
  }
}

// One thread per (frame, block): the residual the block pick added to the frame's clamped rigid shift, refined in the block's table.
__global__ __launch_bounds__(kThreads) void motion_block_refine_kernel(const int64_t* __restrict__ bscores, const int* __restrict__ rigid,
                                                                      const int* __restrict__ block_shifts, long items, int nblk, int S,
                                                                      int D, int* __restrict__ fine) {
  const long n = (2 * D + 1) * (2 * D + 1);
  for (long it = (long)blockIdx.x * kThreads + threadIdx.x; it < items; it += (long)gridDim.x * kThreads) {
    const long f = it / nblk;
    const int by = block_shifts[2 * it], bx = block_shifts[2 * it + 1];
    const int64_t ey = (int64_t)by - dc_motion_clamp(rigid[2 * f], S), ex = (int64_t)bx - dc_motion_clamp(rigid[2 * f + 1], S);
    DcSubShift q;
    q.qy = q.qx = 0;
    if (ey >= -D && ey <= D && ex >= -D && ex <= D) q = dc_motion_refine_entry(bscores + it * n, D, (int)ey, (int)ex);
    fine[2 * it] = dc_motion_fine(by, q.qy);
    fine[2 * it + 1] = dc_motion_fine(bx, q.qx);
  }
}

// ---- piecewise-rigid: block scores, block pick, warp (the definitions are in include/dcunet.h, the arithmetic in motion_math.h) ----
const int kBlkLanesX = 16;                                     // lanes of a wave along x
const int kBlkR = 4;                                           // rows a lane owns
const int kBlkTileW = kBlkLanesX * kPix;                       // 128 columns of a block per sweep
const int kBlkTileH = kWaves * (kWave / kBlkLanesX) * kBlkR;   // 64 rows of a block per strip

__host__ __device__ inline int bssd_stride(int D) { return kBlkTileW + ((2 * D + 7) & ~7); }

// One workgroup owns a whole (block, frame): it walks the block, clipped to the interior [M, H-M) x [M, W-M), in strips of 64 rows
// and sweeps of 128 columns -- a wave is 16 lanes x 8 pixels wide and 4 lanes x 4 rows high, so a block 100 pixels wide keeps
// 13 of 16 lanes busy.  Per tile the frame window around the RIGID shift (dy, dx) of the frame -- read here and clamped to
// [-S, S], which is what keeps the window inside the frame: its first row is >= M + dy - D >= 0, its last <= H - M - 1 + dy + D
// <= H - 1 -- is staged in LDS with its D-wide halo and scored at every residual (ey, ex) by the tile_* pieces above, nr differing
// per 16 lanes here.  The (2D+1)^2 totals of all tiles meet in LDS (zeroed once per frame) and leave with plain stores: every
// score is written, there is no global atomic and no zero launch.
template <int DMAX>
__global__ __launch_bounds__(kThreads) void motion_block_ssd_kernel(const uint16_t* __restrict__ frames, unsigned flip, int tc,
                                                                   const uint16_t* __restrict__ tmpl, int H, int W, int S, int D, int By,
                                                                   int Bx, const int* __restrict__ rigid,
                                                                   unsigned long long* __restrict__ bscores) {
  constexpr int R = kBlkR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nd = 2 * D + 1, M = S + D, stride = bssd_stride(D);
  uint16_t* ft = reinterpret_cast<uint16_t*>(smem);
  unsigned long long* sc = reinterpret_cast<unsigned long long*>(smem + tile_bytes(kBlkTileH, stride, D));
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int cl = lane % kBlkLanesX, rg = wave * (kWave / kBlkLanesX) + lane / kBlkLanesX;
  const int bi = blockIdx.x / Bx, bj = blockIdx.x % Bx;
  const int ya = dc_block_edge(bi, H, By), yb = dc_block_edge(bi + 1, H, By);
  const int xa = dc_block_edge(bj, W, Bx), xb = dc_block_edge(bj + 1, W, Bx);
  const int y0 = ya > M ? ya : M, y1 = yb < H - M ? yb : H - M;
  const int x0 = xa > M ? xa : M, x1 = xb < W - M ? xb : W - M;
  for (int f = blockIdx.y; f < tc; f += gridDim.y) {
    const int dy = dc_motion_clamp(rigid[2 * f], S), dx = dc_motion_clamp(rigid[2 * f + 1], S);
    const uint16_t* fr = frames + (long)f * H * W;
    __syncthreads();                                     // the previous frame's totals have been stored
    for (int i = threadIdx.x; i < nd * nd; i += kThreads) sc[i] = 0;
    for (int ty = y0; ty < y1; ty += kBlkTileH) {
      for (int tx = x0; tx < x1; tx += kBlkTileW) {
        const int th = y1 - ty < kBlkTileH ? y1 - ty : kBlkTileH, tw = x1 - tx < kBlkTileW ? x1 - tx : kBlkTileW;
        const int left = tw - kPix * cl, down = th - rg * R;
        const int np = left < 0 ? 0 : (left < kPix ? left : kPix);      // pixels of this lane
        const int nr = down < 0 ? 0 : (down < R ? down : R);            // rows of this lane
        unsigned mk[kPix], t2[R][kPix / 2];
        const bool ragged = tile_mask(np, mk);
        tile_tmpl<R>(tmpl + (long)(ty + rg * R) * W + tx + kPix * cl, W, nr, np, flip, t2);
        // the window of this tile: th + 2D rows, tw + 2D columns rounded up to the 16-byte pieces the lanes read; LDS (0, 0) is
        // frame (ty + dy - D, tx + dx - D).  What is not staged is read by lanes without pixels only, or masked.
        const int srows = th + 2 * D, scols = ((tw + 7) & ~7) + ((2 * D + 7) & ~7);
        __syncthreads();                                 // the readers of the previous tile are done
        tile_stage(ft, stride, fr, H, W, ty + dy - D, tx + dx - D, srows, scols, flip, wave, lane);
        __syncthreads();
        tile_score<DMAX, R>(ft, stride, D, nr, np, ragged, rg * R, cl, lane, t2, mk, sc);
      }
    }
    __syncthreads();
    unsigned long long* dst = bscores + ((long)f * gridDim.x + blockIdx.x) * nd * nd;
    for (int i = threadIdx.x; i < nd * nd; i += kThreads) dst[i] = sc[i];
  }
}

// One wave per (frame, block): the residual (ey, ex) under the order of motion_math.h, added to the frame's clamped rigid shift.
__global__ __launch_bounds__(kWave) void motion_block_pick_kernel(const int64_t* __restrict__ bscores, const int* __restrict__ rigid,
                                                                 long items, int nblk, int S, int D, int* __restrict__ block_shifts,
                                                                 int64_t* __restrict__ best) {
  const int n = (2 * D + 1) * (2 * D + 1), lane = threadIdx.x;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const DcShiftCand b = pick_wave(bscores + it * n, D, lane);
    if (lane == 0) {
      const long f = it / nblk;
      block_shifts[2 * it] = dc_motion_clamp(rigid[2 * f], S) + b.dy;
      block_shifts[2 * it + 1] = dc_motion_clamp(rigid[2 * f + 1], S) + b.dx;
      if (best) best[it] = b.score;
    }
  }
}

const int kWarpRows = 16;              // rows of one workgroup's tile
const int kWarpCols = 1024;            // its columns, at most

// out[t][y][x] = frames[t][y + fy][x + fx], (fy, fx) the shift field at (y, x).  One workgroup per tile of 16 rows x <= 1024
// columns and frame.  The block edges of both axes, then the taps of the tile's rows and columns (dc_field_tap_edges: a bisection
// and one division each) are derived once per workgroup into LDS -- from the geometry, so no index read from memory addresses
// block_shifts --, then per frame the row blends a[r][j] = (256-w) s[i0][j] + w s[i1][j] of both components, which leaves a pixel
// two multiplications per component, one where a group of 8 lies between the same two centres.
// A thread moves 8 consecutive outputs of one row, cut at multiples of 8 elements of the WHOLE output as in motion_apply_kernel:
// where the field is the same at all 8 (compared one by one: along a row it is monotone between two centres only) the group is
// that kernel's aligned 16-byte store (put8); otherwise it goes value by value (put1).
// SUB (dc_motion_warp_sub): bs holds FINE block shifts, so the field is a fine shift per pixel, which put8 / put1 split.
template <bool SUB>
__global__ __launch_bounds__(kThreads) void motion_warp_kernel(const uint16_t* __restrict__ frames, int tc, const int* __restrict__ bs,
                                                              int By, int Bx, int H, int W, unsigned fill, uint16_t* __restrict__ out,
                                                              int wide, int tilesX, unsigned flip) {
  __shared__ int ctap[kWarpCols];                        // j0 | v << 8 (j1 = j0 + 1 where v > 0)
  __shared__ int rtap[kWarpRows];                        // i0 | w << 8
  __shared__ int64_t a[kWarpRows][DC_MOTION_MAX_BLOCKS][2];
  __shared__ int edge[2][DC_MOTION_MAX_BLOCKS + 1];      // the block edges of the rows and of the columns
  const int tx = blockIdx.x % tilesX, ty = blockIdx.x / tilesX;
  const int xlo = tx * kWarpCols, ylo = ty * kWarpRows;
  const int xhi = xlo + kWarpCols < W ? xlo + kWarpCols : W, yhi = ylo + kWarpRows < H ? ylo + kWarpRows : H;
  const int ncol = xhi - xlo, nrow = yhi - ylo;
  if (threadIdx.x <= By) edge[0][threadIdx.x] = dc_block_edge(threadIdx.x, H, By);
  if (threadIdx.x >= kWave && threadIdx.x - kWave <= Bx) edge[1][threadIdx.x - kWave] = dc_block_edge(threadIdx.x - kWave, W, Bx);
  __syncthreads();
  for (int c = threadIdx.x; c < ncol; c += kThreads) {
    const DcFieldTap t = dc_field_tap_edges(xlo + c, edge[1], Bx);
    ctap[c] = t.i0 | (t.w << 8);
  }
  if (threadIdx.x < nrow) {
    const DcFieldTap t = dc_field_tap_edges(ylo + threadIdx.x, edge[0], By);
    rtap[threadIdx.x] = t.i0 | (t.w << 8);
  }
  const int HW = H * W;
  for (int t = blockIdx.y; t < tc; t += gridDim.y) {
    const int* s = bs + (long)t * By * Bx * 2;
    __syncthreads();                                     // the taps are there; the readers of the previous frame's blends are done
    for (int i = threadIdx.x; i < nrow * Bx * 2; i += kThreads) {
      const int c = i & 1, j = (i >> 1) % Bx, r = (i >> 1) / Bx;
      const int i0 = rtap[r] & 0xff, w = rtap[r] >> 8, i1 = w ? i0 + 1 : i0;
      a[r][j][c] = dc_field_blend(s[(i0 * Bx + j) * 2 + c], s[(i1 * Bx + j) * 2 + c], w);
    }
    __syncthreads();
    const long base = (long)t * HW;
    const uint16_t* f = frames + base;
    // the groups of row y: [A + 8q, A + 8q + 8) of the whole output, cut to the row's columns [xlo, xhi); A = (e0 & ~7)
    const int nq = ncol / 8 + 2;
    for (int g = threadIdx.x; g < nrow * nq; g += kThreads) {
      const int r = g / nq, q = g - r * nq, y = ylo + r;
      const long e0 = base + (long)y * W + xlo, e1 = e0 + ncol;
      const long ga = (e0 & ~7L) + 8L * q;
      const long lo = ga > e0 ? ga : e0, hi = ga + 8 < e1 ? ga + 8 : e1;
      if (lo >= hi) continue;
      const int n = (int)(hi - lo), x = xlo + (int)(lo - e0);
      long fy[8], fx[8];
      bool same = true;
      // j0 never decreases along a row: where the group's ends share it, all 8 pixels blend the same two columns of a[r], and
      // where those are less than 2^14 pixels apart the blend is one 24-bit multiplication per pixel and component
      const int jf = ctap[x - xlo] & 0xff, jn = jf + 1 < Bx ? jf + 1 : jf;         // past the last centre v is 0: any jn does
      const int64_t ay = a[r][jf][0], ax = a[r][jf][1], dy = a[r][jn][0] - ay, dx = a[r][jn][1] - ax;
      if ((ctap[x - xlo + n - 1] & 0xff) == jf && dc_field_delta_small(dy) && dc_field_delta_small(dx)) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int v = ctap[k < n ? x - xlo + k : x - xlo] >> 8;
          fy[k] = dc_field_from_delta(ay, (int)dy, v);
          fx[k] = dc_field_from_delta(ax, (int)dx, v);
          same = same && fy[k] == fy[0] && fx[k] == fx[0];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int ct = ctap[k < n ? x - xlo + k : x - xlo];
          const int j0 = ct & 0xff, v = ct >> 8, j1 = v ? j0 + 1 : j0;
          fy[k] = dc_field_from_rows(a[r][j0][0], a[r][j1][0], v);
          fx[k] = dc_field_from_rows(a[r][j0][1], a[r][j1][1], v);
          same = same && fy[k] == fy[0] && fx[k] == fx[0];
        }
      }
      uint16_t* o = out + lo;                            // the field never leaves the int32 range of the block shifts
      if (wide && n == 8 && same && put8<SUB>(f, y, x, fy[0], fx[0], H, W, flip, fill, o)) continue;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (k < n) o[k] = put1<SUB>(f, y, (long)x + k, fy[k], fx[k], H, W, flip, fill);       // the column in 64 bits from the start
      }
    }
  }
}

// ---- wide search: bin (the definitions are in include/dcunet.h, the arithmetic in motion_math.h; window scores and pick are above) -
// out[t][Y][X] = the rounded mean of the c x c cell (cY.., cX..) of frame t, c = 2^LG.  One memory-bound pass: a thread owns 8
// consecutive input columns of the c rows of one binned row -- c 16-byte loads where the rows are 16-byte aligned (wide: W % 8 == 0
// and an aligned base), value by value otherwise -- and stores the 8 / c bins they hold.  Neighbouring threads read neighbouring
// 16-byte pieces of a row.  The trailing H % c rows and W % c columns are never read for a bin.
template <int LG>
__global__ __launch_bounds__(kThreads) void motion_bin_kernel(const uint16_t* __restrict__ frames, int is_unsigned, int tc, int H, int W,
                                                             uint16_t* __restrict__ out, int wide) {
  constexpr int C = 1 << LG, PER = kPix / C;
  const int Hc = H >> LG, Wc = W >> LG;
  const int G = (Wc * C + kPix - 1) / kPix;              // groups of 8 input columns that hold a binned column
  const long items = (long)tc * Hc * G;
  for (long it = (long)blockIdx.x * kThreads + threadIdx.x; it < items; it += (long)gridDim.x * kThreads) {
    const int g = (int)(it % G);
    const long row = it / G;                             // t * Hc + Y
    const int Y = (int)(row % Hc);
    const long t = row / Hc;
    const int x0 = kPix * g;
    const uint16_t* src = frames + (t * H + (long)Y * C) * W + x0;
    int s[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) s[k] = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const uint16_t* p = src + (long)i * W;
      unsigned w[kPix / 2];
      if (wide) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      } else {
#pragma unroll
        for (int q = 0; q < kPix / 2; ++q) {
          const unsigned lo = x0 + 2 * q < W ? p[2 * q] : 0u, hi = x0 + 2 * q + 1 < W ? p[2 * q + 1] : 0u;
          w[q] = lo | (hi << 16);
        }
      }
#pragma unroll
      for (int k = 0; k < kPix; ++k) {
        const unsigned v = (w[k / 2] >> (16 * (k & 1))) & 0xffffu;
        s[k] += is_unsigned ? (int)v : (int)(int16_t)v;
      }
    }
    uint16_t* dst = out + row * Wc + (long)PER * g;
#pragma unroll
    for (int o = 0; o < PER; ++o) {
      int sum = 0;
#pragma unroll
      for (int j = 0; j < C; ++j) sum += s[o * C + j];
      if (PER * g + o < Wc) dst[o] = (uint16_t)dc_motion_bin_round(sum, LG);
    }
  }
}

// ---- bidirectional scan-phase correction: line scores and the odd-row move (the definitions are in include/dcunet.h) -------------
const int kBidiR = 4;                                          // odd rows a wave owns
const int kBidiTH = kWaves * kBidiR;                           // odd rows of one workgroup's tile: 16
const int kBidiRows = 2 * kBidiTH + 1;                         // frame rows of the tile: its odd rows and the even rows around them

// LDS of a score launch: the tile's frame rows (the odd ones with their P-wide halo), then the 2P+1 totals of the workgroup
__host__ __device__ inline size_t bidi_tile_bytes(int P) { return (size_t)kBidiRows * ssd_stride(P) * sizeof(uint16_t); }
inline int bidi_lds(int P) { return (int)bidi_tile_bytes(P) + (2 * P + 1) * (int)sizeof(long long); }

// The nr odd rows of one lane against their even neighbours, all nd offsets:  acc[k] += (2 f[y][x + k - P] - f[y-1][x] - f[y+1][x])^2.
// LDS row 2 j + 1 is the lane's odd row j (column 0: P columns left of the tile's first interior pixel), rows 2 j and 2 j + 2 the even
// rows around it (column 0: that pixel).  |e| <= 131070, so e^2 needs 34 bits: the product is formed in 64 bits from |e| (one
// 32 x 32 -> 64 multiply-add).  A lane adds at most kBidiR * kPix = 32 of them per offset: < 2^39.  RAG as for ssd_rows.
template <int PMAX, bool RAG>
__device__ __forceinline__ void bidi_rows(const uint16_t* __restrict__ ft, int stride, int P, int nd, int nr, int row0, int lane,
                                         const unsigned (&mk)[kPix], unsigned long long (&acc)[2 * PMAX + 1]) {
  constexpr int NK = 2 * PMAX + 1, FW = kPix + 2 * PMAX;
  uint4 up = *reinterpret_cast<const uint4*>(ft + (long)(2 * row0) * stride + kPix * lane);
#pragma unroll
  for (int j = 0; j < kBidiR; ++j) {
    if (j < nr) {                                        // wave-uniform
      const uint4 dn = *reinterpret_cast<const uint4*>(ft + (long)(2 * (row0 + j) + 2) * stride + kPix * lane);
      const unsigned u2[kPix / 2] = {up.x, up.y, up.z, up.w}, d2[kPix / 2] = {dn.x, dn.y, dn.z, dn.w};
      int n[kPix];
#pragma unroll
      for (int p = 0; p < kPix; ++p) n[p] = (int)((u2[p / 2] >> (16 * (p & 1))) & 0xffffu) + (int)((d2[p / 2] >> (16 * (p & 1))) & 0xffffu);
      const uint4* src = reinterpret_cast<const uint4*>(ft + (long)(2 * (row0 + j) + 1) * stride + kPix * lane);
      unsigned w[FW / 2];
#pragma unroll
      for (int q = 0; q < FW / 8; ++q) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (q * 8 < kPix + 2 * P) v = src[q];            // wave-uniform: the window is kPix + 2P values long
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
      }
      int fw[FW];
#pragma unroll
      for (int i = 0; i < FW; ++i) fw[i] = (int)((w[i / 2] >> (16 * (i & 1))) & 0xffffu);
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        if (k < nd) {                                    // wave-uniform
#pragma unroll
          for (int p = 0; p < kPix; ++p) {
            int e = 2 * fw[p + k] - n[p];                // 18 bits and a sign
            if (RAG) e = (int)((unsigned)e & mk[p]);
            const unsigned a = (unsigned)(e < 0 ? -e : e);
            acc[k] += (unsigned long long)a * a;
          }
        }
      }
      up = dn;
    }
  }
}

// scores[f][p + P] of include/dcunet.h.  One workgroup per tile of kBidiTH odd rows x 512 interior columns and frame.  The tile's
// 2 * kBidiTH + 1 frame rows are staged in LDS once (values with the sign bit flipped for int16: all four terms of a difference
// move by 32768, the difference does not) and reused for all 2P+1 offsets; a lane owns kPix consecutive interior columns of kBidiR
// odd rows.  Outside the frame the tile holds 0, read by lanes without pixels only, or masked: a pixel that counts has
// y + 1 <= H - 1 and P <= x - P, x + P <= W - 1.  The wave adds its sums by shuffles, the workgroup's totals meet in LDS, and ONE
// 64-bit atomic per offset and workgroup goes to memory (integer addition: the order does not matter).
template <int PMAX>
__global__ __launch_bounds__(kThreads) void bidi_scores_kernel(const uint16_t* __restrict__ frames, unsigned flip, int tc, int H, int W, int P,
                                                              unsigned long long* __restrict__ scores, int tilesX) {
  constexpr int NK = 2 * PMAX + 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nd = 2 * P + 1, stride = ssd_stride(P);
  uint16_t* ft = reinterpret_cast<uint16_t*>(smem);
  unsigned long long* sc = reinterpret_cast<unsigned long long*>(smem + bidi_tile_bytes(P));
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int tx = blockIdx.x % tilesX, ty = blockIdx.x / tilesX;
  const int i0 = tx * kTileW, j0 = ty * kBidiTH;         // the tile's first interior column, counted from P, and its first odd row, counted in odd rows
  const int IW = W - 2 * P, NO = (H - 1) / 2;            // interior columns; odd rows y = 2 j + 1 with y + 1 <= H - 1
  const int left = IW - i0 - kPix * lane, down = NO - j0 - wave * kBidiR;
  const int np = left < 0 ? 0 : (left < kPix ? left : kPix);      // interior pixels of this lane
  const int nr = down < 0 ? 0 : (down < kBidiR ? down : kBidiR);  // odd rows of this wave
  unsigned mk[kPix];
  const bool ragged = tile_mask(np, mk);
  for (int f = blockIdx.y; f < tc; f += gridDim.y) {
    const uint16_t* fr = frames + (long)f * H * W;
    __syncthreads();                                     // the readers of the previous frame's tile and totals are done
    for (int r = wave; r < kBidiRows; r += kWaves) {
      // LDS row r is frame row 2 j0 + r; an odd row starts P columns left of the interior pixel an even row starts at
      const int gy = 2 * j0 + r, ox = (r & 1) ? i0 : P + i0, cols = (r & 1) ? stride : kTileW;
      for (int c = lane; c < cols; c += kWave) {
        const int gx = ox + c;
        ft[r * stride + c] = (gy < H && gx < W) ? (uint16_t)(fr[(long)gy * W + gx] ^ flip) : (uint16_t)0;
      }
    }
    for (int i = threadIdx.x; i < nd; i += kThreads) sc[i] = 0;
    __syncthreads();
    if (nr > 0) {                                        // wave-uniform: EVERY lane of the wave takes part in the shuffles
      unsigned long long acc[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) acc[k] = 0;
      if (np > 0) {
        if (ragged) bidi_rows<PMAX, true>(ft, stride, P, nd, nr, wave * kBidiR, lane, mk, acc);
        else bidi_rows<PMAX, false>(ft, stride, P, nd, nr, wave * kBidiR, lane, mk, acc);
      }
      unsigned long long mine = 0;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        if (k < nd) {
          const unsigned long long s = wave_sum64(acc[k]);
          if (lane == k) mine = s;
        }
      }
      if (lane < nd) atomicAdd(&sc[lane], mine);
    }
    __syncthreads();
    unsigned long long* dst = scores + (long)f * nd;
    for (int i = threadIdx.x; i < nd; i += kThreads) {
      const unsigned long long v = sc[i];
      if (v) atomicAdd(dst + i, v);
    }
  }
}

// out[t][y][x] = frames[t][y][x + p] for odd y (fill where x + p leaves the row), frames[t][y][x] for even y: motion_apply_kernel
// with the shift (0, p) on the odd rows and (0, 0) on the even ones -- the same groups of 8 of the WHOLE output, the same put8 / put1.
__global__ __launch_bounds__(kThreads) void bidi_apply_kernel(const uint16_t* __restrict__ frames, int tc, int p, int H, int W, unsigned fill,
                                                             uint16_t* __restrict__ out, int wide) {
  const int HW = H * W;
  for (int t = blockIdx.y; t < tc; t += gridDim.y) {
    const long base = (long)t * HW;
    const int off = (int)(base & 7);
    const int groups = (HW + off + 7) / 8;
    const uint16_t* f = frames + base;
    uint16_t* o = out + base;
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
      const int e0 = g * 8 - off;
      const int a = e0 < 0 ? 0 : e0, b = e0 + 8 < HW ? e0 + 8 : HW;
      int y = a / W, x = a - y * W;
      if (wide && b - a == 8 && x + 8 <= W && put8<false>(f, y, x, 0, (y & 1) ? p : 0, H, W, 0u, fill, o + a)) continue;
      for (int e = a; e < b; ++e) {
        o[e] = put1<false>(f, y, x, 0, (y & 1) ? p : 0, H, W, 0u, fill);
        if (++x == W) { x = 0; ++y; }
      }
    }
  }
}

// ---- launchers.  name: the entry point, for the messages ---------------------------------------------------------------------------
// the frame dimension of a grid (the kernels stride over the frames beyond it)
inline unsigned frame_dim(int tc) { return (unsigned)(tc < 65535 ? tc : 65535); }

template <int LG>
int launch_bin(const uint16_t* frames, int is_unsigned, int tc, int H, int W, uint16_t* out, hipStream_t stream) {
  const int Hc = H >> LG, Wc = W >> LG;
  const long items = (long)tc * Hc * dc_cdiv((long)Wc << LG, kPix), blocks = (items + kThreads - 1) / kThreads;
  const int wide = (int)(W % kPix == 0 && dc_aligned16(frames));
  hipLaunchKernelGGL(motion_bin_kernel<LG>, dim3((unsigned)(blocks < (1L << 20) ? blocks : (1L << 20))), dim3(kThreads), 0, stream, frames,
                     is_unsigned, tc, H, W, out, wide);
  DC_CHECK_LAUNCH("dc_motion_bin");
  return DC_OK;
}

template <int RMAX, int R>
int launch_ssd(const char* name, const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int S, int D, const int* centres,
               int mult, unsigned long long* scores, hipStream_t stream) {
  static DcLdsAttr lds_attr;
  const int TH = kWaves * R;
  auto kern = motion_ssd_kernel<RMAX, R>;
  if (int rc = dc_func_max_lds(lds_attr, reinterpret_cast<const void*>(kern), ssd_lds(TH, ssd_stride(RMAX), RMAX), name)) return rc;
  const int tilesX = dc_cdiv(W - 2 * S, kTileW), tilesY = dc_cdiv(H - 2 * S, TH);
  const dim3 grid((unsigned)(tilesX * tilesY), frame_dim(tc)), block(kThreads);
  hipLaunchKernelGGL(kern, grid, block, ssd_lds(TH, ssd_stride(D), D), stream, (const uint16_t*)frames, is_unsigned ? 0u : 0x8000u, tc,
                     (const uint16_t*)tmpl, H, W, S, D, centres, mult, scores, tilesX);
  DC_CHECK_LAUNCH(name);
  return DC_OK;
}

// The frame-wide scores: the zero launch (the score kernel leaves its totals by atomics), then the instantiation for the window
// half-width D: D <= 4, D <= 8 (what a window table may ask for) or D <= 16 with 4 rows per wave (an exhaustive table, D = S)
int launch_scores(const char* name, const char* zero_name, const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int S,
                  int D, const int* centres, int mult, long* scores, hipStream_t stream) {
  if (tc == 0) return DC_OK;
  const long n = (long)tc * (2 * D + 1) * (2 * D + 1);
  unsigned long long* sc = (unsigned long long*)scores;
  const int blocks = (int)(dc_cdiv(n, kThreads) < kZeroBlocks ? dc_cdiv(n, kThreads) : kZeroBlocks);
  hipLaunchKernelGGL(motion_zero_kernel, dim3(blocks), dim3(kThreads), 0, stream, sc, n);
  DC_CHECK_LAUNCH(zero_name);
  if (D <= 4) return launch_ssd<4, 8>(name, frames, is_unsigned, tc, tmpl, H, W, S, D, centres, mult, sc, stream);
  if (D <= 8) return launch_ssd<8, 8>(name, frames, is_unsigned, tc, tmpl, H, W, S, D, centres, mult, sc, stream);
  return launch_ssd<16, 4>(name, frames, is_unsigned, tc, tmpl, H, W, S, D, centres, mult, sc, stream);
}

template <int DMAX>
int launch_block_ssd(const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int S, int D, int By, int Bx,
                     const int* rigid, unsigned long long* bscores, hipStream_t stream) {
  const dim3 grid((unsigned)(By * Bx), frame_dim(tc)), block(kThreads);
  hipLaunchKernelGGL(motion_block_ssd_kernel<DMAX>, grid, block, ssd_lds(kBlkTileH, bssd_stride(D), D), stream, (const uint16_t*)frames,
                     is_unsigned ? 0u : 0x8000u, tc, (const uint16_t*)tmpl, H, W, S, D, By, Bx, rigid, bscores);
  DC_CHECK_LAUNCH("dc_motion_block_ssd");
  return DC_OK;
}

int launch_pick(const char* name, const long* scores, const int* centres, int mult, int tc, int S, int D, int* shifts, long* best, int* fine,
                hipStream_t stream) {
  if (tc == 0) return DC_OK;
  hipLaunchKernelGGL(motion_pick_kernel, dim3(frame_dim(tc)), dim3(kWave), 0, stream, (const int64_t*)scores, centres, mult, tc, S, D, shifts,
                     (int64_t*)best, fine);
  DC_CHECK_LAUNCH(name);
  return DC_OK;
}

// flip: 0x8000 for int16 where the mover interpolates (SUB), unused otherwise.  wide: out is 16-byte aligned.
template <bool SUB>
int launch_apply(const char* name, const void* frames, unsigned flip, int tc, const int* shifts, int H, int W, int fill, void* out,
                 hipStream_t stream) {
  if (tc == 0) return DC_OK;
  const int bx = dc_cdiv(dc_cdiv((long)H * W + 7, 8), kThreads);
  const dim3 grid((unsigned)(bx < 4096 ? bx : 4096), frame_dim(tc)), block(kThreads);
  hipLaunchKernelGGL(motion_apply_kernel<SUB>, grid, block, 0, stream, (const uint16_t*)frames, flip, tc, shifts, H, W,
                     (unsigned)fill & 0xffffu, (uint16_t*)out, (int)dc_aligned16(out));
  DC_CHECK_LAUNCH(name);
  return DC_OK;
}

template <bool SUB>
int launch_warp(const char* name, const void* frames, unsigned flip, int tc, const int* block_shifts, int By, int Bx, int H, int W, int fill,
                void* out, hipStream_t stream) {
  if (tc == 0) return DC_OK;
  const int tilesX = dc_cdiv(W, kWarpCols);
  const long tiles = (long)tilesX * dc_cdiv(H, kWarpRows);              // H * W <= 2^30: at most 2^30 tiles
  const dim3 grid((unsigned)tiles, frame_dim(tc)), block(kThreads);
  hipLaunchKernelGGL(motion_warp_kernel<SUB>, grid, block, 0, stream, (const uint16_t*)frames, tc, block_shifts, By, Bx, H, W,
                     (unsigned)fill & 0xffffu, (uint16_t*)out, (int)dc_aligned16(out), tilesX, flip);
  DC_CHECK_LAUNCH(name);
  return DC_OK;
}

// out[0 .. n) and frames[0 .. n) of 16-bit values do not overlap
inline bool disjoint16(const void* frames, const void* out, uintptr_t n) {
  const uintptr_t bytes = n * 2, fa = (uintptr_t)frames, oa = (uintptr_t)out;
  return bytes == 0 || fa + bytes <= oa || oa + bytes <= fa;
}

}  // namespace

// Checks that several entry points share.  The messages carry the entry's name, so each takes it as a string literal.
#define DC_REQUIRE_IMAGE(name, H, W) DC_REQUIRE((long)H * W <= (1L << 30), DC_EUNSUP, name ": image %d x %d: H * W is limited to 2^30", H, W)

// the four movers, after their sizes: the fill value, the alignment, out beside frames
#define DC_REQUIRE_MOVE(name, frames, table, out, tc, H, W, fill)                                                                          \
  DC_REQUIRE(fill >= -32768 && fill <= 65535, DC_EINVAL, name ": fill = %d is not a 16-bit value", fill);                                   \
  DC_REQUIRE((((uintptr_t)frames | (uintptr_t)out) & 1) == 0 && (((uintptr_t)table) & 3) == 0, DC_EINVAL, name ": misaligned buffer");      \
  DC_REQUIRE(disjoint16(frames, out, (uintptr_t)tc * H * W), DC_EINVAL, name ": out overlaps frames")

// the two warps, after their sizes: the block grid, the image, the rest of the movers' checks
#define DC_REQUIRE_WARP(name, frames, table, out, tc, By, Bx, H, W, fill)                                                                  \
  DC_REQUIRE(By <= DC_MOTION_MAX_BLOCKS && Bx <= DC_MOTION_MAX_BLOCKS, DC_EUNSUP, name ": %d x %d blocks: the grid is limited to %d x %d", \
             By, Bx, DC_MOTION_MAX_BLOCKS, DC_MOTION_MAX_BLOCKS);                                                                         \
  DC_REQUIRE_IMAGE(name, H, W);                                                                                                            \
  DC_REQUIRE(By <= H && Bx <= W, DC_EINVAL, name ": image %d x %d in %d x %d blocks: a block is empty", H, W, By, Bx);                      \
  DC_REQUIRE_MOVE(name, frames, table, out, tc, H, W, fill)

// the three piecewise entry points that take both radii and the block grid
#define DC_REQUIRE_GRID(name, S, D, By, Bx)                                                                                              \
  DC_REQUIRE(S <= DC_MOTION_MAX_SHIFT, DC_EUNSUP, name ": S = %d: the search radius is limited to %d", S, DC_MOTION_MAX_SHIFT);           \
  DC_REQUIRE(D <= DC_MOTION_MAX_DEV, DC_EUNSUP, name ": D = %d: the block deviation radius is limited to %d", D, DC_MOTION_MAX_DEV);      \
  DC_REQUIRE(By <= DC_MOTION_MAX_BLOCKS && Bx <= DC_MOTION_MAX_BLOCKS, DC_EUNSUP, name ": %d x %d blocks: the grid is limited to %d x %d", \
             By, Bx, DC_MOTION_MAX_BLOCKS, DC_MOTION_MAX_BLOCKS)

// the two window entry points: the radii
#define DC_REQUIRE_WINDOW(name, S, D)                                                                                                        \
  DC_REQUIRE(S <= DC_MOTION_MAX_WIDE_SHIFT, DC_EUNSUP, name ": S = %d: the wide search radius is limited to %d", S, DC_MOTION_MAX_WIDE_SHIFT); \
  DC_REQUIRE(D <= DC_MOTION_MAX_DEV, DC_EUNSUP, name ": D = %d: the window half-width is limited to %d", D, DC_MOTION_MAX_DEV);               \
  DC_REQUIRE(S >= D, DC_EINVAL, name ": S = %d is smaller than the window half-width D = %d", S, D)

extern "C" int dc_motion_ssd(const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int S, long* scores,
                             dc_stream_t stream) {
  DC_REQUIRE(frames && tmpl && scores, DC_EINVAL, "dc_motion_ssd: null pointer");
  DC_REQUIRE(tc >= 0 && S >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_motion_ssd: negative or zero size (tc %d, S %d, H %d, W %d)", tc, S, H, W);
  DC_REQUIRE_FRAMES("dc_motion_ssd", tc);
  DC_REQUIRE(S <= DC_MOTION_MAX_SHIFT, DC_EUNSUP, "dc_motion_ssd: S = %d: the search radius is limited to %d", S, DC_MOTION_MAX_SHIFT);
  DC_REQUIRE_IMAGE("dc_motion_ssd", H, W);
  DC_REQUIRE(H > 2 * S && W > 2 * S, DC_EINVAL, "dc_motion_ssd: image %d x %d has no interior at S = %d (H > 2S and W > 2S)", H, W, S);
  DC_REQUIRE((((uintptr_t)frames | (uintptr_t)tmpl) & 1) == 0 && (((uintptr_t)scores) & 7) == 0, DC_EINVAL, "dc_motion_ssd: misaligned buffer");
  // the exhaustive table is the window of half-width S around centre 0
  return launch_scores("dc_motion_ssd", "dc_motion_ssd(zero)", frames, is_unsigned, tc, tmpl, H, W, S, S, nullptr, 0, scores, (hipStream_t)stream);
}

extern "C" int dc_motion_pick(const long* scores, int tc, int S, int* shifts, long* best, dc_stream_t stream) {
  DC_REQUIRE(scores && shifts, DC_EINVAL, "dc_motion_pick: null pointer");
  DC_REQUIRE(tc >= 0 && S >= 0, DC_EINVAL, "dc_motion_pick: negative size (tc %d, S %d)", tc, S);
  DC_REQUIRE_FRAMES("dc_motion_pick", tc);
  DC_REQUIRE(S <= DC_MOTION_MAX_SHIFT, DC_EUNSUP, "dc_motion_pick: S = %d: the search radius is limited to %d", S, DC_MOTION_MAX_SHIFT);
  DC_REQUIRE((((uintptr_t)scores | (uintptr_t)best) & 7) == 0 && (((uintptr_t)shifts) & 3) == 0, DC_EINVAL, "dc_motion_pick: misaligned buffer");
  return launch_pick("dc_motion_pick", scores, nullptr, 0, tc, S, S, shifts, best, nullptr, (hipStream_t)stream);
}

extern "C" int dc_motion_apply(const void* frames, int tc, const int* shifts, int H, int W, int fill, void* out, dc_stream_t stream) {
  DC_REQUIRE(frames && shifts && out, DC_EINVAL, "dc_motion_apply: null pointer");
  DC_REQUIRE(tc >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_motion_apply: negative or zero size (tc %d, H %d, W %d)", tc, H, W);
  DC_REQUIRE_FRAMES("dc_motion_apply", tc);
  DC_REQUIRE_IMAGE("dc_motion_apply", H, W);
  DC_REQUIRE_MOVE("dc_motion_apply", frames, shifts, out, tc, H, W, fill);
  return launch_apply<false>("dc_motion_apply", frames, 0u, tc, shifts, H, W, fill, out, (hipStream_t)stream);
}

extern "C" int dc_motion_block_ssd(const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int S, int D, int By, int Bx,
                                   const int* rigid, long* bscores, dc_stream_t stream) {
  DC_REQUIRE(frames && tmpl && rigid && bscores, DC_EINVAL, "dc_motion_block_ssd: null pointer");
  DC_REQUIRE(tc >= 0 && S >= 0 && D >= 0 && H > 0 && W > 0 && By > 0 && Bx > 0, DC_EINVAL,
             "dc_motion_block_ssd: negative or zero size (tc %d, S %d, D %d, H %d, W %d, blocks %d x %d)", tc, S, D, H, W, By, Bx);
  DC_REQUIRE_FRAMES("dc_motion_block_ssd", tc);
  DC_REQUIRE_GRID("dc_motion_block_ssd", S, D, By, Bx);
  DC_REQUIRE_IMAGE("dc_motion_block_ssd", H, W);
  DC_REQUIRE(dc_block_axis_ok(H, By, S + D) && dc_block_axis_ok(W, Bx, S + D), DC_EINVAL,
             "dc_motion_block_ssd: image %d x %d in %d x %d blocks: a block has no interior at S + D = %d", H, W, By, Bx, S + D);
  DC_REQUIRE((((uintptr_t)frames | (uintptr_t)tmpl) & 1) == 0 && (((uintptr_t)rigid) & 3) == 0 && (((uintptr_t)bscores) & 7) == 0, DC_EINVAL,
             "dc_motion_block_ssd: misaligned buffer");
  if (tc == 0) return DC_OK;
  unsigned long long* sc = (unsigned long long*)bscores;
  if (D <= 4) return launch_block_ssd<4>(frames, is_unsigned, tc, tmpl, H, W, S, D, By, Bx, rigid, sc, (hipStream_t)stream);
  return launch_block_ssd<8>(frames, is_unsigned, tc, tmpl, H, W, S, D, By, Bx, rigid, sc, (hipStream_t)stream);
}

extern "C" int dc_motion_block_pick(const long* bscores, const int* rigid, int tc, int By, int Bx, int S, int D, int* block_shifts, long* best,
                                    dc_stream_t stream) {
  DC_REQUIRE(bscores && rigid && block_shifts, DC_EINVAL, "dc_motion_block_pick: null pointer");
  DC_REQUIRE(tc >= 0 && S >= 0 && D >= 0 && By > 0 && Bx > 0, DC_EINVAL,
             "dc_motion_block_pick: negative or zero size (tc %d, S %d, D %d, blocks %d x %d)", tc, S, D, By, Bx);
  DC_REQUIRE_FRAMES("dc_motion_block_pick", tc);
  DC_REQUIRE_GRID("dc_motion_block_pick", S, D, By, Bx);
  DC_REQUIRE((((uintptr_t)bscores | (uintptr_t)best) & 7) == 0 && (((uintptr_t)rigid | (uintptr_t)block_shifts) & 3) == 0, DC_EINVAL,
             "dc_motion_block_pick: misaligned buffer");
  if (tc == 0) return DC_OK;
  const long items = (long)tc * By * Bx;
  hipLaunchKernelGGL(motion_block_pick_kernel, dim3((unsigned)(items < (1L << 20) ? items : (1L << 20))), dim3(kWave), 0, (hipStream_t)stream,
                     (const int64_t*)bscores, rigid, items, By * Bx, S, D, block_shifts, (int64_t*)best);
  DC_CHECK_LAUNCH("dc_motion_block_pick");
  return DC_OK;
}

extern "C" int dc_motion_warp(const void* frames, int tc, const int* block_shifts, int By, int Bx, int H, int W, int fill, void* out,
                              dc_stream_t stream) {
  DC_REQUIRE(frames && block_shifts && out, DC_EINVAL, "dc_motion_warp: null pointer");
  DC_REQUIRE(tc >= 0 && H > 0 && W > 0 && By > 0 && Bx > 0, DC_EINVAL, "dc_motion_warp: negative or zero size (tc %d, H %d, W %d, blocks %d x %d)",
             tc, H, W, By, Bx);
  DC_REQUIRE_FRAMES("dc_motion_warp", tc);
  DC_REQUIRE_WARP("dc_motion_warp", frames, block_shifts, out, tc, By, Bx, H, W, fill);
  return launch_warp<false>("dc_motion_warp", frames, 0u, tc, block_shifts, By, Bx, H, W, fill, out, (hipStream_t)stream);
}

extern "C" int dc_motion_refine(const long* scores, const int* shifts, int tc, int S, int* fine, dc_stream_t stream) {
  DC_REQUIRE(scores && shifts && fine, DC_EINVAL, "dc_motion_refine: null pointer");
  DC_REQUIRE(tc >= 0 && S >= 0, DC_EINVAL, "dc_motion_refine: negative size (tc %d, S %d)", tc, S);
  DC_REQUIRE_FRAMES("dc_motion_refine", tc);
  DC_REQUIRE(S <= DC_MOTION_MAX_SHIFT, DC_EUNSUP, "dc_motion_refine: S = %d: the search radius is limited to %d", S, DC_MOTION_MAX_SHIFT);
  DC_REQUIRE((((uintptr_t)scores) & 7) == 0 && (((uintptr_t)shifts | (uintptr_t)fine) & 3) == 0, DC_EINVAL, "dc_motion_refine: misaligned buffer");
  if (tc == 0) return DC_OK;
  hipLaunchKernelGGL(motion_refine_kernel, dim3((unsigned)dc_cdiv(tc, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const int64_t*)scores, shifts, tc, S, fine);
  DC_CHECK_LAUNCH("dc_motion_refine");
  return DC_OK;
}

extern "C" int dc_motion_block_refine(const long* bscores, const int* rigid, const int* block_shifts, int tc, int By, int Bx, int S, int D,
                                      int* fine, dc_stream_t stream) {
  DC_REQUIRE(bscores && rigid && block_shifts && fine, DC_EINVAL, "dc_motion_block_refine: null pointer");
  DC_REQUIRE(tc >= 0 && S >= 0 && D >= 0 && By > 0 && Bx > 0, DC_EINVAL,
             "dc_motion_block_refine: negative or zero size (tc %d, S %d, D %d, blocks %d x %d)", tc, S, D, By, Bx);
  DC_REQUIRE_FRAMES("dc_motion_block_refine", tc);
  DC_REQUIRE_GRID("dc_motion_block_refine", S, D, By, Bx);
  DC_REQUIRE((((uintptr_t)bscores) & 7) == 0 && (((uintptr_t)rigid | (uintptr_t)block_shifts | (uintptr_t)fine) & 3) == 0, DC_EINVAL,
             "dc_motion_block_refine: misaligned buffer");
  if (tc == 0) return DC_OK;
  const long items = (long)tc * By * Bx, blocks = dc_cdiv(items, kThreads);
  hipLaunchKernelGGL(motion_block_refine_kernel, dim3((unsigned)(blocks < (1L << 20) ? blocks : (1L << 20))), dim3(kThreads), 0,
                     (hipStream_t)stream, (const int64_t*)bscores, rigid, block_shifts, items, By * Bx, S, D, fine);
  DC_CHECK_LAUNCH("dc_motion_block_refine");
  return DC_OK;
}

extern "C" int dc_motion_apply_sub(const void* frames, int is_unsigned, int tc, const int* fine, int H, int W, int fill, void* out,
                                   dc_stream_t stream) {
  DC_REQUIRE(frames && fine && out, DC_EINVAL, "dc_motion_apply_sub: null pointer");
  DC_REQUIRE(tc >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_motion_apply_sub: negative or zero size (tc %d, H %d, W %d)", tc, H, W);
  DC_REQUIRE_FRAMES("dc_motion_apply_sub", tc);
  DC_REQUIRE_IMAGE("dc_motion_apply_sub", H, W);
  DC_REQUIRE_MOVE("dc_motion_apply_sub", frames, fine, out, tc, H, W, fill);
  return launch_apply<true>("dc_motion_apply_sub", frames, is_unsigned ? 0u : 0x8000u, tc, fine, H, W, fill, out, (hipStream_t)stream);
}

extern "C" int dc_motion_warp_sub(const void* frames, int is_unsigned, int tc, const int* fine_block_shifts, int By, int Bx, int H, int W,
                                  int fill, void* out, dc_stream_t stream) {
  DC_REQUIRE(frames && fine_block_shifts && out, DC_EINVAL, "dc_motion_warp_sub: null pointer");
  DC_REQUIRE(tc >= 0 && H > 0 && W > 0 && By > 0 && Bx > 0, DC_EINVAL,
             "dc_motion_warp_sub: negative or zero size (tc %d, H %d, W %d, blocks %d x %d)", tc, H, W, By, Bx);
  DC_REQUIRE_FRAMES("dc_motion_warp_sub", tc);
  DC_REQUIRE_WARP("dc_motion_warp_sub", frames, fine_block_shifts, out, tc, By, Bx, H, W, fill);
  return launch_warp<true>("dc_motion_warp_sub", frames, is_unsigned ? 0u : 0x8000u, tc, fine_block_shifts, By, Bx, H, W, fill, out,
                           (hipStream_t)stream);
}

extern "C" int dc_motion_bin(const void* frames, int is_unsigned, int tc, int H, int W, int c, void* out, dc_stream_t stream) {
  DC_REQUIRE(frames && out, DC_EINVAL, "dc_motion_bin: null pointer");
  DC_REQUIRE(tc >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_motion_bin: negative or zero size (tc %d, H %d, W %d)", tc, H, W);
  DC_REQUIRE_FRAMES("dc_motion_bin", tc);
  const int lg = dc_motion_bin_log2(c);
  DC_REQUIRE(lg > 0, DC_EUNSUP, "dc_motion_bin: c = %d: the binning factor is limited to 2, 4 and 8", c);
  DC_REQUIRE_IMAGE("dc_motion_bin", H, W);
  DC_REQUIRE((H >> lg) > 0 && (W >> lg) > 0, DC_EINVAL, "dc_motion_bin: image %d x %d holds no %d x %d bin", H, W, c, c);
  DC_REQUIRE((((uintptr_t)frames | (uintptr_t)out) & 1) == 0, DC_EINVAL, "dc_motion_bin: misaligned buffer");
  const uintptr_t fb = (uintptr_t)tc * H * W * 2, ob = (uintptr_t)tc * (H >> lg) * (W >> lg) * 2, fa = (uintptr_t)frames, oa = (uintptr_t)out;
  DC_REQUIRE(tc == 0 || fa + fb <= oa || oa + ob <= fa, DC_EINVAL, "dc_motion_bin: out overlaps frames");
  if (tc == 0) return DC_OK;
  const uint16_t* f = (const uint16_t*)frames;
  if (lg == 1) return launch_bin<1>(f, is_unsigned, tc, H, W, (uint16_t*)out, (hipStream_t)stream);
  if (lg == 2) return launch_bin<2>(f, is_unsigned, tc, H, W, (uint16_t*)out, (hipStream_t)stream);
  return launch_bin<3>(f, is_unsigned, tc, H, W, (uint16_t*)out, (hipStream_t)stream);
}

extern "C" int dc_motion_ssd_around(const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int S, int D, const int* rows,
                                    int mult, long* wscores, dc_stream_t stream) {
  DC_REQUIRE(frames && tmpl && rows && wscores, DC_EINVAL, "dc_motion_ssd_around: null pointer");
  DC_REQUIRE(tc >= 0 && S >= 0 && D >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_motion_ssd_around: negative or zero size (tc %d, S %d, D %d, H %d, W %d)",
             tc, S, D, H, W);
  DC_REQUIRE_FRAMES("dc_motion_ssd_around", tc);
  DC_REQUIRE_WINDOW("dc_motion_ssd_around", S, D);
  DC_REQUIRE_IMAGE("dc_motion_ssd_around", H, W);
  DC_REQUIRE(H > 2 * S && W > 2 * S, DC_EINVAL, "dc_motion_ssd_around: image %d x %d has no interior at S = %d (H > 2S and W > 2S)", H, W, S);
  DC_REQUIRE((((uintptr_t)frames | (uintptr_t)tmpl) & 1) == 0 && (((uintptr_t)rows) & 3) == 0 && (((uintptr_t)wscores) & 7) == 0, DC_EINVAL,
             "dc_motion_ssd_around: misaligned buffer");
  return launch_scores("dc_motion_ssd_around", "dc_motion_ssd_around(zero)", frames, is_unsigned, tc, tmpl, H, W, S, D, rows, mult, wscores,
                       (hipStream_t)stream);
}

extern "C" int dc_motion_pick_around(const long* wscores, const int* rows, int mult, int tc, int S, int D, int* shifts, long* best, int* fine,
                                     dc_stream_t stream) {
  DC_REQUIRE(wscores && rows && shifts, DC_EINVAL, "dc_motion_pick_around: null pointer");
  DC_REQUIRE(tc >= 0 && S >= 0 && D >= 0, DC_EINVAL, "dc_motion_pick_around: negative size (tc %d, S %d, D %d)", tc, S, D);
  DC_REQUIRE_FRAMES("dc_motion_pick_around", tc);
  DC_REQUIRE_WINDOW("dc_motion_pick_around", S, D);
  DC_REQUIRE((((uintptr_t)wscores | (uintptr_t)best) & 7) == 0 && (((uintptr_t)rows | (uintptr_t)shifts | (uintptr_t)fine) & 3) == 0, DC_EINVAL,
             "dc_motion_pick_around: misaligned buffer");
  return launch_pick("dc_motion_pick_around", wscores, rows, mult, tc, S, D, shifts, best, fine, (hipStream_t)stream);
}

// ---- bidirectional scan-phase correction ------------------------------------------------------------------------------------------
namespace {

template <int PMAX>
int launch_bidi_scores(const void* frames, int is_unsigned, int tc, int H, int W, int P, unsigned long long* scores, hipStream_t stream) {
  const int tilesX = dc_cdiv(W - 2 * P, kTileW), tilesY = dc_cdiv((H - 1) / 2, kBidiTH);
  const dim3 grid((unsigned)(tilesX * tilesY), frame_dim(tc)), block(kThreads);
  hipLaunchKernelGGL(bidi_scores_kernel<PMAX>, grid, block, bidi_lds(P), stream, (const uint16_t*)frames, is_unsigned ? 0u : 0x8000u, tc, H, W, P,
                     scores, tilesX);
  DC_CHECK_LAUNCH("dc_bidi_scores");
  return DC_OK;
}

}  // namespace

extern "C" int dc_bidi_scores(const void* frames, int is_unsigned, int tc, int H, int W, int P, long* scores, dc_stream_t stream) {
  DC_REQUIRE(frames && scores, DC_EINVAL, "dc_bidi_scores: null pointer");
  DC_REQUIRE(tc >= 0 && P >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_bidi_scores: negative or zero size (tc %d, P %d, H %d, W %d)", tc, P, H, W);
  DC_REQUIRE_FRAMES("dc_bidi_scores", tc);
  DC_REQUIRE(P <= DC_BIDI_MAX_OFFSET, DC_EUNSUP, "dc_bidi_scores: P = %d: the offset radius is limited to %d", P, DC_BIDI_MAX_OFFSET);
  DC_REQUIRE((long)H * W <= (1L << 28), DC_EUNSUP, "dc_bidi_scores: image %d x %d: H * W is limited to 2^28", H, W);
  DC_REQUIRE(H >= 3 && W > 2 * P, DC_EINVAL, "dc_bidi_scores: image %d x %d has no odd line between two even ones, or no interior at P = %d (H >= 3 and W > 2P)",
             H, W, P);
  DC_REQUIRE((((uintptr_t)frames) & 1) == 0 && (((uintptr_t)scores) & 7) == 0, DC_EINVAL, "dc_bidi_scores: misaligned buffer");
  if (tc == 0) return DC_OK;
  // the zero launch (the score kernel leaves its totals by atomics), then the instantiation for the radius
  const long n = (long)tc * (2 * P + 1);
  unsigned long long* sc = (unsigned long long*)scores;
  const int blocks = (int)(dc_cdiv(n, kThreads) < kZeroBlocks ? dc_cdiv(n, kThreads) : kZeroBlocks);
  hipLaunchKernelGGL(motion_zero_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, sc, n);
  DC_CHECK_LAUNCH("dc_bidi_scores(zero)");
  if (P <= 4) return launch_bidi_scores<4>(frames, is_unsigned, tc, H, W, P, sc, (hipStream_t)stream);
  if (P <= 8) return launch_bidi_scores<8>(frames, is_unsigned, tc, H, W, P, sc, (hipStream_t)stream);
  return launch_bidi_scores<16>(frames, is_unsigned, tc, H, W, P, sc, (hipStream_t)stream);
}

extern "C" int dc_bidi_apply(const void* frames, int tc, int p, int H, int W, int fill, void* out, dc_stream_t stream) {
  DC_REQUIRE(frames && out, DC_EINVAL, "dc_bidi_apply: null pointer");
  DC_REQUIRE(tc >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_bidi_apply: negative or zero size (tc %d, H %d, W %d)", tc, H, W);
  DC_REQUIRE_FRAMES("dc_bidi_apply", tc);
  DC_REQUIRE_IMAGE("dc_bidi_apply", H, W);
  DC_REQUIRE_MOVE("dc_bidi_apply", frames, nullptr, out, tc, H, W, fill);
  if (tc == 0) return DC_OK;
  const int bx = dc_cdiv(dc_cdiv((long)H * W + 7, 8), kThreads);
  const dim3 grid((unsigned)(bx < 4096 ? bx : 4096), frame_dim(tc)), block(kThreads);
  hipLaunchKernelGGL(bidi_apply_kernel, grid, block, 0, (hipStream_t)stream, (const uint16_t*)frames, tc, p, H, W, (unsigned)fill & 0xffffu,
                     (uint16_t*)out, (int)dc_aligned16(out));
  DC_CHECK_LAUNCH("dc_bidi_apply");
  return DC_OK;
}
