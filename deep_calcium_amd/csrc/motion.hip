// Rigid motion correction on the device: every frame of a recording (T, H, W) of 16-bit frames is compared with a template at every
// whole-pixel shift (dy, dx) in [-S, S]^2 (dc_motion_ssd: the sum of squared differences over the template's interior), the best
// shift is picked under a total order (dc_motion_pick, motion_math.h) and the frame is moved (dc_motion_apply).  Integer arithmetic
// only: a score is the exact int64 sum, so the chunking of a recording never changes a bit and numpy is an exact oracle.
// Sign convention: out[y][x] = frame[y + dy][x + dx]; a frame cut from a scene at offset (+a, +b) relative to the template is found
// as (dy, dx) = (-a, -b).
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
    if (j < nr) {                                        // wave-uniform
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

// One workgroup per tile of the template's INTERIOR (kWaves * R rows x 512 columns) and frame.  The frame tile with its S-wide halo
// is staged in LDS once (values with the sign bit flipped for int16: both operands move by 32768, the difference does not) and
// reused for all nd^2 shifts; a lane owns kPix consecutive interior pixels of R rows, whose template values stay in registers.
// Per dy the lane keeps one 64-bit sum per dx, the wave adds them by shuffles, lane k takes the total of dx = k - S, and the
// workgroup's nd^2 totals meet in LDS (integer atomics) before ONE 64-bit atomic per shift and workgroup goes to memory (integer
// addition: the order does not matter, the result is bit-reproducible).
template <int SMAX, int R>
__global__ __launch_bounds__(kThreads) void motion_ssd_kernel(const uint16_t* __restrict__ frames, unsigned flip, int tc,
                                                             const uint16_t* __restrict__ tmpl, int H, int W, int S,
                                                             unsigned long long* __restrict__ scores, int tilesX) {
  constexpr int NK = 2 * SMAX + 1, TH = kWaves * R;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nd = 2 * S + 1, stride = ssd_stride(S), rows = TH + 2 * S;
  uint16_t* ft = reinterpret_cast<uint16_t*>(smem);
  unsigned long long* sc = reinterpret_cast<unsigned long long*>(smem + (size_t)rows * stride * sizeof(uint16_t));
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int tx = blockIdx.x % tilesX, ty = blockIdx.x / tilesX;
  const int i0 = tx * kTileW, j0 = ty * TH;              // the tile's first interior pixel = frame coordinates of LDS (0, 0)
  const int IW = W - 2 * S, IH = H - 2 * S;
  const int left = IW - i0 - kPix * lane, down = IH - j0 - wave * R;
  const int np = left < 0 ? 0 : (left < kPix ? left : kPix);      // interior pixels of this lane
  const int nr = down < 0 ? 0 : (down < R ? down : R);            // interior rows of this wave
  const bool ragged = __ballot(np > 0 && np < kPix) != 0;
  unsigned mk[kPix];
#pragma unroll
  for (int p = 0; p < kPix; ++p) mk[p] = p < np ? 0xffffffffu : 0u;
  unsigned t2[R][kPix / 2];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const uint16_t* trow = tmpl + (long)(S + j0 + wave * R + j) * W + S + i0 + kPix * lane;
#pragma unroll
    for (int q = 0; q < kPix / 2; ++q) {
      const unsigned lo = (j < nr && 2 * q < np) ? (trow[2 * q] ^ flip) : 0u;
      const unsigned hi = (j < nr && 2 * q + 1 < np) ? (trow[2 * q + 1] ^ flip) : 0u;
      t2[j][q] = lo | (hi << 16);
    }
  }
  for (int f = blockIdx.y; f < tc; f += gridDim.y) {
    const uint16_t* fr = frames + (long)f * H * W;
    __syncthreads();                                     // the readers of the previous frame's tile and totals are done
    for (int r = wave; r < rows; r += kWaves) {
      const int gy = j0 + r;
      for (int c = lane; c < stride; c += kWave) {
        const int gx = i0 + c;
        ft[r * stride + c] = (gy < H && gx < W) ? (uint16_t)(fr[(long)gy * W + gx] ^ flip) : (uint16_t)0;
      }
    }
    for (int i = threadIdx.x; i < nd * nd; i += kThreads) sc[i] = 0;
    __syncthreads();
    if (nr > 0) {                                        // wave-uniform
      for (int m = 0; m < nd; ++m) {
        unsigned long long acc[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[k] = 0;
        if (np > 0) {
          if (ragged) ssd_rows<SMAX, R, true>(ft, stride, S, nd, nr, wave * R + m, lane, t2, mk, acc);
          else ssd_rows<SMAX, R, false>(ft, stride, S, nd, nr, wave * R + m, lane, t2, mk, acc);
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
    __syncthreads();
    unsigned long long* dst = scores + (long)f * nd * nd;
    for (int i = threadIdx.x; i < nd * nd; i += kThreads) {
      const unsigned long long v = sc[i];
      if (v) atomicAdd(dst + i, v);
    }
  }
}

// One wave per frame: every lane scans the shifts lane, lane + 64, ... and the wave folds its 64 candidates; the order of
// motion_math.h is total, so the result is the unique minimum whatever the order of the comparisons.
__global__ __launch_bounds__(kWave) void motion_pick_kernel(const int64_t* __restrict__ scores, int tc, int S, int* __restrict__ shifts,
                                                           int64_t* __restrict__ best) {
  const int n = (2 * S + 1) * (2 * S + 1), lane = threadIdx.x;
  for (int f = blockIdx.x; f < tc; f += gridDim.x) {
    const int64_t* sc = scores + (long)f * n;
    DcShiftCand b = dc_motion_cand(sc, S, lane < n ? lane : 0);
    for (int i = lane + kWave; i < n; i += kWave) {
      const DcShiftCand c = dc_motion_cand(sc, S, i);
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
    if (lane == 0) {
      shifts[2 * f] = b.dy;
      shifts[2 * f + 1] = b.dx;
      if (best) best[f] = b.score;
    }
  }
}

// out[t][y][x] = frames[t][y + dy][x + dx] inside the frame, fill outside.  A thread moves 8 consecutive output values; the groups
// are cut at multiples of 8 elements of the WHOLE output (not of the frame), so a group that lies in one row is one aligned
// 16-byte store.  Its source run starts at any 2-byte address: it is read as the 4 or 5 aligned dwords that hold it (an aligned
// dword that holds one value of the buffer lies inside the buffer's pages) and funnel-shifted.  Groups that cross a row, a frame
// or the edge of the source go value by value.
__global__ __launch_bounds__(kThreads) void motion_apply_kernel(const uint16_t* __restrict__ frames, int tc, const int* __restrict__ shifts,
                                                               int H, int W, unsigned fill, uint16_t* __restrict__ out, int wide) {
  const int HW = H * W;
  const unsigned fill2 = fill | (fill << 16);
  for (int t = blockIdx.y; t < tc; t += gridDim.y) {
    const long dy = shifts[2 * t], dx = shifts[2 * t + 1];
    const long base = (long)t * HW;
    const int off = (int)(base & 7);
    const int groups = (HW + off + 7) / 8;
    const uint16_t* f = frames + base;
    uint16_t* o = out + base;
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
      const int e0 = g * 8 - off;
      const int a = e0 < 0 ? 0 : e0, b = e0 + 8 < HW ? e0 + 8 : HW;
      int y = a / W, x = a - y * W;
      bool done = false;
      if (wide && b - a == 8 && x + 8 <= W) {
        const long sy = y + dy, sx = x + dx;
        uint4 v;
        if (sy < 0 || sy >= H || sx + 8 <= 0 || sx >= W) {
          v = make_uint4(fill2, fill2, fill2, fill2);
          done = true;
        } else if (sx >= 0 && sx + 8 <= W) {
          const uintptr_t addr = reinterpret_cast<uintptr_t>(f + sy * W + sx);
          const unsigned* p = reinterpret_cast<const unsigned*>(addr & ~(uintptr_t)3);
          const unsigned w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3];
          if (addr & 2) {
            const unsigned w4 = p[4];
            v = make_uint4((w0 >> 16) | (w1 << 16), (w1 >> 16) | (w2 << 16), (w2 >> 16) | (w3 << 16), (w3 >> 16) | (w4 << 16));
          } else {
            v = make_uint4(w0, w1, w2, w3);
          }
          done = true;
        }
        if (done) *reinterpret_cast<uint4*>(o + a) = v;
      }
      if (!done) {
        for (int e = a; e < b; ++e) {
          const long sy = y + dy, sx = x + dx;
          o[e] = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? f[sy * W + sx] : (uint16_t)fill;
          if (++x == W) { x = 0; ++y; }
        }
      }
    }
  }
}

template <int SMAX, int R>
int launch_ssd(const uint16_t* frames, int is_unsigned, int tc, const uint16_t* tmpl, int H, int W, int S, unsigned long long* scores,
               hipStream_t stream) {
  static DcLdsAttr lds_attr;
  const int TH = kWaves * R;
  const int nd = 2 * S + 1;
  const int lds = (TH + 2 * S) * ssd_stride(S) * (int)sizeof(uint16_t) + nd * nd * (int)sizeof(unsigned long long);
  const int lds_max = (TH + 2 * SMAX) * ssd_stride(SMAX) * (int)sizeof(uint16_t) + (2 * SMAX + 1) * (2 * SMAX + 1) * (int)sizeof(unsigned long long);
  auto kern = motion_ssd_kernel<SMAX, R>;
  if (int rc = dc_func_max_lds(lds_attr, reinterpret_cast<const void*>(kern), lds_max, "dc_motion_ssd")) return rc;
  const int tilesX = dc_cdiv(W - 2 * S, kTileW), tilesY = dc_cdiv(H - 2 * S, TH);
  const dim3 grid((unsigned)(tilesX * tilesY), (unsigned)(tc < 65535 ? tc : 65535)), block(kThreads);
  hipLaunchKernelGGL(kern, grid, block, lds, stream, frames, is_unsigned ? 0u : 0x8000u, tc, tmpl, H, W, S, scores, tilesX);
  DC_CHECK_LAUNCH("dc_motion_ssd");
  return DC_OK;
}

}  // namespace

extern "C" int dc_motion_ssd(const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int S, long* scores,
                             dc_stream_t stream) {
  DC_REQUIRE(frames && tmpl && scores, DC_EINVAL, "dc_motion_ssd: null pointer");
  DC_REQUIRE(tc >= 0 && S >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_motion_ssd: negative or zero size (tc %d, S %d, H %d, W %d)", tc, S, H, W);
  DC_REQUIRE(S <= DC_MOTION_MAX_SHIFT, DC_EUNSUP, "dc_motion_ssd: S = %d: the search radius is limited to %d", S, DC_MOTION_MAX_SHIFT);
  DC_REQUIRE((long)H * W <= (1L << 30), DC_EUNSUP, "dc_motion_ssd: image %d x %d: H * W is limited to 2^30", H, W);
  DC_REQUIRE(H > 2 * S && W > 2 * S, DC_EINVAL, "dc_motion_ssd: image %d x %d has no interior at S = %d (H > 2S and W > 2S)", H, W, S);
  DC_REQUIRE((((uintptr_t)frames | (uintptr_t)tmpl) & 1) == 0 && (((uintptr_t)scores) & 7) == 0, DC_EINVAL, "dc_motion_ssd: misaligned buffer");
  if (tc == 0) return DC_OK;
  const long n = (long)tc * (2 * S + 1) * (2 * S + 1);
  unsigned long long* sc = (unsigned long long*)scores;
  const int blocks = (int)(dc_cdiv(n, kThreads) < kZeroBlocks ? dc_cdiv(n, kThreads) : kZeroBlocks);
  hipLaunchKernelGGL(motion_zero_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, sc, n);
  DC_CHECK_LAUNCH("dc_motion_ssd(zero)");
  const uint16_t* f = (const uint16_t*)frames;
  const uint16_t* t = (const uint16_t*)tmpl;
  if (S <= 4) return launch_ssd<4, 8>(f, is_unsigned, tc, t, H, W, S, sc, (hipStream_t)stream);
  if (S <= 8) return launch_ssd<8, 8>(f, is_unsigned, tc, t, H, W, S, sc, (hipStream_t)stream);
  return launch_ssd<16, 4>(f, is_unsigned, tc, t, H, W, S, sc, (hipStream_t)stream);
}

extern "C" int dc_motion_pick(const long* scores, int tc, int S, int* shifts, long* best, dc_stream_t stream) {
  DC_REQUIRE(scores && shifts, DC_EINVAL, "dc_motion_pick: null pointer");
  DC_REQUIRE(tc >= 0 && S >= 0, DC_EINVAL, "dc_motion_pick: negative size (tc %d, S %d)", tc, S);
  DC_REQUIRE(S <= DC_MOTION_MAX_SHIFT, DC_EUNSUP, "dc_motion_pick: S = %d: the search radius is limited to %d", S, DC_MOTION_MAX_SHIFT);
  DC_REQUIRE((((uintptr_t)scores | (uintptr_t)best) & 7) == 0 && (((uintptr_t)shifts) & 3) == 0, DC_EINVAL, "dc_motion_pick: misaligned buffer");
  if (tc == 0) return DC_OK;
  hipLaunchKernelGGL(motion_pick_kernel, dim3((unsigned)(tc < 65535 ? tc : 65535)), dim3(kWave), 0, (hipStream_t)stream,
                     (const int64_t*)scores, tc, S, shifts, (int64_t*)best);
  DC_CHECK_LAUNCH("dc_motion_pick");
  return DC_OK;
}

extern "C" int dc_motion_apply(const void* frames, int tc, const int* shifts, int H, int W, int fill, void* out, dc_stream_t stream) {
  DC_REQUIRE(frames && shifts && out, DC_EINVAL, "dc_motion_apply: null pointer");
  DC_REQUIRE(tc >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_motion_apply: negative or zero size (tc %d, H %d, W %d)", tc, H, W);
  DC_REQUIRE((long)H * W <= (1L << 30), DC_EUNSUP, "dc_motion_apply: image %d x %d: H * W is limited to 2^30", H, W);
  DC_REQUIRE(fill >= -32768 && fill <= 65535, DC_EINVAL, "dc_motion_apply: fill = %d is not a 16-bit value", fill);
  DC_REQUIRE((((uintptr_t)frames | (uintptr_t)out) & 1) == 0 && (((uintptr_t)shifts) & 3) == 0, DC_EINVAL, "dc_motion_apply: misaligned buffer");
  const uintptr_t bytes = (uintptr_t)tc * H * W * 2, fa = (uintptr_t)frames, oa = (uintptr_t)out;
  DC_REQUIRE(bytes == 0 || fa + bytes <= oa || oa + bytes <= fa, DC_EINVAL, "dc_motion_apply: out overlaps frames");
  if (tc == 0) return DC_OK;
  const int groups = dc_cdiv((long)H * W + 7, 8);
  const int bx = dc_cdiv(groups, kThreads);
  const dim3 grid((unsigned)(bx < 4096 ? bx : 4096), (unsigned)(tc < 65535 ? tc : 65535)), block(kThreads);
  hipLaunchKernelGGL(motion_apply_kernel, grid, block, 0, (hipStream_t)stream, (const uint16_t*)frames, tc, shifts, H, W,
                     (unsigned)fill & 0xffffu, (uint16_t*)out, (int)((oa & 15) == 0));
  DC_CHECK_LAUNCH("dc_motion_apply");
  return DC_OK;
}
