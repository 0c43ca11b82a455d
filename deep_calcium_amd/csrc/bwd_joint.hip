// Joint backward of a 512^2-class conv block (Conv2D(32 -> 32, 3x3) -> BatchNorm -> ReLU, no Dropout:
// /root/reference/deepcalcium/models/neurons/unet_2d_summary.py:163-167, instances e0b and d0b): ONE kernel stages a
// halo'd tile of dz (formed on load from da and z, dc_bn_bwd_finalize_dzin's table) and of the block input x (BN + ReLU
// on load when the producer's activation is not materialised) ONCE and produces BOTH the data gradient dx and the
// weight-gradient slab.  These layers are HBM-bound end to end (arithmetic intensity 72 flop/byte against a machine
// balance of ~130): the separate data- and weight-gradient kernels read (da, z) twice and x once; here every tensor is
// read once -- da + z + x + dx = 4 tensor passes instead of 7.
//
// One persistent 512-thread workgroup per CU, 4 x 32-pixel tiles (halo'd 6 x 34), fixed wave roles:
//   waves 4-7  producers: request tile t+2's rows (buffer loads, zeros outside the image), form dz / relu(bn(x)) of tile
//              t+1, split into fp16 hi/lo and write the two LDS images of the other stage ([hi|lo][pixel][32 ch] rows
//              of 64 bytes, 16-byte chunks XOR-swizzled by (pixel >> 2) & 3);
//   waves 0-1  data gradient: each owns two pixel rows (2 blocks of 32 px x 32 cin), A = dz at the 9 shifted windows
//              (ds_read_b128, conflict-free through the swizzle), B = the packed weights, resident in LDS for the whole
//              launch; per tile: 108 MFMAs, then the epilogue (dx stores + the BatchNorm-backward sums of the layer in
//              front, accumulated over ALL tiles of the workgroup in registers: one partial row per wave);
//   waves 2-3  weight gradient: each owns two pixel rows as its slice of the contraction, fragments through the
//              transposing ds_read_b64_tr_b16 from the SAME two images, 9 x 16 accumulators kept for the whole launch;
//              per tile: 108 MFMAs.  The two slices are summed through LDS at the end, one slab per workgroup.
// Numerics: those of igemm_f16x3.hip / wgrad_f16x3.hip (split-fp16 operands, power-of-two range-guard scales undone in
// the epilogues, fp32 accumulation); the summation order differs from the separate kernels (tile shape), same tolerance.
// bwd_joint32_kernel<true> (d0b under the head): da = kd (x) s has rank one -- the producers load s (4 bytes per pixel) and form da.
#include <type_traits>
#include "wgrad_common.h"
#include "f16x3_common.h"

// DC_JOINT_ABL (timing experiments only, results are garbage): 1 data-gradient waves skip their MFMA block, 2 weight-gradient
// waves skip theirs, 4 producers do not split / write LDS, 8 producers do not load
#ifndef DC_JOINT_ABL
#define DC_JOINT_ABL 0
#endif

struct JointParams {
  const float* x; const float* xSc; const float* xSh; const float* xAbound;
  const float* da; const float* z; const float* dzCoef;
  const float* s; const float* kh;      // rank-one da (bwd_joint32_kernel<true>): da[pix][c] = (kh[c][1] - kh[c][0]) * s[pix], da unused
  const float* wp;
  float* dx;
  const float* redZ; const float* redMean; const float* redInvstd; const float* redGamma; const float* redBeta;
  float* bnPartial; float* bnAmax;
  float* slabs;
  int N, H, W, tilesX, tilesY;
};

namespace bj {
constexpr int C = 32;
constexpr int TH = 4, TW = 32, THI = TH + 2, TWI = TW + 2, NPIX = THI * TWI;      // 204 halo'd pixels
// An fp16 image of the halo'd tile: [hi | lo plane][pixel][ROW bytes of channels], 16-byte chunks XOR-swizzled.
struct Rows64 {          // 32 channels (dz; x of the 32 -> 32 kernel)
  static constexpr int ROW = 64, PLANE = 13312;     // NPIX * 64 bytes rounded up to a multiple of 1024 (the swizzle reads address bits 8-9)
  // 16-byte chunk c of pixel p lives at chunk c ^ ((p >> 2) & 3): eight consecutive pixels read the same chunk of
  // their 64-byte rows from eight different bank groups; a 4-aligned pixel group keeps its chunks together (tr reads)
  static __device__ __forceinline__ int swz(int rel) { return rel ^ ((rel >> 4) & 0x30); }
};
struct Rows128 {         // 64 channels (x of the 64 -> 32 kernel)
  static constexpr int ROW = 128, PLANE = 26624;    // NPIX * 128 bytes rounded up to a multiple of 1024
  static __device__ __forceinline__ int swz(int rel) { return rel ^ ((rel >> 2) & 0x40); }     // chunk ^= 4 * bit 1 of the pixel
};
constexpr int PLANE = Rows64::PLANE;
constexpr int IMG = 2 * PLANE;               // hi | lo
constexpr int RAW = TH * TW * C * 4;          // the tile's interior x values as loaded (fp32): the pre-BN tensor of the layer in front
constexpr int STAGE = 2 * IMG + RAW;         // dz image | x image | raw interior x
constexpr int W_SLOTS = 9 * 4 * 2 * C;       // packed data-gradient weights: [tap][k8][hi|lo][col] 16-byte slots
constexpr int LDS_BYTES = 2 * STAGE + 64;
constexpr int THREADS = 512;
constexpr int NL = (NPIX * 8 + 255) / 256;   // float4 loads per producer thread and tensor (7)
constexpr unsigned OOB = 0x80000000u;
static_assert(LDS_BYTES <= 160 * 1024 && NPIX * 64 <= PLANE && PLANE % 1024 == 0 && STAGE % 1024 == 0, "LDS plan");

// This workgroup's tiles: each XCD walks a contiguous range of the (image, column, row) list -- consecutive positions
// are vertically adjacent tiles whose halo rows overlap --, its workgroups striding through it (igemm_pp.hip)
struct Tile { int img, y0, x0; };
__device__ __forceinline__ DcXcdRange tile_range(const JointParams& p) {
  return dc_xcd_range(blockIdx.x, (int)gridDim.x, p.N * p.tilesX * p.tilesY);
}
__device__ __forceinline__ Tile decode(const JointParams& p, const DcXcdRange& tiles, int j) {
  const int work = tiles.work(j);
  const int ty = work % p.tilesY, t2 = work / p.tilesY;
  Tile t;
  t.x0 = (t2 % p.tilesX) * TW; t.img = t2 / p.tilesX; t.y0 = ty * TH;
  return t;
}
// image position of halo'd pixel `pix` of a tile; false outside the image and for the slots behind the tile's last pixel
__device__ __forceinline__ bool halo_pixel(const JointParams& p, const Tile& tl, int pix, int& y, int& xx) {
  const int r = __umul24(pix, (65536 + TWI - 1) / TWI) >> 16;          // pix / TWI
  const int c = pix - __umul24(r, TWI);
  y = tl.y0 - 1 + r; xx = tl.x0 - 1 + c;
  return pix < NPIX && (unsigned)y < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
}

// The dz producer: thread t of the 256 holds channel quad q = t & 7 of the pixels pb + 32 k, pb = t >> 3 -- its rows of
// dc_bn_bwd_finalize_dzin's table, the (da, z) request and the dz image of a stage.
// R1 (rank-one da: the block under the head, whose gradient is kd (x) s): the request reads the pixel's s (one dword, the same
// address in the eight lanes of a pixel) instead of its da row and stage() forms da = kd[c] * s, ONE rounding as the head's store
// (head_bwd_pixel, elementwise.hip), before dc_dz_on_load: bit for bit the dz of the materialised da.
template <bool R1>
struct DzProducerT {
  using Ra = typename std::conditional<R1, float, f32x4>::type;      // what a pixel's request of da brings
  int q, pb;
  f32x4 sc, sh, mu, A, D, E;
  f32x4 kd;                                                           // R1: kh[c][1] - kh[c][0] of this thread's channel quad (head_lane)
  __device__ __forceinline__ DzProducerT(const float* coef, int t, const float* kh = nullptr) : q(t & 7), pb(t >> 3) {
    const float* ct = coef + 4 * q;
    sc = *reinterpret_cast<const f32x4*>(ct); sh = *reinterpret_cast<const f32x4*>(ct + C);
    mu = *reinterpret_cast<const f32x4*>(ct + 2 * C); A = *reinterpret_cast<const f32x4*>(ct + 3 * C);
    D = *reinterpret_cast<const f32x4*>(ct + 4 * C); E = *reinterpret_cast<const f32x4*>(ct + 5 * C);
    kd = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (R1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) kd[e] = kh[(4 * q + e) * 2 + 1] - kh[(4 * q + e) * 2];
    }
  }
  // live: bit k = pixel pb + 32 k lies inside the image (the x request of the same tile asks for the same pixels)
  __device__ __forceinline__ void request(const JointParams& p, const Tile& tl, Ra (&ra)[NL], f32x4 (&rz)[NL], unsigned& live) const {
    live = 0u;
    const long img_floats = (long)p.H * p.W * C, img_pixels = (long)p.H * p.W;
    const __amdgpu_buffer_rsrc_t rsA = R1 ? dc_make_rsrc(p.s + tl.img * img_pixels, (unsigned)(img_pixels * 4))
                                          : dc_make_rsrc(p.da + tl.img * img_floats, (unsigned)(img_floats * 4));
    const __amdgpu_buffer_rsrc_t rsZ = dc_make_rsrc(p.z + tl.img * img_floats, (unsigned)(img_floats * 4));
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      int y, xx;
      const bool ok = halo_pixel(p, tl, pb + 32 * k, y, xx);
      const unsigned off = ok ? (unsigned)(((y * p.W + xx) * C + 4 * q) * 4) : OOB;
      if constexpr (R1) {
        // the pixel's byte offset in s from the SAME select as the row offset (pixel * 128 + 16 q -> pixel * 4): plain ALU, so the
        // request stays the straight-line code of the materialised variant (a second select was compiled into branches around
        // the loads, with full vmcnt drains).  OOB >> 5 = 2^26 lies behind any image this kernel serves (H * W * 4 < 2^26).
        const unsigned offs = (off >> 5) & ~3u;
        ra[k] =__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsA, offs, 0, 0));
      } else {
        ra[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, off, 0, 0));
      }
      rz[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsZ, off, 0, 0));
      if (ok) live |= 1u << k;
    }
  }
  __device__ __forceinline__ void stage(const Ra (&ra)[NL], const f32x4 (&rz)[NL], unsigned live, float dz_scale, char* set) const {
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int pix = pb + 32 * k;
      const bool lv = (live >> k) & 1u;
      f32x4 dav;
      if constexpr (R1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) dav[e] = __fmul_rn(kd[e], ra[k]);      // rounds on its own: never fused into dz's fma
      } else {
        dav = ra[k];
      }
      f32x4 dzv;
#pragma unroll
      for (int e = 0; e < 4; ++e)         // outside the image dz is zero, not E - D*mu
        dzv[e] = lv ? dc_dz_on_load(rz[k][e], dav[e], sc[e], sh[e], mu[e], A[e], D[e], E[e]) : 0.f;
      u32x2 dh, dl;
      dc_split_f16(dzv, dz_scale, dh, dl);
      if (pix < NPIX) {
        const int off = Rows64::swz(pix * 64 + q * 8);
        *reinterpret_cast<u32x2*>(set + off) = dh;
        *reinterpret_cast<u32x2*>(set + PLANE + off) = dl;
      }
    }
  }
};
using DzProducer = DzProducerT<false>;

// The producers' schedule over two LDS stages of STAGE_BYTES.  x: two register sets (tile t+2 in flight while t+1 is split);
// (da, z): one set, requested right after the previous tile's has been split -- one tile of MFMA time ahead (wgrad_f16x3.hip's
// B1 scheme: 2 x (x + da + z) does not fit).  request_x(j, set) / stage_x(set, stage) / request_dz(j) / stage_dz(stage).
template <int STAGE_BYTES, class X, class RX, class RD, class SX, class SD>
__device__ __forceinline__ void produce(char* smem, int nt, X& x0, X& x1, RX request_x, RD request_dz, SX stage_x, SD stage_dz) {
  constexpr bool LOAD = !(DC_JOINT_ABL & 8), SPLIT = !(DC_JOINT_ABL & 4);
  if (nt > 0) {
    request_x(0, x0);
    request_dz(0);
    if (nt > 1) request_x(1, x1);
    stage_x(x0, smem);
    stage_dz(smem);
    if (nt > 1) request_dz(1);
  }
  __syncthreads();
  for (int i = 0; i < nt; i += 2) {
    if (LOAD && i + 2 < nt) request_x(i + 2, x0);
    if (SPLIT && i + 1 < nt) { stage_x(x1, smem + STAGE_BYTES); stage_dz(smem + STAGE_BYTES); }
    if (LOAD && i + 2 < nt) request_dz(i + 2);
    __syncthreads();
    if (i + 1 < nt) {
      if (LOAD && i + 3 < nt) request_x(i + 3, x1);
      if (SPLIT && i + 2 < nt) { stage_x(x0, smem); stage_dz(smem); }
      if (LOAD && i + 3 < nt) request_dz(i + 3);
      __syncthreads();
    }
  }
}

// Data gradient, group g = (tap, 16-channel half): the dz fragments of a wave's two pixel rows (lane offsets ar0, ar1) at
// the tap's shifted window (ds_read_b128, conflict-free through the swizzle)
__device__ __forceinline__ void fetch_dz_window(const char* cur, int g, int ar0, int ar1, f16x8 (&ah)[2], f16x8 (&al)[2]) {
  const int tap = g >> 1, ks = g & 1;
  const int toff = ((tap / 3) * TWI + (tap % 3)) * 64 + ks * 32;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const int ao = Rows64::swz((mb ? ar1 : ar0) + toff);
    ah[mb] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(cur + ao));
    al[mb] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(cur + PLANE + ao));
  }
}

// Weight gradient of one staged tile: NG (k-step, tap) groups of 3 MFMAs into the 9 tap accumulators, k-step = (row, 16-pixel
// half); A = the x image (layout XR, behind the dz image) at the tap's shifted window, B = dz, both through the transposing
// reads.  The x fragments of group g+1 (and the dz fragments of the next k-step) are requested before the MFMAs of group g
// issue.  lx / lz: the lane's byte offset inside the x / dz image (first row of its slice, its group of 4 contraction
// pixels, its chunk).
template <class XR, int NG>
__device__ __forceinline__ void wgrad_tile(const char* cur, int lx, int lz, f32x16 (&acc)[9]) {
  f16x8 ah[2], al[2], bh[2], bl[2];
  auto fetch_a = [&](int g, int buf) __attribute__((always_inline)) {
    const int ks = g / 9, tap = g % 9;
    const int r = ks >> 1, xs = ks & 1;
    const int pbase = lx + ((r + tap / 3) * TWI + 16 * xs + tap % 3) * XR::ROW;
    const int a0 = XR::swz(pbase), a1 = XR::swz(pbase + 4 * XR::ROW);
    ah[buf] = dc_tr_frag(cur + IMG, a0, a1);
    al[buf] = dc_tr_frag(cur + IMG + XR::PLANE, a0, a1);
  };
  auto fetch_b = [&](int ks, int buf) __attribute__((always_inline)) {
    const int r = ks >> 1, xs = ks & 1;
    const int brel = lz + ((r + 1) * TWI + 16 * xs + 1) * 64;
    const int b0 = Rows64::swz(brel), b1 = Rows64::swz(brel + 4 * 64);
    bh[buf] = dc_tr_frag(cur, b0, b1);
    bl[buf] = dc_tr_frag(cur + PLANE, b0, b1);
  };
  fetch_b(0, 0);
  fetch_a(0, 0);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int ca = g & 1, ks = g / 9, tap = g % 9, cbuf = ks & 1;
    if (g + 1 < NG) {
      fetch_a(g + 1, ca ^ 1);
      if ((g + 1) % 9 == 0) fetch_b(ks + 1, cbuf ^ 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    dc_mfma3(ah[ca], al[ca], bh[cbuf], bl[cbuf], acc[tap]);
    __builtin_amdgcn_sched_barrier(0);
  }
}
}  // namespace bj

template <bool R1>
__global__ __launch_bounds__(bj::THREADS, 1) void bwd_joint32_kernel(JointParams p) {
  using namespace bj;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  float* tmp = reinterpret_cast<float*>(smem + 2 * STAGE);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0..7

  const float x_scale = dc_block_guard_scale(p.xAbound, C, tmp);
  const float dz_scale = dc_block_guard_scale(p.dzCoef + 6 * C, C, tmp);
  const float w_scale = p.wp[W_SLOTS * 4];                         // trailer of the packed weights
  // the layer in front's pre-BN values for its fused sums: when that tensor IS the x operand (BN + ReLU on load: x = its z) the
  // producers leave the tile's interior values in LDS as they loaded them -- no second trip to HBM (537 MB per launch less)
  const bool red_lds = p.redZ != nullptr && p.redZ == p.x;
  const DcXcdRange tiles = tile_range(p);
  const int nt = tiles.nt;
  const long img_floats = (long)p.H * p.W * C;

  if (wave >= 4) {
    // ============================ producers: HBM -> registers -> the two fp16 hi/lo images =============================
    const DzProducerT<R1> dzp(p.dzCoef, tid & 255, p.kh);
    const int q = dzp.q, pb = dzp.pb;                              // x: the same channel quad and pixels as dz
    const bool xbn = p.xSc != nullptr;
    f32x4 x_sc = {1.f, 1.f, 1.f, 1.f}, x_sh = {0.f, 0.f, 0.f, 0.f};
    if (xbn) { x_sc = *reinterpret_cast<const f32x4*>(p.xSc + 4 * q); x_sh = *reinterpret_cast<const f32x4*>(p.xSh + 4 * q); }
    // the image positions of this thread's NL pixels are recomputed per request
    // (registers: the two x sets + one (da, z) set + the per-channel tables are what the producers hold)
    f32x4 rx0[NL], rx1[NL], rz[NL];
    typename DzProducerT<R1>::Ra ra[NL];
    unsigned live = 0u;                                           // of the tile whose (da, z) are in ra, rz: the one staged next
    auto request_x = [&](int j, f32x4 (&rx)[NL]) __attribute__((always_inline)) {
      const Tile tl = decode(p, tiles, j);
      const __amdgpu_buffer_rsrc_t rsX = dc_make_rsrc(p.x + tl.img * img_floats, (unsigned)(img_floats * 4));
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        int y, xx;
        const bool ok = halo_pixel(p, tl, pb + 32 * k, y, xx);
        const unsigned off = ok ? (unsigned)(((y * p.W + xx) * C + 4 * q) * 4) : OOB;
        rx[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsX, off, 0, 0));
      }
    };
    auto stage_x = [&](const f32x4 (&rx)[NL], char* set) __attribute__((always_inline)) {
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        const int pix = pb + 32 * k;
        const bool lv = (live >> k) & 1u;
        f32x4 xv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xr = rx[k][e];
          xv[e] = xbn ? (lv ? fmaxf(__builtin_fmaf(xr, x_sc[e], x_sh[e]), 0.f) : 0.f) : xr;     // zero padding stays zero
        }
        u32x2 xh, xl;
        dc_split_f16(xv, x_scale, xh, xl);
        if (pix < NPIX) {
          const int off = Rows64::swz(pix * 64 + q * 8);
          *reinterpret_cast<u32x2*>(set + IMG + off) = xh;
          *reinterpret_cast<u32x2*>(set + IMG + PLANE + off) = xl;
          if (red_lds) {
            const int r = __umul24(pix, (65536 + TWI - 1) / TWI) >> 16, c = pix - __umul24(r, TWI);
            if (r >= 1 && r <= TH && c >= 1 && c <= TW)
              *reinterpret_cast<f32x4*>(set + 2 * IMG + (((r - 1) * TW + (c - 1)) * C + 4 * q) * 4) = rx[k];
          }
        }
      }
    };
    produce<STAGE>(smem, nt, rx0, rx1, request_x,
                   [&](int j) __attribute__((always_inline)) { dzp.request(p, decode(p, tiles, j), ra, rz, live); },
                   stage_x, [&](char* set) __attribute__((always_inline)) { dzp.stage(ra, rz, live, dz_scale, set); });
#pragma unroll 1
    for (int k = 0; k < 2 * 9; ++k) __syncthreads();             // the weight-gradient waves' cross-slice reduction
    return;
  }

  const int li = lane & 31, h = lane >> 5;
  if (wave < 2) {
    // ================================ data gradient: 2 rows x 32 px x 32 cin per tile ==================================
    const int wd = wave;
    const float out_scale = 1.f / (dz_scale * w_scale);
    const bool red = p.redZ != nullptr;
    float gsc = 0.f, gsh = 0.f, rmu = 0.f, ris = 0.f;
    if (red) {
      rmu = p.redMean[li]; ris = p.redInvstd[li];
      dc_bn_affine(rmu, ris, p.redGamma[li], p.redBeta[li], gsc, gsh);
    }
    float s1 = 0.f, s2 = 0.f, amax = 0.f;                        // this lane's channel, all tiles of the workgroup
    int a_rel[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) a_rel[mb] = ((2 * wd + mb) * TWI + li) * 64 + h * 16;
    // the 36 weight fragments of this lane (tap, 16-channel half, hi | lo) live in registers for the whole launch: they are the
    // same for every tile, and the LDS they occupied now holds the raw interior x values
    u32x4 wreg[18][2];
    {
      const u32x4* wsrc = reinterpret_cast<const u32x4*>(p.wp) + h * 64 + li;      // slot ((tap*4 + ks*2 + h)*2 + hl)*32 + li
#pragma unroll
      for (int g = 0; g < 18; ++g) {
        wreg[g][0] = wsrc[(g >> 1) * 256 + (g & 1) * 128];
        wreg[g][1] = wsrc[(g >> 1) * 256 + (g & 1) * 128 + 32];
      }
    }
    __syncthreads();                                             // stage 0 is in LDS
    for (int i = 0; i < nt; ++i) {
      const char* cur = smem + (i & 1) * STAGE;
      int ar0 = a_rel[0], ar1 = a_rel[1];
      asm volatile("" : "+v"(ar0), "+v"(ar1));     // opaque per tile: or the 36 swizzled offsets are hoisted and spilled
      f32x16 acc[2];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mb][r] = 0.f;
      const Tile tl = decode(p, tiles, i);
      const __amdgpu_buffer_rsrc_t rsO = dc_make_rsrc(p.dx + tl.img * img_floats, (unsigned)(img_floats * 4));
      __builtin_amdgcn_s_setprio(2);
      {
        // 18 (tap, 16-channel half) groups of 6 MFMAs; the 6 fragments of group g+1 are requested from LDS before the MFMAs
        // of group g issue (one wave per SIMD feeds the pipe: without the explicit double buffer every group paid the LDS
        // latency -- the consumer side alone ran at 45 % of the MFMA issue rate)
        constexpr int NG = (DC_JOINT_ABL & 1) ? 2 : 18;
        f16x8 ah[2][2], al[2][2];
        fetch_dz_window(cur, 0, ar0, ar1, ah[0], al[0]);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const int b = g & 1;
          if (g + 1 < NG) fetch_dz_window(cur, g + 1, ar0, ar1, ah[b ^ 1], al[b ^ 1]);
          __builtin_amdgcn_sched_barrier(0);
          const f16x8 bh = __builtin_bit_cast(f16x8, wreg[g][0]), bl = __builtin_bit_cast(f16x8, wreg[g][1]);
#pragma unroll
          for (int mb = 0; mb < 2; ++mb) dc_mfma3(ah[b][mb], al[b][mb], bh, bl, acc[mb]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
      // ---- epilogue: dx stores (lane = cin channel li, registers = pixels) + the sums of the layer in front ----------
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
        const int oy = tl.y0 + 2 * wd + mb, oxb = tl.x0 + 4 * h;
        const bool row_ok = oy < p.H;
        unsigned offs[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int colc = (r & 3) + 8 * (r >> 2);
          const bool ok = row_ok && (oxb + colc) < p.W;
          offs[r] = ok ? (unsigned)(((oy * p.W + oxb + colc) * C + li) * 4) : OOB;
        }
        float zr[16];
        if (red_lds) {                        // the producers left this tile's interior x (= that layer's z) in LDS
          const float* raw = reinterpret_cast<const float*>(cur + 2 * IMG) + ((2 * wd + mb) * TW + 4 * h) * C + li;
#pragma unroll
          for (int r = 0; r < 16; ++r) zr[r] = raw[((r & 3) + 8 * (r >> 2)) * C];
        } else if (red) {                     // another tensor: requested here, the stores of this block go out while they fly
          // (requesting them a tile ahead / before the MFMA block was measured slower: they compete with the producers' prefetch)
          const __amdgpu_buffer_rsrc_t rsR = dc_make_rsrc(p.redZ + tl.img * img_floats, (unsigned)(img_floats * 4));
#pragma unroll
          for (int r = 0; r < 16; ++r) zr[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsR, offs[r], 0, 0));
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = acc[mb][r] * out_scale;
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsO, offs[r], 0, 0);
        }
        if (red) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            dc_bnred_accum(acc[mb][r] * out_scale, zr[r], gsc, gsh, rmu, ris, !(offs[r] >> 31), s1, s2, amax);
        }
      }
      __syncthreads();
    }
    if (red) {
      s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32); amax = fmaxf(amax, __shfl_xor(amax, 32));
      if (h == 0) {
        const long row = (long)blockIdx.x * 2 + wd;
        p.bnPartial[(row * C + li) * 2] = s1;
        p.bnPartial[(row * C + li) * 2 + 1] = s2;
        if (p.bnAmax) p.bnAmax[row * C + li] = amax;
      }
    }
#pragma unroll 1
    for (int k = 0; k < 2 * 9; ++k) __syncthreads();
    return;
  }

  // ================================== weight gradient: 2 rows of every tile as the contraction slice ====================
  const int ww = wave - 2;
  const int cb = (lane >> 4) & 1, c16 = lane & 15, q4 = c16 >> 2, pp = c16 & 3;
  const int frag = (cb * 2 + (pp >> 1)) * 16 + (pp & 1) * 8;     // 16-channel half, channel quad inside it
  // lane's byte offset inside the image: its wave's first row, its first group of 4 contraction pixels (x = 8h + q4), its chunk
  const int lane_rel = (2 * ww * TWI + 8 * h + q4) * 64 + frag;
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  __syncthreads();
  for (int i = 0; i < nt; ++i) {
    const char* cur = smem + (i & 1) * STAGE;
    int lrel = lane_rel;
    asm volatile("" : "+v"(lrel));               // opaque per tile: or the 80 swizzled offsets are hoisted and spilled
    __builtin_amdgcn_s_setprio(2);
    wgrad_tile<Rows64, (DC_JOINT_ABL & 2) ? 2 : 36>(cur, lrel, lrel, acc);      // 4 k-steps: this wave's two rows x two 16-pixel halves
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }
  WgradParams wp;
  wp.slabs = p.slabs; wp.Cm = C; wp.Cn = C;
  wgrad_store<9, 1, 1, 2>(wp, acc, smem, (int)blockIdx.x, 0, 0, 0, 0, ww, lane, 1.f / (x_scale * dz_scale));
}

// ---------------------------------------------------------------------------------------------------------------------
// The 64 -> 32 block of the same resolution (d0a: x = the 64-channel concat buffer, materialised; dx = its gradient, which
// feeds a Dropout block and the max-pool backward: no fused sums).  Same tiles, same dz image; differences:
//   * the x image has 128-byte pixel rows (64 channels: 8 chunks, XOR-swizzled with bit 1 of the pixel index: the
//     transposing reads of 4 consecutive pixels then cover all 64 banks); two stages of (dz + x) fill the LDS (156 KB), so
//   * the data-gradient weights (74 KB) are NOT LDS-resident: the 72 fragments a tile needs are read from global memory
//     (L2-resident, the same for every workgroup), three (tap, k-step) groups ahead of the MFMAs that use them;
//   * data gradient: waves 0-1, two rows each x 64 cin columns (2 x 2 blocks: the weight fragments are shared by two row
//     blocks, the dz fragments by two column blocks); weight gradient: wave 2 + ww owns the 32 input channels [32 ww, 32 ww + 32)
//     for ALL four rows and all 9 taps (144 accumulators): no cross-wave reduction, each writes its half of the slab.
// Per tile and consumer wave 216 MFMAs; fragment reads 464 KB per tile = 52 % of the LDS bandwidth at full MFMA rate.
namespace bj64 {
using namespace bj;
constexpr int CX = 64;                         // x / dx channels
constexpr int XPLANE = Rows128::PLANE;
constexpr int XIMG = 2 * XPLANE;
constexpr int STAGE64 = IMG + XIMG;            // dz image | x image
constexpr int LDS64 = 2 * STAGE64 + 64;
constexpr int NLX = (NPIX * 16 + 255) / 256;   // float4 loads of x per producer thread (13)
static_assert(LDS64 <= 160 * 1024 && NPIX * 128 <= XPLANE && XPLANE % 1024 == 0 && IMG % 1024 == 0, "LDS plan");
}  // namespace bj64

__global__ __launch_bounds__(bj::THREADS, 1) void bwd_joint64_kernel(JointParams p) {
  using namespace bj64;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  float* tmp = reinterpret_cast<float*>(smem + 2 * STAGE64);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float x_scale = dc_block_guard_scale(p.xAbound, CX, tmp);
  const float dz_scale = dc_block_guard_scale(p.dzCoef + 6 * C, C, tmp);
  constexpr int W_SLOTS64 = 9 * 4 * 2 * CX;     // [tap][k8][hi|lo][64 cols]
  const float w_scale = p.wp[W_SLOTS64 * 4];

  const DcXcdRange tiles = tile_range(p);
  const int nt = tiles.nt;
  const long x_img = (long)p.H * p.W * CX;

  if (wave >= 4) {
    // ============================ producers ===========================================================================
    const int t = tid & 255;
    const DzProducer dzp(p.dzCoef, t);              // dz: channel quad (8), first pixel (32 pixels per pass)
    const int qx = t & 15, pbx = t >> 4;            // x: channel quad (16), first pixel (16 pixels per pass)
    f32x4 rx0[NLX], rx1[NLX], ra[NL], rz[NL];
    unsigned live = 0u;
    auto request_x = [&](int j, f32x4 (&rx)[NLX]) __attribute__((always_inline)) {
      const Tile tl = decode(p, tiles, j);
      const __amdgpu_buffer_rsrc_t rsX = dc_make_rsrc(p.x + tl.img * x_img, (unsigned)(x_img * 4));
#pragma unroll
      for (int k = 0; k < NLX; ++k) {
        int y, xx;
        const bool ok = halo_pixel(p, tl, pbx + 16 * k, y, xx);
        const unsigned off = ok ? (unsigned)(((y * p.W + xx) * CX + 4 * qx) * 4) : OOB;
        rx[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsX, off, 0, 0));      // zeros outside the image
      }
    };
    auto stage_x = [&](const f32x4 (&rx)[NLX], char* set) __attribute__((always_inline)) {
#pragma unroll
      for (int k = 0; k < NLX; ++k) {
        const int pix = pbx + 16 * k;
        u32x2 xh, xl;
        dc_split_f16(rx[k], x_scale, xh, xl);
        if (pix < NPIX) {
          const int off = Rows128::swz(pix * 128 + qx * 8);
          *reinterpret_cast<u32x2*>(set + IMG + off) = xh;
          *reinterpret_cast<u32x2*>(set + IMG + XPLANE + off) = xl;
        }
      }
    };
    produce<STAGE64>(smem, nt, rx0, rx1, request_x,
                     [&](int j) __attribute__((always_inline)) { dzp.request(p, decode(p, tiles, j), ra, rz, live); },
                     stage_x, [&](char* set) __attribute__((always_inline)) { dzp.stage(ra, rz, live, dz_scale, set); });
    return;
  }

  const int li = lane & 31, h = lane >> 5;
  if (wave < 2) {
    // ================================ data gradient: 2 rows x 32 px x 64 cin per tile ==================================
    const int wd = wave;
    const float out_scale = 1.f / (dz_scale * w_scale);
    int a_rel[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) a_rel[mb] = ((2 * wd + mb) * TWI + li) * 64 + h * 16;
    const __amdgpu_buffer_rsrc_t rsW = dc_make_rsrc(p.wp, (unsigned)W_SLOTS64 * 16u);
    const unsigned w_rel = (unsigned)((h * 2 * CX + li) * 16);      // slot ((tap*4 + ks*2 + h)*2 + hl)*64 + nb*32 + li
    __syncthreads();
    for (int i = 0; i < nt; ++i) {
      const char* cur = smem + (i & 1) * STAGE64;
      int ar0 = a_rel[0], ar1 = a_rel[1];
      asm volatile("" : "+v"(ar0), "+v"(ar1));
      f32x16 acc[2][2];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;
      __builtin_amdgcn_s_setprio(2);
      {
        constexpr int NG = 18, AHEAD = 3;                          // weight fragments: global (L2) loads AHEAD groups ahead
        u32x4 wf[AHEAD + 1][2][2];                                 // [ring][nb][hi|lo]
        f16x8 ah[2][2], al[2][2];
        auto fetch_w = [&](int g, int slot) __attribute__((always_inline)) {
          const int tap = g >> 1, ks = g & 1;
          const int soff = ((tap * 4 + ks * 2) * 2) * CX * 16;
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) {
            wf[slot][nb][0] = __builtin_amdgcn_raw_buffer_load_b128(rsW, w_rel + nb * 512, soff, 0);
            wf[slot][nb][1] = __builtin_amdgcn_raw_buffer_load_b128(rsW, w_rel + nb * 512, soff + CX * 16, 0);
          }
        };
#pragma unroll
        for (int g = 0; g < AHEAD; ++g) fetch_w(g, g);
        fetch_dz_window(cur, 0, ar0, ar1, ah[0], al[0]);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const int b = g & 1, ws = g % (AHEAD + 1);
          if (g + AHEAD < NG) fetch_w(g + AHEAD, (g + AHEAD) % (AHEAD + 1));
          if (g + 1 < NG) fetch_dz_window(cur, g + 1, ar0, ar1, ah[b ^ 1], al[b ^ 1]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
              dc_mfma3(ah[b][mb], al[b][mb], __builtin_bit_cast(f16x8, wf[ws][nb][0]), __builtin_bit_cast(f16x8, wf[ws][nb][1]),
                       acc[mb][nb]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
      const Tile tl = decode(p, tiles, i);
      const __amdgpu_buffer_rsrc_t rsO = dc_make_rsrc(p.dx + tl.img * x_img, (unsigned)(x_img * 4));
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
        const int oy = tl.y0 + 2 * wd + mb, oxb = tl.x0 + 4 * h;
        const bool row_ok = oy < p.H;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int colc = (r & 3) + 8 * (r >> 2);
          const bool ok = row_ok && (oxb + colc) < p.W;
          const unsigned off = ok ? (unsigned)(((oy * p.W + oxb + colc) * CX + li) * 4) : OOB;
#pragma unroll
          for (int nb = 0; nb < 2; ++nb)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc[mb][nb][r] * out_scale), rsO, off, nb * 128, 0);
        }
      }
      __syncthreads();
    }
    return;
  }

  // ============== weight gradient: wave 2 + ww = input channels [32 ww, 32 ww + 32), all four rows, all taps ==============
  const int ww = wave - 2;
  const int cb = (lane >> 4) & 1, c16 = lane & 15, q4 = c16 >> 2, pp = c16 & 3;
  const int fragz = (cb * 2 + (pp >> 1)) * 16 + (pp & 1) * 8;                 // dz image: 4 chunks per pixel row
  const int fragx = (ww * 4 + cb * 2 + (pp >> 1)) * 16 + (pp & 1) * 8;        // x image: 8 chunks, this wave's 32-channel half
  const int lane_z = (8 * h + q4) * 64 + fragz, lane_x = (8 * h + q4) * 128 + fragx;
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  __syncthreads();
  for (int i = 0; i < nt; ++i) {
    const char* cur = smem + (i & 1) * STAGE64;
    int lz = lane_z, lx = lane_x;
    asm volatile("" : "+v"(lz), "+v"(lx));
    __builtin_amdgcn_s_setprio(2);
    wgrad_tile<Rows128, 72>(cur, lx, lz, acc);                     // 8 k-steps: all four rows x two 16-pixel halves
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }
  // slab [9][64][32] of this workgroup: rows m = input channel, columns n = dz channel (C/D: col = lane & 31, row = (r&3) + 8 (r>>2) + 4h)
  const float ws_scale = 1.f / (x_scale * dz_scale);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    float* dst = p.slabs + ((long)blockIdx.x * 9 + tap) * CX * C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = 32 * ww + (r & 3) + 8 * (r >> 2) + 4 * h;
      dst[m * C + li] = acc[tap][r] * ws_scale;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
static int joint_grid(int N, int H, int W) {
  static int cus[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
    cus[dev] = n;
  }
  const long total = (long)N * dc_cdiv(W, bj::TW) * dc_cdiv(H, bj::TH);
  return (int)(total < cus[dev] ? total : cus[dev]);
}
static bool joint_serves(int N, int H, int W, int Cin, int Cout) {
  return N > 0 && (Cin == bj::C || Cin == bj64::CX) && Cout == bj::C && W >= 32 && H >= 4 && (long)H * W * Cin * 4 < (1L << 31);
}

// rows of bn_partial / amax_partial (2 per workgroup) when the joint kernel serves this shape, else 0
extern "C" int dc_conv3x3_bwd_joint_blocks(int N, int H, int W, int Cin, int Cout) {
  if (!joint_serves(N, H, W, Cin, Cout)) return 0;
  return 2 * joint_grid(N, H, W);
}
extern "C" long dc_conv3x3_bwd_joint_ws_floats(int N, int H, int W, int Cin, int Cout) {
  if (!joint_serves(N, H, W, Cin, Cout)) return 0;
  const long L = 9L * Cin * Cout;
  return (long)joint_grid(N, H, W) * L + 32 * L;
}
// da materialised (s == kh == NULL) or rank one (da == NULL: da[pix][c] = (kh[c][1] - kh[c][0]) * s[pix], 32 -> 32 only)
static int joint_launch(const char* fn, const float* x, const float* in_sc, const float* in_sh, const float* x_abound,
                        const float* da, const float* s, const float* kh, const float* z, const float* dz_coef, const void* wp16,
                        float* dx, const float* red_z, const float* red_mean, const float* red_invstd, const float* red_gamma,
                        const float* red_beta, float* bn_partial, float* amax_partial, float* dw, float* ws, int N, int H, int W,
                        int Cin, int Cout, dc_stream_t stream) {
  const bool r1 = da == nullptr;
  DC_REQUIRE(x && (r1 ? (s && kh) : true) && z && dz_coef && wp16 && dx && dw && ws, DC_EINVAL, "%s: null pointer", fn);
  DC_REQUIRE(dc_aligned16(x) && dc_aligned16(da) && dc_aligned16(z) && dc_aligned16(dz_coef) && dc_aligned16(wp16) && dc_aligned16(dx),
             DC_EINVAL, "%s: pointers must be 16-byte aligned", fn);
  DC_REQUIRE((in_sc == nullptr) == (in_sh == nullptr) && (!in_sc || (dc_aligned16(in_sc) && dc_aligned16(in_sh))), DC_EINVAL,
             "%s: in_scale / in_shift go together, 16-byte aligned", fn);
  DC_REQUIRE(red_z == nullptr || (red_mean && red_invstd && red_gamma && red_beta && bn_partial), DC_EINVAL,
             "%s: red_z needs red_mean / red_invstd / red_gamma / red_beta / bn_partial", fn);
  DC_REQUIRE(joint_serves(N, H, W, Cin, Cout) && (!r1 || Cin == bj::C), DC_EUNSUP,
             "%s: shape not served (dc_conv3x3_bwd_joint_blocks() == 0): use the separate kernels", fn);
  const int grid = joint_grid(N, H, W);
  DC_REQUIRE(grid > 0, DC_EHIP, "%s: no device", fn);
  static DcLdsAttr lds_attr, lds_attr_r1, lds_attr64;
  if (Cin == bj::C) {
    if (int rc = r1 ? dc_func_max_lds(lds_attr_r1, reinterpret_cast<const void*>(bwd_joint32_kernel<true>), bj::LDS_BYTES, fn)
                    : dc_func_max_lds(lds_attr, reinterpret_cast<const void*>(bwd_joint32_kernel<false>), bj::LDS_BYTES, fn))
      return rc;
  } else {
    DC_REQUIRE(!in_sc && !red_z, DC_EUNSUP, "%s: the 64 -> 32 kernel takes a materialised x and emits no sums", fn);
    if (int rc = dc_func_max_lds(lds_attr64, reinterpret_cast<const void*>(bwd_joint64_kernel), bj64::LDS64, fn))
      return rc;
  }
  JointParams p;
  p.x = x; p.xSc = in_sc; p.xSh = in_sh; p.xAbound = x_abound; p.da = da; p.z = z; p.dzCoef = dz_coef;
  p.s = s; p.kh = kh;
  p.wp = reinterpret_cast<const float*>(wp16); p.dx = dx;
  p.redZ = red_z; p.redMean = red_mean; p.redInvstd = red_invstd; p.redGamma = red_gamma; p.redBeta = red_beta;
  p.bnPartial = bn_partial; p.bnAmax = amax_partial; p.slabs = ws;
  p.N = N; p.H = H; p.W = W; p.tilesX = dc_cdiv(W, bj::TW); p.tilesY = dc_cdiv(H, bj::TH);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  const bool bracket = dc_take_bracket(&ev0, &ev1);          // dc_bracket_next_launch: the matrix kernel without the slab reduction
  if (bracket && ev0) (void)hipEventRecord(ev0, (hipStream_t)stream);
  if (Cin == bj::C && r1)
    hipLaunchKernelGGL(bwd_joint32_kernel<true>, dim3((unsigned)grid), dim3(bj::THREADS), bj::LDS_BYTES, (hipStream_t)stream, p);
  else if (Cin == bj::C)
    hipLaunchKernelGGL(bwd_joint32_kernel<false>, dim3((unsigned)grid), dim3(bj::THREADS), bj::LDS_BYTES, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(bwd_joint64_kernel, dim3((unsigned)grid), dim3(bj::THREADS), bj64::LDS64, (hipStream_t)stream, p);
  if (bracket && ev1) (void)hipEventRecord(ev1, (hipStream_t)stream);
  DC_CHECK_LAUNCH(fn);
  const long L = 9L * Cin * Cout;
  return dc_reduce_partials(ws, grid, L, 1.0f, dw, ws + (long)grid * L, stream);
}
extern "C" int dc_conv3x3_bwd_joint_f16x3(const float* x, const float* in_sc, const float* in_sh, const float* x_abound,
                                          const float* da, const float* z, const float* dz_coef, const void* wp16, float* dx,
                                          const float* red_z, const float* red_mean, const float* red_invstd,
                                          const float* red_gamma, const float* red_beta, float* bn_partial,
                                          float* amax_partial, float* dw, float* ws, int N, int H, int W, int Cin, int Cout,
                                          dc_stream_t stream) {
  DC_REQUIRE(da, DC_EINVAL, "dc_conv3x3_bwd_joint_f16x3: null pointer");
  return joint_launch("dc_conv3x3_bwd_joint_f16x3", x, in_sc, in_sh, x_abound, da, nullptr, nullptr, z, dz_coef, wp16, dx, red_z,
                      red_mean, red_invstd, red_gamma, red_beta, bn_partial, amax_partial, dw, ws, N, H, W, Cin, Cout, stream);
}
// the block under the head (dcunet.h): da given by its rank-one factors (s from dc_head_fwd_bwd_s / dc_head_bwd_bnin_bnred_s, kh)
extern "C" int dc_conv3x3_bwd_joint_r1_f16x3(const float* x, const float* in_sc, const float* in_sh, const float* x_abound,
                                             const float* s, const float* kh, const float* z, const float* dz_coef,
                                             const void* wp16, float* dx, const float* red_z, const float* red_mean,
                                             const float* red_invstd, const float* red_gamma, const float* red_beta,
                                             float* bn_partial, float* amax_partial, float* dw, float* ws, int N, int H, int W,
                                             int Cin, int Cout, dc_stream_t stream) {
  DC_REQUIRE(s && kh, DC_EINVAL, "dc_conv3x3_bwd_joint_r1_f16x3: null pointer");
  DC_REQUIRE(Cin == bj::C, DC_EUNSUP, "dc_conv3x3_bwd_joint_r1_f16x3: Cin = Cout = 32 only");
  return joint_launch("dc_conv3x3_bwd_joint_r1_f16x3", x, in_sc, in_sh, x_abound, nullptr, s, kh, z, dz_coef, wp16, dx, red_z,
                      red_mean, red_invstd, red_gamma, red_beta, bn_partial, amax_partial, dw, ws, N, H, W, Cin, Cout, stream);
}
