// Squared Mahalanobis distances of bf16 descriptor rows for gfx950 (include/vdr.h: vdr_op_mahalanobis).
// Operand: kmeans.hip's -- `problems` problems of `imgs` images of t rows of d bf16 channels, rows ld elements apart, images
// image_stride apart, problems problem_stride apart; R = imgs * t rows per problem.  The model of problem p: mean + p * mean_stride
// ([d] fp32) and whiten + p * whiten_stride ([k][d] fp32); a stride of 0 is one model under every problem.
//
// Tile, accumulator layout, LDS images and the register-staged pipeline: desc_tile.h.
//   mahalanobis_kernel  256 threads; one work item = (problem, 128-row panel of X).  It walks the 128-row tiles of the whitening
//                       matrix; per tile a loop over d in steps of 64 stages four "t128" images: z_hi and z_lo of the panel's
//                       rows -- centred in fp32 and split in the staging pass itself -- and w_hi and w_lo of the tile's
//                       whitening rows, split there too (km_assign_kernel's rule for its centroids).  The rows are the A operand,
//                       the whitening rows the B operand, so a lane holds ONE whitening row j and 16 rows i.  Epilogue per tile,
//                       in that layout: y * y, rounded, added to the lane's running sum of its row (kept across the tiles).  At
//                       the end of the item the row sums are folded over the 32 lanes of a half wave (xor butterfly) and over
//                       the two column waves through LDS -- the image space, which nobody reads any more.  The R x k matrix is
//                       never written.
// No atomics, no scratch; nothing depends on `problems`, on the grid or on a launch heuristic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "desc_tile.h"
#include "vdr_dev.h"
#include "vdr_kernels.h"
#include "../../include/vdr.h"

namespace vdr {
namespace {

constexpr int MH_T = T128;               // rows of a panel, whitening rows of a tile
constexpr int MH_LDS = 4 * T128_OPER;    // z_hi, z_lo, w_hi, w_lo; the row exchange [2][128] fp32 re-uses z_hi's space
static_assert(MH_LDS <= 65536, "no opt-in to large dynamic LDS needed");
static_assert(2 * MH_T * (int)sizeof(float) <= T128_OPER, "the row exchange fits an image");

struct MhArgs {
  const bf16_t* x;
  int64_t ld, is, ps, R;
  int t, d, k, npanels, ntiles;
  const float* mean;    // + p * ms: [d]
  const float* whiten;  // + p * ws: [k][d]
  int64_t ms, ws;
  float* d2;            // [problems][R]
};

__global__ __launch_bounds__(256) void mahalanobis_kernel(MhArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int p = blockIdx.x / a.npanels, panel = blockIdx.x - p * a.npanels;
  const int nk = (a.d + 63) >> 6;

  // staging role: 16-byte chunk ch of the 64-column step, rows rl, rl + 32, rl + 64, rl + 96 of each image
  const int ch = tid & 7, rl = tid >> 3;
  bool rok[4];
  int64_t roff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t r = (int64_t)panel * MH_T + rl + 32 * j;
    rok[j] = r < a.R;
    roff[j] = rok[j] ? desc_row(a, p * a.ps, r) : 0;
  }

  float rs[2][16];
  f32x16 acc[2][2];
  acc_zero(acc);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) rs[m][e] = 0.0f;

  char* szh = smem;
  char* szl = smem + T128_OPER;
  char* swh = smem + 2 * T128_OPER;
  char* swl = smem + 3 * T128_OPER;
  const float* mean = a.mean + (int64_t)p * a.ms;
  const float* whiten = a.whiten + (int64_t)p * a.ws;

#pragma clang loop unroll(disable)
  for (int jt = 0; jt < a.ntiles; ++jt) {
    bool wok[4];
    const float* wrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = jt * MH_T + rl + 32 * j;
      wok[j] = c < a.k;
      wrow[j] = whiten + (int64_t)(wok[j] ? c : 0) * a.d;
    }
    RawChunk<true> rx[4];
    RawChunk<false> rw[4], rm;
    // (a row past R, a whitening row past k or a column past d is fetched as zeros)
    const auto fetch = [&](int step) {
      const int col = step * 64 + ch * 8;
      const bool colok = col < a.d;
      raw_fill(rm, colok, mean, col);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        raw_fill(rx[j], rok[j] && colok, a.x, roff[j] + col);
        raw_fill(rw[j], wok[j] && colok, wrow[j], col);
      }
    };
    const auto stage = [&](int step) {
      const bool colok = step * 64 + ch * 8 < a.d;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool on = rok[j] && colok;  // the zero of a row past R goes in AFTER the centring: -mean does not enter
        bf16x8 zh, zl, wh, wl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float z = on ? rx[j].get(e) - rm.get(e) : 0.0f;
          zh[e] = (bf16_t)z;
          zl[e] = (bf16_t)(z - (float)zh[e]);
          const float w = rw[j].get(e);
          wh[e] = (bf16_t)w;
          wl[e] = (bf16_t)(w - (float)wh[e]);
        }
        const int off = t128_off(rl + 32 * j, ch);
        *reinterpret_cast<bf16x8*>(szh + off) = zh;
        *reinterpret_cast<bf16x8*>(szl + off) = zl;
        *reinterpret_cast<bf16x8*>(swh + off) = wh;
        *reinterpret_cast<bf16x8*>(swl + off) = wl;
      }
    };

    staged_steps(nk, fetch, stage, [&]() { t128_mfma_2a2b(szh, szl, swh, swl, wr, wc, l31, hh, acc); });

    // ---- epilogue of tile jt: the lane's whitening rows jt * 128 + 64 wc + l31 (n = 0) and + 32 (n = 1), ascending; a row past
    // k was staged as zeros and adds +0
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const float y = acc[m][n][e];
          acc[m][n][e] = 0.0f;
          rs[m][e] += y * y;
        }
  }

  // ---- the row sums of the item: over the 32 lanes of a half wave, then over the two column waves
  __syncthreads();  // every wave has read the last step: the image space is free
  float* s_row = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float v = rs[m][e];
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o, 64);
      if (l31 == 0) s_row[wc * MH_T + acc_row(wr, m, e, hh)] = v;
    }
  __syncthreads();
  if (tid < MH_T) {
    const int64_t r = (int64_t)panel * MH_T + tid;
    if (r < a.R) a.d2[(int64_t)p * a.R + r] = s_row[tid] + s_row[MH_T + tid];
  }
}

}  // namespace

hipError_t launch_mahalanobis(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs,
                              int t, int d, const float* mean, int64_t mean_stride, const float* whiten, int64_t whiten_stride,
                              int k, float* d2, hipStream_t st) {
  if (!x || !mean || !whiten || !d2 || problems <= 0 || imgs <= 0 || t <= 0 || d <= 0 || (d & 31) || k < 1 || k > VDR_MAHALANOBIS_MAX_K ||
      ld < d || image_stride < 0 || problem_stride < 0 || mean_stride < 0 || whiten_stride < 0)
    return hipErrorInvalidValue;
  if ((((uintptr_t)x | (uintptr_t)mean | (uintptr_t)whiten) & 15) || ((uintptr_t)d2 & 3) || ((ld | image_stride | problem_stride) & 7) ||
      ((mean_stride | whiten_stride) & 3))
    return hipErrorInvalidValue;
  const int64_t R = (int64_t)imgs * t;
  if (R > INT32_MAX || R * problems > INT32_MAX) return hipErrorInvalidValue;
  MhArgs a;
  a.x = (const bf16_t*)x;
  a.ld = ld, a.is = image_stride, a.ps = problem_stride, a.R = R;
  a.t = t, a.d = d, a.k = k;
  a.npanels = (int)((R + MH_T - 1) / MH_T);
  a.ntiles = (k + MH_T - 1) / MH_T;
  a.mean = mean, a.whiten = whiten, a.ms = mean_stride, a.ws = whiten_stride;
  a.d2 = d2;
  const int64_t items = (int64_t)problems * a.npanels;
  if (items > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mahalanobis_kernel, dim3((unsigned)items), dim3(256), MH_LDS, st, a);
  return hipGetLastError();
}

}  // namespace vdr
