// Log-binned descriptors for gfx950 ("Deep ViT Features as Dense Visual Descriptors", bin=True): every patch's
// descriptor extended with its 8 neighbours and with average-pooled context at 3^k spacing.  F[b, y, x, c] on a gh x gw
// grid, C channels, hierarchy h in {1, 2, 3}:
//   A_k[b, y, x, c] = mean of F over the s x s window (s = 3^k) centred at (y, x), intersected with the grid; A_0 = F
//   bins, in order: k = 0 .. h-1, dy in (-s, 0, +s), dx in (-s, 0, +s), (0, 0) skipped for k >= 1: 1 + 8h bins
//   O[b, y*gw + x, j*C + c] = A_k[b, clamp(y + dy), clamp(x + dx), c]                      (bin-major)
// F is read where it lies: patch rows `ld` elements apart, images `image_stride` apart (a facet inside the qkv
// activation, or the residual stream behind its prefix rows), bf16 or fp32.
//
// Pass A (h >= 2) leaves A_1 (and A_2) as fp32 in `work` [h-1][batch][gh*gw][C].  One lane per 8 channels of one grid
// position; every sum is a fixed-order fp32 sum of that lane alone (rows top to bottom, columns left to right), so a
// value's bits depend on nothing but its window.  The mean is one IEEE division by the in-grid count.
//   A_1: the 3 x 3 window straight from F -- 9 chunk loads, served by L2 after the first touch.
//   A_2: separable -- the 9-wide row sums of F go to the A_1 slot of `work` first, the 9-tall column sums of those and
//        the division to the A_2 slot; A_1 is computed after it.  9 + 9 loads instead of 81.
// Pass B is the copy that matters: the output is (1 + 8h) times the input, and it is written once.  A workgroup owns one
// output row of (1 + 8h) C contiguous elements; a lane moves one 16-byte output chunk at a time (8 bf16 / 4 fp32 channels),
// consecutive lanes consecutive chunks, so a store instruction writes 1 KB of one row.  The source chunk -- F for level
// 0, `work` above -- comes from the clamped neighbour: up to 9 reads of each per level, all but the first from L2.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {
namespace {

VDR_DEV void load8(const void* p, int64_t i, bool bf16, float (&v)[8]) {
  if (bf16) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>((const bf16_t*)p + i);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)a[e];
  } else {
    const f32x4 a0 = *reinterpret_cast<const f32x4*>((const float*)p + i), a1 = *reinterpret_cast<const f32x4*>((const float*)p + i + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = a0[e];
      v[4 + e] = a1[e];
    }
  }
}

// dst[b, y, x, c] (fp32, dense) = sum of src over rows y-ry .. y+ry and columns x-rx .. x+rx inside the grid, divided by
// the number of grid positions of the (2 cy + 1) x (2 cx + 1) window at (y, x) when cy >= 0 (else the bare sum)
template <bool IN_BF16>
__global__ __launch_bounds__(256) void box_sum_kernel(const void* __restrict__ src, int64_t ld, int64_t image_stride,
                                                      float* __restrict__ dst, int64_t total8, int gh, int gw, int C, int ry,
                                                      int rx, int cy, int cx) {
  // (workgroups of one XCD take a contiguous range of positions: the window's re-reads then meet in that XCD's L2)
  const int64_t idx = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (idx >= total8) return;
  const int c8 = C >> 3;
  const int64_t pos = idx / c8;
  const int c = (int)(idx - pos * c8) * 8;
  const int n = gh * gw;
  const int64_t b = pos / n;
  const int pi = (int)(pos - b * n);
  const int y = pi / gw, x = pi - y * gw;
  const int y0 = max(y - ry, 0), y1 = min(y + ry, gh - 1), x0 = max(x - rx, 0), x1 = min(x + rx, gw - 1);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int64_t base = b * image_stride + c;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) {
      float v[8];
      load8(src, base + (int64_t)(yy * gw + xx) * ld, IN_BF16, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
  if (cy >= 0) {
    const float cnt = (float)((min(y + cy, gh - 1) - max(y - cy, 0) + 1) * (min(x + cx, gw - 1) - max(x - cx, 0) + 1));
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = __fdiv_rn(acc[e], cnt);
  }
  float* o = dst + pos * C + c;
  *reinterpret_cast<f32x4*>(o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<f32x4*>(o + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

// Pass B.  One workgroup per output row (image b, position (y, x)), rows dealt to the XCDs in contiguous ranges
// (xcd_remap): the 8 rows that read the same neighbour chunk of a level then run on one XCD, close in time, and all but the
// first read of a chunk is an L2 hit.  The block is two-dimensional -- threadIdx.x: 16-byte chunk within a bin,
// threadIdx.y: bin -- so no lane divides; with blockDim.x == chunks per bin the lanes' stores are one contiguous run.
template <bool IN_BF16, bool OUT_BF16>
__global__ __launch_bounds__(256) void log_bin_kernel(const void* __restrict__ src, int64_t ld, int64_t image_stride,
                                                      const float* __restrict__ work, void* __restrict__ out, int batch, int gh,
                                                      int gw, int C, int bins) {
  constexpr int CH = OUT_BF16 ? 8 : 4;  // channels of a 16-byte output chunk
  const int n = gh * gw;
  const int64_t row = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t b = row / n;
  const int pi = (int)(row - b * n);
  const int y = pi / gw, x = pi - y * gw;
  const int cpb = C / CH;
  const int64_t level_elems = (int64_t)batch * n * C;
  char* orow = (char*)out + row * (int64_t)bins * C * (OUT_BF16 ? 2 : 4);
  for (int j = threadIdx.y; j < bins; j += blockDim.y) {
    // bin j -> level k, offset (dy, dx) in units of s = 3^k
    int k = 0, t = j;
    if (j >= 9) {
      k = 1 + ((j - 9) >> 3);
      t = (j - 9) & 7;
      t += t >= 4;
    }
    const int s = k == 0 ? 1 : k == 1 ? 3 : 9;
    const int ty = t >= 6 ? 2 : t >= 3 ? 1 : 0;
    const int sy = min(max(y + (ty - 1) * s, 0), gh - 1), sx = min(max(x + (t - 3 * ty - 1) * s, 0), gw - 1);
    const int sp = sy * gw + sx;
    for (int cc = threadIdx.x; cc < cpb; cc += blockDim.x) {
    const int c = cc * CH, i = j * cpb + cc;
    u32x4 o;
    if (k == 0) {
      const int64_t si = b * image_stride + (int64_t)sp * ld + c;
      if constexpr (IN_BF16 && OUT_BF16) {
        o = *reinterpret_cast<const u32x4*>((const bf16_t*)src + si);
      } else if constexpr (IN_BF16) {
        const bf16x4 a = *reinterpret_cast<const bf16x4*>((const bf16_t*)src + si);
        o = __builtin_bit_cast(u32x4, f32x4{(float)a[0], (float)a[1], (float)a[2], (float)a[3]});
      } else if constexpr (OUT_BF16) {
        float v[8];
        load8(src, si, false, v);
        bf16x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (bf16_t)v[e];
        o = __builtin_bit_cast(u32x4, r);
      } else {
        o = *reinterpret_cast<const u32x4*>((const float*)src + si);
      }
    } else {
      const float* wp = work + (k - 1) * level_elems + (b * n + sp) * (int64_t)C + c;
      if constexpr (OUT_BF16) {
        float v[8];
        load8(wp, 0, false, v);
        bf16x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (bf16_t)v[e];
        o = __builtin_bit_cast(u32x4, r);
      } else {
        o = *reinterpret_cast<const u32x4*>(wp);
      }
    }
    *reinterpret_cast<u32x4*>(orow + (int64_t)i * 16) = o;
    }
  }
}

template <bool IN_BF16>
hipError_t box_sum(const void* src, int64_t ld, int64_t image_stride, float* dst, int batch, int gh, int gw, int C, int ry,
                   int rx, int cy, int cx, hipStream_t st) {
  const int64_t total8 = (int64_t)batch * gh * gw * (C / 8);
  const dim3 grid((unsigned)((total8 + 255) / 256)), block(256);
  hipLaunchKernelGGL((box_sum_kernel<IN_BF16>), grid, block, 0, st, src, ld, image_stride, dst, total8, gh, gw, C, ry, rx, cy, cx);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_log_bin(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int batch, int gh, int gw, int C,
                          int hierarchy, float* work, void* out, int out_bf16, hipStream_t st) {
  if (!x || !out || batch <= 0 || gh <= 0 || gw <= 0 || C <= 0 || (C & 7) || ld < C || hierarchy < 1 || hierarchy > 3 ||
      (hierarchy > 1 && !work))
    return hipErrorInvalidValue;
  // every chunk a lane loads or stores is 16 bytes on a 16-byte boundary
  const int64_t per16 = in_bf16 ? 8 : 4;
  if ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)work) & 15) || ld % per16 || image_stride % per16) return hipErrorInvalidValue;
  const int64_t n = (int64_t)gh * gw;
  // (a row per workgroup in blockIdx.x; the 8-channel chunks of pass A in 256-lane workgroups)
  if (n > INT32_MAX || (int64_t)batch * n > INT32_MAX || (int64_t)batch * n * (C / 8) / 256 >= INT32_MAX)
    return hipErrorInvalidValue;
  const int64_t level = (int64_t)batch * n * C;
  hipError_t e;
  if (hierarchy == 3) {
    // A_2, separable: 9-wide row sums of F into the A_1 slot, their 9-tall column sums / count into the A_2 slot
    e = in_bf16 ? box_sum<true>(x, ld, image_stride, work, batch, gh, gw, C, 0, 4, -1, -1, st)
                : box_sum<false>(x, ld, image_stride, work, batch, gh, gw, C, 0, 4, -1, -1, st);
    if (e != hipSuccess) return e;
    if ((e = box_sum<false>(work, C, n * C, work + level, batch, gh, gw, C, 4, 0, 4, 4, st)) != hipSuccess) return e;
  }
  if (hierarchy >= 2) {
    e = in_bf16 ? box_sum<true>(x, ld, image_stride, work, batch, gh, gw, C, 1, 1, 1, 1, st)
                : box_sum<false>(x, ld, image_stride, work, batch, gh, gw, C, 1, 1, 1, 1, st);
    if (e != hipSuccess) return e;
  }
  const int bins = 1 + 8 * hierarchy;
  const int cpb = C / (out_bf16 ? 8 : 4), bx = cpb < 256 ? cpb : 256, by = 256 / bx < bins ? 256 / bx : bins;
  const dim3 grid((unsigned)((int64_t)batch * n)), block(bx, by);
#define VDR_LOG_BIN(I, O) \
  hipLaunchKernelGGL((log_bin_kernel<I, O>), grid, block, 0, st, x, ld, image_stride, work, out, batch, gh, gw, C, bins)
  if (in_bf16) {
    if (out_bf16) VDR_LOG_BIN(true, true); else VDR_LOG_BIN(true, false);
  } else {
    if (out_bf16) VDR_LOG_BIN(false, true); else VDR_LOG_BIN(false, false);
  }
#undef VDR_LOG_BIN
  return hipGetLastError();
}

}  // namespace vdr
