// pos_embed resampling for gfx950: DINOv2 / transformers interpolate_pos_encoding, i.e.
//   F.interpolate(table[gh0, gw0, D] as NCHW, size = (gh, gw), mode = "bicubic", align_corners = False)
// on the patch rows of a learned position table (no antialias).  A load-time kernel (vdr_set_input_size): a few million
// outputs at most, so everything is evaluated in fp64 and rounded to fp32 once -- the result is the float64 definition
// rounded once, not one of several fp32 evaluation orders.
//
// Arithmetic (ATen's upsample_bicubic2d, in double; the file is built with -ffp-contract=off):
//   source coordinate  r = (o + 0.5) * (g0 / g) - 0.5  (not clamped),  i = floor(r),  t = r - i
//   cubic convolution, A = -0.75:  w0 = k2(t + 1), w1 = k1(t), w2 = k1(1 - t), w3 = k2(2 - t),
//     k1(x) = ((A + 2) x - (A + 3)) x^2 + 1,   k2(x) = ((A x - 5A) x + 8A) x - 4A
//   taps i - 1 .. i + 2, indices clamped to [0, g0 - 1]
//   out = sum_a wy[a] * (sum_b wx[b] * table[yi[a]][xi[b]][d])
// One thread per output element, d fastest: the 16 taps of a wave are 16 coalesced runs of the table.
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {

namespace {

__device__ inline void cubic_taps(int o, double scale, int g0, double w[4], int idx[4]) {
  constexpr double A = -0.75;
  const double r = ((double)o + 0.5) * scale - 0.5;
  const double fl = floor(r);
  const double t = r - fl;
  const int i = (int)fl;
  const double x0 = t + 1.0, x1 = t, x2 = 1.0 - t, x3 = 2.0 - t;
  w[0] = ((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A;
  w[1] = ((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0;
  w[2] = ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0;
  w[3] = ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A;
#pragma unroll
  for (int k = 0; k < 4; ++k) idx[k] = min(max(i - 1 + k, 0), g0 - 1);
}

__global__ __launch_bounds__(256) void pos_interp_kernel(const float* __restrict__ pos, float* __restrict__ out, int gh0,
                                                         int gw0, int D, int gh, int gw, double sy, double sx) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)gh * gw * D) return;
  const int64_t cell = idx / D;
  const int d = (int)(idx - cell * D);
  const int oy = (int)(cell / gw), ox = (int)(cell - (int64_t)oy * gw);
  double wy[4], wx[4];
  int yi[4], xi[4];
  cubic_taps(oy, sy, gh0, wy, yi);
  cubic_taps(ox, sx, gw0, wx, xi);
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float* row = pos + (int64_t)yi[a] * gw0 * D + d;
    double r = 0.0;
#pragma unroll
    for (int b = 0; b < 4; ++b) r += wx[b] * (double)row[(int64_t)xi[b] * D];
    acc += wy[a] * r;
  }
  out[idx] = (float)acc;
}

// get_rel_pos of segment_anything (and transformers' SamVisionAttention): a relative-position table [L0][D] resampled to
// [L][D] rows by F.interpolate(mode="linear", align_corners=False) along the row axis, per channel.  ATen's
// upsample_linear1d in double:  src = max((i + 0.5) * (L0 / L) - 0.5, 0),  i0 = trunc(src),  i1 = i0 + (i0 < L0 - 1),
// w1 = src - i0,  out = (1 - w1) * table[i0] + w1 * table[i1], rounded to fp32 once.
__global__ __launch_bounds__(256) void relpos_interp_kernel(const float* __restrict__ table, float* __restrict__ out, int L0,
                                                            int D, int L, double scale) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)L * D) return;
  const int i = (int)(idx / D);
  const int d = (int)(idx - (int64_t)i * D);
  double src = ((double)i + 0.5) * scale - 0.5;
  src = src < 0.0 ? 0.0 : src;
  int i0 = (int)src;
  i0 = i0 < L0 - 1 ? i0 : L0 - 1;
  const int i1 = i0 + (i0 < L0 - 1 ? 1 : 0);
  double w1 = src - (double)i0;
  w1 = w1 < 0.0 ? 0.0 : (w1 > 1.0 ? 1.0 : w1);
  const double w0 = 1.0 - w1;
  out[idx] = (float)(w0 * (double)table[(int64_t)i0 * D + d] + w1 * (double)table[(int64_t)i1 * D + d]);
}

}  // namespace

hipError_t launch_relpos_interp(const float* table, int L0, int D, float* out, int L, hipStream_t s) {
  if (!table || !out || L0 <= 0 || D <= 0 || L <= 0) return hipErrorInvalidValue;
  const int64_t total = (int64_t)L * D;
  if (total > ((int64_t)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(relpos_interp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, table, out, L0, D, L,
                     (double)L0 / (double)L);
  return hipGetLastError();
}

hipError_t launch_pos_interp(const float* pos, int gh0, int gw0, int D, float* out, int gh, int gw, hipStream_t s) {
  if (!pos || !out || gh0 <= 0 || gw0 <= 0 || D <= 0 || gh <= 0 || gw <= 0) return hipErrorInvalidValue;
  const int64_t total = (int64_t)gh * gw * D;
  if (total > ((int64_t)1 << 31) * 255) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pos_interp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pos, out, gh0, gw0, D, gh, gw,
                     (double)gh0 / (double)gh, (double)gw0 / (double)gw);
  return hipGetLastError();
}

}  // namespace vdr
