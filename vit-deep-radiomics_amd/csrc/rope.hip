// DINOv3's axial 2-D rotary position embedding for gfx950 (transformers DINOv3ViTRopePositionEmbedding +
// apply_rotary_pos_emb): q and k of the PATCH rows of every block are rotated per head; the CLS / register rows and v are
// not.
//
// Table (load-time, rope2d_table_kernel): patch (y, x) of a gh x gw grid has the coordinates
//   cy = 2 (y + 0.5) / gh - 1,   cx = 2 (x + 0.5) / gw - 1
// and, with inv_freq[i] = theta^(-4 i / dh) for i < dh / 4, the dh / 2 angles
//   a[j] = 2 pi cy inv_freq[j]            j <  dh / 4
//   a[j] = 2 pi cx inv_freq[j - dh / 4]   j >= dh / 4
// (the upper half of the head repeats them).  Angle, cos and sin are evaluated in fp64 and rounded to fp32 once; the
// tables are [gh * gw][dh / 2] fp32, shared by every head, block and image.
//
// Rotation (hot path, rope2d_kernel; the file is built with -ffp-contract=off, so every multiply, add and subtract below
// is one fp32 rounding, in this order):  lo = t[j], hi = t[j + dh / 2] (bf16 -> fp32, exact), c = cos[j], s = sin[j],
//   p1 = lo * c,  p2 = hi * s,  lo' = p1 - p2
//   p3 = hi * c,  p4 = lo * s,  hi' = p3 + p4
// lo' and hi' rounded to bf16 once (nearest even) and stored over lo and hi (transformers' rotate_half convention).
// One lane owns 8 neighbouring lo dims of one (patch row, head) and their 8 hi partners, for q and for k: four 16-byte
// loads of the activation, four of the table, four 16-byte stores.  No LDS, no atomics, no cross-lane traffic; a row's
// result depends on its own bits and the table only, never on the batch.
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {

namespace {

__global__ __launch_bounds__(256) void rope2d_table_kernel(float* __restrict__ cos_out, float* __restrict__ sin_out, int gh,
                                                           int gw, int half, double theta) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)gh * gw * half) return;
  const int64_t cell = idx / half;
  const int j = (int)(idx - cell * half);
  const int y = (int)(cell / gw), x = (int)(cell - (int64_t)y * gw);
  const int quarter = half >> 1;
  const bool is_x = j >= quarter;
  const int i = is_x ? j - quarter : j;
  const double coord = is_x ? 2.0 * ((double)x + 0.5) / (double)gw - 1.0 : 2.0 * ((double)y + 0.5) / (double)gh - 1.0;
  const double inv_freq = pow(theta, -(double)i / (double)quarter);  // theta^(-4 i / dh)
  const double a = 6.283185307179586476925286766559 * coord * inv_freq;
  cos_out[idx] = (float)cos(a);
  sin_out[idx] = (float)sin(a);
}

// lo / hi: 8 bf16 each; c / s: the 8 table entries of their angles
VDR_DEV void rotate8(bf16x8& lo, bf16x8& hi, const float* c, const float* s) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float l = (float)lo[e], h = (float)hi[e];
    const float p1 = l * c[e], p2 = h * s[e], p3 = h * c[e], p4 = l * s[e];
    lo[e] = (bf16_t)(p1 - p2);
    hi[e] = (bf16_t)(p3 + p4);
  }
}

// lane -> (patch row of the batch, head, chunk of 8 lo dims); chunks fastest, so the lanes of a row walk its q columns
template <int DH>
__global__ __launch_bounds__(256) void rope2d_kernel(bf16_t* __restrict__ qkv, const float* __restrict__ cos_t,
                                                     const float* __restrict__ sin_t, int64_t total, int seq, int prefix,
                                                     int heads) {
  constexpr int HALF = DH / 2, CH = DH / 16;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int np = seq - prefix;
  const int c8 = (int)(idx % CH) * 8;
  const int64_t rh = idx / CH;
  const int h = (int)(rh % heads);
  const int64_t pr = rh / heads;  // b * np + j
  const int64_t b = pr / np;
  const int j = (int)(pr - b * np);
  const int64_t ld = (int64_t)3 * heads * DH;
  bf16_t* q = qkv + (b * seq + prefix + j) * ld + h * DH + c8;
  bf16_t* k = q + (int64_t)heads * DH;
  const float* ct = cos_t + (int64_t)j * HALF + c8;
  const float* st = sin_t + (int64_t)j * HALF + c8;
  float c[8], s[8];
  *reinterpret_cast<f32x4*>(c) = *reinterpret_cast<const f32x4*>(ct);
  *reinterpret_cast<f32x4*>(c + 4) = *reinterpret_cast<const f32x4*>(ct + 4);
  *reinterpret_cast<f32x4*>(s) = *reinterpret_cast<const f32x4*>(st);
  *reinterpret_cast<f32x4*>(s + 4) = *reinterpret_cast<const f32x4*>(st + 4);
  bf16x8 qlo = *reinterpret_cast<const bf16x8*>(q), qhi = *reinterpret_cast<const bf16x8*>(q + HALF);
  bf16x8 klo = *reinterpret_cast<const bf16x8*>(k), khi = *reinterpret_cast<const bf16x8*>(k + HALF);
  rotate8(qlo, qhi, c, s);
  rotate8(klo, khi, c, s);
  *reinterpret_cast<bf16x8*>(q) = qlo;
  *reinterpret_cast<bf16x8*>(q + HALF) = qhi;
  *reinterpret_cast<bf16x8*>(k) = klo;
  *reinterpret_cast<bf16x8*>(k + HALF) = khi;
}

}  // namespace

hipError_t launch_rope2d_table(int gh, int gw, int head_dim, float theta, float* cos_out, float* sin_out, hipStream_t s) {
  if (!cos_out || !sin_out || gh <= 0 || gw <= 0 || (head_dim != 32 && head_dim != 64 && head_dim != 128) || !(theta > 1.0f))
    return hipErrorInvalidValue;
  const int64_t total = (int64_t)gh * gw * (head_dim / 2);
  if ((int64_t)gh * gw > ((int64_t)1 << 20)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rope2d_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cos_out, sin_out, gh, gw,
                     head_dim / 2, (double)theta);
  return hipGetLastError();
}

hipError_t launch_rope2d(void* qkv, int batch, int seq, int prefix, int heads, int head_dim, const float* cos_t,
                         const float* sin_t, hipStream_t s) {
  if (!qkv || !cos_t || !sin_t || batch <= 0 || seq <= 0 || prefix < 0 || prefix > seq || heads <= 0) return hipErrorInvalidValue;
  if (head_dim != 32 && head_dim != 64 && head_dim != 128) return hipErrorInvalidValue;
  // 16-byte accesses: the row pitch 3 H dh bf16 is a multiple of 16 bytes at these head dims; the bases must be aligned
  if ((((uintptr_t)qkv) | ((uintptr_t)cos_t) | ((uintptr_t)sin_t)) & 15) return hipErrorInvalidValue;
  if (prefix == seq) return hipSuccess;  // no patch rows
  const int64_t total = (int64_t)batch * (seq - prefix) * heads * (head_dim / 16);
  if (total > ((int64_t)1 << 31) * 255) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  bf16_t* p = (bf16_t*)qkv;
  switch (head_dim) {
    case 32:
      hipLaunchKernelGGL((rope2d_kernel<32>), grid, block, 0, s, p, cos_t, sin_t, total, seq, prefix, heads);
      break;
    case 64:
      hipLaunchKernelGGL((rope2d_kernel<64>), grid, block, 0, s, p, cos_t, sin_t, total, seq, prefix, heads);
      break;
    default:
      hipLaunchKernelGGL((rope2d_kernel<128>), grid, block, 0, s, p, cos_t, sin_t, total, seq, prefix, heads);
      break;
  }
  return hipGetLastError();
}

}  // namespace vdr
