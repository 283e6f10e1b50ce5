// Overlapping im2col for gfx950: the col matrix of Conv2d(C, D, kernel=p, stride=s) with s | p, s < p over [B, C, H, W]
// images (fp32 or bf16 pixels), gh x gw = ((H - p) / s + 1) x ((W - p) / s + 1) patches each:
//   col[b*gh*gw + py*gw + px][c*p*p + ky*p + kx] = image[b, c, py*s + ky, px*s + kx]
// rounded once to bf16, columns C*p*p .. Kp-1 zero.  The patch GEMM (EPI_PATCH) reads col as it reads the stride-p one.
// HBM-bound: every pixel lands in up to (p/s)^2 rows, so the kernel reads each pixel (p/s) times -- once per patch row it
// belongs to, from L2 after the first -- and writes (p/s)^2 times its bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {
namespace {

// ---------------------------------------------------------------------------------------------
// The LDS form (p even, s >= 2).  A workgroup owns patch row py of image b and up to tpb neighbouring patches t0 .. t0+nt-1.
//
// Fill: the C*p image-row segments those patches cover -- (nt-1)*s + p contiguous pixels each, starting at pixel t0*s
// of image row py*s + ky of channel c -- are read once as whole vectors (P8, p % 8 == 0: 8 pixels = one 16-byte bf16
// load or two 16-byte fp32 loads; else pixel pairs, p even: 4 / 8 bytes), converted, and stored to LDS row r = c*p + ky at
// byte r*RS + 2*x.  t0*s and W are multiples of the vector, so every vector is aligned and ends inside its image row (a
// last vector may run past the segment, never past the row).  Consecutive lanes take consecutive vectors of a row.
//
// Drain: element k = r*p + kx of patch t is LDS[r*RS + 2*(t*s + kx)], so a 16-byte chunk of a col row (8 consecutive k)
// is 8 consecutive pixels of one LDS row when p % 8 == 0, read at the alignment A = gcd(2s, 16) bytes that every patch
// start has: one ds_read_b128 (s % 8 == 0), two b64 (s % 4 == 0) or four b32 (s % 2 == 0) -- never an access off its
// natural alignment (those are replayed at 64 cycles).  A lane owns one chunk and stores it with one 16-byte global
// store; consecutive lanes own NP = 16 / A neighbouring patches of the same chunk, then the next chunk:
//   lane index i -> patch tg*NP + i % NP, chunk (i / NP) % (Kp / 8),
// so a store instruction writes runs of 64 / NP chunks (1024 / NP contiguous bytes) per col row.
//
// Banks.  Two choices make the drain conflict-free (computed with the bank rules of ds_read_b32 -- 32 banks, 32-lane
// groups -- and ds_read_b64 / b128 -- 64 banks, 32- / 16-lane groups; 1.00 = one LDS cycle per group):
//  * RS is an ODD multiple of 2p bytes.  Modulo the 256-byte bank row the rows of a patch then lie as in a dense
//    [p][p] bf16 array: the chunks of a patch, in chunk order, sit 16 bytes apart and tile the bank row.
//  * Neighbouring patches start s pixels = A bytes (mod 16) apart, NOT 2p: with one patch per lane group every lane
//    would read dword j of a 16-byte slot in the same step and meet the other lanes 4 banks on (4-way at s = 2, 2-way
//    at s = 4).  The NP patches a lane group interleaves fill exactly the A-byte steps between two chunks.
//   p = 16 and 32, every s, C = 1 and 3: 1.00.  p = 8: 1.00 at s = 2; at s = 4 (a row is one chunk) 1.33 (C = 3) / 2.0 (C = 1).
//  * p = 14 (pairs, four b32 reads per chunk walking (r, kx) by increments; s = 7: odd patches start on an odd pixel and
//    read their pairs as two 16-bit halves): RS = 8 (mod 16) bytes: 1.00 (C = 1) / 1.8 (C = 3).
// LDS: C*p*RS bytes; tpb = 32 patches, halved until that is <= 64 KB (p = 32, C = 3, s = 16: tpb = 16, 54 KB).
// ---------------------------------------------------------------------------------------------
template <bool IN_BF16, bool P8, int A>
__global__ __launch_bounds__(256) void im2col_overlap_kernel(const void* __restrict__ images, bf16_t* __restrict__ col, int C,
                                                             int H, int W, int p, int s, int gh, int gw, int Kp, int tpb,
                                                             int blocks_per_row, int RS) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int V = P8 ? 8 : 2;  // pixels per fill vector
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int xb = bid % blocks_per_row;
  bid /= blocks_per_row;
  const int py = bid % gh;
  const int b = bid / gh;
  const int t0 = xb * tpb;
  const int nt = min(tpb, gw - t0);  // patches of this workgroup
  // ---- fill ----
  const int nv = ((nt - 1) * s + p + V - 1) / V;  // vectors per row segment
  const int nvec = C * p * nv;
  const int64_t img_base = ((int64_t)b * C * H + (int64_t)py * s) * W + (int64_t)t0 * s;
  auto src_of = [&](int i, int* dst) {
    const int r = i / nv, v = i - r * nv;
    const int c = r / p, ky = r - c * p;
    *dst = r * RS + v * (V * 2);
    return img_base + ((int64_t)c * H + ky) * W + v * V;
  };
  constexpr int U = 4;  // vectors in flight per lane
  for (int i0 = tid; i0 < nvec; i0 += 256 * U) {
    int dst[U];
    if constexpr (P8) {
      bf16x8 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * 256;
        if (i >= nvec) break;
        const int64_t src = src_of(i, &dst[u]);
        if constexpr (IN_BF16) {
          v[u] = *reinterpret_cast<const bf16x8*>((const bf16_t*)images + src);
        } else {
          const f32x4 a0 = *reinterpret_cast<const f32x4*>((const float*)images + src);
          const f32x4 a1 = *reinterpret_cast<const f32x4*>((const float*)images + src + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[u][e] = (bf16_t)a0[e];
            v[u][4 + e] = (bf16_t)a1[e];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i0 + u * 256 < nvec) *reinterpret_cast<bf16x8*>(smem + dst[u]) = v[u];
    } else {
      bf16x2 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * 256;
        if (i >= nvec) break;
        const int64_t src = src_of(i, &dst[u]);
        if constexpr (IN_BF16) {
          v[u] = *reinterpret_cast<const bf16x2*>((const bf16_t*)images + src);
        } else {
          const float2 f = *reinterpret_cast<const float2*>((const float*)images + src);
          v[u][0] = (bf16_t)f.x;
          v[u][1] = (bf16_t)f.y;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i0 + u * 256 < nvec) *reinterpret_cast<bf16x2*>(smem + dst[u]) = v[u];
    }
  }
  __syncthreads();
  // ---- drain ----
  constexpr int NP = P8 ? 16 / A : 1;  // neighbouring patches interleaved across consecutive lanes
  const int k8 = Kp >> 3, Kreal = C * p * p;
  const int64_t row0 = ((int64_t)b * gh + py) * gw + t0;
  const int total = ((nt + NP - 1) / NP) * k8 * NP;
  for (int i = tid; i < total; i += 256) {
    const int ts = i % NP, q = i / NP;
    const int tg = q / k8, ch = q - tg * k8;
    const int t = tg * NP + ts;
    if (t >= nt) continue;
    const int k0 = ch * 8;
    u32x4 o = {0u, 0u, 0u, 0u};
    if constexpr (P8) {
      if (k0 < Kreal) {  // (Kreal is a multiple of 64 here: a chunk is whole or padding)
        const int r = k0 / p, kx = k0 - r * p;
        const char* src = smem + r * RS + (t * s + kx) * 2;
        if constexpr (A == 16) {
          o = *reinterpret_cast<const u32x4*>(src);
        } else if constexpr (A == 8) {
          const u32x2 lo = *reinterpret_cast<const u32x2*>(src), hi = *reinterpret_cast<const u32x2*>(src + 8);
          o = u32x4{lo[0], lo[1], hi[0], hi[1]};
        } else {
          const uint32_t* w = reinterpret_cast<const uint32_t*>(src);
          o = u32x4{w[0], w[1], w[2], w[3]};
        }
      }
    } else {
      // p even, not a multiple of 8: the chunk's four pixel pairs, (r, kx) walked by increments (a pair never straddles
      // two rows: k and p are even)
      int r = k0 / p, kx = k0 - r * p;
      const bool odd = A == 2 && (t & 1);  // (s odd: the patch starts on an odd pixel)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k0 + 2 * j < Kreal) {
          const char* src = smem + r * RS + (t * s + kx) * 2;
          if (odd) {
            const uint16_t* h = reinterpret_cast<const uint16_t*>(src);
            o[j] = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
          } else {
            o[j] = *reinterpret_cast<const uint32_t*>(src);
          }
        }
        kx += 2;
        if (kx >= p) {
          kx = 0;
          ++r;
        }
      }
    }
    *reinterpret_cast<u32x4*>(col + (row0 + t) * Kp + k0) = o;
  }
}

// The plain form for what the LDS form leaves (s = 1, odd p, unaligned images, a width that is no multiple of the fill
// vector, C*p rows beyond 64 KB of LDS): one thread per 16-byte chunk, one scalar load per element.
template <bool IN_BF16>
__global__ __launch_bounds__(256) void im2col_overlap_plain_kernel(const void* __restrict__ images, bf16_t* __restrict__ col,
                                                                   int64_t total8, int C, int H, int W, int p, int s, int gh,
                                                                   int gw, int Kp) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total8) return;
  const int k8 = Kp >> 3;
  const int64_t row = idx / k8;
  const int kk = (int)(idx - row * k8) * 8;
  const int n = gh * gw;
  const int64_t b = row / n;
  const int pi = (int)(row - b * n);
  const int py = pi / gw, px = pi - py * gw;
  const int pp = p * p, Kreal = C * pp;
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = kk + e;
    float val = 0.0f;
    if (k < Kreal) {
      const int c = k / pp;
      const int rem = k - c * pp;
      const int ky = rem / p, kx = rem - ky * p;
      const int64_t src = ((b * C + c) * H + (py * s + ky)) * (int64_t)W + px * s + kx;
      val = IN_BF16 ? (float)((const bf16_t*)images)[src] : ((const float*)images)[src];
    }
    o[e] = (bf16_t)val;
  }
  *reinterpret_cast<bf16x8*>(col + row * Kp + kk) = o;
}

// LDS row stride of the overlap kernel for tiles of tpb patches (see its header): P8: the odd multiple of 2p bytes that
// holds the segment rounded up to whole 8-pixel vectors; else the segment in pixel pairs, rounded up to 16 bytes, + 8
int overlap_row_stride(int p, int s, int tpb) {
  const int wseg = (tpb - 1) * s + p;
  if ((p & 7) == 0) {
    const int bytes = ((wseg + 7) / 8) * 16;
    return 2 * p * (((bytes + 2 * p - 1) / (2 * p)) | 1);
  }
  return ((((wseg + 1) / 2) * 4 + 15) / 16) * 16 + 8;
}

template <bool IN_BF16, bool P8, int A>
hipError_t launch_overlap(const void* images, void* col, int batch, int C, int H, int W, int p, int s, int gh, int gw, int Kp,
                          int tpb, int RS, hipStream_t st) {
  const int bpr = (gw + tpb - 1) / tpb;
  const dim3 grid((unsigned)((int64_t)batch * gh * bpr)), block(256);
  hipLaunchKernelGGL((im2col_overlap_kernel<IN_BF16, P8, A>), grid, block, (size_t)C * p * RS, st, images, (bf16_t*)col, C, H, W,
                     p, s, gh, gw, Kp, tpb, bpr, RS);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_im2col_strided(const void* images, int in_bf16, void* col, int batch, int C, int H, int W, int p, int s,
                                 int Kp, hipStream_t st) {
  if (batch <= 0 || C <= 0 || p <= 0 || s <= 0 || s > p || p % s || H < p || W < p || (H - p) % s || (W - p) % s || (Kp & 63) ||
      Kp < C * p * p)
    return hipErrorInvalidValue;
  if (s == p) return launch_im2col(images, in_bf16, col, batch, C, H, W, p, Kp, st);
  const int gh = (H - p) / s + 1, gw = (W - p) / s + 1;
  if ((int64_t)batch * gh * gw > INT32_MAX) return hipErrorInvalidValue;
  const bool p8 = (p & 7) == 0;
  const int V = p8 ? 8 : 2;
  if (s >= 2 && !(p & 1) && W % V == 0 && (((uintptr_t)images) & 15) == 0) {
    // tiles of 32 patches (a whole row when it has fewer), halved while the C*p row segments exceed 64 KB of LDS; a tile
    // that is not the whole row starts at pixel t0*s with t0 a multiple of 8, i.e. on a fill vector
    int tpb = 32;
    while (tpb > 8 && (int64_t)C * p * overlap_row_stride(p, s, tpb) > 65536) tpb >>= 1;
    if (gw < tpb) tpb = gw;
    const int RS = overlap_row_stride(p, s, tpb);
    if ((int64_t)C * p * RS <= 65536 && (int64_t)batch * gh * ((gw + tpb - 1) / tpb) <= INT32_MAX) {
      const int A = p8 ? ((s & 7) == 0 ? 16 : (s & 3) == 0 ? 8 : 4) : ((s & 1) ? 2 : 4);
#define VDR_OVERLAP(P8, AL)                                                                                                 \
  return in_bf16 ? launch_overlap<true, P8, AL>(images, col, batch, C, H, W, p, s, gh, gw, Kp, tpb, RS, st)                 \
                 : launch_overlap<false, P8, AL>(images, col, batch, C, H, W, p, s, gh, gw, Kp, tpb, RS, st)
      if (p8 && A == 16) VDR_OVERLAP(true, 16);
      if (p8 && A == 8) VDR_OVERLAP(true, 8);
      if (p8) VDR_OVERLAP(true, 4);
      if (A == 4) VDR_OVERLAP(false, 4);
      VDR_OVERLAP(false, 2);
#undef VDR_OVERLAP
    }
  }
  const int64_t total8 = (int64_t)batch * gh * gw * (Kp / 8);
  const dim3 grid((unsigned)((total8 + 255) / 256)), block(256);
  if (in_bf16)
    hipLaunchKernelGGL((im2col_overlap_plain_kernel<true>), grid, block, 0, st, images, (bf16_t*)col, total8, C, H, W, p, s, gh, gw, Kp);
  else
    hipLaunchKernelGGL((im2col_overlap_plain_kernel<false>), grid, block, 0, st, images, (bf16_t*)col, total8, C, H, W, p, s, gh, gw, Kp);
  return hipGetLastError();
}

}  // namespace vdr
