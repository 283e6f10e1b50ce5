// HBM-bound row kernels for gfx950: LayerNorm (+ row gather / CLS extraction), im2col for the
// patchify conv, CLS-row and token assembly.
//
// LayerNorm replaces nn.LayerNorm (reference src/models_archs.py:136,145; norm1/norm2/norm of the
// ViT blocks): biased variance, fp32 statistics, eps configurable.  One 64-lane wave per row, the
// whole row held in registers (4 elements per lane per pass), two-pass mean/variance with
// wave-wide shuffle reductions — 2*D*sizeof bytes of HBM traffic per row and nothing else.
// The row maps fold the x[:,0,:] CLS slice (models_archs.py:147) and the x[:,1:,:] dense slice
// (tfds_dense_descriptor.py:130-133) into the final LayerNorm.
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {

struct LnK {
  const void* x;
  void* y;
  const float* gamma;
  const float* beta;
  const float* cls;
  int64_t rows;
  int D;
  float eps;
  int irpg;
  int64_t igs;
  int ioff;
  int orpg;
  int64_t ogs;
  int ooff;
  int cls_period;
  int win_ws, win_g;
  int64_t ldy;  // output row stride in elements
  int vec_out;  // 1: every output row start is 16-byte (fp32) / 8-byte (bf16) aligned -> vector stores
};

VDR_DEV int64_t map_row(int64_t r, int rpg, int64_t gs, int off) {
  if (rpg >= (1 << 30)) return r;
  const int64_t g = r / rpg;
  return g * gs + off + (r - g * rpg);
}

// One row of D values held by one wave: lane l owns columns k*256 + 4l .. 4l+3 of pass k (zeros past D).  The
// LayerNorm kernel and the pooled reduction both normalise through these helpers, so their per-row arithmetic is one.
template <bool IN_BF16, int NP>
VDR_DEV void row_load(const void* x, int64_t row, int D, int lane, float (&v)[NP][4]) {
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = k * 256 + lane * 4;
    if (c < D) {
      if (IN_BF16) {
        const bf16x4 t = *reinterpret_cast<const bf16x4*>((const bf16_t*)x + row * D + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = (float)t[e];
      } else {
        const f32x4 t = *reinterpret_cast<const f32x4*>((const float*)x + row * D + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = t[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[k][e] = 0.0f;
    }
  }
}

// two-pass mean and biased variance of the row in fp32 (wave-wide shuffle sums), rstd = rsqrtf(var + eps)
template <int NP>
VDR_DEV void row_mean_rstd(const float (&v)[NP][4], int D, int lane, float eps, float& mean, float& rstd) {
  float sum = 0.0f;
#pragma unroll
  for (int k = 0; k < NP; ++k)
    if (k * 256 + lane * 4 < D) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sum += v[k][e];
    }
  const float invD = 1.0f / (float)D;
  mean = wave_sum(sum) * invD;
  float sq = 0.0f;
#pragma unroll
  for (int k = 0; k < NP; ++k)
    if (k * 256 + lane * 4 < D) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[k][e] - mean;
        sq += d * d;
      }
    }
  rstd = rsqrtf(wave_sum(sq) * invD + eps);
}

VDR_DEV float ln_affine(float v, float mean, float rstd, float g, float b) { return (v - mean) * rstd * g + b; }

template <bool IN_BF16, bool OUT_BF16, int NP>
__global__ __launch_bounds__(256) void layernorm_kernel(LnK p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= p.rows) return;
  const int64_t ir = map_row(r, p.irpg, p.igs, p.ioff);
  int64_t orow = map_row(r, p.orpg, p.ogs, p.ooff);
  if (p.win_ws > 0) {
    // window partition (segment_anything window_partition): token (b, y, x) -> window-major order
    const int g = p.win_g, ws = p.win_ws, nw = (g + ws - 1) / ws;
    const int64_t b = r / (g * g);
    const int rem = (int)(r - b * g * g);
    const int y = rem / g, x = rem - y * g;
    orow = ((b * nw + y / ws) * nw + x / ws) * (int64_t)(ws * ws) + (y % ws) * ws + (x % ws);
  }
  const bool from_cls = p.cls != nullptr && (r % p.cls_period) == 0;
  float v[NP][4];
  if (from_cls) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = k * 256 + lane * 4;
      if (c < p.D) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p.cls + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = t[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = 0.0f;
      }
    }
  } else {
    row_load<IN_BF16, NP>(p.x, ir, p.D, lane, v);
  }
  float mean, rstd;
  row_mean_rstd<NP>(v, p.D, lane, p.eps, mean, rstd);
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = k * 256 + lane * 4;
    if (c < p.D) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(p.gamma + c);
      const f32x4 bt = *reinterpret_cast<const f32x4*>(p.beta + c);
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = ln_affine(v[k][e], mean, rstd, g[e], bt[e]);
      const int64_t oi = orow * p.ldy + c;
      if (OUT_BF16) {
        bf16x4 ob;
#pragma unroll
        for (int e = 0; e < 4; ++e) ob[e] = (bf16_t)o[e];
        if (p.vec_out) {
          *reinterpret_cast<bf16x4*>((bf16_t*)p.y + oi) = ob;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) ((bf16_t*)p.y)[oi + e] = ob[e];
        }
      } else if (p.vec_out) {
        f32x4 of;
#pragma unroll
        for (int e = 0; e < 4; ++e) of[e] = o[e];
        *reinterpret_cast<f32x4*>((float*)p.y + oi) = of;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) ((float*)p.y)[oi + e] = o[e];
      }
    }
  }
}

template <bool IB, bool OB>
static hipError_t ln_dispatch(const LnK& k, hipStream_t s) {
  const int np = (k.D + 255) / 256;
  const dim3 grid((unsigned)((k.rows + 3) / 4)), block(256);
#define VDR_LN(NP)                                                              \
  case NP:                                                                      \
    hipLaunchKernelGGL((layernorm_kernel<IB, OB, NP>), grid, block, 0, s, k);   \
    break;
  switch (np) {
    VDR_LN(1) VDR_LN(2) VDR_LN(3) VDR_LN(4) VDR_LN(5) VDR_LN(6) VDR_LN(7) VDR_LN(8)
    default:
      return hipErrorInvalidValue;
  }
#undef VDR_LN
  return hipGetLastError();
}

// vector stores of 4 elements need every row start aligned to 4 elements
static int rows_aligned(const void* y, int64_t ldy, int es) { return (ldy % 4) == 0 && ((uintptr_t)y % (4 * es)) == 0; }

hipError_t launch_layernorm(const LnArgs& a, hipStream_t s) {
  if (a.rows <= 0 || a.D <= 0 || (a.D & 3) || a.D > 2048 || (a.ldy != 0 && a.ldy < a.D)) return hipErrorInvalidValue;
  LnK k;
  k.x = a.x;
  k.y = a.y;
  k.gamma = a.gamma;
  k.beta = a.beta;
  k.cls = a.cls;
  k.rows = a.rows;
  k.D = a.D;
  k.eps = a.eps;
  k.irpg = a.imap.rpg;
  k.igs = a.imap.gstride;
  k.ioff = a.imap.off;
  k.orpg = a.omap.rpg;
  k.ogs = a.omap.gstride;
  k.ooff = a.omap.off;
  k.cls_period = a.cls_period > 0 ? a.cls_period : 1;
  k.win_ws = a.win_ws;
  k.win_g = a.win_g;
  k.ldy = a.ldy ? a.ldy : a.D;
  k.vec_out = a.ldy == 0 || rows_aligned(a.y, k.ldy, a.out_bf16 ? 2 : 4);
  if (a.in_bf16) return a.out_bf16 ? ln_dispatch<true, true>(k, s) : ln_dispatch<true, false>(k, s);
  return a.out_bf16 ? ln_dispatch<false, true>(k, s) : ln_dispatch<false, false>(k, s);
}

// ---------------------------------------------------------------------------------------------
// Mean-pooled patch rows (vdr_forward_layers, VDR_OUT_POOLED: DINOv2 create_linear_input's avgpool).  Pass 1: one
// workgroup per (chunk of POOL_CHUNK patch rows, image); wave w takes rows w, w+4, ... of the chunk in order, normalises
// each with the LayerNorm kernel's helpers (norm = 1) and adds the fp32 values into per-lane column sums; the next row's
// loads are issued before the current row's reductions.  The four waves' sums meet in LDS and are added in wave order:
// part[b][chunk][:].  Pass 2: sum over the chunks in order, times 1/n, one rounding to the output dtype.  The chunking
// does not depend on the batch, so an image's result is the same in any batch.
// ---------------------------------------------------------------------------------------------
struct PoolK {
  const void* x;
  const float* gamma;
  const float* beta;
  float* part;
  int ntok, ncls, n, D, chunks;
  float eps;
};

template <bool IN_BF16, bool NORM, int NP>
__global__ __launch_bounds__(256) void pool_rows_kernel(PoolK p) {
  extern __shared__ __attribute__((aligned(16))) float red[];  // [4][D]: the waves' column sums
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int j0 = chunk * POOL_CHUNK;
  const int cnt = min(POOL_CHUNK, p.n - j0);  // rows of this chunk (the last one may be ragged)
  const int64_t row0 = (int64_t)b * p.ntok + p.ncls + j0;
  float g[NP][4], bt[NP][4], acc[NP][4];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = k * 256 + lane * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[k][e] = 0.0f;
    if (NORM && c < p.D) {
      const f32x4 tg = *reinterpret_cast<const f32x4*>(p.gamma + c);
      const f32x4 tb = *reinterpret_cast<const f32x4*>(p.beta + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        g[k][e] = tg[e];
        bt[k][e] = tb[e];
      }
    }
  }
  float v[NP][4], nx[NP][4];
  int j = wv;
  if (j < cnt) row_load<IN_BF16, NP>(p.x, row0 + j, p.D, lane, v);
  for (; j < cnt; j += 4) {
    const bool more = j + 4 < cnt;
    if (more) row_load<IN_BF16, NP>(p.x, row0 + j + 4, p.D, lane, nx);
    if (NORM) {
      float mean, rstd;
      row_mean_rstd<NP>(v, p.D, lane, p.eps, mean, rstd);
#pragma unroll
      for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] += ln_affine(v[k][e], mean, rstd, g[k][e], bt[k][e]);
    } else {
#pragma unroll
      for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] += v[k][e];
    }
    if (more) {
#pragma unroll
      for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = nx[k][e];
    }
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = k * 256 + lane * 4;
    if (c < p.D) {
      f32x4 t;
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = acc[k][e];
      *reinterpret_cast<f32x4*>(&red[wv * p.D + c]) = t;
    }
  }
  __syncthreads();
  float* dst = p.part + ((int64_t)b * p.chunks + chunk) * p.D;
  for (int c = threadIdx.x * 4; c < p.D; c += 1024) {
    f32x4 t = *reinterpret_cast<const f32x4*>(&red[c]);
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const f32x4 u = *reinterpret_cast<const f32x4*>(&red[w * p.D + c]);
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] += u[e];
    }
    *reinterpret_cast<f32x4*>(dst + c) = t;
  }
}

template <bool OUT_BF16>
__global__ __launch_bounds__(256) void pool_finish_kernel(const float* __restrict__ part, int chunks, int D, int batch, float inv_n,
                                                          void* __restrict__ y, int64_t ldy) {
  const int d4 = D >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)batch * d4) return;
  const int64_t b = idx / d4;
  const int c = (int)(idx - b * d4) * 4;
  const float* src = part + b * chunks * (int64_t)D + c;
  f32x4 t = *reinterpret_cast<const f32x4*>(src);
  for (int k = 1; k < chunks; ++k) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(src + (int64_t)k * D);
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] += u[e];
  }
  // (scalar stores: y + b*ldy need not be vector-aligned -- a column slice of a wider matrix)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float o = t[e] * inv_n;
    if (OUT_BF16)
      ((bf16_t*)y)[b * ldy + c + e] = (bf16_t)o;
    else
      ((float*)y)[b * ldy + c + e] = o;
  }
}

template <bool IB, bool NORM>
static hipError_t pool_dispatch(const PoolK& k, int np, dim3 grid, hipStream_t s) {
#define VDR_POOL(NP)                                                                         \
  case NP:                                                                                   \
    hipLaunchKernelGGL((pool_rows_kernel<IB, NORM, NP>), grid, dim3(256), (size_t)16 * k.D, s, k);          \
    break;
  switch (np) {
    VDR_POOL(1) VDR_POOL(2) VDR_POOL(3) VDR_POOL(4) VDR_POOL(5) VDR_POOL(6) VDR_POOL(7) VDR_POOL(8)
    default:
      return hipErrorInvalidValue;
  }
#undef VDR_POOL
  return hipGetLastError();
}

hipError_t launch_pool_rows(const void* x, int in_bf16, int norm, const float* gamma, const float* beta, float eps, int batch,
                            int ntok, int ncls, int n, int D, float* part, void* y, int out_bf16, int64_t ldy, hipStream_t s) {
  if (batch <= 0 || n <= 0 || ncls < 0 || ntok < n + ncls || D <= 0 || (D & 3) || D > 2048 || batch > 65535 ||
      (ldy != 0 && ldy < D) || (norm && (!gamma || !beta)))
    return hipErrorInvalidValue;
  PoolK k;
  k.x = x;
  k.gamma = gamma;
  k.beta = beta;
  k.part = part;
  k.ntok = ntok;
  k.ncls = ncls;
  k.n = n;
  k.D = D;
  k.chunks = (n + POOL_CHUNK - 1) / POOL_CHUNK;
  k.eps = eps;
  const dim3 grid((unsigned)k.chunks, (unsigned)batch);
  const int np = (D + 255) / 256;
  hipError_t e = in_bf16 ? (norm ? pool_dispatch<true, true>(k, np, grid, s) : pool_dispatch<true, false>(k, np, grid, s))
                         : (norm ? pool_dispatch<false, true>(k, np, grid, s) : pool_dispatch<false, false>(k, np, grid, s));
  if (e != hipSuccess) return e;
  const int64_t total = (int64_t)batch * (D / 4);
  const float inv_n = 1.0f / (float)n;
  const int64_t ld = ldy ? ldy : D;
  if (out_bf16)
    hipLaunchKernelGGL((pool_finish_kernel<true>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, k.chunks, D, batch,
                       inv_n, y, ld);
  else
    hipLaunchKernelGGL((pool_finish_kernel<false>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, k.chunks, D, batch,
                       inv_n, y, ld);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// im2col for Conv2d(C, D, kernel=p, stride=p) over [B, C, H, W] images, gh x gw = (H / p) x (W / p) patches each:
// col[b*n + py*gw + px][c*p*p + ky*p + kx].  One thread writes 8 consecutive k (one 16-byte store).
// ---------------------------------------------------------------------------------------------
template <bool IN_BF16>
__global__ __launch_bounds__(256) void im2col_kernel(const void* __restrict__ images, bf16_t* __restrict__ col,
                                                     int64_t total8, int C, int H, int W, int p, int gh, int gw, int Kp, int fast) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total8) return;
  const int k8 = Kp >> 3;
  const int64_t row = idx / k8;
  const int kk = (int)(idx - row * k8) * 8;
  const int n = gh * gw;
  const int64_t b = row / n;
  const int pi = (int)(row - b * n);
  const int py = pi / gw, px = pi - py * gw;
  const int pp = p * p;
  const int Kreal = C * pp;
  bf16x8 o;
  if (fast && kk < Kreal) {
    const int c = kk / pp;
    const int rem = kk - c * pp;
    const int ky = rem / p, kx = rem - ky * p;
    const int64_t src = ((b * C + c) * H + (py * p + ky)) * (int64_t)W + px * p + kx;
    if (IN_BF16) {
      o = *reinterpret_cast<const bf16x8*>((const bf16_t*)images + src);
    } else {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>((const float*)images + src);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>((const float*)images + src + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = (bf16_t)a0[e];
        o[4 + e] = (bf16_t)a1[e];
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = kk + e;
      float val = 0.0f;
      if (k < Kreal) {
        const int c = k / pp;
        const int rem = k - c * pp;
        const int ky = rem / p, kx = rem - ky * p;
        const int64_t src = ((b * C + c) * H + (py * p + ky)) * (int64_t)W + px * p + kx;
        val = IN_BF16 ? (float)((const bf16_t*)images)[src] : ((const float*)images)[src];
      }
      o[e] = (bf16_t)val;
    }
  }
  *reinterpret_cast<bf16x8*>(col + row * Kp + kk) = o;
}

// The same matrix for patch sides that are not a multiple of 8 (p = 14: DINOv2, ViT-L/14, ViT-g/14), through LDS: a
// workgroup takes up to 32 neighbouring patches of one patch row -- in the image that is C*p runs of 32*p contiguous
// pixels, read as coalesced pairs (p even: a pair never straddles two patches), converted and scattered into an LDS
// image [patch][Kp] (row stride Kp*2 + 32 bytes: consecutive patches start 8 banks apart) -- and writes the rows out as
// whole 16-byte chunks.  (The direct kernel above needs 8 scalar loads and 8 index divisions per 16-byte store here:
// 2.0 TB/s of pixels + rows in the reference's dinov2 mode; this form: see DESIGN.md §6 f-2.)
template <bool IN_BF16>
__global__ __launch_bounds__(256) void im2col_rows_kernel(const void* __restrict__ images, bf16_t* __restrict__ col, int C,
                                                          int H, int W, int p, int gh, int gw, int Kp, int tpb, int blocks_per_row) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int RS = Kp * 2 + 32;
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int xb = bid % blocks_per_row;
  bid /= blocks_per_row;
  const int py = bid % gh;
  const int b = bid / gh;
  const int t0 = xb * tpb;
  const int nt = min(tpb, gw - t0);  // patches of this workgroup
  const int pp = p * p, Kreal = C * pp;
  // zero the K padding
  const int padw = (Kp - Kreal) >> 1;  // dwords per row (Kreal and Kp are even)
  for (int i = tid; i < nt * padw; i += 256) {
    const int r = i / padw, j = i - r * padw;
    *reinterpret_cast<uint32_t*>(smem + r * RS + (Kreal + 2 * j) * 2) = 0u;
  }
  // pixels: a thread owns pixel pair j of the workgroup's run (its patch and kx fixed once) and walks the C*p image rows
  const int ppr = (nt * p) >> 1;
  const int64_t img_base = ((int64_t)b * C * H + py * p) * W + t0 * p;
  for (int j = tid; j < ppr; j += 256) {
    const int x = 2 * j;
    const int t = x / p, kx = x - t * p;
    char* dst = smem + t * RS + kx * 2;
    auto load = [&](int64_t src) {
      bf16x2 v;
      if (IN_BF16) {
        v = *reinterpret_cast<const bf16x2*>((const bf16_t*)images + src);
      } else {
        const float2 f = *reinterpret_cast<const float2*>((const float*)images + src);
        v[0] = (bf16_t)f.x;
        v[1] = (bf16_t)f.y;
      }
      return v;
    };
    for (int c = 0; c < C; ++c) {
      const int64_t src = img_base + (int64_t)c * H * W + x;
      char* d = dst + c * pp * 2;
      int ky = 0;
      for (; ky + 7 <= p; ky += 7) {  // 7 rows in flight (p = 14: two rounds)
        bf16x2 v[7];
#pragma unroll
        for (int u = 0; u < 7; ++u) v[u] = load(src + (int64_t)(ky + u) * W);
#pragma unroll
        for (int u = 0; u < 7; ++u) *reinterpret_cast<bf16x2*>(d + (ky + u) * p * 2) = v[u];
      }
      for (; ky < p; ++ky) *reinterpret_cast<bf16x2*>(d + ky * p * 2) = load(src + (int64_t)ky * W);
    }
  }
  __syncthreads();
  const int k8 = Kp >> 3;
  const int64_t row0 = ((int64_t)b * gh + py) * gw + t0;
  for (int i = tid; i < nt * k8; i += 256) {
    const int r = i / k8, ch = i - r * k8;
    *reinterpret_cast<bf16x8*>(col + (row0 + r) * Kp + ch * 8) = *reinterpret_cast<const bf16x8*>(smem + r * RS + ch * 16);
  }
}

hipError_t launch_im2col(const void* images, int in_bf16, void* col, int batch, int C, int H, int W, int p,
                         int Kp, hipStream_t s) {
  if (batch <= 0 || p <= 0 || H <= 0 || W <= 0 || H % p || W % p || (Kp & 63) || Kp < C * p * p) return hipErrorInvalidValue;
  const int gh = H / p, gw = W / p;
  if ((p & 7) && !(p & 1) && !(W & 1) && (((uintptr_t)images) & 7) == 0) {
    // even patch side that is not a multiple of 8: the LDS form
    const int tpb = gw < 32 ? gw : 32;
    const int bpr = (gw + tpb - 1) / tpb;
    const size_t lds = (size_t)tpb * (Kp * 2 + 32);
    if (lds <= 65536) {
      const dim3 grid((unsigned)((int64_t)batch * gh * bpr)), block(256);
      if (in_bf16)
        hipLaunchKernelGGL((im2col_rows_kernel<true>), grid, block, lds, s, images, (bf16_t*)col, C, H, W, p, gh, gw, Kp, tpb, bpr);
      else
        hipLaunchKernelGGL((im2col_rows_kernel<false>), grid, block, lds, s, images, (bf16_t*)col, C, H, W, p, gh, gw, Kp, tpb, bpr);
      return hipGetLastError();
    }
  }
  // the fast path reads 8 pixels with vector loads: needs p % 8 == 0 (and so W % 8 == 0) so that every
  // 8-pixel run starts 16-byte aligned (the image base is assumed 16-byte aligned)
  const int fast = ((p & 7) == 0 && (W & 7) == 0 && (((uintptr_t)images) & 15) == 0) ? 1 : 0;
  const int64_t total8 = (int64_t)batch * gh * gw * (Kp / 8);
  const dim3 grid((unsigned)((total8 + 255) / 256)), block(256);
  if (in_bf16)
    hipLaunchKernelGGL((im2col_kernel<true>), grid, block, 0, s, images, (bf16_t*)col, total8, C, H, W, p, gh, gw, Kp, fast);
  else
    hipLaunchKernelGGL((im2col_kernel<false>), grid, block, 0, s, images, (bf16_t*)col, total8, C, H, W, p, gh, gw, Kp, fast);
  return hipGetLastError();
}

// prefix rows of an image: x[b*row_stride][:] = cls + pos[0]; x[b*row_stride + 1 + r][:] = reg[r] (register tokens, r < P - 1:
// no position is added to them); one rounding to bf16
__global__ __launch_bounds__(256) void prefix_rows_kernel(const float* __restrict__ cls, const float* __restrict__ pos,
                                                          const float* __restrict__ reg, int P, bf16_t* __restrict__ x,
                                                          int batch, int64_t row_stride, int D) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)batch * P * D) return;
  const int64_t br = idx / D;
  const int d = (int)(idx - br * D);
  const int64_t b = br / P;
  const int p = (int)(br - b * P);
  const float v = p == 0 ? cls[d] + (pos ? pos[d] : 0.0f) : reg[(int64_t)(p - 1) * D + d];
  x[(b * row_stride + p) * D + d] = (bf16_t)v;
}

hipError_t launch_prefix_rows(const float* cls, const float* pos, const float* reg, int n_reg, void* x, int batch,
                              int64_t row_stride, int D, hipStream_t s) {
  if (n_reg < 0 || (n_reg > 0 && !reg) || row_stride < 1 + n_reg) return hipErrorInvalidValue;
  const int64_t total = (int64_t)batch * (1 + n_reg) * D;
  hipLaunchKernelGGL(prefix_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cls, pos, reg, 1 + n_reg,
                     (bf16_t*)x, batch, row_stride, D);
  return hipGetLastError();
}

// token model: x[b*(S+c) + c + i] = tok[b*S + i] (+ pos[c+i]);  x[b*(S+c)] = cls (+ pos[0])
template <bool IN_BF16>
__global__ __launch_bounds__(256) void assemble_kernel(const void* __restrict__ tok, const float* __restrict__ cls,
                                                       const float* __restrict__ pos, bf16_t* __restrict__ x,
                                                       int batch, int seq, int D, int has_cls) {
  const int N = seq + has_cls;
  const int d4 = D >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)batch * N * d4) return;
  const int64_t row = idx / d4;
  const int d = (int)(idx - row * d4) * 4;
  const int64_t b = row / N;
  const int t = (int)(row - b * N);
  float v[4];
  if (has_cls && t == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = cls[d + e];
  } else {
    const int64_t src = (b * seq + (t - has_cls)) * (int64_t)D + d;
    if (IN_BF16) {
      const bf16x4 a = *reinterpret_cast<const bf16x4*>((const bf16_t*)tok + src);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (float)a[e];
    } else {
      const f32x4 a = *reinterpret_cast<const f32x4*>((const float*)tok + src);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = a[e];
    }
  }
  if (pos) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += pos[(int64_t)t * D + d + e];
  }
  bf16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (bf16_t)v[e];
  *reinterpret_cast<bf16x4*>(x + row * D + d) = o;
}

hipError_t launch_assemble_tokens(const void* tok, int in_bf16, const float* cls, const float* pos, void* x,
                                  int batch, int seq, int D, int has_cls, hipStream_t s) {
  if (D & 3) return hipErrorInvalidValue;
  const int64_t total = (int64_t)batch * (seq + has_cls) * (D / 4);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (in_bf16)
    hipLaunchKernelGGL((assemble_kernel<true>), grid, block, 0, s, tok, cls, pos, (bf16_t*)x, batch, seq, D, has_cls);
  else
    hipLaunchKernelGGL((assemble_kernel<false>), grid, block, 0, s, tok, cls, pos, (bf16_t*)x, batch, seq, D, has_cls);
  return hipGetLastError();
}

// y[r][:] = x[imap(r)][:]  (bf16 or fp32 in; bf16 or fp32 out) — the x[:,0,:] / x[:,1:,:] slice for models
// without a final norm (post-LN nn.TransformerEncoder, models_archs.py:147), the raw residual stream of
// vdr_forward_layers (norm = 0), the fp32 copy of the stream (resid_fp32), a q / k / v facet out of the qkv activation
// (ldx = 3D).  Input row stride ldx, output row stride ldy elements.
template <bool IN_F32, bool OUT_BF16>
__global__ __launch_bounds__(256) void gather_rows_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                          int64_t rows, int D, int rpg, int64_t gs, int off, int64_t ldx,
                                                          int64_t ldy, int vec_out) {
  const int d4 = D >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * d4) return;
  const int64_t r = idx / d4;
  const int d = (int)(idx - r * d4) * 4;
  const int64_t ir = map_row(r, rpg, gs, off);
  float v[4];
  if (IN_F32) {
    const f32x4 a = *reinterpret_cast<const f32x4*>((const float*)x + ir * ldx + d);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = a[e];
  } else {
    const bf16x4 a = *reinterpret_cast<const bf16x4*>((const bf16_t*)x + ir * ldx + d);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)a[e];
  }
  const int64_t oi = r * ldy + d;
  if (OUT_BF16) {
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (bf16_t)v[e];
    if (vec_out) {
      *reinterpret_cast<bf16x4*>((bf16_t*)y + oi) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) ((bf16_t*)y)[oi + e] = o[e];
    }
  } else if (vec_out) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = v[e];
    *reinterpret_cast<f32x4*>((float*)y + oi) = o;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) ((float*)y)[oi + e] = v[e];
  }
}

hipError_t launch_gather_rows(const void* x, void* y, int out_bf16, int64_t rows, int D, RowMap imap,
                              hipStream_t s, int in_f32, int64_t ldy, int64_t ldx) {
  if ((D & 3) || (ldy != 0 && ldy < D) || (ldx != 0 && (ldx < D || (ldx & 3)))) return hipErrorInvalidValue;
  const int64_t total = rows * (D / 4);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const int64_t ld = ldy ? ldy : D;
  const int vec = ldy == 0 || rows_aligned(y, ld, out_bf16 ? 2 : 4);
#define VDR_GATHER(F, B)                                                                                                  \
  hipLaunchKernelGGL((gather_rows_kernel<F, B>), grid, block, 0, s, x, y, rows, D, imap.rpg, imap.gstride, imap.off, ldx ? ldx : (int64_t)D, ld, vec)
  if (in_f32) {
    if (out_bf16) VDR_GATHER(true, true); else VDR_GATHER(true, false);
  } else {
    if (out_bf16) VDR_GATHER(false, true); else VDR_GATHER(false, false);
  }
#undef VDR_GATHER
  return hipGetLastError();
}

// (sum, sumsq) partials per 64-column group -> (mean, rstd) per row.  The sums come from the producing
// GEMM's epilogue; variance = E[x^2] - mean^2 evaluated in double from the fp32 partials.
__global__ __launch_bounds__(64) void ln_finalize_kernel(const float* __restrict__ part, int groups, int64_t stride,
                                                          float* __restrict__ stats, int64_t rows, float eps) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= rows) return;
  double s1 = 0.0, s2 = 0.0;
  for (int g0 = 0; g0 < groups; g0 += 16) {
    float2 v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {  // 16 independent loads in flight (coalesced across the wave): one round trip for D <= 1024
      const int g = g0 + j < groups ? g0 + j : groups - 1;
      v[j] = *reinterpret_cast<const float2*>(part + ((int64_t)g * stride + r) * 2);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (g0 + j < groups) {
        s1 += (double)v[j].x;
        s2 += (double)v[j].y;
      }
  }
  *reinterpret_cast<float2*>(stats + r * 2) = ln_mean_rstd(s1, s2, groups, eps);
}

hipError_t launch_ln_finalize(const float* part, int groups, int64_t stride, float* stats, int64_t rows, int D,
                              float eps, hipStream_t s) {
  if (rows <= 0 || groups <= 0 || D != 64 * groups) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ln_finalize_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, s, part, groups, stride,
                     stats, rows, eps);
  return hipGetLastError();
}

// the prefix rows as prefix_rows_kernel, one wave per (image, prefix row, 64-column group), plus that group's partial sums
__global__ __launch_bounds__(64) void prefix_rows_stats_kernel(const float* __restrict__ cls, const float* __restrict__ pos,
                                                               const float* __restrict__ reg, int P, bf16_t* __restrict__ x,
                                                               float* __restrict__ part, int64_t part_stride, int groups,
                                                               int64_t row_stride, int D) {
  const int bp = blockIdx.x / groups, g = blockIdx.x - bp * groups;
  const int b = bp / P, p = bp - b * P;
  const int d = g * 64 + threadIdx.x;
  const int64_t row = (int64_t)b * row_stride + p;
  const bf16_t o = (bf16_t)(p == 0 ? cls[d] + (pos ? pos[d] : 0.0f) : reg[(int64_t)(p - 1) * D + d]);
  x[row * D + d] = o;
  const float r = (float)o;
  const float s1 = wave_sum(r), s2 = wave_sum(r * r);
  if (threadIdx.x == 0) {
    float* dst = part + ((int64_t)g * part_stride + row) * 2;
    dst[0] = s1;
    dst[1] = s2;
  }
}

hipError_t launch_prefix_rows_stats(const float* cls, const float* pos, const float* reg, int n_reg, void* x, float* part,
                                    int64_t part_stride, int batch, int64_t row_stride, int D, hipStream_t s) {
  if ((D & 63) || n_reg < 0 || (n_reg > 0 && !reg) || row_stride < 1 + n_reg) return hipErrorInvalidValue;
  const int groups = D / 64;
  hipLaunchKernelGGL(prefix_rows_stats_kernel, dim3((unsigned)(batch * (1 + n_reg) * groups)), dim3(64), 0, s, cls, pos, reg,
                     1 + n_reg, (bf16_t*)x, part, part_stride, groups, row_stride, D);
  return hipGetLastError();
}

// LayerNorm in place over bf16 rows that also leaves the (sum, sumsq) partials of its OUTPUT rows, one slot per (64-column
// group, row): the input LayerNorm of a model that keeps the LayerNorm fold (CLIP's pre_layrnorm, vdr_config.input_ln).
// Block 0's folded qkv GEMM reads part [D/64][part_stride][2] exactly as the patch epilogue and prefix_rows_stats_kernel
// leave it for a model without input LayerNorm.  One wave per row, the LayerNorm kernel's helpers (same bits as
// launch_layernorm on the same row); lane l holds columns 256 k + 4 l .. + 3 of pass k, so a 64-column group is 16
// neighbouring lanes of one pass: four xor-shuffle adds inside the 16-lane row, lane 0 of the row stores.  The sums are
// of the bf16 values stored (what the consumer multiplies).  No atomics; a row's bits do not depend on the batch.
template <int NP>
__global__ __launch_bounds__(256) void ln_rows_stats_kernel(bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, int64_t rows, int D,
                                                            float* __restrict__ part, int64_t part_stride) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float v[NP][4];
  row_load<true, NP>(x, r, D, lane, v);
  float mean, rstd;
  row_mean_rstd<NP>(v, D, lane, eps, mean, rstd);
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = k * 256 + lane * 4;
    float s1 = 0.0f, s2 = 0.0f;
    if (c < D) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
      const f32x4 bt = *reinterpret_cast<const f32x4*>(beta + c);
      bf16x4 ob;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ob[e] = (bf16_t)ln_affine(v[k][e], mean, rstd, g[e], bt[e]);
        const float q = (float)ob[e];
        s1 += q;
        s2 = fmaf(q, q, s2);
      }
      *reinterpret_cast<bf16x4*>(x + r * D + c) = ob;
    }
    // (every lane takes part in the exchange; D % 64 == 0, so a 16-lane row is inside D or outside it as a whole)
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o, 64);
      s2 += __shfl_xor(s2, o, 64);
    }
    if ((lane & 15) == 0 && c < D) {
      float* dst = part + ((int64_t)(c >> 6) * part_stride + r) * 2;
      dst[0] = s1;
      dst[1] = s2;
    }
  }
}

hipError_t launch_ln_rows_stats(void* x, const float* gamma, const float* beta, float eps, int64_t rows, int D, float* part,
                                int64_t part_stride, hipStream_t s) {
  if (rows <= 0 || D <= 0 || (D & 63) || D > 2048 || part_stride < rows) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define VDR_LNS(NP)                                                                                                          \
  case NP:                                                                                                                   \
    hipLaunchKernelGGL((ln_rows_stats_kernel<NP>), grid, block, 0, s, (bf16_t*)x, gamma, beta, eps, rows, D, part, part_stride); \
    break;
  switch ((D + 255) / 256) {
    VDR_LNS(1) VDR_LNS(2) VDR_LNS(3) VDR_LNS(4) VDR_LNS(5) VDR_LNS(6) VDR_LNS(7) VDR_LNS(8)
    default:
      return hipErrorInvalidValue;
  }
#undef VDR_LNS
  return hipGetLastError();
}

// 3x3 / pad 1 im2col over NHWC tokens (the SAM neck's second conv): one thread moves 8 channels (16 B)
__global__ __launch_bounds__(256) void im2col3_kernel(const bf16_t* __restrict__ y, bf16_t* __restrict__ col,
                                                      int64_t total, int g, int C) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c8 = C >> 3;
  const int64_t row = idx / (9 * c8);
  const int rem = (int)(idx - row * 9 * c8);
  const int j = rem / c8, c = (rem - j * c8) * 8;
  const int ky = j / 3, kx = j - ky * 3;
  const int64_t b = row / (g * g);
  const int pix = (int)(row - b * g * g);
  const int py = pix / g + ky - 1, px = pix % g + kx - 1;
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (bf16_t)0.0f;
  if (py >= 0 && py < g && px >= 0 && px < g) v = *reinterpret_cast<const bf16x8*>(y + ((b * g + py) * g + px) * (int64_t)C + c);
  *reinterpret_cast<bf16x8*>(col + row * (int64_t)(9 * C) + j * C + c) = v;
}

hipError_t launch_im2col3(const void* y, void* col, int batch, int g, int C, hipStream_t s) {
  if (C & 7) return hipErrorInvalidValue;
  const int64_t total = (int64_t)batch * g * g * 9 * (C / 8);
  hipLaunchKernelGGL(im2col3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const bf16_t*)y, (bf16_t*)col,
                     total, g, C);
  return hipGetLastError();
}

}  // namespace vdr
