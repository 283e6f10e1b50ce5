// The kernels of SAM's mask decoder for gfx950 (include/vdr.h, "mask decoder ops"): the two-way transformer works on 7 tokens
// per (image, box) problem against g*g image cells, so nothing here is shaped like the encoder's square attention or its
// large-M GEMMs.
//
//   cross_attention   softmax(q k^T dh^-1/2) v with a handful of rows on one side, operands read in place as column slices of
//                     wider buffers, an optional fp32 additive table per row on q and on k (the positional-encoding term of a
//                     stacked projection, shared by every problem):
//                       few keys  (tk <= 16): the problem's k and v in LDS as fp32, one lane per (query row, head);
//                       few queries (tq <= 16): the keys split over the 4 waves of a workgroup per (problem, head), one online
//                         softmax per (wave, key slot) and query, merged by a shuffle tree inside the wave and in wave order
//                         through LDS -- attention_pool's scheme with tq running sums.  k and v are read once, 16 bytes a lane.
//   token_linear      y = [relu](x W^T + b) [+ resid] for the token-side rows (M = a few per problem): 8 rows per workgroup in
//                     LDS, 16 output columns per workgroup with K split over 16 lanes each (fp32 fmaf chains, the 16 partial
//                     sums added in order through LDS).  `groups` weight sets, row r using set r % groups (the four
//                     hypernetwork MLPs in one launch).
//   mask_upscale      the tail: GELU of the LayerNorm2d rows, ConvTranspose2d(64, 32, 2, 2) on the MFMA, bias, GELU, the
//                     contraction with the problem's hyper [4, 32] and the scatter to [P, 4, 4g, 4g] fp32.  The 32-channel
//                     4g x 4g map is never written.
//
// Built with -ffp-contract=off (Makefile): every multiply and add outside the explicit fmaf calls is rounded once, so t - m is
// exactly 0 for the key that holds the maximum and equal keys give p = 1 (the designed inputs of tests/test_sam_decoder_gpu.py).
// No atomics; which lane sums what depends on the shapes only, never on the problem count or a problem's position.
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {

namespace {

constexpr float LOG2E = 1.44269504088896341f;
template <int DH>
constexpr float xattn_scale_log2e() {
  return DH == 16 ? 0.25f * LOG2E : 0.17677669529663688f * LOG2E;
}

struct XAttnArgs {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  const float* q_add;
  const float* k_add;
  bf16_t* out;
  int64_t ldq, ldk, ldv, ldo;
  int tq, tk, heads;
};

// ---- few keys: tk <= 16 --------------------------------------------------------------------------------------------------
constexpr int XA_TK = 16, XA_HD = 256;

template <int DH>
__global__ __launch_bounds__(256) void xattn_few_keys_kernel(XAttnArgs a) {
  __shared__ __attribute__((aligned(16))) float ks[XA_TK * XA_HD];
  __shared__ __attribute__((aligned(16))) float vs[XA_TK * XA_HD];
  const int p = blockIdx.y, HD = a.heads * DH;
  for (int idx = threadIdx.x; idx < a.tk * (HD / 8); idx += 256) {  // 16-byte chunks (HD is a multiple of 16)
    const int j = idx / (HD / 8), c = 8 * (idx - j * (HD / 8));
    const bf16x8 k8 = *reinterpret_cast<const bf16x8*>(a.k + ((int64_t)p * a.tk + j) * a.ldk + c);
    const bf16x8 v8 = *reinterpret_cast<const bf16x8*>(a.v + ((int64_t)p * a.tk + j) * a.ldv + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float kf = (float)k8[e];
      if (a.k_add) kf = kf + a.k_add[(int64_t)j * HD + c + e];
      ks[j * HD + c + e] = kf;
      vs[j * HD + c + e] = (float)v8[e];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  if (i >= a.tq) return;
  for (int h = wave; h < a.heads; h += 4) {
    float qf[DH];
    const bf16_t* qp = a.q + ((int64_t)p * a.tq + i) * a.ldq + h * DH;
#pragma unroll
    for (int c = 0; c < DH / 8; ++c) {
      const bf16x8 q8 = *reinterpret_cast<const bf16x8*>(qp + 8 * c);
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[8 * c + e] = (float)q8[e];
    }
    if (a.q_add) {
      const float* qa = a.q_add + (int64_t)i * HD + h * DH;
#pragma unroll
      for (int c = 0; c < DH / 4; ++c) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(qa + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) qf[4 * c + e] = qf[4 * c + e] + t[e];
      }
    }
    float t[XA_TK];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < XA_TK; ++j) {
      t[j] = -INFINITY;
      if (j < a.tk) {
        const float* kr = ks + j * HD + h * DH;
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) {
          const f32x4 k4 = *reinterpret_cast<const f32x4*>(kr + 4 * c);
#pragma unroll
          for (int e = 0; e < 4; ++e) s = fmaf(qf[4 * c + e], k4[e], s);
        }
        t[j] = s * xattn_scale_log2e<DH>();
        m = fmaxf(m, t[j]);
      }
    }
    float l = 0.0f, acc[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] = 0.0f;
#pragma unroll
    for (int j = 0; j < XA_TK; ++j) {
      if (j < a.tk) {
        const float pj = fast_exp2(t[j] - m);
        l = l + pj;
        const float* vr = vs + j * HD + h * DH;
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) {
          const f32x4 v4 = *reinterpret_cast<const f32x4*>(vr + 4 * c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[4 * c + e] = fmaf(pj, v4[e], acc[4 * c + e]);
        }
      }
    }
    bf16_t* op = a.out + ((int64_t)p * a.tq + i) * a.ldo + h * DH;
#pragma unroll
    for (int c = 0; c < DH / 8; ++c) {
      bf16x8 o8;
#pragma unroll
      for (int e = 0; e < 8; ++e) o8[e] = (bf16_t)(acc[8 * c + e] / l);
      *reinterpret_cast<bf16x8*>(op + 8 * c) = o8;
    }
  }
}

// ---- few queries: tq <= TQ, any tk -----------------------------------------------------------------------------------------
template <int DH, int TQ>
__global__ __launch_bounds__(256) void xattn_few_queries_kernel(XAttnArgs a) {
  constexpr int LPK = DH / 8, KPW = 64 / LPK, STEP = 4 * KPW, RS = DH + 4;
  __shared__ __attribute__((aligned(16))) float qs[TQ * DH];
  __shared__ __attribute__((aligned(16))) float sm[4 * TQ * RS];  // per (wave, query): acc[DH], m, l
  const int p = blockIdx.x / a.heads, h = blockIdx.x - p * a.heads;
  const int HD = a.heads * DH, tq = a.tq, n = a.tk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane / LPK, ch = lane - slot * LPK;
  for (int idx = threadIdx.x; idx < TQ * DH; idx += 256) {
    const int i = idx / DH, d = idx - i * DH;
    float qf = 0.0f;
    if (i < tq) {
      qf = (float)a.q[((int64_t)p * tq + i) * a.ldq + h * DH + d];
      if (a.q_add) qf = qf + a.q_add[(int64_t)i * HD + h * DH + d];
    }
    qs[idx] = qf;
  }
  __syncthreads();
  const bf16_t* kb = a.k + (int64_t)p * n * a.ldk + h * DH + 8 * ch;
  const bf16_t* vb = a.v + (int64_t)p * n * a.ldv + h * DH + 8 * ch;
  const float* kab = a.k_add ? a.k_add + h * DH + 8 * ch : nullptr;
  // (keys past the end read the last row: a valid address, the values are never used)
  auto load = [&](int j, bf16x8& k8, bf16x8& v8) {
    const int64_t jj = j < n ? j : n - 1;
    k8 = *reinterpret_cast<const bf16x8*>(kb + jj * a.ldk);
    v8 = *reinterpret_cast<const bf16x8*>(vb + jj * a.ldv);
  };
  float m[TQ], l[TQ], acc[TQ][8];
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    m[i] = -INFINITY;
    l[i] = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.0f;
  }
  int j = wave * KPW + slot;
  bf16x8 kc, vc;
  load(j, kc, vc);
  for (int j0 = 0; j0 < n; j0 += STEP) {  // (workgroup-uniform trip count: every lane takes part in the shuffles)
    bf16x8 kn, vn;
    load(j + STEP, kn, vn);
    float kf[8], vf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      kf[e] = (float)kc[e];
      vf[e] = (float)vc[e];
    }
    if (kab) {
      const float* ka = kab + (int64_t)(j < n ? j : n - 1) * HD;
      const f32x4 t0 = *reinterpret_cast<const f32x4*>(ka), t1 = *reinterpret_cast<const f32x4*>(ka + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        kf[e] = kf[e] + t0[e];
        kf[4 + e] = kf[4 + e] + t1[e];
      }
    }
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
      if (i < tq) {  // (uniform)
        const float* qr = qs + i * DH + 8 * ch;
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(qr), q1 = *reinterpret_cast<const f32x4*>(qr + 4);
        float s = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(kf[e], q0[e], s);
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(kf[4 + e], q1[e], s);
        s = s + __shfl_xor(s, 1, 64);
        if (LPK == 4) s = s + __shfl_xor(s, 2, 64);
        const float t = s * xattn_scale_log2e<DH>();
        if (j < n) {
          const float mn = fmaxf(m[i], t);
          const float sc = fast_exp2(m[i] - mn), pj = fast_exp2(t - mn);
          l[i] = fmaf(l[i], sc, pj);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[i][e] = fmaf(acc[i][e], sc, pj * vf[e]);
          m[i] = mn;
        }
      }
    }
    kc = kn;
    vc = vn;
    j += STEP;
  }
  // the KPW slots of a wave meet in a shuffle tree (lanes of equal ch: strides LPK, 2 LPK, .. 32), the 4 waves in LDS
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    if (i < tq) {
      float M = m[i];
#pragma unroll
      for (int o = LPK; o < 64; o <<= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
      const float f = m[i] == -INFINITY ? 0.0f : fast_exp2(m[i] - M);  // (a slot that saw no key)
      float li = l[i] * f, ai[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ai[e] = acc[i][e] * f;
#pragma unroll
      for (int o = LPK; o < 64; o <<= 1) {
        li = li + __shfl_xor(li, o, 64);
#pragma unroll
        for (int e = 0; e < 8; ++e) ai[e] = ai[e] + __shfl_xor(ai[e], o, 64);
      }
      if (slot == 0) {
        float* dst = sm + (wave * TQ + i) * RS;
        *reinterpret_cast<f32x4*>(dst + 8 * ch) = f32x4{ai[0], ai[1], ai[2], ai[3]};
        *reinterpret_cast<f32x4*>(dst + 8 * ch + 4) = f32x4{ai[4], ai[5], ai[6], ai[7]};
        if (ch == 0) {
          dst[DH] = M;
          dst[DH + 1] = li;
        }
      }
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < tq * DH; idx += 256) {
    const int i = idx / DH, d = idx - i * DH;
    float M = -INFINITY;
    for (int w = 0; w < 4; ++w) M = fmaxf(M, sm[(w * TQ + i) * RS + DH]);
    float L = 0.0f, A = 0.0f;
    for (int w = 0; w < 4; ++w) {
      const float mw = sm[(w * TQ + i) * RS + DH];
      const float f = mw == -INFINITY ? 0.0f : fast_exp2(mw - M);  // (a wave that saw no key)
      L = fmaf(sm[(w * TQ + i) * RS + DH + 1], f, L);
      A = fmaf(sm[(w * TQ + i) * RS + d], f, A);
    }
    a.out[((int64_t)p * tq + i) * a.ldo + h * DH + d] = (bf16_t)(A / L);
  }
}

// ---- token-side linear -------------------------------------------------------------------------------------------------------
constexpr int TL_ROWS = 8, TL_MAX_K = 2048;

struct TokLinArgs {
  const bf16_t* x;
  const bf16_t* x_add;
  const bf16_t* W;
  const float* bias;
  const bf16_t* resid;
  void* y;
  int64_t ldx, ldxa, ldr, ldy;
  int M, N, K, groups, relu, out_f32;
  int x_rpg;       // > 0: row r of x starts at element (r / x_rpg) * x_gs + (r % x_rpg) * ldx (the mask tokens of every problem)
  int64_t x_gs;
};

// 16 output columns per workgroup, K split 16 ways: thread (c = tid & 15, ks = tid >> 4) sums the 8-element chunks j = ks, ks + 16,
// ks + 32, .. of column c's weight row (the 16 ks of a column read one contiguous 256-byte run per step), the 16 partial sums
// of a (row, column) meet in LDS and are added in ascending ks.
constexpr int TL_COLS = 16, TL_KS = 16;

__global__ __launch_bounds__(256) void token_linear_kernel(TokLinArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[TL_ROWS * TL_MAX_K];
  __shared__ float red[TL_KS][TL_ROWS][TL_COLS + 1];
  const int g = blockIdx.y % a.groups, tile = blockIdx.y / a.groups;
  // row i of this workgroup is r = (tile * TL_ROWS + i) * groups + g
  for (int idx = threadIdx.x; idx < TL_ROWS * a.K; idx += 256) {
    const int i = idx / a.K, k = idx - i * a.K;
    const int64_t r = ((int64_t)tile * TL_ROWS + i) * a.groups + g;
    float xf = 0.0f;
    if (r < a.M) {
      const int64_t xo = a.x_rpg > 0 ? (r / a.x_rpg) * a.x_gs + (r % a.x_rpg) * a.ldx : r * a.ldx;
      xf = (float)a.x[xo + k];
      if (a.x_add) xf = (float)(bf16_t)(xf + (float)a.x_add[r * a.ldxa + k]);
    }
    xs[i * a.K + k] = xf;
  }
  __syncthreads();
  const int c = threadIdx.x & (TL_COLS - 1), ks = threadIdx.x >> 4;
  const int n = blockIdx.x * TL_COLS + c;
  const int nc = n < a.N ? n : a.N - 1;  // (columns past the end read the last row: a valid address, never stored)
  const bf16_t* w = a.W + ((int64_t)g * a.N + nc) * a.K;
  float acc[TL_ROWS];
#pragma unroll
  for (int i = 0; i < TL_ROWS; ++i) acc[i] = 0.0f;
  for (int k0 = 8 * ks; k0 < a.K; k0 += 8 * TL_KS) {
    const bf16x8 w8 = *reinterpret_cast<const bf16x8*>(w + k0);
    float wf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) wf[e] = (float)w8[e];
#pragma unroll
    for (int i = 0; i < TL_ROWS; ++i) {
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(xs + i * a.K + k0), x1 = *reinterpret_cast<const f32x4*>(xs + i * a.K + k0 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i] = fmaf(x0[e], wf[e], acc[i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i] = fmaf(x1[e], wf[4 + e], acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < TL_ROWS; ++i) red[ks][i][c] = acc[i];
  __syncthreads();
  if (threadIdx.x >= TL_ROWS * TL_COLS) return;
  const int i = threadIdx.x >> 4;  // (c as above: 16 consecutive columns of one row per 16 lanes)
  const int64_t r = ((int64_t)tile * TL_ROWS + i) * a.groups + g;
  if (r >= a.M || n >= a.N) return;
  float v = red[0][i][c];
#pragma unroll
  for (int q = 1; q < TL_KS; ++q) v = v + red[q][i][c];
  v = v + (a.bias ? a.bias[(int64_t)g * a.N + n] : 0.0f);
  if (a.relu) v = fmaxf(v, 0.0f);
  if (a.resid) v = v + (float)a.resid[r * a.ldr + n];
  if (a.out_f32) reinterpret_cast<float*>(a.y)[r * a.ldy + n] = v;
  else reinterpret_cast<bf16_t*>(a.y)[r * a.ldy + n] = (bf16_t)v;
}

// ---- the upscale tail ------------------------------------------------------------------------------------------------------
// Row R = (p * g*g + cy * g + cx) * 4 + dy1 * 2 + dx1 of x [P g g 4, 64] is pixel (2 cy + dy1, 2 cx + dx1) of the 2g x 2g map.
// One wave per 32 rows; for each of the 4 sub-pixels s2 = dy2 * 2 + dx2 one 32 x 32 x 64 product on mfma_f32_32x32x16_bf16 with
// the WEIGHT as the A operand (its row = output channel) and the data rows as B, so that a lane holds 16 of one data row's 32
// channels (c = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) and the contraction with hyper [4, 32] is an fmaf chain over its
// registers in ascending reg, then lower half-wave + upper half-wave.
__global__ __launch_bounds__(256) void mask_upscale_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W,
                                                           const float* __restrict__ bias, const float* __restrict__ hyper,
                                                           float* __restrict__ out, int64_t rows, int g, int gelu_in) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
  if (row0 >= rows) return;  // (wave-uniform; no workgroup barrier below)
  const int64_t R = row0 + r, Rc = R < rows ? R : rows - 1;
  bf16x8 xf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    xf[s] = *reinterpret_cast<const bf16x8*>(x + Rc * 64 + 16 * s + 8 * hh);
    if (gelu_in) {
#pragma unroll
      for (int e = 0; e < 8; ++e) xf[s][e] = (bf16_t)gelu_erf((float)xf[s][e]);
    }
  }
  const int n = g * g;
  const int64_t cellp = Rc >> 2;
  const int sub1 = (int)(Rc & 3);
  const int64_t p = cellp / n;
  const int cell = (int)(cellp - p * n);
  const int cy = cell / g, cx = cell - cy * g;
  const int y1 = 2 * cy + (sub1 >> 1), x1 = 2 * cx + (sub1 & 1);
  float hy[4][16], bs[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias + 8 * q + 4 * hh);
#pragma unroll
    for (int e = 0; e < 4; ++e) bs[4 * q + e] = b4[e];
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
      const f32x4 h4 = *reinterpret_cast<const f32x4*>(hyper + (p * 4 + mm) * 32 + 8 * q + 4 * hh);
#pragma unroll
      for (int e = 0; e < 4; ++e) hy[mm][4 * q + e] = h4[e];
    }
  }
  const int G4 = 4 * g;
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16x8 wf = *reinterpret_cast<const bf16x8*>(W + (s2 * 32 + r) * 64 + 16 * s + 8 * hh);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf[s], acc, 0, 0, 0);
    }
    float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float u = gelu_erf(acc[e] + bs[e]);
#pragma unroll
      for (int mm = 0; mm < 4; ++mm) part[mm] = fmaf(hy[mm][e], u, part[mm]);
    }
    float tot[4];
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
      const float other = __shfl_xor(part[mm], 32, 64);
      tot[mm] = hh ? other + part[mm] : part[mm] + other;  // lower half-wave's channels first
    }
    if (R < rows) {
      const int Y = 2 * y1 + (s2 >> 1), X = 2 * x1 + (s2 & 1);
#pragma unroll
      for (int mm = 0; mm < 2; ++mm) {
        const int ms = 2 * hh + mm;  // the lower lane of a pair stores masks 0, 1, the upper 2, 3
        out[((p * 4 + ms) * G4 + Y) * G4 + X] = hh ? tot[2 + mm] : tot[mm];
      }
    }
  }
}

// ---- the decode's set-up ---------------------------------------------------------------------------------------------------
// tokens [P, 7, 256] bf16: rows 0 .. 4 the iou / mask tokens (fixed [5, 256] fp32), rows 5, 6 the box corners: the Fourier features
// cat(sin, cos)(2 pi (2 c - 1) G), c = (corner + 0.5) / img, in double, plus the corner embedding.  2 * 128 sines and cosines per
// box, once per decode: this is the one place a kernel of the library evaluates trigonometry, on a few hundred values.
__global__ void decoder_tokens_kernel(const float* __restrict__ boxes, const float* __restrict__ fixed, const float* __restrict__ gauss,
                                      const float* __restrict__ corner, bf16_t* __restrict__ tok, int P, float img) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * 7 * 256) return;
  const int c = idx & 255, t = (idx >> 8) % 7, p = idx / (7 * 256);
  float v;
  if (t < 5) {
    v = fixed[t * 256 + c];
  } else {
    const int corner_i = t - 5, f = c & 127;
    const double x = ((double)boxes[p * 4 + 2 * corner_i] + 0.5) / (double)img, y = ((double)boxes[p * 4 + 2 * corner_i + 1] + 0.5) / (double)img;
    const double ph = 6.283185307179586476925286766559 * ((2.0 * x - 1.0) * (double)gauss[f] + (2.0 * y - 1.0) * (double)gauss[128 + f]);
    v = (float)((c < 128 ? sin(ph) : cos(ph)) + (double)corner[corner_i * 256 + c]);
  }
  tok[idx] = (bf16_t)v;
}

// keys [P n, 256] bf16 = bf16(emb + no_mask): emb fp32 [B, 256, n] (channels_last = 0) or [B, n, 256] (1), problem p reads image p / nb
__global__ void decoder_keys_kernel(const float* __restrict__ emb, const float* __restrict__ no_mask, bf16_t* __restrict__ keys, int64_t total,
                                    int n, int nb, int channels_last) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx & 255);
  const int64_t row = idx >> 8, p = row / n;
  const int cell = (int)(row - p * n);
  const int64_t b = p / nb;
  const float e = channels_last ? emb[(b * n + cell) * 256 + c] : emb[(b * 256 + c) * n + cell];
  keys[idx] = (bf16_t)(e + no_mask[c]);
}

}  // namespace

hipError_t launch_decoder_setup(const float* boxes, const float* fixed, const float* gauss, const float* corner, const float* emb,
                                int channels_last, const float* no_mask, void* tok, void* keys, int B, int nb, int g, float img, hipStream_t s) {
  const int P = B * nb, n = g * g;
  if (B <= 0 || nb <= 0 || g <= 0 || (int64_t)P * n * 256 > ((int64_t)1 << 40)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(decoder_tokens_kernel, dim3((unsigned)((P * 7 * 256 + 255) / 256)), dim3(256), 0, s, boxes, fixed, gauss, corner, (bf16_t*)tok, P, img);
  const int64_t total = (int64_t)P * n * 256;
  hipLaunchKernelGGL(decoder_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, emb, no_mask, (bf16_t*)keys, total, n, nb, channels_last);
  return hipGetLastError();
}

// the keys alone (decoder_keys_kernel): what a decode with prompts but without a mask prompt launches next to its own tokens kernel
hipError_t launch_decoder_keys(const float* emb, int channels_last, const float* no_mask, void* keys, int B, int nb, int g, hipStream_t s) {
  const int P = B * nb, n = g * g;
  if (B <= 0 || nb <= 0 || g <= 0 || (int64_t)P * n * 256 > ((int64_t)1 << 40)) return hipErrorInvalidValue;
  const int64_t total = (int64_t)P * n * 256;
  hipLaunchKernelGGL(decoder_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, emb, no_mask, (bf16_t*)keys, total, n, nb, channels_last);
  return hipGetLastError();
}

hipError_t launch_cross_attention(const void* q, int64_t ldq, const float* q_add, const void* k, int64_t ldk, const float* k_add,
                                  const void* v, int64_t ldv, void* out, int64_t ldo, int problems, int tq, int tk, int heads,
                                  int head_dim, hipStream_t s) {
  if (problems <= 0 || tq <= 0 || tk <= 0 || heads <= 0 || (head_dim != 16 && head_dim != 32)) return hipErrorInvalidValue;
  const int64_t HD = (int64_t)heads * head_dim;
  if (ldq < HD || ldk < HD || ldv < HD || ldo < HD || ((ldq | ldk | ldv | ldo) & 7)) return hipErrorInvalidValue;
  if ((int64_t)problems * heads > 0x7fffffff || problems > 65535) return hipErrorInvalidValue;
  XAttnArgs a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, q_add, k_add, (bf16_t*)out, ldq, ldk, ldv, ldo, tq, tk, heads};
  if (tk <= XA_TK) {
    if (HD > XA_HD) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((tq + 63) / 64), (unsigned)problems);
    if (head_dim == 16) hipLaunchKernelGGL((xattn_few_keys_kernel<16>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((xattn_few_keys_kernel<32>), grid, dim3(256), 0, s, a);
  } else if (tq <= 16) {
    const dim3 grid((unsigned)(problems * heads));
    if (head_dim == 16 && tq <= 8) hipLaunchKernelGGL((xattn_few_queries_kernel<16, 8>), grid, dim3(256), 0, s, a);
    else if (head_dim == 16) hipLaunchKernelGGL((xattn_few_queries_kernel<16, 16>), grid, dim3(256), 0, s, a);
    else if (tq <= 8) hipLaunchKernelGGL((xattn_few_queries_kernel<32, 8>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((xattn_few_queries_kernel<32, 16>), grid, dim3(256), 0, s, a);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_token_linear(const void* x, int64_t ldx, const void* x_add, int64_t ldxa, const void* W, const float* bias,
                               const void* resid, int64_t ldr, void* y, int out_f32, int64_t ldy, int M, int N, int K, int groups,
                               int relu, hipStream_t s, int x_rpg, int64_t x_gs) {
  if (M <= 0 || N <= 0 || K <= 0 || (K & 7) || K > TL_MAX_K || groups <= 0 || groups > M) return hipErrorInvalidValue;
  if (ldx < K || (x_add && ldxa < K) || (resid && ldr < N) || ldy < N) return hipErrorInvalidValue;
  const int per_group = (M + groups - 1) / groups;
  const int64_t gy = (int64_t)((per_group + TL_ROWS - 1) / TL_ROWS) * groups;
  if (gy > 65535) return hipErrorInvalidValue;
  TokLinArgs a{(const bf16_t*)x, (const bf16_t*)x_add, (const bf16_t*)W, bias, (const bf16_t*)resid, y, ldx, ldxa, ldr, ldy,
               M, N, K, groups, relu, out_f32, x_rpg, x_gs};
  hipLaunchKernelGGL(token_linear_kernel, dim3((unsigned)((N + TL_COLS - 1) / TL_COLS), (unsigned)gy), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_mask_upscale(const void* x, const void* W, const float* bias, const float* hyper, float* out, int problems,
                               int g, int gelu_in, hipStream_t s) {
  if (problems <= 0 || g <= 0 || g > 64) return hipErrorInvalidValue;
  const int64_t rows = (int64_t)problems * g * g * 4;
  const int64_t blocks = (rows + 127) / 128;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mask_upscale_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)W, bias, hyper,
                     out, rows, g, gelu_in);
  return hipGetLastError();
}

}  // namespace vdr
