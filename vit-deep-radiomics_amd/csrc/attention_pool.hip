// One-query attention pooling for gfx950: the core of SigLIP's multihead attention pooling head (transformers
// SiglipMultiheadAttentionPoolingHead: one learned probe attends over every token of the image).
//
//   out[b, h*dh + d] = sum_j softmax_j(q_h . k[b, j, h] dh^-1/2) v[b, j, h, d],   j < n
//
// q [H*dh] fp32 is the projected probe, the same for every image; kv [B*n, ldkv] bf16 holds k in columns [0, H*dh) and v
// in [H*dh, 2 H*dh) (the output of one k/v GEMM); out [B, H*dh] bf16.
//
// The kernel is memory-bound: B n 2D bf16 are read once, in 16-byte loads, and nothing else of size moves.  One
// workgroup of 4 waves per (image, head).  A key's head slice is dh/8 chunks of 16 bytes, one per lane: LPK = dh / 8 lanes
// per key, KPW = 64 / LPK keys per wave and step (16 / 8 / 5 / 4 for dh 32 / 64 / 96 / 128; dh 96 leaves 4 lanes idle),
// wave w takes keys w KPW + slot + 4 KPW i.  A lane multiplies its 8 k values with its 8 q values (fp32 fma chain), the
// LPK lanes of a key add up (xor-shuffles inside groups of 4, then the group sums in order), and every (wave, slot)
// runs its own online softmax over its keys in fp32: running maximum m, l = sum p, acc[8] = sum p v for the lane's 8
// columns, p = 2^(t - m), t = s c with c the fp32 dh^-1/2 log2(e) of the attention kernels.  The next step's k and v are
// requested before the current step's arithmetic.  At the end the 4 KPW partial states meet in LDS and are combined in
// slot order: M = max m_s, out = (sum_s acc_s 2^(m_s - M)) / (sum_s l_s 2^(m_s - M)), one IEEE division per output, one
// rounding to bf16.  No atomics; the key -> (wave, slot) map depends on n only, so a row's bits do not depend on the
// batch it travels in.
// Built with -ffp-contract=off (Makefile): every multiply and add outside the explicit fmaf calls is rounded once, so that
// t - m is exactly 0 for the key that holds the maximum (contracted into fma(s, c, -m) it would be the rounding residual of t).
// Designed inputs (tests/test_clip_ops_gpu.py): all keys equal -> every p is 2^0 = 1, acc = sum v exactly, out =
// bf16(sum v / n); one key ahead by a margin that underflows every other 2^x -> out = that key's v row exactly.
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {

namespace {

constexpr int POOL_WAVES = 4;

template <int DH>
constexpr float pool_scale_log2e() {
  return DH == 64   ? 0.125f * 1.44269504088896341f
         : DH == 32 ? 0.17677669529663688f * 1.44269504088896341f
         : DH == 96 ? 0.10206207261596575f * 1.44269504088896341f
                    : 0.08838834764831845f * 1.44269504088896341f;
}

template <int DH>
__global__ __launch_bounds__(POOL_WAVES * 64) void attention_pool_kernel(const float* __restrict__ q, const bf16_t* __restrict__ kv,
                                                                        int64_t ldkv, bf16_t* __restrict__ out, int n, int heads) {
  constexpr int LPK = DH / 8, KPW = 64 / LPK, SLOTS = POOL_WAVES * KPW, RS = DH + 4;
  __shared__ __attribute__((aligned(16))) float sm[SLOTS * RS];  // per (wave, slot): acc[DH], m, l
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane / LPK, ch = lane - slot * LPK;
  const bool live = slot < KPW;
  const int D = heads * DH;
  float qv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) qv[e] = q[h * DH + 8 * ch + e];
  const bf16_t* base = kv + (int64_t)b * n * ldkv + h * DH + 8 * ch;
  // (keys past the end and the idle lanes read the last row: a valid address, the values are never used)
  auto load = [&](int j, bf16x8& k8, bf16x8& v8) {
    const bf16_t* p = base + (int64_t)(j < n ? j : n - 1) * ldkv;
    k8 = *reinterpret_cast<const bf16x8*>(p);
    v8 = *reinterpret_cast<const bf16x8*>(p + D);
  };
  float m = -INFINITY, l = 0.0f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
  int j = wave * KPW + (live ? slot : 0);
  bf16x8 kc, vc;
  load(j, kc, vc);
  for (int j0 = 0; j0 < n; j0 += SLOTS) {  // (workgroup-uniform trip count: every lane takes part in the exchanges)
    bf16x8 kn, vn;
    load(j + SLOTS, kn, vn);
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf((float)kc[e], qv[e], s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    float t = 0.0f;
#pragma unroll
    for (int i = 0; i < LPK / 4; ++i) t += __shfl(s, (slot * LPK + 4 * i) & 63, 64);
    t *= pool_scale_log2e<DH>();
    if (live && j < n) {
      const float mn = fmaxf(m, t);
      const float sc = fast_exp2(m - mn), p = fast_exp2(t - mn);
      l = fmaf(l, sc, p);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(acc[e], sc, p * (float)vc[e]);
      m = mn;
    }
    kc = kn;
    vc = vn;
    j += SLOTS;
  }
  if (live) {
    float* dst = sm + (wave * KPW + slot) * RS;
    *reinterpret_cast<f32x4*>(dst + 8 * ch) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(dst + 8 * ch + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    if (ch == 0) {
      dst[DH] = m;
      dst[DH + 1] = l;
    }
  }
  __syncthreads();
  const int d = threadIdx.x;
  if (d < DH) {
    float M = -INFINITY;
    for (int s = 0; s < SLOTS; ++s) M = fmaxf(M, sm[s * RS + DH]);
    float L = 0.0f, A = 0.0f;
    for (int s = 0; s < SLOTS; ++s) {  // (a slot that saw no key has m = -inf: its factor is 2^-inf = 0)
      const float f = fast_exp2(sm[s * RS + DH] - M);
      L = fmaf(sm[s * RS + DH + 1], f, L);
      A = fmaf(sm[s * RS + d], f, A);
    }
    out[(int64_t)b * D + h * DH + d] = (bf16_t)(A / L);
  }
}

}  // namespace

hipError_t launch_attention_pool(const float* q, const void* kv, int64_t ldkv, void* out, int batch, int n, int heads,
                                 int head_dim, hipStream_t s) {
  if (batch <= 0 || n <= 0 || heads <= 0 || (int64_t)batch * heads > 0x7fffffff) return hipErrorInvalidValue;
  if (ldkv < (int64_t)2 * heads * head_dim || (ldkv & 7) || ((uintptr_t)kv & 15)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(batch * heads)), block(POOL_WAVES * 64);
#define VDR_POOL(DH)                                                                                                        \
  case DH:                                                                                                                  \
    hipLaunchKernelGGL((attention_pool_kernel<DH>), grid, block, 0, s, q, (const bf16_t*)kv, ldkv, (bf16_t*)out, n, heads); \
    break;
  switch (head_dim) {
    VDR_POOL(32) VDR_POOL(64) VDR_POOL(96) VDR_POOL(128)
    default:
      return hipErrorInvalidValue;
  }
#undef VDR_POOL
  return hipGetLastError();
}

}  // namespace vdr
