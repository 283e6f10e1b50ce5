// Attention maps for gfx950: the normalised softmax probabilities P = softmax(q k^T dh^-1/2) of the first q_rows query
// rows of every (sequence, head), from the packed qkv activation the attention kernels read (head dims 32, 64, 96, 128,
// any seq >= 1).  The fused kernels (attention.hip, attention_hd.hip) never store P; this kernel recomputes the scores.
//
// Arithmetic, fixed so that designed inputs have exactly known outputs (the file is built with -ffp-contract=off: every
// multiply and add below is its own rounding):
//   s = q.k in fp32 on the bf16 MFMA;  t = s * c, c = dh^-1/2 log2(e) as the attention kernels spell it;
//   m = max_k t;  e = exp2(t - m);  l = sum_k e (fp32, a fixed order);  r = 1 / l (one correctly rounded division);
//   p = e * r.  head_mean: (p_0 + p_1 + ... + p_{H-1}, in head order) * RN(1 / H).
// So a uniform row is exactly RN(1/seq), a row with one surviving key is exactly 1.0.  No atomics: a (sequence, head)
// row's bits depend neither on batch nor on the launch.
//
// One workgroup (1..4 waves) per (sequence, head, block of query tiles); head_mean: per (sequence, block of query tiles),
// looping over the heads.  Wave w owns query tile w (32 queries) of the block and reads K straight from global memory
// (one (sequence, head)'s keys are a few tens of KB, shared through L2 by every wave that reads them).  Three passes
// over the keys, 32 keys per MFMA tile:
//   1. S^T = K.Q^T (key on the accumulator row, query on the lane, as in attention_hd.hip): m per query, lane-local
//   2. the same scores again: l = sum e, then r = 1/l; (m, r) go to LDS
//   3. S = Q.K^T (the same fragments as the A / B operands swapped: key on the lane): p = e * r, and one store
//      instruction writes 32 consecutive keys of two query rows -- whole 128-byte lines of an fp32 map
// The MFMA's fp32 sum over k does not depend on which operand is A, so pass 3's scores are pass 1's, bit for bit.
#include "attention_tile.h"

namespace vdr {

struct AttnProbsK {
  const bf16_t* qkv;
  void* out;
  int seq, heads, q_rows;
  int64_t ld_qkv;
  float inv_heads;  // RN(1 / heads)
};

template <int DH, bool MEAN, bool BF16>
__global__ __launch_bounds__(256) void attn_probs_kernel(AttnProbsK p) {
  constexpr int KS = DH / 16;  // 16-deep k steps of one 32 x 32 score tile
  constexpr float sc = attn_scale_log2e<DH>();  // (a constant: untouched by this file's -ffp-contract=off)
  extern __shared__ float2 smr[];  // [wave][head of the loop][32 queries] (m, r)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  const int hh = lane >> 5;
  const int l31 = lane & 31;

  // grid: (sequence, head) x blocks of nw query tiles, block fastest, XCD-contiguous (the blocks of one (sequence,
  // head) share an L2 and its K)
  const int nqt = (p.q_rows + 31) >> 5;
  const int nqb = (nqt + nw - 1) / nw;
  const int nh = MEAN ? 1 : p.heads;  // heads of the grid
  const int hn = MEAN ? p.heads : 1;  // heads a workgroup loops over
  const int vid = nqb > 1 ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
  const int bh = vid / nqb;
  const int qblk = vid - bh * nqb;
  const int b = bh / nh;
  const int h0 = MEAN ? 0 : bh - b * nh;
  const int qt = qblk * nw + wave;
  const bool active = qt < nqt;  // wave-uniform
  const int seq = p.seq;
  const int nkt = (seq + 31) >> 5;
  const bf16_t* qb = p.qkv + (int64_t)b * seq * p.ld_qkv;
  const bf16_t* kb = qb + (int64_t)p.heads * DH;
  // query rows past q_rows are computed as a copy of the last one and never stored; keys past seq read the last key and
  // are masked (passes 1, 2) or not stored (pass 3)
  const int qrow = min(qt * 32 + l31, p.q_rows - 1);
  float2* mr = smr + wave * hn * 32;

  // lane (l31, hh) holds dims 16 ks + 8 hh .. +7 of row l31 of the tile: the B operand of S^T = K.Q^T and the A operand
  // of S = Q.K^T for Q, the other operand of each for K
  auto load_q = [&](int h, bf16x8 (&qf)[KS]) {
    const bf16_t* src = qb + (int64_t)qrow * p.ld_qkv + h * DH + hh * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(src + ks * 16);
  };
  auto load_k = [&](int h, int k0, bf16x8 (&kf)[KS]) {
    const bf16_t* src = kb + (int64_t)min(k0 + l31, seq - 1) * p.ld_qkv + h * DH + hh * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kf[ks] = *reinterpret_cast<const bf16x8*>(src + ks * 16);
  };
  auto scores_t = [&](const bf16x8 (&kf)[KS], const bf16x8 (&qf)[KS], int k0) {  // S^T tile, keys >= seq at -inf
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);
    if (k0 + 32 > seq) mask_keys(s, k0, hh, seq);
    return s;
  };

  if (active) {
    for (int hi = 0; hi < hn; ++hi) {
      const int h = h0 + hi;
      bf16x8 qf[KS], kf[KS], kn[KS];
      load_q(h, qf);
      // pass 1: m = max_k RN(s c) = RN(max_k s * c) (rounding is monotonic and c > 0)
      float smax = -INFINITY;
      load_k(h, 0, kf);
      for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) load_k(h, (kt + 1) * 32, kn);
        f32x16 st[1] = {scores_t(kf, qf, kt * 32)};
        smax = fmaxf(smax, row_max_tiles<1>(st));
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = kn[ks];
      }
      smax = fmaxf(smax, __shfl_xor(smax, 32, 64));
      const float m = smax * sc;
      // pass 2: l = sum_k exp2(s c - m), even / odd accumulator elements apart, folded at the end
      f32x2 l2 = {0.0f, 0.0f};
      load_k(h, 0, kf);
      for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) load_k(h, (kt + 1) * 32, kn);
        const f32x16 s = scores_t(kf, qf, kt * 32);
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          f32x2 x = {fast_exp2(s[e] * sc - m), fast_exp2(s[e + 1] * sc - m)};
          l2 += x;
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = kn[ks];
      }
      float l = l2[0] + l2[1];
      l += __shfl_xor(l, 32, 64);
      if (hh == 0) mr[hi * 32 + l31] = make_float2(m, 1.0f / l);
    }
  }
  __syncthreads();
  if (!active) return;

  // pass 3: lane (key l31, hh) holds rows (e & 3) + 8 (e >> 2) + 4 hh of the tile in accumulator element e
  const int64_t obase = MEAN ? (int64_t)b * p.q_rows : ((int64_t)b * p.heads + h0) * p.q_rows;
  auto row_stats = [&](int hi, float (&mm)[16], float (&rr)[16]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4* src = reinterpret_cast<const float4*>(mr + hi * 32 + 8 * g + 4 * hh);
      const float4 a = src[0], c = src[1];
      mm[4 * g + 0] = a.x, rr[4 * g + 0] = a.y, mm[4 * g + 1] = a.z, rr[4 * g + 1] = a.w;
      mm[4 * g + 2] = c.x, rr[4 * g + 2] = c.y, mm[4 * g + 3] = c.z, rr[4 * g + 3] = c.w;
    }
  };
  auto scores = [&](const bf16x8 (&qf)[KS], const bf16x8 (&kf)[KS]) {
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[ks], kf[ks], s, 0, 0, 0);
    return s;
  };
  auto store_tile = [&](const f32x16& pv, int k0) {
    const int key = k0 + l31;
    if (key >= seq) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = qt * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      if (row >= p.q_rows) continue;
      const int64_t idx = (obase + row) * seq + key;
      if constexpr (BF16)
        reinterpret_cast<bf16_t*>(p.out)[idx] = (bf16_t)pv[e];
      else
        reinterpret_cast<float*>(p.out)[idx] = pv[e];
    }
  };

  if constexpr (!MEAN) {
    bf16x8 qf[KS], kf[KS], kn[KS];
    float mm[16], rr[16];
    load_q(h0, qf);
    row_stats(0, mm, rr);
    load_k(h0, 0, kf);
    for (int kt = 0; kt < nkt; ++kt) {
      if (kt + 1 < nkt) load_k(h0, (kt + 1) * 32, kn);
      f32x16 s = scores(qf, kf);
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = fast_exp2(s[e] * sc - mm[e]) * rr[e];
      store_tile(s, kt * 32);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) kf[ks] = kn[ks];
    }
  } else {
    for (int kt = 0; kt < nkt; ++kt) {
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
      for (int h = 0; h < p.heads; ++h) {
        bf16x8 qf[KS], kf[KS];
        float mm[16], rr[16];
        load_q(h, qf);
        load_k(h, kt * 32, kf);
        row_stats(h, mm, rr);
        const f32x16 s = scores(qf, kf);
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] += fast_exp2(s[e] * sc - mm[e]) * rr[e];
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] *= p.inv_heads;
      store_tile(acc, kt * 32);
    }
  }
}

template <int DH, bool MEAN, bool BF16>
static hipError_t launch_probs(const AttnProbsK& k, int batch, hipStream_t s) {
  const int nqt = (k.q_rows + 31) / 32;
  const int hn = MEAN ? k.heads : 1;
  int nw = nqt < 4 ? nqt : 4;
  while (nw > 0 && (size_t)nw * hn * 32 * sizeof(float2) > 65536) --nw;  // (head_mean with more than 64 heads: fewer waves)
  if (nw == 0) return hipErrorInvalidValue;
  const int64_t grid = (int64_t)batch * (MEAN ? 1 : k.heads) * ((nqt + nw - 1) / nw);
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((attn_probs_kernel<DH, MEAN, BF16>), dim3((unsigned)grid), dim3(64 * nw), (size_t)nw * hn * 32 * sizeof(float2),
                     s, k);
  return hipGetLastError();
}

template <int DH>
static hipError_t launch_probs_dh(const AttnProbsK& k, int batch, int head_mean, int out_bf16, hipStream_t s) {
  if (head_mean) return out_bf16 ? launch_probs<DH, true, true>(k, batch, s) : launch_probs<DH, true, false>(k, batch, s);
  return out_bf16 ? launch_probs<DH, false, true>(k, batch, s) : launch_probs<DH, false, false>(k, batch, s);
}

hipError_t launch_attention_probs(const void* qkv, void* out, int batch, int seq, int heads, int head_dim, int q_rows,
                                  int head_mean, int out_bf16, hipStream_t s) {
  if (batch <= 0 || seq <= 0 || heads <= 0 || q_rows < 1 || q_rows > seq) return hipErrorInvalidValue;
  AttnProbsK k;
  k.qkv = (const bf16_t*)qkv;
  k.out = out;
  k.seq = seq;
  k.heads = heads;
  k.q_rows = q_rows;
  k.ld_qkv = (int64_t)3 * heads * head_dim;
  k.inv_heads = 1.0f / (float)heads;
  switch (head_dim) {
    case 32: return launch_probs_dh<32>(k, batch, head_mean, out_bf16, s);
    case 64: return launch_probs_dh<64>(k, batch, head_mean, out_bf16, s);
    case 96: return launch_probs_dh<96>(k, batch, head_mean, out_bf16, s);
    case 128: return launch_probs_dh<128>(k, batch, head_mean, out_bf16, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace vdr
