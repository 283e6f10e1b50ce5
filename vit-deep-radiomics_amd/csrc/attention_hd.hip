// Fused multi-head self-attention for gfx950 at head dims 32, 96 and 128:  out = softmax(q k^T dh^-1/2) v per
// (sequence, head).  Head dim 64 stays on attention.hip (the dispatcher, launch_attention, sends only dh != 64 here).
//
// Needed by the drop-ins whenever num_heads does not give 64 columns per head: the reference's classifiers and
// CrossAttentionLayer (src/models_archs.py) accept any num_heads that divides input_dim -- DINOv2-small features
// (D = 384) at the configured 4 heads are dh = 96, the 256-wide MedSAM features at 8 / 2 heads dh = 32 / 128.
//
// One workgroup (4 waves) per (sequence, head, block of 128 queries); wave w owns query tile w (32 queries) of the
// block.  The keys run in chunks of KC (128 at dh 32, 64 otherwise) with an online softmax; every chunk is staged by
// the whole workgroup through registers into LDS (the next chunk's global loads are issued before the current chunk is
// computed, so they land under its MFMAs):
//   K  [KC][dh] bf16, rows padded by 16 B (stride = 16 B x odd): the ds_read_b128 row reads of S^T = K.Q^T hit 16
//      distinct 16-byte bank slots per lane group
//   V  [KC][dh] bf16 row-major, row stride = 64 or 192 mod 256 B (dh 32: 64, 96: 192, 128: 320): the 4 rows x 64 B
//      that one 32-lane half reads with ds_read_b64_tr_b16 cover the 64 banks once
// Per 32-key tile (MFMA 32x32x16 bf16, key on the accumulator row, query on the lane, as in attention.hip)
//     S^T = K . Q^T,   P = exp2(S * dh^-1/2 log2 e - m), rounded to bf16 in the accumulator registers,
//     O^T += V^T . P^T (the V fragment read transposed in the key order the accumulator registers hold)
// so a softmax row lives in one lane pair (lane, lane ^ 32) and P never touches LDS.
//
// Per-sequence lengths (lens[b] + len_add, sequences padded to seq): keys past the length are masked to -inf, chunks
// and 16-key slices that lie wholly past it are skipped (wave-uniform), so a valid row's bits depend neither on the
// padding rows' contents nor on how far the sequence is padded.  Nothing depends on batch * heads: the grid grows,
// the arithmetic of a (sequence, head) does not.
#include "attention_tile.h"

namespace vdr {

struct AttnHdK {
  const bf16_t* qkv;
  bf16_t* out;
  int seq, heads;
  int64_t ld_qkv, ld_out;
  const int* lens;  // non-null: valid length of batch entry b = min(seq, lens[b] + len_add)
  int len_add;
};

template <int DH>
struct HdShape {
  static constexpr int KC = DH == 32 ? 128 : 64;        // keys per chunk
  static constexpr int NT = KC / 32;                    // 32-key tiles per chunk
  static constexpr int KS = DH / 16;                    // 16-deep k steps of S^T = K.Q^T
  static constexpr int ND = DH / 32;                    // 32-dim blocks of O^T
  static constexpr int CPR = DH / 8;                    // 16-byte pieces per row
  static constexpr int PPT = KC * CPR / 256;            // pieces per thread and operand (K or V) per chunk
  static constexpr int KSTR = 2 * DH + 16;              // K row stride (bytes)
  static constexpr int VSTR = DH == 128 ? 320 : 2 * DH; // V row stride (bytes), 64 or 192 mod 256
  static constexpr int LDS = KC * (KSTR + VSTR);
  static_assert(KC * CPR % 256 == 0, "every thread stages the same number of pieces");
  static_assert((KSTR / 16) % 2 == 1 && (VSTR % 256 == 64 || VSTR % 256 == 192), "bank layout");
};

// one 32-dim block of an output row: lane (query, hh) holds dims 8g + 4hh + e (e = 0..3) of the block, its partner lane
// (xor 32) the other 4 of every 8.  One v_permlane32_swap per dword gives each lane 16 contiguous bytes (store_row64_bf16's
// exchange, per block).  Every lane executes it; `ok` gates the stores only.
VDR_DEV void attn_hd_store_block(bf16_t* dst, const f32x16& o, float inv, int hh, bool ok) {
#pragma unroll
  for (int gp = 0; gp < 2; ++gp) {
    uint32_t a[2], b[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      bf16x2 va, vb;
      va[0] = (bf16_t)(o[8 * gp + 2 * d] * inv);
      va[1] = (bf16_t)(o[8 * gp + 2 * d + 1] * inv);
      vb[0] = (bf16_t)(o[8 * gp + 4 + 2 * d] * inv);
      vb[1] = (bf16_t)(o[8 * gp + 4 + 2 * d + 1] * inv);
      const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, va), __builtin_bit_cast(uint32_t, vb), false, false);
      a[d] = r[0];
      b[d] = r[1];
    }
    u32x4 v;
    v[0] = a[0];
    v[1] = a[1];
    v[2] = b[0];
    v[3] = b[1];
    if (ok) *reinterpret_cast<u32x4*>(dst + 8 * (2 * gp + hh)) = v;
  }
}

template <int DH>
__global__ __launch_bounds__(256, 2) void attn_hd_kernel(AttnHdK p) {
  using S = HdShape<DH>;
  constexpr int KC = S::KC, NT = S::NT, KS = S::KS, ND = S::ND, CPR = S::CPR, PPT = S::PPT;
  constexpr int KSTR = S::KSTR, VSTR = S::VSTR;
  __shared__ __attribute__((aligned(16))) char smem[S::LDS];
  char* sK = smem;
  char* sV = smem + KC * KSTR;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5;
  const int l31 = lane & 31;

  // grid: (sequence, head) x blocks of 4 query tiles
  const int nqt = (p.seq + 31) >> 5;
  const AttnItem it = attn_item((nqt + 3) >> 2, p.heads);
  const int b = it.b, hd = it.hd;
  const int HD = p.heads * DH;
  const bf16_t* qb = p.qkv + (int64_t)b * p.seq * p.ld_qkv + hd * DH;
  const bf16_t* kb = qb + HD;
  const bf16_t* vb = qb + 2 * HD;
  const int len = p.lens ? min(p.seq, p.lens[b] + p.len_add) : p.seq;
  const int n_chunks = (len + KC - 1) / KC;  // chunks wholly past the length are never staged
  const int qt = it.yb * 4 + wave;
  const bool active = qt < nqt;  // wave-uniform
  constexpr float sc = attn_scale_log2e<DH>();

  // staging: thread tid moves pieces tid + 256 i (row = piece / CPR, 16-byte column = piece % CPR) of K and of V;
  // rows past the valid length repeat its last row (the padding rule of stage_kv_chunk)
  bf16x8 rk[PPT], rv[PPT];
  const int last = max(len, 1) - 1;
  auto stage_load = [&](int kc0) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int piece = tid + 256 * i;
      const int r = piece / CPR, c = piece - (piece / CPR) * CPR;
      const int key = min(kc0 + r, last);
      rk[i] = *reinterpret_cast<const bf16x8*>(kb + (int64_t)key * p.ld_qkv + c * 8);
      rv[i] = *reinterpret_cast<const bf16x8*>(vb + (int64_t)key * p.ld_qkv + c * 8);
    }
  };
  auto stage_store = [&]() {
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int piece = tid + 256 * i;
      const int r = piece / CPR, c = piece - (piece / CPR) * CPR;
      *reinterpret_cast<bf16x8*>(sK + r * KSTR + c * 16) = rk[i];
      *reinterpret_cast<bf16x8*>(sV + r * VSTR + c * 16) = rv[i];
    }
  };

  bf16x8 qf[KS];
  load_q_frags(qb + (int64_t)min(qt * 32 + l31, p.seq - 1) * p.ld_qkv + hh * 8, qf);
  f32x16 o[ND];
  zero_tiles(o);
  float m_run = -INFINITY, l_run = 0.0f;

  // transposed V read with AttnLane's lane roles, on this file's padded, unswizzled V image
  const int tq = (lane & 15) >> 2, tp = lane & 3, dg = (lane >> 4) & 1;
  const lds_cptr sVr = (lds_cptr)sV + (4 * hh + tq) * VSTR + (16 * dg + 4 * tp) * 2;
  int vcol[ND];  // byte column of 32-dim block nd
#pragma unroll
  for (int nd = 0; nd < ND; ++nd) vcol[nd] = nd * 64;
  const char* sKr = sK + l31 * KSTR + hh * 16;

  auto process = [&](int kc0, bool rescale) {
    f32x16 s[NT];
    zero_tiles(s);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sKr + t * 32 * KSTR + ks * 32);
        s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (kc0 + t * 32 + 32 > len) mask_keys(s[t], kc0 + t * 32, hh, len);
    float mx = row_max_tiles<NT>(s);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    if (rescale) online_rescale(m_run, m_new, sc, l_run, o);
    m_run = m_new;
    const float mb = m_new * sc;
    f32x2 lsum2 = {0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        if (kc0 + t * 32 + s2 * 16 >= len) continue;  // wholly masked slice (wave-uniform): P = 0
        pv_slice(s[t], s2, sc, -mb, lsum2, sVr + (t * 32 + s2 * 16) * VSTR, VSTR, vcol, o);
      }
    }
    l_run += lsum2[0] + lsum2[1];
  };

  stage_load(0);
  for (int c = 0; c < n_chunks; ++c) {
    if (c) __syncthreads();  // every wave is done reading the previous chunk
    stage_store();
    __syncthreads();
    if (c + 1 < n_chunks) stage_load((c + 1) * KC);  // lands under this chunk's compute
    if (active) process(c * KC, c > 0);
  }
  if (!active) return;
  const float inv = finish_row(l_run);
  const int q = qt * 32 + l31;
  bf16_t* dst = p.out + ((int64_t)b * p.seq + (q < p.seq ? q : 0)) * p.ld_out + hd * DH;
#pragma unroll
  for (int nd = 0; nd < ND; ++nd) attn_hd_store_block(dst + nd * 32, o[nd], inv, hh, q < p.seq);
}

template <int DH>
static hipError_t launch_hd(const AttnHdK& k, int batch, hipStream_t s) {
  const int nqt = (k.seq + 31) / 32;
  const int64_t grid = (int64_t)batch * k.heads * ((nqt + 3) / 4);
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_hd_kernel<DH>, dim3((unsigned)grid), dim3(256), 0, s, k);
  return hipGetLastError();
}

hipError_t launch_attention_hd(const void* qkv, void* out, int batch, int seq, int heads, int head_dim, hipStream_t s,
                               const int* lens, int len_add) {
  if (batch <= 0 || seq <= 0 || heads <= 0) return hipErrorInvalidValue;
  AttnHdK k;
  k.qkv = (const bf16_t*)qkv;
  k.out = (bf16_t*)out;
  k.seq = seq;
  k.heads = heads;
  k.ld_qkv = (int64_t)3 * heads * head_dim;
  k.ld_out = (int64_t)heads * head_dim;
  k.lens = lens;
  k.len_add = len_add;
  switch (head_dim) {
    case 32: return launch_hd<32>(k, batch, s);
    case 96: return launch_hd<96>(k, batch, s);
    case 128: return launch_hd<128>(k, batch, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace vdr
