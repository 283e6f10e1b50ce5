// The tile core of the fused attention kernels (attention.hip, attention_relpos.hip, attention_hd.hip): the pieces that
// every kernel with the S^T = K.Q^T / O^T = V^T.P^T data flow runs unchanged.  Each piece is written once here; what
// differs between the kernels (tile count, head-dim blocks, strides, the clamp row, the initial accumulator, the exp2
// offset) arrives as data or as a template shape, never as a flag that names the caller.  The loops over chunks, tiles
// and slices, the logit bias and the masks stay in the kernels.
#pragma once
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef const __attribute__((address_space(3))) char* lds_cptr;

// dh^-1/2 * log2(e): the exp2 scale of the raw q.k scores.  One spelling for every kernel (the attention maps of
// attention_probs.hip restate the fused kernels' arithmetic and take the same constant).
template <int DH>
constexpr float attn_scale_log2e() {
  return DH == 64 ? 0.125f * 1.44269504088896341f
                  : DH == 32 ? 0.17677669529663688f * 1.44269504088896341f
                             : DH == 96 ? 0.10206207261596575f * 1.44269504088896341f : 0.08838834764831845f * 1.44269504088896341f;
}

// Lane constants of the head-dim-64 LDS images ([key][64] bf16 rows of 128 B).
//   K: 16-B chunk ^ ((key >> 1) & 7)            (ds_read_b128 row reads of the 32x32x16 operand)
//   V: 16-B chunk ^ (((key >> 1) & 1) << 2)     (ds_read_b64_tr_b16 blocks of 4 keys x 16 d: the two even / odd keys
//                                                of a block land in different halves of their 32 banks)
// Transposed V read: lane 4q+p of a 16-lane group addresses key row q, d columns 4p..4p+3 of a 4 x 16 block and
// receives d column (lane & 15) of the 4 keys (groups: d half (lane >> 4) & 1, key offset 4 hh).
struct AttnLane {
  int hh, l31;  // half of the wave (keys / dims + 4), row of the 32-row tile
  int swz;      // K chunk swizzle of row l31
  int vrow;     // byte offset of this lane's transposed read inside a V image; + 16-key slices (multiples of 8 keep (key >> 1) & 1)
  int vch[2];   // ... plus the swizzled 16-B chunk of 32-dim block nd
};
VDR_DEV AttnLane attn_lane(int lane) {
  AttnLane ln;
  ln.hh = lane >> 5;
  ln.l31 = lane & 31;
  ln.swz = (lane >> 1) & 7;
  const int tq = (lane & 15) >> 2, tp = lane & 3, dg = (lane >> 4) & 1;
  const int vkey = 4 * ln.hh + tq;
  ln.vrow = vkey * 128 + 8 * (tp & 1);
#pragma unroll
  for (int nd = 0; nd < 2; ++nd) ln.vch[nd] = ((4 * nd + 2 * dg + (tp >> 1)) ^ (((vkey >> 1) & 1) << 2)) * 16;
  return ln;
}

// Workgroup -> (batch entry b, head hd, query block yb) of a 1-D grid of (image, head) x nyb query blocks, query block
// fastest, walked in XCD-contiguous order: the query blocks of one (image, head) run next to each other on ONE XCD and
// find its K / V in that L2.  (As a 2-D grid with the query block on y they were a whole grid row apart: every block
// re-read K / V from HBM -- ViT-L/14@336, 5 query blocks per head: 0.83 GB per launch at 5.2 TB/s; the 32 query blocks
// of one global-attention head of MedSAM: 6.4 GB per launch at B = 16.)
struct AttnItem {
  int b, hd, yb;
};
VDR_DEV AttnItem attn_item(int nyb, int heads) {
  const int vid = nyb > 1 ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
  const int bh = vid / nyb;
  AttnItem it;
  it.yb = vid - bh * nyb;
  it.b = bh / heads;
  it.hd = bh - it.b * heads;
  return it;
}

template <int N>
VDR_DEV void zero_tiles(f32x16 (&a)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int e = 0; e < 16; ++e) a[n][e] = 0.0f;
}

// Q fragments of one query row (B operand of S^T = K.Q^T): lane (query l31, hh) holds dims 16 ks + 8 hh .. +7, KS x 16 B
// straight from global.  `src` = the (clamped) row's head + hh * 8.
template <int KS>
VDR_DEV void load_q_frags(const bf16_t* src, bf16x8 (&qf)[KS]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(src + ks * 16);
}

// Staging of one chunk of NT*32 keys (head dim 64) by a 4-wave workgroup: K and V rows straight into LDS, 8 rows per
// wave-instruction, swizzled as AttnLane reads them.  V stays row-major: the transposed read hands every lane
// V[key0 .. key0+3][d] -- the P.V operand -- so there is no register-staged transpose.  The LDS-DMA is an opaque
// instruction (glds16_raw): hipcc orders nothing after it, the explicit vmcnt(0) + barrier of stage_wait does.
// Rows past `last` (the last valid key: length - 1) repeat it: a 16-key slice that straddles the length still runs its
// P.V MFMA, where a masked key's P = 0 times a NaN / Inf padding row would give NaN (0 x finite = 0).
template <int NT>
VDR_DEV void stage_kv_chunk(const bf16_t* kb, const bf16_t* vb, int64_t ld, int kc0, int last, char* sK, char* sV, int wave,
                            int lane) {
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int piece = wave * NT + q;  // 0 .. 4*NT-1, rows piece*8 .. +7
    const int r = piece * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    int key = kc0 + r;
    key = key < last ? key : last;
    glds16_raw(kb + (int64_t)key * ld + c * 8, sK + piece * 1024);
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int piece = wave * NT + q;
    const int r = piece * 8 + (lane >> 3);
    const int c = (lane & 7) ^ (((r >> 1) & 1) << 2);
    int key = kc0 + r;
    key = key < last ? key : last;
    glds16_raw(vb + (int64_t)key * ld + c * 8, sV + piece * 1024);
  }
}
VDR_DEV void stage_wait() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// S^T = K . Q^T of NT 32-key tiles against the staged K image; s[] comes in holding each tile's initial accumulator and
// goes out holding its scores.  Wave priority follows the phase: low while the wave streams these MFMAs, high for the
// vector-heavy softmax / P.V that follows (measured in attn_persist_kernel).
template <int NT>
VDR_DEV void qk_tiles(const char* sK, const AttnLane& ln, const bf16x8 (&qf)[4], f32x16 (&s)[NT]) {
  __builtin_amdgcn_s_setprio(0);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 kf =
          *reinterpret_cast<const bf16x8*>(sK + (t * 32 + ln.l31) * 128 + (((2 * ks + ln.hh) ^ ln.swz) * 16));
      s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[t], 0, 0, 0);
    }
  }
  __builtin_amdgcn_s_setprio(2);
}

// Online softmax: the running row sum and output move from the old maximum to the new one.  `sc` = exp2 scale of the scores.
template <int ND>
VDR_DEV void online_rescale(float m_run, float m_new, float sc, float& l_run, f32x16 (&o)[ND]) {
  const float alpha = fast_exp2((m_run - m_new) * sc);
  l_run *= alpha;
#pragma unroll
  for (int nd = 0; nd < ND; ++nd)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[nd][e] *= alpha;
}

// One 16-key slice (s2 = 0 / 1) of score tile st: P = 2^(st * sc + off) rounded to bf16 in the accumulator layout, its
// row sum into lsum2 (fp32, (even, odd) elements: every kernel sums in this order, so their outputs stay bitwise
// equal), then O^T += V^T . P^T over ND 32-dim blocks: per block two transposed 8-key reads, joined in the permuted
// key order the accumulator registers (and so P) hold.  `v` = this lane's transposed-read address at the slice's first
// key row, vstride the V row stride, vcol[nd] the byte column of block nd.  The sched_barrier keeps the exp / convert
// of later slices from being hoisted over this one (VGPR cap).
template <int ND>
VDR_DEV void pv_slice(const f32x16& st, int s2, float sc, float off, f32x2& lsum2, lds_cptr v, int vstride,
                      const int (&vcol)[ND], f32x16 (&o)[ND]) {
  bf16x8 pf;
  softmax_slice8(st, s2, sc, off, lsum2, pf);
#pragma unroll
  for (int nd = 0; nd < ND; ++nd) {
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(v + vcol[nd]));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(v + 8 * vstride + vcol[nd]));
    bf16x8 vf;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      vf[j] = lo[j];
      vf[4 + j] = hi[j];
    }
    o[nd] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[nd], 0, 0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// End of a row: the sum lives in the lane pair (lane, lane ^ 32); returns 1 / l.
VDR_DEV float finish_row(float l_run) {
  const float l = l_run + __shfl_xor(l_run, 32, 64);
  return 1.0f / l;
}

// Host: launch of a 256-thread kernel on the 1-D grid that attn_item decodes (batch x heads x query blocks of
// qt_per_block tiles) with `lds` bytes of dynamic LDS.  The kernel's opt-in limit is raised to lds_limit (>= lds: a
// kernel whose request varies passes its largest) once per instantiation and device, not per launch.
template <auto FN, class K>
static hipError_t launch_query_blocks(size_t lds, size_t lds_limit, const K& k, int batch, hipStream_t s) {
  static KernelState st;
  const int dev = current_device_index();
  if (dev < 0) return hipErrorInvalidDevice;
  if (hipError_t e = raise_lds_limit(st, (const void*)FN, dev, lds_limit)) return e;
  const int nqt = (k.seq + 31) / 32;
  const dim3 grid((unsigned)(batch * k.heads * ((nqt + k.qt_per_block - 1) / k.qt_per_block)));
  hipLaunchKernelGGL(FN, grid, dim3(256), lds, s, k);
  return hipGetLastError();
}

}  // namespace vdr
