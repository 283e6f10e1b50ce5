// The tile core of the descriptor-analysis kernels (nn_cosine.hip, affinity.hip, local_corr.hip, pca.hip, kmeans.hip,
// mahalanobis.hip, upsample.hip): one 128 x 128 fp32 tile per workgroup
// of 4 waves, wave (wr, wc) = (wave >> 1, wave & 1) owning the 64 x 64 sub-tile at (64 wr, 64 wc) as 2 x 2
// mfma_f32_32x32x16_bf16 accumulators.  Every piece that fixes the BITS of a result -- the accumulator layout, the k order of
// the MFMA steps, the comparator folds, the ascending sums, the cosine row norm -- is written once here, and so are the two
// pipelines that feed the tile (staged_steps through registers, dma_steps by LDS-DMA); the kernels keep what is theirs
// (centring, hi/lo split, one-hot build, source rows, epilogues, masks, work layouts).
//   Accumulator layout: element e of acc[m][n] of lane (hh = lane >> 5, l31 = lane & 31) is tile row acc_row(wr, m, e, hh),
//   tile column acc_col(wc, n, l31): a lane holds ONE column of the B operand and 16 rows of the A operand.
//   Two LDS images of a staged operand step, by the index the product contracts over:
//   t128  [128 rows][64 bf16], contraction over the contiguous index (X Y^T): 128-B rows, 16-B chunk c of row r at slot
//         c ^ ((r >> 1) & 7) (the K image of attention_tile.h: conflict-free ds_read_b128 fragment reads).
//   tr    [64 rows][128 bf16], contraction over the ROW index (Z^T Z): 256-B rows, 16-B chunk c of row r at slot
//         c ^ (((r & 3) << 2) | ((r >> 2) & 3)), read with ds_read_b64_tr_b16: lane 4q + p of a 16-lane group addresses row q,
//         columns 4p .. 4p+3 of a 4-row x 16-column block and receives column (lane & 15) of the 4 rows.  A lane's 8 k-values are
//         rows 4hh .. 4hh+3 and 8 + 4hh .. 8 + 4hh+3 of the k-step -- the same permutation on both operands, so the MFMA sums
//         the right products.
#pragma once
#include "vdr_dev.h"

namespace vdr {

// ---- accumulators ---------------------------------------------------------------------------------
VDR_DEV int acc_row(int wr, int m, int e, int hh) { return wr * 64 + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh; }
VDR_DEV int acc_col(int wc, int n, int l31) { return wc * 64 + n * 32 + l31; }

VDR_DEV void acc_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.0f;
}

// the tile to part[row * ld + col]; BOUNDED: only rows < rows, columns < cols
template <bool BOUNDED>
VDR_DEV void acc_store(float* part, int64_t ld, int rows, int cols, int wr, int wc, int l31, int hh, const f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = acc_row(wr, m, e, hh), col = acc_col(wc, n, l31);
        if (!BOUNDED || (row < rows && col < cols)) part[row * ld + col] = acc[m][n][e];
      }
}

// ---- the t128 image ---------------------------------------------------------------------------------
constexpr int T128 = 128;               // tile side
constexpr int T128_OPER = T128 * 128;   // bytes of one staged operand tile

// byte offset of 16-byte chunk ch (0..7) of row `row` in a staged operand tile
VDR_DEV int t128_off(int row, int ch) { return 128 * row + 16 * (ch ^ ((row >> 1) & 7)); }

// MFMA k-steps KS0 .. KS1-1 (16 columns each) of the staged 64-column step: the A operand at sx, the B operand at sx + T128_OPER
template <int KS0, int KS1>
VDR_DEV void t128_mfma(const char* sx, int wr, int wc, int l31, int hh, f32x16 (&acc)[2][2]) {
  const int swz = (l31 >> 1) & 7;
#pragma unroll
  for (int ks = KS0; ks < KS1; ++ks) {
    const int off = ((2 * ks + hh) ^ swz) * 16;
    bf16x8 af[2], bf[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) af[m] = *reinterpret_cast<const bf16x8*>(sx + (wr * 64 + m * 32 + l31) * 128 + off);
#pragma unroll
    for (int n = 0; n < 2; ++n) bf[n] = *reinterpret_cast<const bf16x8*>(sx + T128_OPER + (wc * 64 + n * 32 + l31) * 128 + off);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[m], bf[n], acc[m][n], 0, 0, 0);
  }
}

// the four MFMA k-steps of a staged 64-column step with ONE A image against TWO B images accumulated into the same tile
// (kmeans.hip: X against the hi and the lo half of the centroids): per 16-column k-step the products with b0, then those with b1
VDR_DEV void t128_mfma_a2b(const char* sa, const char* sb0, const char* sb1, int wr, int wc, int l31, int hh, f32x16 (&acc)[2][2]) {
  const int swz = (l31 >> 1) & 7;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int off = ((2 * ks + hh) ^ swz) * 16;
    bf16x8 af[2], b0[2], b1[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) af[m] = *reinterpret_cast<const bf16x8*>(sa + (wr * 64 + m * 32 + l31) * 128 + off);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      b0[n] = *reinterpret_cast<const bf16x8*>(sb0 + (wc * 64 + n * 32 + l31) * 128 + off);
      b1[n] = *reinterpret_cast<const bf16x8*>(sb1 + (wc * 64 + n * 32 + l31) * 128 + off);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[m], b0[n], acc[m][n], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[m], b1[n], acc[m][n], 0, 0, 0);
  }
}

// the four MFMA k-steps of a staged 64-column step with TWO A images against TWO B images accumulated into the same tile
// (mahalanobis.hip: the hi and the lo half of the centred rows against those of the whitening rows): per 16-column k-step the
// products a0 b0, then a0 b1, then a1 b0; a1 b1 is not taken
VDR_DEV void t128_mfma_2a2b(const char* sa0, const char* sa1, const char* sb0, const char* sb1, int wr, int wc, int l31, int hh,
                            f32x16 (&acc)[2][2]) {
  const int swz = (l31 >> 1) & 7;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int off = ((2 * ks + hh) ^ swz) * 16;
    bf16x8 a0[2], a1[2], b0[2], b1[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      a0[m] = *reinterpret_cast<const bf16x8*>(sa0 + (wr * 64 + m * 32 + l31) * 128 + off);
      a1[m] = *reinterpret_cast<const bf16x8*>(sa1 + (wr * 64 + m * 32 + l31) * 128 + off);
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      b0[n] = *reinterpret_cast<const bf16x8*>(sb0 + (wc * 64 + n * 32 + l31) * 128 + off);
      b1[n] = *reinterpret_cast<const bf16x8*>(sb1 + (wc * 64 + n * 32 + l31) * 128 + off);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[m], b0[n], acc[m][n], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[m], b1[n], acc[m][n], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[m], b0[n], acc[m][n], 0, 0, 0);
  }
}

// ---- the tr image -----------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) bf16x4 tr_lds_bf16x4;
typedef const __attribute__((address_space(3))) char* tr_lds_cptr;

constexpr int TR_STEP = 64;             // rows staged per step
constexpr int TR_IMG = TR_STEP * 256;   // bytes of one staged tile

// byte offset of 16-byte chunk ch (0..15) of row `row` in a staged [rows][128 x bf16] tile
VDR_DEV int tr_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// the operand of one 16-row k-step for the 32 columns at cb: column cb + (lane & 31), rows 4hh..4hh+3 | 8+4hh..8+4hh+3
VDR_DEV bf16x8 tr_read(tr_lds_cptr img, int ks, int cb, int lane) {
  const int hh = lane >> 5, dg = (lane >> 4) & 1, tq = (lane & 15) >> 2, tp = lane & 3;
  const int row = ks * 16 + 4 * hh + tq;
  const int ch = (cb >> 3) + 2 * dg + (tp >> 1);
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((tr_lds_bf16x4*)(img + tr_off(row, ch) + 8 * (tp & 1)));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((tr_lds_bf16x4*)(img + tr_off(row + 8, ch) + 8 * (tp & 1)));
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = lo[j];
    f[4 + j] = hi[j];
  }
  return f;
}

// the four MFMA k-steps (16 rows each) of a staged 64-row step: acc += imgA^T imgB
VDR_DEV void tr_mfma(tr_lds_cptr imgA, tr_lds_cptr imgB, int wr, int wc, int lane, f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int ks = 0; ks < TR_STEP / 16; ++ks) {
    bf16x8 af[2], bf[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) af[m] = tr_read(imgA, ks, wr * 64 + m * 32, lane);
#pragma unroll
    for (int n = 0; n < 2; ++n) bf[n] = tr_read(imgB, ks, wc * 64 + n * 32, lane);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[m], bf[n], acc[m][n], 0, 0, 0);
  }
}

// the first NKS MFMA k-steps of a staged step with TWO A images against ONE B image accumulated into the same tile
// (upsample.hip: the hi and the lo half of the weights against the window's descriptors; its window fills NKS * 16 rows): per
// 16-row k-step the products with a0, then those with a1
template <int NKS>
VDR_DEV void tr_mfma_2a(tr_lds_cptr imgA0, tr_lds_cptr imgA1, tr_lds_cptr imgB, int wr, int wc, int lane, f32x16 (&acc)[2][2]) {
  static_assert(NKS >= 1 && NKS <= TR_STEP / 16, "k-steps of one staged step");
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    bf16x8 a0[2], a1[2], bf[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      a0[m] = tr_read(imgA0, ks, wr * 64 + m * 32, lane);
      a1[m] = tr_read(imgA1, ks, wr * 64 + m * 32, lane);
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) bf[n] = tr_read(imgB, ks, wc * 64 + n * 32, lane);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[m], bf[n], acc[m][n], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[m], bf[n], acc[m][n], 0, 0, 0);
  }
}

// ---- staging through registers ------------------------------------------------------------------------
// The pipeline of the kernels whose operands pass through registers on their way to LDS (a subtraction, a split or a one-hot
// build in between rules the LDS-DMA out): fetch(s) loads step s into registers, stage(s) writes the fetched step into the LDS
// image, mma() multiplies the image; the loads of step s + 1 are in flight under the MFMAs of step s.
template <class Fetch, class Stage, class Mma>
VDR_DEV void staged_steps(int nsteps, Fetch fetch, Stage stage, Mma mma) {
  fetch(0);
#pragma clang loop unroll(disable)
  for (int step = 0; step < nsteps; ++step) {
    __syncthreads();  // every wave has read the previous step
    stage(step);
    __syncthreads();
    if (step + 1 < nsteps) fetch(step + 1);
    mma();
  }
}

// 8 consecutive elements (16 bytes of bf16, two 16-byte halves of fp32) held raw between the fetch and the staging
template <bool BF16>
struct RawChunk;
template <>
struct RawChunk<true> {
  bf16x8 v;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16_t)0.0f;
  }
  __device__ __forceinline__ void load(const void* x, int64_t off) { v = *reinterpret_cast<const bf16x8*>((const bf16_t*)x + off); }
  __device__ __forceinline__ float get(int e) const { return (float)v[e]; }
};
template <>
struct RawChunk<false> {
  f32x4 lo, hi;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int e = 0; e < 4; ++e) lo[e] = hi[e] = 0.0f;
  }
  __device__ __forceinline__ void load(const void* x, int64_t off) {
    lo = *reinterpret_cast<const f32x4*>((const float*)x + off);
    hi = *reinterpret_cast<const f32x4*>((const float*)x + off + 4);
  }
  __device__ __forceinline__ float get(int e) const { return e < 4 ? lo[e] : hi[e - 4]; }
};
// the chunk at x + off when ok, zeros otherwise (every lane always has a value to stage: EXEC stays all ones in the MFMAs)
template <bool BF16>
VDR_DEV void raw_fill(RawChunk<BF16>& c, bool ok, const void* x, int64_t off) {
  if (ok) c.load(x, off);
  else c.zero();
}

// ---- staging by LDS-DMA: the cosine kernels ---------------------------------------------------------------
// nn_cosine.hip, knn.hip, affinity.hip and local_corr.hip multiply raw bf16 rows, so their operands go global -> LDS directly.
// All take dma_wait and t128_dma_chunk; local_corr_kernel and knn_kernel run on t128_dma_stage and dma_steps, nn_cosine_kernel and
// affinity_bits_kernel keep spelled-out copies of those two (1 - 3 % slower through them: DESIGN 4.6t) -- a change to either
// is a change to all three, and a new kernel starts from the helpers.
// the staged step has landed, for every wave: the DMAs are opaque to hipcc, so the wait is spelled out
VDR_DEV void dma_wait() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// One K step (64 channels from kk * 64) of both operands into the staging buffer at sx, the A image first: 4 + 4 DMA
// instructions per wave, 8 rows x 128 B each.  The DMA writes linearly, so the swizzle of the t128 image is applied to the
// per-lane SOURCE chunk.  A lane stages tile rows t128_dma_row(wave, lane, q), q = 0..3, of each operand; xo[q] / yo[q] are
// the element offsets of their source rows: always valid rows (the kernels clamp; what a clamped row contributes is dropped
// in their epilogues).  d % 64 == 32: the last step's unused chunks re-read chunks 0..3, nothing past the end of a row is touched.
VDR_DEV int t128_dma_row(int wave, int lane, int q) { return (wave * 4 + q) * 8 + (lane >> 3); }
// the 16-byte chunk of the source row's K step that this lane copies for tile row r: the swizzle, and in a short last step
// (d % 64 == 32) chunks 0..3 again
VDR_DEV int t128_dma_chunk(int lane, int r, bool shortk) {
  const int c = (lane & 7) ^ ((r >> 1) & 7);
  return shortk ? c & 3 : c;
}
VDR_DEV void t128_dma_stage(const bf16_t* xp, const bf16_t* yp, const int64_t (&xo)[4], const int64_t (&yo)[4], int d, int kk, char* sx,
                            int wave, int lane) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int col = kk * 64 + t128_dma_chunk(lane, t128_dma_row(wave, lane, q), d - kk * 64 < 64) * 8;
    glds16_raw(xp + xo[q] + col, sx + (wave * 4 + q) * 1024);
    glds16_raw(yp + yo[q] + col, sx + T128_OPER + (wave * 4 + q) * 1024);
  }
}

// One loop over the nk K steps of tiles jt0 .. jt1-1 through two staging buffers of 2 T128_OPER bytes at smem: step s + 1 is
// staged under the MFMAs of step s (pass s = -1 only stages step 0); the step after a tile's last one is the first of the next
// tile.  (jt, kk) is the step in the MFMAs, (njt, nkk) the one being staged; it goes into the other buffer, which every wave
// finished reading before the barrier that ended the previous pass.  stage(tile, k, buffer) issues the DMAs, epilogue(tile)
// consumes acc after the tile's last step (and zeroes it if another tile follows).
template <class Stage, class Epilogue>
VDR_DEV void dma_steps(int jt0, int jt1, int d, char* smem, int wr, int wc, int l31, int hh, f32x16 (&acc)[2][2], Stage stage,
                       Epilogue epilogue) {
  const int nk = (d + 63) >> 6;
  const int nsteps = (jt1 - jt0) * nk;
  int jt = jt0, kk = -1, buf = 1;
#pragma clang loop unroll(disable)
  for (int s = -1; s < nsteps; ++s) {
    int njt = jt, nkk = kk + 1;
    if (nkk == nk) {
      nkk = 0;
      ++njt;
    }
    if (s + 1 < nsteps) stage(njt, nkk, smem + (buf ^ 1) * 2 * T128_OPER);
    if (s >= 0) {
      const char* sx = smem + buf * 2 * T128_OPER;
      t128_mfma<0, 2>(sx, wr, wc, l31, hh, acc);
      if (d - kk * 64 >= 64) t128_mfma<2, 4>(sx, wr, wc, l31, hh, acc);
      if (kk + 1 == nk) epilogue(jt);
    }
    dma_wait();
    buf ^= 1;
    jt = njt;
    kk = nkk;
  }
}

// the launch-side check of one operand: t rows of d channels, d a multiple of 32 within the row, 16-byte aligned rows
inline bool cos_operand_ok(const void* x, int64_t ld, int64_t ps, int64_t t, int d) {
  return x && t > 0 && d > 0 && !(d & 31) && ld >= d && ps >= 0 && !((uintptr_t)x & 15) && !((ld | ps) & 7);
}

// The column tiles of a (problem, panel) cut into runs so that a launch has about COS_TARGET_ITEMS work items (two workgroups
// per CU): run `split` takes `base` tiles, the first `rem` runs one more.  Only decides which workgroup computes a tile.
constexpr int COS_TARGET_ITEMS = 512;
struct RunSplit {
  int nsplit, base, rem;
};
inline RunSplit run_split(int64_t items, int64_t ntiles) {
  int64_t n = COS_TARGET_ITEMS / items;
  n = n < 1 ? 1 : n > ntiles ? ntiles : n;
  return {(int)n, (int)(ntiles / n), (int)(ntiles % n)};
}
VDR_DEV void run_tiles(int split, int base, int rem, int& jt0, int& jt1) {
  jt0 = split * base + min(split, rem);
  jt1 = jt0 + base + (split < rem);
}

// ---- addressing -------------------------------------------------------------------------------------
// element offset of row r (0 .. R-1) of a problem that starts at element `base`: its images of a.t rows are a.is apart, rows a.ld
template <class Args>
VDR_DEV int64_t desc_row(const Args& a, int64_t base, int64_t r) {
  const int64_t q = r / a.t;
  return base + q * a.is + (r - q * a.t) * a.ld;
}

// pair (i <= j) number `pair` of the upper triangle of nt x nt tiles, row by row
VDR_DEV void tri_pair(int pair, int nt, int& i, int& j) {
  i = 0;
  while (pair >= nt - i) {
    pair -= nt - i;
    ++i;
  }
  j = i + pair;
}

// ---- reductions, each in ONE fixed order ----------------------------------------------------------------
// sum of squares of a row of d elements (d % 8 == 0): one wave per row, a lane sums its 16-byte chunks lane, lane + 64, ... in
// chunk order, then the xor butterfly
VDR_DEV float row_sumsq(const bf16_t* src, int d, int lane) {
  float ss = 0.0f;
  for (int c = lane * 8; c < d; c += 512) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = (float)v[e];
      ss += f * f;
    }
  }
  return wave_sum(ss);
}
VDR_DEV float row_sumsq(const float* src, int d, int lane) {
  float ss = 0.0f;
  for (int c = lane * 8; c < d; c += 512) {
    RawChunk<false> v;
    v.load(src, c);
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += v.get(e) * v.get(e);
  }
  return wave_sum(ss);
}

// rn(v) = 1 / max(sqrt(sum v^2), 1e-8) of the cosine kernels, IEEE sqrt and division: the one place it is written
VDR_DEV float cosine_rn(float ss) { return __fdiv_rn(1.0f, fmaxf(__fsqrt_rn(ss), 1e-8f)); }

// src[0] + src[stride] + ... + src[(n - 1) stride], ascending: the definition of every chunked sum's bits
VDR_DEV float fold_chunks(const float* src, int n, int64_t stride) {
  float sum = src[0];
  for (int q = 1; q < n; ++q) sum += src[q * stride];
  return sum;
}

// The sixteen row lanes of a (problem, chunk, 128-column) workgroup folded ascending: thread (rl = tid >> 4, ch = tid & 15)
// hands in the sums of its 8 columns; thread tid < 128 writes the sum of column tid to dst[tid] if that column is < cols
VDR_DEV void fold_row_lanes(float (&s)[16][128], int tid, const float (&acc)[8], int cols, float* dst) {
  const int ch = tid & 15, rl = tid >> 4;
#pragma unroll
  for (int e = 0; e < 8; ++e) s[rl][ch * 8 + e] = acc[e];
  __syncthreads();
  if (tid < 128 && tid < cols) {
    float sum = s[0][tid];
#pragma unroll
    for (int j = 1; j < 16; ++j) sum += s[j][tid];
    dst[tid] = sum;
  }
}

// fixed binary tree over the 256 threads of a workgroup through s[256]; every thread returns the total
template <class T, class Op>
VDR_DEV T block_reduce_256(T* s, int tid, T v, Op op) {
  s[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s[tid] = op(s[tid], s[tid + o]);
    __syncthreads();
  }
  return s[0];
}

// The per-lane running row best (value, index) of the accumulator layout reduced over the 32 lanes of a half wave (xor
// butterfly), then over the two column waves through s_rowv / s_rowi [2][128]; `better(v, i, bv, bi)` is a total order on pairs
// with distinct indices, so the grouping does not matter.  Returns the best of tile row tid for tid < 128.
struct RowBest {
  float v;
  int i;
};
// the comparison of the cosine matches (nn_cosine.hip, local_corr.hip): greater value, then lower index
struct NnBetter {
  __device__ __forceinline__ bool operator()(float v, int i, float bv, int bi) const { return v > bv || (v == bv && i < bi); }
};
constexpr NnBetter nn_better;
template <class Better>
VDR_DEV RowBest row_best_reduce(const float (&rbv)[2][16], const int (&rbi)[2][16], float* s_rowv, int* s_rowi, int tid, Better better) {
  const int wave = tid >> 6, wr = wave >> 1, wc = wave & 1, l31 = tid & 31, hh = (tid >> 5) & 1;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float v = rbv[m][e];
      int i = rbi[m][e];
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (better(ov, oi, v, i)) {
          v = ov;
          i = oi;
        }
      }
      if (l31 == 0) {
        s_rowv[wc * 128 + acc_row(wr, m, e, hh)] = v;
        s_rowi[wc * 128 + acc_row(wr, m, e, hh)] = i;
      }
    }
  __syncthreads();
  RowBest b = {0.0f, 0};
  if (tid < 128) {
    b.v = s_rowv[tid];
    b.i = s_rowi[tid];
    if (better(s_rowv[128 + tid], s_rowi[128 + tid], b.v, b.i)) {
      b.v = s_rowv[128 + tid];
      b.i = s_rowi[128 + tid];
    }
  }
  return b;
}

}  // namespace vdr
