// PCA of dense descriptor maps for gfx950 (include/vdr.h: vdr_op_col_mean, vdr_op_covariance, vdr_op_pca_project).
// Operand of all three: `problems` problems of `imgs` images of t rows of d channels (bf16 or fp32), rows ld elements
// apart, images image_stride apart, image q of problem p = image p * imgs + q; R = imgs * t rows per problem.
//
//   col_mean     pca_mean_kernel: one workgroup = (problem, 1024-row chunk, 128 columns); thread (row lane tid >> 4, 16-byte
//                column chunk tid & 15) sums rows row lane, + 16, + 32 ... of the chunk, the 16 row lanes are folded ascending
//                through LDS.  pca_mean_finish_kernel folds the chunk sums ascending and divides once.
//   covariance   pca_cov_kernel: 256 threads, one work item = (problem, pair ci <= cj of 128-column tiles, 1024-row chunk).
//                The centring (fp32 subtraction, ONE rounding to bf16) rules out the LDS-DMA: every thread owns one fixed
//                16-byte column chunk of each tile, keeps its 8 + 8 means in registers, loads the next 64-row step into
//                registers under the MFMAs of the current one, and writes the centred bf16 values into the row-contracting
//                "tr" image of desc_tile.h (tile, accumulator layout, pipeline and transposed read: there).  Rows past the
//                chunk / R and columns past d are staged as zeros.  The item's 128 x 128 partial goes to `work`;
//                pca_cov_finish_kernel folds the chunks ascending, divides once, and writes (c1, c2) and (c2, c1) from the
//                same value; of a diagonal tile only c1 <= c2 is read.
//   pca_project  pca_project_kernel: components and mean in LDS, one wave per row (16 rows per wave): a lane multiplies its
//                16-byte chunks lane, lane + 64, ... in chunk order into k fp32 sums, then the xor butterfly.  The
//                workgroup's min / max go to `work`; pca_minmax_kernel folds them per problem (min and max are exact in any
//                order), pca_scale_kernel rescales in place when asked.
//   gram         (vdr_op_gram, the t x t side for t < d)  pca_gram_kernel: one work item = (problem, pair ti <= tj of
//                128-ROW tiles, chunk of VDR_GRAM_CHUNK columns).  The product contracts over the contiguous index, so the
//                tile is nn_cosine.hip's "t128" image of desc_tile.h, staged through registers like the covariance:
//                a thread owns 16-byte chunk tid & 7 of rows (tid >> 3) + 32 j of each tile and the 8 means of its columns.
//                The partial goes to `work` in the covariance's layout and pca_cov_finish_kernel folds it (matrix side t,
//                divisor t - 1).  The mean at any d is pca_mean_kernel's (launch_col_mean_any: the same launches, the same bits).
//   back_project (vdr_op_pca_back_project)  pca_back_kernel: pca_mean_kernel's workgroup and fold with k weighted sums per
//                column; pca_back_finish_kernel folds the
//                chunks ascending and normalises each component with a float64 norm.
// No atomics anywhere; nothing depends on `problems`, on the grid or on a launch heuristic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "desc_tile.h"
#include "vdr_dev.h"
#include "vdr_kernels.h"
#include "../../include/vdr.h"

namespace vdr {
namespace {

constexpr int PCA_CHUNK = VDR_COV_CHUNK;    // rows per chunk: a constant of the definition
constexpr int PCA_T = 128;                  // columns of a tile
constexpr int PCA_STEP = TR_STEP;           // rows staged per step (tile_tr.h)
constexpr int PCA_IMG = TR_IMG;             // bytes of one staged tile
constexpr int PCA_PROJ_ROWS = 64;           // rows of one projection workgroup
static_assert(PCA_CHUNK % PCA_STEP == 0, "a chunk is whole steps");

struct PcaArgs {
  const void* x;
  int64_t ld, is, R;
  int imgs, t, d, in_bf16;
  int nt, npairs, nchunks;
  const float* mean;
  float* part;  // scratch
};

// first element of problem p: the problems lie one after another
VDR_DEV int64_t pca_base(const PcaArgs& a, int p) { return (int64_t)p * a.imgs * a.is; }

VDR_DEV void pca_load8(const PcaArgs& a, int64_t off, float (&v)[8]) {
  if (a.in_bf16) {
    const bf16x8 b = *reinterpret_cast<const bf16x8*>((const bf16_t*)a.x + off);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)b[e];
  } else {
    const f32x4 lo = *reinterpret_cast<const f32x4*>((const float*)a.x + off);
    const f32x4 hi = *reinterpret_cast<const f32x4*>((const float*)a.x + off + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = lo[e];
      v[4 + e] = hi[e];
    }
  }
}

// ---- column mean ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pca_mean_kernel(PcaArgs a) {
  __shared__ float s[16][PCA_T];
  const int ncg = a.nt;
  int id = blockIdx.x;
  const int cg = id % ncg;
  id /= ncg;
  const int chunk = id % a.nchunks, p = id / a.nchunks;
  const int ch = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = cg * PCA_T + ch * 8;
  const int64_t r0 = (int64_t)chunk * PCA_CHUNK;
  const int64_t r1 = r0 + PCA_CHUNK < a.R ? r0 + PCA_CHUNK : a.R;
  float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (col < a.d)
    for (int64_t r = r0 + rl; r < r1; r += 16) {
      float v[8];
      pca_load8(a, desc_row(a, pca_base(a, p), r) + col, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
  fold_row_lanes(s, threadIdx.x, acc, a.d - cg * PCA_T, a.part + ((int64_t)p * a.nchunks + chunk) * a.d + cg * PCA_T);
}

__global__ __launch_bounds__(256) void pca_mean_finish_kernel(PcaArgs a, int problems, float* mean) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)problems * a.d) return;
  const int64_t p = idx / a.d;
  const int c = (int)(idx - p * a.d);
  mean[idx] = __fdiv_rn(fold_chunks(a.part + p * a.nchunks * a.d + c, a.nchunks, a.d), (float)a.R);
}

// ---- covariance -------------------------------------------------------------------------------------
// This kernel spells the pieces of desc_tile.h out (pair decode, row addressing, zero-or-load, zeroing, pipeline, transposed-read
// MFMA step, partial store) and takes only the raw chunk type from it: on the shared pieces it measured 0.2 - 0.6 us (up to 1.2 %)
// slower than its parent on the bf16 workloads, outside the A/A spread; the pipeline helper alone costs three more waits per pass.
// As written its assembly is the parent's, line for line (profiles/descriptor_tile_refactor_ab.txt).
template <bool BF16>
__global__ __launch_bounds__(256) void pca_cov_kernel(PcaArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  int id = blockIdx.x;
  const int chunk = id % a.nchunks;
  id /= a.nchunks;
  const int pair = id % a.npairs, p = id / a.npairs;
  int ci = 0, rem = pair;
  while (rem >= a.nt - ci) {
    rem -= a.nt - ci;
    ++ci;
  }
  const int cj = ci + rem;
  const bool diag = ci == cj;

  // staging role: one 16-byte column chunk of each tile, rows rl, rl + 16, rl + 32, rl + 48 of a step
  const int ch = tid & 15, rl = tid >> 4;
  const int col[2] = {ci * PCA_T + ch * 8, cj * PCA_T + ch * 8};
  const bool cok[2] = {col[0] < a.d, !diag && col[1] < a.d};
  float mu[2][8];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) mu[s][e] = cok[s] ? a.mean[(int64_t)p * a.d + col[s] + e] : 0.0f;

  const int64_t r0 = (int64_t)chunk * PCA_CHUNK;
  const int64_t r1 = r0 + PCA_CHUNK < a.R ? r0 + PCA_CHUNK : a.R;
  const int nsteps = (int)((r1 - r0 + PCA_STEP - 1) / PCA_STEP);

  RawChunk<BF16> raw[2][4];
  const auto fetch = [&](int step) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t r = r0 + step * PCA_STEP + rl + 16 * j;
      const int64_t q = r / a.t;
      const int64_t off = r < r1 ? ((int64_t)p * a.imgs + q) * a.is + (r - q * a.t) * a.ld : 0;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (r < r1 && cok[s]) raw[s][j].load(a.x, off + col[s]);
        else raw[s][j].zero();
      }
    }
  };
  const auto stage = [&](int step) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool rok = r0 + step * PCA_STEP + rl + 16 * j < r1;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s == 1 && diag) continue;
        bf16x8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (bf16_t)(rok && cok[s] ? raw[s][j].get(e) - mu[s][e] : 0.0f);
        *reinterpret_cast<bf16x8*>(smem + s * PCA_IMG + tr_off(rl + 16 * j, ch)) = z;
      }
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.0f;

  const tr_lds_cptr imgA = (tr_lds_cptr)smem;
  const tr_lds_cptr imgB = imgA + (diag ? 0 : PCA_IMG);
  fetch(0);
#pragma clang loop unroll(disable)
  for (int step = 0; step < nsteps; ++step) {
    __syncthreads();  // every wave has read the previous step
    stage(step);
    __syncthreads();
    if (step + 1 < nsteps) fetch(step + 1);
#pragma unroll
    for (int ks = 0; ks < PCA_STEP / 16; ++ks) {
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

  float* part = a.part + (((int64_t)p * a.npairs + pair) * a.nchunks + chunk) * (PCA_T * PCA_T);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wr * 64 + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        part[row * PCA_T + wc * 64 + n * 32 + l31] = acc[m][n][e];
      }
}

__global__ __launch_bounds__(256) void pca_cov_finish_kernel(PcaArgs a, float* cov) {
  constexpr int BLOCKS = PCA_T * PCA_T / 256;
  int id = blockIdx.x;
  const int idx = (id % BLOCKS) * 256 + threadIdx.x;
  id /= BLOCKS;
  const int pair = id % a.npairs, p = id / a.npairs;
  int ci, cj;
  tri_pair(pair, a.nt, ci, cj);
  const int i = idx >> 7, j = idx & 127;
  const int gi = ci * PCA_T + i, gj = cj * PCA_T + j;
  if (gi >= a.d || gj >= a.d || (ci == cj && i > j)) return;
  const float* src = a.part + ((int64_t)p * a.npairs + pair) * a.nchunks * (PCA_T * PCA_T) + idx;
  const float v = __fdiv_rn(fold_chunks(src, a.nchunks, PCA_T * PCA_T), (float)(a.R - 1));
  float* c = cov + (int64_t)p * a.d * a.d;
  c[(int64_t)gi * a.d + gj] = v;
  c[(int64_t)gj * a.d + gi] = v;
}

// ---- Gram (t x t) -----------------------------------------------------------------------------------
constexpr int GRAM_CHUNK = VDR_GRAM_CHUNK;  // columns per chunk: a constant of the definition
constexpr int GRAM_STEP = 64;               // columns staged per step
static_assert(GRAM_CHUNK % GRAM_STEP == 0, "a chunk is whole steps");

// a.nt / a.npairs: 128-row tiles over t and their pairs; a.nchunks: column chunks over d
template <bool BF16>
__global__ __launch_bounds__(256) void pca_gram_kernel(PcaArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  int id = blockIdx.x;
  const int chunk = id % a.nchunks;
  id /= a.nchunks;
  const int pair = id % a.npairs, p = id / a.npairs;
  int ti, tj;
  tri_pair(pair, a.nt, ti, tj);
  const bool diag = ti == tj;

  // staging role: 16-byte chunk ch of the 64-column step, rows rl, rl + 32, rl + 64, rl + 96 of each tile
  const int ch = tid & 7, rl = tid >> 3;
  const int c0 = chunk * GRAM_CHUNK;
  const int c1 = c0 + GRAM_CHUNK < a.d ? c0 + GRAM_CHUNK : a.d;
  const int nsteps = (c1 - c0 + GRAM_STEP - 1) / GRAM_STEP;
  bool rok[2][4];
  int64_t roff[2][4];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = (s ? tj : ti) * T128 + rl + 32 * j;
      rok[s][j] = r < a.t && !(s == 1 && diag);
      roff[s][j] = rok[s][j] ? desc_row(a, pca_base(a, p), r) : 0;
    }

  RawChunk<BF16> raw[2][4];
  float mu[8], mu_next[8];
  const auto fetch = [&](int step) {
    const int col = c0 + step * GRAM_STEP + ch * 8;
    const bool cok = col < c1;
#pragma unroll
    for (int e = 0; e < 8; ++e) mu_next[e] = cok ? a.mean[(int64_t)p * a.d + col + e] : 0.0f;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) raw_fill(raw[s][j], rok[s][j] && cok, a.x, roff[s][j] + col);
  };
  // (a row past t or a column past the chunk was fetched as zeros and has a zero mean: it is staged as zero)
  const auto stage = [&](int) {
#pragma unroll
    for (int e = 0; e < 8; ++e) mu[e] = mu_next[e];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int src = s == 1 && diag ? 0 : s;  // a diagonal pair stages the one tile as both operands
        bf16x8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (bf16_t)(rok[src][j] ? raw[src][j].get(e) - mu[e] : 0.0f);
        *reinterpret_cast<bf16x8*>(smem + s * T128_OPER + t128_off(rl + 32 * j, ch)) = z;
      }
  };

  f32x16 acc[2][2];
  acc_zero(acc);
  staged_steps(nsteps, fetch, stage, [&]() { t128_mfma<0, 4>(smem, wr, wc, l31, hh, acc); });
  acc_store<false>(a.part + (((int64_t)p * a.npairs + pair) * a.nchunks + chunk) * (PCA_T * PCA_T), PCA_T, PCA_T, PCA_T, wr, wc, l31, hh, acc);
}

// ---- back-projection (Gram eigenvectors -> components) ----------------------------------------------
// part[((p * nchunks + chunk) * k + j) * d + c] = sum over the chunk's rows of u[p, j, r] * (float(x[r, c]) - mean[p, c])
__global__ __launch_bounds__(256) void pca_back_kernel(PcaArgs a, const float* u, int k) {
  __shared__ float s[16][PCA_T];
  const int ncg = a.nt;
  int id = blockIdx.x;
  const int cg = id % ncg;
  id /= ncg;
  const int chunk = id % a.nchunks, p = id / a.nchunks;
  const int ch = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = cg * PCA_T + ch * 8;
  const bool cok = col < a.d;
  const int64_t r0 = (int64_t)chunk * PCA_CHUNK;
  const int64_t r1 = r0 + PCA_CHUNK < a.R ? r0 + PCA_CHUNK : a.R;
  float mu[8], acc[8][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) mu[e] = cok ? a.mean[(int64_t)p * a.d + col + e] : 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] = 0.0f;
  if (cok)
    for (int64_t r = r0 + rl; r < r1; r += 16) {
      float v[8];
      pca_load8(a, desc_row(a, pca_base(a, p), r) + col, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] -= mu[e];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < k) {
          const float w = u[((int64_t)p * k + j) * a.R + r];
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[j][e] += w * v[e];
        }
    }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j >= k) break;  // (uniform)
    __syncthreads();  // every thread has read the previous component
    fold_row_lanes(s, threadIdx.x, acc[j], a.d - cg * PCA_T, a.part + (((int64_t)p * a.nchunks + chunk) * k + j) * a.d + cg * PCA_T);
  }
}

// one workgroup per (problem, component): chunk sums folded ascending, the squared norm in float64 (a thread's columns
// tid, tid + 256, ... ascending, then a fixed binary tree over the 256 threads), one float64 division per element
__global__ __launch_bounds__(256) void pca_back_finish_kernel(PcaArgs a, const float* values, int k, float* comps) {
  __shared__ double s[256];
  const int p = blockIdx.x / k, j = blockIdx.x - p * k;
  float* out = comps + ((int64_t)p * k + j) * a.d;
  double ss = 0.0;
  for (int c = threadIdx.x; c < a.d; c += 256) {
    const float sum = fold_chunks(a.part + ((int64_t)p * a.nchunks * k + j) * a.d + c, a.nchunks, (int64_t)k * a.d);
    out[c] = sum;
    ss += (double)sum * (double)sum;
  }
  const double norm = sqrt(block_reduce_256(s, (int)threadIdx.x, ss, [](double x, double y) { return x + y; }));
  const bool live = values[(int64_t)p * k + j] > 0.0f && norm > 0.0;
  for (int c = threadIdx.x; c < a.d; c += 256) out[c] = live ? (float)((double)out[c] / norm) : 0.0f;
}

// ---- projection -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pca_project_kernel(PcaArgs a, const float* comps, int k, int nblocks, float* proj) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_mean = reinterpret_cast<float*>(smem);  // [d]
  float* s_comp = s_mean + a.d;                     // [k][d]
  float (*s_mm)[2] = reinterpret_cast<float (*)[2]>(s_comp + k * a.d);  // [4][2]
  const int p = blockIdx.x / nblocks, blk = blockIdx.x - p * nblocks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int c = threadIdx.x * 4; c < a.d; c += 1024)
    *reinterpret_cast<f32x4*>(s_mean + c) = *reinterpret_cast<const f32x4*>(a.mean + (int64_t)p * a.d + c);
  for (int c = threadIdx.x * 4; c < k * a.d; c += 1024)
    *reinterpret_cast<f32x4*>(s_comp + c) = *reinterpret_cast<const f32x4*>(comps + (int64_t)p * k * a.d + c);
  __syncthreads();
  float lo = INFINITY, hi = -INFINITY;
  const int64_t rbase = (int64_t)blk * PCA_PROJ_ROWS + wave * (PCA_PROJ_ROWS / 4);
  for (int i = 0; i < PCA_PROJ_ROWS / 4; ++i) {
    const int64_t r = rbase + i;
    if (r >= a.R) break;  // (wave-uniform)
    const int64_t off = desc_row(a, pca_base(a, p), r);
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = lane * 8; c < a.d; c += 512) {
      float v[8];
      pca_load8(a, off + c, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] -= s_mean[c + e];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < k) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[j] += v[e] * s_comp[j * a.d + c + e];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < k) {
        const float s = wave_sum(acc[j]);
        lo = fminf(lo, s);
        hi = fmaxf(hi, s);
        if (lane == 0) proj[((int64_t)p * a.R + r) * k + j] = s;
      }
  }
  if (lane == 0) {
    s_mm[wave][0] = lo;
    s_mm[wave][1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      lo = fminf(lo, s_mm[w][0]);
      hi = fmaxf(hi, s_mm[w][1]);
    }
    a.part[((int64_t)p * nblocks + blk) * 2] = lo;
    a.part[((int64_t)p * nblocks + blk) * 2 + 1] = hi;
  }
}

__global__ __launch_bounds__(256) void pca_minmax_kernel(const float* part, int nblocks, float* minmax) {
  struct MinMax {
    float lo, hi;
  };
  __shared__ MinMax s[256];
  const int p = blockIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int b = threadIdx.x; b < nblocks; b += 256) {
    lo = fminf(lo, part[((int64_t)p * nblocks + b) * 2]);
    hi = fmaxf(hi, part[((int64_t)p * nblocks + b) * 2 + 1]);
  }
  const MinMax mm = block_reduce_256(s, (int)threadIdx.x, MinMax{lo, hi},
                                     [](MinMax x, MinMax y) { return MinMax{fminf(x.lo, y.lo), fmaxf(x.hi, y.hi)}; });
  if (threadIdx.x == 0) {
    minmax[2 * p] = mm.lo;
    minmax[2 * p + 1] = mm.hi;
  }
}

__global__ __launch_bounds__(256) void pca_scale_kernel(float* proj, const float* minmax, int64_t per_problem, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t p = idx / per_problem;
  const float lo = minmax[2 * p], hi = minmax[2 * p + 1];
  if (hi != lo) proj[idx] = __fdiv_rn(proj[idx] - lo, hi - lo);
}

int64_t pca_chunks(int64_t R) { return (R + PCA_CHUNK - 1) / PCA_CHUNK; }
int64_t pca_proj_blocks(int64_t R) { return (R + PCA_PROJ_ROWS - 1) / PCA_PROJ_ROWS; }

bool pca_args(PcaArgs& a, const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
              void* work, int dmax = 2048) {
  if (!x || !work || problems <= 0 || imgs <= 0 || t <= 0 || d <= 0 || (d & 31) || d > dmax || ld < d || image_stride < 0)
    return false;
  const int64_t per16 = in_bf16 ? 8 : 4;
  if ((((uintptr_t)x | (uintptr_t)work) & 15) || ld % per16 || image_stride % per16) return false;
  const int64_t R = (int64_t)imgs * t;
  if (R > INT32_MAX || R * problems > INT32_MAX) return false;
  a.x = x;
  a.ld = ld, a.is = image_stride, a.R = R;
  a.imgs = imgs, a.t = t, a.d = d, a.in_bf16 = in_bf16;
  a.nt = (d + PCA_T - 1) / PCA_T;
  a.npairs = a.nt * (a.nt + 1) / 2;
  a.nchunks = (int)pca_chunks(R);
  a.mean = nullptr;
  a.part = (float*)work;
  return true;
}

}  // namespace

size_t pca_work_bytes(int problems, int imgs, int t, int d) {
  if (problems <= 0 || imgs <= 0 || t <= 0 || d <= 0) return 0;
  const int64_t R = (int64_t)imgs * t, nt = (d + PCA_T - 1) / PCA_T;
  const int64_t mean = pca_chunks(R) * d, cov = nt * (nt + 1) / 2 * pca_chunks(R) * (PCA_T * PCA_T), proj = pca_proj_blocks(R) * 2;
  int64_t n = mean > cov ? mean : cov;
  n = n > proj ? n : proj;
  return (size_t)((n * problems * 4 + 15) & ~(int64_t)15);
}

static hipError_t col_mean(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                           int dmax, void* work, float* mean, hipStream_t st) {
  PcaArgs a;
  if (!mean || !pca_args(a, x, in_bf16, ld, image_stride, problems, imgs, t, d, work, dmax)) return hipErrorInvalidValue;
  const int64_t grid = (int64_t)problems * a.nchunks * a.nt;
  if (grid > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pca_mean_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(pca_mean_finish_kernel, dim3((unsigned)(((int64_t)problems * d + 255) / 256)), dim3(256), 0, st, a, problems, mean);
  return hipGetLastError();
}

hipError_t launch_col_mean(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                           void* work, float* mean, hipStream_t st) {
  return col_mean(x, in_bf16, ld, image_stride, problems, imgs, t, d, 2048, work, mean, st);
}

hipError_t launch_covariance(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                             const float* mean, void* work, float* cov, hipStream_t st) {
  PcaArgs a;
  if (!mean || !cov || !pca_args(a, x, in_bf16, ld, image_stride, problems, imgs, t, d, work) || a.R < 2) return hipErrorInvalidValue;
  a.mean = mean;
  const int64_t items = (int64_t)problems * a.npairs * a.nchunks;
  const int64_t fin = (int64_t)problems * a.npairs * (PCA_T * PCA_T / 256);
  if (items > INT32_MAX || fin > INT32_MAX) return hipErrorInvalidValue;
  if (in_bf16) hipLaunchKernelGGL(pca_cov_kernel<true>, dim3((unsigned)items), dim3(256), 2 * PCA_IMG, st, a);
  else hipLaunchKernelGGL(pca_cov_kernel<false>, dim3((unsigned)items), dim3(256), 2 * PCA_IMG, st, a);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(pca_cov_finish_kernel, dim3((unsigned)fin), dim3(256), 0, st, a, cov);
  return hipGetLastError();
}

hipError_t launch_pca_project(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int imgs, int t, int d,
                              const float* mean, const float* comps, int k, int scale, void* work, float* proj, float* minmax,
                              hipStream_t st) {
  PcaArgs a;
  if (!mean || !comps || !proj || !minmax || k < 1 || k > 8 ||
      !pca_args(a, x, in_bf16, ld, image_stride, problems, imgs, t, d, work))
    return hipErrorInvalidValue;
  a.mean = mean;
  const int nblocks = (int)pca_proj_blocks(a.R);
  const int64_t grid = (int64_t)problems * nblocks;
  const size_t lds = (size_t)(k + 1) * d * 4 + 32;
  static KernelState ks;
  const int dev = current_device_index();
  if (dev < 0) return hipErrorInvalidDevice;
  if (hipError_t e = raise_lds_limit(ks, (const void*)pca_project_kernel, dev, lds)) return e;
  hipLaunchKernelGGL(pca_project_kernel, dim3((unsigned)grid), dim3(256), lds, st, a, comps, k, nblocks, proj);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(pca_minmax_kernel, dim3((unsigned)problems), dim3(256), 0, st, a.part, nblocks, minmax);
  if (hipError_t e = hipGetLastError()) return e;
  if (scale) {
    const int64_t per = a.R * k, total = per * problems;
    hipLaunchKernelGGL(pca_scale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, proj, minmax, per, total);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

static int64_t gram_chunks(int d) { return (d + GRAM_CHUNK - 1) / GRAM_CHUNK; }

size_t pca_topk_side_work_bytes(int problems, int t, int d, int k) {
  if (problems <= 0 || t <= 0 || d <= 0 || k <= 0) return 0;
  const int64_t nt = (t + T128 - 1) / T128;
  const int64_t mean = pca_chunks(t) * d, gram = nt * (nt + 1) / 2 * gram_chunks(d) * (PCA_T * PCA_T), back = pca_chunks(t) * k * d;
  int64_t n = mean > gram ? mean : gram;
  n = n > back ? n : back;
  return (size_t)((n * problems * 4 + 15) & ~(int64_t)15);
}

hipError_t launch_col_mean_any(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int t, int d, void* work,
                               float* mean, hipStream_t st) {
  return col_mean(x, in_bf16, ld, image_stride, problems, 1, t, d, INT32_MAX & ~31, work, mean, st);
}

hipError_t launch_gram(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int t, int d, const float* mean,
                       void* work, float* gram, hipStream_t st) {
  PcaArgs a;
  if (!mean || !gram || t < 2 || t > 4096 || !pca_args(a, x, in_bf16, ld, image_stride, problems, 1, t, d, work, INT32_MAX & ~31))
    return hipErrorInvalidValue;
  a.mean = mean;
  a.nt = (t + T128 - 1) / T128;
  a.npairs = a.nt * (a.nt + 1) / 2;
  a.nchunks = (int)gram_chunks(d);
  const int64_t items = (int64_t)problems * a.npairs * a.nchunks;
  const int64_t fin = (int64_t)problems * a.npairs * (PCA_T * PCA_T / 256);
  if (items > INT32_MAX || fin > INT32_MAX) return hipErrorInvalidValue;
  if (in_bf16) hipLaunchKernelGGL(pca_gram_kernel<true>, dim3((unsigned)items), dim3(256), 2 * T128_OPER, st, a);
  else hipLaunchKernelGGL(pca_gram_kernel<false>, dim3((unsigned)items), dim3(256), 2 * T128_OPER, st, a);
  if (hipError_t e = hipGetLastError()) return e;
  PcaArgs f = a;  // the fold of the covariance, on a t x t matrix: side t, divisor R - 1 = t - 1
  f.d = t;
  hipLaunchKernelGGL(pca_cov_finish_kernel, dim3((unsigned)fin), dim3(256), 0, st, f, gram);
  return hipGetLastError();
}

hipError_t launch_pca_back_project(const void* x, int in_bf16, int64_t ld, int64_t image_stride, int problems, int t, int d,
                                   const float* mean, const float* u, const float* values, int k, void* work, float* comps,
                                   hipStream_t st) {
  PcaArgs a;
  if (!mean || !u || !values || !comps || k < 1 || k > 8 ||
      !pca_args(a, x, in_bf16, ld, image_stride, problems, 1, t, d, work, INT32_MAX & ~31))
    return hipErrorInvalidValue;
  a.mean = mean;
  const int64_t grid = (int64_t)problems * a.nchunks * a.nt;
  if (grid > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pca_back_kernel, dim3((unsigned)grid), dim3(256), 0, st, a, u, k);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(pca_back_finish_kernel, dim3((unsigned)(problems * k)), dim3(256), 0, st, a, values, k, comps);
  return hipGetLastError();
}

}  // namespace vdr
