// Cosine nearest neighbours between two descriptor maps for gfx950 (include/vdr.h, vdr_op_nn_cosine): for `pairs`
// problems X_p [tx, d], Y_p [ty, d] (bf16 rows ldx / ldy elements apart, pairs x_stride / y_stride apart, 0 allowed)
//   sim(i, j)  = (dot(x_i, y_j) * rn(x_i)) * rn(y_j),   rn(v) = 1 / max(sqrt(sum v^2), 1e-8)
//   row_sim[i] = max_j sim(i, j), row_idx[i] the lowest j that attains it; col_sim / col_idx likewise over i.
// The tx x ty similarity matrix is never written: it exists one 128 x 128 tile at a time in MFMA accumulators.
//
// Three launches, no atomics:
//   cosine_rnorm_kernel  rn (cosine_rn of desc_tile.h) of every row of X and Y into `work`: one wave per row.  Also the
//                      row norms of local_corr.hip (launch_cosine_rnorm, vdr_kernels.h).
//   nn_cosine_kernel   256 threads; one work item = (pair, run of Y's tiles, 128-row panel of X; run_split of desc_tile.h).
//                      It walks its 128-row tiles of Y; per tile a K loop over d in steps of 64 stages both operands
//                      global -> LDS (LDS-DMA, two buffers: step s + 1 is in flight under the MFMAs of step s).  The loop
//                      and the staging are the kernel's own copy of dma_steps / t128_dma_stage of desc_tile.h: through
//                      the helpers it ran up to 3 % slower.  X is the A operand, Y the B operand of the
//                      tile of desc_tile.h, so a lane holds ONE column j and 16 rows i.
//                      Epilogue per tile, in that layout: scale, mask the ragged rows / columns with -inf, fold every
//                      element into the lane's running row best (kept across the tiles), reduce the tile's column best
//                      over registers, lane halves and the two row waves (LDS), write it as a partial (value, index).
//                      At the end of the item row_best_reduce; the row best is written as a partial too.
//   nn_finish_kernel   folds the row partials over the splits and the column partials over the panels, ascending.
// Every fold uses one comparison -- greater value, then lower index -- which is a total order on (value, index) pairs
// with distinct indices: the result is the same whatever the grouping, so it depends neither on the split count (a
// launch heuristic) nor on `pairs`.  dot is the MFMA's fp32 accumulation in k order; both are fixed.
//
// Rows past the end of a map repeat its last row (finite values, masked in the epilogue); the image, the source chunk a
// lane copies (swizzle, short last step of d % 64 == 32: t128_dma_chunk) and the wait (dma_wait) are desc_tile.h's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "desc_tile.h"
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {
namespace {

constexpr int NN_T = T128;                  // tile side (rows of X per panel, rows of Y per tile)
constexpr int NN_RN = 4 * T128_OPER;        // s_rn [2][256] float: tile parity x (rn of the tile's Y rows | of the panel's X rows)
constexpr int NN_COL = NN_RN + 2048;        // column exchange: value [128], index [128]
constexpr int NN_ROW = NN_COL + 1024;       // row exchange: value [2][128], index [2][128]
constexpr int NN_LDS = NN_ROW + 2048;

// (flat, in this order: with the fields regrouped by side nn_cosine_kernel spills 150 SGPRs instead of 142)
struct NnArgs {
  const bf16_t *x, *y;
  int64_t ldx, xs, ldy, ys;
  int tx, ty, d, npanels, ntiles, nsplit, tx_pad, ty_pad, do_cols;
  int split_base, split_rem;  // tiles per split: ntiles / nsplit, and the first ntiles % nsplit splits take one more
  float *rnx, *rny;      // [pairs][tx_pad], [pairs][ty_pad]
  float* colv;           // [pairs][npanels][ty_pad]
  int32_t* coli;
  float* rowv;           // [pairs][nsplit][tx_pad]
  int32_t* rowi;
};

__global__ __launch_bounds__(256) void cosine_rnorm_kernel(CosSide X, CosSide Y, int d, int pairs) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nx = (int64_t)pairs * X.t;
  if (row >= nx + (int64_t)pairs * Y.t) return;
  const CosSide s = row < nx ? X : Y;
  const int64_t r = row < nx ? row : row - nx;
  const int64_t p = r / s.t;
  const int i = (int)(r - p * s.t);
  const float ss = row_sumsq((const bf16_t*)s.x + p * s.ps + (int64_t)i * s.ld, d, lane);
  if (lane == 0) s.rn[p * s.t_pad + i] = cosine_rn(ss);
}

// one K step of (panel, tile jt) into staging buffer `buf`: 4 + 4 DMA instructions per wave, 8 rows x 128 B each
VDR_DEV void nn_stage(const NnArgs& a, const bf16_t* xp, const bf16_t* yp, int64_t p, int panel, int jt, int kk, char* smem,
                      int buf, int wave, int lane) {
  const int k0 = kk * 64;
  const bool shortk = a.d - k0 < 64;
  char* sx = smem + buf * 2 * T128_OPER;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int piece = wave * 4 + q;
    const int r = piece * 8 + (lane >> 3);
    const int c = t128_dma_chunk(lane, r, shortk);
    const int xr = min(panel * NN_T + r, a.tx - 1), yr = min(jt * NN_T + r, a.ty - 1);
    glds16_raw(xp + (int64_t)xr * a.ldx + k0 + c * 8, sx + piece * 1024);
    glds16_raw(yp + (int64_t)yr * a.ldy + k0 + c * 8, sx + T128_OPER + piece * 1024);
  }
  if (kk == 0 && wave == 0) {  // the tile's rn values ride on the same wait: lanes 0..31 Y's, 32..63 the panel's
    const float* src = lane < 32 ? a.rny + p * a.ty_pad + jt * NN_T + lane * 4 : a.rnx + p * a.tx_pad + panel * NN_T + (lane - 32) * 4;
    glds16_raw(src, smem + NN_RN + (jt & 1) * 1024);
  }
}

__global__ __launch_bounds__(256, 2) void nn_cosine_kernel(NnArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  // (pair, split, panel), panel fastest, in XCD-contiguous order: the panels that read the same tiles of Y_p run next to
  // each other on one XCD and meet in its L2
  const int vid = xcd_remap(blockIdx.x, gridDim.x);
  const int ps = vid / a.npanels, panel = vid - ps * a.npanels;
  const int p = ps / a.nsplit, split = ps - p * a.nsplit;
  int jt0, jt1;
  run_tiles(split, a.split_base, a.split_rem, jt0, jt1);
  const bf16_t* xp = a.x + (int64_t)p * a.xs;
  const bf16_t* yp = a.y + (int64_t)p * a.ys;

  float rbv[2][16];
  int rbi[2][16];
  f32x16 acc[2][2];
  acc_zero(acc);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      rbv[m][e] = -INFINITY;
      rbi[m][e] = INT32_MAX;
    }
  float* s_rn = reinterpret_cast<float*>(smem + NN_RN);
  float* s_colv = reinterpret_cast<float*>(smem + NN_COL);
  int* s_coli = reinterpret_cast<int*>(smem + NN_COL + 512);

  // dma_steps of desc_tile.h, spelled out (see there for the counters and the buffers)
  const int nk = (a.d + 63) >> 6;
  const int nsteps = (jt1 - jt0) * nk;
  int jt = jt0, kk = -1, buf = 1;
#pragma clang loop unroll(disable)
  for (int s = -1; s < nsteps; ++s) {
    int njt = jt, nkk = kk + 1;
    if (nkk == nk) {
      nkk = 0;
      ++njt;
    }
    if (s + 1 < nsteps) nn_stage(a, xp, yp, p, panel, njt, nkk, smem, buf ^ 1, wave, lane);
    if (s >= 0) {
      const char* sx = smem + buf * 2 * T128_OPER;
      t128_mfma<0, 2>(sx, wr, wc, l31, hh, acc);
      if (a.d - kk * 64 >= 64) t128_mfma<2, 4>(sx, wr, wc, l31, hh, acc);
      if (kk + 1 == nk) {
        // ---- epilogue of tile jt
        const float* rn = s_rn + (jt & 1) * 256;
        float rny[2], cbv[2];
        int gcol[2], cbi[2];
        bool cok[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          rny[n] = rn[acc_col(wc, n, l31)];
          gcol[n] = jt * NN_T + wc * 64 + n * 32 + l31;  // acc_col spelled out: through the helper, two more SGPRs spill
          cok[n] = gcol[n] < a.ty;
          cbv[n] = -INFINITY;
          cbi[n] = INT32_MAX;
        }
        // rows of the panel this lane may count, as (constant < per-lane threshold) with the threshold made opaque here:
        // written as `grow < tx` the 32 lane masks are loop invariants that hipcc keeps in SGPR pairs and spills (mask_keys)
        int rthr = a.tx - panel * NN_T - wr * 64 - 4 * hh;
        asm volatile("" : "+v"(rthr));
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int rloc = acc_row(wr, m, e, hh);
            const int grow = panel * NN_T + rloc;
            const bool rok = acc_row(0, m, e, 0) < rthr;
            const float rnx = rn[128 + rloc];
#pragma unroll
            for (int n = 0; n < 2; ++n) {
              const float v = (acc[m][n][e] * rnx) * rny[n];
              acc[m][n][e] = 0.0f;
              // (ascending j within the lane, ascending i within the column: a strict > keeps the lowest index)
              const float vr = cok[n] ? v : -INFINITY;
              if (vr > rbv[m][e]) {
                rbv[m][e] = vr;
                rbi[m][e] = gcol[n];
              }
              const float vc = rok ? v : -INFINITY;
              if (vc > cbv[n]) {
                cbv[n] = vc;
                cbi[n] = grow;
              }
            }
          }
        if (a.do_cols) {
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            const float ov = __shfl_xor(cbv[n], 32, 64);
            const int oi = __shfl_xor(cbi[n], 32, 64);
            if (nn_better(ov, oi, cbv[n], cbi[n])) {
              cbv[n] = ov;
              cbi[n] = oi;
            }
            if (wr == 1 && hh == 0) {
              s_colv[acc_col(wc, n, l31)] = cbv[n];
              s_coli[acc_col(wc, n, l31)] = cbi[n];
            }
          }
          __syncthreads();
          if (wr == 0 && hh == 0) {
            const int64_t base = ((int64_t)p * a.npanels + panel) * a.ty_pad;
#pragma unroll
            for (int n = 0; n < 2; ++n) {
              const float ov = s_colv[acc_col(wc, n, l31)];
              const int oi = s_coli[acc_col(wc, n, l31)];
              if (nn_better(ov, oi, cbv[n], cbi[n])) {
                cbv[n] = ov;
                cbi[n] = oi;
              }
              if (cok[n]) {
                a.colv[base + gcol[n]] = cbv[n];
                a.coli[base + gcol[n]] = cbi[n];
              }
            }
          }
        }
      }
    }
    dma_wait();
    buf ^= 1;
    jt = njt;
    kk = nkk;
  }
  // ---- row best of the item
  const int t = threadIdx.x;
  const RowBest b = row_best_reduce(rbv, rbi, reinterpret_cast<float*>(smem + NN_ROW), reinterpret_cast<int*>(smem + NN_ROW + 1024), t,
                                    nn_better);
  if (t < 128) {
    // (rows past tx land in the padding of the partial and are never read)
    const int64_t o = ((int64_t)p * a.nsplit + split) * a.tx_pad + panel * NN_T + t;
    a.rowv[o] = b.v;
    a.rowi[o] = b.i;
  }
}

__global__ __launch_bounds__(256) void nn_finish_kernel(NnArgs a, int pairs, float* row_sim, int32_t* row_idx, float* col_sim,
                                                        int32_t* col_idx) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nx = (int64_t)pairs * a.tx, ny = a.do_cols ? (int64_t)pairs * a.ty : 0;
  if (idx < nx) {
    const int64_t p = idx / a.tx;
    const int i = (int)(idx - p * a.tx);
    const float* pv = a.rowv + p * a.nsplit * a.tx_pad + i;
    const int32_t* pi = a.rowi + p * a.nsplit * a.tx_pad + i;
    float v = pv[0];
    int b = pi[0];
    for (int s = 1; s < a.nsplit; ++s) {
      const float ov = pv[(int64_t)s * a.tx_pad];
      const int oi = pi[(int64_t)s * a.tx_pad];
      if (nn_better(ov, oi, v, b)) {
        v = ov;
        b = oi;
      }
    }
    row_sim[idx] = v;
    row_idx[idx] = b;
  } else if (idx - nx < ny) {
    const int64_t c = idx - nx, p = c / a.ty;
    const int j = (int)(c - p * a.ty);
    const float* pv = a.colv + p * a.npanels * a.ty_pad + j;
    const int32_t* pi = a.coli + p * a.npanels * a.ty_pad + j;
    float v = pv[0];
    int b = pi[0];
    for (int s = 1; s < a.npanels; ++s) {
      const float ov = pv[(int64_t)s * a.ty_pad];
      const int oi = pi[(int64_t)s * a.ty_pad];
      if (nn_better(ov, oi, v, b)) {
        v = ov;
        b = oi;
      }
    }
    col_sim[c] = v;
    col_idx[c] = b;
  }
}

// the sections of `work`, in 4-byte elements; each a multiple of 128 elements, so every section starts 16-byte aligned
struct NnLayout {
  int64_t npanels, ntiles, tx_pad, ty_pad, rn_x, rn_y, col, row;
};
NnLayout nn_layout(int pairs, int tx, int ty) {
  NnLayout l;
  l.npanels = (tx + NN_T - 1) / NN_T;
  l.ntiles = (ty + NN_T - 1) / NN_T;
  l.tx_pad = l.npanels * NN_T;
  l.ty_pad = l.ntiles * NN_T;
  l.rn_x = (int64_t)pairs * l.tx_pad;
  l.rn_y = (int64_t)pairs * l.ty_pad;
  l.col = (int64_t)pairs * l.npanels * l.ty_pad;
  // pairs * nsplit * tx_pad with nsplit <= max(1, COS_TARGET_ITEMS / (pairs * npanels)): never more than this, and monotone
  const int64_t items = (int64_t)pairs * l.npanels;
  l.row = (items > COS_TARGET_ITEMS ? items : COS_TARGET_ITEMS) * NN_T;
  return l;
}

}  // namespace

hipError_t launch_cosine_rnorm(const CosSide& X, const CosSide& Y, int d, int pairs, hipStream_t st) {
  const int64_t rows = (int64_t)pairs * X.t + (int64_t)pairs * Y.t;
  hipLaunchKernelGGL(cosine_rnorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, X, Y, d, pairs);
  return hipGetLastError();
}

size_t nn_cosine_work_bytes(int pairs, int tx, int ty) {
  if (pairs <= 0 || tx <= 0 || ty <= 0) return 0;
  const NnLayout l = nn_layout(pairs, tx, ty);
  return (size_t)(l.rn_x + l.rn_y + 2 * l.col + 2 * l.row) * 4;
}

hipError_t launch_nn_cosine(const void* x, int64_t ldx, int64_t x_stride, int tx, const void* y, int64_t ldy, int64_t y_stride,
                            int ty, int pairs, int d, void* work, float* row_sim, int32_t* row_idx, float* col_sim,
                            int32_t* col_idx, hipStream_t st) {
  if (!cos_operand_ok(x, ldx, x_stride, tx, d) || !cos_operand_ok(y, ldy, y_stride, ty, d) || !work || ((uintptr_t)work & 15) ||
      !row_sim || !row_idx || (!col_sim) != (!col_idx) || pairs <= 0)
    return hipErrorInvalidValue;
  if ((int64_t)pairs * (tx > ty ? tx : ty) > INT32_MAX) return hipErrorInvalidValue;
  const NnLayout l = nn_layout(pairs, tx, ty);
  NnArgs a;
  a.x = (const bf16_t*)x;
  a.y = (const bf16_t*)y;
  a.ldx = ldx, a.xs = x_stride, a.ldy = ldy, a.ys = y_stride;
  a.tx = tx, a.ty = ty, a.d = d;
  a.npanels = (int)l.npanels, a.ntiles = (int)l.ntiles, a.tx_pad = (int)l.tx_pad, a.ty_pad = (int)l.ty_pad;
  const int64_t items = (int64_t)pairs * l.npanels;
  const RunSplit run = run_split(items, l.ntiles);
  a.nsplit = run.nsplit, a.split_base = run.base, a.split_rem = run.rem;
  a.do_cols = col_sim != nullptr;
  a.rnx = (float*)work;
  a.rny = a.rnx + l.rn_x;
  a.colv = a.rny + l.rn_y;
  a.coli = (int32_t*)(a.colv + l.col);
  a.rowv = (float*)(a.coli + l.col);
  a.rowi = (int32_t*)(a.rowv + l.row);
  if (items * a.nsplit > INT32_MAX) return hipErrorInvalidValue;

  static KernelState ks;
  const int dev = current_device_index();
  if (dev < 0) return hipErrorInvalidDevice;
  if (hipError_t e = raise_lds_limit(ks, (const void*)nn_cosine_kernel, dev, NN_LDS)) return e;
  if (hipError_t e = launch_cosine_rnorm({a.x, ldx, x_stride, tx, a.tx_pad, a.rnx}, {a.y, ldy, y_stride, ty, a.ty_pad, a.rny}, d, pairs, st))
    return e;
  hipLaunchKernelGGL(nn_cosine_kernel, dim3((unsigned)(items * a.nsplit)), dim3(256), NN_LDS, st, a);
  if (hipError_t e = hipGetLastError()) return e;
  const int64_t outs = (int64_t)pairs * tx + (a.do_cols ? (int64_t)pairs * ty : 0);
  hipLaunchKernelGGL(nn_finish_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, a, pairs, row_sim, row_idx, col_sim,
                     col_idx);
  return hipGetLastError();
}

}  // namespace vdr
