// Windowed correlation of two descriptor maps on one grid for gfx950 (include/vdr.h, vdr_op_local_correlation): for `pairs`
// problems X_p, Y_p [t = gh * gw, d] (bf16 rows ldx / ldy elements apart, pairs x_stride / y_stride apart, 0 allowed)
//   cost[p, i, w] = sim(i, j) = (dot(x_i, y_j) * rn(x_i)) * rn(y_j)   for the candidate j of window slot w of query i,
//                   -inf where that candidate lies outside the grid;   best_sim / best_idx the maximum over the window.
// sim is vdr_op_nn_cosine's, bit for bit: the same rn, the same MFMA steps in the same k order, the same association
// (`transposed`: the association of the reverse direction, (dot * rn(y_j)) * rn(x_i), the bits of nn_cosine's column side).
//
// Three launches, no atomics:
//   cosine_rnorm_kernel  (nn_cosine.hip) rn of every row of X and Y into `work`: nn_cosine's, by the same kernel.
//   local_corr_kernel  256 threads; one work item = (pair, panel of 8 x 16 queries, tile of 128 halo candidates), the mapping
//                      of local_corr_map.h.  nn_cosine_kernel's K loop (dma_steps of desc_tile.h, over one tile) with gathered
//                      source rows (t128_dma_stage): per step of 64 channels both operands go global -> LDS by LDS-DMA into
//                      the t128 image, two buffers, step s + 1 in flight under the MFMAs of step s.  The per-lane source rows
//                      are the mapping's `src`: positions outside
//                      the grid, past the ragged panel or past the halo load a clamped (valid) row, whose finite values are
//                      dropped in the epilogue.  Epilogue: a lane holds ONE candidate and 16 query rows per accumulator; for
//                      every element whose candidate falls in the query's window (lc_slot) it stores sim -- or -inf for a
//                      candidate outside the grid -- to cost[p, i, slot].  The halo holds each (query, slot) once, so every
//                      entry of cost has exactly one writer and nothing is pre-filled.  Consecutive lanes are consecutive
//                      halo columns, so the 4-byte stores fall in runs of up to 2r + 1.
//   lc_finish_kernel   (only when the best pair is asked for) one wave per query folds its in-grid slots with NnBetter --
//                      greater value, then lower candidate index: a total order, so the lane grouping does not matter.
// With cost == NULL the tile kernel writes the cost rows into `work` and the fold reads them there.  Every value depends on
// (gh, gw, r, d, inputs) alone: an item never looks at another problem, and there is no launch heuristic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "desc_tile.h"
#include "local_corr_map.h"
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {
namespace {

constexpr int LC_RN = 4 * T128_OPER;    // s_rn [256] float: rn of the tile's candidates | of the panel's queries
constexpr int LC_LDS = LC_RN + 1024;
static_assert(LC_TILE == T128, "the panel and the halo tile are operands of the t128 image");

struct LcArgs {
  const bf16_t *x, *y;
  int64_t ldx, xs, ldy, ys;
  LcGeom g;
  int t, d, t_pad;
  int transposed;    // sim = (dot * rn(y_j)) * rn(x_i): the association of the reverse direction (include/vdr.h)
  float *rnx, *rny;  // [pairs][t_pad] each
  float* cost;       // [pairs][t][W * W]: the caller's, or the scratch copy in `work`
};

__global__ __launch_bounds__(256, 2) void local_corr_kernel(LcArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  // (pair, panel, tile), tile fastest, in XCD-contiguous order: the tiles of a panel share its queries and most of their
  // candidates with the neighbouring panels, and meet in one XCD's L2
  const int vid = xcd_remap(blockIdx.x, gridDim.x);
  const int pp = vid / a.g.ntiles, tile = vid - pp * a.g.ntiles;
  const int p = pp / a.g.npanels, panel = pp - p * a.g.npanels;
  const bf16_t* xp = a.x + (int64_t)p * a.xs;
  const bf16_t* yp = a.y + (int64_t)p * a.ys;
  float* s_rn = reinterpret_cast<float*>(smem + LC_RN);

  // the rows this lane stages, fixed over the K loop: 4 of the panel and 4 of the tile (element offsets of clamped rows)
  int64_t xo[4], yo[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = t128_dma_row(wave, lane, q);
    xo[q] = (int64_t)lc_map(a.g, panel, tile, 0, r).src * a.ldx;
    yo[q] = (int64_t)lc_map(a.g, panel, tile, 1, r).src * a.ldy;
  }
  {  // rn of the item's 128 candidates and 128 queries, gathered through the same mapping; visible after the first dma_wait
    const int t = threadIdx.x, side = t < 128 ? 1 : 0, r = t & 127;
    const int src = lc_map(a.g, panel, tile, side, r).src;
    s_rn[t] = (side ? a.rny : a.rnx)[(int64_t)p * a.t_pad + src];
  }

  f32x16 acc[2][2];
  acc_zero(acc);
  // one tile.  Its epilogue follows the loop instead of being handed in: inside the loop its lane masks are loop invariants
  // kept in SGPR pairs, and the kernel goes to 256 VGPRs, 68 + 12 spills, 52 bytes of scratch and occupancy 2
  dma_steps(0, 1, a.d, smem, wr, wc, l31, hh, acc,
            [&](int, int kk, char* sx) { t128_dma_stage(xp, yp, xo, yo, a.d, kk, sx, wave, lane); }, [](int) {});

  // ---- epilogue: this lane's two candidates against its 32 queries
  float rny[2];
  LcPos cp[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int col = acc_col(wc, n, l31);
    rny[n] = s_rn[col];
    cp[n] = lc_map(a.g, panel, tile, 1, col);
  }
  const int64_t WW = (int64_t)a.g.W * a.g.W;
  float* cost = a.cost + (int64_t)p * a.t * WW;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int rloc = acc_row(wr, m, e, hh);
      const LcPos qp = lc_map(a.g, panel, tile, 0, rloc);
      const float rnx = s_rn[128 + rloc];
      float* crow = cost + (int64_t)qp.src * WW;  // (src is the query's own row when qp.ok, and a valid one otherwise)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const float v = a.transposed ? (acc[m][n][e] * rny[n]) * rnx : (acc[m][n][e] * rnx) * rny[n];
        const int slot = lc_slot(a.g, qp.y, qp.x, cp[n].y, cp[n].x);
        if (qp.ok && slot >= 0) crow[slot] = cp[n].ok ? v : -INFINITY;
      }
    }
}

// one wave per query: the in-grid slots of its cost row folded to (best value, lowest candidate index that attains it)
__global__ __launch_bounds__(256) void lc_finish_kernel(LcArgs a, int pairs, float* best_sim, int32_t* best_idx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)pairs * a.t) return;
  const int i = (int)(row % a.t);
  const int qy = i / a.g.gw, qx = i - qy * a.g.gw;
  const int WW = a.g.W * a.g.W;
  const float* c = a.cost + row * WW;
  float bv = -INFINITY;
  int bi = INT32_MAX;
  for (int w = lane; w < WW; w += 64) {
    const int wy = w / a.g.W;
    const int cy = qy + wy - a.g.r, cx = qx + (w - wy * a.g.W) - a.g.r;
    if (cy < 0 || cy >= a.g.gh || cx < 0 || cx >= a.g.gw) continue;
    const float v = c[w];
    const int j = cy * a.g.gw + cx;
    if (nn_better(v, j, bv, bi)) {
      bv = v;
      bi = j;
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (nn_better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    best_sim[row] = bv;
    best_idx[row] = bi;
  }
}

// the sections of `work`, in 4-byte elements, each a multiple of 4 elements (16 bytes)
struct LcLayout {
  int64_t t_pad, rn, cost;
};
LcLayout lc_layout(int pairs, int gh, int gw, int radius) {
  LcLayout l;
  const int64_t t = (int64_t)gh * gw, W = 2 * radius + 1;
  l.t_pad = (t + LC_TILE - 1) / LC_TILE * LC_TILE;
  l.rn = (int64_t)pairs * l.t_pad;
  l.cost = ((int64_t)pairs * t * W * W + 3) / 4 * 4;
  return l;
}

}  // namespace

size_t local_correlation_work_bytes(int pairs, int gh, int gw, int radius) {
  if (pairs <= 0 || gh <= 0 || gw <= 0 || radius < 1 || radius > LC_MAX_RADIUS) return 0;
  const LcLayout l = lc_layout(pairs, gh, gw, radius);
  return (size_t)(2 * l.rn + l.cost) * 4;
}

hipError_t launch_local_correlation(const void* x, int64_t ldx, int64_t x_stride, const void* y, int64_t ldy, int64_t y_stride,
                                    int pairs, int gh, int gw, int d, int radius, int transposed, void* work, float* cost,
                                    float* best_sim, int32_t* best_idx, hipStream_t st) {
  const int64_t t = (int64_t)gh * gw, WW = (int64_t)(2 * radius + 1) * (2 * radius + 1);
  if (gh <= 0 || gw <= 0 || !cos_operand_ok(x, ldx, x_stride, t, d) || !cos_operand_ok(y, ldy, y_stride, t, d) || !work ||
      ((uintptr_t)work & 15) || (!best_sim) != (!best_idx) || (!cost && !best_sim) || pairs <= 0 || radius < 1 || radius > LC_MAX_RADIUS)
    return hipErrorInvalidValue;
  if (t > INT32_MAX || (int64_t)pairs * t > INT32_MAX / WW) return hipErrorInvalidValue;  // pairs * t * W * W <= 2^31 - 1
  const LcLayout l = lc_layout(pairs, gh, gw, radius);
  LcArgs a;
  a.x = (const bf16_t*)x;
  a.y = (const bf16_t*)y;
  a.ldx = ldx, a.xs = x_stride, a.ldy = ldy, a.ys = y_stride;
  a.g = lc_geom(gh, gw, radius);
  a.t = (int)t, a.d = d, a.t_pad = (int)l.t_pad;
  a.transposed = transposed != 0;
  float* w = (float*)work;
  a.rnx = w;
  a.rny = a.rnx + l.rn;
  a.cost = cost ? cost : a.rny + l.rn;
  const int64_t items = (int64_t)pairs * a.g.npanels * a.g.ntiles;
  if (items > INT32_MAX) return hipErrorInvalidValue;

  static KernelState ks;
  const int dev = current_device_index();
  if (dev < 0) return hipErrorInvalidDevice;
  if (hipError_t e = raise_lds_limit(ks, (const void*)local_corr_kernel, dev, LC_LDS)) return e;
  const int64_t rows = (int64_t)pairs * t;
  if (hipError_t e = launch_cosine_rnorm({a.x, ldx, x_stride, a.t, a.t_pad, a.rnx}, {a.y, ldy, y_stride, a.t, a.t_pad, a.rny}, d, pairs, st))
    return e;
  hipLaunchKernelGGL(local_corr_kernel, dim3((unsigned)items), dim3(256), LC_LDS, st, a);
  if (hipError_t e = hipGetLastError()) return e;
  if (best_sim) {
    hipLaunchKernelGGL(lc_finish_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a, pairs, best_sim, best_idx);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace vdr
