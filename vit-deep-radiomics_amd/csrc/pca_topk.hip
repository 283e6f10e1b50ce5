// The k largest eigenpairs of symmetric positive semi-definite fp32 matrices for gfx950 (include/vdr.h, vdr_op_sym_topk):
// block subspace iteration with a Rayleigh-Ritz step on a block of 16 columns, everything on the device, no atomics, no
// host synchronisation.  One iteration is three launches; every launch returns at once for a problem whose `done` flag is
// set, so the host enqueues max_iter iterations and never looks.
//
//   topk_av_kernel     W = A V, the hot kernel (A is read once per iteration; exact fp32 FMAs, no bf16).  A is symmetric, so
//                      W[r, :] = sum_c A[c, r] V[c, :]: thread tid of a workgroup owns output row r = 256 rb + tid and walks
//                      the rows c of its slab -- the wave reads A[c, r .. r+63] as one coalesced line, V[c, 0..15] is the
//                      same for every lane and comes from LDS as a broadcast.  No cross-lane reduction.  The contraction is
//                      split into slabs of VDR_TOPK_SLAB rows (a constant of the definition, not a launch heuristic), one
//                      workgroup per (problem, row block, slab); the slab partials go to `work`.
//   topk_fold_kernel   W = the slab partials folded in ascending slab order.
//   topk_small_kernel  one workgroup per problem, float64: H = V^T W (symmetrised), the Ritz pairs of H by a cyclic Jacobi
//                      in round-robin order (8 disjoint rotations at a time, at most TK_SWEEPS sweeps), the residuals
//                      ||W y_j - theta_j V y_j||, the convergence test, and the next block: Z_j = W y_j / theta_j rounded to
//                      fp32, G = Z^T Z, Cholesky G = L L^T, V = Z L^-T.  (V^T r_j = 0, so G = I + a positive semi-definite
//                      term: its pivots are >= 1 up to rounding.)  A column whose Ritz value is not above 2^-40 theta_1, or
//                      whose pivot is not above 2^-30 of its diagonal, is dropped (set to zero) for good: that is how a
//                      matrix of rank < 16 and n < 16 are handled.  On convergence, or in the last iteration, it writes
//                      the outputs.  With first != 0 it only builds the start block.
// Row sums of the small kernel: wave w takes the rows r = w (mod 4) ascending, the four wave sums are folded ascending.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vdr_dev.h"
#include "vdr_kernels.h"
#include "../../include/vdr.h"

namespace vdr {
namespace {

constexpr int TK_B = 16;                  // block width
constexpr int TK_SLAB = VDR_TOPK_SLAB;    // rows of the contraction per work item
constexpr int TK_ROWS = 256;              // output rows per work item
constexpr int TK_SWEEPS = 10;             // Jacobi sweeps of the 16 x 16 problem, at most

struct TopkArgs {
  const float* a;  // [P][n][n]
  int n, k, b, nslab, nrb, max_iter;
  float tol;
  float *v, *w, *z, *wpart;  // [P][n][16], [P][n][16], [P][n][16], [P][nslab][n][16]
  int* done;                 // [P]
  float *values, *vectors, *resid;
  int32_t* iters;
};

// the start block: a +-1 pattern from an integer hash of (row, column) and nothing else (include/vdr.h)
VDR_DEV float topk_start(uint32_t row, uint32_t col) {
  uint32_t h = (row * 0x9E3779B1u) ^ (col * 0x85EBCA6Bu);
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  h *= 0x297A2D39u;
  h ^= h >> 15;
  return (h & 1u) ? -1.0f : 1.0f;
}

__global__ __launch_bounds__(256) void topk_av_kernel(TopkArgs t) {
  __shared__ __attribute__((aligned(16))) float sv[TK_SLAB][TK_B];
  int id = blockIdx.x;
  const int slab = id % t.nslab;
  id /= t.nslab;
  const int rb = id % t.nrb, p = id / t.nrb;
  if (t.done[p]) return;  // (uniform)
  const int n = t.n;
  const int c0 = slab * TK_SLAB;
  const int c1 = c0 + TK_SLAB < n ? c0 + TK_SLAB : n;
  const float* v = t.v + ((int64_t)p * n + c0) * TK_B;
  for (int i = threadIdx.x; i < (c1 - c0) * (TK_B / 4); i += 256)
    reinterpret_cast<f32x4*>(&sv[0][0])[i] = reinterpret_cast<const f32x4*>(v)[i];
  __syncthreads();
  const int r = rb * TK_ROWS + threadIdx.x;
  const int rc = r < n ? r : n - 1;  // (rows past n read row n - 1 and are not stored)
  const float* a = t.a + (int64_t)p * n * n + rc;
  float acc[TK_B];
#pragma unroll
  for (int j = 0; j < TK_B; ++j) acc[j] = 0.0f;
  int c = c0;
  for (; c + 8 <= c1; c += 8) {
    float av[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) av[q] = a[(int64_t)(c + q) * n];
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int j = 0; j < TK_B; ++j) acc[j] = fmaf(av[q], sv[c - c0 + q][j], acc[j]);
  }
  for (; c < c1; ++c) {
    const float av = a[(int64_t)c * n];
#pragma unroll
    for (int j = 0; j < TK_B; ++j) acc[j] = fmaf(av, sv[c - c0][j], acc[j]);
  }
  if (r < n) {
    float* dst = t.wpart + (((int64_t)p * t.nslab + slab) * n + r) * TK_B;
#pragma unroll
    for (int q = 0; q < 4; ++q) reinterpret_cast<f32x4*>(dst)[q] = f32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
  }
}

__global__ __launch_bounds__(256) void topk_fold_kernel(TopkArgs t, int problems) {
  const int64_t per = (int64_t)t.n * (TK_B / 4);
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= per * problems) return;
  const int64_t p = idx / per, e = idx - p * per;
  if (t.done[p]) return;
  const f32x4* src = reinterpret_cast<const f32x4*>(t.wpart) + p * t.nslab * per + e;
  f32x4 sum = src[0];
  for (int s = 1; s < t.nslab; ++s) sum += src[(int64_t)s * per];
  reinterpret_cast<f32x4*>(t.w)[idx] = sum;
}

// S = X^T Y over the n rows, [16][16] float64 into LDS `out`; `tmp` holds the four wave sums.  Lane l of a wave owns the
// entries (i = l >> 2, j = 4 (l & 3) .. + 3).
VDR_DEV void topk_xty(const float* x, const float* y, int n, double (*tmp)[TK_B][TK_B], double (*out)[TK_B]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane >> 2, j0 = 4 * (lane & 3);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r = wave; r < n; r += 4) {
    const double xv = (double)x[(int64_t)r * TK_B + i];
    const f32x4 yv = *reinterpret_cast<const f32x4*>(y + (int64_t)r * TK_B + j0);
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = fma(xv, (double)yv[q], s[q]);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) tmp[wave][i][j0 + q] = s[q];
  __syncthreads();
  {
    const int ii = threadIdx.x >> 4, jj = threadIdx.x & 15;
    out[ii][jj] = ((tmp[0][ii][jj] + tmp[1][ii][jj]) + tmp[2][ii][jj]) + tmp[3][ii][jj];
  }
  __syncthreads();
}

// partner of index i in step `step` (0..14) of the round-robin order of 16 players: 15 stays, the rest rotate
VDR_DEV int topk_partner(int i, int step) {
  if (i == 15) return step;
  if (i == step) return 15;
  return (2 * step - i + 30) % 15;
}

__global__ __launch_bounds__(256) void topk_small_kernel(TopkArgs t, int it, int first) {
  __shared__ double tmp[4][TK_B][TK_B];
  __shared__ double H[TK_B][TK_B], Y[TK_B][TK_B], T1[TK_B][TK_B], T2[TK_B][TK_B];
  __shared__ double red[256];
  __shared__ double theta[TK_B], rs[TK_B], inv_scale[TK_B];
  __shared__ double cs[TK_B][2];
  __shared__ int order[TK_B], live[TK_B];
  __shared__ int s_flag;
  const int p = blockIdx.x, tid = threadIdx.x, n = t.n, k = t.k;
  if (t.done[p]) return;  // (uniform)
  float* V = t.v + (int64_t)p * n * TK_B;
  float* W = t.w + (int64_t)p * n * TK_B;
  float* Z = t.z + (int64_t)p * n * TK_B;
  const int i = tid >> 4, j = tid & 15;

  if (first) {
    // start block: the identity for n <= 16 (one step is then the whole problem), the hashed +-1 pattern otherwise
    for (int e = tid; e < n * TK_B; e += 256) {
      const int r = e >> 4, c = e & 15;
      Z[e] = c >= t.b ? 0.0f : n <= TK_B ? (r == c ? 1.0f : 0.0f) : topk_start((uint32_t)r, (uint32_t)c);
    }
    __syncthreads();
  } else {
    // ---- Rayleigh-Ritz: H = V^T W, symmetrised
    topk_xty(V, W, n, tmp, T1);
    H[i][j] = 0.5 * (T1[i][j] + T1[j][i]);
    Y[i][j] = i == j ? 1.0 : 0.0;
    __syncthreads();
    // ---- cyclic Jacobi, round-robin order: H <- J^T H J, Y <- Y J with J the 8 disjoint rotations of the step
    for (int sweep = 0; sweep < TK_SWEEPS; ++sweep) {
      // done once a sweep has left no off-diagonal entry above 2^-52 of the largest diagonal one (from the second
      // iteration on V is last iteration's Ritz basis and H is nearly diagonal to begin with)
      red[tid] = i == j ? 0.0 : fabs(H[i][j]);
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
        __syncthreads();
      }
      double dmax = 0.0;
      for (int q = 0; q < TK_B; ++q) dmax = fmax(dmax, fabs(H[q][q]));
      const bool diagonal = red[0] <= dmax * 0x1p-52;
      __syncthreads();
      if (diagonal) break;  // (uniform)
      for (int step = 0; step < 15; ++step) {
        if (tid < TK_B) {
          const int q = topk_partner(tid, step);
          const int lo = tid < q ? tid : q, hi = tid < q ? q : tid;
          const double apq = H[lo][hi], app = H[lo][lo], aqq = H[hi][hi];
          double c = 1.0, s = 0.0;
          if (fabs(apq) > 1e-300 && fabs(apq) > 1e-40 * (fabs(app) + fabs(aqq))) {
            const double tau = (aqq - app) / (2.0 * apq);
            const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + tt * tt);
            s = tt * c;
          }
          // column lo' = c lo - s hi, column hi' = s lo + c hi: as seen from this index
          cs[tid][0] = c;
          cs[tid][1] = tid == lo ? -s : s;
        }
        __syncthreads();
        {
          const int q = topk_partner(j, step);
          const double c = cs[j][0], s = cs[j][1];
          T1[i][j] = c * H[i][j] + s * H[i][q];
          T2[i][j] = c * Y[i][j] + s * Y[i][q];
        }
        __syncthreads();
        {
          const int q = topk_partner(i, step);
          const double c = cs[i][0], s = cs[i][1];
          H[i][j] = c * T1[i][j] + s * T1[q][j];
          Y[i][j] = T2[i][j];
        }
        __syncthreads();
      }
    }
    // ---- descending order of the Ritz values; the dropped columns (zero rows of H: Ritz value 0, vector e_j) go last
    if (tid < TK_B) theta[tid] = H[tid][tid];
    __syncthreads();
    if (tid < TK_B) {
      int rank = 0;
      for (int q = 0; q < TK_B; ++q) rank += theta[q] > theta[tid] || (theta[q] == theta[tid] && q < tid);
      order[rank] = tid;
    }
    __syncthreads();
    if (tid < TK_B) {
      const double th1 = theta[order[0]];
      const double th = theta[order[tid]];
      live[tid] = th > 0.0 && th > th1 * 0x1p-40;
      inv_scale[tid] = live[tid] ? 1.0 / th : 0.0;
    }
    __syncthreads();
    // ---- per row: V y_c, W y_c (Ritz order); residual sums; Z_c = W y_c / theta_c.  Thread (row lane tid >> 2, column
    // group cg = tid & 3) takes rows row lane, + 64, ... ascending and the Ritz columns 4 cg .. 4 cg + 3.
    {
      const int cg = tid & 3;
      double racc[4] = {0.0, 0.0, 0.0, 0.0};
      for (int r = tid >> 2; r < n; r += 64) {
        float vr[TK_B], wr[TK_B];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 a = reinterpret_cast<const f32x4*>(V + (int64_t)r * TK_B)[q];
          const f32x4 b = reinterpret_cast<const f32x4*>(W + (int64_t)r * TK_B)[q];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            vr[4 * q + e] = a[e];
            wr[4 * q + e] = b[e];
          }
        }
        f32x4 zr;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = 4 * cg + q, oc = order[c];
          double vy = 0.0, wy = 0.0;
#pragma unroll
          for (int m = 0; m < TK_B; ++m) {
            vy = fma((double)vr[m], Y[m][oc], vy);
            wy = fma((double)wr[m], Y[m][oc], wy);
          }
          const double res = wy - theta[oc] * vy;
          racc[q] = fma(res, res, racc[q]);
          zr[q] = (float)(wy * inv_scale[c]);
        }
        *reinterpret_cast<f32x4*>(Z + (int64_t)r * TK_B + 4 * cg) = zr;
      }
      // residual norms: a fixed binary tree over the 64 row lanes of each column group
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        __syncthreads();
        red[tid] = racc[q];
        __syncthreads();
        for (int o = 128; o >= 4; o >>= 1) {
          if (tid < o) red[tid] += red[tid + o];
          __syncthreads();
        }
        if (tid < 4) rs[4 * tid + q] = sqrt(red[tid]);
      }
    }
    __syncthreads();
    // ---- the test: the k leading residuals against tol * theta_1
    if (tid == 0) {
      const double th1 = theta[order[0]];
      double worst = 0.0;
      for (int c = 0; c < k; ++c) worst = rs[c] > worst ? rs[c] : worst;
      const bool conv = worst <= (double)t.tol * th1;
      s_flag = conv || it + 1 >= t.max_iter;
      if (s_flag) {
        t.resid[p] = th1 > 0.0 ? (float)(worst / th1) : 0.0f;
        t.iters[p] = it + 1;
        for (int c = 0; c < k; ++c) t.values[(int64_t)p * k + c] = (float)theta[order[c]];
      }
    }
    __syncthreads();
    if (s_flag) {
      // ---- outputs: x_c = V y_c normalised in float64, largest-magnitude entry positive (lowest index on a tie)
      for (int c = 0; c < k; ++c) {
        const int oc = order[c];
        double ss = 0.0;
        for (int r = tid; r < n; r += 256) {
          double vy = 0.0;
#pragma unroll
          for (int m = 0; m < TK_B; ++m) vy = fma((double)V[(int64_t)r * TK_B + m], Y[m][oc], vy);
          ss = fma(vy, vy, ss);
        }
        __syncthreads();
        red[tid] = ss;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
          if (tid < o) red[tid] += red[tid + o];
          __syncthreads();
        }
        const double norm = sqrt(red[0]);
        __syncthreads();
        float* out = t.vectors + ((int64_t)p * k + c) * n;
        float best = -1.0f;
        int besti = INT32_MAX;
        for (int r = tid; r < n; r += 256) {
          double vy = 0.0;
#pragma unroll
          for (int m = 0; m < TK_B; ++m) vy = fma((double)V[(int64_t)r * TK_B + m], Y[m][oc], vy);
          const float f = norm > 0.0 ? (float)(vy / norm) : 0.0f;
          out[r] = f;
          if (fabsf(f) > best) {  // (ascending r: a strict > keeps the lowest index)
            best = fabsf(f);
            besti = r;
          }
        }
        // arg max over the threads: (value, then lower index) is a total order, any tree gives the same answer
        float* redf = reinterpret_cast<float*>(red);
        int* redi = reinterpret_cast<int*>(red) + 256;
        redf[tid] = best;
        redi[tid] = besti;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
          if (tid < o) {
            const float ov = redf[tid + o];
            const int oi = redi[tid + o];
            if (ov > redf[tid] || (ov == redf[tid] && oi < redi[tid])) {
              redf[tid] = ov;
              redi[tid] = oi;
            }
          }
          __syncthreads();
        }
        const int at = redi[0];
        __syncthreads();
        const bool flip = at != INT32_MAX && out[at] < 0.0f;  // (every thread reads the value its owner wrote before the barriers)
        __syncthreads();
        if (flip)
          for (int r = tid; r < n; r += 256) out[r] = -out[r];
        __syncthreads();
      }
      if (tid == 0) t.done[p] = 1;
      return;
    }
  }

  // ---- orthonormalise Z into V: G = Z^T Z, Cholesky with dropped columns, V = Z L^-T
  __syncthreads();
  topk_xty(Z, Z, n, tmp, T1);
  H[i][j] = 0.5 * (T1[i][j] + T1[j][i]);  // G
  T2[i][j] = 0.0;                          // L (lower), its diagonal holds 1 / L_jj; a dropped column stays all zero
  __syncthreads();
  for (int c = 0; c < TK_B; ++c) {
    if (tid == 0) {
      double d = H[c][c];
      for (int m = 0; m < c; ++m) d -= T2[c][m] * T2[c][m];
      const bool ok = H[c][c] > 0.0 && d > H[c][c] * 0x1p-30;
      live[c] = ok;
      theta[c] = ok ? sqrt(d) : 0.0;  // L_cc
    }
    __syncthreads();
    if (tid > c && tid < TK_B && live[c]) {
      double s = H[tid][c];
      for (int m = 0; m < c; ++m) s -= T2[tid][m] * T2[c][m];
      T2[tid][c] = s / theta[c];
    }
    __syncthreads();
  }
  for (int r = tid; r < n; r += 256) {
    float zr[TK_B];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 a = reinterpret_cast<const f32x4*>(Z + (int64_t)r * TK_B)[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) zr[4 * q + e] = a[e];
    }
    double x[TK_B];
    float xo[TK_B];
#pragma unroll
    for (int c = 0; c < TK_B; ++c) {
      double s = (double)zr[c];
#pragma unroll
      for (int m = 0; m < TK_B; ++m)
        if (m < c) s -= x[m] * T2[c][m];
      x[c] = live[c] ? s / theta[c] : 0.0;
      xo[c] = (float)x[c];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      reinterpret_cast<f32x4*>(V + (int64_t)r * TK_B)[q] = f32x4{xo[4 * q], xo[4 * q + 1], xo[4 * q + 2], xo[4 * q + 3]};
  }
}

// the sections of `work`, in 4-byte elements, each a multiple of 4 (16-byte aligned)
struct TopkLayout {
  int64_t nslab, block, v, w, z, wpart, done;
};
TopkLayout topk_layout(int problems, int n) {
  TopkLayout l;
  l.nslab = (n + TK_SLAB - 1) / TK_SLAB;
  l.block = (int64_t)problems * n * TK_B;
  l.v = 0;
  l.w = l.block;
  l.z = 2 * l.block;
  l.wpart = 3 * l.block;
  l.done = l.wpart + l.nslab * l.block;
  return l;
}

}  // namespace

size_t sym_topk_work_bytes(int problems, int n) {
  if (problems <= 0 || n <= 0) return 0;
  const TopkLayout l = topk_layout(problems, n);
  return (size_t)((l.done + ((problems + 3) & ~3)) * 4);
}

hipError_t launch_sym_topk(const float* a, int problems, int n, int k, float tol, int max_iter, void* work, float* values,
                           float* vectors, int32_t* iters, float* resid, hipStream_t st) {
  if (!a || !work || !values || !vectors || !iters || !resid || problems <= 0 || n < 2 || n > 4096 || k < 1 || k > 8 || k > n ||
      max_iter < 1 || !(tol >= 0.0f))
    return hipErrorInvalidValue;
  if ((((uintptr_t)a | (uintptr_t)work) & 15)) return hipErrorInvalidValue;
  const TopkLayout l = topk_layout(problems, n);
  TopkArgs t;
  t.a = a;
  t.n = n, t.k = k, t.b = n < TK_B ? n : TK_B, t.max_iter = max_iter, t.tol = tol;
  t.nslab = (int)l.nslab;
  t.nrb = (n + TK_ROWS - 1) / TK_ROWS;
  float* w = (float*)work;
  t.v = w + l.v, t.w = w + l.w, t.z = w + l.z, t.wpart = w + l.wpart;
  t.done = (int*)(w + l.done);
  t.values = values, t.vectors = vectors, t.resid = resid, t.iters = iters;
  const int64_t av = (int64_t)problems * t.nrb * t.nslab;
  const int64_t fold = ((int64_t)problems * n * (TK_B / 4) + 255) / 256;
  if (av > INT32_MAX || fold > INT32_MAX) return hipErrorInvalidValue;
  if (hipError_t e = hipMemsetAsync(t.done, 0, (size_t)problems * 4, st)) return e;
  hipLaunchKernelGGL(topk_small_kernel, dim3((unsigned)problems), dim3(256), 0, st, t, -1, 1);
  if (hipError_t e = hipGetLastError()) return e;
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(topk_av_kernel, dim3((unsigned)av), dim3(256), 0, st, t);
    hipLaunchKernelGGL(topk_fold_kernel, dim3((unsigned)fold), dim3(256), 0, st, t, problems);
    hipLaunchKernelGGL(topk_small_kernel, dim3((unsigned)problems), dim3(256), 0, st, t, it, 0);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

}  // namespace vdr
