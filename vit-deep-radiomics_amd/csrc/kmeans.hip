// Lloyd's k-means over bf16 descriptor maps for gfx950 (include/vdr.h: vdr_op_kmeans_assign, vdr_op_kmeans_update).
// Operand of both: `problems` problems of `imgs` images of t rows of d bf16 channels, rows ld elements apart, images
// image_stride apart, problems problem_stride apart (0: one map under many sets of centroids); R = imgs * t rows per problem.
//
// Tile, accumulator layout, LDS images, the register-staged pipeline and every reduction: desc_tile.h.
//   assign   km_norms_kernel    xx of every row and cc of every centroid into `work` (row_sumsq: one wave per row).
//            km_assign_kernel   256 threads; one work item = (problem, 128-row panel of X).  It walks the 128-centroid tiles;
//                               per tile a loop over d in steps of 64 stages three "t128" images: the panel's X rows, c_hi
//                               and c_lo of the tile's centroids -- split from the fp32 values in the staging pass itself, so
//                               the operands go through registers, not the LDS-DMA.  X is the A operand, the centroids the B
//                               operand, so a lane holds ONE centroid j and 16 rows i.  Epilogue per tile, in that layout:
//                               h = cc_j - 2 s, centroids past k masked, every element folded into the lane's running row
//                               best (kept across the tiles).  At the end of the item the row best is reduced (its own copy of
//                               row_best_reduce); label, min_dist and a changed flag per row are written.  The R x k matrix is never written.
//            km_assign_finish_kernel  one workgroup per problem: inertia in col_mean's order, the changed flags counted.
//   update   km_update_kernel   256 threads; one work item = (problem, 128-cluster tile, 128-column tile, chunk of
//                               VDR_KMEANS_CHUNK rows): onehot^T X on the "tr" image.  A thread owns one 16-byte column
//                               chunk of the X tile and the same chunk (8 clusters) of the one-hot image, which it builds in
//                               LDS from the labels of its rows.  The item's partial sums go to `work`.
//            km_update_finish_kernel  one workgroup per (problem, cluster): counts the cluster's rows (integers), folds the
//                               chunk sums ascending and divides once; an empty cluster's centroid is not touched.
// Every kernel returns at once for a problem whose `active` flag is 0.  No atomics anywhere; nothing depends on `problems`,
// on the grid or on a launch heuristic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "desc_tile.h"
#include "vdr_dev.h"
#include "vdr_kernels.h"
#include "../../include/vdr.h"

namespace vdr {
namespace {

constexpr int KM_T = T128;                      // rows of a panel, centroids of a tile
constexpr int KM_CHUNK = VDR_KMEANS_CHUNK;      // rows per chunk of the update: a constant of the definition
constexpr int KM_SUM_CHUNK = VDR_COV_CHUNK;     // rows per chunk of the inertia sum (col_mean's order)
constexpr int KM_ROW = 3 * T128_OPER;           // row exchange: value [2][128], index [2][128]
constexpr int KM_LDS = KM_ROW + 2048;
static_assert(KM_CHUNK % TR_STEP == 0, "a chunk is whole steps");
static_assert(KM_LDS <= 65536, "no opt-in to large dynamic LDS needed");

struct KmArgs {
  const bf16_t* x;
  int64_t ld, is, ps, R;
  int imgs, t, d, k, npanels, ntiles, nchunks, nct;
  const int32_t* active;
  const float* cent;   // [problems][k][d]
  float *xx, *cc;      // scratch [problems][R], [problems][k]
  int32_t* chg;        // scratch [problems][R]
  float* part;         // scratch [problems][nchunks][k][d]
};

VDR_DEV bool km_on(const KmArgs& a, int64_t p) { return !a.active || a.active[p] != 0; }

struct KmBetter {  // lower value, then lower index
  __device__ __forceinline__ bool operator()(float v, int i, float bv, int bi) const { return v < bv || (v == bv && i < bi); }
};

// ---- assign ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void km_norms_kernel(KmArgs a, int problems) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nx = (int64_t)problems * a.R, nc = (int64_t)problems * a.k;
  if (row >= nx + nc) return;
  if (row < nx) {
    const int64_t p = row / a.R, r = row - p * a.R;
    if (!km_on(a, p)) return;
    const float ss = row_sumsq(a.x + desc_row(a, p * a.ps, r), a.d, lane);
    if (lane == 0) a.xx[row] = ss;
  } else {
    const int64_t cr = row - nx, p = cr / a.k;
    if (!km_on(a, p)) return;
    const float ss = row_sumsq(a.cent + cr * a.d, a.d, lane);
    if (lane == 0) a.cc[cr] = ss;
  }
}

__global__ __launch_bounds__(256) void km_assign_kernel(KmArgs a, int32_t* labels, float* min_dist) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int p = blockIdx.x / a.npanels, panel = blockIdx.x - p * a.npanels;
  if (!km_on(a, p)) return;  // (uniform over the workgroup)
  const int nk = (a.d + 63) >> 6;

  // staging role: 16-byte chunk ch of the 64-column step, rows rl, rl + 32, rl + 64, rl + 96 of each image
  const int ch = tid & 7, rl = tid >> 3;
  bool rok[4];
  int64_t roff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t r = (int64_t)panel * KM_T + rl + 32 * j;
    rok[j] = r < a.R;
    roff[j] = rok[j] ? desc_row(a, p * a.ps, r) : 0;
  }

  float rbv[2][16];
  int rbi[2][16];
  f32x16 acc[2][2];
  acc_zero(acc);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      rbv[m][e] = INFINITY;
      rbi[m][e] = INT32_MAX;
    }

  char* sx = smem;
  char* shi = smem + T128_OPER;
  char* slo = smem + 2 * T128_OPER;
  const float* cent = a.cent + (int64_t)p * a.k * a.d;

#pragma clang loop unroll(disable)
  for (int jt = 0; jt < a.ntiles; ++jt) {
    bool cok[4];
    const float* crow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = jt * KM_T + rl + 32 * j;
      cok[j] = c < a.k;
      crow[j] = cent + (int64_t)(cok[j] ? c : 0) * a.d;
    }
    RawChunk<true> rx[4];
    RawChunk<false> rc[4];
    // (a row past R, a centroid past k or a column past d is fetched as zeros and staged as zeros)
    const auto fetch = [&](int step) {
      const int col = step * 64 + ch * 8;
      const bool colok = col < a.d;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        raw_fill(rx[j], rok[j] && colok, a.x, roff[j] + col);
        raw_fill(rc[j], cok[j] && colok, crow[j], col);
      }
    };
    const auto stage = [&](int) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf16x8 h, l;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float c = rc[j].get(e);
          h[e] = (bf16_t)c;
          l[e] = (bf16_t)(c - (float)h[e]);
        }
        const int off = t128_off(rl + 32 * j, ch);
        *reinterpret_cast<bf16x8*>(sx + off) = rx[j].v;
        *reinterpret_cast<bf16x8*>(shi + off) = h;
        *reinterpret_cast<bf16x8*>(slo + off) = l;
      }
    };

    staged_steps(nk, fetch, stage, [&]() { t128_mfma_a2b(sx, shi, slo, wr, wc, l31, hh, acc); });

    // ---- epilogue of tile jt
    float ccv[2];
    int gcol[2];
    bool jok[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      gcol[n] = jt * KM_T + acc_col(wc, n, l31);
      jok[n] = gcol[n] < a.k;
      ccv[n] = jok[n] ? a.cc[(int64_t)p * a.k + gcol[n]] : 0.0f;
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const float h = ccv[n] - 2.0f * acc[m][n][e];
          acc[m][n][e] = 0.0f;
          // (ascending j within the lane: a strict < keeps the lowest index)
          if (jok[n] && h < rbv[m][e]) {
            rbv[m][e] = h;
            rbi[m][e] = gcol[n];
          }
        }
  }

  // ---- row best of the item: row_best_reduce spelled out -- through the helper the whole kernel is scheduled differently and the
  // d = 13056 assign is 1.3 % slower: over the 32 lanes of a half wave, then over the two column waves
  float* s_rowv = reinterpret_cast<float*>(smem + KM_ROW);
  int* s_rowi = reinterpret_cast<int*>(smem + KM_ROW + 1024);
  const KmBetter better;
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
  if (tid < 128) {
    float v = s_rowv[tid];
    int i = s_rowi[tid];
    if (better(s_rowv[128 + tid], s_rowi[128 + tid], v, i)) {
      v = s_rowv[128 + tid];
      i = s_rowi[128 + tid];
    }
    const int64_t r = (int64_t)panel * KM_T + tid;
    if (r < a.R) {
      const int64_t o = (int64_t)p * a.R + r;
      a.chg[o] = labels[o] != i;
      labels[o] = i;
      min_dist[o] = fmaxf(a.xx[o] + v, 0.0f);
    }
  }
}

// inertia[p]: min_dist summed in col_mean's order -- inside a chunk of VDR_COV_CHUNK rows sixteen interleaved sums (rows r,
// r + 16, ... ascending) folded in ascending r, then the chunk sums in ascending chunk order; changed[p]: the flags counted
__global__ __launch_bounds__(256) void km_assign_finish_kernel(KmArgs a, const float* min_dist, float* inertia, int32_t* changed) {
  __shared__ float s_part[16][16];
  __shared__ float s_chunk[16];
  __shared__ int s_cnt[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  if (!km_on(a, p)) return;
  const float* md = min_dist + (int64_t)p * a.R;
  const int32_t* chg = a.chg + (int64_t)p * a.R;
  int cnt = 0;
  for (int64_t r = tid; r < a.R; r += 256) cnt += chg[r];
  const int64_t nchunks = (a.R + KM_SUM_CHUNK - 1) / KM_SUM_CHUNK;
  const int cs = tid >> 4, rl = tid & 15;
  float total = 0.0f;
  for (int64_t c0 = 0; c0 < nchunks; c0 += 16) {
    const int64_t r0 = (c0 + cs) * KM_SUM_CHUNK;
    const int64_t r1 = r0 + KM_SUM_CHUNK < a.R ? r0 + KM_SUM_CHUNK : a.R;
    float sum = 0.0f;
    for (int64_t r = r0 + rl; r < r1; r += 16) sum += md[r];
    __syncthreads();
    s_part[cs][rl] = sum;
    __syncthreads();
    if (tid < 16) s_chunk[tid] = fold_chunks(s_part[tid], 16, 1);
    __syncthreads();
    if (tid == 0) {
      const int n = nchunks - c0 < 16 ? (int)(nchunks - c0) : 16;
      int j = 0;
      if (c0 == 0) total = s_chunk[j++];
      for (; j < n; ++j) total += s_chunk[j];
    }
  }
  cnt = block_reduce_256(s_cnt, tid, cnt, [](int x, int y) { return x + y; });
  if (tid == 0) {
    inertia[p] = total;
    changed[p] = cnt;
  }
}

// ---- update ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void km_update_kernel(KmArgs a, const int32_t* labels) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  int id = blockIdx.x;
  const int chunk = id % a.nchunks;
  id /= a.nchunks;
  const int ct = id % a.nct;
  id /= a.nct;
  const int kt = id % a.ntiles, p = id / a.ntiles;
  if (!km_on(a, p)) return;  // (uniform over the workgroup)

  // staging role: one 16-byte column chunk of the X tile and the same chunk (8 clusters) of the one-hot tile, rows rl, rl + 16,
  // rl + 32, rl + 48 of a step
  const int ch = tid & 15, rl = tid >> 4;
  const int col = ct * 128 + ch * 8;
  const bool cok = col < a.d;
  const int c0 = kt * KM_T + ch * 8;
  const int64_t r0 = (int64_t)chunk * KM_CHUNK;
  const int64_t r1 = r0 + KM_CHUNK < a.R ? r0 + KM_CHUNK : a.R;
  const int nsteps = (int)((r1 - r0 + TR_STEP - 1) / TR_STEP);
  const int32_t* lab = labels + (int64_t)p * a.R;

  RawChunk<true> raw[4];
  int rlab[4];
  // (a row past the chunk has label -1 and zeros: it is in no cluster)
  const auto fetch = [&](int step) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t r = r0 + step * TR_STEP + rl + 16 * j;
      const bool rok = r < r1;
      rlab[j] = rok ? lab[r] : -1;
      raw_fill(raw[j], rok && cok, a.x, desc_row(a, p * a.ps, r) + col);
    }
  };
  const auto stage = [&](int) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x8 oh;
#pragma unroll
      for (int e = 0; e < 8; ++e) oh[e] = (bf16_t)(rlab[j] == c0 + e ? 1.0f : 0.0f);
      const int off = tr_off(rl + 16 * j, ch);
      *reinterpret_cast<bf16x8*>(smem + off) = oh;
      *reinterpret_cast<bf16x8*>(smem + TR_IMG + off) = raw[j].v;
    }
  };

  f32x16 acc[2][2];
  acc_zero(acc);
  const tr_lds_cptr imgA = (tr_lds_cptr)smem;
  const tr_lds_cptr imgB = imgA + TR_IMG;
  // staged_steps spelled out: through the helper this kernel drops to 104 VGPRs and a third wave per SIMD, and a refactor leaves
  // the occupancy as it was
  fetch(0);
#pragma clang loop unroll(disable)
  for (int step = 0; step < nsteps; ++step) {
    __syncthreads();  // every wave has read the previous step
    stage(step);
    __syncthreads();
    if (step + 1 < nsteps) fetch(step + 1);
    tr_mfma(imgA, imgB, wr, wc, lane, acc);
  }

  // the tile's clusters < k and columns < d of part[p][chunk][k][d]
  float* part = a.part + (((int64_t)p * a.nchunks + chunk) * a.k + kt * KM_T) * a.d + ct * 128;
  acc_store<true>(part, a.d, a.k - kt * KM_T, a.d - ct * 128, wr, wc, l31, hh, acc);
}

__global__ __launch_bounds__(256) void km_update_finish_kernel(KmArgs a, const int32_t* labels, float* centroids, int32_t* counts) {
  __shared__ int s_cnt[256];
  const int p = blockIdx.x / a.k, j = blockIdx.x - p * a.k, tid = threadIdx.x;
  if (!km_on(a, p)) return;
  const int32_t* lab = labels + (int64_t)p * a.R;
  int cnt = 0;
  for (int64_t r = tid; r < a.R; r += 256) cnt += lab[r] == j;
  cnt = block_reduce_256(s_cnt, tid, cnt, [](int x, int y) { return x + y; });
  if (tid == 0) counts[(int64_t)p * a.k + j] = cnt;
  if (cnt == 0) return;  // an empty cluster keeps its centroid's bits
  const float n = (float)cnt;
  float* out = centroids + ((int64_t)p * a.k + j) * a.d;
  for (int c = tid; c < a.d; c += 256) {
    out[c] = __fdiv_rn(fold_chunks(a.part + ((int64_t)p * a.nchunks * a.k + j) * a.d + c, a.nchunks, (int64_t)a.k * a.d), n);
  }
}

int64_t km_chunks(int64_t R) { return (R + KM_CHUNK - 1) / KM_CHUNK; }
int64_t km_pad4(int64_t n) { return (n + 3) & ~(int64_t)3; }  // 4-byte elements: every section starts 16-byte aligned

bool km_args(KmArgs& a, const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs, int t,
             int d, int k, const int32_t* active, void* work) {
  if (!x || !work || problems <= 0 || imgs <= 0 || t <= 0 || d <= 0 || (d & 31) || k < 1 || k > 1024 || ld < d || image_stride < 0 ||
      problem_stride < 0)
    return false;
  if ((((uintptr_t)x | (uintptr_t)work) & 15) || ((ld | image_stride | problem_stride) & 7)) return false;
  const int64_t R = (int64_t)imgs * t;
  if (R > INT32_MAX || R * problems > INT32_MAX || k > R) return false;
  a.x = (const bf16_t*)x;
  a.ld = ld, a.is = image_stride, a.ps = problem_stride, a.R = R;
  a.imgs = imgs, a.t = t, a.d = d, a.k = k;
  a.npanels = (int)((R + KM_T - 1) / KM_T);
  a.ntiles = (k + KM_T - 1) / KM_T;
  a.nchunks = (int)km_chunks(R);
  a.nct = (d + 127) / 128;
  a.active = active;
  a.cent = nullptr;
  float* w = (float*)work;
  a.xx = w;
  a.cc = a.xx + km_pad4((int64_t)problems * R);
  a.chg = (int32_t*)(a.cc + km_pad4((int64_t)problems * k));
  a.part = w;  // (the update's partial sums overlay the assign's sections: each op writes what it reads)
  return true;
}

}  // namespace

size_t kmeans_work_bytes(int problems, int imgs, int t, int d, int k) {
  if (problems <= 0 || imgs <= 0 || t <= 0 || d <= 0 || k <= 0) return 0;
  const int64_t R = (int64_t)imgs * t;
  const int64_t assign = 2 * km_pad4((int64_t)problems * R) + km_pad4((int64_t)problems * k);
  const int64_t update = (int64_t)problems * km_chunks(R) * k * d;
  return (size_t)(km_pad4(assign > update ? assign : update) * 4);
}

hipError_t launch_kmeans_assign(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs,
                                int t, int d, int k, const float* centroids, const int32_t* active, void* work, int32_t* labels,
                                float* min_dist, float* inertia, int32_t* changed, hipStream_t st) {
  KmArgs a;
  if (!centroids || !labels || !min_dist || !inertia || !changed || ((uintptr_t)centroids & 15) ||
      !km_args(a, x, ld, image_stride, problem_stride, problems, imgs, t, d, k, active, work))
    return hipErrorInvalidValue;
  a.cent = centroids;
  const int64_t rows = (int64_t)problems * a.R + (int64_t)problems * k;
  const int64_t items = (int64_t)problems * a.npanels;
  if (items > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(km_norms_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a, problems);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(km_assign_kernel, dim3((unsigned)items), dim3(256), KM_LDS, st, a, labels, min_dist);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(km_assign_finish_kernel, dim3((unsigned)problems), dim3(256), 0, st, a, min_dist, inertia, changed);
  return hipGetLastError();
}

hipError_t launch_kmeans_update(const void* x, int64_t ld, int64_t image_stride, int64_t problem_stride, int problems, int imgs,
                                int t, int d, int k, const int32_t* labels, const int32_t* active, void* work, float* centroids,
                                int32_t* counts, hipStream_t st) {
  KmArgs a;
  if (!labels || !centroids || !counts || !km_args(a, x, ld, image_stride, problem_stride, problems, imgs, t, d, k, active, work))
    return hipErrorInvalidValue;
  const int64_t items = (int64_t)problems * a.ntiles * a.nct * a.nchunks, fin = (int64_t)problems * k;
  if (items > INT32_MAX || fin > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(km_update_kernel, dim3((unsigned)items), dim3(256), 2 * TR_IMG, st, a, labels);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(km_update_finish_kernel, dim3((unsigned)fin), dim3(256), 0, st, a, labels, centroids, counts);
  return hipGetLastError();
}

}  // namespace vdr
