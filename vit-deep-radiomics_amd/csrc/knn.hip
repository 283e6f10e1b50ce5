// k nearest neighbours between two descriptor maps for gfx950 (include/vdr.h, vdr_op_knn): for `pairs` problems of queries
// X_p [tq, d] and candidates Y_p [tc, d] (bf16 rows ldx / ldy elements apart, pairs x_stride / y_stride apart, 0 allowed)
//   cosine  s(i, j) = (dot(x_i, y_j) * rn(x_i)) * rn(y_j)                   better: greater, then lower j   (nn_cosine's bits)
//   l2      s(i, j) = fmaxf(fmaf(-2, dot(x_i, y_j), ss(x_i) + ss(y_j)), 0)  better: smaller, then lower j
// and the k best eligible candidates of every query, best first, as val / idx [pairs][tq][k].  The tq x tc score matrix is
// never written: it exists one 128 x 128 tile at a time in MFMA accumulators.  Inside the kernels a score is a KEY, lower is
// better: -s for cosine, s for l2; one comparison serves both metrics.
//
// Three launches, no atomics; every index they form comes from knn_map.h, which tests/knn_map_cases.cpp walks on the host:
//   cosine_rnorm_kernel  (nn_cosine.hip) rn of every row, or knn_sumsq_kernel, its copy that stores ss (l2), into `work`.
//   knn_kernel<KL, L2>   256 threads; one work item = (pair, run of candidate tiles, 128-query panel).  dma_steps /
//                        t128_dma_stage of desc_tile.h with the CANDIDATES as the A operand and the queries as the B operand:
//                        a lane holds ONE query per accumulator column n and meets 32 candidates of it per tile, in ascending
//                        index order over the whole run.  Per query it keeps a sorted list of KL = 4 / 8 / 16 (key, index)
//                        pairs in registers.  The first KL - k places hold (-inf, -1), which nothing beats, so the entry to
//                        beat is always the statically indexed list[KL - 1]: no register array is indexed by k.
//                        Because the lane's candidates ascend, `<` on the key alone keeps equal keys in index order.  A
//                        candidate past tc or on the excluded diagonal gets the key +inf and never enters.  At the end of the
//                        item the last k places go to the partial lists of (query, run, sub = 2 wr + hh): four lists per query
//                        and run, merged later.  The lists never touch LDS, so no LDS region is both a staging buffer and a
//                        merge buffer; the only LDS besides the two staging buffers holds the tile's norms.
//   knn_finish_kernel    four threads per query: thread g folds the partial lists g, g + 4, ... of the 4 nsplit into a list of KL
//                        with the FULL comparator (key, then index), a list's k entries loaded together; the four lists are
//                        then folded pairwise through shuffles, and thread 0 writes val / idx.
// The comparator is a total order on pairs with distinct indices, so the k best of a union are the k best of the k best of its
// parts: the bits depend on (tq, tc, d, k, inputs), not on the run split, `pairs` or the problem's position.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "desc_tile.h"
#include "knn_map.h"
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {
namespace {

static_assert(KNN_TILE == T128 && KNN_TARGET_ITEMS == COS_TARGET_ITEMS, "knn_map.h restates desc_tile.h");
constexpr int KNN_RN = 4 * T128_OPER;  // s_rn [2][256] float: tile parity x (norms of the tile's candidates | of the panel's queries)
constexpr int KNN_LDS = KNN_RN + 2048;
constexpr int KNN_NONE = INT32_MAX;    // the index of an empty place: loses every tie

struct KnnArgs {
  const bf16_t *x, *y;
  int64_t ldx, xs, ldy, ys;
  KnnPlan pl;
  int d, exclude_diag, l2;
  float *nq, *nc;  // [pairs][tq_pad], [pairs][tc_pad]: rn (cosine) or ss (l2)
  float* pkey;     // knn_part_off
  int32_t* pidx;
};

// ss of every row of X and Y: cosine_rnorm_kernel (nn_cosine.hip) without the rn
__global__ __launch_bounds__(256) void knn_sumsq_kernel(CosSide X, CosSide Y, int d, int pairs) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nx = (int64_t)pairs * X.t;
  if (row >= nx + (int64_t)pairs * Y.t) return;
  const CosSide s = row < nx ? X : Y;
  const int64_t r = row < nx ? row : row - nx;
  const int p = (int)(r / s.t);
  const int i = (int)(r - (int64_t)p * s.t);
  const float ss = row_sumsq((const bf16_t*)s.x + knn_row_off(p, s.ps, i, s.ld), d, lane);
  if (lane == 0) s.rn[knn_norm_off(p, s.t_pad, 0, i)] = ss;
}

// (key, index) into a sorted list whose last place it beats: it takes that place and moves up past every worse key.
// FULL: ties by the lower index (the merges); otherwise the caller feeds ascending indices and `<` on the key is enough.
template <int KL, bool FULL>
VDR_DEV void knn_insert(float (&lk)[KL], int (&li)[KL], float key, int id) {
  lk[KL - 1] = key;
  li[KL - 1] = id;
#pragma unroll
  for (int i = KL - 1; i > 0; --i) {
    const bool up = lk[i] < lk[i - 1] || (FULL && lk[i] == lk[i - 1] && li[i] < li[i - 1]);
    const float tk = up ? lk[i - 1] : lk[i];
    const int ti = up ? li[i - 1] : li[i];
    lk[i - 1] = up ? lk[i] : lk[i - 1];
    li[i - 1] = up ? li[i] : li[i - 1];
    lk[i] = tk;
    li[i] = ti;
  }
}
// the empty list of k places: KL - k unbeatable ones in front, k that everything beats behind
template <int KL>
VDR_DEV void knn_list_init(float (&lk)[KL], int (&li)[KL], int k) {
  asm volatile("" : "+v"(k));  // (a per-lane value: as a uniform one the KL conditions are kept as SGPR masks and spilled)
#pragma unroll
  for (int i = 0; i < KL; ++i) {
    lk[i] = i < KL - k ? -INFINITY : INFINITY;
    li[i] = i < KL - k ? -1 : KNN_NONE;
  }
}

template <int KL, bool L2>
__global__ __launch_bounds__(256, 2) void knn_kernel(KnnArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  // (pair, run, panel), panel fastest, in XCD-contiguous order: the panels that read the same candidate tiles meet in one L2
  const KnnItem it = knn_item(a.pl, blockIdx.x, gridDim.x);
  int jt0, jt1;
  knn_run(a.pl, it.split, jt0, jt1);
  const bf16_t* xp = a.x + knn_row_off(it.p, a.xs, 0, a.ldx);
  const bf16_t* yp = a.y + knn_row_off(it.p, a.ys, 0, a.ldy);
  const float* s_rn = reinterpret_cast<const float*>(smem + KNN_RN);

  // the panel's rows this lane stages, fixed over the item (element offsets of clamped rows)
  int64_t qo[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) qo[q] = knn_row_off(0, 0, knn_src_row(it.panel, t128_dma_row(wave, lane, q), a.pl.tq), a.ldx);

  float lk[2][KL];
  int li[2][KL];
#pragma unroll
  for (int n = 0; n < 2; ++n) knn_list_init<KL>(lk[n], li[n], a.pl.k);
  f32x16 acc[2][2];
  acc_zero(acc);

  dma_steps(
      jt0, jt1, a.d, smem, wr, wc, l31, hh, acc,
      [&](int jt, int kk, char* sx) {
        int64_t co[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) co[q] = knn_row_off(0, 0, knn_src_row(jt, t128_dma_row(wave, lane, q), a.pl.tc), a.ldy);
        t128_dma_stage(yp, xp, co, qo, a.d, kk, sx, wave, lane);
        if (kk == 0 && wave == 0) {  // the tile's norms ride on the same wait: lanes 0..31 the candidates', 32..63 the panel's
          const float* src = lane < 32 ? a.nc + knn_norm_off(it.p, a.pl.tc_pad, jt, lane * 4)
                                       : a.nq + knn_norm_off(it.p, a.pl.tq_pad, it.panel, (lane - 32) * 4);
          glds16_raw(src, smem + KNN_RN + (jt & 1) * 1024);
        }
      },
      [&](int jt) {
        // ---- epilogue of tile jt: this lane's two queries against its 32 candidates, in ascending candidate order
        const float* rn = s_rn + (jt & 1) * 256;
        float nqv[2];
        // candidates this lane may count, as (constant < / != per-lane value) with the values made opaque: written on the
        // global row the 32 lane masks are loop invariants that hipcc keeps in SGPR pairs (nn_cosine.hip, mask_keys)
        int rthr = a.pl.tc - jt * KNN_TILE - wr * 64 - 4 * hh;
        asm volatile("" : "+v"(rthr));
        int diag[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int col = acc_col(wc, n, l31);
          nqv[n] = rn[128 + col];
          diag[n] = a.exclude_diag ? it.panel * KNN_TILE + col - jt * KNN_TILE - wr * 64 - 4 * hh : -1;
          asm volatile("" : "+v"(diag[n]));
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int r0 = acc_row(0, m, e, 0);
            const int rloc = acc_row(wr, m, e, hh);
            const float ncv = rn[rloc];
            const int gc = jt * KNN_TILE + rloc;
#pragma unroll
            for (int n = 0; n < 2; ++n) {
              const float dot = acc[m][n][e];
              acc[m][n][e] = 0.0f;
              // (l2: + 0.0f turns a -0 of the clamp into +0; cosine: the key is -s, negated back at the output)
              const float key = L2 ? fmaxf(fmaf(-2.0f, dot, nqv[n] + ncv), 0.0f) + 0.0f : -((dot * nqv[n]) * ncv);
              const bool ok = r0 < rthr && r0 != diag[n];
              const float kk = ok ? key : INFINITY;
              if (kk < lk[n][KL - 1]) knn_insert<KL, false>(lk[n], li[n], kk, gc);
            }
          }
      });

  // ---- the item's four lists per query: the last k places, best first; one writer per (query, run, sub, slot)
  const int sub = 2 * wr + hh;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int gq = it.panel * KNN_TILE + acc_col(wc, n, l31);
    int first = KL - a.pl.k;
    asm volatile("" : "+v"(first));  // (as in knn_list_init)
    if (gq < a.pl.tq) {
#pragma unroll
      for (int i = 0; i < KL; ++i)
        if (i >= first) {
          const long long o = knn_part_off(a.pl, it.p, it.split, sub, i - first, gq);
          a.pkey[o] = lk[n][i];
          a.pidx[o] = li[n][i];
        }
    }
  }
}

// (key, index) beats the list's last place: the full comparator
template <int KL>
VDR_DEV bool knn_enters(const float (&lk)[KL], const int (&li)[KL], float key, int id) {
  return key < lk[KL - 1] || (key == lk[KL - 1] && id < li[KL - 1]);
}

constexpr int KNN_MERGE = 4;  // threads per query in the merge (a power of two, lanes next to each other)

template <int KL>
__global__ __launch_bounds__(256) void knn_finish_kernel(KnnArgs a, float* val, int32_t* idx) {
  const int64_t rows = (int64_t)a.pl.pairs * a.pl.tq;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int g = (int)(t & (KNN_MERGE - 1));
  // a group past the end repeats the last query -- every lane takes part in the shuffles -- and stores nothing
  const bool live = t / KNN_MERGE < rows;
  const int64_t row = live ? t / KNN_MERGE : rows - 1;
  const int p = (int)(row / a.pl.tq), q = (int)(row - (int64_t)p * a.pl.tq);
  int first = KL - a.pl.k;
  asm volatile("" : "+v"(first));  // (as in knn_list_init)
  float lk[KL];
  int li[KL];
  knn_list_init<KL>(lk, li, a.pl.k);
  // thread g folds the partial lists g, g + 4, ...: a list's k entries are loaded together (one latency per list, not per
  // entry); the places past k hold what never enters
  for (int l = g; l < a.pl.nsplit * KNN_SUBS; l += KNN_MERGE) {
    float ek[KL];
    int ei[KL];
#pragma unroll
    for (int s = 0; s < KL; ++s) {
      ek[s] = INFINITY;
      ei[s] = KNN_NONE;
      if (s < a.pl.k) {
        const long long o = knn_part_off(a.pl, p, l / KNN_SUBS, l % KNN_SUBS, s, q);
        ek[s] = a.pkey[o];
        ei[s] = a.pidx[o];
      }
    }
#pragma unroll
    for (int s = 0; s < KL; ++s)
      if (knn_enters<KL>(lk, li, ek[s], ei[s])) knn_insert<KL, true>(lk, li, ek[s], ei[s]);
  }
  // the group's lists folded pairwise: both partners take a copy of the other's list, then insert its last k places.  The
  // lists of two partners hold distinct candidates, and the order is total, so both end with the same list.
#pragma clang loop unroll(disable)
  for (int o = 1; o < KNN_MERGE; o <<= 1) {
    float ek[KL];
    int ei[KL];
#pragma unroll
    for (int i = 0; i < KL; ++i) {
      ek[i] = __shfl_xor(lk[i], o, 64);
      ei[i] = __shfl_xor(li[i], o, 64);
    }
#pragma unroll
    for (int i = 0; i < KL; ++i)
      if (i >= first && knn_enters<KL>(lk, li, ek[i], ei[i])) knn_insert<KL, true>(lk, li, ek[i], ei[i]);
  }
  if (live && g == 0) {
#pragma unroll
    for (int i = 0; i < KL; ++i)
      if (i >= first) {
        const long long o = knn_out_off(a.pl, p, q, i - first);
        val[o] = a.l2 ? lk[i] : -lk[i];
        idx[o] = li[i];
      }
  }
}

template <int KL>
hipError_t knn_launch(const KnnArgs& a, float* val, int32_t* idx, hipStream_t st) {
  static KernelState ks[2];
  const int dev = current_device_index();
  if (dev < 0) return hipErrorInvalidDevice;
  const void* fn = a.l2 ? (const void*)knn_kernel<KL, true> : (const void*)knn_kernel<KL, false>;
  if (hipError_t e = raise_lds_limit(ks[a.l2], fn, dev, KNN_LDS)) return e;
  if (a.l2) hipLaunchKernelGGL((knn_kernel<KL, true>), dim3((unsigned)a.pl.items), dim3(256), KNN_LDS, st, a);
  else hipLaunchKernelGGL((knn_kernel<KL, false>), dim3((unsigned)a.pl.items), dim3(256), KNN_LDS, st, a);
  if (hipError_t e = hipGetLastError()) return e;
  const int64_t rows = (int64_t)a.pl.pairs * a.pl.tq;
  hipLaunchKernelGGL((knn_finish_kernel<KL>), dim3((unsigned)((rows * KNN_MERGE + 255) / 256)), dim3(256), 0, st, a, val, idx);
  return hipGetLastError();
}

}  // namespace

size_t knn_work_bytes(int pairs, int tq, int tc, int k) {
  if (pairs <= 0 || tq <= 0 || tc <= 0 || k < 1 || k > KNN_MAX_K) return 0;
  return (size_t)knn_work_elems(pairs, tq, tc, k) * 4;
}

hipError_t launch_knn(const void* x, int64_t ldx, int64_t x_stride, int tq, const void* y, int64_t ldy, int64_t y_stride, int tc,
                      int pairs, int d, int k, int l2, int exclude_diag, void* work, float* val, int32_t* idx, hipStream_t st) {
  if (!cos_operand_ok(x, ldx, x_stride, tq, d) || !cos_operand_ok(y, ldy, y_stride, tc, d) || !work || ((uintptr_t)work & 15) || !val ||
      !idx || pairs <= 0 || k < 1 || k > KNN_MAX_K || (int64_t)tc - (exclude_diag ? 1 : 0) < k)
    return hipErrorInvalidValue;
  if ((int64_t)pairs * (tq > tc ? tq : tc) > INT32_MAX || (int64_t)pairs * tq * k > INT32_MAX) return hipErrorInvalidValue;
  KnnArgs a;
  a.x = (const bf16_t*)x;
  a.y = (const bf16_t*)y;
  a.ldx = ldx, a.xs = x_stride, a.ldy = ldy, a.ys = y_stride;
  a.pl = knn_plan(pairs, tq, tc, k);
  a.d = d, a.exclude_diag = exclude_diag != 0, a.l2 = l2 != 0;
  const RunSplit run = run_split((int64_t)pairs * a.pl.npanels, a.pl.ntiles);  // the plan's split IS desc_tile.h's
  if (run.nsplit != a.pl.nsplit || run.base != a.pl.base || run.rem != a.pl.rem || a.pl.items > INT32_MAX) return hipErrorInvalidValue;
  float* w = (float*)work;
  a.nq = w + a.pl.off_nq;
  a.nc = w + a.pl.off_nc;
  a.pkey = w + a.pl.off_pkey;
  a.pidx = (int32_t*)(w + a.pl.off_pidx);

  const CosSide X = {a.x, ldx, x_stride, tq, a.pl.tq_pad, a.nq}, Y = {a.y, ldy, y_stride, tc, a.pl.tc_pad, a.nc};
  if (a.l2) {
    const int64_t rows = (int64_t)pairs * tq + (int64_t)pairs * tc;
    hipLaunchKernelGGL(knn_sumsq_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, X, Y, d, pairs);
    if (hipError_t e = hipGetLastError()) return e;
  } else if (hipError_t e = launch_cosine_rnorm(X, Y, d, pairs, st)) {
    return e;
  }
  return k <= 4 ? knn_launch<4>(a, val, idx, st) : k <= 8 ? knn_launch<8>(a, val, idx, st) : knn_launch<16>(a, val, idx, st);
}

}  // namespace vdr
