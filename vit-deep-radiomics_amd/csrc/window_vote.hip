// Multi-source soft window vote for gfx950 (include/vdr.h, vdr_op_window_vote): for `problems` problems on one gh x gw grid,
// every patch takes the k best of the in-grid candidates of its S windows -- S cost volumes [t, W * W] as
// vdr_op_local_correlation writes them -- under the total order (greater value, lower source, lower slot), and votes the
// candidates' soft class rows with softmax or uniform weights.  Selection is exact comparisons; the vote is the fp32
// operations of the header in the header's order (this file is built with -ffp-contract=off).
//
// One launch, no atomics:
//   window_vote_kernel  256 threads = 4 waves, ONE WAVE PER QUERY (p, i).  Lane l owns the row elements e = l + 64 * n,
//                       e = s * W * W + w, at most 37 of them (S = 8, r = 8: 2312 floats).  It works out once which of them
//                       lie inside the grid -- from (gh, gw, r), never from the -inf of the cost volume --, keeps that as a
//                       64-bit mask and copies the in-grid values into the wave's LDS row, where only lane l reads them
//                       again: the LDS is per-lane storage that a runtime trip count may index, which a register array is
//                       not (it would go to scratch).  k rounds: a lane-local maximum over the lane's eligible
//                       elements in ascending e, a butterfly on the full (value, e) key, the winner broadcast from lane 0;
//                       its owner clears the mask bit, and LANE m KEEPS NEIGHBOUR m -- no list indexed by the wave-uniform
//                       m exists.  Lane m turns e into idx = s * t + j and its weight; the k steps of the two sums read
//                       (weight, idx) of lane m by a shuffle, LANE c GATHERS CLASS c (C <= 64: one coalesced row per
//                       neighbour) and divides once.  A butterfly on (score, lowest class) gives the label.
// Every entry has one writer (scores: lane c; idx / val: lane m; labels: lane 0 of the query's wave), every store is a
// plain vector store, and a query reads its own problem alone: the bits depend on (gh, gw, r, S, k, C, weights, T, inputs).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>

#include "../../include/vdr.h"
#include "local_corr_map.h"
#include "vdr_kernels.h"

namespace vdr {
namespace {

constexpr int WV_WAVES = 4;      // queries per block
constexpr int WV_NONE = INT_MAX;  // "no element": loses against every element

struct WvArgs {
  const float *cost, *src;  // [P][S][t][W * W], [P][S][t][C]
  int P, S, gh, gw, r, k, C;
  int uniform;
  float inv_t;  // 1.0f / temperature, rounded once on the host
  float* scores;
  int32_t *labels, *idx;
  float* val;
};

// a beats b: greater value, then lower index; WV_NONE never wins and always loses
__device__ __forceinline__ bool wv_better(float av, int ai, float bv, int bi) {
  return ai != WV_NONE && (bi == WV_NONE || av > bv || (av == bv && ai < bi));
}

__global__ __launch_bounds__(64 * WV_WAVES) void window_vote_kernel(WvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_rows[];  // [WV_WAVES][S * W * W]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = a.gh * a.gw, W = 2 * a.r + 1, WW = W * W, len = a.S * WW;
  const int64_t q = (int64_t)blockIdx.x * WV_WAVES + wave;
  if (q >= (int64_t)a.P * t) return;  // (a whole wave; the kernel has no barrier)
  const int p = (int)(q / t), i = (int)(q - (int64_t)p * t);
  const int qy = i / a.gw, qx = i - qy * a.gw;
  float* row = s_rows + wave * len;

  // which of the lane's elements are candidates (inside the grid), and their values
  uint64_t ok = 0;
  for (int n = 0, e = lane; e < len; ++n, e += 64) {
    const int s = e / WW, w = e - s * WW, wy = w / W;
    const int cy = qy + wy - a.r, cx = qx + (w - wy * W) - a.r;
    if ((unsigned)cy < (unsigned)a.gh && (unsigned)cx < (unsigned)a.gw) {
      ok |= 1ull << n;
      row[e] = a.cost[(((int64_t)p * a.S + s) * t + i) * WW + w];
    }
  }

  // k rounds of selection; lane m keeps neighbour m.  The own position in source 0 is in the grid for every query: it is what
  // a lane without a neighbour holds (lanes >= k), and what a round without a winner would record -- which cannot happen:
  // a query has at least S * min(gh, r + 1) * min(gw, r + 1) candidates and the entry point refuses a larger k.
  const int e_self = a.r * W + a.r;
  float my_v = 0.f;
  int my_e = e_self;
  for (int m = 0; m < a.k; ++m) {
    float bv = 0.f;
    int be = WV_NONE;
    for (int n = 0, e = lane; e < len; ++n, e += 64) {
      if ((ok >> n) & 1) {
        const float v = row[e];
        if (be == WV_NONE || v > bv) {  // (ascending e inside the lane: > alone keeps the lowest e of equal values)
          bv = v;
          be = e;
        }
      }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oe = __shfl_xor(be, o, 64);
      if (wv_better(ov, oe, bv, be)) {
        bv = ov;
        be = oe;
      }
    }
    bv = __shfl(bv, 0, 64);  // one winner for the whole wave, whatever the values are
    be = __shfl(be, 0, 64);
    if (be == WV_NONE) be = e_self;
    if ((be & 63) == lane) ok &= ~(1ull << (be >> 6));
    if (lane == m) {
      my_v = bv;
      my_e = be;
    }
  }

  // lane m: the neighbour's row s * t + j of this problem's src, and its weight
  const int ms = my_e / WW, mw = my_e - ms * WW, mwy = mw / W;
  const int my_row = ms * t + (qy + mwy - a.r) * a.gw + (qx + (mw - mwy * W) - a.r);
  const float v0 = __shfl(my_v, 0, 64);
  const float my_w = a.uniform ? 1.0f : expf((my_v - v0) * a.inv_t);
  if (a.idx && lane < a.k) {
    a.idx[q * a.k + lane] = my_row;
    a.val[q * a.k + lane] = my_v;
  }

  // lane c: class c.  Both sums in fp32, ascending in m, from the first term; one division.
  const float* src = a.src + (int64_t)p * a.S * t * a.C;
  float num = 0.f, den = 0.f;
  for (int m = 0; m < a.k; ++m) {
    const float em = __shfl(my_w, m, 64);
    const int rm = __shfl(my_row, m, 64);
    const float x = lane < a.C ? src[(int64_t)rm * a.C + lane] : 0.f;
    const float ex = em * x;
    num = m == 0 ? ex : num + ex;
    den = m == 0 ? em : den + em;
  }
  const float score = num / den;
  if (lane < a.C) a.scores[q * a.C + lane] = score;

  if (a.labels) {  // the lowest class of the largest score
    float bs = score;
    int bc = lane < a.C ? lane : WV_NONE;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float os = __shfl_xor(bs, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      if (wv_better(os, oc, bs, bc)) {
        bs = os;
        bc = oc;
      }
    }
    if (lane == 0) a.labels[q] = bc == WV_NONE ? 0 : bc;
  }
}

}  // namespace

hipError_t launch_window_vote(const float* cost, const float* src, int problems, int sources, int gh, int gw, int radius, int k,
                              int n_classes, int weights, float temperature, float* scores, int32_t* labels, int32_t* idx,
                              float* val, hipStream_t st) {
  static_assert(VDR_WINDOW_VOTE_MAX_SOURCES * (2 * LC_MAX_RADIUS + 1) * (2 * LC_MAX_RADIUS + 1) <= 64 * 64,
                "a lane's elements must fit its 64-bit mask");
  static_assert(VDR_WINDOW_VOTE_MAX_K <= 64 && VDR_WINDOW_VOTE_MAX_CLASSES <= 64, "lane m keeps neighbour m, lane c class c");
  if (!cost || !src || !scores || (!idx) != (!val) || problems <= 0 || gh <= 0 || gw <= 0 || sources < 1 ||
      sources > VDR_WINDOW_VOTE_MAX_SOURCES || radius < 1 || radius > LC_MAX_RADIUS || k < 1 || k > VDR_WINDOW_VOTE_MAX_K ||
      n_classes < 1 || n_classes > VDR_WINDOW_VOTE_MAX_CLASSES || (weights != VDR_VOTE_SOFTMAX && weights != VDR_VOTE_UNIFORM) ||
      !(temperature > 0.f) || !(temperature <= FLT_MAX))
    return hipErrorInvalidValue;
  const int64_t t = (int64_t)gh * gw, WW = (int64_t)(2 * radius + 1) * (2 * radius + 1);
  const int64_t corner = (int64_t)sources * (gh < radius + 1 ? gh : radius + 1) * (gw < radius + 1 ? gw : radius + 1);
  if (t > INT32_MAX || (int64_t)problems * t > INT32_MAX || k > corner) return hipErrorInvalidValue;
  if ((int64_t)problems * t * sources > INT32_MAX / (WW > n_classes ? WW : n_classes)) return hipErrorInvalidValue;
  WvArgs a;
  a.cost = cost, a.src = src;
  a.P = problems, a.S = sources, a.gh = gh, a.gw = gw, a.r = radius, a.k = k, a.C = n_classes;
  a.uniform = weights == VDR_VOTE_UNIFORM;
  a.inv_t = 1.0f / temperature;
  a.scores = scores, a.labels = labels, a.idx = idx, a.val = val;
  const int64_t rows = (int64_t)problems * t;
  const size_t lds = (size_t)WV_WAVES * sources * WW * sizeof(float);  // at most 4 * 2312 * 4 = 36992 bytes
  hipLaunchKernelGGL(window_vote_kernel, dim3((unsigned)((rows + WV_WAVES - 1) / WV_WAVES)), dim3(64 * WV_WAVES), lds, st, a);
  return hipGetLastError();
}

}  // namespace vdr
