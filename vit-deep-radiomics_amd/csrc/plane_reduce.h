// The ONE integer reduction of the mask-plane kernels (mask_stats.hip, components.hip, edt.hip, mask_prompt.hip): a few int32
// sums plus the inclusive box of the counted pixels, or one packed 64-bit key.  A thread accumulates its pixels, the wave
// reduces by lane exchange, the workgroup's wave leaders meet in LDS behind one barrier, ONE partial slot per workgroup goes to
// the workspace, and a one-wave-per-plane finish kernel reduces the plane's slots.  The combine rules, the identity and the
// slot layout compile as plain C++ (tests/plane_reduce_cases.cpp walks them on the host); only the lane exchange and the LDS
// step are device code.  Sum, min and max of integers are associative and commutative, so the result depends on no order of
// lanes, waves, slots or workgroups.  No read-modify-write of shared memory here: every LDS cell and every slot has one writer.
//
//   value k of PlaneAcc<NS>   k < NS a sum; NS, NS + 1 the box minima (x, y); NS + 2, NS + 3 the box maxima (x, y)
//   identity                  sums 0, minima at (w, h) -- one past the last column and row -- maxima -1: an empty box
//   slot                      PR_SLOT int32, value k at slot[k] (NS + 4 <= PR_SLOT; the rest is never written or read)
//   flags                     an or-flag is carried as a sum of 0 / 1 (a plane has at most 2^24 pixels) and tested against 0
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PR_HD __host__ __device__ inline
#else
#define PR_HD inline
#endif

namespace vdr {

constexpr int PR_SLOT = 8;  // int32 of a partial slot

template <int NS> struct PlaneAcc {
  static_assert(NS >= 1 && NS + 4 <= PR_SLOT, "a slot holds the sums and the box");
  int v[NS + 4];
  PR_HD int& sum(int k) { return v[k]; }
  PR_HD int sum(int k) const { return v[k]; }
  PR_HD int box(int k) const { return v[NS + k]; }  // min x, min y, max x, max y
  PR_HD void take(int x, int y) {                   // the box grows by one pixel (the sums are the caller's)
    v[NS] = x < v[NS] ? x : v[NS], v[NS + 1] = y < v[NS + 1] ? y : v[NS + 1];
    v[NS + 2] = x > v[NS + 2] ? x : v[NS + 2], v[NS + 3] = y > v[NS + 3] ? y : v[NS + 3];
  }
};

// the rule of value k
template <int NS> PR_HD int pr_combine_value(int k, int a, int b) { return k < NS ? a + b : k < NS + 2 ? (b < a ? b : a) : (b > a ? b : a); }

template <int NS> PR_HD PlaneAcc<NS> pr_identity(int w, int h) {
  PlaneAcc<NS> a;
  for (int k = 0; k < NS; ++k) a.v[k] = 0;
  a.v[NS] = w, a.v[NS + 1] = h, a.v[NS + 2] = -1, a.v[NS + 3] = -1;
  return a;
}

template <int NS> PR_HD PlaneAcc<NS> pr_combine(const PlaneAcc<NS>& a, const PlaneAcc<NS>& b) {
  PlaneAcc<NS> r;
  for (int k = 0; k < NS + 4; ++k) r.v[k] = pr_combine_value<NS>(k, a.v[k], b.v[k]);
  return r;
}

template <int NS> PR_HD void pr_store(const PlaneAcc<NS>& a, int32_t* slot) {
  for (int k = 0; k < NS + 4; ++k) slot[k] = a.v[k];
}

template <int NS> PR_HD PlaneAcc<NS> pr_load(const int32_t* slot) {
  PlaneAcc<NS> a;
  for (int k = 0; k < NS + 4; ++k) a.v[k] = slot[k];
  return a;
}

// value k of the workgroup, from the wave leaders' accumulators in `wred`
template <int NS, int WAVES> PR_HD int pr_waves_value(const int (*wred)[PR_SLOT], int k) {
  int v = wred[0][k];
  for (int w = 1; w < WAVES; ++w) v = pr_combine_value<NS>(k, v, wred[w][k]);  // fixed trip count
  return v;
}

#if defined(__HIPCC__) || defined(__CUDACC__)
// ---- device only: the lane exchange (fixed trip count: six halvings) and the LDS step --------------------------------------------
__device__ inline int pr_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int NS> __device__ inline PlaneAcc<NS> pr_wave_reduce(PlaneAcc<NS> a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    PlaneAcc<NS> b;
#pragma unroll
    for (int k = 0; k < NS + 4; ++k) b.v[k] = __shfl_xor(a.v[k], o);
    a = pr_combine(a, b);
  }
  return a;
}

// Workgroup reduce of WAVES * 64 threads, every one of which calls it: wave leaders to `wred`, one barrier.  Afterwards any
// thread reads value k of the workgroup with pr_waves_value<NS, WAVES>(wred, k).
template <int NS, int WAVES> __device__ inline void pr_block_reduce(PlaneAcc<NS> a, int (*wred)[PR_SLOT]) {
  a = pr_wave_reduce(a);
  if ((threadIdx.x & 63) == 0) pr_store(a, wred[threadIdx.x >> 6]);
  __syncthreads();
}

// ... and the workgroup's slot: thread k writes value k, one writer each
template <int NS, int WAVES> __device__ inline void pr_block_store(PlaneAcc<NS> a, int (*wred)[PR_SLOT], int32_t* slot) {
  pr_block_reduce<NS, WAVES>(a, wred);
  if (threadIdx.x < NS + 4) slot[threadIdx.x] = pr_waves_value<NS, WAVES>(wred, threadIdx.x);
}

// the 64-bit key of the arg-best reductions (cc_best_key, edt_peak_key), exchanged as two 32-bit halves: the wave's largest
// (MAX) or smallest key
template <bool MAX> __device__ inline unsigned long long pr_wave_key(unsigned long long key) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(key >> 32), o), lo = __shfl_xor((unsigned)key, o);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    key = (MAX ? u > key : u < key) ? u : key;
  }
  return key;
}
__device__ inline unsigned long long pr_wave_min_key(unsigned long long key) { return pr_wave_key<false>(key); }
__device__ inline unsigned long long pr_wave_max_key(unsigned long long key) { return pr_wave_key<true>(key); }

// the workgroup's largest key, in thread 0 only: wave leaders to `wred[WAVES]`, one barrier
template <int WAVES> __device__ inline unsigned long long pr_block_max_key(unsigned long long key, unsigned long long* wred) {
  key = pr_wave_max_key(key);
  if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < WAVES; ++w) key = wred[w] > key ? wred[w] : key;  // fixed trip count
  return key;
}
#endif

}  // namespace vdr
