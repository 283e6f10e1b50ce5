// Connected components of mask planes for gfx950 (include/vdr.h: vdr_op_mask_binarize, vdr_op_connected_components,
// vdr_op_mask_clean).  The root of a selected pixel is the lowest pixel index of its component: a function of the partition
// alone, so every correct algorithm and every order of execution give the same integers.
//
//   cc_tile_kernel      a workgroup owns a 64 x 64 tile of one plane (components_map.h): it labels the tile in LDS by union-find
//                       (runs of a thread's 16 pixels first, then unions with the strip to the left and the row above) and
//                       writes each pixel's label as the plane index of its tile root and the tile root's pixel count.
//   cc_seam_kernel      a thread per pixel on a tile's left column or top row: union with its neighbours across the seam, on
//                       the label plane in global memory (find + atomicMin).
//   cc_flatten_kernel   every pixel follows its chain to the root and stores it; a tile root that is no plane root adds its
//                       count to the plane root's (one atomicAdd per (tile, component)); plane roots are counted.
//   cc_best_kernel      the per-plane minimum of the key (2^31 - 1 - area, root): the largest component, lowest root on a tie
//                       (the wave's minimum by plane_reduce.h, then one atomicMin per wave).
//   cc_apply_kernel     one step of mask_clean per pixel from area[root]; the chunk's changed count, area and box of the result
//                       go to ONE partial slot, which cc_finish_kernel (one wave per plane) reduces: plane_reduce.h, both.
//   mask_binarize_kernel  mask_stats' up-sampling, written instead of counted: ms_axis and the blend order of mask_stats.hip.
//
// INTEGER ATOMICS live in this file and only here: atomicMin on labels and on the best key, atomicAdd on pixel counts.  The
// library's "no atomics" rule exists because a float sum depends on the order of arrival; an integer minimum and an integer sum
// do not, and every output here is defined by the partition (the root is the component's lowest index whichever union came
// first; an area is a count).  Intermediate label values DO depend on the order -- outputs never do.
// Every loop carries its termination argument beside it (here or in components_map.h); the same code runs on the host first,
// tile by tile in both orders under a step cap (tests/components_map_cases.cpp).
// Built with -ffp-contract=off (Makefile) for mask_binarize: every multiply and add of the interpolation is rounded once.
#include "vdr_dev.h"
#include "vdr_kernels.h"
#include "mask_stats_map.h"
#include "components_map.h"
#include "plane_reduce.h"

namespace vdr {

namespace {

// labels in global memory: relaxed loads and stores at device scope (a label another workgroup lowered is seen, not a cached
// copy; a stale value would still be a valid, larger label of the same chain), integer atomics for min and add
struct CcGlobal {
  static __device__ inline int load(const int* L, int i) { return __hip_atomic_load(const_cast<int*>(L) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ inline void store(int* L, int i, int v) { __hip_atomic_store(L + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ inline int fetch_min(int* L, int i, int v) { return __hip_atomic_fetch_min(L + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ inline void add(int* A, int i, int v) { __hip_atomic_fetch_add(A + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// the same in LDS, at workgroup scope
struct CcLocal {
  static __device__ inline int load(const int* L, int i) { return __hip_atomic_load(const_cast<int*>(L) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ inline void store(int* L, int i, int v) { __hip_atomic_store(L + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ inline int fetch_min(int* L, int i, int v) { return __hip_atomic_fetch_min(L + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ inline void add(int* A, int i, int v) { __hip_atomic_fetch_add(A + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const uint8_t* __restrict__ mask, CcGeom q, int value, int conn8, int* __restrict__ L,
                                                             int* __restrict__ area, int* __restrict__ count,
                                                             unsigned long long* __restrict__ best) {
  __shared__ int lab[CC_LDS];
  __shared__ int cnt[CC_LDS];
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / q.tiles, t = blockIdx.x - plane * q.tiles;
  const int64_t off = (int64_t)plane * q.H * q.W;
  const CcTile c = cc_tile(q, t);
  if (t == 0 && tid == 0) {  // the per-plane accumulators of the later passes start here: one writer, a kernel boundary before their use
    if (count) count[plane] = 0;
    if (best) best[plane] = CC_NO_BEST;
  }
  cc_tile_load(c, q.W, mask + off, value, tid, lab, cnt);
  __syncthreads();
  cc_tile_runs(tid, lab);
  __syncthreads();
  cc_tile_unions<CcLocal>(tid, conn8, lab);
  __syncthreads();
  cc_tile_flatten<CcLocal>(tid, lab, cnt);
  __syncthreads();
  cc_tile_store(c, q.W, tid, lab, cnt, L + off, area + off);
}

__global__ __launch_bounds__(CC_THREADS) void cc_seam_kernel(CcGeom q, int conn8, int* L) {
  const int s = blockIdx.x * CC_THREADS + threadIdx.x;
  if (s >= q.nv + q.nh) return;
  cc_seam_unions<CcGlobal>(q, s, conn8, L + (int64_t)blockIdx.y * q.H * q.W);
}

// root may be L itself (mask_clean flattens in place): no __restrict__ on the two
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(CcGeom q, int* L, int* area, int* root, int* __restrict__ count) {
  const int plane = blockIdx.y, HW = q.H * q.W;
  const int64_t off = (int64_t)plane * HW;
  int roots = 0;
  for (int k = 0; k < CC_PER_THREAD; ++k) {  // fixed trip count
    const int i = blockIdx.x * CC_CHUNK + k * CC_THREADS + threadIdx.x;
    if (i < HW) roots += cc_flatten_pixel<CcGlobal>(i, L + off, area + off, root + off);
  }
  roots = pr_wave_sum(roots);
  if ((threadIdx.x & 63) == 0 && roots) atomicAdd(count + plane, roots);
}

__global__ __launch_bounds__(CC_THREADS) void cc_best_kernel(CcGeom q, const int* __restrict__ area, unsigned long long* __restrict__ best) {
  const int plane = blockIdx.y, HW = q.H * q.W;
  const int* a = area + (int64_t)plane * HW;
  unsigned long long key = CC_NO_BEST;
  for (int k = 0; k < CC_PER_THREAD; ++k) {  // fixed trip count
    const int i = blockIdx.x * CC_CHUNK + k * CC_THREADS + threadIdx.x;
    if (i < HW && a[i] > 0) {
      const unsigned long long u = cc_best_key(a[i], i);
      key = u < key ? u : key;
    }
  }
  key = pr_wave_min_key(key);
  if ((threadIdx.x & 63) == 0 && key != CC_NO_BEST) atomicMin(best + plane, key);
}

using CcAcc = PlaneAcc<2>;  // sums: pixels the step changed (a flag: tested against 0), area of the result (plane_reduce.h)
constexpr int CC_CHANGED = 0, CC_AREA = 1;
static_assert(CC_SLOT == PR_SLOT, "the partial slot");

// src may be out itself (the second step reads the first step's result): a pixel is read and written by its own thread only
__global__ __launch_bounds__(CC_THREADS) void cc_apply_kernel(CcGeom q, int step, int min_area, const uint8_t* src, const int* __restrict__ L,
                                                              const int* __restrict__ area, const unsigned long long* __restrict__ best,
                                                              uint8_t* out, int32_t* __restrict__ slots) {
  __shared__ int wred[CC_THREADS / 64][PR_SLOT];
  const int plane = blockIdx.y, HW = q.H * q.W, tid = threadIdx.x;
  const int64_t off = (int64_t)plane * HW;
  const int broot = step >= CC_STEP_ISLANDS ? cc_best_root(best[plane]) : -1;
  CcAcc acc = pr_identity<2>(q.W, q.H);
  for (int k = 0; k < CC_PER_THREAD; ++k) {  // fixed trip count
    const int i = blockIdx.x * CC_CHUNK + k * CC_THREADS + tid;
    if (i >= HW) continue;
    const int set = src[off + i] != 0;
    const int o = cc_apply_pixel(step, set, i, L + off, area + off, broot, min_area);
    out[off + i] = (uint8_t)o;
    acc.sum(CC_CHANGED) += o != set;
    if (o) {
      const int y = i / q.W;
      ++acc.sum(CC_AREA);
      acc.take(i - y * q.W, y);
    }
  }
  pr_block_store<2, CC_THREADS / 64>(acc, wred, slots + ((int64_t)plane * q.chunks + blockIdx.x) * CC_SLOT);
}

// one wave per plane: slots_a (the hole step's, may be null) gives bit 0 of changed, slots_b bit 1 and the statistics
__global__ __launch_bounds__(64) void cc_finish_kernel(CcGeom q, const int32_t* __restrict__ slots_a, const int32_t* __restrict__ slots_b,
                                                       int32_t* __restrict__ changed, int32_t* __restrict__ stats) {
  const int plane = blockIdx.x, lane = threadIdx.x;
  int ca = 0;
  CcAcc acc = pr_identity<2>(q.W, q.H);
  for (int c = lane; c < q.chunks; c += 64) {  // chunks is finite and c grows by 64
    const int64_t s = ((int64_t)plane * q.chunks + c) * CC_SLOT;
    if (slots_a) ca += slots_a[s + CC_CHANGED];
    acc = pr_combine(acc, pr_load<2>(slots_b + s));
  }
  ca = pr_wave_sum(ca);
  acc = pr_wave_reduce(acc);
  if (lane) return;  // every lane holds the plane's integers; one writes them
  changed[plane] = (ca ? 1 : 0) | (acc.sum(CC_CHANGED) ? 2 : 0);
  stats[plane * 5] = acc.sum(CC_AREA);
#pragma unroll
  for (int k = 0; k < 4; ++k) stats[plane * 5 + 1 + k] = acc.sum(CC_AREA) > 0 ? acc.box(k) : 0;  // an empty plane: 0, 0, 0, 0
}

// one thread per output pixel; the arithmetic of mask_stats_kernel: horizontal blends of the two source rows, then the vertical one
__global__ __launch_bounds__(CC_THREADS) void mask_binarize_kernel(const float* __restrict__ logits, int64_t plane_stride, int group,
                                                                   int64_t group_stride, MsGeom q, float thr, uint8_t* __restrict__ out) {
  const int ox = blockIdx.x * CC_THREADS + threadIdx.x, oy = blockIdx.y, plane = blockIdx.z;
  if (ox >= q.ow) return;
  const float* lg = logits + ms_plane_offset(plane, group, group_stride, plane_stride);
  const MsAxis cx = ms_axis(ox, q.sx, q.W), ry = ms_axis(oy, q.sy, q.H);
  const float* r0 = lg + (int64_t)ry.i0 * q.W;
  const float* r1 = lg + (int64_t)ry.i1 * q.W;
  const float top = cx.l0 * r0[cx.i0] + cx.l1 * r0[cx.i1];
  const float bot = cx.l0 * r1[cx.i0] + cx.l1 * r1[cx.i1];
  const float v = ry.l0 * top + ry.l1 * bot;
  out[((int64_t)plane * q.oh + oy) * q.ow + ox] = v > thr ? 1 : 0;
}

bool cc_shape_ok(int P, int H, int W) { return P >= 1 && P <= CC_MAX_PLANES && H >= 1 && H <= CC_MAX_SIDE && W >= 1 && W <= CC_MAX_SIDE; }

// tile, seam, flatten of one labelling: three launches
void cc_label(const uint8_t* mask, const CcGeom& q, int value, int conn8, int* L, int* area, int* root, int* count, unsigned long long* best,
              hipStream_t s) {
  const int items = q.nv + q.nh;
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)(q.P * q.tiles)), dim3(CC_THREADS), 0, s, mask, q, value, conn8, L, area, count, best);
  hipLaunchKernelGGL(cc_seam_kernel, dim3((unsigned)((items + CC_THREADS - 1) / CC_THREADS > 0 ? (items + CC_THREADS - 1) / CC_THREADS : 1), (unsigned)q.P),
                     dim3(CC_THREADS), 0, s, q, conn8, L);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)q.chunks, (unsigned)q.P), dim3(CC_THREADS), 0, s, q, L, area, root, count);
}

}  // namespace

size_t components_workspace_bytes(int P, int H, int W, int clean) {
  if (!cc_shape_ok(P, H, W)) return 0;
  return (size_t)cc_work(cc_geom(P, H, W), clean).bytes;
}

hipError_t launch_connected_components(const uint8_t* mask, int P, int H, int W, int connectivity, int value, void* work, int32_t* root,
                                       int32_t* area, int32_t* count, hipStream_t s) {
  if (!cc_shape_ok(P, H, W) || (connectivity != 4 && connectivity != 8)) return hipErrorInvalidValue;
  const CcGeom q = cc_geom(P, H, W);
  cc_label(mask, q, value, connectivity == 8, (int*)work, area, root, count, nullptr, s);
  return hipGetLastError();
}

hipError_t launch_mask_clean(const uint8_t* mask, int P, int H, int W, int min_area, int connectivity, int mode, void* work, uint8_t* out,
                             int32_t* changed, int32_t* stats, hipStream_t s) {
  if (!cc_shape_ok(P, H, W) || (connectivity != 4 && connectivity != 8) || min_area < 0) return hipErrorInvalidValue;
  const CcGeom q = cc_geom(P, H, W);
  const CcWork w = cc_work(q, 1);
  char* base = (char*)work;
  int* L = (int*)(base + w.L);
  int* area = (int*)(base + w.area);
  unsigned long long* best = (unsigned long long*)(base + w.best);
  int* count = (int*)(base + w.count);
  int32_t* slots_a = (int32_t*)(base + w.slots_a);
  int32_t* slots_b = (int32_t*)(base + w.slots_b);
  const int conn8 = connectivity == 8;
  const dim3 grid((unsigned)q.chunks, (unsigned)q.P);
  const uint8_t* cur = mask;
  const bool holes = mode & 1, islands = mode & 2, largest = mode & 4;
  if (holes) {
    cc_label(cur, q, 0, conn8, L, area, L, count, best, s);
    hipLaunchKernelGGL(cc_apply_kernel, grid, dim3(CC_THREADS), 0, s, q, CC_STEP_HOLES, min_area, cur, (const int*)L, (const int*)area,
                       (const unsigned long long*)best, out, slots_a);
    cur = out;
  }
  int step = CC_STEP_COPY;
  if (islands || largest) {
    step = largest ? CC_STEP_LARGEST : CC_STEP_ISLANDS;
    cc_label(cur, q, 1, conn8, L, area, L, count, best, s);
    hipLaunchKernelGGL(cc_best_kernel, grid, dim3(CC_THREADS), 0, s, q, (const int*)area, best);
  }
  hipLaunchKernelGGL(cc_apply_kernel, grid, dim3(CC_THREADS), 0, s, q, step, min_area, cur, (const int*)L, (const int*)area,
                     (const unsigned long long*)best, out, slots_b);
  hipLaunchKernelGGL(cc_finish_kernel, dim3((unsigned)q.P), dim3(64), 0, s, q, holes ? (const int32_t*)slots_a : (const int32_t*)nullptr,
                     (const int32_t*)slots_b, changed, stats);
  return hipGetLastError();
}

hipError_t launch_mask_binarize(const float* logits, int64_t plane_stride, int group, int64_t group_stride, int P, int H, int W, int oh, int ow,
                                float threshold, uint8_t* out, hipStream_t s) {
  if (!mask_stats_workspace_bytes(P, H, W, oh, ow) || group < 1 || plane_stride < (int64_t)H * W) return hipErrorInvalidValue;
  const MsGeom q = ms_geom(P, H, W, oh, ow);
  hipLaunchKernelGGL(mask_binarize_kernel, dim3((unsigned)((ow + CC_THREADS - 1) / CC_THREADS), (unsigned)oh, (unsigned)P), dim3(CC_THREADS), 0, s,
                     logits, plane_stride, group, group_stride, q, threshold, out);
  return hipGetLastError();
}

}  // namespace vdr
