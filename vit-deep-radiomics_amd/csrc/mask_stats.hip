// The statistics of SAM's automatic mask generator for gfx950 (include/vdr.h, vdr_op_mask_stats): per plane of low-resolution
// logits the pixel counts of its bilinear up-sampling above thr + off, thr and thr - off and the box of the pixels above thr.
// The up-sampled plane is never written.
//
//   mask_stats_kernel   a workgroup owns a band of output rows of one plane (mask_stats_map.h) and stages the source rows the band
//                       reads in LDS, once (a 4 x up-sampling reads each staged row for 4 output rows).  A thread owns output
//                       columns: the horizontal blends of the two source rows of an output row depend on the column and the
//                       source row alone, so the thread keeps them while the source rows stay the same -- at 4 x that is 1 LDS read
//                       per 2 pixels instead of 4 per pixel -- and the rows' indices and weights come from a table in LDS
//                       (one broadcast read per row).  Three counts and a box: the plane reduction of plane_reduce.h, ONE
//                       partial slot per band.
//   mask_stats_finish   one wave per plane reduces the plane's slots (plane_reduce.h again) and writes its seven integers.
//
// No atomics, one writer per output, integer reductions only: a plane's outputs depend neither on P nor on its position.
// Built with -ffp-contract=off (Makefile): every multiply and add of the interpolation is rounded once.
#include "vdr_dev.h"
#include "vdr_kernels.h"
#include "mask_stats_map.h"
#include "plane_reduce.h"

namespace vdr {

namespace {

using MsAcc = PlaneAcc<3>;  // sums: n_hi, n_mid, n_lo (plane_reduce.h)
constexpr int MS_HI = 0, MS_MID = 1, MS_LO = 2;
static_assert(MS_SLOT == PR_SLOT, "the partial slot");

__global__ __launch_bounds__(MS_THREADS) void mask_stats_kernel(const float* __restrict__ logits, int64_t plane_stride, int group,
                                                                int64_t group_stride, MsGeom q, float t_hi, float thr, float t_lo,
                                                                int vec, int32_t* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float stage[MS_STAGE_ROWS * MS_MAX_SIDE];
  __shared__ MsAxis rowtab[MS_BAND];
  __shared__ int wred[MS_THREADS / 64][PR_SLOT];
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / q.bands, band = blockIdx.x - plane * q.bands;
  const MsBand b = ms_band(q, band);
  const int W = q.W, nrows = b.r1 - b.r0;
  const float* lg = logits + ms_plane_offset(plane, group, group_stride, plane_stride) + (int64_t)b.lo * W;
  const int total = b.n * W;  // at most MS_STAGE_ROWS * MS_MAX_SIDE: the staged rows are one contiguous run of the plane
  if (vec) {
    for (int i = 4 * tid; i < total; i += 4 * MS_THREADS) *reinterpret_cast<f32x4*>(stage + i) = *reinterpret_cast<const f32x4*>(lg + i);
  } else {
    for (int i = tid; i < total; i += MS_THREADS) stage[i] = lg[i];
  }
  if (tid < nrows) {
    MsAxis a = ms_axis(b.r0 + tid, q.sy, q.H);
    a.i0 = (a.i0 - b.lo) * W, a.i1 = (a.i1 - b.lo) * W;  // offsets of the two rows inside the stage
    rowtab[tid] = a;
  }
  __syncthreads();
  MsAcc acc = pr_identity<3>(q.ow, q.oh);
  for (int ox = tid; ox < q.ow; ox += MS_THREADS) {
    const MsAxis cx = ms_axis(ox, q.sx, W);
    auto blend = [&](int row) { return cx.l0 * stage[row + cx.i0] + cx.l1 * stage[row + cx.i1]; };
    int c0 = -1, c1 = -1;
    float top = 0.0f, bot = 0.0f;
    int y0 = q.oh, y1 = -1;  // the column's rows above thr
    for (int r = 0; r < nrows; ++r) {
      const MsAxis ry = rowtab[r];
      if (ry.i0 != c0 || ry.i1 != c1) {  // (uniform in the workgroup)
        top = ry.i0 == c1 ? bot : blend(ry.i0);
        bot = ry.i1 == ry.i0 ? top : blend(ry.i1);
        c0 = ry.i0, c1 = ry.i1;
      }
      const float v = ry.l0 * top + ry.l1 * bot;
      acc.sum(MS_HI) += v > t_hi;
      acc.sum(MS_LO) += v > t_lo;
      if (v > thr) {
        const int oy = b.r0 + r;
        ++acc.sum(MS_MID);
        y0 = oy < y0 ? oy : y0;
        y1 = oy > y1 ? oy : y1;
      }
    }
    if (y1 >= 0) acc.take(ox, y0), acc.take(ox, y1);
  }
  pr_block_store<3, MS_THREADS / 64>(acc, wred, part + ms_slot(q, plane, band, 0));
}

__global__ __launch_bounds__(64) void mask_stats_finish_kernel(const int32_t* __restrict__ part, MsGeom q, int32_t* __restrict__ counts,
                                                               int32_t* __restrict__ box) {
  const int plane = blockIdx.x, lane = threadIdx.x;
  MsAcc acc = pr_identity<3>(q.ow, q.oh);
  for (int band = lane; band < q.bands; band += 64) acc = pr_combine(acc, pr_load<3>(part + ms_slot(q, plane, band, 0)));
  acc = pr_wave_reduce(acc);
  if (lane) return;  // every lane holds the plane's seven integers; one writes them
#pragma unroll
  for (int k = 0; k < 3; ++k) counts[plane * 3 + k] = acc.sum(k);
#pragma unroll
  for (int k = 0; k < 4; ++k) box[plane * 4 + k] = acc.sum(MS_MID) > 0 ? acc.box(k) : 0;  // an empty mask: 0, 0, 0, 0
}

}  // namespace

size_t mask_stats_workspace_bytes(int P, int H, int W, int oh, int ow) {
  if (P < 1 || P > 65535 || H < 1 || H > MS_MAX_SIDE || W < 1 || W > MS_MAX_SIDE || oh < 1 || oh > MS_MAX_OUT || ow < 1 || ow > MS_MAX_OUT) return 0;
  return (size_t)ms_slots(ms_geom(P, H, W, oh, ow)) * MS_SLOT * sizeof(int32_t);
}

hipError_t launch_mask_stats(const float* logits, int64_t plane_stride, int group, int64_t group_stride, int P, int H, int W, int oh, int ow,
                             float threshold, float offset, void* work, int32_t* counts, int32_t* box, hipStream_t s) {
  if (!mask_stats_workspace_bytes(P, H, W, oh, ow) || group < 1 || plane_stride < (int64_t)H * W) return hipErrorInvalidValue;
  const MsGeom q = ms_geom(P, H, W, oh, ow);
  for (int band = 0; band < q.bands; ++band) {  // what the kernel stages fits its LDS (mask_stats_map.h argues it; tests/mask_stats_map_cases.cpp walks it)
    const MsBand b = ms_band(q, band);
    if (b.lo < 0 || b.n < 1 || b.n > MS_STAGE_ROWS || b.lo + b.n > H) return hipErrorInvalidValue;
  }
  const float t_hi = threshold + offset, t_lo = threshold - offset;
  const int vec = !(W & 3) && !(plane_stride & 3) && !(group_stride & 3) && !((uintptr_t)logits & 15);
  hipLaunchKernelGGL(mask_stats_kernel, dim3((unsigned)ms_slots(q)), dim3(MS_THREADS), 0, s, logits, plane_stride, group, group_stride, q, t_hi,
                     threshold, t_lo, vec, (int32_t*)work);
  hipLaunchKernelGGL(mask_stats_finish_kernel, dim3((unsigned)P), dim3(64), 0, s, (const int32_t*)work, q, counts, box);
  return hipGetLastError();
}

}  // namespace vdr
