// The ONE mapping of the mask statistics kernels (mask_stats.hip; the definition is vdr_op_mask_stats's in include/vdr.h): which
// output rows a work item owns, which source rows it stages in LDS, the bilinear source index and weights of an output row or
// column, and the partial slot a work item writes and the finish reads.  The kernels, the launch plan and the host program
// tests/mask_stats_map_cases.cpp all call it; it includes nothing and compiles as plain C++ (no fused multiply-add: the .hip
// file is compiled with -ffp-contract=off, a host compiler contracts nothing without being asked).
//
//   plane   p of P: H x W fp32 at logits + (p / group) * group_stride + (p % group) * plane_stride elements
//   item    blockIdx.x = p * bands + band; a band is `rows` consecutive output rows [r0, r1) and every output column
//   stage   the source rows [lo, lo + n) the band's rows read, n <= MS_STAGE_ROWS, contiguous in the plane
//   slot    part[(p * bands + band) * MS_SLOT + k], k = 0 .. 6: n_hi, n_mid, n_lo, min x, min y, max x, max y of the band
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MS_HD __host__ __device__ inline
#else
#define MS_HD inline
#endif

namespace vdr {

constexpr int MS_THREADS = 256;
constexpr int MS_BAND = 32;        // output rows of a band at most
constexpr int MS_STAGE_ROWS = 32;  // source rows staged at most: 32 x 256 fp32 = 32 KB of LDS
constexpr int MS_MAX_SIDE = 256;   // H, W
constexpr int MS_MAX_OUT = 4096;   // oh, ow
constexpr int MS_SLOT = 8;         // int32 of a partial slot (7 used)

struct MsGeom {
  int P, H, W, oh, ow;
  int rows;   // output rows of a band (the last band may be shorter)
  int bands;  // per plane
  float sy, sx;
};

// rows: (rows - 1) * H / oh <= 28, so a band's first and last source index are at most 28 (+ rounding) apart and, with the + 1
// of the lower neighbour row and the truncations, its staged rows number at most 32 (walked for every case by the host program)
MS_HD MsGeom ms_geom(int P, int H, int W, int oh, int ow) {
  MsGeom q;
  q.P = P, q.H = H, q.W = W, q.oh = oh, q.ow = ow;
  q.sy = (float)H / (float)oh;
  q.sx = (float)W / (float)ow;
  const int fit = 1 + (28 * oh) / H;
  q.rows = fit < MS_BAND ? fit : MS_BAND;
  q.bands = (oh + q.rows - 1) / q.rows;
  return q;
}

// torch's upsample_bilinear2d(align_corners=False) source of output index o along an axis of n source samples
struct MsAxis {
  int i0, i1;
  float l0, l1;
};

MS_HD MsAxis ms_axis(int o, float scale, int n) {
  MsAxis a;
  float src = ((float)o + 0.5f) * scale - 0.5f;  // three roundings
  src = src < 0.0f ? 0.0f : src;
  a.i0 = (int)src;
  a.i0 = a.i0 < n - 1 ? a.i0 : n - 1;  // (never binds for the sizes the op accepts: src < n)
  a.l1 = src - (float)a.i0;
  a.l0 = 1.0f - a.l1;
  a.i1 = a.i0 + (a.i0 < n - 1 ? 1 : 0);
  return a;
}

struct MsBand {
  int r0, r1;  // output rows [r0, r1)
  int lo, n;   // staged source rows [lo, lo + n)
};

MS_HD MsBand ms_band(const MsGeom& q, int band) {
  MsBand b;
  b.r0 = band * q.rows;
  b.r1 = b.r0 + q.rows < q.oh ? b.r0 + q.rows : q.oh;
  b.lo = ms_axis(b.r0, q.sy, q.H).i0;               // i0 and i1 do not decrease with the output row
  b.n = ms_axis(b.r1 - 1, q.sy, q.H).i1 - b.lo + 1;
  return b;
}

// element offset of plane p
MS_HD long long ms_plane_offset(long long p, int group, long long group_stride, long long plane_stride) {
  return (p / group) * group_stride + (p % group) * plane_stride;
}

// element offset (int32) of value k of the partial slot of (plane, band)
MS_HD long long ms_slot(const MsGeom& q, long long p, int band, int k) { return (p * q.bands + band) * MS_SLOT + k; }

MS_HD long long ms_slots(const MsGeom& q) { return (long long)q.P * q.bands; }

}  // namespace vdr
