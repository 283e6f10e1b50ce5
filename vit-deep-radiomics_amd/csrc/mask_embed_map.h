// The ONE mapping of the fused keys kernel (mask_prompt.hip; the definition is vdr_op_mask_embed's in include/vdr.h): which
// problem, cell, image and mask a row of a tile stands for, and every offset the kernel forms from them.  The kernel, the
// launch plan and the host program tests/mask_embed_map_cases.cpp all call it; it includes nothing and compiles as plain C++.
//
//   keys   [P * n, 256] bf16, row R = p * n + cell, cell = cy * g + cx, n = g * g
//   tile   ME_CELLS consecutive rows R (a tile may span two problems; the last one may be ragged)
//   emb    fp32 [B, 256, n] (channels_last = 0) or [B, n, 256] (1); problem p reads image p / nb
//   mask   fp32 [P, 4g, 4g], or [B, 4g, 4g] with mask_per_image (problem p reads mask p / nb); cell (cy, cx) reads the 4 x 4
//          pixels (4 cy + py, 4 cx + px)
// Rows past the end (`ok` false) load row P * n - 1 (a valid address; the value is never stored).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ME_HD __host__ __device__ inline
#else
#define ME_HD inline
#endif

namespace vdr {

constexpr int ME_CELLS = 32;  // rows of keys per tile (one workgroup)
constexpr int ME_C = 256;     // channels

struct MeGeom {
  int g, n, P, nb, channels_last, mask_per_image;
  long long rows;   // P * n
  long long tiles;  // ceil(rows / ME_CELLS)
};

ME_HD MeGeom me_geom(int P, int nb, int g, int channels_last, int mask_per_image) {
  MeGeom m;
  m.g = g, m.n = g * g, m.P = P, m.nb = nb, m.channels_last = channels_last, m.mask_per_image = mask_per_image;
  m.rows = (long long)P * m.n;
  m.tiles = (m.rows + ME_CELLS - 1) / ME_CELLS;
  return m;
}

struct MeRow {
  long long R;    // the row to load, in [0, rows)
  bool ok;        // the row exists: it is stored
  int cell, cy, cx;
  long long p, b, m;   // problem, image, mask
};

ME_HD MeRow me_row(const MeGeom& q, long long tile, int i) {
  MeRow r;
  const long long R = tile * ME_CELLS + i;
  r.ok = R < q.rows;
  r.R = r.ok ? R : q.rows - 1;
  r.p = r.R / q.n;
  r.cell = (int)(r.R - r.p * q.n);
  r.cy = r.cell / q.g;
  r.cx = r.cell - r.cy * q.g;
  r.b = r.p / q.nb;
  r.m = q.mask_per_image ? r.b : r.p;
  return r;
}

// element offset of emb[image of the row, channel c, cell of the row]
ME_HD long long me_emb_offset(const MeGeom& q, const MeRow& r, int c) {
  return q.channels_last ? (r.b * q.n + r.cell) * ME_C + c : (r.b * ME_C + c) * q.n + r.cell;
}

// element offset of the first of the 4 contiguous pixels of row py (0 .. 3) of the cell's 4 x 4 block; a multiple of 4
ME_HD long long me_mask_offset(const MeGeom& q, const MeRow& r, int py) {
  const long long G4 = 4LL * q.g;
  return (r.m * G4 + 4 * r.cy + py) * G4 + 4 * r.cx;
}

// element offset of keys[row, c]
ME_HD long long me_key_offset(const MeRow& r, int c) { return r.R * ME_C + c; }

}  // namespace vdr
