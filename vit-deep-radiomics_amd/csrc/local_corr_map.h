// The ONE mapping of the windowed correlation (local_corr.hip; the definition is vdr_op_local_correlation's in include/vdr.h):
// which grid position, source row and window slot a row of a staged tile stands for.  The kernel, the launch plan and the host
// program tests/local_corr_map_cases.cpp all call it; it includes nothing and compiles as plain C++.
//
//   grid       gh x gw positions, t = gh * gw rows, row = y * gw + x
//   panel      an LC_PH x LC_PW block of query positions (128 rows of the A operand), panels row-major over the grid
//   halo       the panel grown by r on every side: (LC_PH + 2r) x (LC_PW + 2r) candidate positions, numbered row-major and cut
//              into tiles of 128 (the B operand): 2 tiles at r = 1, 3 at r = 4, 6 at r = 8
//   work item  (pair, panel, tile), tile fastest
//
// lc_map(g, panel, tile, side, row): side 0 is row `row` of the panel, side 1 row `row` of halo tile `tile`.  It returns the
// position (y, x) -- for a candidate it may lie outside the grid, for both it may lie past the ragged edge --, whether it counts
// (`ok`: in the grid, and for a candidate inside the halo), and `src`, the row to LOAD: the position clamped into the grid,
// always in [0, t).  No address is ever formed from an unclamped position.
// lc_slot(g, q, c): the window slot (dy + r) * W + (dx + r) of candidate position c as seen from query position q, or -1 when
// it is outside the window.  Every (in-grid query, slot) pair turns up in exactly one (tile, row) of the query's panel -- the halo
// holds the whole window of every query of its panel once --, so the item that meets it OWNS cost[p, i, slot]: it writes sim
// when the candidate is in the grid and -inf when it is not.  There is no fill pass.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC_HD __host__ __device__ inline
#else
#define LC_HD inline
#endif

namespace vdr {

constexpr int LC_PH = 8;            // panel height
constexpr int LC_PW = 16;           // panel width (a power of two: the kernel splits a panel row with a shift)
constexpr int LC_TILE = 128;        // rows of a panel, rows of a halo tile
constexpr int LC_MAX_RADIUS = 8;    // VDR_LOCAL_CORR_MAX_RADIUS (include/vdr.h)
static_assert(LC_PH * LC_PW == LC_TILE, "a panel is one A operand");

struct LcGeom {
  int gh, gw, r, W;       // grid, radius, window side 2r + 1
  int npy, npx, npanels;  // panels down, across, all
  int hh, hw, ntiles;     // halo height and width, halo tiles per panel
};

LC_HD LcGeom lc_geom(int gh, int gw, int r) {
  LcGeom g;
  g.gh = gh, g.gw = gw, g.r = r, g.W = 2 * r + 1;
  g.npy = (gh + LC_PH - 1) / LC_PH;
  g.npx = (gw + LC_PW - 1) / LC_PW;
  g.npanels = g.npy * g.npx;
  g.hh = LC_PH + 2 * r;
  g.hw = LC_PW + 2 * r;
  g.ntiles = (g.hh * g.hw + LC_TILE - 1) / LC_TILE;
  return g;
}

struct LcPos {
  int y, x;   // the position the row stands for (unclamped)
  int src;    // the row to load, in [0, gh * gw)
  bool ok;    // the position counts: inside the grid (and, for a candidate, inside the halo)
};

LC_HD int lc_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

LC_HD LcPos lc_map(const LcGeom& g, int panel, int tile, int side, int row) {
  const int py = panel / g.npx, px = panel - py * g.npx;
  LcPos p;
  bool inside = true;
  if (side == 0) {
    p.y = py * LC_PH + row / LC_PW;
    p.x = px * LC_PW + row % LC_PW;
  } else {
    const int h = tile * LC_TILE + row;
    const int hy = h / g.hw, hx = h - hy * g.hw;
    inside = hy < g.hh;
    p.y = py * LC_PH - g.r + hy;
    p.x = px * LC_PW - g.r + hx;
  }
  p.ok = inside && p.y >= 0 && p.y < g.gh && p.x >= 0 && p.x < g.gw;
  p.src = lc_clamp(p.y, g.gh - 1) * g.gw + lc_clamp(p.x, g.gw - 1);
  return p;
}

LC_HD int lc_slot(const LcGeom& g, int qy, int qx, int cy, int cx) {
  const int dy = cy - qy, dx = cx - qx;
  if (dy < -g.r || dy > g.r || dx < -g.r || dx > g.r) return -1;
  return (dy + g.r) * g.W + (dx + g.r);
}

}  // namespace vdr
