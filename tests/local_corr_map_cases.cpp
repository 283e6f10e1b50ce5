// Host-only check of the mapping of the windowed correlation (csrc/local_corr_map.h), the one function the kernel, its launch
// plan and this program share.  For every (gh, gw, r) of the list it walks all work items (pair, panel, tile) and all 128 x 128
// (query row, candidate row) elements of each, exactly as the kernel's epilogue does, and checks:
//   * every source row the staging would load is in [0, t), on both sides, whatever the position;
//   * every (in-grid query, window slot) is met by exactly one element of exactly one item -- its owner, which stores sim when
//     the candidate is in the grid and -inf when it is not -- so every entry of cost has one writer and none is left out;
//   * where the candidate counts, it IS the candidate of that slot by the definition: j = (qy + dy) * gw + (qx + dx);
//     where it does not, the definition's position is outside the grid;
//   * every offset into cost is inside pairs * t * W * W;
//   * the halo tiles per panel are 2, 2, 3 and 6 at r = 1, 2, 4 and 8.
// Prints one line per case; exits 1 on the first violation.  Built and run by tests/test_local_correlation_cpu.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "local_corr_map.h"

using namespace vdr;

static int fail(const char* what, int gh, int gw, int r, long a, long b) {
  std::printf("FAIL %dx%d r=%d: %s (%ld, %ld)\n", gh, gw, r, what, a, b);
  return 1;
}

static int run_case(int gh, int gw, int r, int pairs) {
  const LcGeom g = lc_geom(gh, gw, r);
  const int64_t t = (int64_t)gh * gw, WW = (int64_t)g.W * g.W, total = pairs * t * WW;
  std::vector<uint8_t> owners((size_t)total, 0);
  int64_t sims = 0, infs = 0;
  for (int p = 0; p < pairs; ++p)
    for (int panel = 0; panel < g.npanels; ++panel)
      for (int tile = 0; tile < g.ntiles; ++tile) {
        LcPos q[LC_TILE], c[LC_TILE];
        for (int row = 0; row < LC_TILE; ++row) {
          q[row] = lc_map(g, panel, tile, 0, row);
          c[row] = lc_map(g, panel, tile, 1, row);
          if (q[row].src < 0 || q[row].src >= t) return fail("query source row outside [0, t)", gh, gw, r, q[row].src, row);
          if (c[row].src < 0 || c[row].src >= t) return fail("candidate source row outside [0, t)", gh, gw, r, c[row].src, row);
          if (q[row].ok && q[row].src != q[row].y * gw + q[row].x) return fail("an in-grid query does not load its own row", gh, gw, r, row, 0);
          if (c[row].ok && c[row].src != c[row].y * gw + c[row].x) return fail("an in-grid candidate does not load its own row", gh, gw, r, row, 0);
        }
        for (int qr = 0; qr < LC_TILE; ++qr)
          for (int cr = 0; cr < LC_TILE; ++cr) {
            const int slot = lc_slot(g, q[qr].y, q[qr].x, c[cr].y, c[cr].x);
            if (!q[qr].ok || slot < 0) continue;
            if (slot >= WW) return fail("slot past the window", gh, gw, r, slot, WW);
            const int64_t off = ((int64_t)p * t + q[qr].src) * WW + slot;
            if (off < 0 || off >= total) return fail("offset outside cost", gh, gw, r, (long)off, (long)total);
            if (++owners[(size_t)off] > 1) return fail("a (query, slot) with two owners", gh, gw, r, q[qr].src, slot);
            const int dy = slot / g.W - r, dx = slot % g.W - r;
            const int cy = q[qr].y + dy, cx = q[qr].x + dx;
            const bool in_grid = cy >= 0 && cy < gh && cx >= 0 && cx < gw;
            if (c[cr].ok != in_grid) return fail("in-grid flag disagrees with the definition", gh, gw, r, q[qr].src, slot);
            if (in_grid && c[cr].src != cy * gw + cx) return fail("not the candidate of this slot", gh, gw, r, c[cr].src, cy * gw + cx);
            in_grid ? ++sims : ++infs;
          }
      }
  for (int64_t o = 0; o < total; ++o)
    if (owners[(size_t)o] != 1) return fail("a (query, slot) without an owner", gh, gw, r, (long)(o / WW), (long)(o % WW));
  std::printf("ok %dx%d r=%d pairs=%d: panels %d tiles %d items %d, %lld sims + %lld -inf = %lld entries\n", gh, gw, r, pairs, g.npanels,
              g.ntiles, pairs * g.npanels * g.ntiles, (long long)sims, (long long)infs, (long long)total);
  return 0;
}

int main() {
  const int want_tiles[LC_MAX_RADIUS + 1] = {0, 2, 2, 3, 3, 4, 5, 6, 6};
  for (int r = 1; r <= LC_MAX_RADIUS; ++r)
    if (lc_geom(1, 1, r).ntiles != want_tiles[r]) return fail("halo tiles per panel", 1, 1, r, lc_geom(1, 1, r).ntiles, want_tiles[r]);
  // 1x1; one below, at and one above the 8 x 16 panel in each dimension; small and ragged grids; several panels both ways
  const int grids[][2] = {{1, 1}, {1, 5}, {3, 3}, {5, 7}, {7, 15}, {7, 16}, {7, 17}, {8, 15}, {8, 16}, {8, 17}, {9, 15}, {9, 16}, {9, 17},
                          {14, 14}, {17, 33}, {2, 40}, {40, 2}};
  for (const auto& gr : grids)
    for (int r : {1, 2, 4, 8})
      if (run_case(gr[0], gr[1], r, 2)) return 1;
  return 0;
}
