// Host-only walk of the index arithmetic of the k-nearest-neighbour op (csrc/knn_map.h), the one header the three kernels of
// csrc/knn.hip, their launch and this program share.  For every case it goes through all workgroups of the tile kernel, all
// threads of the merge and all rows of the norm pass, forms every offset exactly as the kernels do, and checks:
//   * the workgroups map one-to-one onto the (pair, run, panel) items;
//   * every candidate tile of every (pair, panel) belongs to exactly one run;
//   * every row the staging loads is in [0, t) and every 16-byte chunk it copies lies inside that row's d channels, inside the
//     extent the entry point promises for the operand: (pairs - 1) * stride + (t - 1) * ld + d elements;
//   * every norm element written or copied lies inside its section of `work`, the sections are 16-byte aligned, do not overlap
//     and end at vdr_knn_work_bytes;
//   * every partial slot of a query < tq is written once (tile kernel) and read once (merge), inside its section;
//   * every output slot has exactly one writer, inside pairs * tq * k.
// The chunk a lane copies within a row is t128_dma_chunk of csrc/desc_tile.h (device code), restated in dma_chunk below.
// Prints one line per case; exits 1 on the first violation.  Built and run by tests/test_knn_op_cpu.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "knn_map.h"

using namespace vdr;

struct Case {
  int pairs, tq, tc, d, k;
  long long ldx, xs, ldy, ys;  // strides in elements; -1: packed (ld = d, stride = t * ld)
};

static int fail(const Case& c, const char* what, long long a, long long b) {
  std::printf("FAIL %dx%dx%d d=%d k=%d: %s (%lld, %lld)\n", c.pairs, c.tq, c.tc, c.d, c.k, what, a, b);
  return 1;
}

// rows of a staged tile that (wave, lane) copies, and the chunk of the K step: desc_tile.h's t128_dma_row / t128_dma_chunk
static int dma_row(int wave, int lane, int q) { return (wave * 4 + q) * 8 + (lane >> 3); }
static int dma_chunk(int lane, int r, bool shortk) {
  const int c = (lane & 7) ^ ((r >> 1) & 7);
  return shortk ? c & 3 : c;
}

static int run_case(Case c) {
  if (c.ldx < 0) c.ldx = c.d;
  if (c.ldy < 0) c.ldy = c.d;
  if (c.xs < 0) c.xs = (long long)c.tq * c.ldx;
  if (c.ys < 0) c.ys = (long long)c.tc * c.ldy;
  const KnnPlan pl = knn_plan(c.pairs, c.tq, c.tc, c.k);
  const long long x_extent = (c.pairs - 1) * c.xs + (c.tq - 1) * c.ldx + c.d, y_extent = (c.pairs - 1) * c.ys + (c.tc - 1) * c.ldy + c.d;
  const long long part = pl.off_pidx - pl.off_pkey, outs = (long long)c.pairs * c.tq * c.k;
  // ---- the sections of work
  if (pl.off_nq != 0 || pl.off_nc - pl.off_nq != (long long)c.pairs * pl.tq_pad || pl.off_pkey - pl.off_nc != (long long)c.pairs * pl.tc_pad ||
      pl.total - pl.off_pidx != part || part < (long long)c.pairs * pl.nsplit * KNN_SUBS * c.k * c.tq)
    return fail(c, "sections of work", pl.off_nc, pl.off_pkey);
  if ((pl.off_nc | pl.off_pkey | pl.off_pidx | pl.total) & 3) return fail(c, "a section is not 16-byte aligned", pl.off_pidx, pl.total);
  if (knn_work_elems(c.pairs, c.tq, c.tc, c.k) != pl.total) return fail(c, "work size", pl.total, 0);
  if (pl.nsplit < 1 || pl.nsplit > pl.ntiles || (long long)pl.nsplit * pl.base + pl.rem != pl.ntiles || pl.rem >= pl.nsplit)
    return fail(c, "run split", pl.nsplit, pl.ntiles);
  if (pl.items != (long long)c.pairs * pl.nsplit * pl.npanels || pl.items > INT32_MAX) return fail(c, "items", pl.items, 0);

  // ---- the norm pass: one wave per row writes element i of its map
  for (int side = 0; side < 2; ++side) {
    const int t = side ? c.tc : c.tq, t_pad = side ? pl.tc_pad : pl.tq_pad;
    for (int p = 0; p < c.pairs; ++p)
      for (int i = 0; i < t; i += (t > 4096 ? 97 : 1)) {  // (affine in i: long maps are sampled, both ends included below)
        for (int ii : {i, t - 1}) {
          const long long src = knn_row_off(p, side ? c.ys : c.xs, ii, side ? c.ldy : c.ldx);
          if (src < 0 || src + c.d > (side ? y_extent : x_extent)) return fail(c, "norm pass reads outside the operand", src, ii);
          const long long o = knn_norm_off(p, t_pad, 0, ii);
          if (o < 0 || o >= (long long)c.pairs * t_pad) return fail(c, "norm element outside its section", o, ii);
        }
      }
  }

  // ---- the tile kernel
  std::vector<uint8_t> item_seen((size_t)pl.items, 0), written((size_t)part, 0), read((size_t)part, 0), out((size_t)outs, 0);
  std::vector<uint8_t> tile_seen((size_t)c.pairs * pl.npanels * pl.ntiles, 0);
  const int nk = (c.d + 63) / 64;
  long long stores = 0;
  for (long long b = 0; b < pl.items; ++b) {
    const KnnItem it = knn_item(pl, (int)b, (int)pl.items);
    if (it.p < 0 || it.p >= c.pairs || it.split < 0 || it.split >= pl.nsplit || it.panel < 0 || it.panel >= pl.npanels)
      return fail(c, "item outside the grid of items", b, it.p);
    const long long id = ((long long)it.p * pl.nsplit + it.split) * pl.npanels + it.panel;
    if (++item_seen[(size_t)id] > 1) return fail(c, "two workgroups on one item", b, id);
    int jt0, jt1;
    knn_run(pl, it.split, jt0, jt1);
    if (jt0 < 0 || jt1 <= jt0 || jt1 > pl.ntiles) return fail(c, "run outside the tiles", jt0, jt1);
    for (int jt = jt0; jt < jt1; ++jt) {
      if (++tile_seen[((size_t)it.p * pl.npanels + it.panel) * pl.ntiles + jt] > 1) return fail(c, "a tile in two runs", it.panel, jt);
      for (int wave = 0; wave < 4; ++wave)
        for (int lane = 0; lane < 64; ++lane) {
          for (int q = 0; q < 4; ++q) {
            const int r = dma_row(wave, lane, q);
            const int xr = knn_src_row(it.panel, r, c.tq), yr = knn_src_row(jt, r, c.tc);
            if (xr < 0 || xr >= c.tq || yr < 0 || yr >= c.tc) return fail(c, "source row outside its map", xr, yr);
            for (int kk = 0; kk < nk; ++kk) {
              const int col = kk * 64 + dma_chunk(lane, r, c.d - kk * 64 < 64) * 8;
              if (col < 0 || col + 8 > c.d) return fail(c, "chunk outside the row's d channels", col, c.d);
              const long long xo = knn_row_off(it.p, c.xs, 0, c.ldx) + knn_row_off(0, 0, xr, c.ldx) + col;
              const long long yo = knn_row_off(it.p, c.ys, 0, c.ldy) + knn_row_off(0, 0, yr, c.ldy) + col;
              if (xo < 0 || xo + 8 > x_extent) return fail(c, "query chunk outside the operand", xo, x_extent);
              if (yo < 0 || yo + 8 > y_extent) return fail(c, "candidate chunk outside the operand", yo, y_extent);
            }
          }
          if (wave == 0) {  // the 16-byte copy of four norms
            const long long o = lane < 32 ? knn_norm_off(it.p, pl.tc_pad, jt, lane * 4) : knn_norm_off(it.p, pl.tq_pad, it.panel, (lane - 32) * 4);
            const long long sec = (long long)c.pairs * (lane < 32 ? pl.tc_pad : pl.tq_pad);
            if (o < 0 || o + 4 > sec || (o & 3)) return fail(c, "norm copy outside its section or unaligned", o, sec);
          }
        }
    }
    // the item's partial lists: lane (wc, n, l31) owns query column wc * 64 + n * 32 + l31, list sub = 2 wr + hh
    for (int col = 0; col < KNN_TILE; ++col) {
      const int gq = it.panel * KNN_TILE + col;
      if (gq >= c.tq) continue;
      for (int sub = 0; sub < KNN_SUBS; ++sub)
        for (int slot = 0; slot < c.k; ++slot) {
          const long long o = knn_part_off(pl, it.p, it.split, sub, slot, gq);
          if (o < 0 || o >= part) return fail(c, "partial slot outside its section", o, part);
          if (++written[(size_t)o] > 1) return fail(c, "a partial slot with two writers", o, gq);
          ++stores;
        }
    }
  }
  for (size_t i = 0; i < item_seen.size(); ++i)
    if (item_seen[i] != 1) return fail(c, "an item without a workgroup", (long long)i, 0);
  for (size_t i = 0; i < tile_seen.size(); ++i)
    if (tile_seen[i] != 1) return fail(c, "a tile in no run", (long long)i, 0);

  // ---- the merge: four threads per (pair, query), list l read by thread l % 4 -- every list by exactly one of them
  for (int p = 0; p < c.pairs; ++p)
    for (int q = 0; q < c.tq; ++q) {
      for (int l = 0; l < pl.nsplit * KNN_SUBS; ++l)
        for (int s = 0; s < c.k; ++s) {
          const long long o = knn_part_off(pl, p, l / KNN_SUBS, l % KNN_SUBS, s, q);
          if (o < 0 || o >= part) return fail(c, "merge reads outside the partials", o, part);
          if (++read[(size_t)o] > 1) return fail(c, "a partial slot with two readers", o, q);
          if (written[(size_t)o] != 1) return fail(c, "merge reads a slot nobody wrote", o, q);
        }
      for (int s = 0; s < c.k; ++s) {
        const long long o = knn_out_off(pl, p, q, s);
        if (o < 0 || o >= outs) return fail(c, "output slot outside pairs * tq * k", o, outs);
        if (++out[(size_t)o] > 1) return fail(c, "an output slot with two writers", o, q);
      }
    }
  for (long long o = 0; o < part; ++o)
    if (written[(size_t)o] != read[(size_t)o]) return fail(c, "a partial slot written but never read", o, written[(size_t)o]);
  for (long long o = 0; o < outs; ++o)
    if (out[(size_t)o] != 1) return fail(c, "an output slot without a writer", o, 0);
  std::printf("ok %dx%dx%d d=%d k=%d ld=%lld/%lld stride=%lld/%lld: panels %d tiles %d runs %d items %lld, %lld partial slots, %lld outputs, work %lld bytes\n",
              c.pairs, c.tq, c.tc, c.d, c.k, c.ldx, c.ldy, c.xs, c.ys, pl.npanels, pl.ntiles, pl.nsplit, pl.items, stores, outs, pl.total * 4);
  return 0;
}

int main() {
  std::vector<Case> cases;
  // the ragged small shapes of tests/test_knn_gpu.py: tq x tc x d x k x pairs
  for (int tq : {1, 127, 129, 300})
    for (int tc : {16, 64, 129, 700})
      for (int d : {32, 96, 448})
        for (int pairs : {1, 3}) cases.push_back({pairs, tq, tc, d, tc == 16 ? 16 : (tq % 2 ? 5 : 9), -1, -1, -1, -1});
  for (int k : {1, 4, 5, 8, 9, 16}) {
    cases.push_back({3, 300, 700, 96, k, -1, -1, -1, -1});
    cases.push_back({3, 129, k, 32, k, -1, -1, -1, -1});  // tc == k: every candidate is returned
  }
  cases.push_back({5, 300, 700, 64, 5, -1, -1, -1, -1});   // problem 3 of 5: another split count
  cases.push_back({1, 257, 700, 64, 16, -1, -1, -1, -1});
  // the benchmark ladder
  cases.push_back({64, 196, 196, 768, 16, -1, -1, -1, -1});
  cases.push_back({32, 729, 729, 768, 16, -1, -1, -1, -1});
  cases.push_back({1, 3969, 3969, 768, 16, -1, -1, -1, -1});
  cases.push_back({8, 3969, 3969, 768, 16, -1, -1, -1, -1});  // cosine and l2 share every index: the metric changes no address
  cases.push_back({8, 3969, 3969, 768, 1, -1, -1, -1, -1});
  cases.push_back({1, 1024, 65536, 768, 16, -1, -1, -1, -1});
  cases.push_back({1, 8192, 8192, 384, 16, -1, -1, -1, -1});
  // strides of 0 and ld > d: a bank under every query set, a facet inside a 3 d wide buffer
  cases.push_back({3, 300, 700, 64, 5, -1, -1, -1, 0});
  cases.push_back({3, 300, 700, 64, 5, 192, -1, 192, -1});
  cases.push_back({4, 129, 129, 96, 8, 288, 0, 288, 0});
  for (const Case& c : cases)
    if (run_case(c)) return 1;
  std::printf("cases %zu\n", cases.size());
  return 0;
}
