// The ONE index arithmetic of the k-nearest-neighbour op (knn.hip; the definition is vdr_op_knn's in include/vdr.h): every
// offset the three kernels and the launch form -- operand rows, the norm arrays, the partial lists, the outputs --, the work
// item -> (pair, run, panel) mapping, the tiles of a run and the size of `work`.  The kernels, the launch and the host program
// tests/knn_map_cases.cpp all call it; it includes nothing and compiles as plain C++, so every address can be walked without
// a device.
//
//   queries    X_p [tq, d], cut into npanels panels of 128 rows (the B operand of the tile of desc_tile.h)
//   candidates Y_p [tc, d], cut into ntiles tiles of 128 rows (the A operand); the tiles of a (pair, panel) are cut into
//              nsplit runs (knn_split: run_split of desc_tile.h restated, checked equal at the launch)
//   work item  (pair, run, panel), panel fastest, handed out in XCD-contiguous order (knn_item restates xcd_remap of vdr_dev.h)
//   work       [ nq: pairs x tq_pad | nc: pairs x tc_pad | pkey | pidx ] in 4-byte elements; nq / nc hold rn (cosine) or ss (l2)
//   partials   pkey / pidx [pair][run][sub = 4][slot = k][tq]: the k best of query q among the candidates that wave row wr and
//              lane half hh of the item saw (sub = 2 wr + hh), best first; q fastest, so a half wave stores 128 contiguous bytes
//   outputs    val / idx [pair][tq][k]
// A row past the end of a map loads the map's last row (knn_src_row): no address is ever formed from an unclamped row.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KNN_HD __host__ __device__ inline
#else
#define KNN_HD inline
#endif

namespace vdr {

constexpr int KNN_TILE = 128;          // rows of a panel, rows of a candidate tile
constexpr int KNN_MAX_K = 16;          // VDR_KNN_MAX_K (include/vdr.h)
constexpr int KNN_SUBS = 4;            // partial lists per (query, run): wave row x lane half
constexpr int KNN_TARGET_ITEMS = 512;  // COS_TARGET_ITEMS of desc_tile.h

struct KnnPlan {
  int pairs, tq, tc, k;
  int npanels, ntiles, tq_pad, tc_pad;
  int nsplit, base, rem;  // runs per (pair, panel); run `split` takes base tiles, the first rem runs one more
  long long items;        // pairs * nsplit * npanels work items
  long long off_nq, off_nc, off_pkey, off_pidx, total;  // sections of work, in 4-byte elements, each a multiple of 4
};

KNN_HD void knn_split(long long items, long long ntiles, int& nsplit, int& base, int& rem) {
  long long n = KNN_TARGET_ITEMS / items;
  n = n < 1 ? 1 : n > ntiles ? ntiles : n;
  nsplit = (int)n, base = (int)(ntiles / n), rem = (int)(ntiles % n);
}

// (pairs, tq, tc, k all positive, k <= KNN_MAX_K: the entry point refuses the rest)
KNN_HD KnnPlan knn_plan(int pairs, int tq, int tc, int k) {
  KnnPlan pl;
  pl.pairs = pairs, pl.tq = tq, pl.tc = tc, pl.k = k;
  pl.npanels = (int)(((long long)tq + KNN_TILE - 1) / KNN_TILE);
  pl.ntiles = (int)(((long long)tc + KNN_TILE - 1) / KNN_TILE);
  pl.tq_pad = pl.npanels * KNN_TILE;
  pl.tc_pad = pl.ntiles * KNN_TILE;
  knn_split((long long)pairs * pl.npanels, pl.ntiles, pl.nsplit, pl.base, pl.rem);
  pl.items = (long long)pairs * pl.nsplit * pl.npanels;
  const long long part = ((long long)pairs * pl.nsplit * KNN_SUBS * k * tq + 3) / 4 * 4;
  pl.off_nq = 0;
  pl.off_nc = pl.off_nq + (long long)pairs * pl.tq_pad;
  pl.off_pkey = pl.off_nc + (long long)pairs * pl.tc_pad;
  pl.off_pidx = pl.off_pkey + part;
  pl.total = pl.off_pidx + part;
  return pl;
}

KNN_HD long long knn_work_elems(int pairs, int tq, int tc, int k) { return knn_plan(pairs, tq, tc, k).total; }

// workgroup `block` of `nblocks` -> work item: the permutation of xcd_remap (workgroups go round-robin over the 8 XCDs; each XCD
// gets a contiguous range of items), then (pair, run, panel) with the panel fastest
struct KnnItem {
  int p, split, panel;
};
KNN_HD int knn_xcd_order(int block, int nblocks) {
  const int xcd = block & 7;
  const int q = nblocks >> 3, r = nblocks & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (block >> 3);
}
KNN_HD KnnItem knn_item(const KnnPlan& pl, int block, int nblocks) {
  const int vid = knn_xcd_order(block, nblocks);
  const int ps = vid / pl.npanels;
  KnnItem it;
  it.panel = vid - ps * pl.npanels;
  it.p = ps / pl.nsplit;
  it.split = ps - it.p * pl.nsplit;
  return it;
}

// the candidate tiles jt0 .. jt1-1 of run `split`
KNN_HD void knn_run(const KnnPlan& pl, int split, int& jt0, int& jt1) {
  jt0 = split * pl.base + (split < pl.rem ? split : pl.rem);
  jt1 = jt0 + pl.base + (split < pl.rem ? 1 : 0);
}

// the row to LOAD for row r (0..127) of block `blk` (a panel or a tile) of a map of t rows: clamped, always in [0, t)
KNN_HD int knn_src_row(int blk, int r, int t) {
  const long long row = (long long)blk * KNN_TILE + r;
  return row < t ? (int)row : t - 1;
}
// element offset of row `row` of problem p: rows ld elements apart, problems ps apart
KNN_HD long long knn_row_off(int p, long long ps, int row, long long ld) { return (long long)p * ps + (long long)row * ld; }
// element of a norm array [pairs][t_pad]: row r of block blk (always inside the padding, whatever r)
KNN_HD long long knn_norm_off(int p, int t_pad, int blk, int r) { return (long long)p * t_pad + (long long)blk * KNN_TILE + r; }
// element of pkey / pidx
KNN_HD long long knn_part_off(const KnnPlan& pl, int p, int split, int sub, int slot, int q) {
  return ((((long long)p * pl.nsplit + split) * KNN_SUBS + sub) * pl.k + slot) * pl.tq + q;
}
// element of val / idx
KNN_HD long long knn_out_off(const KnnPlan& pl, int p, int q, int slot) { return ((long long)p * pl.tq + q) * pl.k + slot; }

}  // namespace vdr
