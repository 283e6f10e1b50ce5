// Host program (its own main) over csrc/edt3d_map.h (and csrc/edt_map.h, whose row pass is the x pass), the mapping and the searches
// the 3-D distance-transform kernels (csrc/edt3d.hip) are written on.  For every shape it checks that each pass owns every voxel
// exactly once and that the workspace sections hold what is indexed; and it RUNS the three passes -- the very functions the kernels
// call -- plane by plane, tile by tile, thread by thread, in forward and in reversed order, in arrays of exactly the promised
// extents (the sanitized build turns an index outside them into a failed run), against brute force and against the separable form
// without any early stop: d2 and the peak through the partial slots, for all eight `outside` masks, for the set and for the clear
// voxels, under several spacings.  Every search is held to its step cap max(c, side - 1 - c).  The threshold-only early exits must
// give the same `within` as the full search at every r2 tried; the exit that would NOT be exact (the y search stopping at
// best <= r2) is shown to be wrong on a designed volume.  Built and run by tests/test_edt3d_cpu.py, once plainly and once with
// -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>

#include "edt3d_map.h"

using namespace vdr;

static long long fails = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (fails++ < 10) std::printf("FAIL %s (line %d)\n", #cond, __LINE__);   \
    }                                                                          \
  } while (0)

static uint32_t rng_state = 2024u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static std::vector<uint8_t> pattern(int kind, int Z, int H, int W) {
  const size_t n = (size_t)Z * H * W;
  std::vector<uint8_t> m(n, 1);
  auto clear = [&](int z, int y, int x) { m[((size_t)z * H + y) * W + x] = 0; };
  switch (kind) {
    case 0: m.assign(n, 0); break;                             // empty
    case 1: break;                                             // full
    case 2: clear(0, 0, 0); break;                             // one clear voxel in a corner: the deepest searches
    case 3: clear(Z / 2, H / 2, W / 2); break;
    case 4:                                                    // checkerboard
      for (int z = 0; z < Z; ++z)
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) m[((size_t)z * H + y) * W + x] = (x + y + z) & 1;
      break;
    case 5:
    case 6:                                                    // Bernoulli 0.5 and 0.97
      for (auto& v : m) v = rnd() % 100 < (kind == 5 ? 50u : 97u);
      break;
    case 7:                                                    // a clear slab in the middle slice and a clear voxel at the far corner
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) clear(Z / 2, y, x);
      clear(Z - 1, H - 1, W - 1);
      break;
    default:                                                   // the eight corners
      for (int c = 0; c < 8; ++c) clear(c & 4 ? Z - 1 : 0, c & 2 ? H - 1 : 0, c & 1 ? W - 1 : 0);
      break;
  }
  return m;
}
constexpr int KINDS = 9;

// ---- the references -----------------------------------------------------------------------------------------------------------------
static long long sq(long long q, long long o) { return q * o * q * o; }

static void brute(const std::vector<uint8_t>& sel, int Z, int H, int W, const int q[3], int outside, std::vector<long long>& d2) {
  const int n = Z * H * W;
  std::vector<int> c;
  for (int i = 0; i < n; ++i)
    if (!sel[i]) c.push_back(i);
  d2.assign((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    if (!sel[i]) continue;
    const int z = i / (H * W), y = i / W % H, x = i % W;
    long long best = EDT3_NONE;
    for (int j : c) {
      const long long d = sq(q[0], z - j / (H * W)) + sq(q[1], y - j / W % H) + sq(q[2], x - j % W);
      best = d < best ? d : best;
    }
    if (outside & 4) best = std::min(best, std::min(sq(q[0], z + 1), sq(q[0], Z - z)));
    if (outside & 2) best = std::min(best, std::min(sq(q[1], y + 1), sq(q[1], H - y)));
    if (outside & 1) best = std::min(best, std::min(sq(q[2], x + 1), sq(q[2], W - x)));
    d2[i] = best;
  }
}

// the separable form without any early stop: one axis after the other, every candidate of the line
static void separable(const std::vector<uint8_t>& sel, int Z, int H, int W, const int q[3], int outside, std::vector<long long>& d2) {
  const int n = Z * H * W;
  const long long INF = 1ll << 61;
  std::vector<long long> f((size_t)n), t((size_t)n);
  for (int i = 0; i < n; ++i) f[i] = sel[i] ? INF : 0;
  const int side[3] = {Z, H, W}, stride[3] = {H * W, W, 1}, bit[3] = {4, 2, 1};
  for (int a = 2; a >= 0; --a) {
    for (int i = 0; i < n; ++i) {
      const int c = i / stride[a] % side[a], base = i - c * stride[a];
      long long best = INF;
      for (int cc = 0; cc < side[a]; ++cc) best = std::min(best, f[base + cc * stride[a]] + sq(q[a], c - cc));
      if (outside & bit[a]) best = std::min(best, std::min(sq(q[a], c + 1), sq(q[a], side[a] - c)));
      t[i] = best < INF ? best : INF;
    }
    f.swap(t);
  }
  d2.assign((size_t)n, 0);
  for (int i = 0; i < n; ++i) d2[i] = !sel[i] ? 0 : f[i] >= INF ? EDT3_NONE : f[i];
}

// ---- ownership and extents ----------------------------------------------------------------------------------------------------------
static void walk_geometry(int Z, int H, int W) {
  for (int P : {1, 3}) {
    CHECK(edt3_shape_ok(P, Z, H, W));
    const Edt3Geom q = edt3_geom(P, Z, H, W, 1, 1, 1, 0);
    CHECK(q.pl.P == P * Z && q.pl.H == H && q.pl.W == W && q.ztiles == Z * q.pl.ctiles);
    const Edt3Work w = edt3_work(P, Z, H, W);
    const long long n = (long long)P * Z * H * W;
    CHECK(w.g == 0 && w.vec >= 2 * n && w.vec % 16 == 0 && w.vec < 2 * n + 16);
    CHECK(w.slots >= w.vec + 4 * n && w.slots % 16 == 0 && w.slots < w.vec + 4 * n + 16);
    CHECK(w.slots + 8 * (edt3_slot(q, P - 1, Z - 1, q.pl.ctiles - 1) + 2) == w.bytes);
    // the tiles of the y and the z pass own every voxel of every slice once; the slots are distinct
    std::vector<int> own((size_t)H * W, 0);
    for (int t = 0; t < q.pl.ctiles; ++t)
      for (int tid = 0; tid < EDT_THREADS; ++tid)
        for (int j = 0; j < EDT_CROWS; ++j) {
          int y, x;
          edt_col_owner(q.pl, t, tid, j, &y, &x);
          if (x < W && y < H) ++own[(size_t)y * W + x];
        }
    long long bad = 0;
    for (int v : own) bad += v != 1;
    CHECK(bad == 0);
    std::vector<char> seen((size_t)P * q.ztiles, 0);
    for (int v = 0; v < P; ++v)
      for (int z = 0; z < Z; ++z)
        for (int t = 0; t < q.pl.ctiles; ++t) {
          const long long s = edt3_slot(q, v, z, t);
          CHECK(s % 2 == 0 && s / 2 >= 0 && s / 2 < (long long)seen.size());
          if (s / 2 < (long long)seen.size()) CHECK(seen[(size_t)(s / 2)]++ == 0);
        }
  }
}

// ---- the passes themselves ------------------------------------------------------------------------------------------------------------
struct Run {
  std::vector<long long> d2;
  Edt3Peak peak;
  long long bad_steps = 0, ysteps = 0, zsteps = 0;
};

// thr < 0: the full search; y_exit_at_best: the exit the y search must NOT take, to show that it is wrong
static Run passes(const std::vector<uint8_t>& m, int Z, int H, int W, const int sp[3], int value, int outside, int rev, long long thr,
                  bool y_exit_at_best = false) {
  const Edt3Geom q = edt3_geom(1, Z, H, W, sp[0], sp[1], sp[2], outside);
  const int hw = H * W, n = Z * hw;
  Run out;
  std::vector<short> g((size_t)n, (short)0x5a5a);
  std::vector<short> row((size_t)EDT_RROWS * EDT_ROW_LDS);
  std::vector<int> sl(EDT_THREADS), sr(EDT_THREADS);
  for (int pz = 0; pz < Z; ++pz) {
    const int z = rev ? Z - 1 - pz : pz;
    for (int b = 0; b < q.pl.rblocks; ++b) {
      const int rb = rev ? q.pl.rblocks - 1 - b : b;
      row.assign(row.size(), (short)0x7b7b);  // stale LDS
      auto each = [&](auto f) {
        for (int k = 0; k < EDT_THREADS; ++k) f(rev ? EDT_THREADS - 1 - k : k);
      };
      each([&](int tid) { edt_row_load(q.pl, rb, m.data() + (size_t)z * hw, value, tid, row.data()); });
      each([&](int tid) { edt_row_summary(q.pl, rb, tid, row.data(), sl.data(), sr.data()); });
      each([&](int tid) { edt_row_scan(q.pl, rb, outside & 1, tid, row.data(), sl.data(), sr.data()); });
      each([&](int tid) { edt_row_store(q.pl, rb, tid, row.data(), g.data() + (size_t)z * hw); });
    }
  }
  std::vector<unsigned> vec((size_t)n, 0x5a5a5a5au);
  for (int pz = 0; pz < Z; ++pz) {
    const int z = rev ? Z - 1 - pz : pz;
    for (int b = 0; b < q.pl.ctiles; ++b) {
      const int t = rev ? q.pl.ctiles - 1 - b : b;
      for (int k = 0; k < EDT_THREADS; ++k) {
        const int tid = rev ? EDT_THREADS - 1 - k : k;
        for (int j = 0; j < EDT_CROWS; ++j) {
          int y, x;
          edt_col_owner(q.pl, t, tid, j, &y, &x);
          if (x >= W || y >= H) continue;
          Edt3Hit h = edt3_search_y(g.data() + (size_t)z * hw, H, W, y, x, q.qy, q.qx, (outside >> 1) & 1, thr);
          if (y_exit_at_best) {  // what a search that stopped at its first best <= thr would leave: the own row's candidate
            const int o = g[(size_t)z * hw + y * W + x];
            if (o != 0 && o != EDT_NO_ROW && edt3_sq(q.qx, o) <= thr) h.vec = edt3_pack(0, o);
          }
          vec[(size_t)z * hw + y * W + x] = h.vec;
          out.bad_steps += h.steps > (y > H - 1 - y ? y : H - 1 - y);
          out.ysteps += h.steps;
        }
      }
    }
  }
  out.d2.assign((size_t)n, -7);
  std::vector<long long> slots((size_t)2 * q.ztiles, 0x5a5a5a5a5a5all);
  for (int pz = 0; pz < Z; ++pz) {
    const int z = rev ? Z - 1 - pz : pz;
    for (int b = 0; b < q.pl.ctiles; ++b) {
      const int t = rev ? q.pl.ctiles - 1 - b : b;
      std::vector<Edt3Peak> pk(EDT_THREADS, edt3_peak_none());
      for (int k = 0; k < EDT_THREADS; ++k) {
        const int tid = rev ? EDT_THREADS - 1 - k : k;
        for (int j = 0; j < EDT_CROWS; ++j) {
          int y, x;
          edt_col_owner(q.pl, t, tid, j, &y, &x);
          if (x >= W || y >= H) continue;
          const Edt3Hit h = edt3_search_z(vec.data(), Z, hw, z, y * W + x, q.qz, q.qy, q.qx, (outside >> 2) & 1, thr);
          out.d2[(size_t)z * hw + y * W + x] = h.d2;
          out.bad_steps += h.steps > (z > Z - 1 - z ? z : Z - 1 - z);
          out.zsteps += h.steps;
          edt3_peak_take(&pk[tid], h.d2, (long long)z * hw + y * W + x);
        }
      }
      // the two-step reduction of the workgroup: the largest d2, then the largest index key among the threads that attain it
      long long top = 0;
      for (const Edt3Peak& p : pk) top = p.d2 > top ? p.d2 : top;
      unsigned long long key = 0;
      for (const Edt3Peak& p : pk) key = edt3_index_key(p, top) > key ? edt3_index_key(p, top) : key;
      const long long s = edt3_slot(q, 0, z, t);
      slots[(size_t)s] = top, slots[(size_t)s + 1] = edt3_index_of_key(key);
    }
  }
  // the finish kernel: 64 lanes over the slots, then the same two steps
  std::vector<Edt3Peak> lane(64, edt3_peak_none());
  for (int l = 0; l < 64; ++l)
    for (int t = l; t < q.ztiles; t += 64) edt3_peak_take(&lane[l], slots[2 * (size_t)t], slots[2 * (size_t)t + 1]);
  long long top = 0;
  for (const Edt3Peak& p : lane) top = p.d2 > top ? p.d2 : top;
  unsigned long long key = 0;
  for (const Edt3Peak& p : lane) key = edt3_index_key(p, top) > key ? edt3_index_key(p, top) : key;
  out.peak.d2 = top, out.peak.i = edt3_index_of_key(key);
  return out;
}

static const int SPACINGS[5][3] = {{1, 1, 1}, {3, 1, 1}, {1, 2, 5}, {2560, 717, 717}, {65535, 1, 300}};

static void run(int Z, int H, int W, int kind, const int sp[3], bool big) {
  const std::vector<uint8_t> m = pattern(kind, Z, H, W);
  const int n = Z * H * W;
  for (int value = 0; value < 2; ++value) {
    std::vector<uint8_t> sel(n);
    for (int i = 0; i < n; ++i) sel[i] = (m[i] != 0) == (value != 0);
    for (int outside = 0; outside < 8; ++outside) {
      if (big && outside != 0 && outside != 7 && outside != 4) continue;
      if (big && Z > 1000 && (outside != 0 || value == 0)) continue;  // the deepest search: the set voxels, nothing outside
      std::vector<long long> d0;
      separable(sel, Z, H, W, sp, outside, d0);
      if (n <= 700) {
        std::vector<long long> db;
        brute(sel, Z, H, W, sp, outside, db);
        CHECK(db == d0);
      }
      long long pd = 0, pi = -1;
      for (int i = 0; i < n; ++i)
        if (d0[i] > pd) pd = d0[i], pi = i;
      Run full;
      for (int rev = 0; rev < 2; ++rev) {
        if (big && rev) continue;
        const Run r = passes(m, Z, H, W, sp, value, outside, rev, -1);
        CHECK(r.d2 == d0);
        CHECK(r.peak.d2 == pd && r.peak.i == pi);
        CHECK(r.bad_steps == 0);
        if (!rev) full = r;
      }
      // threshold only: the same `within` as the full search, never more steps
      if (outside != 0 && outside != 7 && outside != 2 && outside != 5) continue;
      const long long r2s[] = {0, 1, (long long)sp[2] * sp[2], 4ll * sp[1] * sp[1] + sp[0], 9ll * sp[0] * sp[0], 1000000000000ll};
      for (long long r2 : r2s) {
        if (big && r2 != r2s[4] && (Z > 1000 || r2 != r2s[2])) continue;
        const Run r = passes(m, Z, H, W, sp, value, outside, 0, r2);
        long long bad = 0;
        for (int i = 0; i < n; ++i) bad += (r.d2[i] <= r2) != (d0[i] <= r2);
        CHECK(bad == 0);
        CHECK(r.bad_steps == 0 && r.ysteps <= full.ysteps && r.zsteps <= full.zsteps);
      }
    }
  }
}

// A 3 x 2 x 4 volume, all set but (z 0, y 0, x 3) and (z 0, y 1, x 0).  In slice 0 the voxel (0, 0, 0) has the in-plane value 1 (one
// step along y), but its own row offers 9 first (three steps along x).  At r2 = 9 a y search that stopped at best <= r2 would leave
// the 9, and the voxel (2, 0, 0), whose d2 is 4 + 1 = 5, would see 4 + 9 = 13 and be left outside.
static void the_exit_the_y_search_must_not_take() {
  const int Z = 3, H = 2, W = 4, sp[3] = {1, 1, 1};
  std::vector<uint8_t> m((size_t)Z * H * W, 1);
  m[0 * H * W + 0 * W + 3] = 0;  // (z 0, y 0, x 3): three steps along x from (0, 0, 0)
  m[0 * H * W + 1 * W + 0] = 0;  // (z 0, y 1, x 0): one step along y from (0, 0, 0)
  const long long r2 = 9;
  std::vector<uint8_t> sel = m;
  std::vector<long long> d0;
  brute(sel, Z, H, W, sp, 0, d0);
  CHECK(d0[2 * H * W] == 5);  // (2, 0, 0): 4 + 1
  const Run good = passes(m, Z, H, W, sp, 1, 0, 0, r2);
  const Run wrong = passes(m, Z, H, W, sp, 1, 0, 0, r2, true);
  long long bad_good = 0, bad_wrong = 0;
  for (int i = 0; i < Z * H * W; ++i) bad_good += (good.d2[i] <= r2) != (d0[i] <= r2), bad_wrong += (wrong.d2[i] <= r2) != (d0[i] <= r2);
  CHECK(bad_good == 0);
  CHECK(bad_wrong > 0);  // 4 + 9 > 9: the voxel would be left outside
  std::printf("y exit at best <= r2: %lld voxels wrong (the exit is not taken)\n", bad_wrong);
}

int main() {
  int cases = 0;
  auto shape = [&](int Z, int H, int W, bool big) {
    const long long before = fails;
    walk_geometry(Z, H, W);
    int used = 0;
    for (int s = 0; s < 5; ++s) {
      const int* sp = SPACINGS[s];
      if (!edt3_spacing_ok(Z, H, W, sp[0], sp[1], sp[2])) continue;
      if (big && s != (Z > 1000 ? 3 : Z > 50 ? 0 : 3)) continue;
      ++used;
      for (int kind = 0; kind < KINDS; ++kind)
        if (!big || kind == 2 || (kind == 6 && Z < 1000)) run(Z, H, W, kind, sp, big);
    }
    const Edt3Geom q = edt3_geom(1, Z, H, W, 1, 1, 1, 0);
    std::printf("Z %d H %d W %d: ctiles %d ztiles %d spacings %d fails %lld\n", Z, H, W, q.pl.ctiles, q.ztiles, used, fails - before);
    ++cases;
  };
  shape(1, 1, 1, false);
  shape(1, 6, 7, false);
  shape(7, 1, 5, false);
  shape(2, 2, 2, false);
  shape(5, 9, 13, false);
  shape(3, 17, 16, false);
  shape(9, 5, 4, false);    // every k of the z search's rounds of EDT3_U on both sides
  shape(2, 17, 65, false);  // two tiles across, two down
  shape(33, 24, 19, true);
  shape(40, 5, 130, true);
  shape(4096, 1, 2, true);  // the search depth at its limit
  the_exit_the_y_search_must_not_take();
  // the limits
  CHECK(!edt3_shape_ok(1, 4097, 1, 1) && !edt3_shape_ok(1, 1, 0, 1) && !edt3_shape_ok(16, 4096, 1, 1) && edt3_shape_ok(15, 4096, 1, 1));
  CHECK(edt3_shape_ok(1, 1024, 1024, 1024) && !edt3_shape_ok(1, 1025, 1024, 1024) && !edt3_shape_ok(0, 1, 1, 1));
  CHECK(edt3_spacing_ok(4096, 1, 2, 2560, 717, 717) && !edt3_spacing_ok(4096, 1, 2, 65535, 1, 300) && !edt3_spacing_ok(1, 1, 1, 0, 1, 1));
  CHECK(!edt3_spacing_ok(1, 1, 1, 1, 65536, 1) && edt3_spacing_ok(1, 1, 1, 65535, 65535, 65535));
  // 94906265^2 is the first square above 2^53
  CHECK(edt3_spacing_ok(1445, 1, 1, 65535, 1, 1) && !edt3_spacing_ok(1449, 1, 1, 65535, 1, 1));
  CHECK(edt3_sq(65535, 4099) == 65535ll * 4099 * 65535 * 4099 && edt3_sq(7, -3) == 441);
  CHECK(edt3_oy(edt3_pack(-4096, 4096)) == -4096 && edt3_ox(edt3_pack(-4096, 4096)) == 4096 && edt3_ox(edt3_pack(0, EDT_NO_ROW)) == EDT_NO_ROW);
  CHECK(edt3_g2(2, 3, edt3_pack(-2, 5)) == 16 + 225 && edt3_g2(1, 1, 0) == 0 && edt3_g2(1, 1, edt3_pack(0, EDT_NO_ROW)) == EDT3_NONE);
  {
    Edt3Peak p = edt3_peak_none();
    edt3_peak_take(&p, 0, 5);
    CHECK(p.i == -1);
    edt3_peak_take(&p, EDT3_NONE, (1ll << 30) - 1);
    edt3_peak_take(&p, EDT3_NONE, 0);
    edt3_peak_take(&p, 7, -1);
    CHECK(p.d2 == EDT3_NONE && p.i == 0 && edt3_index_of_key(edt3_index_key(p, EDT3_NONE)) == 0 && edt3_index_key(p, 5) == 0);
    CHECK(edt3_index_of_key(0) == -1);
  }
  std::printf("cases %d fails %lld\n", cases, fails);
  return fails ? 1 : 0;
}
