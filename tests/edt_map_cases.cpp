// Host program (its own main) over csrc/edt_map.h, the mapping and the search the distance-transform kernels (csrc/edt.hip) are
// written on.  For every shape it checks that each pass owns every pixel exactly once (the loads, the segments and the stores of
// the row pass, the tiles of the column pass), that a row's pixels fall on distinct LDS places inside the row's array, and that
// the workspace sections hold what is indexed; and it RUNS the passes -- the very functions the kernels call -- workgroup by
// workgroup, thread by thread, in forward and in reversed order, in arrays of exactly the promised extents (the sanitized build
// turns an index outside them into a failed run), against brute force: d2, nearest under the lowest-index rule, the peak through
// the partial slots, with and without `outside`, for the set and for the clear pixels.  Every search is held to its step cap
// max(y, H - 1 - y).  Built and run by tests/test_edt_cpu.py, once plainly and once with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>

#include "edt_map.h"

using namespace vdr;

static long long fails = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (fails++ < 10) std::printf("FAIL %s (line %d)\n", #cond, __LINE__);   \
    }                                                                          \
  } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

// the planes: what is SET; the transform is run on the set (value 1) and on the clear (value 0) pixels of each
static std::vector<uint8_t> pattern(int kind, int H, int W) {
  std::vector<uint8_t> m((size_t)H * W, 1);
  auto clear = [&](int y, int x) { m[(size_t)y * W + x] = 0; };
  switch (kind) {
    case 0: m.assign((size_t)H * W, 0); break;                 // empty
    case 1: break;                                             // full
    case 2: clear(0, 0); break;                                // one clear pixel in a corner: the deepest search
    case 3: clear(H / 2, W / 2); break;
    case 4:                                                    // checkerboard
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) m[(size_t)y * W + x] = (x + y) & 1;
      break;
    case 5:
    case 6:                                                    // Bernoulli 0.5 and 0.97
      for (auto& v : m) v = rnd() % 100 < (kind == 5 ? 50u : 97u);
      break;
    case 7:                                                    // a clear column at the right edge and a clear pixel at the origin
      for (int y = 0; y < H; ++y) clear(y, W - 1);
      clear(0, 0);
      break;
    default:                                                   // the four corners: ties along both axes
      clear(0, 0), clear(0, W - 1), clear(H - 1, 0), clear(H - 1, W - 1);
      break;
  }
  return m;
}
constexpr int KINDS = 9;

// ---- the reference ------------------------------------------------------------------------------------------------------------------
// brute force over every non-selected pixel, in index order with a strict comparison: the lowest index among the nearest
static void brute(const std::vector<uint8_t>& sel, int H, int W, int outside, std::vector<int>& d2, std::vector<int>& nearest) {
  std::vector<int> cy, cx;
  for (int i = 0; i < H * W; ++i)
    if (!sel[i]) cy.push_back(i / W), cx.push_back(i % W);
  d2.assign((size_t)H * W, 0), nearest.assign((size_t)H * W, -1);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int i = y * W + x;
      if (!sel[i]) continue;
      long long best = EDT_NONE;
      int bi = -1;
      for (size_t c = 0; c < cy.size(); ++c) {
        const long long d = (long long)(y - cy[c]) * (y - cy[c]) + (long long)(x - cx[c]) * (x - cx[c]);
        if (d < best) best = d, bi = cy[c] * W + cx[c];
      }
      if (outside) {
        const long long b[4] = {(long long)(y + 1) * (y + 1), (long long)(H - y) * (H - y), (long long)(x + 1) * (x + 1), (long long)(W - x) * (W - x)};
        for (long long v : b) best = v < best ? v : best;
      }
      d2[i] = (int)best, nearest[i] = bi;
    }
}

// for the large planes: the separable form without any early stop (every row of the column, the row distance by a walk both ways)
static void separable(const std::vector<uint8_t>& sel, int H, int W, int outside, std::vector<int>& d2, std::vector<int>& nearest) {
  std::vector<int> off((size_t)H * W, 0);
  std::vector<char> none((size_t)H * W, 0);
  for (int y = 0; y < H; ++y) {
    const uint8_t* s = sel.data() + (size_t)y * W;
    std::vector<int> left(W), right(W);
    int last = outside ? -1 : -EDT_FAR;
    for (int x = 0; x < W; ++x) last = s[x] ? last : x, left[x] = last;
    int next = outside ? W : EDT_FAR;
    for (int x = W - 1; x >= 0; --x) next = s[x] ? next : x, right[x] = next;
    for (int x = 0; x < W; ++x) {
      const int dl = x - left[x], dr = right[x] - x;
      off[(size_t)y * W + x] = dl <= dr ? -dl : dr;
      none[(size_t)y * W + x] = dl > 4096 && dr > 4096;
    }
  }
  d2.assign((size_t)H * W, 0), nearest.assign((size_t)H * W, -1);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int i = y * W + x;
      if (!sel[i]) continue;
      long long best = EDT_NONE;
      int bi = -1;
      for (int yy = 0; yy < H; ++yy) {  // rows in rising order, strict comparison: the lowest row, and in it the lower column
        if (none[(size_t)yy * W + x]) continue;
        const long long o = off[(size_t)yy * W + x], d = (long long)(y - yy) * (y - yy) + o * o;
        if (d < best) best = d, bi = yy * W + x + (int)o;
      }
      if (outside) {
        const long long b[2] = {(long long)(y + 1) * (y + 1), (long long)(H - y) * (H - y)};
        for (long long v : b) best = v < best ? v : best;
      }
      d2[i] = (int)best, nearest[i] = outside ? -1 : bi;
    }
}

// ---- ownership and extents ----------------------------------------------------------------------------------------------------------
static void walk_geometry(int H, int W) {
  const EdtGeom q = edt_geom(1, H, W);
  CHECK(q.seg >= 1 && q.seg <= EDT_MAX_SEG && q.seg * EDT_LANES >= W && (q.seg - 1) * EDT_LANES < W);
  CHECK(q.pitch >= q.seg && q.pitch % 4 == 2 && q.pitch <= EDT_MAX_SEG + 2 && EDT_LANES * q.pitch <= EDT_ROW_LDS);
  CHECK(q.rblocks * EDT_RROWS >= H && (q.rblocks - 1) * EDT_RROWS < H);
  // a row's pixels in LDS: distinct places inside the row's array
  std::vector<int> place(EDT_ROW_LDS, 0);
  for (int x = 0; x < W; ++x) {
    const int i = edt_lds_index(q, x);
    CHECK(i >= 0 && i < EDT_ROW_LDS);
    if (i >= 0 && i < EDT_ROW_LDS) CHECK(place[i]++ == 0);
  }
  // the row pass: the strided loops of load / store and the segments of summary / scan own every pixel once
  std::vector<int> strided((size_t)H * W, 0), segs((size_t)H * W, 0);
  for (int rb = 0; rb < q.rblocks; ++rb)
    for (int tid = 0; tid < EDT_THREADS; ++tid) {
      for (int r = 0; r < EDT_RROWS; ++r) {
        const int y = rb * EDT_RROWS + r;
        if (y >= H) break;
        for (int x = tid; x < W; x += EDT_THREADS) ++strided[(size_t)y * W + x];
      }
      int r, y, x0, x1;
      edt_row_owner(q, rb, tid, &r, &y, &x0, &x1);
      CHECK(r >= 0 && r < EDT_RROWS && x0 >= 0 && x1 <= W);
      if (y < H)
        for (int x = x0; x < x1; ++x) ++segs[(size_t)y * W + x];
    }
  // the column pass: tiles, rounds and threads own every pixel once
  std::vector<int> cols((size_t)H * W, 0);
  for (int t = 0; t < q.ctiles; ++t)
    for (int tid = 0; tid < EDT_THREADS; ++tid)
      for (int j = 0; j < EDT_CROWS; ++j) {
        int y, x;
        edt_col_owner(q, t, tid, j, &y, &x);
        CHECK(x >= 0 && y >= 0);
        if (x < W && y < H) ++cols[(size_t)y * W + x];
      }
  long long bad = 0;
  for (size_t i = 0; i < (size_t)H * W; ++i) bad += strided[i] != 1 || segs[i] != 1 || cols[i] != 1;
  CHECK(bad == 0);
  // the workspace: the row offsets, then the slots, nothing overlapping, the last slot inside
  for (int P : {1, 3}) {
    const EdtGeom qp = edt_geom(P, H, W);
    const EdtWork w = edt_work(qp);
    CHECK(w.g == 0 && w.slots >= 2ll * P * H * W && w.slots % 16 == 0 && w.slots < 2ll * P * H * W + 16);
    CHECK(w.slots + 4 * (edt_slot(qp, P - 1, qp.ctiles - 1) + 2) == w.bytes);
  }
}

// ---- the passes themselves ------------------------------------------------------------------------------------------------------------
static void run(int H, int W, int kind, bool big) {
  const EdtGeom q = edt_geom(1, H, W);
  const std::vector<uint8_t> m = pattern(kind, H, W);
  const int n = H * W;
  for (int value = 0; value < 2; ++value) {
    std::vector<uint8_t> sel(n);
    for (int i = 0; i < n; ++i) sel[i] = (m[i] != 0) == (value != 0);
    for (int outside = 0; outside < 2; ++outside) {
      std::vector<int> d0, n0;
      (big ? separable : brute)(sel, H, W, outside, d0, n0);
      for (int rev = 0; rev < 2; ++rev) {
        if (big && rev) continue;
        // the row pass, workgroup by workgroup; a barrier = every thread has finished the phase
        std::vector<short> g((size_t)n, (short)0x5a5a);
        std::vector<short> row((size_t)EDT_RROWS * EDT_ROW_LDS);
        std::vector<int> sl(EDT_THREADS), sr(EDT_THREADS);
        for (int b = 0; b < q.rblocks; ++b) {
          const int rb = rev ? q.rblocks - 1 - b : b;
          row.assign(row.size(), (short)0x7b7b);  // stale LDS
          auto each = [&](auto f) {
            for (int k = 0; k < EDT_THREADS; ++k) f(rev ? EDT_THREADS - 1 - k : k);
          };
          each([&](int tid) { edt_row_load(q, rb, m.data(), value, tid, row.data()); });
          each([&](int tid) { edt_row_summary(q, rb, tid, row.data(), sl.data(), sr.data()); });
          each([&](int tid) { edt_row_scan(q, rb, outside, tid, row.data(), sl.data(), sr.data()); });
          each([&](int tid) { edt_row_store(q, rb, tid, row.data(), g.data()); });
        }
        long long bad = 0;
        for (int i = 0; i < n; ++i) {  // the row offsets: 0 exactly on the pixels that are not selected, |g| <= 4096 or the sentinel
          bad += (g[i] == 0) != (sel[i] == 0);
          bad += g[i] != EDT_NO_ROW && (g[i] > 4096 || g[i] < -4096);
        }
        CHECK(bad == 0);
        // the column pass, tile by tile: d2, nearest, steps, the tile's slot; then the peak from the slots
        std::vector<int> slots((size_t)2 * q.ctiles, 0x5a5a5a5a);
        long long bad_d = 0, bad_n = 0, bad_steps = 0, steps = 0;
        for (int ties = 0; ties < 2; ++ties) {
          if (ties && outside) continue;
          for (int b = 0; b < q.ctiles; ++b) {
            const int t = rev ? q.ctiles - 1 - b : b;
            unsigned long long key = 0;
            for (int k = 0; k < EDT_THREADS; ++k) {
              const int tid = rev ? EDT_THREADS - 1 - k : k;
              for (int j = 0; j < EDT_CROWS; ++j) {
                int y, x;
                edt_col_owner(q, t, tid, j, &y, &x);
                if (x >= W || y >= H) continue;
                const EdtHit h = edt_search(g.data(), H, W, y, x, outside, ties);
                const int i = y * W + x, kmax = y > H - 1 - y ? y : H - 1 - y;
                bad_d += h.d2 != d0[i];
                if (ties) bad_n += (h.yn < 0 ? -1 : h.yn * W + x + g[(size_t)h.yn * W + x]) != n0[i];
                bad_steps += h.steps > kmax;
                if (!ties) steps += h.steps;
                const unsigned long long u = edt_peak_key(h.d2, i);
                key = u > key ? u : key;
              }
            }
            const long long s = edt_slot(q, 0, t);
            slots[(size_t)s] = edt_peak_d2(key), slots[(size_t)s + 1] = edt_peak_index(key);
          }
          unsigned long long key = 0;
          for (int t = 0; t < q.ctiles; ++t) {
            const long long s = edt_slot(q, 0, t);
            const unsigned long long u = slots[(size_t)s + 1] < 0 ? 0ull : edt_peak_key(slots[(size_t)s], slots[(size_t)s + 1]);
            key = u > key ? u : key;
          }
          int pd = 0, pi = -1;
          for (int i = 0; i < n; ++i)
            if (d0[i] > pd) pd = d0[i], pi = i;
          CHECK(edt_peak_d2(key) == pd && edt_peak_index(key) == pi);
        }
        CHECK(bad_d == 0);
        CHECK(bad_n == 0);
        CHECK(bad_steps == 0);
        if (kind == 4 && (W > 1 || outside)) CHECK(steps == 0);  // a checkerboard: every search for d2 alone ends before its first row
      }
    }
  }
}

int main() {
  int cases = 0;
  auto shape = [&](int H, int W, bool big) {
    const long long before = fails;
    walk_geometry(H, W);
    for (int kind = 0; kind < KINDS; ++kind)
      if (!big || kind == 2 || kind == 5 || kind == 6) run(H, W, kind, big);  // the large planes: the deepest search and the random ones
    const EdtGeom q = edt_geom(1, H, W);
    std::printf("H %d W %d: seg %d pitch %d rblocks %d ctiles %d fails %lld\n", H, W, q.seg, q.pitch, q.rblocks, q.ctiles, fails - before);
    ++cases;
  };
  // the strip lengths of the kernels: 4 rows a row-pass workgroup, 16 rows and 64 columns a column-pass tile, 64 segments a row
  const int sides[] = {1, 2, 3, 4, 5, 9, 15, 16, 17, 33, 63, 64, 65};
  const int ns = sizeof(sides) / sizeof(sides[0]);
  for (int a = 0; a < ns; ++a)
    for (int d : {0, 1, 5, 9}) shape(sides[a], sides[(a + d) % ns], false);  // every side as H and as W, with several partners
  shape(129, 257, true);
  shape(300, 517, true);
  shape(1, 4096, true);
  shape(4096, 1, true);
  shape(3, 1025, true);  // seg 17, pitch 18
  // the largest plane: geometry and sections only
  {
    const EdtGeom q = edt_geom(65535, 4096, 4096);
    CHECK(q.seg == 64 && q.pitch == 66 && q.rblocks == 1024 && q.ctiles == 64 * 256);
    const EdtWork w = edt_work(q);
    CHECK(w.slots == 2ll * 65535 * 4096 * 4096 && w.bytes == w.slots + 8ll * 65535 * 16384);
    CHECK(edt_slot(q, 65534, q.ctiles - 1) == 2ll * 65535 * 16384 - 2);
    CHECK(2ll * 4099 * 4099 < (1ll << 31) && edt_peak_index(edt_peak_key(EDT_NONE, 0)) == 0 && edt_peak_d2(edt_peak_key(EDT_NONE, 0)) == EDT_NONE);
    CHECK(edt_peak_index(0) == -1 && edt_peak_d2(0) == 0);
  }
  std::printf("cases %d fails %lld\n", cases, fails);
  return fails ? 1 : 0;
}
