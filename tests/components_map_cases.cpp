// Host program (its own main) over csrc/components_map.h, the mapping and the union-find the connected-component kernels
// (csrc/components.hip) are written on.  For every shape and both connectivities it checks that every pixel lies in exactly one
// tile, that every adjacent pair of pixels in different tiles is enumerated by the seam pass, that every index the passes form
// stays inside its plane, its LDS plane and its workspace section, and it RUNS the passes -- the very functions the kernels
// call, with a policy whose atomics are plain -- tile by tile, thread by thread, in forward and in reversed order, against a
// plain breadth-first search: roots, areas, counts and the three clean steps.  Every policy access counts a step; a cap on the
// steps turns a loop that does not end into a failed run.  Built and run by tests/test_components_cpu.py, once plainly and once
// with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>

#include "components_map.h"

using namespace vdr;

static long long fails = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (fails++ < 10) std::printf("FAIL %s (line %d)\n", #cond, __LINE__);   \
    }                                                                          \
  } while (0)

// the host policy: plain min / add, every access inside [0, n) of the array it was told about, every access one step
struct Host {
  static long long steps, cap;
  static const int* lo;
  static long long n;
  static void tick(const int* L, long long i) {
    if (!(L == lo && i >= 0 && i < n)) {
      std::printf("FAIL access %lld outside [0, %lld)\n", i, n);
      std::exit(3);
    }
    if (++steps > cap) {
      std::printf("FAIL step cap %lld exceeded: a loop does not end\n", cap);
      std::exit(2);
    }
  }
  static int load(const int* L, int i) { return tick(L, i), L[i]; }
  static void store(int* L, int i, int v) { tick(L, i), L[i] = v; }
  static int fetch_min(int* L, int i, int v) {
    tick(L, i);
    const int old = L[i];
    L[i] = v < old ? v : old;
    return old;
  }
  static void add(int* A, int i, int v) { A[i] += v; }
  static void arm(const int* base, long long count, long long budget) { lo = base, n = count, steps = 0, cap = budget; }
};
long long Host::steps = 0, Host::cap = 0, Host::n = 0;
const int* Host::lo = nullptr;

// breadth-first search: root = the lowest index of the component, area at the root
static void bfs(const std::vector<uint8_t>& m, int H, int W, int conn8, int value, std::vector<int>& root, std::vector<int>& area, int& count) {
  const int n = H * W;
  root.assign(n, -1), area.assign(n, 0), count = 0;
  std::vector<int> queue;
  for (int s = 0; s < n; ++s) {
    if ((m[s] != 0) != (value != 0) || root[s] >= 0) continue;
    queue.assign(1, s), root[s] = s, ++count;
    for (size_t h = 0; h < queue.size(); ++h) {
      const int i = queue[h], y = i / W, x = i % W;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if ((!dx && !dy) || (!conn8 && dx && dy)) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
          const int j = yy * W + xx;
          if ((m[j] != 0) == (value != 0) && root[j] < 0) root[j] = s, queue.push_back(j);
        }
    }
    area[s] = (int)queue.size();
  }
}

// the three passes as the kernels run them; rev: tiles, threads, seam items and pixels in reversed order
static void label(const std::vector<uint8_t>& m, const CcGeom& q, int conn8, int value, bool rev, std::vector<int>& L, std::vector<int>& area,
                  std::vector<int>& root, int& count, bool in_place) {
  const int n = q.H * q.W;
  L.assign(n, -7), area.assign(n, -7), root.assign(n, -7);
  std::vector<int> lab(CC_LDS, -9), cnt(CC_LDS, -9);
  for (int tt = 0; tt < q.tiles; ++tt) {
    const int t = rev ? q.tiles - 1 - tt : tt;
    const CcTile c = cc_tile(q, t);
    lab.assign(CC_LDS, -9), cnt.assign(CC_LDS, -9);  // LDS is not initialised: whatever is read must have been written
    auto each = [&](auto f) {
      for (int k = 0; k < CC_THREADS; ++k) f(rev ? CC_THREADS - 1 - k : k);
    };
    each([&](int tid) { cc_tile_load(c, q.W, m.data(), value, tid, lab.data(), cnt.data()); });
    each([&](int tid) { cc_tile_runs(tid, lab.data()); });
    Host::arm(lab.data(), CC_LDS, 64ll * CC_LDS * 8);
    each([&](int tid) { cc_tile_unions<Host>(tid, conn8, lab.data()); });
    each([&](int tid) { cc_tile_flatten<Host>(tid, lab.data(), cnt.data()); });
    for (int i = 0; i < CC_LDS; ++i) CHECK(lab[i] == -9 || (lab[i] >= -1 && lab[i] <= i));
    each([&](int tid) { cc_tile_store(c, q.W, tid, lab.data(), cnt.data(), L.data(), area.data()); });
  }
  for (int i = 0; i < n; ++i) CHECK(L[i] >= -1 && L[i] <= i && area[i] >= 0);  // every pixel written, the invariant holds
  Host::arm(L.data(), n, 2000ll * n + 1000000);
  for (int ss = 0; ss < q.nv + q.nh; ++ss) cc_seam_unions<Host>(q, rev ? q.nv + q.nh - 1 - ss : ss, conn8, L.data());
  for (int i = 0; i < n; ++i) CHECK(L[i] >= -1 && L[i] <= i);
  count = 0;
  int* out = in_place ? L.data() : root.data();
  for (int ii = 0; ii < q.chunks * CC_CHUNK; ++ii) {
    const int i = rev ? q.chunks * CC_CHUNK - 1 - ii : ii;
    if (i < n) count += cc_flatten_pixel<Host>(i, L.data(), area.data(), out);
  }
  if (in_place) root = L;
}

static int best_of(const std::vector<int>& area) {
  unsigned long long key = CC_NO_BEST;
  for (size_t i = 0; i < area.size(); ++i)
    if (area[i] > 0) {
      const unsigned long long u = cc_best_key(area[i], (int)i);
      key = u < key ? u : key;
    }
  return cc_best_root(key);
}

static void walk_geometry(int H, int W) {
  const CcGeom q = cc_geom(3, H, W);
  const int n = H * W;
  std::vector<int> owner(n, 0);
  std::vector<int> tile_of(n, -1);
  for (int t = 0; t < q.tiles; ++t) {
    const CcTile c = cc_tile(q, t);
    CHECK(c.w >= 1 && c.w <= CC_T && c.h >= 1 && c.h <= CC_T && c.x0 >= 0 && c.y0 >= 0 && c.x0 + c.w <= W && c.y0 + c.h <= H);
    for (int tid = 0; tid < CC_THREADS; ++tid) {
      CHECK(cc_seg_base(tid) >= 0 && cc_seg_base(tid) + CC_SEG <= CC_LDS);
      for (int k = 0; k < CC_PER_THREAD; ++k) {
        const int idx = k * CC_THREADS + tid, ly = idx / CC_T, lx = idx - ly * CC_T;
        CHECK(ly * CC_PITCH + lx < CC_LDS);
        if (lx < c.w && ly < c.h) ++owner[(c.y0 + ly) * W + c.x0 + lx], tile_of[(c.y0 + ly) * W + c.x0 + lx] = t;
      }
    }
  }
  long long bad = 0;
  for (int i = 0; i < n; ++i) bad += owner[i] != 1;
  CHECK(bad == 0);
  // every adjacent pair in different tiles is enumerated (connectivity 8: all of them; 4: the edge neighbours)
  for (int conn8 = 0; conn8 < 2; ++conn8) {
    std::vector<std::pair<int, int>> seen;
    for (int s = 0; s < q.nv + q.nh; ++s) {
      const CcSeam m = cc_seam_item(q, s);
      CHECK(m.x >= 0 && m.x < W && m.y >= 0 && m.y < H);
      for (int d = -1; d <= 1; ++d) {
        if (d && !conn8) continue;
        const int j = cc_seam_partner(q, m, d);
        CHECK(j >= -1 && j < n);
        if (j >= 0) seen.push_back({m.y * W + m.x, j}), seen.push_back({j, m.y * W + m.x});
      }
    }
    std::vector<uint8_t> hit((size_t)n * 8, 0);  // pair (i, direction)
    static const int DX[8] = {1, -1, 0, 0, 1, 1, -1, -1}, DY[8] = {0, 0, 1, -1, 1, -1, 1, -1};
    for (auto& pr : seen) {
      const int i = pr.first, j = pr.second, dx = j % W - i % W, dy = j / W - i / W;
      for (int k = 0; k < 8; ++k)
        if (DX[k] == dx && DY[k] == dy) hit[(size_t)i * 8 + k] = 1;
    }
    long long missed = 0;
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < (conn8 ? 8 : 4); ++k) {
        const int x = i % W + DX[k], y = i / W + DY[k];
        if (x < 0 || x >= W || y < 0 || y >= H) continue;
        if (tile_of[y * W + x] != tile_of[i]) missed += !hit[(size_t)i * 8 + k];
      }
    CHECK(missed == 0);
  }
  // the chunks cover the plane once; the workspace sections are disjoint, ordered and aligned
  CHECK((long long)q.chunks * CC_CHUNK >= n && (long long)(q.chunks - 1) * CC_CHUNK < n);
  const CcWork w = cc_work(q, 1), w0 = cc_work(q, 0);
  const long long px = 3ll * n;
  CHECK(w0.bytes == 4 * px && w.L == 0 && w.area == 4 * px && w.best == 8 * px && w.best % 8 == 0 && w.count >= w.best + 8 * 3);
  CHECK(w.slots_a >= w.count + 4 * 3 && w.slots_a % 8 == 0 && w.slots_b == w.slots_a + 4ll * CC_SLOT * 3 * q.chunks);
  CHECK(w.bytes == w.slots_b + 4ll * CC_SLOT * 3 * q.chunks && w.bytes <= 8 * px + 16 * 3 + 8 + 64ll * 3 * q.chunks);
}

static unsigned rng_state = 12345u;
static unsigned rnd() { return rng_state = rng_state * 1664525u + 1013904223u, rng_state >> 8; }

static std::vector<uint8_t> pattern(int kind, int H, int W) {
  std::vector<uint8_t> m((size_t)H * W, 0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      uint8_t v = 0;
      switch (kind) {
        case 0: v = (rnd() % 100) < 41; break;
        case 1: v = (rnd() % 100) < 59 ? 255 : 0; break;
        case 2: v = 1; break;
        case 3: v = (x + y) & 1; break;                                                   // checkerboard
        case 4: v = (y % 2 == 0) || (x == ((y / 2) % 2 ? 0 : W - 1)); break;             // serpentine
        case 5: v = (x == y) || (x + y == 63 + 64) || (x + y == 63); break;              // diagonals through the four-tile corner
        case 6: v = (y == 0) || (x % 2 == 0); break;                                      // comb
        case 7: {                                                                         // concentric rings
          const int r = x < y ? x : y, r2 = W - 1 - x < H - 1 - y ? W - 1 - x : H - 1 - y, d = r < r2 ? r : r2;
          v = d % 2 == 0;
        } break;
      }
      m[(size_t)y * W + x] = v;
    }
  return m;
}

static void run(int H, int W, int kind) {
  const CcGeom q = cc_geom(1, H, W);
  const std::vector<uint8_t> m = pattern(kind, H, W);
  const int n = H * W;
  for (int conn8 = 0; conn8 < 2; ++conn8)
    for (int value = 0; value < 2; ++value) {
      std::vector<int> r0, a0, L, a, r;
      int c0 = 0, c = 0;
      bfs(m, H, W, conn8, value, r0, a0, c0);
      for (int rev = 0; rev < 2; ++rev)
        for (int in_place = 0; in_place < 2; ++in_place) {
          label(m, q, conn8, value, rev, L, a, r, c, in_place);
          long long bad = 0;
          for (int i = 0; i < n; ++i) bad += r[i] != r0[i] || a[i] != a0[i];
          CHECK(bad == 0);
          CHECK(c == c0);
        }
      // the clean steps against their statement on the breadth-first search
      const int best = best_of(a), min_area = 5;
      int best0 = -1;
      for (int i = 0; i < n; ++i)
        if (a0[i] > 0 && (best0 < 0 || a0[i] > a0[best0])) best0 = i;
      CHECK(best == best0);
      for (int i = 0; i < n; ++i) {
        const int set = (m[i] != 0) == (value != 0);  // the pixels labelled are the ones a step treats as its subject
        if (value == 0) {
          const int o = cc_apply_pixel(CC_STEP_HOLES, m[i] != 0, i, r.data(), a.data(), best, min_area);
          CHECK(o == ((m[i] != 0) || a0[r0[i]] < min_area));
        } else {
          CHECK(cc_apply_pixel(CC_STEP_ISLANDS, set, i, r.data(), a.data(), best, min_area) == (set && (a0[r0[i]] >= min_area || r0[i] == best0)));
          CHECK(cc_apply_pixel(CC_STEP_LARGEST, set, i, r.data(), a.data(), best, min_area) == (set && r0[i] == best0));
          CHECK(cc_apply_pixel(CC_STEP_COPY, set, i, nullptr, nullptr, -1, min_area) == set);
        }
      }
    }
}

int main() {
  const int sides[] = {1, 2, CC_T - 1, CC_T, CC_T + 1, 2 * CC_T + 1};
  int cases = 0;
  auto shape = [&](int H, int W) {
    const long long before = fails;
    walk_geometry(H, W);
    for (int kind = 0; kind < 8; ++kind) run(H, W, kind);
    std::printf("H %d W %d: tiles %d seam items %d chunks %d fails %lld\n", H, W, cc_geom(1, H, W).tiles, cc_geom(1, H, W).nv + cc_geom(1, H, W).nh,
                cc_geom(1, H, W).chunks, fails - before);
    ++cases;
  };
  for (int H : sides)
    for (int W : sides) shape(H, W);
  shape(129, 257);
  shape(300, 517);
  // the largest plane: geometry and sections only
  {
    const CcGeom q = cc_geom(65535, 4096, 4096);
    CHECK(q.tiles == 4096 && q.nv == 63 * 4096 && q.nh == 63 * 4096 && q.chunks == 4096);
    CHECK((long long)q.P * q.tiles < (1ll << 31));
    const CcSeam m = cc_seam_item(q, q.nv + q.nh - 1);
    CHECK(m.x == 4095 && m.y == 63 * 64 && cc_seam_partner(q, m, 1) == -1 && cc_seam_partner(q, m, 0) == (63 * 64 - 1) * 4096 + 4095);
    CHECK(cc_work(q, 1).bytes > 8ll * 65535 * 4096 * 4096);
  }
  std::printf("cases %d fails %lld\n", cases, fails);
  return fails ? 1 : 0;
}
