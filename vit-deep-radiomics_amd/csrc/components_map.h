// The ONE mapping and the ONE union-find of the connected-component kernels (components.hip; the definitions are
// vdr_op_connected_components' and vdr_op_mask_clean's in include/vdr.h): the tile geometry, what each thread of the tile pass
// does in each of its phases, the enumeration of the pixel pairs that straddle a seam between tiles, find and union, the chunks
// of the linear passes and the workspace sections.  The kernels, the launch plan and the host program
// tests/components_map_cases.cpp all call it: the host program runs the very same phase functions tile by tile with a policy
// whose "atomics" are plain min / add and whose loads count steps.  It includes nothing and compiles as plain C++.
//
//   plane   p of P: H x W, pixel index i = y * W + x (int32: H W <= 2^24)
//   tile    CC_T x CC_T pixels, tile t = tyi * tx + txi of a plane; blockIdx.x = p * tiles + t in the tile pass
//   label   L[i] >= 0: the index of another (or the same) selected pixel of i's component, ALWAYS L[i] <= i; -1: not selected.
//           The invariant L[i] <= i makes every chain strictly decreasing until it meets a root (L[r] == r).
//   seam    item s of nv + nh per plane: a pixel in the left column of a tile that has a left neighbour tile (s < nv) or in the
//           top row of a tile that has an upper neighbour tile; its partners lie at x - 1 (rows y - 1 .. y + 1) or at y - 1
//           (columns x - 1 .. x + 1); at connectivity 4 only the middle one
//   chunk   CC_CHUNK consecutive pixel indices of a plane: the work item of the flatten, best and apply passes
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CC_HD __host__ __device__ inline
#else
#define CC_HD inline
#endif

namespace vdr {

constexpr int CC_T = 64;                       // tile side
constexpr int CC_PITCH = CC_T + 1;             // LDS row pitch of a tile: the 64 rows of a wave's column strip fall into 64 banks
constexpr int CC_LDS = CC_T * CC_PITCH;        // int32 of one LDS plane of a tile
constexpr int CC_THREADS = 256;
constexpr int CC_SEG = 16;                     // pixels of a row a thread walks: CC_T / (CC_THREADS / CC_T)
constexpr int CC_PER_THREAD = CC_T * CC_T / CC_THREADS;  // 16
constexpr int CC_MAX_SIDE = 4096;
constexpr int CC_CHUNK = 4096;                 // pixels of a chunk of the linear passes
constexpr int CC_SLOT = 8;                     // int32 of a partial slot (6 used): changed, area, min x, min y, max x, max y
constexpr int CC_MAX_PLANES = 65535;

struct CcGeom {
  int P, H, W;
  int tx, ty, tiles;  // tiles across, down, per plane
  int nv, nh;         // seam items of the vertical and of the horizontal seams, per plane (each < 64 * 4096)
  int chunks;         // per plane
};

CC_HD CcGeom cc_geom(int P, int H, int W) {
  CcGeom q;
  q.P = P, q.H = H, q.W = W;
  q.tx = (W + CC_T - 1) / CC_T, q.ty = (H + CC_T - 1) / CC_T;
  q.tiles = q.tx * q.ty;
  q.nv = (q.tx - 1) * H, q.nh = (q.ty - 1) * W;
  q.chunks = (H * W + CC_CHUNK - 1) / CC_CHUNK;
  return q;
}

struct CcTile {
  int x0, y0, w, h;
};

CC_HD CcTile cc_tile(const CcGeom& q, int t) {
  CcTile c;
  const int tyi = t / q.tx, txi = t - tyi * q.tx;
  c.x0 = txi * CC_T, c.y0 = tyi * CC_T;
  c.w = q.W - c.x0 < CC_T ? q.W - c.x0 : CC_T;
  c.h = q.H - c.y0 < CC_T ? q.H - c.y0 : CC_T;
  return c;
}

// ---- find and union ---------------------------------------------------------------------------------------------------------------
// Pol::load(L, i), Pol::store(L, i, v), Pol::fetch_min(L, i, v) -> the old value, Pol::add(A, i, v).  On the device fetch_min is
// an integer atomicMin and add an integer atomicAdd; on the host they are plain.  All of it relies on ONE invariant that every
// writer keeps: a stored label is <= its own index and names a pixel of the same component.

template <class Pol>
CC_HD int cc_find(int* L, int i) {
  // terminates: L[i] <= i always, so the loop moves to a strictly smaller index each time round and indices are >= 0: at most i
  // rounds.  (A concurrent fetch_min only lowers labels; a stale read gives an older, larger label of the same chain.)
  for (;;) {
    const int p = Pol::load(L, i);
    if (p == i) return i;
    i = p;
  }
}

template <class Pol>
CC_HD void cc_union(int* L, int a, int b) {
  // terminates: every round either returns or replaces a by `old`, a label read from L[a] that differs from a and is therefore
  // strictly below it (the invariant), and b never grows (find only descends): a + b strictly decreases and is >= 0.
  // A retry happens only after the label of a was seen strictly decreased by another union.
  for (;;) {
    a = cc_find<Pol>(L, a);
    b = cc_find<Pol>(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    // a > b: hang the (supposed) root a below b.  old == a: a was a root at that instant and now points to b.  Otherwise another
    // union moved a first: L[a] is now min(old, b), both in the component, and the pair (old, b) is still to be joined.
    const int old = Pol::fetch_min(L, a, b);
    if (old == a) return;
    a = old;
  }
}

// ---- the tile pass: the phases of thread tid of CC_THREADS, a barrier between two phases ---------------------------------------------
// lab and cnt are the tile's two LDS planes (CC_LDS int32 each), addressed ly * CC_PITCH + lx; labels are such addresses: the
// order of the addresses inside a tile is the order of the pixel indices, so the lowest address of a component of the tile is
// its lowest pixel index.

// phase A: load, lane-contiguous along x.  selected = inside the plane and (mask != 0) == (value != 0)
CC_HD void cc_tile_load(const CcTile& c, int W, const unsigned char* plane, int value, int tid, int* lab, int* cnt) {
  for (int k = 0; k < CC_PER_THREAD; ++k) {  // fixed trip count
    const int idx = k * CC_THREADS + tid, ly = idx / CC_T, lx = idx - ly * CC_T;
    const int li = ly * CC_PITCH + lx;
    bool sel = false;
    if (lx < c.w && ly < c.h) sel = (plane[(long long)(c.y0 + ly) * W + c.x0 + lx] != 0) == (value != 0);
    lab[li] = sel ? li : -1;
    cnt[li] = 0;
  }
}

CC_HD int cc_seg_base(int tid) { return (tid % CC_T) * CC_PITCH + (tid / CC_T) * CC_SEG; }  // row tid % 64, columns 16 (tid / 64) ..

// phase B: a thread labels the runs of its own 16 pixels of one row with the run's first address (no other thread touches them)
CC_HD void cc_tile_runs(int tid, int* lab) {
  const int base = cc_seg_base(tid);
  int start = -1;
  for (int j = 0; j < CC_SEG; ++j) {  // fixed trip count
    if (lab[base + j] >= 0) {
      start = start < 0 ? base + j : start;
      lab[base + j] = start;
    } else {
      start = -1;
    }
  }
}

// phase C: the unions of a thread's pixels with the pixel to the left of its strip and with the row above.  Which pixels are
// selected (lab >= 0) never changes after phase A, so reading it beside concurrent unions is safe.  A pixel whose upper
// neighbour is selected joins it unless its left neighbour and that one's upper neighbour are selected too (then the two rows'
// runs are already joined further left); without an upper neighbour, at connectivity 8, it joins the two diagonal ones.
template <class Pol>
CC_HD void cc_tile_unions(int tid, int conn8, int* lab) {
  const int base = cc_seg_base(tid);
  const int row = tid % CC_T, lx0 = (tid / CC_T) * CC_SEG;
  for (int j = 0; j < CC_SEG; ++j) {  // fixed trip count; every union inside terminates (cc_union)
    const int li = base + j, lx = lx0 + j;
    if (Pol::load(lab, li) < 0) continue;
    const bool left = lx > 0 && Pol::load(lab, li - 1) >= 0;
    if (j == 0 && left) cc_union<Pol>(lab, li, li - 1);
    if (row == 0) continue;
    const int up = li - CC_PITCH;
    if (Pol::load(lab, up) >= 0) {
      if (!(left && Pol::load(lab, up - 1) >= 0)) cc_union<Pol>(lab, li, up);
    } else if (conn8) {
      if (lx > 0 && Pol::load(lab, up - 1) >= 0) cc_union<Pol>(lab, li, up - 1);
      if (lx < CC_T - 1 && Pol::load(lab, up + 1) >= 0) cc_union<Pol>(lab, li, up + 1);
    }
  }
}

// phase D: every pixel gets its tile root; the areas are counted per run of equal roots, one add per run
template <class Pol>
CC_HD void cc_tile_flatten(int tid, int* lab, int* cnt) {
  const int base = cc_seg_base(tid);
  int prev = -1, acc = 0;
  for (int j = 0; j < CC_SEG; ++j) {  // fixed trip count
    const int li = base + j;
    if (Pol::load(lab, li) < 0) continue;
    const int r = cc_find<Pol>(lab, li);
    Pol::store(lab, li, r);  // a root of li's own tree: still a valid label, still <= li
    if (r != prev) {
      if (acc) Pol::add(cnt, prev, acc);
      prev = r, acc = 0;
    }
    ++acc;
  }
  if (acc) Pol::add(cnt, prev, acc);
}

// phase E: store, lane-contiguous along x: the label as the plane index of the tile root, the tile's area at the tile root
CC_HD void cc_tile_store(const CcTile& c, int W, int tid, const int* lab, const int* cnt, int* L, int* area) {
  for (int k = 0; k < CC_PER_THREAD; ++k) {  // fixed trip count
    const int idx = k * CC_THREADS + tid, ly = idx / CC_T, lx = idx - ly * CC_T;
    if (lx >= c.w || ly >= c.h) continue;
    const int li = ly * CC_PITCH + lx, r = lab[li];
    const int g = (c.y0 + ly) * W + c.x0 + lx;
    const int ry = r / CC_PITCH, rx = r - ry * CC_PITCH;
    L[g] = r < 0 ? -1 : (c.y0 + ry) * W + c.x0 + rx;
    area[g] = r == li ? cnt[li] : 0;
  }
}

// ---- the seam pass ------------------------------------------------------------------------------------------------------------------
struct CcSeam {
  int x, y;      // the pixel of the item
  int vertical;  // its partners: vertical seam: (x - 1, y + d); horizontal seam: (x + d, y - 1), d = -1, 0, 1
};

CC_HD CcSeam cc_seam_item(const CcGeom& q, int s) {
  CcSeam m;
  if (s < q.nv) {
    const int k = s / q.H;
    m.x = (k + 1) * CC_T, m.y = s - k * q.H, m.vertical = 1;
  } else {
    const int u = s - q.nv, k = u / q.W;
    m.x = u - k * q.W, m.y = (k + 1) * CC_T, m.vertical = 0;
  }
  return m;
}

// partner d (-1, 0, 1) of a seam item: its pixel index, or -1 when it lies outside the plane
CC_HD int cc_seam_partner(const CcGeom& q, const CcSeam& m, int d) {
  const int px = m.vertical ? m.x - 1 : m.x + d, py = m.vertical ? m.y + d : m.y - 1;
  if (px < 0 || px >= q.W || py < 0 || py >= q.H) return -1;
  return py * q.W + px;
}

template <class Pol>
CC_HD void cc_seam_unions(const CcGeom& q, int s, int conn8, int* L) {
  const CcSeam m = cc_seam_item(q, s);
  const int i = m.y * q.W + m.x;
  if (Pol::load(L, i) < 0) return;
  for (int d = -1; d <= 1; ++d) {  // fixed trip count; every union inside terminates (cc_union)
    if (d && !conn8) continue;
    const int j = cc_seam_partner(q, m, d);
    if (j >= 0 && Pol::load(L, j) >= 0) cc_union<Pol>(L, i, j);
  }
}

// ---- the flatten pass, one pixel ----------------------------------------------------------------------------------------------------
// root[i] = find(i); the area a tile root carries moves to the plane root with one add.  Only tile roots carry an area, only
// plane roots receive one, and a plane root is never emptied: no slot is written by two parties.  Returns 1 for a plane root.
template <class Pol>
CC_HD int cc_flatten_pixel(int i, int* L, int* area, int* root) {
  if (Pol::load(L, i) < 0) {
    if (root != L) root[i] = -1;
    return 0;
  }
  const int r = cc_find<Pol>(L, i);
  if (root == L) Pol::store(L, i, r);  // in place: a root of i's own tree is a valid label <= i for every concurrent find
  else root[i] = r;
  if (r == i) return 1;
  const int a = area[i];
  if (a > 0) {
    Pol::add(area, r, a);
    area[i] = 0;
  }
  return 0;
}

// the key of "largest, lowest root on a tie" as one unsigned minimum: (2^31 - 1 - area) in the high word, the root in the low
CC_HD unsigned long long cc_best_key(int area, int root) {
  return ((unsigned long long)(unsigned)(0x7fffffff - area) << 32) | (unsigned)root;
}
constexpr unsigned long long CC_NO_BEST = ~0ull;
CC_HD int cc_best_root(unsigned long long key) { return key == CC_NO_BEST ? -1 : (int)(unsigned)(key & 0xffffffffull); }

// ---- the clean steps ----------------------------------------------------------------------------------------------------------------
constexpr int CC_STEP_COPY = 0, CC_STEP_HOLES = 1, CC_STEP_ISLANDS = 2, CC_STEP_LARGEST = 3;

// the new value of a pixel whose old value is `set`; lab / area / best are read only where the step needs them
CC_HD int cc_apply_pixel(int step, int set, int i, const int* L, const int* area, int best, int min_area) {
  if (step == CC_STEP_HOLES) return set ? 1 : (area[L[i]] < min_area ? 1 : 0);
  if (step == CC_STEP_ISLANDS) return set ? (area[L[i]] >= min_area || L[i] == best ? 1 : 0) : 0;
  if (step == CC_STEP_LARGEST) return set ? (L[i] == best ? 1 : 0) : 0;
  return set;
}

// ---- the workspace ------------------------------------------------------------------------------------------------------------------
// connected_components: [ L : 4 P H W ]                                        (root is written from it, area is the output)
// mask_clean:           [ L : 4 P H W ][ area : 4 P H W ][ best : 8 P ][ count : 4 P, padded to 8 ][ slots A ][ slots B ]
//                       slots: P * chunks * CC_SLOT int32 each (32 bytes per 4096 pixels): A the hole step's, B the last step's
struct CcWork {
  long long L, area, best, count, slots_a, slots_b, bytes;  // byte offsets
};

CC_HD CcWork cc_work(const CcGeom& q, int clean) {
  CcWork w;
  const long long px = (long long)q.P * q.H * q.W;
  w.L = 0;
  w.area = w.best = w.count = w.slots_a = w.slots_b = -1;
  w.bytes = 4 * px;
  if (clean) {
    w.area = 4 * px;
    w.best = 8 * px;
    w.count = w.best + 8ll * q.P;
    w.slots_a = w.count + 8ll * ((q.P + 1) / 2);
    w.slots_b = w.slots_a + 4ll * CC_SLOT * q.P * q.chunks;
    w.bytes = w.slots_b + 4ll * CC_SLOT * q.P * q.chunks;
  }
  return w;
}

}  // namespace vdr
