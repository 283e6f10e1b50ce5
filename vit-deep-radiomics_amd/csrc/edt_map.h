// The ONE mapping and the ONE search of the Euclidean distance transform kernels (edt.hip; the definition is
// vdr_op_distance_transform's in include/vdr.h): which thread owns which pixel in the row pass and in the column pass, where a
// pixel of a row sits in LDS, what each thread of the row pass does in each of its phases, the outward search of the column
// pass, the key of the peak, the partial slots and the workspace sections.  The kernels, the launch plan and the host program
// tests/edt_map_cases.cpp all call it: the host program runs the very same phase functions thread by thread, in both orders,
// and counts the steps of every search.  It includes nothing and compiles as plain C++.
//
//   plane    p of P: H x W, pixel index i = y * W + x (int32: H W <= 2^24)
//   row g    int16 per pixel, the ROW OFFSET: 0 for a pixel that is not selected; for a selected pixel the signed distance
//            x' - x to the nearest non-selected pixel x' of its own row (the lower x' on a tie, so a negative offset), or
//            EDT_NO_ROW when the row has none.  With `outside` the columns -1 and W count as non-selected: |g| <= 4096.
//   row pass a workgroup owns EDT_RROWS rows of one plane, one wave a row; a lane owns `seg` = ceil(W / 64) consecutive pixels
//   column pass  a workgroup owns a tile of EDT_CX columns x EDT_CY rows; a wave owns rows wave, wave + 4, .. of it, a lane a column
//   slot     two int32 per column-pass tile: the tile's largest d2 and the lowest pixel index that attains it (0, -1: none)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EDT_HD __host__ __device__ inline
#else
#define EDT_HD inline
#endif

namespace vdr {

constexpr int EDT_THREADS = 256;
constexpr int EDT_LANES = 64;                          // a wave; a row of the row pass is cut into 64 segments
constexpr int EDT_RROWS = EDT_THREADS / EDT_LANES;     // rows of a row-pass workgroup: 4
constexpr int EDT_MAX_SIDE = 4096;
constexpr int EDT_MAX_PLANES = 65535;
constexpr int EDT_MAX_SEG = EDT_MAX_SIDE / EDT_LANES;  // 64
constexpr int EDT_ROW_LDS = EDT_LANES * (EDT_MAX_SEG + 2);  // int16 of one row in LDS at the largest pitch (66): 4224
constexpr int EDT_CX = 64, EDT_CY = 16;                // the tile of the column pass
constexpr int EDT_CROWS = EDT_CY / EDT_RROWS;          // rows of a tile a wave walks: 4
constexpr int EDT_U = 4;                               // rows above and below a search looks at per round
constexpr int EDT_NONE = 0x7fffffff;                   // VDR_EDT_NONE: no candidate at all
constexpr int EDT_NO_ROW = -32768;                     // the row offset of "no non-selected pixel in this row"; never squared
constexpr int EDT_FAR = 1 << 20;                       // a column further away than any real one (|x - x'| <= 4096 << 2^20)
constexpr int EDT_ROW_FAR = 32767;                     // the clamped left distance of "none to the left"

struct EdtGeom {
  int P, H, W;
  int seg, pitch;   // pixels a lane owns in the row pass; the LDS pitch of a segment in int16
  int rblocks;      // row-pass workgroups per plane
  int ctx, ctiles;  // column-pass tiles across, per plane
};

EDT_HD EdtGeom edt_geom(int P, int H, int W) {
  EdtGeom q;
  q.P = P, q.H = H, q.W = W;
  q.seg = (W + EDT_LANES - 1) / EDT_LANES;
  // the pitch in 4-byte words, pitch / 2, is odd: lanes l and l + 1 at the same place in their segments are an odd number of
  // banks apart, so the 32 lanes of an LDS lane group fall into 32 different banks
  q.pitch = q.seg + ((6 - (q.seg & 3)) & 3);  // the next number that is 2 mod 4
  q.rblocks = (H + EDT_RROWS - 1) / EDT_RROWS;
  q.ctx = (W + EDT_CX - 1) / EDT_CX;
  q.ctiles = q.ctx * ((H + EDT_CY - 1) / EDT_CY);
  return q;
}

// where pixel x of a row sits in the row's LDS array: segment x / seg, place x % seg.  < 64 * pitch <= EDT_ROW_LDS
EDT_HD int edt_lds_index(const EdtGeom& q, int x) {
  const int l = x / q.seg;
  return l * q.pitch + (x - l * q.seg);
}

// ---- the row pass: the phases of thread tid of EDT_THREADS, a barrier between two phases -------------------------------------------
// row: EDT_RROWS arrays of EDT_ROW_LDS int16; sl / sr: EDT_THREADS int32 each (a segment's last and first non-selected column)

// phase A: load, lane-contiguous along x: 1 for a selected pixel, 0 otherwise.  selected = (mask != 0) == (value != 0)
EDT_HD void edt_row_load(const EdtGeom& q, int rb, const unsigned char* plane, int value, int tid, short* row) {
  for (int r = 0; r < EDT_RROWS; ++r) {  // fixed trip count
    const int y = rb * EDT_RROWS + r;
    if (y >= q.H) break;
    // terminates: x grows by EDT_THREADS each round and the loop ends at x >= W
    for (int x = tid; x < q.W; x += EDT_THREADS)
      row[r * EDT_ROW_LDS + edt_lds_index(q, x)] = (plane[(long long)y * q.W + x] != 0) == (value != 0) ? 1 : 0;
  }
}

// the row and the columns [x0, x1) thread tid owns in phases B and C (x0 >= x1: nothing; the row may lie below the plane)
EDT_HD void edt_row_owner(const EdtGeom& q, int rb, int tid, int* r, int* y, int* x0, int* x1) {
  *r = tid / EDT_LANES;
  *y = rb * EDT_RROWS + *r;
  const int l = tid - *r * EDT_LANES;
  *x0 = l * q.seg;
  *x1 = *x0 + q.seg < q.W ? *x0 + q.seg : q.W;
}

// phase B: the last and the first non-selected column of the thread's segment (-EDT_FAR / EDT_FAR: none)
EDT_HD void edt_row_summary(const EdtGeom& q, int rb, int tid, const short* row, int* sl, int* sr) {
  int r, y, x0, x1;
  edt_row_owner(q, rb, tid, &r, &y, &x0, &x1);
  int last = -EDT_FAR, first = EDT_FAR;
  if (y < q.H) {
    const short* a = row + r * EDT_ROW_LDS + edt_lds_index(q, x0) - x0;  // the segment is contiguous in LDS: place x at a[x]
    for (int x = x0; x < x1; ++x) {  // at most seg <= 64 rounds
      if (a[x] == 0) {
        last = x;
        first = first == EDT_FAR ? x : first;
      }
    }
  }
  sl[tid] = last, sr[tid] = first;
}

// phase C: the nearest non-selected column to the left of the segment (over the summaries of the lanes before) and to its right
// (the lanes behind); then the segment forwards, leaving the distance to the left, and backwards, leaving the row offset
EDT_HD void edt_row_scan(const EdtGeom& q, int rb, int outside, int tid, short* row, const int* sl, const int* sr) {
  int r, y, x0, x1;
  edt_row_owner(q, rb, tid, &r, &y, &x0, &x1);
  if (y >= q.H) return;
  const int l = tid - r * EDT_LANES;
  int last = outside ? -1 : -EDT_FAR, next = outside ? q.W : EDT_FAR;
  for (int j = 0; j < l; ++j) last = sl[r * EDT_LANES + j] > last ? sl[r * EDT_LANES + j] : last;                // at most 63 rounds
  for (int j = l + 1; j < EDT_LANES; ++j) next = sr[r * EDT_LANES + j] < next ? sr[r * EDT_LANES + j] : next;  // at most 63 rounds
  if (x0 >= x1) return;  // a lane behind the row's end owns nothing
  short* a = row + r * EDT_ROW_LDS + edt_lds_index(q, x0) - x0;  // the segment is contiguous in LDS: place x at a[x]
  for (int x = x0; x < x1; ++x) {  // at most seg rounds
    if (a[x] == 0) {
      last = x;
    } else {
      const int dl = x - last;
      a[x] = (short)(dl < EDT_ROW_FAR ? dl : EDT_ROW_FAR);
    }
  }
  for (int x = x1 - 1; x >= x0; --x) {  // at most seg rounds
    const int dl = a[x];
    if (dl == 0) {
      next = x;
      continue;
    }
    const int dr = next - x;  // > EDT_ROW_FAR when there is none to the right
    // the lower column on a tie: the left one.  dl == EDT_ROW_FAR <= dr: none on either side
    a[x] = (short)(dl <= dr ? (dl == EDT_ROW_FAR ? EDT_NO_ROW : -dl) : dr);
  }
}

// phase D: store, lane-contiguous along x
EDT_HD void edt_row_store(const EdtGeom& q, int rb, int tid, const short* row, short* g) {
  for (int r = 0; r < EDT_RROWS; ++r) {  // fixed trip count
    const int y = rb * EDT_RROWS + r;
    if (y >= q.H) break;
    // terminates: x grows by EDT_THREADS each round and the loop ends at x >= W
    for (int x = tid; x < q.W; x += EDT_THREADS) g[(long long)y * q.W + x] = row[r * EDT_ROW_LDS + edt_lds_index(q, x)];
  }
}

// ---- the column pass ------------------------------------------------------------------------------------------------------------------
// the pixel that thread tid of tile t owns in its round j of EDT_CROWS; x >= W or y >= H: none
EDT_HD void edt_col_owner(const EdtGeom& q, int t, int tid, int j, int* y, int* x) {
  const int tyi = t / q.ctx, txi = t - tyi * q.ctx;
  *x = txi * EDT_CX + tid % EDT_LANES;
  *y = tyi * EDT_CY + j * EDT_RROWS + tid / EDT_LANES;
}

struct EdtHit {
  int d2;     // the squared distance; 0: the pixel is not selected; EDT_NONE: no candidate
  int yn;     // the row of the nearest non-selected pixel (its column is x + g[yn * W + x]); -1: none.  Not read with `outside`
  int steps;  // rows looked at above or below, for the host program's cap
};

// d2(y, x) = min over y' of (y - y')^2 + g(y', x)^2, searched outwards from y' = y.  Every row index is clamped into
// 0 .. H - 1 before it is used, so every read lies inside the plane.
//   ties = 0: only d2 is wanted; the search stops as soon as k^2 >= best (no row further away can be strictly nearer)
//   ties = 1: the nearest pixel is wanted too; it goes on while k^2 <= best, since a row with k^2 == best and g == 0 ties
// A candidate above (row y - k) replaces an equal one: it is the lowest row seen so far; one below (y + k) only a larger one.
// Within one round the EDT_U rows of either side are looked at without a test in between (loads in flight): a row beyond the
// stopping distance has k^2 + g^2 >= k^2 > best (>= best without ties, where an equal replacement changes nothing that is read).
// No overflow: k <= 4095 + EDT_U, |g| <= 4096, so k^2 + g^2 <= 2 * 4099^2 < 2^26; EDT_NO_ROW is tested for and never squared.
EDT_HD EdtHit edt_search(const short* g, int H, int W, int y, int x, int outside, int ties) {
  EdtHit h;
  h.steps = 0;
  const int o = g[y * W + x];
  if (o == 0) {
    h.d2 = 0, h.yn = -1;
    return h;
  }
  int best = o == EDT_NO_ROW ? EDT_NONE : o * o, by = o == EDT_NO_ROW ? -1 : y;
  if (outside) {
    const int b = y + 1 < H - y ? y + 1 : H - y;
    best = b * b < best ? b * b : best;
  }
  const int kmax = y > H - 1 - y ? y : H - 1 - y;
  // terminates: k grows by EDT_U each round and the loop ends at k > kmax = max(y, H - 1 - y) <= 4095 at the latest
  for (int k = 1; k <= kmax && (ties ? k * k <= best : k * k < best); k += EDT_U) {
    int up[EDT_U], dn[EDT_U];
    for (int u = 0; u < EDT_U; ++u) {  // fixed trip count: the loads
      const int a = y - k - u, b = y + k + u;
      up[u] = g[(a < 0 ? 0 : a) * W + x];
      dn[u] = g[(b > H - 1 ? H - 1 : b) * W + x];
    }
    for (int u = 0; u < EDT_U; ++u) {  // fixed trip count
      const int kk = k + u;
      if (y - kk >= 0 && up[u] != EDT_NO_ROW) {
        const int c = kk * kk + up[u] * up[u];
        if (c <= best) best = c, by = y - kk;
      }
      if (y + kk < H && dn[u] != EDT_NO_ROW) {
        const int c = kk * kk + dn[u] * dn[u];
        if (c < best) best = c, by = y + kk;
      }
      h.steps += kk <= kmax;
    }
  }
  h.d2 = best, h.yn = by;
  return h;
}

// the peak as one unsigned maximum: d2 in the high word, 2^31 - 1 - i in the low: the larger d2, then the lower index.
// Only pixels with d2 > 0 give a key; 0 is "none" and decodes to (0, -1).
EDT_HD unsigned long long edt_peak_key(int d2, int i) {
  return d2 > 0 ? ((unsigned long long)(unsigned)d2 << 32) | (unsigned)(0x7fffffff - i) : 0ull;
}
EDT_HD int edt_peak_d2(unsigned long long key) { return (int)(unsigned)(key >> 32); }
EDT_HD int edt_peak_index(unsigned long long key) { return key ? 0x7fffffff - (int)(unsigned)(key & 0xffffffffull) : -1; }

// ---- the workspace ------------------------------------------------------------------------------------------------------------------
// [ g : 2 P H W, rounded up to 16 ][ slots : 8 P ctiles ]   one slot (two int32) per column-pass tile: 8 bytes per 1024 pixels
struct EdtWork {
  long long g, slots, bytes;  // byte offsets
};

EDT_HD EdtWork edt_work(const EdtGeom& q) {
  EdtWork w;
  w.g = 0;
  w.slots = (2ll * q.P * q.H * q.W + 15) / 16 * 16;
  w.bytes = w.slots + 8ll * q.P * q.ctiles;
  return w;
}

EDT_HD long long edt_slot(const EdtGeom& q, int plane, int tile) { return 2 * ((long long)plane * q.ctiles + tile); }  // in int32

}  // namespace vdr
