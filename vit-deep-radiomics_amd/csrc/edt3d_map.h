// The ONE mapping and the TWO searches of the 3-D Euclidean distance transform kernels (edt3d.hip; the definition is
// vdr_op_distance_transform_3d's in include/vdr.h): the geometry of a call, what the y pass leaves per voxel, the outward searches
// along y and along z with their weights, the peak's order, the partial slots and the workspace sections.  The x pass is
// edt_map.h's row pass, phase function for phase function, over the P Z planes of the call.  The kernels, the launch plan and the
// host program tests/edt3d_map_cases.cpp all call what is here: the host program runs the very same functions thread by thread, in
// both orders, and counts the steps of every search.  It includes edt_map.h and nothing else, and compiles as plain C++.
//
//   volume   v of P: Z x H x W, voxel index i = (z H + y) W + x (int32: Z H W <= 2^30); plane z of volume v is plane v Z + z of P Z
//   spacing  (qz, qy, qx), integers in 1 .. 65535; the squared distance of an offset (dz, dy, dx) is (qz dz)^2 + (qy dy)^2 + (qx dx)^2
//   row g    int16 per voxel, edt_map.h's ROW OFFSET along x (with `outside` bit 0 the columns -1 and W count as not selected)
//   vec      uint32 per voxel, two int16: the low half ox, the high half oy -- the IN-PLANE VECTOR from the voxel to a nearest
//            non-selected pixel of its own plane under the weights (qy, qx); 0 for a voxel that is not selected (and only for one:
//            a selected voxel is at least one step from anything not selected); ox = EDT_NO_ROW when the plane has no candidate.
//            With `outside` bit 1 the rows -1 and H count: oy = -(y + 1) or H - y, ox = 0.  |oy| <= H, |ox| <= W.
//   y pass, z pass   edt_col_owner's tile of 64 columns x 16 rows of one plane, a thread a voxel, lanes along x
//   slot     two int64 per z-pass tile: the tile's largest d2 and the lowest voxel index that attains it (0, -1: none)
//
// Arithmetic: a weighted step q |o| is below 65535 * 4100 < 2^32 and is formed in 32 bits; its square is one 32 x 32 -> 64
// multiply; a candidate is the sum of at most three squares, each at most (q side)^2, so every real value is at most
// (qz Z)^2 + (qy H)^2 + (qx W)^2 <= 2^53 (edt3_shape_ok) and every intermediate below 3 * 2^58: signed 64-bit never overflows.
// Compares are int64 (gfx950 has v_cmp_*_u64 / i64 and v_mad_u64_u32; fp64 would cost a conversion per candidate and buy nothing).
#pragma once
#include "edt_map.h"

namespace vdr {

constexpr long long EDT3_NONE = 0x7fffffffffffffffll;  // VDR_EDT3_NONE: no candidate at all
constexpr int EDT3_MAX_Q = 65535;
constexpr long long EDT3_MAX_VOXELS = 1ll << 30;       // of one volume
constexpr long long EDT3_MAX_D2 = 1ll << 53;           // exact in int64 and in float64
constexpr int EDT3_U = 4;                              // rows / slices on either side a search looks at per round

struct Edt3Geom {
  int P, Z, H, W;
  unsigned qz, qy, qx;
  int outside;   // bit 2 = z, bit 1 = y, bit 0 = x
  EdtGeom pl;    // the P Z planes: the row pass's and the tiles' geometry
  int ztiles;    // z-pass tiles (and slots) of one volume: Z * pl.ctiles
};

// sides 1 .. 4096, P Z <= 65535, Z H W <= 2^30
EDT_HD bool edt3_shape_ok(int P, int Z, int H, int W) {
  if (P < 1 || Z < 1 || Z > EDT_MAX_SIDE || H < 1 || H > EDT_MAX_SIDE || W < 1 || W > EDT_MAX_SIDE) return false;
  return (long long)P * Z <= EDT_MAX_PLANES && (long long)Z * H * W <= EDT3_MAX_VOXELS;
}

// each q in 1 .. 65535 and (qz Z)^2 + (qy H)^2 + (qx W)^2 <= 2^53.  No overflow: a term is below (2^16 * 2^12)^2 = 2^56
EDT_HD bool edt3_spacing_ok(int Z, int H, int W, int qz, int qy, int qx) {
  if (qz < 1 || qz > EDT3_MAX_Q || qy < 1 || qy > EDT3_MAX_Q || qx < 1 || qx > EDT3_MAX_Q) return false;
  const long long a = (long long)qz * Z, b = (long long)qy * H, c = (long long)qx * W;
  return a * a + b * b + c * c <= EDT3_MAX_D2;
}

EDT_HD Edt3Geom edt3_geom(int P, int Z, int H, int W, int qz, int qy, int qx, int outside) {
  Edt3Geom q;
  q.P = P, q.Z = Z, q.H = H, q.W = W;
  q.qz = (unsigned)qz, q.qy = (unsigned)qy, q.qx = (unsigned)qx;
  q.outside = outside;
  q.pl = edt_geom(P * Z, H, W);
  q.ztiles = Z * q.pl.ctiles;
  return q;
}

// (q o)^2: q |o| in 32 bits (q <= 65535, |o| <= 4095 + EDT3_U: below 2^32), the square in 64
EDT_HD long long edt3_sq(unsigned q, int o) {
  const unsigned a = q * (unsigned)(o < 0 ? -o : o);
  return (long long)((unsigned long long)a * a);
}

EDT_HD unsigned edt3_pack(int oy, int ox) { return ((unsigned)(oy & 0xffff) << 16) | (unsigned)(ox & 0xffff); }
EDT_HD int edt3_oy(unsigned v) { return (int)(short)(unsigned short)(v >> 16); }
EDT_HD int edt3_ox(unsigned v) { return (int)(short)(unsigned short)(v & 0xffffu); }
// the in-plane squared distance a vector stands for; EDT3_NONE for "no candidate in this plane", 0 for a voxel that is not selected
EDT_HD long long edt3_g2(unsigned qy, unsigned qx, unsigned v) {
  const int ox = edt3_ox(v);
  return ox == EDT_NO_ROW ? EDT3_NONE : edt3_sq(qy, edt3_oy(v)) + edt3_sq(qx, ox);
}

struct Edt3Hit {
  long long d2;  // y search: the in-plane value of vec (EDT3_NONE: none); z search: the voxel's d2
  unsigned vec;  // y search only
  int steps;     // rows / slices looked at on one side, for the host program's cap
};

// thr < 0: the full search.  thr = r2 >= 0: the call wants `within` alone, and a search may also end where nothing further
// out can matter to d2 <= r2 (below).

// The y search: vec(y, x) = the offset that attains min over y' of (qy (y - y'))^2 + (qx g(y', x))^2, searched outwards from
// y' = y; every row index is clamped into 0 .. H - 1 before it is used.  It stops as soon as (qy k)^2 >= best: no row further
// away can be strictly nearer.  Within a round the EDT3_U rows of either side are looked at without a test in between (loads in
// flight): a row beyond the stopping distance has a candidate >= (qy k)^2 >= best and replaces nothing (strict comparison).
// thr >= 0: it also stops when (qy k)^2 > thr.  Every row not yet seen then has an in-plane value > thr, so no voxel of this
// column, in any slice, can come within thr through it: the vector left behind is the true one if its value is <= thr and stands
// for some value > thr otherwise, and `within` needs no more.  It does NOT stop at best <= thr: a row further out may still be
// nearer in the plane, and a voxel two slices away may need exactly that difference.
EDT_HD Edt3Hit edt3_search_y(const short* g, int H, int W, int y, int x, unsigned qy, unsigned qx, int outside_y, long long thr) {
  Edt3Hit h;
  h.steps = 0;
  const int o = g[y * W + x];
  if (o == 0) {
    h.d2 = 0, h.vec = 0;
    return h;
  }
  long long best = o == EDT_NO_ROW ? EDT3_NONE : edt3_sq(qx, o);
  int oy = 0, ox = o;
  if (outside_y) {
    const int up = y + 1, dn = H - y;
    const int b = up <= dn ? -up : dn;
    const long long c = edt3_sq(qy, b);
    if (c < best) best = c, oy = b, ox = 0;
  }
  const int kmax = y > H - 1 - y ? y : H - 1 - y;
  // terminates: k grows by EDT3_U each round and the loop ends at k > kmax = max(y, H - 1 - y) <= 4095 at the latest
  for (int k = 1; k <= kmax; k += EDT3_U) {
    const long long k2 = edt3_sq(qy, k);
    if (k2 >= best || (thr >= 0 && k2 > thr)) break;
    int up[EDT3_U], dn[EDT3_U];
    for (int u = 0; u < EDT3_U; ++u) {  // fixed trip count: the loads
      const int a = y - k - u, b = y + k + u;
      up[u] = g[(a < 0 ? 0 : a) * W + x];
      dn[u] = g[(b > H - 1 ? H - 1 : b) * W + x];
    }
    for (int u = 0; u < EDT3_U; ++u) {  // fixed trip count
      const int kk = k + u;
      const long long kk2 = edt3_sq(qy, kk);
      if (y - kk >= 0 && up[u] != EDT_NO_ROW) {
        const long long c = kk2 + edt3_sq(qx, up[u]);
        if (c < best) best = c, oy = -kk, ox = up[u];
      }
      if (y + kk < H && dn[u] != EDT_NO_ROW) {
        const long long c = kk2 + edt3_sq(qx, dn[u]);
        if (c < best) best = c, oy = kk, ox = dn[u];
      }
      h.steps += kk <= kmax;
    }
  }
  h.d2 = best;
  h.vec = best == EDT3_NONE ? edt3_pack(0, EDT_NO_ROW) : edt3_pack(oy, ox);
  return h;
}

// The z search: d2(z, y, x) = min over z' of (qz (z - z'))^2 + g2(vec(z', y, x)), searched outwards from z' = z over the
// slices of ONE volume (vec points at its slice 0; hw = H W; yx = y W + x); every slice index is clamped into 0 .. Z - 1 before
// it is used, so every read lies inside the volume.  It stops as soon as (qz k)^2 >= best, at most max(z, Z - 1 - z) steps.
// thr >= 0: it also stops at best <= thr (the voxel is inside already) and at (qz k)^2 > thr (nothing further out can bring it
// inside); best <= thr holds at the end exactly when the full search's does.
EDT_HD Edt3Hit edt3_search_z(const unsigned* vec, int Z, int hw, int z, int yx, unsigned qz, unsigned qy, unsigned qx, int outside_z,
                             long long thr) {
  Edt3Hit h;
  h.steps = 0, h.vec = 0;
  const unsigned own = vec[z * hw + yx];  // z hw + yx < Z H W <= 2^30
  if (own == 0) {
    h.d2 = 0;
    return h;
  }
  long long best = edt3_g2(qy, qx, own);
  if (outside_z) {
    const int b = z + 1 < Z - z ? z + 1 : Z - z;
    const long long c = edt3_sq(qz, b);
    best = c < best ? c : best;
  }
  const int kmax = z > Z - 1 - z ? z : Z - 1 - z;
  // terminates: k grows by EDT3_U each round and the loop ends at k > kmax = max(z, Z - 1 - z) <= 4095 at the latest
  for (int k = 1; k <= kmax; k += EDT3_U) {
    const long long k2 = edt3_sq(qz, k);
    if (k2 >= best || (thr >= 0 && (best <= thr || k2 > thr))) break;
    unsigned up[EDT3_U], dn[EDT3_U];
    for (int u = 0; u < EDT3_U; ++u) {  // fixed trip count: the loads
      const int a = z - k - u, b = z + k + u;
      up[u] = vec[(a < 0 ? 0 : a) * hw + yx];
      dn[u] = vec[(b > Z - 1 ? Z - 1 : b) * hw + yx];
    }
    for (int u = 0; u < EDT3_U; ++u) {  // fixed trip count
      const int kk = k + u;
      const long long kk2 = edt3_sq(qz, kk);
      if (z - kk >= 0 && edt3_ox(up[u]) != EDT_NO_ROW) {
        const long long c = kk2 + edt3_g2(qy, qx, up[u]);
        best = c < best ? c : best;
      }
      if (z + kk < Z && edt3_ox(dn[u]) != EDT_NO_ROW) {
        const long long c = kk2 + edt3_g2(qy, qx, dn[u]);
        best = c < best ? c : best;
      }
      h.steps += kk <= kmax;
    }
  }
  h.d2 = best;
  return h;
}

// the peak: the larger d2, then the lower voxel index; only voxels with d2 > 0 count.  (0, -1): none.  d2 reaches 2^63 - 1 and the
// index 2^30: the pair does not fit one 64-bit key, so it is reduced in two steps (the largest d2, then the lowest index among
// the ones that attain it), each through plane_reduce.h's key reduction.
struct Edt3Peak {
  long long d2, i;
};
EDT_HD Edt3Peak edt3_peak_none() {
  Edt3Peak p;
  p.d2 = 0, p.i = -1;
  return p;
}
EDT_HD void edt3_peak_take(Edt3Peak* p, long long d2, long long i) {
  if (i >= 0 && d2 > 0 && (d2 > p->d2 || (d2 == p->d2 && i < p->i))) p->d2 = d2, p->i = i;
}
// the second step's key of a candidate that attains the largest d2 `top` (0: it does not, or there is none): larger = lower index
EDT_HD unsigned long long edt3_index_key(const Edt3Peak& p, long long top) {
  return top > 0 && p.d2 == top && p.i >= 0 ? (unsigned long long)(0x7fffffffll - p.i) : 0ull;  // i < 2^30: the key is > 0
}
EDT_HD long long edt3_index_of_key(unsigned long long key) { return key ? 0x7fffffffll - (long long)key : -1; }

// ---- the workspace ------------------------------------------------------------------------------------------------------------------
// [ g : 2 N, rounded up to 16 ][ vec : 4 N, rounded up to 16 ][ slots : 16 P ztiles ]   N = P Z H W voxels
struct Edt3Work {
  long long g, vec, slots, bytes;  // byte offsets
};

EDT_HD Edt3Work edt3_work(int P, int Z, int H, int W) {
  Edt3Work w;
  const long long n = (long long)P * Z * H * W;
  const EdtGeom pl = edt_geom(P * Z, H, W);
  w.g = 0;
  w.vec = (2 * n + 15) / 16 * 16;
  w.slots = w.vec + (4 * n + 15) / 16 * 16;
  w.bytes = w.slots + 16ll * P * Z * pl.ctiles;
  return w;
}

EDT_HD long long edt3_slot(const Edt3Geom& q, int volume, int z, int tile) {  // in int64
  return 2 * (((long long)volume * q.Z + z) * q.pl.ctiles + tile);
}

}  // namespace vdr
