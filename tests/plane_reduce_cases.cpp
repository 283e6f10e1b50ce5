// Host program over csrc/plane_reduce.h, the integer reduction of the mask-plane kernels: the combine rules, identity and slot
// layout the kernels compile, walked as plain C++ (its own main; the tests build it plainly and under the sanitizers).  Per NS
// and plane size: the identity is neutral; combine is commutative and associative on designed values (the all-empty
// accumulator, a single pixel at (0, 0) and at (W - 1, H - 1), sums at and next to 2^24, a full plane); a slot round-trips and
// the store touches NS + 4 values only; a plane's per-pixel accumulators reduced forwards, reversed, as a pairwise tree and as
// four "waves" through pr_waves_value give the integers of a brute-force count and box.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "plane_reduce.h"

using namespace vdr;

template <int NS> static bool same(const PlaneAcc<NS>& a, const PlaneAcc<NS>& b) {
  for (int k = 0; k < NS + 4; ++k)
    if (a.v[k] != b.v[k]) return false;
  return true;
}

// pixel (x, y) as the kernels count it: sum k gets bit k of `bits`, the box takes the pixel when bit 0 is set
template <int NS> static PlaneAcc<NS> pixel(int W, int H, int x, int y, unsigned bits) {
  PlaneAcc<NS> a = pr_identity<NS>(W, H);
  for (int k = 0; k < NS; ++k) a.sum(k) += (bits >> k) & 1;
  if (bits & 1) a.take(x, y);
  return a;
}

template <int NS> static PlaneAcc<NS> tree(const std::vector<PlaneAcc<NS>>& v, size_t lo, size_t hi, const PlaneAcc<NS>& id) {
  if (hi - lo <= 1) return hi == lo ? id : v[lo];
  return pr_combine(tree<NS>(v, lo, lo + (hi - lo) / 2, id), tree<NS>(v, lo + (hi - lo) / 2, hi, id));
}

template <int NS> static int plane_case(int W, int H, unsigned seed) {
  int fails = 0;
  const PlaneAcc<NS> id = pr_identity<NS>(W, H);
  std::vector<PlaneAcc<NS>> d = {id, pixel<NS>(W, H, 0, 0, 1), pixel<NS>(W, H, W - 1, H - 1, 1), pixel<NS>(W, H, W / 2, H / 3, ~0u)};
  for (int big : {(1 << 24) - 1, 1 << 24, (1 << 24) - W * H, W * H}) {  // (the last: a full plane)
    PlaneAcc<NS> a = pixel<NS>(W, H, W - 1, 0, 1);
    a.take(0, H - 1);
    for (int k = 0; k < NS; ++k) a.sum(k) = big - k;
    d.push_back(a);
  }
  for (const auto& a : d) {
    fails += !same(pr_combine(id, a), a) + !same(pr_combine(a, id), a);
    int32_t slot[PR_SLOT + 2];
    for (int32_t& s : slot) s = -77;
    pr_store(a, slot + 1);
    fails += !same(pr_load<NS>(slot + 1), a) || slot[0] != -77;
    for (int k = NS + 4; k < PR_SLOT + 1; ++k) fails += slot[1 + k] != -77;
    for (const auto& b : d) {  // (three sums near 2^24 stay far below 2^31)
      fails += !same(pr_combine(a, b), pr_combine(b, a));
      for (const auto& c : d) fails += !same(pr_combine(pr_combine(a, b), c), pr_combine(a, pr_combine(b, c)));
    }
  }
  for (int density = 0; density < 4; ++density) {  // empty, sparse, half, full: every order against brute force
    std::vector<PlaneAcc<NS>> px;
    PlaneAcc<NS> want = id, fwd = id, rev = id, wave[4] = {id, id, id, id}, blk;
    unsigned s = seed * 2654435761u + density;
    for (int i = 0; i < W * H; ++i) {
      const int x = i % W, y = i / W;
      s = s * 1664525u + 1013904223u;
      const unsigned r = s >> 8;
      const unsigned bits = (density == 0 ? 0u : density == 3 ? ~0u : (r % (density == 1 ? 97 : 2) == 0 ? 1u : 0u) | ((r >> 9) & 6u)) & ((1u << NS) - 1);
      px.push_back(pixel<NS>(W, H, x, y, bits));
      for (int k = 0; k < NS; ++k) want.v[k] += (bits >> k) & 1;  // brute force: counts, then the box by comparisons
      if (bits & 1) {
        if (x < want.v[NS]) want.v[NS] = x;
        if (y < want.v[NS + 1]) want.v[NS + 1] = y;
        if (x > want.v[NS + 2]) want.v[NS + 2] = x;
        if (y > want.v[NS + 3]) want.v[NS + 3] = y;
      }
    }
    for (size_t i = 0; i < px.size(); ++i) {  // (the waves: pixels dealt round-robin; a wave may stay at the identity)
      fwd = pr_combine(fwd, px[i]), rev = pr_combine(rev, px[px.size() - 1 - i]);
      wave[i % 4] = pr_combine(wave[i % 4], px[i]);
    }
    int wred[4][PR_SLOT];
    for (int w = 0; w < 4; ++w) pr_store(wave[w], wred[w]);
    for (int k = 0; k < NS + 4; ++k) blk.v[k] = pr_waves_value<NS, 4>(wred, k);
    fails += !same(fwd, want) + !same(rev, want) + !same(tree<NS>(px, 0, px.size(), id), want) + !same(blk, want);
    if (density == 0) fails += !same(want, id);
    if (density == 3) fails += want.box(0) != 0 || want.box(1) != 0 || want.box(2) != W - 1 || want.box(3) != H - 1 || want.sum(0) != W * H;
  }
  std::printf("NS %d W %d H %d: designed %zu fails %d\n", NS, W, H, d.size(), fails);
  return fails;
}

int main() {
  const int shapes[][2] = {{1, 1}, {7, 1}, {1, 9}, {64, 4}, {65, 5}, {33, 128}, {256, 256}, {517, 300}};
  int cases = 0, fails = 0;
  unsigned seed = 1;
  for (const auto& s : shapes) {
    fails += plane_case<1>(s[0], s[1], seed) + plane_case<2>(s[0], s[1], seed + 1) + plane_case<3>(s[0], s[1], seed + 2);
    cases += 3, seed += 3;
  }
  std::printf("cases %d fails %d\n", cases, fails);
  return fails != 0;
}
