// Host program (its own main) over csrc/mask_stats_map.h, the mapping the mask statistics kernels (csrc/mask_stats.hip) are
// written on: it walks every work item the launch makes, exactly as the kernels do, and checks that every source row an item
// stages and every source element it reads lies inside its plane (and inside the stage), that every output pixel belongs to
// exactly one (item, thread), and that every partial slot has one writer and one reader.  Built and run by
// tests/test_amg_cpu.py, once plainly and once with -fsanitize=address,undefined.
#include <cstdio>
#include <vector>

#include "mask_stats_map.h"

using namespace vdr;

static long long fails = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (fails++ < 10) std::printf("FAIL %s (line %d)\n", #cond, __LINE__);   \
    }                                                                          \
  } while (0)

// layout 0: one token of [P, 4, H, W] (group 1); 1: tokens 1 .. 3 of [P / 3, 4, H, W] (group 3); 2: dense planes (group = P)
static void walk(int P, int H, int W, int oh, int ow, int layout) {
  const MsGeom q = ms_geom(P, H, W, oh, ow);
  const long long HW = (long long)H * W;
  const int group = layout == 0 ? 1 : layout == 1 ? 3 : P;
  const long long plane_stride = HW, group_stride = layout == 2 ? 0 : 4 * HW, base = layout == 1 ? HW : 0;
  const long long extent = layout == 2 ? P * HW : (long long)(layout == 1 ? P / 3 : P) * 4 * HW;
  std::vector<float> in((size_t)extent, 1.0f);
  std::vector<float> stage((size_t)MS_STAGE_ROWS * MS_MAX_SIDE, 0.0f);
  std::vector<unsigned char> owners((size_t)oh * ow, 0);
  std::vector<unsigned char> written((size_t)ms_slots(q), 0), read((size_t)ms_slots(q), 0);
  float sink = 0.0f;
  CHECK(q.rows >= 1 && q.rows <= MS_BAND && q.bands == (oh + q.rows - 1) / q.rows);
  int max_stage = 0;
  for (long long item = 0; item < ms_slots(q); ++item) {
    const long long plane = item / q.bands;
    const int band = (int)(item - plane * q.bands);
    const MsBand b = ms_band(q, band);
    CHECK(b.r0 >= 0 && b.r0 < b.r1 && b.r1 <= oh && b.r1 - b.r0 <= MS_BAND);
    CHECK(b.lo >= 0 && b.n >= 1 && b.n <= MS_STAGE_ROWS && b.lo + b.n <= H);
    max_stage = b.n > max_stage ? b.n : max_stage;
    // the staging copy: b.n * W contiguous elements of the plane from row b.lo
    const long long off = base + ms_plane_offset(plane, group, group_stride, plane_stride) + (long long)b.lo * W;
    const long long total = (long long)b.n * W;
    CHECK(off >= 0 && off + total <= extent && total <= (long long)stage.size());
    if (!(off >= 0 && off + total <= extent && total <= (long long)stage.size())) continue;
    for (long long i = 0; i < total; ++i) stage[(size_t)i] = in[(size_t)(off + i)];
    if (plane > 0) {  // the pixel map is the same for every plane: walk it once, for plane 0
      CHECK(ms_slot(q, plane, band, 0) == item * MS_SLOT);
      ++written[(size_t)item];
      continue;
    }
    for (int tid = 0; tid < MS_THREADS; ++tid) {
      for (int ox = tid; ox < ow; ox += MS_THREADS) {
        const MsAxis cx = ms_axis(ox, q.sx, W);
        CHECK(cx.i0 >= 0 && cx.i0 <= cx.i1 && cx.i1 < W && cx.i1 - cx.i0 <= 1);
        for (int r = 0; r < b.r1 - b.r0; ++r) {
          const MsAxis ry = ms_axis(b.r0 + r, q.sy, H);
          CHECK(ry.i0 >= b.lo && ry.i0 <= ry.i1 && ry.i1 < b.lo + b.n && ry.i1 - ry.i0 <= 1);
          CHECK(ry.l1 >= 0.0f && ry.l1 <= 1.0f && cx.l1 >= 0.0f && cx.l1 <= 1.0f);
          const long long a = (long long)(ry.i0 - b.lo) * W + cx.i0, d = (long long)(ry.i1 - b.lo) * W + cx.i1;
          CHECK(a >= 0 && d < total);
          if (a >= 0 && d < total) sink += stage[(size_t)a] + stage[(size_t)d];
          ++owners[(size_t)(b.r0 + r) * ow + ox];
        }
      }
    }
    CHECK(ms_slot(q, plane, band, 0) == item * MS_SLOT && ms_slot(q, plane, band, 6) == item * MS_SLOT + 6);
    ++written[(size_t)item];
  }
  // the finish: lane (band mod 64) of plane p's wave reads slot (p, band)
  for (long long plane = 0; plane < P; ++plane)
    for (int lane = 0; lane < 64; ++lane)
      for (int band = lane; band < q.bands; band += 64) {
        const long long s = ms_slot(q, plane, band, 0);
        CHECK(s >= 0 && s % MS_SLOT == 0 && s / MS_SLOT < ms_slots(q));
        if (s >= 0 && s / MS_SLOT < ms_slots(q)) ++read[(size_t)(s / MS_SLOT)];
      }
  long long unowned = 0, twice = 0, slot_bad = 0;
  for (unsigned char o : owners) unowned += o == 0, twice += o > 1;
  for (size_t i = 0; i < written.size(); ++i) slot_bad += written[i] != 1 || read[i] != 1;
  CHECK(unowned == 0);
  CHECK(twice == 0);
  CHECK(slot_bad == 0);
  std::printf("P %d H %d W %d oh %d ow %d layout %d: rows %d bands %d stage %d unowned %lld twice %lld slots %lld bad %lld (%g)\n", P, H, W, oh, ow,
              layout, q.rows, q.bands, max_stage, unowned, twice, ms_slots(q), slot_bad, (double)sink);
}

int main() {
  const int shapes[][4] = {{1, 1, 3, 5},       {8, 8, 32, 32},     {12, 20, 50, 75},  {17, 3, 9, 2},     {64, 64, 256, 256},
                           {256, 256, 1024, 1024}, {256, 256, 1, 1},   {256, 256, 2, 2},  {256, 1, 100, 7},  {1, 256, 7, 4096},
                           {256, 8, 4096, 5},  {256, 256, 255, 257}, {200, 256, 13, 300}, {3, 5, 4096, 64}, {256, 256, 9, 9},
                           {255, 7, 31, 1}};
  int cases = 0;
  for (const auto& s : shapes)
    for (int layout = 0; layout < 3; ++layout) {
      walk(layout == 1 ? 6 : 3, s[0], s[1], s[2], s[3], layout);
      ++cases;
    }
  // every down-sampling ratio of the tallest plane: the staged rows must fit whatever the ratio
  for (int oh = 1; oh <= 256; ++oh) {
    const MsGeom q = ms_geom(1, 256, 4, oh, 1);
    for (int band = 0; band < q.bands; ++band) {
      const MsBand b = ms_band(q, band);
      CHECK(b.n >= 1 && b.n <= MS_STAGE_ROWS && b.lo >= 0 && b.lo + b.n <= 256);
    }
  }
  std::printf("cases %d fails %lld\n", cases, fails);
  return fails ? 1 : 0;
}
