// Host program (its own main) over csrc/mask_embed_map.h, the mapping the fused keys kernel (csrc/mask_prompt.hip) is written on:
// it walks every tile and row the launch makes, exactly as the kernel does, and checks that every embedding and mask read stays
// inside its extent, that every element of keys has one writer, and that none is left unwritten.  Built and run by
// tests/test_sam_prompts_cpu.py, once plainly and once with -fsanitize=address,undefined.
#include <cstdio>
#include <vector>

#include "mask_embed_map.h"

using namespace vdr;

static long long fails = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (fails++ < 10) std::printf("FAIL %s (line %d)\n", #cond, __LINE__);   \
    }                                                                          \
  } while (0)

static void walk(int g, int P, int nb, int channels_last, int mask_per_image) {
  const MeGeom q = me_geom(P, nb, g, channels_last, mask_per_image);
  const int B = P / nb, n = g * g;
  const long long emb_extent = (long long)B * ME_C * n;
  const long long mask_extent = (long long)(mask_per_image ? B : P) * 16 * n;
  std::vector<unsigned char> writers((size_t)q.rows * ME_C, 0);
  std::vector<float> emb((size_t)emb_extent, 1.0f), mask((size_t)mask_extent, 1.0f);
  float sink = 0.0f;
  CHECK(q.tiles == (q.rows + ME_CELLS - 1) / ME_CELLS);
  for (long long tile = 0; tile < q.tiles; ++tile) {
    for (int i = 0; i < ME_CELLS; ++i) {
      const MeRow r = me_row(q, tile, i);
      CHECK(r.R >= 0 && r.R < q.rows);
      CHECK(r.ok == (tile * ME_CELLS + i < q.rows));
      CHECK(r.p >= 0 && r.p < P && r.b == r.p / nb && r.b < B);
      CHECK(r.m == (mask_per_image ? r.p / nb : r.p));
      CHECK(r.cy >= 0 && r.cy < g && r.cx >= 0 && r.cx < g && r.cell == r.cy * g + r.cx);
      // the staging loads: every channel of the row (the channel-last path reads 4 at a time from a multiple of 4)
      for (int c = 0; c < ME_C; ++c) {
        const long long o = me_emb_offset(q, r, c);
        CHECK(o >= 0 && o < emb_extent);
        if (o >= 0 && o < emb_extent) sink += emb[(size_t)o];
        if (channels_last && (c & 3) == 0) CHECK((o & 3) == 0 && o + 3 < emb_extent);
      }
      for (int py = 0; py < 4; ++py) {
        const long long o = me_mask_offset(q, r, py);
        CHECK(o >= 0 && (o & 3) == 0 && o + 3 < mask_extent);   // one 16-byte load
        if (o >= 0 && o + 3 < mask_extent) sink += mask[(size_t)o] + mask[(size_t)o + 3];
      }
      if (!r.ok) continue;
      for (int c = 0; c < ME_C; ++c) {
        const long long o = me_key_offset(r, c);
        CHECK(o >= 0 && o < q.rows * ME_C);
        if (o >= 0 && o < q.rows * ME_C) ++writers[(size_t)o];
      }
    }
    // the store: the rows of a tile are one contiguous run of keys, cut at the end of the last tile
    const long long row0 = tile * ME_CELLS, left = q.rows - row0;
    const long long chunks = (left < ME_CELLS ? left : ME_CELLS) * (ME_C / 8);
    CHECK(row0 * ME_C + 8 * chunks <= q.rows * ME_C);
    CHECK(me_key_offset(me_row(q, tile, 0), 0) == row0 * ME_C);
  }
  long long unwritten = 0, twice = 0;
  for (unsigned char w : writers) {
    unwritten += w == 0;
    twice += w > 1;
  }
  CHECK(unwritten == 0);
  CHECK(twice == 0);
  std::printf("g %d P %d nb %d channels_last %d mask_per_image %d: tiles %lld rows %lld unwritten %lld twice %lld (%g)\n", g, P, nb, channels_last,
              mask_per_image, q.tiles, q.rows, unwritten, twice, (double)sink);
}

int main() {
  int cases = 0;
  for (int g : {1, 3, 10, 64})
    for (int P : {1, 3, 5})
      for (int nb : {1, 3})
        for (int cl = 0; cl < 2; ++cl)
          for (int mpi = 0; mpi < 2; ++mpi) {
            if (P % nb) continue;  // a call has whole images
            walk(g, P, nb, cl, mpi);
            ++cases;
          }
  std::printf("cases %d fails %lld\n", cases, fails);
  return fails ? 1 : 0;
}
