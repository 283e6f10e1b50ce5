// The 128 x 128 "row by row over d" MFMA tile shared by nn_cosine.hip (X_p against Y_p) and the Gram kernel of pca.hip
// (Z_p against itself): both operands are [128 rows][64 bf16] LDS images of one 64-column K step, the product contracts
// over the contiguous index.
//   LDS image: 128-B rows, 16-B chunk c of row r at slot c ^ ((r >> 1) & 7) (the K image of attention_tile.h: conflict-free
//   ds_read_b128 fragment reads); the A operand at sx, the B operand at sx + T128_OPER.
//   Wave (wr, wc) of 4 owns the 64 x 64 sub-tile at (64 wr, 64 wc) as 2 x 2 mfma_f32_32x32x16_bf16 accumulators: a lane holds
//   ONE column j = 64 wc + 32 n + (lane & 31) of the B operand's rows and 16 rows i = 64 wr + 32 m + (e & 3) + 8 (e >> 2) +
//   4 (lane >> 5) of the A operand's.
#pragma once
#include "vdr_dev.h"

namespace vdr {

constexpr int T128 = 128;               // tile side
constexpr int T128_OPER = T128 * 128;   // bytes of one staged operand tile

// byte offset of 16-byte chunk ch (0..7) of row `row` in a staged operand tile
VDR_DEV int t128_off(int row, int ch) { return 128 * row + 16 * (ch ^ ((row >> 1) & 7)); }

// MFMA k-steps KS0 .. KS1-1 (16 columns each) of the staged 64-column step
template <int KS0, int KS1>
VDR_DEV void t128_mfma(const char* sx, int wr, int wc, int l31, int hh, f32x16 (&acc)[2][2]) {
  const int swz = (l31 >> 1) & 7;
#pragma unroll
  for (int ks = KS0; ks < KS1; ++ks) {
    const int off = ((2 * ks + hh) ^ swz) * 16;
    bf16x8 af[2], bf[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) af[m] = *reinterpret_cast<const bf16x8*>(sx + (wr * 64 + m * 32 + l31) * 128 + off);
#pragma unroll
    for (int n = 0; n < 2; ++n) bf[n] = *reinterpret_cast<const bf16x8*>(sx + T128_OPER + (wc * 64 + n * 32 + l31) * 128 + off);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[m], bf[n], acc[m][n], 0, 0, 0);
  }
}

// the four MFMA k-steps of a staged 64-column step with ONE A image against TWO B images accumulated into the same tile
// (kmeans.hip: X against the hi and the lo half of the centroids): per 16-column k-step the products with b0, then those with b1
VDR_DEV void t128_mfma_a2b(const char* sa, const char* sb0, const char* sb1, int wr, int wc, int l31, int hh, f32x16 (&acc)[2][2]) {
  const int swz = (l31 >> 1) & 7;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int off = ((2 * ks + hh) ^ swz) * 16;
    bf16x8 af[2], b0[2], b1[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) af[m] = *reinterpret_cast<const bf16x8*>(sa + (wr * 64 + m * 32 + l31) * 128 + off);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      b0[n] = *reinterpret_cast<const bf16x8*>(sb0 + (wc * 64 + n * 32 + l31) * 128 + off);
      b1[n] = *reinterpret_cast<const bf16x8*>(sb1 + (wc * 64 + n * 32 + l31) * 128 + off);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[m], b0[n], acc[m][n], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[m], b1[n], acc[m][n], 0, 0, 0);
  }
}

}  // namespace vdr
