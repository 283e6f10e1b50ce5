// The "contract over the ROW index" MFMA operand shared by the covariance kernel of pca.hip (Z^T Z) and the update kernel of
// kmeans.hip (onehot^T X): a staged [64 rows][128 x bf16] LDS image of one 64-row step, whose operand of a 16-row k-step --
// "a column of the image over 8 rows" -- is read with ds_read_b64_tr_b16.
//   LDS image: plain 256-byte rows, 16-byte chunk ch of row r at slot ch ^ (((r & 3) << 2) | ((r >> 2) & 3)).
//   Read: lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p+3 of a 4-row x 16-column block and receives column
//   (lane & 15) of the 4 rows.  A lane's 8 k-values are rows 4hh .. 4hh+3 and 8 + 4hh .. 8 + 4hh+3 of the k-step (hh = lane >> 5)
//   -- the same permutation on both operands, so the MFMA sums the right products.
#pragma once
#include "vdr_dev.h"

namespace vdr {

typedef __attribute__((address_space(3))) bf16x4 tr_lds_bf16x4;
typedef const __attribute__((address_space(3))) char* tr_lds_cptr;

constexpr int TR_STEP = 64;             // rows staged per step
constexpr int TR_IMG = TR_STEP * 256;   // bytes of one staged tile

// byte offset of 16-byte chunk ch (0..15) of row `row` in a staged [rows][128 x bf16] tile
VDR_DEV int tr_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// the operand of one 16-row k-step for the 32 columns at cb: column cb + (lane & 31), rows 4hh..4hh+3 | 8+4hh..8+4hh+3
VDR_DEV bf16x8 tr_read(tr_lds_cptr img, int ks, int cb, int lane) {
  const int hh = lane >> 5, dg = (lane >> 4) & 1, tq = (lane & 15) >> 2, tp = lane & 3;
  const int row = ks * 16 + 4 * hh + tq;
  const int ch = (cb >> 3) + 2 * dg + (tp >> 1);
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((tr_lds_bf16x4*)(img + tr_off(row, ch) + 8 * (tp & 1)));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((tr_lds_bf16x4*)(img + tr_off(row + 8, ch) + 8 * (tp & 1)));
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = lo[j];
    f[4 + j] = hi[j];
  }
  return f;
}

}  // namespace vdr
