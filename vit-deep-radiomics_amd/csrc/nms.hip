// Greedy box non-maximum suppression for gfx950 (include/vdr.h, vdr_op_nms): torchvision's definition, bit for bit.
//
//   nms_matrix_kernel   position i of `order` against positions j > i: bit (j mod 64) of word [i][j / 64] of the suppression matrix is
//                       iou(i, j) > threshold.  A workgroup of 64 threads is one 64 x 64 block on or above the diagonal: the 64
//                       column boxes and their areas are staged in LDS, thread t builds the word of row t.  Words below the
//                       diagonal are neither written nor read.
//   nms_walk_kernel     ONE wave walks the matrix; lane w holds word w of the removed set (N <= 4096: 64 words).  Per block of
//                       64 positions: the 64 x 64 diagonal block is in registers (one word a lane, loaded one block ahead), so the
//                       serial part -- "is position i still alive, then add its row" -- is 64 steps of scalar work with no memory
//                       access; then the block's rows are OR-ed into the removed set, every row loaded and the rows that are not
//                       kept masked out, so that the loads are independent and coalesced (a row is 512 contiguous bytes).  The
//                       dependent chain is therefore one load latency per BLOCK, not per kept box.
//
// No atomics, a fixed order: bitwise reproducible.  Built with -ffp-contract=off (Makefile): (area_i + area_j) - inter with
// inter = w * h must not become one fused multiply-add.
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {

namespace {

__global__ __launch_bounds__(64) void nms_matrix_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ order, int N,
                                                        int words, float threshold, unsigned long long* __restrict__ mat) {
  const int cb = blockIdx.x, rb = blockIdx.y, t = threadIdx.x;
  if (cb < rb) return;
  __shared__ float cbox[64][5];
  auto load = [&](int pos, float* b) {  // the box at a position of `order`; an index outside 0 .. N - 1 reads nothing and suppresses nothing
    const int o = pos < N ? order[pos] : -1;
    const bool ok = (unsigned)o < (unsigned)N;
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = ok ? boxes[o * 4 + k] : nan;
    b[4] = (b[2] - b[0]) * (b[3] - b[1]);
  };
  load(cb * 64 + t, cbox[t]);
  __syncthreads();
  const int i = rb * 64 + t;
  if (i >= N) return;
  float bi[5];
  load(i, bi);
  const int left = N - cb * 64, ncol = left < 64 ? left : 64;
  unsigned long long bits = 0;
  for (int jj = rb == cb ? t + 1 : 0; jj < ncol; ++jj) {
    const float* bj = cbox[jj];
    const float xx0 = bi[0] > bj[0] ? bi[0] : bj[0], yy0 = bi[1] > bj[1] ? bi[1] : bj[1];
    const float xx1 = bi[2] < bj[2] ? bi[2] : bj[2], yy1 = bi[3] < bj[3] ? bi[3] : bj[3];
    float w = xx1 - xx0, h = yy1 - yy0;
    w = w < 0.0f ? 0.0f : w;
    h = h < 0.0f ? 0.0f : h;
    const float inter = w * h;
    const float iou = inter / ((bi[4] + bj[4]) - inter);
    if (iou > threshold) bits |= 1ull << jj;  // (a NaN -- two zero-area boxes -- does not suppress)
  }
  mat[(size_t)i * words + cb] = bits;
}

__device__ inline unsigned long long readlane64(unsigned long long v, int lane) {  // lane: uniform
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, lane), hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void nms_walk_kernel(const unsigned long long* __restrict__ mat, const int32_t* __restrict__ order, int N,
                                                      int words, uint8_t* __restrict__ keep, int32_t* __restrict__ kept,
                                                      int32_t* __restrict__ count) {
  const int lane = threadIdx.x;
  unsigned long long removed = 0;  // lane w: word w of the set of suppressed positions
  unsigned long long diag = lane < N ? mat[(size_t)lane * words] : 0;  // lane t: word b of row 64 b + t
  int total = 0;
  for (int b = 0; b < words; ++b) {
    const int base = b * 64, left = N - base, nb = left < 64 ? left : 64;
    unsigned long long next = 0;
    if (b + 1 < words && base + 64 + lane < N) next = mat[(size_t)(base + 64 + lane) * words + b + 1];
    unsigned long long cur = readlane64(removed, b), km = 0;
    for (int bit = 0; bit < nb; ++bit) {
      const unsigned long long row = readlane64(diag, bit);
      if (!((cur >> bit) & 1)) {
        km |= 1ull << bit;
        cur |= row;
      }
    }
    if (lane > b && lane < words) {
      // every row of the block is loaded, kept or not, and masked afterwards: loads under a branch on km cannot be batched, and
      // 64 rows one after the other were the whole cost of the all-kept case (a row that is not kept costs one 512-byte line)
      const unsigned long long* rowp = mat + (size_t)base * words + lane;
#pragma unroll 16
      for (int bit = 0; bit < nb; ++bit) {
        const unsigned long long row = rowp[(size_t)bit * words];
        removed |= ((km >> bit) & 1) ? row : 0ull;
      }
    }
    if (lane < nb) {
      const int o = order[base + lane];
      const int k = (int)((km >> lane) & 1);
      if ((unsigned)o < (unsigned)N) keep[o] = (uint8_t)k;
      if (k) kept[total + __popcll(km & ((1ull << lane) - 1))] = o;
    }
    total += __popcll(km);
    diag = next;
  }
  for (int i = total + lane; i < N; i += 64) kept[i] = -1;
  if (lane == 0) count[0] = total;
}

}  // namespace

size_t nms_workspace_bytes(int n) {
  if (n < 1 || n > NMS_MAX_BOXES) return 0;
  return (size_t)n * ((n + 63) / 64) * sizeof(unsigned long long);
}

hipError_t launch_nms(const float* boxes, const int32_t* order, int n, float iou_threshold, void* work, uint8_t* keep, int32_t* kept,
                      int32_t* count, hipStream_t s) {
  if (!nms_workspace_bytes(n)) return hipErrorInvalidValue;
  const int words = (n + 63) / 64;
  hipLaunchKernelGGL(nms_matrix_kernel, dim3((unsigned)words, (unsigned)words), dim3(64), 0, s, boxes, order, n, words, iou_threshold,
                     (unsigned long long*)work);
  hipLaunchKernelGGL(nms_walk_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)work, order, n, words, keep, kept, count);
  return hipGetLastError();
}

}  // namespace vdr
