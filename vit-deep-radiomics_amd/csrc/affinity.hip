// Thresholded patch-affinity graphs of dense descriptor maps for gfx950 (include/vdr.h, vdr_op_affinity_bits and
// vdr_op_bits_matvec): for `pairs` problems X_p [t, d] (bf16 rows ldx elements apart, problems x_stride apart, 0 allowed)
//   sim(i, j) = dot(x_i, x_j) * (rn(x_i) * rn(x_j)),   rn(v) = 1 / max(sqrt(sum v^2), 1e-8)   (cosine_rn of desc_tile.h)
//   B[i, j]   = sim(i, j) > tau, the diagonal cleared with exclude_diag
// written one BIT per pair: bit (j & 31) of word bits[p][i][j >> 5], rows `pitch` = 4 ceil(t / 128) words apart.  The two norms
// are multiplied FIRST: fp32 multiplication commutes, dot(i, j) and dot(j, i) are the same products summed in the same k order,
// so sim is symmetric bit for bit and so is B.  The t x t matrix of scores is never written: it exists one 128 x 128 tile at a
// time in MFMA accumulators, and the epilogue folds the tile into 4 words per row.
//
// Launches, no atomics:
//   aff_rnorm_kernel      rn of every row into `work` (row_sumsq: one wave per row; cosine_rn of desc_tile.h).
//   affinity_bits_kernel  256 threads; one work item = (problem, run of 128-column tiles, 128-row panel; run_split of
//                         desc_tile.h), nn_cosine_kernel's loop: per tile a K loop over d in steps of 64 stages the panel's
//                         rows (A operand) and the tile's rows (B operand) global -> LDS by LDS-DMA, two buffers, step s + 1
//                         in flight under the MFMAs of step s.  Like nn_cosine_kernel it keeps its own copy of dma_steps /
//                         t128_dma_stage of desc_tile.h (1 - 3 % slower through the helpers); the source chunk a
//                         lane copies (t128_dma_chunk) and the wait (dma_wait) are the header's.
//                         Epilogue per tile: a lane holds ONE column and 16 rows per accumulator (desc_tile.h), so the wave
//                         ballot of `sim > tau` for element e of acc[m][n] is 32 columns of row acc_row(wr, m, e, 0) in its low
//                         half and the same 32 columns of row acc_row(wr, m, e, 1) in its high half: two finished words.  Word
//                         (m, e, hh, n) is kept by lane 32 hh + 16 m + e in register n (a select per ballot), and each lane
//                         stores its two words -- columns 64 wc .. 64 wc + 63 of one row -- with one 8-byte store.  Ragged
//                         columns and the diagonal are cleared on the finished words, ragged rows are not stored;
//                         pitch * 32 == 128 * ntiles, so the padding words are those zeros.  Every word has exactly one writer.
//   bits_matvec_kernel    Y[p, i, c] = sum over j with B[i, j] of V[p, j, c]: per row 64 lane sums -- lane l adds the set bits of
//                         words l, l + 64, ... in ascending word order, ascending bit order within a word, starting from 0.0f --
//                         folded by wave_sum (xor butterfly 32, 16, .., 1).  degree is the popcount of the row.  V is staged
//                         through LDS and shared by the 16 rows of a workgroup (at the kernel).
// Every value is a function of (t, nv, inputs) alone: the split of the column tiles into runs only decides which workgroup
// computes a word, never how.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "desc_tile.h"
#include "vdr_dev.h"
#include "vdr_kernels.h"

namespace vdr {
namespace {

constexpr int AF_T = T128;
constexpr int AF_RN = 4 * T128_OPER;        // s_rn [2][256] float: tile parity x (rn of the tile's rows | of the panel's rows)
constexpr int AF_LDS = AF_RN + 2048;

struct AffArgs {
  const bf16_t* x;
  int64_t ldx, xs;
  int t, d, npanels, nsplit, t_pad, pitch, exclude_diag;
  int split_base, split_rem;  // tiles per run: npanels / nsplit, and the first npanels % nsplit runs take one more
  float tau;
  float* rn;        // [pairs][t_pad]
  uint32_t* bits;   // [pairs][t][pitch]
};

// rn of every row into `work`.  The kernel's own one-sided copy of cosine_rnorm_kernel (nn_cosine.hip): through the two-sided
// kernel the op ran 0.2 - 5.8 us (0.3 - 2.6 %) slower at an A/A spread of 0.1 - 0.6 %
__global__ __launch_bounds__(256) void aff_rnorm_kernel(AffArgs a, int pairs) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)pairs * a.t) return;
  const int64_t p = row / a.t;
  const int i = (int)(row - p * a.t);
  const float ss = row_sumsq(a.x + p * a.xs + (int64_t)i * a.ldx, a.d, lane);
  if (lane == 0) a.rn[p * a.t_pad + i] = cosine_rn(ss);
}

// one K step of (panel, tile jt) into staging buffer `buf`: 4 + 4 DMA instructions per wave, 8 rows x 128 B each
VDR_DEV void aff_stage(const AffArgs& a, const bf16_t* xp, int64_t p, int panel, int jt, int kk, char* smem, int buf, int wave,
                       int lane) {
  const int k0 = kk * 64;
  const bool shortk = a.d - k0 < 64;
  char* sx = smem + buf * 2 * T128_OPER;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int piece = wave * 4 + q;
    const int r = piece * 8 + (lane >> 3);
    const int c = t128_dma_chunk(lane, r, shortk);
    const int xr = min(panel * AF_T + r, a.t - 1), yr = min(jt * AF_T + r, a.t - 1);
    glds16_raw(xp + (int64_t)xr * a.ldx + k0 + c * 8, sx + piece * 1024);
    glds16_raw(xp + (int64_t)yr * a.ldx + k0 + c * 8, sx + T128_OPER + piece * 1024);
  }
  if (kk == 0 && wave == 0) {  // the tile's rn values ride on the same wait: lanes 0..31 the tile's, 32..63 the panel's
    const float* src = a.rn + p * a.t_pad + (lane < 32 ? jt * AF_T + lane * 4 : panel * AF_T + (lane - 32) * 4);
    glds16_raw(src, smem + AF_RN + (jt & 1) * 1024);
  }
}

__global__ __launch_bounds__(256, 2) void affinity_bits_kernel(AffArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  // (problem, run, panel), panel fastest, in XCD-contiguous order: the panels that read the same column tiles run next to
  // each other on one XCD and meet in its L2
  const int vid = xcd_remap(blockIdx.x, gridDim.x);
  const int ps = vid / a.npanels, panel = vid - ps * a.npanels;
  const int p = ps / a.nsplit, split = ps - p * a.nsplit;
  int jt0, jt1;
  run_tiles(split, a.split_base, a.split_rem, jt0, jt1);
  const bf16_t* xp = a.x + (int64_t)p * a.xs;

  f32x16 acc[2][2];
  acc_zero(acc);
  const float* s_rn = reinterpret_cast<const float*>(smem + AF_RN);
  // the row this lane stores in the epilogue: word (m, e, hh) lives in lane 32 hh + 16 m + e
  const int srow = panel * AF_T + acc_row(wr, (lane >> 4) & 1, lane & 15, hh);
  uint32_t* const dst = a.bits + ((int64_t)p * a.t + min(srow, a.t - 1)) * a.pitch + wc * 2;

  // dma_steps of desc_tile.h, spelled out
  const int nk = (a.d + 63) >> 6;
  const int nsteps = (jt1 - jt0) * nk;
  int jt = jt0, kk = -1, buf = 1;
#pragma clang loop unroll(disable)
  for (int s = -1; s < nsteps; ++s) {
    int njt = jt, nkk = kk + 1;
    if (nkk == nk) {
      nkk = 0;
      ++njt;
    }
    if (s + 1 < nsteps) aff_stage(a, xp, p, panel, njt, nkk, smem, buf ^ 1, wave, lane);
    if (s >= 0) {
      const char* sx = smem + buf * 2 * T128_OPER;
      t128_mfma<0, 2>(sx, wr, wc, l31, hh, acc);
      if (a.d - kk * 64 >= 64) t128_mfma<2, 4>(sx, wr, wc, l31, hh, acc);
      if (kk + 1 == nk) {
        // ---- epilogue of tile jt (every lane takes part in every ballot: no divergence in here)
        const float* rn = s_rn + (jt & 1) * 256;
        float rny[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) rny[n] = rn[acc_col(wc, n, l31)];
        // the lane that keeps a ballot, made opaque here: compared as plain `l31 == constant` the 32 lane masks are loop
        // invariants that hipcc keeps in SGPR pairs and spills (mask_keys in vdr_dev.h tells the same story)
        int lsel = l31;
        asm volatile("" : "+v"(lsel));
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float rnx = rn[128 + acc_row(wr, m, e, hh)];
#pragma unroll
            for (int n = 0; n < 2; ++n) {
              const float v = acc[m][n][e] * (rnx * rny[n]);
              acc[m][n][e] = 0.0f;
              const unsigned long long bal = __ballot(v > a.tau);
              w[n] = lsel == m * 16 + e ? (hh ? (uint32_t)(bal >> 32) : (uint32_t)bal) : w[n];
              // the word is pinned here: left alone, hipcc issues all 64 comparisons first, keeps their SGPR pairs and spills them
              asm volatile("" : "+v"(w[n]));
            }
          }
        // the ragged columns (their rn is whatever `work` held) and the diagonal are cleared on the finished words
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int wi = jt * 4 + wc * 2 + n;
          const int valid = a.t - wi * 32;
          w[n] &= valid >= 32 ? ~0u : valid <= 0 ? 0u : (1u << valid) - 1u;
          if (a.exclude_diag && (srow >> 5) == wi) w[n] &= ~(1u << (srow & 31));
        }
        if (srow < a.t) {
          u32x2 o;
          o[0] = w[0];
          o[1] = w[1];
          *reinterpret_cast<u32x2*>(dst + jt * 4) = o;
        }
      }
    }
    dma_wait();
    buf ^= 1;
    jt = njt;
    kk = nkk;
  }
}

constexpr int MV_ROWS = 4;                     // rows per wave of bits_matvec_kernel
constexpr int MV_WORDS = 64;                   // words (of 32 columns) staged per step: one per lane
template <int NV>
constexpr int mv_lds_bytes() { return MV_WORDS * (32 * NV + 1) * 4; }

// Y[p, i, c] = sum over j with B[i, j] of V[p, j, c].  A workgroup owns 16 rows of ONE problem (4 per wave) and walks the columns
// in steps of 64 words; per step the 2048 x NV values of V are staged into LDS once (coalesced; word q at float offset
// q (32 NV + 1): the odd stride spreads the lanes over the banks).  Lane l takes word step * 64 + l -- so its words are l, l + 64, ..
// in ascending order -- and adds, bit by bit in ascending order, V[j] where the bit is set and 0.0f where it is not, to each of
// its 4 rows.  acc + 0.0f == acc for every acc the sum can hold (it starts at +0.0f, so it is never -0.0f): the bits are those of
// a loop that skips the clear bits, which is how include/vdr.h states the order.  A select, not a multiplication by the bit: a
// non-finite V[j] behind a clear bit stays out.  (A wave per row that walks its set bits and loads V[j] from global memory pays NV
// scalar loads at a lane stride of 128 NV bytes per set bit: bound by L1 / L2 traffic.)
template <int NV>
__global__ __launch_bounds__(256) void bits_matvec_kernel(const uint32_t* __restrict__ bits, int pitch, int t, int groups,
                                                               const float* __restrict__ v, float* __restrict__ y,
                                                               int32_t* __restrict__ degree) {
  extern __shared__ float s_v[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int p = blockIdx.x / groups, g = blockIdx.x - p * groups;
  const int row0 = g * (4 * MV_ROWS) + wave * MV_ROWS;
  const float* vp = v + (int64_t)p * t * NV;
  const uint32_t* bp = bits + (int64_t)p * t * pitch;
  const int nw = (t + 31) >> 5;
  float acc[MV_ROWS][NV];
  int deg[MV_ROWS];
#pragma unroll
  for (int r = 0; r < MV_ROWS; ++r) {
    deg[r] = 0;
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[r][c] = 0.0f;
  }
  for (int w0 = 0; w0 < nw; w0 += MV_WORDS) {
    __syncthreads();  // every wave has read the previous step
    const int ncols = min(t - w0 * 32, MV_WORDS * 32);
    for (int e = tid; e < ncols * NV; e += 256) s_v[e + ((e / NV) >> 5)] = vp[(int64_t)w0 * 32 * NV + e];
    __syncthreads();
    const int wi = w0 + lane;
    if (wi < nw) {
      uint32_t w[MV_ROWS];
#pragma unroll
      for (int r = 0; r < MV_ROWS; ++r) {
        w[r] = row0 + r < t ? bp[(int64_t)(row0 + r) * pitch + wi] : 0u;
        if (wi == nw - 1 && (t & 31)) w[r] &= (1u << (t & 31)) - 1u;  // (columns >= t: their LDS slots hold whatever was there)
        deg[r] += __popc(w[r]);
      }
      const float* sv = s_v + lane * (32 * NV + 1);
#pragma unroll 4
      for (int b = 0; b < 32; ++b) {
        float vv[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) vv[c] = sv[b * NV + c];
#pragma unroll
        for (int r = 0; r < MV_ROWS; ++r) {
          const bool on = (w[r] >> b) & 1u;
#pragma unroll
          for (int c = 0; c < NV; ++c) acc[r][c] += on ? vv[c] : 0.0f;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < MV_ROWS; ++r) {
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[r][c] = wave_sum(acc[r][c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) deg[r] += __shfl_xor(deg[r], o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < MV_ROWS; ++r)
      if (row0 + r < t) {
        const int64_t row = (int64_t)p * t + row0 + r;
#pragma unroll
        for (int c = 0; c < NV; ++c) y[row * NV + c] = acc[r][c];
        if (degree) degree[row] = deg[r];
      }
  }
}

template <int NV>
hipError_t bits_matvec_nv(const uint32_t* bits, int pitch, int t, int pairs, const float* v, float* y, int32_t* degree, hipStream_t st) {
  static KernelState ks;
  const int dev = current_device_index();
  if (dev < 0) return hipErrorInvalidDevice;
  if (hipError_t e = raise_lds_limit(ks, (const void*)bits_matvec_kernel<NV>, dev, mv_lds_bytes<NV>())) return e;
  const int groups = (t + 4 * MV_ROWS - 1) / (4 * MV_ROWS);
  hipLaunchKernelGGL(bits_matvec_kernel<NV>, dim3((unsigned)((int64_t)pairs * groups)), dim3(256), mv_lds_bytes<NV>(), st, bits, pitch,
                     t, groups, v, y, degree);
  return hipGetLastError();
}

}  // namespace

int affinity_pitch(int t) { return t <= 0 ? 0 : (t + AF_T - 1) / AF_T * 4; }

size_t affinity_work_bytes(int pairs, int t) {
  if (pairs <= 0 || t <= 0) return 0;
  return (size_t)pairs * ((t + AF_T - 1) / AF_T * AF_T) * 4;
}

hipError_t launch_affinity_bits(const void* x, int64_t ldx, int64_t x_stride, int t, int pairs, int d, float tau, int exclude_diag,
                                void* work, uint32_t* bits, int pitch, hipStream_t st) {
  if (!cos_operand_ok(x, ldx, x_stride, t, d) || !work || !bits || (((uintptr_t)work | (uintptr_t)bits) & 15) || pairs <= 0 ||
      pitch != affinity_pitch(t))
    return hipErrorInvalidValue;
  if ((int64_t)pairs * t > INT32_MAX) return hipErrorInvalidValue;
  AffArgs a;
  a.x = (const bf16_t*)x;
  a.ldx = ldx, a.xs = x_stride;
  a.t = t, a.d = d;
  a.npanels = (t + AF_T - 1) / AF_T;
  a.t_pad = a.npanels * AF_T;
  a.pitch = pitch;
  a.exclude_diag = exclude_diag != 0;
  a.tau = tau;
  const int64_t items = (int64_t)pairs * a.npanels;
  const RunSplit run = run_split(items, a.npanels);
  a.nsplit = run.nsplit, a.split_base = run.base, a.split_rem = run.rem;
  a.rn = (float*)work;
  a.bits = bits;
  if (items * a.nsplit > INT32_MAX) return hipErrorInvalidValue;

  static KernelState ks;
  const int dev = current_device_index();
  if (dev < 0) return hipErrorInvalidDevice;
  if (hipError_t e = raise_lds_limit(ks, (const void*)affinity_bits_kernel, dev, AF_LDS)) return e;
  hipLaunchKernelGGL(aff_rnorm_kernel, dim3((unsigned)(((int64_t)pairs * t + 3) / 4)), dim3(256), 0, st, a, pairs);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(affinity_bits_kernel, dim3((unsigned)(items * a.nsplit)), dim3(256), AF_LDS, st, a);
  return hipGetLastError();
}

hipError_t launch_bits_matvec(const uint32_t* bits, int pitch, int t, int pairs, const float* v, int nv, float* y, int32_t* degree,
                              hipStream_t st) {
  if (!bits || !v || !y || pairs <= 0 || t <= 0 || nv < 1 || nv > 8 || pitch != affinity_pitch(t)) return hipErrorInvalidValue;
  if ((int64_t)pairs * t > INT32_MAX) return hipErrorInvalidValue;
  switch (nv) {
    case 1: return bits_matvec_nv<1>(bits, pitch, t, pairs, v, y, degree, st);
    case 2: return bits_matvec_nv<2>(bits, pitch, t, pairs, v, y, degree, st);
    case 3: return bits_matvec_nv<3>(bits, pitch, t, pairs, v, y, degree, st);
    case 4: return bits_matvec_nv<4>(bits, pitch, t, pairs, v, y, degree, st);
    case 5: return bits_matvec_nv<5>(bits, pitch, t, pairs, v, y, degree, st);
    case 6: return bits_matvec_nv<6>(bits, pitch, t, pairs, v, y, degree, st);
    case 7: return bits_matvec_nv<7>(bits, pitch, t, pairs, v, y, degree, st);
    default: return bits_matvec_nv<8>(bits, pitch, t, pairs, v, y, degree, st);
  }
}

}  // namespace vdr
