// Tile variant 31: the 256 x 256 x 64 "8-phase" GEMM for the write-once linears with many tiles (attn.qkv, mlp.fc1 of the
// frozen ViTs called at src/tfds_dense_descriptor.py:123; the nn.Linear calls of nn.MultiheadAttention /
// nn.TransformerEncoderLayer, reference src/models_archs.py:130-135):  C[M, N] = epi(A[M, K] . W[N, K]^T),
// bf16 in / fp32 accumulate / bf16 out, EPI_BIAS or an activation epilogue (erf-GELU, QuickGELU, tanh-GELU), optionally with the consumer-side LayerNorm fold.
//
// The structure is cdna_hip_programming.md 5, "The 256^2 8-phase template", built from its description and measured as a
// micro-benchmark first (tools/micro/gemm8p.hip, profiles/r04_gemm8p_micro.txt: bitwise equal to ring4; with its output
// leaving as non-temporal BUFFER stores behind a wave-uniform descriptor qkv 0.80 x and fc1 0.85 x of ring4's time at a
// bias-only epilogue, 1.25-1.37 PF at 4096^3):
//   * one 512-thread workgroup per CU, persistent over a static tile list; 8 waves = 2 (M) x 4 (N), a wave owns 128 x 64 of
//     the tile = 8 x 4 accumulator tiles of v_mfma_f32_16x16x32_bf16 (128 registers);
//   * LDS: 2 K-tile buffers x {A rows 0-127, A rows 128-255, W rows 0-127, W rows 128-255} x [128 rows][128 B] = 128 KB,
//     every half-tile filled by 2 LDS-DMA instructions per thread (8 rows x 128 B: whole lines per wave-instruction),
//     16-byte chunks XOR-swizzled on the source address and on the ds_read_b128 address (conflict-free fragment reads);
//     W in the plain PyTorch layout [N][K] (no packed copy);
//   * a K-tile is 4 phases of 16 MFMAs (a 64 x 32 quadrant of the wave tile x K = 64); a phase is
//         ds_read fragments | one or two half-tiles of LDS-DMA | [counted vmcnt] | lgkmcnt(0) | s_barrier |
//         s_setprio 1 | 16 MFMAs | s_setprio 0 | s_barrier
//     and waves 4-7 (the second M half: the second wave of every SIMD) run ONE barrier behind waves 0-3, so a wave's MFMA
//     segment always faces its SIMD partner's load segment (ping-pong);
//   * the DMA stream never drains and runs on ACROSS output tiles: A1 + W0 of K-tile t+1 are issued in t's 1st phase, W1
//     in its 2nd, A0 of t+2 in its 4th (a half-tile is re-staged one phase after the lgkmcnt + barrier that retired its
//     last read); the counted vmcnt(2) of the 4th phase leaves that last half-tile in flight;
//   * no epilogue phase: a 64-row half of the wave tile is final after the 2nd / 4th phase of the tile's last K-tile and
//     is finished (LayerNorm fold, bias, erf-GELU, bf16) and stored in the LOAD segments of the following phases, facing
//     the partner wave's MFMAs; the next tile's first MFMA into a quadrant starts from C = 0.  W rows are permuted inside a
//     32-column block so that a lane's registers of two neighbouring accumulator tiles are 8 consecutive columns, and lanes
//     r, r ^ 8 of a 16-lane row exchange one 16-byte block (DPP row_ror:8): a store instruction covers 8 rows x 128 B --
//     whole lines straight from the accumulator layout, no LDS staging;
//   * per-tile constants (bias, column sums of the folded weight, (mean, rstd) of the tile's 256 rows: 4 KB) arrive by
//     LDS-DMA too, double buffered by tile parity: no vector-memory load in the kernel is a plain load, so every counted
//     vmcnt written here is exact (LDS-DMA pieces and stores count together, in issue order).
// Same products in the same order and the same epilogue formula as ring3 / ring4: outputs are bitwise equal
// (tests/test_ops_gpu.py::test_linear_8phase_*).  Shapes: N % 256 == 0, K % 128 == 0, K >= 256; M % 256 == 0, or A / the row
// statistics readable up to M rounded up to 256 (GemmArgs::a_rows: the forward's workspace buffers are) -- the rows of the
// last tile past M are computed from whatever is there and never stored; enough tiles to fill the chip evenly
// (gemm_8p_eligible: ViT-g/14 at batch 32 has 594 tiles = 2.3 rounds of 256 workgroups and stays on ring4).
#include "gemm_8p_kernel.h"

namespace vdr {

// the QuickGELU / tanh-GELU instantiations (gemm_8p_act.hip)
hipError_t launch_gemm_8p_act(const G8& g, int epi, bool fold, int grid, int dev, hipStream_t s);

// whether tile variant 31 takes this launch (and is expected to pay: many tiles, a write-once bf16 output)
// the tile-count rule alone: one workgroup per CU walks tiles / CUs rounds -- at least two, and the last one reasonably full
// (a 2.3-round launch runs 3 rounds long: measured on ViT-g/14's qkv, 594 tiles: 114 us against ring4's 107; a launch of
// less than one round -- one MedSAM slice, M = 4096: 144 / 192 tiles -- pays the pipeline fill and the four epilogue slots once
// per 12 K-tiles: qkv 27.1 -> 28.9 us, fc1 31.4 -> 32.4 against the 128-row ring4 tiles)
// gemm_8p_rounds: the rounds such a launch runs, 0 where the rule refuses the shape, and (idle) the part of a round its
// last round leaves the chip empty, 0 .. 0.15 x rounds (the forward's split policy counts both)
int64_t gemm_8p_rounds(int64_t M, int N, double* idle) {
  if (idle) *idle = 0.0;
  if (M <= 0 || (N & 255)) return 0;
  int n_cu = device_cu_count(current_device_index());
  if (n_cu <= 0) n_cu = 256;
  const int64_t tiles = ((M + 255) / 256) * (int64_t)(N / 256), slots = n_cu & ~7;
  if (tiles < 2 * slots) return 0;
  const int64_t rounds = (tiles + slots - 1) / slots;
  if ((double)tiles < 0.85 * (double)(rounds * slots)) return 0;
  if (idle) *idle = (double)(rounds * slots - tiles) / (double)slots;
  return rounds;
}

bool gemm_8p_shape_ok(int64_t M, int N) { return gemm_8p_rounds(M, N, nullptr) > 0; }

bool gemm_8p_eligible(const GemmArgs& a, int epi) {
  if (epi != EPI_BIAS && !epi_is_act(epi)) return false;
  if (a.out_f32 || a.win_ws || a.a_rpg || a.patch_p || a.ln_part || a.ln_cpart || a.w_interleaved || a.resid32 || a.C32) return false;
  if (a.omap.rpg < (1 << 30) || a.a_scale || a.w_scale || a.c_scale) return false;
  if (a.M <= 0 || (a.N & 255) || (a.K & 127) || a.K < 256) return false;
  const int64_t Mr = (a.M + 255) & ~(int64_t)255;
  if (Mr != a.M && a.a_rows < Mr) return false;  // a ragged last tile reads 256 rows of A (and of the row statistics)
  if (a.lda < a.K || a.ldw < a.K || a.ldc < a.N) return false;
  if ((a.ln_stats != nullptr) != (a.colsum != nullptr)) return false;
  if ((double)Mr * a.ldc * 2.0 >= 2147483648.0 || (double)Mr * a.lda * 2.0 >= 4294967296.0 || (double)a.N * a.ldw * 2.0 >= 4294967296.0)
    return false;  // 32-bit store offsets / lane offsets
  if (((uintptr_t)a.A | (uintptr_t)a.W | (uintptr_t)a.C) & 15) return false;
  if ((a.lda | a.ldw | a.ldc) & 7) return false;
  return gemm_8p_shape_ok(a.M, a.N);
}

hipError_t launch_gemm_8p(const GemmArgs& a, int epi, hipStream_t s) {
  if (!gemm_8p_eligible(a, epi)) return hipErrorInvalidValue;
  const int dev = current_device_index();
  if (dev < 0) return hipErrorInvalidDevice;
  const float* bias = a.bias;
  if (!bias) {
    // a zero bias of at least N entries (bias == NULL), per device.  (load-time path in practice: every Linear of the models has a
    // bias; kept correct for vdr_op_linear callers.)  It grows by doubling under a lock, and an outgrown buffer stays allocated:
    // another thread may hold its pointer between this block and its launch (all of them together are smaller than the last)
    static std::mutex mu;
    static float* zeros[VDR_MAX_DEVICES] = {};
    static int zeros_n[VDR_MAX_DEVICES] = {};
    std::lock_guard<std::mutex> lock(mu);
    if (zeros_n[dev] < a.N) {
      int n = zeros_n[dev] ? zeros_n[dev] : 256;
      while (n < a.N) n *= 2;
      float* z = nullptr;
      hipError_t e = hipMalloc(&z, (size_t)n * 4);
      if (e == hipSuccess) e = hipMemset(z, 0, (size_t)n * 4);
      if (e != hipSuccess) return e;
      zeros[dev] = z;
      zeros_n[dev] = n;
    }
    bias = zeros[dev];
  }
  G8 g{(const bf16_t*)a.A, (const bf16_t*)a.W, bias, a.colsum, a.ln_stats, (bf16_t*)a.C, (int)a.M, a.N, a.K,
       (int)a.lda, (int)a.ldw, (int)a.ldc, a.N / 256, (int)(((a.M + 255) / 256) * (a.N / 256)), 0};
  g.nt_store = output_exceeds_cache(a.M, a.ldc) ? 1 : 0;
  int n_cu = device_cu_count(dev);
  if (n_cu <= 0) n_cu = 256;
  const int grid = n_cu & ~7;
  const bool fold = a.ln_stats != nullptr;
  switch (epi) {
    case EPI_BIAS:
      return fold ? launch_8p_instance<EPI_BIAS, true>(g, grid, dev, s) : launch_8p_instance<EPI_BIAS, false>(g, grid, dev, s);
    case EPI_BIAS_GELU:
      return fold ? launch_8p_instance<EPI_BIAS_GELU, true>(g, grid, dev, s) : launch_8p_instance<EPI_BIAS_GELU, false>(g, grid, dev, s);
    case EPI_BIAS_QGELU:
    case EPI_BIAS_TGELU:
      return launch_gemm_8p_act(g, epi, fold, grid, dev, s);  // (instantiated in gemm_8p_act.hip)
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace vdr
