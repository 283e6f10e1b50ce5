// The 8-phase GEMM kernel of tile variant 31 (description: gemm_8p.hip).  A header so that its instantiations can live in
// two translation units: gemm_8p.hip (EPI_BIAS, EPI_BIAS_GELU; the launcher and the shape rules) and gemm_8p_act.hip
// (EPI_BIAS_QGELU, EPI_BIAS_TGELU).  Everything here has internal linkage.
// The epilogue (epi_tiles) is written for its issue slots -- both waves of a SIMD run it with the matrix pipe idle: per site
// 303 vector instructions and 18 s_nop with erf-GELU and the fold (before: 335 and 40), 88 and 9 bias-only with the fold
// (123 and 11); fc1 245 -> 239 us, qkv 158 -> 157 us per launch at ViT-B/16 batch 256 (profiles/gemm8p_epilogue_isa.txt,
// profiles/gemm8p_epilogue_ab.txt).
#pragma once
#include <utility>

#include "gemm_kernels.h"

namespace vdr {

// the kernel argument block (one type for both translation units)
struct G8 {
  const bf16_t* A;
  const bf16_t* W;
  const float* bias;    // [N] (never null: the launcher substitutes zeros)
  const float* colsum;  // FOLD: [N]
  const float* stats;   // FOLD: (mean, rstd) [M][2]
  bf16_t* C;
  int M, N, K;
  int lda, ldw, ldc;    // row strides in elements
  int tn, ntiles;
  int nt_store;
};

namespace {

template <int... I, class F>
VDR_DEV void sfor_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
VDR_DEV void sfor(F&& f) {
  sfor_impl(std::make_integer_sequence<int, N>{}, f);
}

// 1 KB per wave-instruction, global -> LDS; uniform 64-bit base + 32-bit lane offset; LDS address in M0.  (The base is
// produced by scalar arithmetic: tools/hazard_scan.py checks that no VALU writes it within 5 wait states of the asm.)
VDR_DEV void dma16(const void* base_uniform, uint32_t lane_off, uint32_t lds_addr) {
  asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(lane_off), "s"(base_uniform), "{m0}"(lds_addr) : "memory");
}


constexpr int BUFB = 65536;  // one K-tile buffer: A0 | A1 | W0 | W1, 16 KB each
constexpr int HALFB = 16384;
constexpr int LDS_CONST = 2 * BUFB;  // 2 x [bias 1 KB | colsum 1 KB | stats 2 KB]
constexpr int LDS_TOTAL = 2 * BUFB + 2 * 4096;

template <int EPI, bool FOLD>
__global__ __launch_bounds__(512) void gemm_8p_kernel(G8 p) {
  static_assert(EPI == EPI_BIAS || epi_is_act(EPI), "write-once outputs only");
  extern __shared__ __attribute__((aligned(1024))) char lds[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int r = lane & 15, q = lane >> 4;
  const uint32_t lda2 = (uint32_t)p.lda * 2, ldw2 = (uint32_t)p.ldw * 2;  // bytes per operand row

  // ---- staging: lane part of the source address; rows w*8 + (lane >> 3) (+ 64 j) of a half-tile, chunk lane & 7 ----
  const int row8 = wave * 8 + (lane >> 3);
  const uint32_t offA = (uint32_t)row8 * lda2 + (uint32_t)(((lane & 7) ^ ((row8 >> 1) & 7)) << 4);
  const uint32_t offB = (uint32_t)row8 * ldw2 + (uint32_t)(((lane & 7) ^ (((row8 >> 1) & 1) | (((row8 >> 3) & 3) << 1))) << 4);

  // ---- fragment read addresses (byte offsets inside a K-tile buffer) ----
  //  A: row 16 i + r of the wave's half, chunk (4 kk + q) ^ ((row >> 1) & 7)
  //  W: accumulator tile j of the wave's 64 columns reads row slots 32 (j >> 1) + 4 (j & 1) + 8 (r >> 2) + (r & 3):
  //     lane (r, q) then holds columns 32 (j >> 1) + 8 q + 4 (j & 1) + e of output row r; chunk ^ (row bits 1, 3, 4)
  uint32_t a_rd[2], b_rd[2];
  {
    const int sA = (r >> 1) & 7;
    const int sB = ((r >> 1) & 1) | ((r >> 2) << 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      a_rd[kk] = lds0 + wr * HALFB + r * 128 + (((4 * kk + q) ^ sA) << 4);
      b_rd[kk] = lds0 + 2 * HALFB + (wc >> 1) * HALFB + (wc & 1) * 8192 + (8 * (r >> 2) + (r & 3)) * 128 + (((4 * kk + q) ^ sB) << 4);
    }
  }
  auto lds_read = [&](uint32_t addr) -> bf16x8 {
    return *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>((uintptr_t)addr);
  };

  // ---- tile list: workgroups of one XCD (id % 8) take neighbouring tiles (they share A row panels in that L2) ----
  // Row-major on purpose.  PMC (profiles/r04_pmc_traffic.txt): fc1 reads 453 MB per launch against 82 MB of operands -- every
  // XCD streams all of W (4.7 MB) once per round of 32 tiles.  Walking column groups of 3 / 4 / 6 tile columns instead
  // (an XCD's 32 tiles = 8 tile rows x 4 columns: W traffic down 9 x) measured SLOWER in the forward: qkv 1.79 -> 1.88 / 1.83
  // / 1.82 ms per step, fc1 2.50 -> 2.51 / 2.55 / 2.50 -- the L2 misses are not what the loop waits for.
  const int nwg = gridDim.x;
  const int vid = (blockIdx.x & 7) * (nwg >> 3) + (blockIdx.x >> 3);
  auto tile_bases = [&](int L, const char*& a, const char*& w, int& m0, int& n0) {
    const int tmi = L / p.tn, tni = L - tmi * p.tn;
    m0 = tmi * 256;
    n0 = tni * 256;
    a = (const char*)p.A + (size_t)m0 * lda2;
    w = (const char*)p.W + (size_t)n0 * ldw2;
  };

  f32x4 acc[8][4];
  bf16x8 fa[2][4];  // [kk][m tile of the current M half]
  bf16x8 fb[2][2];  // [kk][n tile of the current N half] (the n0 fragments are read again in a K-tile's 4th phase)

  // stage one half-tile: kind 0 A0, 1 A1, 2 W0, 3 W1
  auto stage = [&](auto kind_, const char* a, const char* w, int kt, int buf) {
    constexpr int kind = decltype(kind_)::value;
    const uint32_t ld2 = kind < 2 ? lda2 : ldw2;
    const char* src = (kind < 2 ? a : w) + (size_t)((kind & 1) * 128) * ld2 + (size_t)kt * 128;
    const uint32_t dst = lds0 + buf * BUFB + kind * HALFB + wave * 1024;
    dma16(src, kind < 2 ? offA : offB, dst);
    dma16(src + (size_t)64 * ld2, kind < 2 ? offA : offB, dst + 8192);
  };
  auto read_a = [&](auto mh_, int buf) {
    constexpr int mh = decltype(mh_)::value;
    sfor<2>([&](auto kk) { sfor<4>([&](auto i) { fa[kk][i] = lds_read(a_rd[kk] + buf * BUFB + (4 * mh + i) * 2048); }); });
  };
  auto read_b = [&](auto nh_, int buf) {
    constexpr int nh = decltype(nh_)::value;
    sfor<2>([&](auto kk) { sfor<2>([&](auto j) { fb[kk][j] = lds_read(b_rd[kk] + buf * BUFB + nh * 4096 + j * 512); }); });
  };
  auto mfma_quadrant = [&](auto mh_, auto nh_, auto zero_) {
    constexpr int mh = decltype(mh_)::value, nh = decltype(nh_)::value;
    constexpr bool zero = decltype(zero_)::value;
    __builtin_amdgcn_s_setprio(1);
    sfor<2>([&](auto kk) {
      sfor<4>([&](auto i) {
        sfor<2>([&](auto j) {
          constexpr int ii = 4 * mh + i, jj = 2 * nh + j;
          if constexpr (zero && kk == 0)
            acc[ii][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kk][j], fa[kk][i], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          else
            acc[ii][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kk][j], fa[kk][i], acc[ii][jj], 0, 0, 0);
        });
      });
    });
    __builtin_amdgcn_s_setprio(0);
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using T = std::true_type;
  using F = std::false_type;

  // Epilogue of two m-tiles (i0, i0 + 1) of one M half, both n halves: one "site", expanded 10 times in the kernel.  The
  // arithmetic is epilogue_bf16's (gemm_epi.h), in the accumulator layout:  v = fma(rs, acc, fma(-rs mu, csum, bias)), the
  // activation, one bf16 rounding.  A lane holds 16 B of output row r in each 32-column block (p = 0, 1); lanes r and r ^ 8
  // exchange one block so that a store instruction covers 8 rows x 128 B instead of 16 rows x 64 B.
  // Both waves of a SIMD run their sites side by side with the matrix pipe idle, so every issue slot here is paid in full:
  // what the ISA of a site holds, and what was taken out of it (hazard no-ops behind transcendentals and between dependent
  // packed instructions, the 4-instruction exchange, per-m-tile reads of the constants, a quarter-rate multiply in the
  // addresses), is counted in profiles/gemm8p_epilogue_isa.txt; the times are in profiles/gemm8p_epilogue_ab.txt.
  // (the descriptor ends after the last valid row: the rows of a ragged last tile past M are dropped by the range check)
  const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc((void*)p.C, (short)0, p.M * p.ldc * 2, 0x00020000);
  const uint32_t ldc2 = (uint32_t)p.ldc * 2;  // bytes per output row (below 2^24: M ldc 2 fits the 32-bit range of the descriptor)
  auto epi_tiles = [&](auto mh_, auto i0_, int m0, int n0, int par) {
    constexpr int mh = decltype(mh_)::value, i0 = decltype(i0_)::value;
    // Addresses: everything that is the same in all 64 lanes (tile, wave, M half, m-tile, constant buffer) is scalar
    // arithmetic, added to the lane term by one instruction.  (The offset of a store stays a vector operand: the rows of a
    // ragged last tile are dropped by the descriptor's range check, which this code relies on for the vector offset only.)
    // The lane terms are rebuilt from an opaque copy of the lane id at every site, about 14 vector instructions: hoisted out
    // of the K loop by hipcc they are long-lived registers of a kernel at its 256-register cap -- spilt, and a scratch
    // reload inside the loop would count in vmcnt next to the LDS-DMA pieces.
    uint32_t lane_ = (uint32_t)lane;
    asm volatile("" : "+v"(lane_));
    const uint32_t q16 = lane_ & 0x30;  // 16 q: this lane's 16 bytes of a 64-byte output block, 8 q floats of the constants
    const uint32_t cb = lds0 + LDS_CONST + par * 4096;
    const uint32_t baddr = (cb + wc * 256) + q16 * 2;
    const uint32_t saddr = (cb + 2048 + (wr * 128 + 64 * mh + 16 * i0) * 8) + (lane_ & 15) * 8;
    typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
    typedef __attribute__((address_space(3))) f32x2 lds_f32x2;
    // store: row (r & 7) of an 8-row group, block 0 in lanes r < 8 and block 1 (+ 64 bytes) in lanes r >= 8
    const uint32_t voff = __umul24(lane_ & 7, ldc2) + (q16 + ((lane_ & 8) << 3));  // (v_mad_u32_u24: full rate)
    const uint32_t soff = (uint32_t)(m0 + wr * 128 + 64 * mh + 16 * i0) * ldc2 + (uint32_t)(n0 + wc * 64) * 2;
    // (mean, rstd) of this lane's row in both m-tiles
    f32x2 rs2[2] = {{1.0f, 1.0f}, {1.0f, 1.0f}}, nrm2[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
    if constexpr (FOLD) {
      sfor<2>([&](auto di) {
        const f32x2 st = *reinterpret_cast<const lds_f32x2*>((uintptr_t)(saddr + di * 128));
        const float nrm = -st[1] * st[0];
        rs2[di] = f32x2{st[1], st[1]};
        nrm2[di] = f32x2{nrm, nrm};
      });
    }
    // One 32-column block at a time, both m-tiles on it: its 4 constant vectors (16 live registers; both blocks' would be
    // 32 and spill) are read from LDS once per site and block, not once per m-tile.  Block 0 of the two m-tiles waits in
    // ob0 (8 registers) for block 1; an m-tile leaves as soon as its block 1 is rounded.
    bf16x8 ob0[2];
    sfor<2>([&](auto pb) {
      const f32x4 b0 = *reinterpret_cast<const lds_f32x4*>((uintptr_t)(baddr + pb * 128));
      const f32x4 b1 = *reinterpret_cast<const lds_f32x4*>((uintptr_t)(baddr + pb * 128 + 16));
      f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
      if constexpr (FOLD) {
        c0 = *reinterpret_cast<const lds_f32x4*>((uintptr_t)(baddr + 1024 + pb * 128));
        c1 = *reinterpret_cast<const lds_f32x4*>((uintptr_t)(baddr + 1024 + pb * 128 + 16));
      }
      sfor<2>([&](auto di) {
        constexpr int i = i0 + di, ii = 4 * mh + i;
        bf16x8 ob;
        // The block's 8 values per accumulator tile are 4 pairs of neighbouring registers: pair k is elements e, e + 1
        // (e = 2 (k >> 1)) of tile 2 pb + (k & 1).  fold: epilogue_bf16's formula, two fused multiply-adds (without the
        // fold rs = 1, nrm = 0, csum = 0: acc + bias exactly) as v_pk_fma_f32, bit for bit the scalar operations, two per
        // issue slot.  put: one bf16 rounding (v_cvt_pk_bf16_f32) into the pair's place of the 16 output bytes.
        auto fold = [&](auto k_) -> f32x2 {
          constexpr int k = decltype(k_)::value, t = 2 * pb + (k & 1), e = 2 * (k >> 1);
          const f32x4& bb = (k & 1) ? b1 : b0;
          const f32x4& cc = (k & 1) ? c1 : c0;
          return __builtin_elementwise_fma(rs2[di], f32x2{acc[ii][t][e], acc[ii][t][e + 1]},
                                           __builtin_elementwise_fma(nrm2[di], f32x2{cc[e], cc[e + 1]}, f32x2{bb[e], bb[e + 1]}));
        };
        auto put = [&](auto k_, f32x2 v) {
          constexpr int k = decltype(k_)::value, o = 4 * (k & 1) + 2 * (k >> 1);
          ob[o] = (bf16_t)v[0];
          ob[o + 1] = (bf16_t)v[1];
        };
        // The activations run on two pairs at a time, in the order written (a sched_barrier between the steps holds hipcc
        // to it).  Two hazards cost an s_nop each, issue cycles that compute nothing, when a result is read in the slot right
        // behind its instruction: that of a v_exp_f32 / v_rcp_f32, and that of a packed instruction (v_pk_fma_f32 ...).
        // So the packed chains of the two pairs are left to hipcc to interleave, the four transcendentals are issued
        // together and their two consumers follow in the same order: each reads a result that is at least two slots old.
        // Every value goes through the operations of epi_act2 (vdr_dev.h) in their order.
        auto B = [] { __builtin_amdgcn_sched_barrier(0); };
        [[maybe_unused]] f32x2 x[4], a[4], u[4], g[4];
        sfor<2>([&](auto h) {
          using K0 = std::integral_constant<int, 2 * h>;
          using K1 = std::integral_constant<int, 2 * h + 1>;
          if constexpr (EPI == EPI_BIAS_GELU) {
            // H: a = min(|x|, 5.7), u = max(x, 0);  P: g = Q(a);  E: g = 2^g;  M: g = u - a g;  then the rounding.  (H and P
            // apart: the clamps are asm statements, which hipcc does not count as the wait state between two dependent
            // packed instructions)
            auto H = [&](auto k) { gelu_erf2_clamp(fold(k), a[k], u[k]); };
            auto P = [&](auto k) { g[k] = gelu_erf2_poly(a[k]); };
            auto E = [&](auto k) { g[k] = fast_exp2_2(g[k]); };
            auto M = [&](auto k) { g[k] = gelu_erf2_tail(a[k], g[k], u[k]); };
            H(K0{}); H(K1{}); B();
            P(K0{}); P(K1{}); B();
            E(K0{}); B(); E(K1{}); B();
            M(K0{}); B(); M(K1{}); B();
            put(K0{}, g[K0::value]); B(); put(K1{}, g[K1::value]);
          } else if constexpr (epi_is_act(EPI)) {
            // H: the exponent g = -t log2 e;  E: g = 2^g;  D: g = g + 1;  R: g = 1 / g;  M: g = x g;  C: round
            auto H = [&](auto k) {
              x[k] = fold(k);
              if constexpr (EPI == EPI_BIAS_QGELU) g[k] = quick_gelu2_e2(x[k]);
              else g[k] = gelu_tanh2_e2(x[k]);
            };
            auto E = [&](auto k) { g[k] = fast_exp2_2(g[k]); };
            auto D = [&](auto k) { g[k] = g[k] + f32x2{1.0f, 1.0f}; };
            auto R = [&](auto k) { g[k] = fast_rcp_2(g[k]); };
            auto M = [&](auto k) { g[k] = x[k] * g[k]; };
            H(K0{}); H(K1{}); B();
            E(K0{}); B(); E(K1{}); B();
            D(K0{}); B(); D(K1{}); B();
            R(K0{}); B(); R(K1{}); B();
            M(K0{}); B(); M(K1{}); B();
            put(K0{}, g[K0::value]); B(); put(K1{}, g[K1::value]);
          } else {
            put(K0{}, fold(K0{}));
            put(K1{}, fold(K1{}));
          }
        });
        B();  // (also keeps hipcc from fetching the next block's constants ahead: VGPR cap)
        if constexpr (pb == 0) {
          ob0[di] = ob;
        } else {
          // Lanes r and r ^ 8 exchange one block: rows 0-7 of the m-tile take [own block 0 | row r - 8's block 1], rows 8-15
          // [row r + 8's block 0 | own block 1].  Two instructions per dword: a select whose second source comes through DPP
          // row_ror:8 (lane predicate r < 8 in VCC), and a DPP move that only writes the lanes r < 8 (bank mask 0x3: banks are
          // 4 lanes of a 16-lane row).  Written as asm: select + __builtin_amdgcn_update_dpp + two selects compile to select,
          // move, DPP move, select, select per dword.  hipcc pads no hazard inside an asm statement: a DPP source needs 2 wait states behind the vector
          // instruction that wrote it -- here a v_cvt_pk_bf16_f32 above, or a copy hipcc makes to place the operands -- so the
          // statement opens with s_nop 1; inside it no DPP source is written before it is read.
          const u32x4 w0 = __builtin_bit_cast(u32x4, ob0[di]), w1 = __builtin_bit_cast(u32x4, ob);
          uint32_t a0 = w0[0], a1 = w0[1], a2 = w0[2], a3 = w0[3], b0 = w1[0], b1 = w1[1], b2 = w1[2], b3 = w1[3];
          uint32_t d0, d1, d2, d3;
          asm volatile(
              "s_nop 1\n\t"
              "s_mov_b32 vcc_lo, 0x00ff00ff\n\t"  // lanes with (lane & 8) == 0
              "s_mov_b32 vcc_hi, 0x00ff00ff\n\t"
              "v_cndmask_b32_dpp %[d0], %[b0], %[a0], vcc row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
              "v_cndmask_b32_dpp %[d1], %[b1], %[a1], vcc row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
              "v_cndmask_b32_dpp %[d2], %[b2], %[a2], vcc row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
              "v_cndmask_b32_dpp %[d3], %[b3], %[a3], vcc row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
              "v_mov_b32_dpp %[b0], %[a0] row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
              "v_mov_b32_dpp %[b1], %[a1] row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
              "v_mov_b32_dpp %[b2], %[a2] row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
              "v_mov_b32_dpp %[b3], %[a3] row_ror:8 row_mask:0xf bank_mask:0x3"
              : [d0] "=&v"(d0), [d1] "=&v"(d1), [d2] "=&v"(d2), [d3] "=&v"(d3), [b0] "+v"(b0), [b1] "+v"(b1), [b2] "+v"(b2), [b3] "+v"(b3)
              : [a0] "v"(a0), [a1] "v"(a1), [a2] "v"(a2), [a3] "v"(a3)
              : "vcc");
          const u32x4 da = {d0, d1, d2, d3}, db = {b0, b1, b2, b3};
          const uint32_t s_a = soff + (16 * di) * ldc2, s_b = soff + (16 * di + 8) * ldc2;
          // (opaque: as a hoisted condition hipcc keeps it as a lane mask and rebuilds it with two vector instructions per site)
          int nt = p.nt_store;
          asm volatile("" : "+s"(nt));
          if (nt) {
            __builtin_amdgcn_raw_buffer_store_b128(da, crs, voff + s_a, 0, 2 /* nt */);
            __builtin_amdgcn_raw_buffer_store_b128(db, crs, voff + s_b, 0, 2);
          } else {
            __builtin_amdgcn_raw_buffer_store_b128(da, crs, voff + s_a, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(db, crs, voff + s_b, 0, 0);
          }
        }
      });
    });
  };
  auto seg_sync_a = [&]() {  // end of a load segment: own LDS reads retired, then the rendezvous
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  auto seg_sync_b = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };

  int L = vid;
  if (L >= p.ntiles) return;
  const char *ca, *cw, *na, *nw_;
  int m0, n0, nm0, nn0;
  tile_bases(L, ca, cw, m0, n0);
  const int nk = p.K >> 6;
  int par = 0;
  // constants of a tile: one 1-KB piece each by waves 0 .. 3 (bias, column sums, two halves of the row statistics)
  auto stage_consts = [&](int m0_, int n0_, int par_) {
    const uint32_t cb = lds0 + LDS_CONST + par_ * 4096;
    if (wave == 0) dma16((const char*)p.bias + (size_t)n0_ * 4, (uint32_t)lane * 16, cb);
    if constexpr (FOLD) {
      if (wave == 1) dma16((const char*)p.colsum + (size_t)n0_ * 4, (uint32_t)lane * 16, cb + 1024);
      if (wave == 2) dma16((const char*)p.stats + (size_t)m0_ * 8, (uint32_t)lane * 16, cb + 2048);
      if (wave == 3) dma16((const char*)p.stats + (size_t)(m0_ + 128) * 8, (uint32_t)lane * 16, cb + 3072);
    }
  };

  // ---- prologue: K-tile 0 complete, A0 of K-tile 1 in flight ----
  stage(I0{}, ca, cw, 0, 0);
  stage(I1{}, ca, cw, 0, 0);
  stage(I2{}, ca, cw, 0, 0);
  stage(I3{}, ca, cw, 0, 0);
  stage(I0{}, ca, cw, 1, 1);
  asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wr == 1) __builtin_amdgcn_s_barrier();  // the second M half runs one barrier behind
  __builtin_amdgcn_sched_barrier(0);

  bool have_prev = false;
  int pm0 = 0, pn0 = 0;

  // one K-tile pair (K-tiles t0 in buffer 0, t0 + 1 in buffer 1); FIRST: the tile's first pair (C = 0, the previous
  // tile's second M half leaves in phases 2 and 3); LAST: the tile's last pair (the first M half leaves in phases 7 and 8,
  // the DMA stream moves on to the next tile: K-tiles t0 + 2, t0 + 3 are its K-tiles 0, 1)
  auto pair = [&](auto first_, auto last_, int t0) {
    constexpr bool FIRST = decltype(first_)::value, LAST = decltype(last_)::value;
    const char* a2 = LAST ? na : ca;
    const char* w2 = LAST ? nw_ : cw;
    const int k2 = LAST ? 0 : t0 + 2, k3 = LAST ? 1 : t0 + 3;
    // Where a finished M half leaves.  Waves 0-3 ("X") do it at the head of a load segment, waves 4-7 ("Y", one barrier
    // behind) at the tail of the MFMA segment that faces it: the SAME slot of wall-clock time, so the two waves of a SIMD
    // run their epilogues side by side (a wave issues one vector instruction per ~5.4 cycles, a SIMD takes one per ~2.7:
    // profiles/r03_valu_rate_micro.txt) instead of one after the other with the partner's 16 MFMAs long finished --
    // measured with every wave in its load segments: the erf-GELU cost 35 us of an fc1 launch, tools/ab_epi.py.
    const bool X = wr == 0;
    // ---- K-tile t0, buffer 0 ----
    // phase 1: quadrant (m0, n0)
    read_b(I0{}, 0);
    read_a(I0{}, 0);
    if constexpr (FIRST) stage_consts(m0, n0, par);
    stage(I1{}, ca, cw, t0 + 1, 1);  // A1 and W0 of t0 + 1 (buffer 1's W halves were last read in the previous pair's phase 8)
    stage(I2{}, ca, cw, t0 + 1, 1);
    // (a tile's first pair stages W1 here too -- its half of buffer 1 was last read in the previous pair's phase 6 -- so that
    // the stores of the previous tile's second M half, phases 1 to 3, are all BEHIND this K-tile's last piece: the counted
    // wait of phase 4 never waits for the acknowledgement of a store)
    if constexpr (FIRST) stage(I3{}, ca, cw, t0 + 1, 1);
    seg_sync_a();
    mfma_quadrant(I0{}, I0{}, std::integral_constant<bool, FIRST>{});
    if constexpr (FIRST) {
      if (have_prev && !X) {
        __builtin_amdgcn_sched_barrier(0);
        epi_tiles(I1{}, I0{}, pm0, pn0, par ^ 1);
      }
    }
    seg_sync_b();
    // phase 2: (m0, n1)
    read_b(I1{}, 0);
    if constexpr (!FIRST) stage(I3{}, ca, cw, t0 + 1, 1);  // W1 of t0 + 1
    // the previous tile's second M half (final after its phase 8) leaves in phases 2 and 3
    if constexpr (FIRST) {
      if (have_prev && X) epi_tiles(I1{}, I0{}, pm0, pn0, par ^ 1);
    }
    seg_sync_a();
    mfma_quadrant(I0{}, I1{}, std::integral_constant<bool, FIRST>{});
    if constexpr (FIRST) {
      if (have_prev && !X) {
        __builtin_amdgcn_sched_barrier(0);
        epi_tiles(I1{}, I2{}, pm0, pn0, par ^ 1);
      }
    }
    seg_sync_b();
    // phase 3: (m1, n1)
    read_a(I1{}, 0);
    if constexpr (FIRST) {
      if (have_prev && X) epi_tiles(I1{}, I2{}, pm0, pn0, par ^ 1);
    }
    seg_sync_a();
    mfma_quadrant(I1{}, I1{}, std::integral_constant<bool, FIRST>{});
    seg_sync_b();
    // phase 4: (m1, n0)
    read_b(I0{}, 0);
    stage(I0{}, a2, w2, k2, 0);  // A0 of t0 + 2 (buffer 0's W halves are read until this phase: the n0 fragments again)
    // K-tile t0 + 1 has landed (this wave's pieces; the barrier does the rest); younger: A0 of t0 + 2 and the 8 stores
    if (FIRST && have_prev) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    seg_sync_a();
    mfma_quadrant(I1{}, I0{}, std::integral_constant<bool, FIRST>{});
    seg_sync_b();
    // ---- K-tile t0 + 1, buffer 1 ----
    // phase 5: (m0, n0)
    read_b(I0{}, 1);
    read_a(I0{}, 1);
    stage(I1{}, a2, w2, k2, 0);  // A1 and W0 of t0 + 2
    stage(I2{}, a2, w2, k2, 0);
    seg_sync_a();
    mfma_quadrant(I0{}, I0{}, F{});
    seg_sync_b();
    // phase 6: (m0, n1)
    read_b(I1{}, 1);
    stage(I3{}, a2, w2, k2, 0);  // W1 of t0 + 2
    seg_sync_a();
    mfma_quadrant(I0{}, I1{}, F{});
    if constexpr (LAST) {
      if (!X) {  // first M half (final with this segment), m-tiles 0, 1
        __builtin_amdgcn_sched_barrier(0);
        epi_tiles(I0{}, I0{}, m0, n0, par);
      }
    }
    seg_sync_b();
    // phase 7: (m1, n1)
    read_a(I1{}, 1);
    if constexpr (LAST) {
      if (X) epi_tiles(I0{}, I0{}, m0, n0, par);
    }
    seg_sync_a();
    mfma_quadrant(I1{}, I1{}, F{});
    if constexpr (LAST) {
      if (!X) {  // ... m-tiles 2, 3
        __builtin_amdgcn_sched_barrier(0);
        epi_tiles(I0{}, I2{}, m0, n0, par);
      }
    }
    seg_sync_b();
    // phase 8: (m1, n0)
    read_b(I0{}, 1);
    stage(I0{}, a2, w2, k3, 1);  // A0 of t0 + 3
    // K-tile t0 + 2 has landed: younger than its last piece are A0 of t0 + 3 (2) and, in a LAST pair, the stores issued since
    // phase 6's staging (X: the 4 of phase 7; Y: all 8)
    if constexpr (LAST) {
      if (X) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    }
    if constexpr (LAST) {
      if (X) epi_tiles(I0{}, I2{}, m0, n0, par);
    }
    seg_sync_a();
    mfma_quadrant(I1{}, I0{}, F{});
    seg_sync_b();
  };

  for (;;) {
    const int Ln = L + nwg;
    const bool more = Ln < p.ntiles;
    // (no next tile: the stream re-loads this tile's first K-tiles into buffers nobody reads again)
    tile_bases(more ? Ln : L, na, nw_, nm0, nn0);
    pair(T{}, F{}, 0);
    for (int t0 = 2; t0 < nk - 2; t0 += 2) pair(F{}, F{}, t0);
    pair(F{}, T{}, nk - 2);
    have_prev = true;
    pm0 = m0;
    pn0 = n0;
    par ^= 1;
    if (!more) break;
    L = Ln;
    ca = na;
    cw = nw_;
    m0 = nm0;
    n0 = nn0;
  }
  // the last tile's second M half; then the first M half waits for the second's extra barrier
  epi_tiles(I1{}, I0{}, pm0, pn0, par ^ 1);
  epi_tiles(I1{}, I2{}, pm0, pn0, par ^ 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (wr == 0) __builtin_amdgcn_s_barrier();
}

// one launch: the > 64 KB dynamic-LDS opt-in once per instantiation and device, then the persistent grid
template <int EPI, bool FOLD>
hipError_t launch_8p_instance(const G8& g, int grid, int dev, hipStream_t s) {
  auto fn = gemm_8p_kernel<EPI, FOLD>;
  static KernelState st;
  if (hipError_t e = raise_lds_limit(st, (const void*)fn, dev, LDS_TOTAL)) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(512), LDS_TOTAL, s, g);
  return hipGetLastError();
}

}  // namespace

}  // namespace vdr
