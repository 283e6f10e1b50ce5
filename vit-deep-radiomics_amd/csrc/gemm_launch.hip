// GemmArgs -> launch: every argument check of launch_gemm / launch_gemm_mx and the launch shape (tile counts, tile order, store policy,
// LDS bytes, persistent form) as plain host code that needs no device (tests/test_gemm_launch_cpu.py), and the launch of a selected kernel.
#include <algorithm>
#include <cstdlib>

#include "gemm_launch.h"

namespace vdr {

// integer tuning knob from the environment: read in tuning builds (-DVDR_TUNING, `make tuning`) only; the shipped
// library has no environment dependence
static inline int tuning_env(const char* name, int dflt) {
  const char* e = VDR_TUNING_BUILD ? getenv(name) : nullptr;
  return e && *e ? atoi(e) : dflt;
}

// What the bf16 and the MX launches share: the operand / output fields, the tile counts and the tile order.
// elem: bytes per operand element (an e4m3 panel is BN x K bytes); gn_forced >= 0: tuning override; false: no tiles, or more than a grid holds
static bool fill_common(const GemmArgs& a, const TileVariant& row, size_t elem, int gn_forced, GemmK& k) {
  k.A = (const bf16_t*)a.A;
  k.W = (const bf16_t*)a.W;
  k.w_il = a.w_interleaved;
  k.bias = a.bias;
  k.resid = (const bf16_t*)a.resid;
  k.gamma = a.gamma;
  k.pos = a.pos;
  k.C = (bf16_t*)a.C;
  k.M = a.M;
  k.N = a.N;
  k.K = a.K;
  k.lda = a.lda;
  k.ldw = a.ldw;
  k.ldc = a.ldc;
  k.ldr = a.ldr;
  k.rpg = a.omap.rpg;
  k.gstride = a.omap.gstride;
  k.off = a.omap.off;
  const int BM = row.bm(), BN = row.bn();
  const int64_t tiles_m = (a.M + BM - 1) / BM;
  k.tiles_n = (a.N + BN - 1) / BN;
  k.tiles_m = (int)tiles_m;
  // column-group width: tiles are walked in groups of gn tile columns (tile_of) so that a group's W panels (BN x K
  // bf16 each) stay in the XCD's 4 MB L2 next to the A row panels in flight.  Measured:
  //   per launch, M = 50432, interleaved rounds (tools/kbench.py --variants (gn+1)*1000+26): qkv (9 columns, panel
  //   393 KB) 0.192 ms row-major, 0.174 / 0.171 / 0.175 / 0.176 for gn = 2 / 3 / 4 / 5; fc1 (12 columns) 0.276
  //   row-major, 0.266 / 0.265 / 0.266 for gn = 2 / 4 / 5, 0.275 for 6;
  //   whole forward, same device (tools/ab_forward.py): ViT-B (K = 768) 10.54 ms row-major, 10.37 / 10.40 / 10.40 for
  //   gn = 3 / 4 / 5; ViT-L/14 (K = 1024) 26.91 row-major, 26.47 / 26.64 for gn = 2 / 3; ViT-g/14 (K = 1536, 32 tile
  //   columns in w12) 22.79 row-major, 20.09 / 20.07 for gn = 2 / 3 (-12 %).
  // Rule: about 1.7 MB of W per group, i.e. gn = 4 / 3 / 2 for K = 768 / 1024 / 1536.  (Round 1 grouped only when W
  // as a whole exceeded the L2; with the whole-line operand loads the L2 misses weigh more and qkv gains too.)
  // K >= 3072 panels (>= 1.6 MB) give gn = 1: row-major, which is all a 3-column fc2 can use anyway.
  const size_t panel = (size_t)BN * a.K * elem;
  int gn = (int)((1700u << 10) / panel);
  if (gn < 2 || gn >= k.tiles_n) gn = 0;  // a single column at a time re-reads A once per column: never better than row-major
  k.gn = gn_forced >= 0 ? gn_forced : gn;
  const int64_t nwg = tiles_m * k.tiles_n;
  k.nwg = (int)nwg;
  k.ln_part = a.ln_part;
  k.part_stride = a.part_stride;
  return nwg > 0 && nwg <= 0x7fffffff;
}

hipError_t build_gemm_launch(const GemmArgs& a, int epi, int variant, GemmLaunch* L) {
  if (a.K <= 0 || (a.K & 63) || (a.N & 7) || a.M <= 0) return hipErrorInvalidValue;
  if (epi == EPI_SWIGLU && (a.N & 63)) return hipErrorInvalidValue;
  // tuning builds: tools/ encode the ablation bits and a forced gn into the variant number
  const int abl = VDR_TUNING_BUILD ? variant % 1000 / 100 : 0, gn_forced = VDR_TUNING_BUILD && variant >= 1000 ? variant / 1000 - 1 : -1;
  if (VDR_TUNING_BUILD) variant %= 100;
  if (a.out_f32 && epi != EPI_BIAS && epi != EPI_PATCH) return hipErrorInvalidValue;
  if (a.ln_part && (a.N & 63)) return hipErrorInvalidValue;
  *L = GemmLaunch();
  if (!(L->row = tile_variant(variant))) return hipErrorInvalidValue;
  const TileVariant& row = *L->row;
  if (row.family == TILE_8P) return hipSuccess;  // (gemm_8p_eligible)
  GemmK& k = L->k;
  k.resid32 = a.resid32;
  k.C32 = a.C32;
  if (a.resid32 || a.C32) {  // the fp32 residual stream: its own instantiation of the residual kernels
    if (epi != EPI_BIAS_RESID || !a.resid32 || !a.C32 || a.win_ws || !row.can(CAP_RESID32)) return hipErrorInvalidValue;
    epi = EPI_BIAS_RESID32;
  }
  VDR_KNOB int gn_env = tuning_env("VDR_GEMM_GN", -1), nt_env = tuning_env("VDR_GEMM_NT", -1);
  if (!fill_common(a, row, 2, gn_forced >= 0 ? gn_forced : gn_env, k)) return hipErrorInvalidValue;
  const size_t BM = row.bm(), BN = row.bn();
  k.win_ws = a.win_ws;
  k.win_g = a.win_g;
  k.a_rpg = a.a_rpg;
  k.a_gs = a.a_gs;
  k.a_is = a.a_is;
  k.out_f32 = a.out_f32;
  if (a.patch_p) {
    const int P = a.patch_p;
    if (epi != EPI_PATCH || !row.can(CAP_PATCH) || (P != 8 && P != 16 && P != 32) || a.patch_g <= 0 || a.patch_C <= 0 || a.K != a.patch_C * P * P ||
        a.M % ((int64_t)a.patch_g * a.patch_g) || a.a_rpg || ((uintptr_t)a.A & 15))
      return hipErrorInvalidValue;
    k.pg_ps = P == 8 ? 3 : P == 16 ? 4 : 5;
    k.pg_g = a.patch_g;
    k.pg_C = a.patch_C;
  }
  k.nt_store = nt_env >= 0 ? nt_env : output_exceeds_cache(a.M, a.ldc) && !a.resid;
  k.ln_stats = a.ln_stats;
  k.colsum = a.colsum;
  k.ln_fold = a.ln_stats || a.ln_cpart;
  if (a.fin_stats) {  // producer-side finalisation: ring4 kernels, residual epilogue, rows stored where they are computed
    if (!row.can(CAP_FIN_STATS) || epi_base(epi) != EPI_BIAS_RESID || !a.ln_part || !a.fin_cnt || a.win_ws || (a.N & 63)) return hipErrorInvalidValue;
    k.fin_stats = a.fin_stats;
    k.fin_cnt = a.fin_cnt;
    k.fin_groups = a.N / 64;
    k.fin_eps = a.fin_eps;
  }
  if (a.ldc >= ((int64_t)1 << 24)) return hipErrorInvalidValue;  // (epilogue_bf16 addresses a wave tile with 32-bit byte offsets)
  // (the residual epilogue, epilogue_resid: bf16 in place or out of place, no consumer-side fold, 32-bit row numbers)
  if (epi_base(epi) == EPI_BIAS_RESID && (k.ln_fold || a.out_f32 || a.M >= ((int64_t)1 << 31))) return hipErrorInvalidValue;
  if (a.ln_cpart) {
    if (!row.can(CAP_LN_CPART) || a.ln_groups < 1 || a.ln_groups > 16 || a.ln_stats) return hipErrorInvalidValue;
    k.ln_cpart = a.ln_cpart;
    k.ln_groups = a.ln_groups;
    k.ln_cstride = a.ln_cstride;
    k.ln_eps = a.ln_eps;
  }
  k.abl = abl;
#ifdef VDR_GEMM_STAMPS
  k.stamps = g_gemm_stamps;
#endif
  if (a.a_rpg && !row.can(CAP_A_RPG)) return hipErrorInvalidValue;  // the two-stride A gather stays on ring3

  L->epi = epi;
  L->tag1 = row.family == TILE_RING4 && epi_base(epi) == EPI_BIAS_RESID && a.K > a.N;
  // the persistent form is used for the residual epilogue only (see gemm_ring4p_kernel for what it gains and loses)
  L->persistent = row.can(CAP_PERSISTENT) && epi_base(epi) == EPI_BIAS_RESID;
  if (VDR_TUNING_BUILD && row.can(CAP_PERSISTENT)) {
    VDR_KNOB int pers_env = tuning_env("VDR_GEMM_PERSISTENT", -1);
    if (pers_env >= 0) L->persistent = L->persistent && pers_env;
    if (pers_env == 2 || (abl & 2)) L->persistent = true;  // every epilogue (experiments)
  }
  const size_t staging = (size_t)row.waves_m * row.waves_n * 32 * 272;  // epilogue images (ring3 / ring4: one per wave)
  const size_t stats = a.ln_cpart ? BM * 8 : 0;  // (mean, rstd) of the tile's BM rows
  if (row.family == TILE_RING4) L->lds = std::max(2 * BM * 128 + row.depth * BN * 64, staging + stats);
  else if (row.family == TILE_RING3K) L->lds = std::max((BM + BN) * 64 * 2 * row.depth, (size_t)65536 + 4 * 32 * 272);  // K reduction + staging
  else L->lds = std::max((BM + BN) * 64 * row.depth, staging);
  if (row.family == TILE_RING3 && stats) {  // behind the ring / staging area
    k.stats_off = (int)L->lds;
    L->lds += stats;
  }
  // tools/: extra dynamic LDS per workgroup (e.g. 40000 on ring4: one workgroup per CU instead of two)
  if (const int pad = tuning_env("VDR_GEMM_LDS_PAD", 0); pad > 0) L->lds += (size_t)pad;
  return hipSuccess;
}

hipError_t build_mx_launch(const GemmArgs& a, int epi, int variant, GemmLaunch* L) {
  if (a.K <= 0 || (a.K & 63) || (a.N & 63) || a.M <= 0 || !a.a_scale || !a.w_scale) return hipErrorInvalidValue;
  if (a.ln_stats || a.win_ws || a.a_rpg || a.out_f32 || a.M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
  if (a.c_scale) {  // MX output
    if (epi == EPI_BIAS_GELU) epi = EPI_BIAS_GELU_MX;
    else if (epi == EPI_SWIGLU) epi = EPI_SWIGLU_MX;
    else return hipErrorInvalidValue;
  }
  *L = GemmLaunch();
  if (!(L->row = tile_variant(variant, true))) return hipErrorInvalidValue;
  const TileVariant& row = *L->row;
  GemmK& k = L->k;
  // tile order: about 1.7 MB of W payload per column group (fill_common; an e4m3 panel is BN x K bytes)
  if (!fill_common(a, row, 1, tuning_env("VDR_MX_GN", -1), k)) return hipErrorInvalidValue;
  k.sA = (const uint8_t*)a.a_scale;
  k.sW = (const uint8_t*)a.w_scale;
  k.sa_rows = mx_rows_pad(a.M);
  k.sw_rows = mx_rows_pad(a.N);
  k.sC = (uint8_t*)a.c_scale;
  k.sc_rows = mx_rows_pad(a.M);
  const size_t NW = (size_t)row.waves_m * row.waves_n;
  L->epi = epi;
  L->lds = std::max(row.depth * ((size_t)(row.bm() + row.bn()) * 64 + NW * 256), NW * 32 * 272);  // ring, epilogue staging
  return hipSuccess;
}

// L on the kernels selected for it: one workgroup per tile of `plain`, or, where L wants the persistent form and has more
// tiles than the chip holds workgroups of it at once, that many workgroups of `persistent`
hipError_t launch_built(const GemmLaunch& L, GemmKernel plain, GemmKernel persistent, hipStream_t s) {
  const int dev = current_device_index();
  if (dev < 0) return hipErrorInvalidDevice;
  if (!plain.fn) return hipErrorInvalidValue;  // no instantiation for this epilogue
  const int block = L.row->block();
  GemmKernel kn = plain;
  int grid = L.k.nwg;
  if (L.persistent && persistent.fn) {
    const int slots = persistent_slots(*persistent.st, (const void*)persistent.fn, dev, block, L.lds);
    if (slots <= 0) return hipErrorUnknown;
    if (grid > slots) kn = persistent, grid = slots;
  }
  if (hipError_t e = raise_lds_limit(*kn.st, (const void*)kn.fn, dev, L.lds)) return e;
  hipLaunchKernelGGL(kn.fn, dim3((unsigned)grid), dim3((unsigned)block), L.lds, s, L.k);
  return hipGetLastError();
}

}  // namespace vdr
