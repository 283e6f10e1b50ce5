// Between a GemmArgs and a kernel on a stream (internal): what gemm_launch.hip derives from a GemmArgs, an epilogue and a
// row of TILE_VARIANTS, and the launch of a selected kernel.  Kernel selection lives beside the kernels (gemm_kernels.h, gemm_mx.hip).
#pragma once
#include "gemm_epi.h"

namespace vdr {

#ifdef VDR_GEMM_STAMPS
inline unsigned long long* g_gemm_stamps = nullptr;  // tools/micro/gemm_stamps.hip
#endif

struct GemmLaunch {
  const TileVariant* row = nullptr;
  GemmK k{};
  int epi = 0;              // the epilogue instantiation: EPI_BIAS_RESID32 for EPI_BIAS_RESID with resid32 / C32, the _MX forms with c_scale
  bool tag1 = false;        // the residual GEMM with K > N -- fc2 -- launches the TAG 1 symbol of the same code: profiles tell it from the out-projection
  bool persistent = false;  // the persistent form is wanted (taken when the launch has more tiles than the chip holds workgroups)
  size_t lds = 0;           // dynamic LDS bytes (0: variant 31, see below)
};

// Every argument check of launch_gemm / launch_gemm_mx and the whole launch shape; no device needed (tests/test_gemm_launch_cpu.py
// pins both).  hipErrorInvalidValue: refused.  A variant of the 8-phase family comes back with row set and nothing else:
// gemm_8p.hip has its own rules.  Tuning builds (-DVDR_TUNING): `variant` also carries what tools/ encode into it,
// variant / 100 = ablation bits (GemmK::abl; 2xx: the persistent form for every epilogue), (gn + 1) * 1000 + v = forced gn.
hipError_t build_gemm_launch(const GemmArgs& a, int epilogue, int variant, GemmLaunch* L);
hipError_t build_mx_launch(const GemmArgs& a, int epilogue, int variant, GemmLaunch* L);

// write-once output larger than half the Infinity Cache: stored non-temporal
static inline bool output_exceeds_cache(int64_t M, int64_t ldc) { return (double)M * (double)ldc * 2.0 >= 128e6; }

struct GemmKernel {  // a selected instantiation and its launch state; fn null: no such instantiation
  void (*fn)(GemmK) = nullptr;
  KernelState* st = nullptr;
};

// (gemm_launch.hip)
hipError_t launch_built(const GemmLaunch& L, GemmKernel plain, GemmKernel persistent, hipStream_t s);

}  // namespace vdr
