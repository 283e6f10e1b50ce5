// bf16 MFMA GEMM with fused epilogues for gfx950:  C[M,N] = epi(A[M,K] . W[N,K]^T)   -- entry point, the ring3 tile
// variants and the weight packer.  Kernels live in gemm_kernels.h; the ring4 variants are instantiated in gemm_ring4.hip
// (so that the two halves compile in parallel); the argument checks and the launch shape are gemm_launch.hip's.
//
// Replaces the nn.Linear calls under nn.MultiheadAttention / nn.TransformerEncoderLayer
// (reference src/models_archs.py:130-135) and attn.qkv / attn.proj / mlp.fc1 / mlp.fc2 of the
// frozen ViTs called at src/tfds_dense_descriptor.py:123, plus the patchify conv as a GEMM
// (src/tfds_dense_descriptor.py:128).
#include "gemm_kernels.h"

namespace vdr {

hipError_t launch_gemm_ring4(const GemmLaunch& L, hipStream_t s);                           // gemm_ring4.hip
hipError_t launch_gemm_8p(const GemmArgs& a, int epilogue, hipStream_t s);                   // gemm_8p.hip

// [N][K] (row stride ld) -> pair-interleaved [N/2][K/32][2][32]; one 16-byte chunk per thread
__global__ __launch_bounds__(256) void w_interleave_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int N, int K,
                                                           int64_t ld) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // destination chunk
  const int64_t total = (int64_t)N * (K >> 3);
  if (i >= total) return;
  const int c = (int)(i & 3), r1 = (int)((i >> 2) & 1);
  const int64_t t = i >> 3;
  const int kb = (int)(t % (K >> 5));
  const int64_t pair = t / (K >> 5);
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + (2 * pair + r1) * ld + kb * 32 + c * 8);
  *reinterpret_cast<bf16x8*>(dst + i * 8) = v;
}

hipError_t launch_w_interleave(const void* src, void* dst, int N, int K, int64_t ld, hipStream_t s) {
  if (N <= 0 || (N & 1) || K <= 0 || (K & 31)) return hipErrorInvalidValue;
  const int64_t total = (int64_t)N * (K >> 3);
  hipLaunchKernelGGL(w_interleave_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const bf16_t*)src, (bf16_t*)dst, N, K, ld);
  return hipGetLastError();
}

hipError_t launch_gemm(const GemmArgs& a, int epilogue, int variant, hipStream_t s) {
  GemmLaunch L;
  if (hipError_t e = build_gemm_launch(a, epilogue, variant, &L)) return e;  // every refusal but variant 31's own
  if (L.row->family == TILE_8P) return launch_gemm_8p(a, epilogue, s);
  return L.row->family == TILE_RING4 ? launch_gemm_ring4(L, s) : launch_tiles<22, 23, 24, 25>(L, s);
}

}  // namespace vdr
