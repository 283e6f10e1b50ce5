// Tile variant 31 with the sigmoid-gated activations: the QuickGELU (CLIP) and tanh-GELU (SigLIP) instantiations of the
// 8-phase GEMM kernel (gemm_8p_kernel.h; structure, shape rules and launcher: gemm_8p.hip), with and without the
// consumer-side LayerNorm fold.  Replaces mlp.fc1 + activation of the CLIP / SigLIP vision towers' blocks (transformers
// CLIPMLP / SiglipMLP) where the launch is large enough for the 8-phase schedule.  A translation unit of their own: the
// resource rules of the kernel (no scratch, no vector-memory instruction its counted waits do not know) are checked
// per file, four instantiations each (tests/test_abi_cpu.py, tests/test_clip_cpu.py).
#include "gemm_kernels.h"
#include "gemm_8p_kernel.h"

namespace vdr {

hipError_t launch_gemm_8p_act(const G8& g, int epi, bool fold, int grid, int dev, hipStream_t s) {
  if (epi == EPI_BIAS_QGELU)
    return fold ? launch_8p_instance<EPI_BIAS_QGELU, true>(g, grid, dev, s) : launch_8p_instance<EPI_BIAS_QGELU, false>(g, grid, dev, s);
  if (epi == EPI_BIAS_TGELU)
    return fold ? launch_8p_instance<EPI_BIAS_TGELU, true>(g, grid, dev, s) : launch_8p_instance<EPI_BIAS_TGELU, false>(g, grid, dev, s);
  return hipErrorInvalidValue;
}

}  // namespace vdr
