// ring4 tile variants 26-29 (gemm_kernels.h: both operands staged in whole 128-B lines).  Own translation unit so that
// its instantiations compile in parallel with the ring3 ones of gemm.hip.
#include "gemm_kernels.h"

namespace vdr {

hipError_t launch_gemm_ring4(const GemmLaunch& L, hipStream_t s) { return launch_tiles<26, 27, 28, 29>(L, s); }

}  // namespace vdr
