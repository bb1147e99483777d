// ffn_fused_kernel<32, true, FfnProj>: the level-0 FFN kernel with the stage tail and the attention projection (rf_fused_tile.h), in a
// translation unit of its own so that the kernels of rf_fused.hip and rf_fused_tail.hip compile exactly as they do without it.
#undef RF_STAMP      // the cycle stamps belong to rf_fused.hip's instantiation
#include "rf_fused_tile.h"

namespace rf {

int launch_ffn_fused_proj32(const FfnArgs& a, const FfnTail& tail, const FfnProj& pj, dim3 grid, hipStream_t st) {
    ffn_fused_kernel<32, true, FfnProj><<<grid, 256, 0, st>>>(a, tail, pj);
    return check_launch("ffn_fused (stage tail, projection)");
}

}  // namespace rf
