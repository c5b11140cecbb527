// Global -> LDS loads without registers in between (gfx950 LDS-DMA), shared by the streaming kernels of knn.hip and dgl_fc_stream.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// lane i's 16 bytes land at lds_dst + 16 i (lds_dst wave-uniform): global_load_lds_dwordx4, no registers in between.  The destination
// is lane-linear, so a swizzled LDS image comes from permuting the SOURCE addresses of the lanes (and reading through the same XOR).
// The load counts in vmcnt like any other vector load.
__device__ __forceinline__ void lds_dma_1k(const void* gsrc_lane, uint32_t lds_dst) {
    uint32_t keep;
    lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc_lane), "s"(lds_dst)
                 : "memory");
}
