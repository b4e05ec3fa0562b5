// Device code of the batch-1 production instantiations of the decode GEMV alone: compiles in seconds, without a GPU, so that
// tests/test_gemv_isa_cpu.py and tests/test_gemv_noepi_isa_cpu.py can hold their registers, occupancy and counted waits (not part of
// the library).
#include "gemv_kernel.h"

namespace {
template __global__ void gemv_bf16_kernel<1, 2, 8, true, false, 4>(GemvParams);
template __global__ void gemv_bf16_kernel<1, 2, 8, true, false, 8>(GemvParams);
template __global__ void gemv_bf16_kernel<1, 2, 8, true, true, 4>(GemvParams);
template __global__ void gemv_bf16_kernel<1, 2, 8, true, true, 8>(GemvParams);
// the operand-free form at K of one batch: one unit per wave at 4 and 8 waves (QKV), looping at 8 waves (gate|up, lm_head)
template __global__ void gemv_bf16_noepi_kernel<1, 2, 8, true, 4, GEMV_K_ONE, 1>(GemvParams);
template __global__ void gemv_bf16_noepi_kernel<1, 2, 8, true, 8, GEMV_K_ONE, 1>(GemvParams);
template __global__ void gemv_bf16_noepi_kernel<1, 2, 8, true, 8, GEMV_K_ONE, 4>(GemvParams);
}  // namespace
