// Device code of the four batch-1 production instantiations of the decode GEMV alone: compiles in seconds, without a GPU, so that
// tests/test_gemv_isa_cpu.py can hold their registers, occupancy and counted waits (not part of the library).
#include "gemv_kernel.h"

namespace {
template __global__ void gemv_bf16_kernel<1, 2, 8, true, false, 4>(GemvParams);
template __global__ void gemv_bf16_kernel<1, 2, 8, true, false, 8>(GemvParams);
template __global__ void gemv_bf16_kernel<1, 2, 8, true, true, 4>(GemvParams);
template __global__ void gemv_bf16_kernel<1, 2, 8, true, true, 8>(GemvParams);
}  // namespace
