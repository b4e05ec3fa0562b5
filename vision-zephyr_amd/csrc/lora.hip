// LoRA branch of the Stage-2 finetune step (train_engine.hip): the dropout of the adapter's input and the gate|up column permutation.
//
// peft's adapted linear (ref:vis_zephyr/train/train.py:933-951 -> peft `Linear.forward`): y = W x + scaling * B (A dropout(x)), each
// adapted module with its own nn.Dropout(p).  The trainer never stores a mask: the kernel below writes
//     out = res + keep(c) * x * scaling / (1 - p)        (bf16, fp32 arithmetic, one rounding; res optional)
// and the backward writes the same mask again from the same counter (the input gradient of the branch and dA's operand).
//     keep(c) = Philox4x32-10(key = seed, counter = (c / 4, sample * row_stride + position, layer * 7 + module, optimiser step)) word c % 4
//               >= thr,   thr = floor(p * 2^32)
// with `sample` the index of the row's sample within the OPTIMISER batch (sample_base + row / S), so splitting the batch into
// micro-batches changes no mask.  vz_hip/lora.py::dropout_keep is the numpy restatement (tests/test_lora_*: bit for bit).
#include "vz_common.h"

namespace {

// one thread = 8 consecutive columns (one 16-byte load / store); two Philox calls cover them
__global__ void __launch_bounds__(256) lora_dropout_kernel(const bf16_t* __restrict__ x, long ldx, bf16_t* out, long ldo, const bf16_t* res,
                                                           long ldr, int rows, int cols, int S, long sample_base, long row_stride, unsigned tag,
                                                           unsigned step, unsigned k0, unsigned k1, unsigned thr, float scale) {
    const int cpr = cols >> 3;
    const long n = (long)rows * cpr;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / cpr), c = (int)(i - (long)r * cpr) << 3;
        const unsigned c1 = (unsigned)((sample_base + r / S) * row_stride + r % S);
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0;            // p = 0: every word >= thr = 0, no draw needed
        if (thr) {
            w0 = philox4x32_10((unsigned)(c >> 2), c1, tag, step, k0, k1);
            w1 = philox4x32_10((unsigned)(c >> 2) + 1u, c1, tag, step, k0, k1);
        }
        const unsigned w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
        const u16x8 xv = *(const u16x8*)(x + (size_t)r * ldx + c);
        u16x8 rv = {0, 0, 0, 0, 0, 0, 0, 0};
        if (res) rv = *(const u16x8*)(res + (size_t)r * ldr + c);
        u16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = w[j] >= thr ? bf16_to_f32(xv[j]) * scale : 0.f;
            o[j] = f32_to_bf16(res ? bf16_to_f32(rv[j]) + v : v);
        }
        *(u16x8*)(out + (size_t)r * ldo + c) = o;
    }
}

// the engine's fused gate|up layout (vz_hip/engine.py: gu.w rows = 16 gate rows, 16 up rows, repeated) <-> [gate | up] halves.
// to_plain: dst[r][h * I + 16 g + w] = src[r][32 g + 16 h + w]; else the inverse.  8 columns (16 bytes) per thread.
__global__ void __launch_bounds__(256) gu_permute_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, long rows, int I, int to_plain) {
    const int cpr = (2 * I) >> 3;
    const long n = rows * cpr;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cpr;
        const int pc = (int)(i - r * cpr) << 3;                      // plain column
        const int h = pc >= I, q = pc - h * I, g = q >> 4, w = q & 15;
        const int ic = 32 * g + 16 * h + w;                           // interleaved column
        const size_t ro = (size_t)r * 2 * I;
        if (to_plain) *(u16x8*)(dst + ro + pc) = *(const u16x8*)(src + ro + ic);
        else          *(u16x8*)(dst + ro + ic) = *(const u16x8*)(src + ro + pc);
    }
}

int grid_for(long n) { return (int)std::min<long>((n + 255) / 256, 4096); }

}  // namespace

unsigned vz_lora_threshold(float p) { return (unsigned)std::floor((double)p * 4294967296.0); }
float vz_lora_factor(float scaling, float p) { return (float)((double)scaling / (1.0 - (double)p)); }

int vz_launch_lora_dropout(const bf16_t* x, long ldx, bf16_t* out, long ldo, const bf16_t* res, long ldr, int rows, int cols, int S,
                           long sample_base, long row_stride, int tag, int step, unsigned long long seed, float p, float scaling, hipStream_t s) {
    VZ_CHECK_ARG(x && out && rows >= 0 && cols > 0 && (cols & 7) == 0 && S >= 1 && sample_base >= 0 && row_stride >= S && p >= 0.f && p < 1.f,
                 "lora_dropout: bad argument (rows %d cols %d S %d stride %ld p %g)", rows, cols, S, row_stride, (double)p);
    VZ_CHECK_ARG((ldx & 7) == 0 && (ldo & 7) == 0 && (!res || (ldr & 7) == 0) && ldx >= cols && ldo >= cols && (!res || ldr >= cols) &&
                 ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)res & 15) == 0,
                 "lora_dropout: leading dimensions must be multiples of 8 and the bases 16-byte aligned");
    VZ_CHECK_ARG((sample_base + (long)(rows + S - 1) / S) * row_stride <= 0xFFFFFFFFL, "lora_dropout: row counter exceeds 32 bits");
    if (rows == 0) return VZ_OK;
    const long n = (long)rows * (cols >> 3);
    hipLaunchKernelGGL(lora_dropout_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, ldx, out, ldo, res, ldr, rows, cols, S, sample_base, row_stride,
                       (unsigned)tag, (unsigned)step, (unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), vz_lora_threshold(p),
                       vz_lora_factor(scaling, p));
    VZ_CHECK_HIP(hipGetLastError());
    return VZ_OK;
}

int vz_launch_gu_permute(const bf16_t* src, bf16_t* dst, long rows, int I, int to_plain, hipStream_t s) {
    VZ_CHECK_ARG(src && dst && src != dst && rows >= 0 && I > 0 && (I & 15) == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0,
                 "gu_permute: bad argument");
    if (rows == 0) return VZ_OK;
    const long n = rows * ((2 * I) >> 3);
    hipLaunchKernelGGL(gu_permute_kernel, dim3(grid_for(n)), dim3(256), 0, s, src, dst, rows, I, to_plain);
    VZ_CHECK_HIP(hipGetLastError());
    return VZ_OK;
}

extern "C" int vz_op_lora_dropout(const void* d_x, int ldx, void* d_out, int ldo, int rows, int cols, int S, long sample_base, long row_stride,
                                  int tag, int step, unsigned long long seed, float p, float scaling, vz_stream stream) {
    return vz_launch_lora_dropout((const bf16_t*)d_x, ldx, (bf16_t*)d_out, ldo, nullptr, 0, rows, cols, S, sample_base, row_stride, tag, step,
                                  seed, p, scaling, (hipStream_t)stream);
}
