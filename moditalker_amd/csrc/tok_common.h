// Device helpers the token stages share (ae.hip, atom.hip, hubert.hip, tok_attn.hip, conv_x3.hip's GEGLU).  Internal; gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { ACT_NONE = 0, ACT_GELU = 1, ACT_MISH = 2, ACT_SILU = 3 };

// exact (erf) GELU, F.gelu's default
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float act_apply(float y, int act) {
    if (act == ACT_GELU) return gelu_erf(y);
    if (act == ACT_MISH) return y * tanhf(y > 20.0f ? y : log1pf(expf(y)));
    if (act == ACT_SILU) return y / (1.0f + expf(-y));
    return y;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// LayerNorm statistics by one wave of the row of K floats at x[off ..] (+ the row at x2[off ..] when x2 is not null): lane-strided sums, two
// passes (mean, then the centred sum of squares).  Every lane returns the same mean and rstd.  x2 is tested inside the loops as the
// caller's own (wave-uniform) pointer, so the compiler hoists the test out of them.
// (ae.hip's k_layernorm is NOT this: it keeps the row in registers and sums pairwise with fmaf, so its summation order differs.)
__device__ __forceinline__ void ln_row_stats(const float* x, const float* x2, size_t off, int K, float eps, int lane, float* mean_out, float* rstd_out) {
    float s = 0.0f;
    for (int k = lane; k < K; k += 64) s += x[off + k] + (x2 ? x2[off + k] : 0.0f);
    const float mean = wave_sum(s) / (float)K;
    float v = 0.0f;
    for (int k = lane; k < K; k += 64) {
        const float d = x[off + k] + (x2 ? x2[off + k] : 0.0f) - mean;
        v += d * d;
    }
    *mean_out = mean;
    *rstd_out = 1.0f / sqrtf(wave_sum(v) / (float)K + eps);
}
