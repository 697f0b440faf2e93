// The two kernels AToM (atom.hip) and HuBERT (hubert.hip) share: softmax attention of one head and the strided row copy.
#include "plan_internal.h"
#include "tok_common.h"

namespace {
// Attention of one (clip, stream, head, 16 queries): softmax(q k^T scale) v, nn.MultiheadAttention's core.  Keys go by in chunks of KCH in
// index order with a running max m and sum l; the accumulator is rescaled by exp(m_old - m_new).  Every loop is bounded by Lq / Lk, so
// any query and key length is served; with Lk <= KCH (AToM: 3 L + 2 <= 512 keys) there is one chunk and the running form IS the plain
// softmax, bit for bit: alpha = exp(-inf) = 0 scales an all-zero accumulator and l = 0 * 0 + sum.
template <int KCH>
__global__ __launch_bounds__(256) void k_tok_attn(const TokAttnArgs a) {
    __shared__ float s_q[16][68];
    __shared__ float s_p[16][KCH];
    __shared__ float s_m[16], s_l[16], s_alpha[16];
    constexpr int UNROLL_D = KCH == 512 ? 4 : 1;
    const int tid = threadIdx.x, h = blockIdx.y, bz = blockIdx.z, b = bz / a.S, st = bz - b * a.S;
    const int q0 = blockIdx.x * 16;
    const float* qb = a.q + (size_t)b * a.q_bs + (size_t)st * a.q_ss + h * a.d;
    const float* kb = a.k + (size_t)b * a.k_bs + (size_t)st * a.k_ss + h * a.d;
    const float* vb = a.v + (size_t)b * a.k_bs + (size_t)st * a.k_ss + h * a.d;
    const int qi = tid >> 4, d4 = (tid & 15) * 4;
    if (d4 < a.d) {
        f32x4 x{0.0f, 0.0f, 0.0f, 0.0f};
        if (q0 + qi < a.Lq) x = *reinterpret_cast<const f32x4*>(qb + (size_t)(q0 + qi) * a.q_rs + d4) * a.scale;
        *reinterpret_cast<f32x4*>(&s_q[qi][d4]) = x;
    }
    if (tid < 16) {
        s_m[tid] = -INFINITY;
        s_l[tid] = 0.0f;
    }
    f32x4 acc{0.0f, 0.0f, 0.0f, 0.0f};
    __syncthreads();
    for (int k0 = 0; k0 < a.Lk; k0 += KCH) {
        const int nk = min(KCH, a.Lk - k0);
        {   // scores: thread = (key, group of 4 queries)
            const int g = tid & 3;
            for (int kj = tid >> 2; kj < nk; kj += 64) {
                const float* kr = kb + (size_t)(k0 + kj) * a.k_rs;
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
                // <512> (AToM, one chunk): four key quads in flight.  The compiler unrolled this loop by four when the kernel had no chunk loop
                // around it and leaves it rolled now; rolled, a 50-step AToM sample is 2 % slower than before (profiles/tok_shared_ab.txt).
                // <256> (HuBERT) stays rolled, as it always compiled: 72 registers instead of 102, 7 waves per SIMD instead of 4.
#pragma unroll UNROLL_D
                for (int dd = 0; dd < a.d; dd += 4) {
                    const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + dd);
                    const f32x4 q0v = *reinterpret_cast<const f32x4*>(&s_q[4 * g + 0][dd]), q1v = *reinterpret_cast<const f32x4*>(&s_q[4 * g + 1][dd]);
                    const f32x4 q2v = *reinterpret_cast<const f32x4*>(&s_q[4 * g + 2][dd]), q3v = *reinterpret_cast<const f32x4*>(&s_q[4 * g + 3][dd]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        s0 = fmaf(q0v[i], kv[i], s0);
                        s1 = fmaf(q1v[i], kv[i], s1);
                        s2 = fmaf(q2v[i], kv[i], s2);
                        s3 = fmaf(q3v[i], kv[i], s3);
                    }
                }
                s_p[4 * g + 0][kj] = s0;
                s_p[4 * g + 1][kj] = s1;
                s_p[4 * g + 2][kj] = s2;
                s_p[4 * g + 3][kj] = s3;
            }
        }
        __syncthreads();
        {   // a wave per 4 rows: new running max, the chunk's exponentials, the running sum
            const int wave = tid >> 6, lane = tid & 63;
            for (int r = wave * 4; r < wave * 4 + 4; ++r) {
                float m = -INFINITY;
                for (int kj = lane; kj < nk; kj += 64) m = fmaxf(m, s_p[r][kj]);
#pragma unroll
                for (int of = 32; of > 0; of >>= 1) m = fmaxf(m, __shfl_xor(m, of, 64));
                const float m_old = s_m[r], m_new = fmaxf(m_old, m);
                float sum = 0.0f;
                for (int kj = lane; kj < nk; kj += 64) {
                    const float e = expf(s_p[r][kj] - m_new);
                    s_p[r][kj] = e;
                    sum += e;
                }
                sum = wave_sum(sum);
                if (lane == 0) {
                    const float al = expf(m_old - m_new);      // (first chunk: exp(-inf) = 0)
                    s_alpha[r] = al;
                    s_l[r] = s_l[r] * al + sum;
                    s_m[r] = m_new;
                }
            }
        }
        __syncthreads();
        if (d4 < a.d) {
            acc *= s_alpha[qi];
            for (int kj = 0; kj < nk; ++kj) acc += *reinterpret_cast<const f32x4*>(vb + (size_t)(k0 + kj) * a.k_rs + d4) * s_p[qi][kj];
        }
        __syncthreads();
    }
    if (d4 < a.d && q0 + qi < a.Lq)
        *reinterpret_cast<f32x4*>(a.o + (size_t)b * a.o_bs + (size_t)st * a.o_ss + (size_t)(q0 + qi) * a.o_rs + h * a.d + d4) = acc * (1.0f / s_l[qi]);
}

__global__ void k_tok_copy(const float* src, long long src_bs, float* dst, long long dst_bs, long long n, int nb) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * nb) return;
    const long long b = i / n, w = i - b * n;
    dst[b * dst_bs + w] = src[b * src_bs + w];
}
}  // namespace

hipError_t launch_tok_attn(const TokAttnArgs& a, int nb, int kch, hipStream_t s) {
    const dim3 grid((unsigned)((a.Lq + 15) / 16), (unsigned)a.H, (unsigned)(nb * a.S));
    if (kch == 256) hipLaunchKernelGGL(k_tok_attn<256>, grid, dim3(256), 0, s, a);
    else if (kch == 512) hipLaunchKernelGGL(k_tok_attn<512>, grid, dim3(256), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_tok_copy(const float* src, long long src_bs, float* dst, long long dst_bs, long long n, int nb, hipStream_t s) {
    if (n * nb <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tok_copy, dim3((unsigned)((n * nb + 255) / 256)), dim3(256), 0, s, src, src_bs, dst, dst_bs, n, nb);
    return hipGetLastError();
}
