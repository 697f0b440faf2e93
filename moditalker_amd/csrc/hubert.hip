// HuBERT audio features for gfx950: the stage in front of AToM.  A 16 kHz waveform in, last_hidden_state [B, T, hidden] out -- what
// data/data_utils/preprocess/process_audio.py:9-55 gets from transformers' HubertModel (facebook/hubert-large-ls960-ft: seven layer-normed
// conv layers, LayerNorm + projection, a weight-normed grouped positional conv, 24 stable-layer-norm transformer layers of width 1024)
// and from Wav2Vec2FeatureExtractor's normalisation.
//
// Layout: every activation is token-major, [clip][token][channel].  That makes each strided Conv1d of layers 2..7 a plain GEMM: output
// token t reads input tokens t s .. t s + k - 1, which are k C CONTIGUOUS floats, against the weight repacked once to [Cout][tap][Cin].
// The grouped positional conv is the same GEMM per group with a two-level K index (tap, channel of the group) and a bounds test on the
// token (zero padding; a clip never reads its neighbour in the batch).  So one kernel, k_hub_gemm, serves the convs, the positional conv
// and every Linear:
//   * 64 x 64 outputs per workgroup, a 32 x 32 quadrant per wave, exact-f32 MFMA (16x16x4), operands straight from global memory as
//     16-byte loads ([N][K] weights as the checkpoint stores them).  Every wave walks the whole of K in index order, so an output element
//     depends on its own row, its column and the weights only: neither the grid nor the batch size can change a bit.
//   * optional LayerNorm prologue over K (Linears), bias / exact-erf GELU / residual epilogue.
// LayerNorm + GELU of a conv layer is its own in-place pass (k_hub_ln, a wave per row): the next layer's GEMM row spans k tokens, each with
// its own statistics.  Layer 1 (one input channel, K = 10) is k_hub_conv0.  Attention is tok_attn.hip's k_tok_attn<256>, shared with
// atom.hip: 16 queries of one head per workgroup, keys in chunks of 256 with a running max / sum (any key length: 1000 at a full 20 s
// clip), keys in index order.
// A forward is one linear chain of plain launches on the caller's stream; shapes follow the clip length, so nothing is captured.
#include "plan_internal.h"
#include "tok_common.h"

namespace {
constexpr int HUB_KCH = 256;       // keys per chunk of k_tok_attn here
constexpr int HUB_PARTS = 256;     // workgroups (= partial sums) of a normalisation pass

// ---- the GEMM
// Logical output row r: clip b = r / T_out, token t = r % T_out.  Reduction index k: tap = k / kc, channel kk = k % kc; the A element is
// A[b a_bs + (t tok_step + tap - pad) tap_stride + g a_goff + kk], zero when that token is outside [0, T_in).  kc and K are multiples of 4,
// so a lane's quad never straddles a tap.  Group g (blockIdx.z) owns weight rows / output columns g N .. g N + N - 1.
// (not atom.hip's k_tok_linear, which splits K over the four waves and meets in LDS: the bits and the tile shapes differ by design)
struct HubGemm {
    const float* A;
    long long a_bs;
    int tap_stride, tok_step, kc, pad, T_in, a_goff;
    int T_out, M, K, N;
    const float* W;                // [groups N][K]
    const float* bias;             // [groups N]
    const float *ln_g, *ln_b;      // LayerNorm of the row over K (kc == K only); nullptr: none
    float eps;
    int act;
    const float* res;              // residual, addressed like the output; nullptr: none
    float* out;
    int ldo;
};

__global__ __launch_bounds__(256) void k_hub_gemm(const HubGemm a) {
    __shared__ float s_stat[64][2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64, g = blockIdx.z;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    if (a.ln_g) {
        for (int i = 0; i < 16; ++i) {
            const int rr = wave * 16 + i, r = m0 + rr;
            float mean = 0.0f, rstd = 0.0f;
            if (r < a.M) ln_row_stats(a.A, nullptr, (size_t)r * a.tap_stride, a.K, a.eps, lane, &mean, &rstd);
            if (lane == 0) {
                s_stat[rr][0] = mean;
                s_stat[rr][1] = rstd;
            }
        }
        __syncthreads();
    }
    const int j = lane & 15, q = lane >> 4;
    const float* abase[2];
    int tok0[2];
    float mean[2], rstd[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int r = min(m0 + wr + rb * 16 + j, a.M - 1);       // (rows past M repeat the last row; they are not stored)
        const int b = r / a.T_out, t = r - b * a.T_out;
        abase[rb] = a.A + (size_t)b * a.a_bs + (size_t)g * a.a_goff;
        tok0[rb] = t * a.tok_step - a.pad;
        mean[rb] = a.ln_g ? s_stat[r - m0][0] : 0.0f;
        rstd[rb] = a.ln_g ? s_stat[r - m0][1] : 1.0f;
    }
    const float* wrow[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) wrow[cb] = a.W + ((size_t)g * a.N + min(n0 + wc + cb * 16 + j, a.N - 1)) * a.K;
    f32x4 acc[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const f32x4 zero4{0.0f, 0.0f, 0.0f, 0.0f};
    const int nch = (a.K + 15) >> 4;
    const bool flat = a.kc == a.K;
    for (int c = 0; c < nch; ++c) {
        // lane (j, q) holds elements 16 c + 4 q .. + 3 of A row j and of W row j; the four MFMA steps pair element i of both.  A quad
        // past K or on a padding token multiplies zeros: every lane reaches the MFMAs, none branches around them.
        const int k = 16 * c + 4 * q;
        const bool kin = k < a.K;
        const int tap = flat ? 0 : k / a.kc, kk = k - tap * a.kc;
        f32x4 bw[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) bw[cb] = kin ? *reinterpret_cast<const f32x4*>(wrow[cb] + k) : zero4;
        f32x4 gm{1.0f, 1.0f, 1.0f, 1.0f}, be = zero4;
        if (a.ln_g && kin) {
            gm = *reinterpret_cast<const f32x4*>(a.ln_g + k);
            be = *reinterpret_cast<const f32x4*>(a.ln_b + k);
        }
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int tok = tok0[rb] + tap;
            const bool ok = kin && tok >= 0 && tok < a.T_in;
            f32x4 x = ok ? *reinterpret_cast<const f32x4*>(abase[rb] + (size_t)tok * a.tap_stride + kk) : zero4;
            if (a.ln_g && kin) x = (x - mean[rb]) * rstd[rb] * gm + be;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[i], bw[cb][i], acc[rb][cb], 0, 0, 0);
        }
    }
    // C/D map of the 16x16 forms: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int col = n0 + wc + cb * 16 + j;
            if (col >= a.N) continue;
            const int cg = g * a.N + col;
            const float bias = a.bias[cg];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m0 + wr + rb * 16 + 4 * q + i;
                if (row >= a.M) continue;
                float y = act_apply(acc[rb][cb][i] + bias, a.act);
                const size_t o = (size_t)row * a.ldo + cg;
                if (a.res) y += a.res[o];
                a.out[o] = y;
            }
        }
}
hipError_t launch_hub_gemm(const HubGemm& a, int groups, hipStream_t s) {
    hipLaunchKernelGGL(k_hub_gemm, dim3((unsigned)((a.N + 63) / 64), (unsigned)((a.M + 63) / 64), (unsigned)groups), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- LayerNorm over the C channels of a row (+ GELU): a wave per row, two passes; out may be x
__global__ __launch_bounds__(256) void k_hub_ln(const float* x, float* out, const float* gm, const float* be, int M, int C, float eps, int act) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const float* row = x + (size_t)r * C;
    float mean, rstd;
    ln_row_stats(row, nullptr, 0, C, eps, lane, &mean, &rstd);
    float* o = out + (size_t)r * C;
    for (int k = lane; k < C; k += 64) {
        const float y = (row[k] - mean) * rstd * gm[k] + be[k];
        o[k] = act_apply(y, act);
    }
}
hipError_t launch_hub_ln(const float* x, float* out, const float* gm, const float* be, int M, int C, float eps, int act, hipStream_t s) {
    hipLaunchKernelGGL(k_hub_ln, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, out, gm, be, M, C, eps, act);
    return hipGetLastError();
}

// ---- conv layer 1: one input channel.  out[b][t][c] = bias[c] + sum_j w[c][j] wave[b][t s + j]; t s + j <= (T - 1) s + k - 1 < n
__global__ __launch_bounds__(256) void k_hub_conv0(const float* wave, long long n, const float* w, const float* bias, float* out, int T, int C, int k,
                                                   int s, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long r = i / C;
    const int c = (int)(i - r * C);
    const long long b = r / T, t = r - b * T;
    const float* x = wave + b * n + t * s;
    float acc = 0.0f;
    for (int jj = 0; jj < k; ++jj) acc = fmaf(w[c * k + jj], x[jj], acc);
    out[i] = acc + bias[c];
}

// ---- waveform normalisation: fixed-order reductions in fp64.  A pass writes HUB_PARTS partial sums; the next launch adds them up in index
// order (every workgroup does, redundantly: same order, same value).
__device__ double hub_block_sum(double v, double* s_red) {
    const int tid = threadIdx.x;
    s_red[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) s_red[tid] += s_red[tid + w];
        __syncthreads();
    }
    const double r = s_red[0];
    __syncthreads();
    return r;
}
__device__ double hub_parts_total(const double* part) {
    double t = 0.0;
    for (int i = 0; i < HUB_PARTS; ++i) t += part[i];
    return t;
}
// part_in == nullptr: partial sums of x; else partial sums of (x - mean)^2 with mean = total(part_in) / n
__global__ __launch_bounds__(256) void k_hub_norm_part(const float* x, long long n, const double* part_in, double* part_out) {
    __shared__ double s_red[256];
    const double mean = part_in ? hub_parts_total(part_in) / (double)n : 0.0;
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)HUB_PARTS * 256) {
        const double dlt = (double)x[i] - mean;
        s += part_in ? dlt * dlt : dlt;
    }
    s = hub_block_sum(s, s_red);
    if (threadIdx.x == 0) part_out[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_hub_norm_apply(const float* x, long long n, const double* part_sum, const double* part_sq, float* out) {
    const double mean = hub_parts_total(part_sum) / (double)n;
    const double var = hub_parts_total(part_sq) / (double)n;
    const double rstd = 1.0 / sqrt(var + 1e-7);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = (float)(((double)x[i] - mean) * rstd);
}

// ---- weight preparation (once after a load)
// Conv1d weight [N][C][k] -> [N][k][C] times scale[tap] (nullptr: 1)
__global__ void k_hub_repack(const float* src, float* dst, const float* scale, int N, int C, int k) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * C * k) return;
    const int n = (int)(i / ((long long)C * k)), rem = (int)(i - (long long)n * C * k), tap = rem / C, ci = rem - tap * C;
    dst[i] = src[((size_t)n * C + ci) * k + tap] * (scale ? scale[tap] : 1.0f);
}
// weight_norm(dim = 2): scale[tap] = g[tap] / |v[:, :, tap]|; one workgroup per tap
__global__ __launch_bounds__(256) void k_hub_pos_scale(const float* v, const float* g, float* scale, long long rows, int k) {
    __shared__ double s_red[256];
    const int tap = blockIdx.x;
    double s = 0.0;
    for (long long r = threadIdx.x; r < rows; r += 256) {
        const double e = v[r * k + tap];
        s += e * e;
    }
    s = hub_block_sum(s, s_red);
    if (threadIdx.x == 0) scale[tap] = g[tap] / (float)sqrt(s);
}

// =====================================================================================================================================
struct HubState {
    mtv_hubert_config f;
    int H, nl, nc, ff, Cg;
    std::map<std::string, float*> w;            // parameter name -> device copy (the checkpoint's own layout)
    std::vector<float*> Wc;                     // conv layers 2..: [Cout][tap][Cin]
    float *Wpos, *pscale;                       // positional conv, weight norm applied: [H][tap][H / groups]
    std::vector<float*> Wqkv, bqkv;             // q | k | v projections of a layer as one [3 H][H] matrix
    float *FA, *FB, *P, *X, *QKV, *ATT, *FFB, *tap_pos, *tap_l0;
    double* part;                               // [2][HUB_PARTS]
    unsigned prepared_serial = 0;
    bool prepared = false, keep = false;
    int last_rows = 0;
    const float* last_feat = nullptr;
};
HubState* hub_of(mtv_ctx* c) { return c && c->kind == CTX_HUBERT ? static_cast<HubState*>(c->ext.get()) : nullptr; }

// frames after every conv layer; false when a layer has no valid window
bool hub_frames(const mtv_hubert_config& f, long long n, int* T) {
    for (int i = 0; i < f.n_conv; ++i) {
        if (n < f.conv_kernel[i]) return false;
        n = (n - f.conv_kernel[i]) / f.conv_stride[i] + 1;
        T[i] = (int)n;
    }
    return true;
}

hipError_t hub_prepare(mtv_ctx* c, HubState& S) {
    if (S.prepared && S.prepared_serial == c->load_serial) return hipSuccess;
    for (int i = 1; i < S.nc; ++i) {
        const int N = S.f.conv_dim[i], C = S.f.conv_dim[i - 1], k = S.f.conv_kernel[i];
        const long long n = (long long)N * C * k;
        hipLaunchKernelGGL(k_hub_repack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                           S.w.at("feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight"), S.Wc[i], (const float*)nullptr, N, C, k);
    }
    const std::string pc = "encoder.pos_conv_embed.conv.parametrizations.weight.original";
    const int k = S.f.pos_taps;
    hipLaunchKernelGGL(k_hub_pos_scale, dim3((unsigned)k), dim3(256), 0, nullptr, S.w.at(pc + "1"), S.w.at(pc + "0"), S.pscale, (long long)S.H * S.Cg, k);
    const long long n = (long long)S.H * S.Cg * k;
    hipLaunchKernelGGL(k_hub_repack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, S.w.at(pc + "1"), S.Wpos, S.pscale, S.H, S.Cg, k);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) {
        S.prepared = true;
        S.prepared_serial = c->load_serial;
    }
    return e;
}

HubGemm hub_linear(const float* A, int lda, int M, int K, const float* W, const float* bias, int N, float* out, int ldo) {
    HubGemm a{};
    a.A = A;
    a.tap_stride = lda;
    a.tok_step = 1;
    a.kc = K;
    a.T_in = a.T_out = a.M = M;
    a.K = K;
    a.N = N;
    a.W = W;
    a.bias = bias;
    a.out = out;
    a.ldo = ldo;
    return a;
}

// The launch chain of one forward: wave [B][n] -> out [B][T][H]
void hub_build(HubState* Sp, std::vector<Op>& ops, const float* wave, int n, int B, const int* T, float* out) {
    HubState& S = *Sp;
    const mtv_hubert_config& f = S.f;
    const int H = S.H, ffn = S.ff, Tt = T[S.nc - 1], M = B * Tt, d = H / f.heads;
    auto add = [&](const std::string& name, double flops, std::function<hipError_t(hipStream_t)> fn) {
        Op op{std::move(fn), name};
        op.flops = flops;
        ops.push_back(std::move(op));
    };
    auto add_gemm = [&](const std::string& name, const HubGemm& a, int groups = 1) {
        add(name, 2.0 * a.M * a.K * a.N * groups, [a, groups](hipStream_t s) { return launch_hub_gemm(a, groups, s); });
    };
    auto add_ln = [&](const std::string& name, const float* x, float* o, const std::string& pre, int rows, int C, float eps, int act) {
        const float *gm = S.w.at(pre + ".weight"), *be = S.w.at(pre + ".bias");
        add(name, 0.0, [=](hipStream_t s) { return launch_hub_ln(x, o, gm, be, rows, C, eps, act, s); });
    };
    float *cur = S.FA, *nxt = S.FB;
    {
        const std::string pre = "feature_extractor.conv_layers.0.";
        const float *w = S.w.at(pre + "conv.weight"), *bias = S.w.at(pre + "conv.bias");
        const int C = f.conv_dim[0], k = f.conv_kernel[0], st = f.conv_stride[0], T0 = T[0];
        const long long total = (long long)B * T0 * C;
        add("conv0", 2.0 * total * k, [=](hipStream_t s) {
            hipLaunchKernelGGL(k_hub_conv0, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, wave, (long long)n, w, bias, cur, T0, C, k, st, total);
            return hipGetLastError();
        });
        add_ln("conv0.ln_gelu", cur, cur, pre + "layer_norm", B * T0, C, 1e-5f, ACT_GELU);
    }
    for (int i = 1; i < S.nc; ++i) {
        const std::string pre = "feature_extractor.conv_layers." + std::to_string(i) + ".", tag = "conv" + std::to_string(i);
        const int Ci = f.conv_dim[i - 1], Co = f.conv_dim[i], k = f.conv_kernel[i];
        HubGemm a = hub_linear(cur, Ci, B * T[i], k * Ci, S.Wc[i], S.w.at(pre + "conv.bias"), Co, nxt, Co);
        a.a_bs = (long long)T[i - 1] * Ci;
        a.tok_step = f.conv_stride[i];
        a.kc = Ci;
        a.T_in = T[i - 1];
        a.T_out = T[i];
        add_gemm(tag, a);
        add_ln(tag + ".ln_gelu", nxt, nxt, pre + "layer_norm", B * T[i], Co, 1e-5f, ACT_GELU);
        std::swap(cur, nxt);
    }
    S.last_feat = cur;
    S.last_rows = M;
    const int Cl = f.conv_dim[S.nc - 1];
    HubGemm a = hub_linear(cur, Cl, M, Cl, S.w.at("feature_projection.projection.weight"), S.w.at("feature_projection.projection.bias"), H, S.P, H);
    a.ln_g = S.w.at("feature_projection.layer_norm.weight");
    a.ln_b = S.w.at("feature_projection.layer_norm.bias");
    a.eps = f.eps;
    add_gemm("feature_projection", a);
    // x + gelu(pos_conv(x)): zero padding of pos_taps / 2 tokens on both sides of every clip; an even tap count drops the last output, which
    // leaves exactly rows 0 .. T - 1 of the padded conv
    a = hub_linear(S.P, H, M, f.pos_taps * S.Cg, S.Wpos, S.w.at("encoder.pos_conv_embed.conv.bias"), S.Cg, S.X, H);
    a.a_bs = (long long)Tt * H;
    a.kc = S.Cg;
    a.pad = f.pos_taps / 2;
    a.T_in = a.T_out = Tt;
    a.a_goff = S.Cg;
    a.act = ACT_GELU;
    a.res = S.P;
    add_gemm("pos_conv", a, f.pos_groups);
    auto add_keep = [&](const std::string& name, float* dst) {
        const float* src = S.X;
        const long long cnt = (long long)M * H;
        add(name, 0.0, [=](hipStream_t s) { return launch_tok_copy(src, 0, dst, 0, cnt, 1, s); });
    };
    if (S.keep) add_keep("keep.after_pos_conv", S.tap_pos);
    for (int l = 0; l < S.nl; ++l) {
        const std::string pre = "encoder.layers." + std::to_string(l) + ".", tag = "L" + std::to_string(l) + ".";
        a = hub_linear(S.X, H, M, H, S.Wqkv[l], S.bqkv[l], 3 * H, S.QKV, 3 * H);
        a.ln_g = S.w.at(pre + "layer_norm.weight");
        a.ln_b = S.w.at(pre + "layer_norm.bias");
        a.eps = f.eps;
        add_gemm(tag + "qkv", a);
        TokAttnArgs t{};
        t.q = S.QKV;
        t.k = S.QKV + H;
        t.v = S.QKV + 2 * H;
        t.o = S.ATT;
        t.q_bs = t.k_bs = (long long)Tt * 3 * H;
        t.q_rs = t.k_rs = 3 * H;
        t.o_bs = (long long)Tt * H;
        t.o_rs = H;
        t.Lq = t.Lk = Tt;
        t.H = f.heads;
        t.d = d;
        t.S = 1;
        t.scale = 1.0f / std::sqrt((float)d);
        add(tag + "attn", 4.0 * B * (double)Tt * Tt * H, [t, B](hipStream_t s) { return launch_tok_attn(t, B, HUB_KCH, s); });
        a = hub_linear(S.ATT, H, M, H, S.w.at(pre + "attention.out_proj.weight"), S.w.at(pre + "attention.out_proj.bias"), H, S.X, H);
        a.res = S.X;
        add_gemm(tag + "out_proj", a);
        a = hub_linear(S.X, H, M, H, S.w.at(pre + "feed_forward.intermediate_dense.weight"), S.w.at(pre + "feed_forward.intermediate_dense.bias"), ffn, S.FFB, ffn);
        a.ln_g = S.w.at(pre + "final_layer_norm.weight");
        a.ln_b = S.w.at(pre + "final_layer_norm.bias");
        a.eps = f.eps;
        a.act = ACT_GELU;
        add_gemm(tag + "ff1", a);
        a = hub_linear(S.FFB, ffn, M, ffn, S.w.at(pre + "feed_forward.output_dense.weight"), S.w.at(pre + "feed_forward.output_dense.bias"), H, S.X, H);
        a.res = S.X;
        add_gemm(tag + "ff2", a);
        if (S.keep && l == 0) add_keep("keep.layer_0", S.tap_l0);
    }
    add_ln("encoder.layer_norm", S.X, out, "encoder.layer_norm", M, H, f.eps, ACT_NONE);
}

// the argument checks of forward / num_launches / profile; nothing has been launched when they fail
int hub_check(mtv_ctx* c, HubState* S, int n_samples, int batch, int* T) {
    if (!S) return fail(MTV_ERR_INVALID, "not a HuBERT context");
    int rc = check_ready(c, batch);
    if (rc != MTV_OK) return rc;
    if (n_samples < 1 || n_samples > S->f.max_samples)
        return fail(MTV_ERR_INVALID, "n_samples " + std::to_string(n_samples) + " outside [1, max_samples = " + std::to_string(S->f.max_samples) + "]");
    if (!hub_frames(S->f, n_samples, T)) return fail(MTV_ERR_INVALID, "the clip is shorter than the conv encoder's receptive field: no output frame");
    return MTV_OK;
}
}  // namespace

extern "C" {

int mtv_hubert_create(const mtv_hubert_config* cfg, mtv_ctx** out) {
    if (!cfg || !out) return fail(MTV_ERR_INVALID, "null argument");
    const mtv_hubert_config& f = *cfg;
    if (f.hidden < 4 || f.hidden % 4 || f.intermediate < 4 || f.intermediate % 4) return fail(MTV_ERR_INVALID, "hidden and intermediate must be multiples of 4");
    if (f.heads < 1 || f.hidden % f.heads) return fail(MTV_ERR_INVALID, "hidden must be divisible by heads");
    const int d = f.hidden / f.heads;
    if (d % 4 || d > 64) return fail(MTV_ERR_INVALID, "head dim must be a multiple of 4, at most 64");
    if (f.n_conv < 1 || f.n_conv > MTV_HUBERT_MAX_CONV) return fail(MTV_ERR_INVALID, "n_conv outside [1, 8]");
    for (int i = 0; i < f.n_conv; ++i)
        if (f.conv_dim[i] < 4 || f.conv_dim[i] % 4 || f.conv_kernel[i] < 1 || f.conv_stride[i] < 1)
            return fail(MTV_ERR_INVALID, "conv_dim must be multiples of 4, conv_kernel and conv_stride positive");
    if (f.pos_taps < 1 || f.pos_groups < 1 || f.hidden % f.pos_groups || (f.hidden / f.pos_groups) % 4)
        return fail(MTV_ERR_INVALID, "hidden / pos_groups must be a multiple of 4");
    if (f.n_layers < 1 || f.max_batch < 1 || !(f.eps > 0.0f)) return fail(MTV_ERR_INVALID, "bad sizes");
    int Tm[MTV_HUBERT_MAX_CONV];
    if (f.max_samples < 1 || !hub_frames(f, f.max_samples, Tm)) return fail(MTV_ERR_INVALID, "max_samples is shorter than the conv encoder's receptive field");
    if ((double)f.max_batch * Tm[0] * f.conv_dim[0] >= 2147483648.0) return fail(MTV_ERR_INVALID, "max_batch x max_samples too large (row indices are 32-bit)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(MTV_ERR_HIP, "no HIP device available");
    std::unique_ptr<mtv_ctx> c(new mtv_ctx());
    c->cfg.max_batch = f.max_batch;
    int rc = ctx_init_common(c.get());
    if (rc != MTV_OK) return rc;
    auto st = std::make_shared<HubState>();
    HubState& S = *st;
    S.f = f;
    const int H = S.H = f.hidden, nl = S.nl = f.n_layers, nc = S.nc = f.n_conv, ffn = S.ff = f.intermediate, Cg = S.Cg = f.hidden / f.pos_groups;
    const int B = f.max_batch, Tt = Tm[nc - 1];
    bool ok = true;
    auto W = [&](const std::string& key, std::vector<int64_t> shape) { ok = ok && (S.w[key] = c->wcopy(key, std::move(shape))) != nullptr; };
    auto WB = [&](const std::string& pre, int n, int k) { W(pre + ".weight", {n, k}); W(pre + ".bias", {n}); };
    auto LN = [&](const std::string& pre, int n) { W(pre + ".weight", {n}); W(pre + ".bias", {n}); };
    auto BUF = [&](float*& p, const std::string& name, size_t n) { ok = ok && (p = c->buf(name, n)) != nullptr; };
    // transformers' HubertModel state_dict, in its order (masked_spec_embed is not read by an inference forward)
    S.Wc.assign(nc, nullptr);
    for (int i = 0; i < nc; ++i) {
        const std::string pre = "feature_extractor.conv_layers." + std::to_string(i);
        const int Ci = i ? f.conv_dim[i - 1] : 1;
        W(pre + ".conv.weight", {f.conv_dim[i], Ci, f.conv_kernel[i]});
        W(pre + ".conv.bias", {f.conv_dim[i]});
        LN(pre + ".layer_norm", f.conv_dim[i]);
        if (i) BUF(S.Wc[i], "h.Wc" + std::to_string(i), (size_t)f.conv_dim[i] * Ci * f.conv_kernel[i]);
    }
    LN("feature_projection.layer_norm", f.conv_dim[nc - 1]);
    WB("feature_projection.projection", H, f.conv_dim[nc - 1]);
    W("encoder.pos_conv_embed.conv.bias", {H});
    W("encoder.pos_conv_embed.conv.parametrizations.weight.original0", {1, 1, f.pos_taps});
    W("encoder.pos_conv_embed.conv.parametrizations.weight.original1", {H, Cg, f.pos_taps});
    LN("encoder.layer_norm", H);
    S.Wqkv.assign(nl, nullptr);
    S.bqkv.assign(nl, nullptr);
    for (int l = 0; ok && l < nl; ++l) {
        const std::string pre = "encoder.layers." + std::to_string(l);
        BUF(S.Wqkv[l], "h.Wqkv" + std::to_string(l), (size_t)3 * H * H);
        BUF(S.bqkv[l], "h.bqkv" + std::to_string(l), (size_t)3 * H);
        if (!ok) break;
        const char* names[3] = {"k_proj", "v_proj", "q_proj"};      // (state_dict order; the fused matrix is q | k | v)
        const int part[3] = {1, 2, 0};
        for (int i = 0; i < 3; ++i) {
            c->slot(pre + ".attention." + names[i] + ".weight", {H, H}, ROLE_COPY, S.Wqkv[l] + (size_t)part[i] * H * H, 0);
            c->slot(pre + ".attention." + names[i] + ".bias", {H}, ROLE_COPY, S.bqkv[l] + (size_t)part[i] * H, 0);
        }
        WB(pre + ".attention.out_proj", H, H);
        LN(pre + ".layer_norm", H);
        WB(pre + ".feed_forward.intermediate_dense", ffn, H);
        WB(pre + ".feed_forward.output_dense", H, ffn);
        LN(pre + ".final_layer_norm", H);
    }
    BUF(S.Wpos, "h.Wpos", (size_t)H * Cg * f.pos_taps);
    BUF(S.pscale, "h.pscale", (size_t)f.pos_taps);
    size_t fa = 0, fb = 0;      // conv layer i writes FA (i even) or FB (i odd)
    for (int i = 0; i < nc; ++i) {
        const size_t n = (size_t)B * Tm[i] * f.conv_dim[i];
        (i & 1 ? fb : fa) = std::max(i & 1 ? fb : fa, n);
    }
    BUF(S.FA, "h.FA", fa);
    BUF(S.FB, "h.FB", fb ? fb : 4);
    const size_t rows = (size_t)B * Tt;
    BUF(S.P, "h.P", rows * H);
    BUF(S.X, "h.X", rows * H);
    BUF(S.QKV, "h.QKV", rows * 3 * H);
    BUF(S.ATT, "h.ATT", rows * H);
    BUF(S.FFB, "h.FF", rows * ffn);
    BUF(S.tap_pos, "h.tap_pos", rows * H);
    BUF(S.tap_l0, "h.tap_l0", rows * H);
    float* part = nullptr;
    BUF(part, "h.part", (size_t)4 * HUB_PARTS);      // 2 x HUB_PARTS doubles
    if (!ok) return fail(MTV_ERR_HIP, "allocation failed");
    S.part = reinterpret_cast<double*>(part);
    c->kind = CTX_HUBERT;
    c->ext = st;
    *out = c.release();
    return MTV_OK;
}

int mtv_hubert_destroy(mtv_ctx* c) {
    if (c && c->kind != CTX_HUBERT) return fail(MTV_ERR_INVALID, "not a HuBERT context");
    delete c;
    return MTV_OK;
}

int mtv_hubert_normalize(mtv_ctx* c, const float* wave, int64_t n, float* out, void* stream) {
    HubState* S = hub_of(c);
    if (!S) return fail(MTV_ERR_INVALID, "not a HuBERT context");
    if (!wave || !out) return fail(MTV_ERR_INVALID, "null tensor pointer");
    if (n < 1) return fail(MTV_ERR_INVALID, "n must be at least 1");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_hub_norm_part, dim3(HUB_PARTS), dim3(256), 0, s, wave, (long long)n, (const double*)nullptr, S->part);
    hipLaunchKernelGGL(k_hub_norm_part, dim3(HUB_PARTS), dim3(256), 0, s, wave, (long long)n, (const double*)S->part, S->part + HUB_PARTS);
    const long long blocks = std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_hub_norm_apply, dim3((unsigned)blocks), dim3(256), 0, s, wave, (long long)n, (const double*)S->part, (const double*)(S->part + HUB_PARTS), out);
    HIPCHK(hipGetLastError());
    return MTV_OK;
}

int mtv_hubert_frames(const mtv_ctx* c, int n_samples) {
    HubState* S = hub_of(const_cast<mtv_ctx*>(c));
    if (!S) return fail(MTV_ERR_INVALID, "not a HuBERT context");
    int T[MTV_HUBERT_MAX_CONV];
    return n_samples >= 1 && hub_frames(S->f, n_samples, T) ? T[S->nc - 1] : 0;
}

int mtv_hubert_num_frames(int n_samples) {
    mtv_hubert_config f{};
    f.n_conv = 7;
    const int k[7] = {10, 3, 3, 3, 3, 2, 2}, st[7] = {5, 2, 2, 2, 2, 2, 2};
    for (int i = 0; i < 7; ++i) {
        f.conv_kernel[i] = k[i];
        f.conv_stride[i] = st[i];
    }
    int T[MTV_HUBERT_MAX_CONV];
    return n_samples >= 1 && hub_frames(f, n_samples, T) ? T[6] : 0;
}

int mtv_hubert_forward(mtv_ctx* c, const float* wave, int n_samples, int batch, float* out, void* stream) {
    HubState* S = hub_of(c);
    int T[MTV_HUBERT_MAX_CONV];
    int rc = hub_check(c, S, n_samples, batch, T);
    if (rc != MTV_OK) return rc;
    if (!wave || !out) return fail(MTV_ERR_INVALID, "null tensor pointer");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hub_prepare(c, *S));
    std::vector<Op> ops;
    hub_build(S, ops, wave, n_samples, batch, T, out);
    return run_op_list(ops, s);
}

int mtv_hubert_num_launches(mtv_ctx* c, int n_samples, int batch, int* n_out) {
    HubState* S = hub_of(c);
    if (!S || !n_out) return fail(MTV_ERR_INVALID, "not a HuBERT context / null argument");
    int T[MTV_HUBERT_MAX_CONV];
    if (batch < 1 || batch > S->f.max_batch || n_samples < 1 || n_samples > S->f.max_samples || !hub_frames(S->f, n_samples, T))
        return fail(MTV_ERR_INVALID, "no forward exists at this clip length / batch");
    *n_out = 2 * S->nc + 2 + 5 * S->nl + 1 + (S->keep ? 2 : 0);
    return MTV_OK;
}

int mtv_hubert_profile(mtv_ctx* c, const float* wave, int n_samples, int batch, int iters, mtv_op_time* out, int cap, int* n_out, void* stream) {
    HubState* S = hub_of(c);
    int T[MTV_HUBERT_MAX_CONV];
    int rc = hub_check(c, S, n_samples, batch, T);
    if (rc != MTV_OK) return rc;
    if (!wave || !n_out || iters < 1) return fail(MTV_ERR_INVALID, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hub_prepare(c, *S));
    std::vector<Op> ops;
    hub_build(S, ops, wave, n_samples, batch, T, S->tap_l0);      // (the result lands in a scratch tensor)
    return profile_ops(c, ops, iters, out, cap, n_out, s);
}

int mtv_hubert_debug_keep(mtv_ctx* c, int keep) {
    HubState* S = hub_of(c);
    if (!S) return fail(MTV_ERR_INVALID, "not a HuBERT context");
    S->keep = keep != 0;
    return MTV_OK;
}

int mtv_hubert_debug_tap(mtv_ctx* c, const char* name, float* dst, int64_t cap, int* rows_out, int* channels_out) {
    HubState* S = hub_of(c);
    if (!S || !name) return fail(MTV_ERR_INVALID, "not a HuBERT context / null argument");
    const std::string nm(name);
    const float* src = nullptr;
    int C = S->H;
    if (nm == "extract_features") {
        src = S->last_feat;
        C = S->f.conv_dim[S->nc - 1];
    } else if (nm == "after_pos_conv" || nm == "layer_0") {
        if (!S->keep) return fail(MTV_ERR_STATE, "tap '" + nm + "' needs mtv_hubert_debug_keep(ctx, 1) before the forward");
        src = nm == "layer_0" ? S->tap_l0 : S->tap_pos;
    } else {
        return fail(MTV_ERR_INVALID, "unknown tap: " + nm);
    }
    if (!src || S->last_rows < 1) return fail(MTV_ERR_STATE, "no forward has run yet");
    if (rows_out) *rows_out = S->last_rows;
    if (channels_out) *channels_out = C;
    if (dst) {
        if (cap < (int64_t)S->last_rows * C) return fail(MTV_ERR_INVALID, "tap destination too small");
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(dst, src, (size_t)S->last_rows * C * sizeof(float), hipMemcpyDefault));
    }
    return MTV_OK;
}

}  // extern "C"
