// AToM's MotionDecoder (AToM/model/model.py:242-470) and the eta=1 DDIM loop around it (AToM/model/diffusion.py:212-250) for gfx950.
//
// The audio-to-motion stage in front of MToV: HuBERT features [B, 2 L, cond_dim] + first-frame landmarks [B, L, 204] in, a landmark
// sequence [B, L, 204] out (L = 156 at full size), d_model 512, 8 FiLM decoder layers, 8 heads of 64.  A guided forward is two passes
// (unconditional, conditional) and a sample is 50 of those: ~100 forwards of ~8 GFLOP, every one a weight stream over a few hundred rows.
//
// What this file does differently from the reference, without changing its arithmetic:
//   * everything that does not depend on the timestep runs ONCE per call (atom_setup): cond_projection -> cond_encoder, face_projection ->
//     face_encoder, the mean pools and non_attn_*_projection, the `where` against the null embeddings, and the keys / values of every decoder
//     layer's two cross-attentions for all rows of `memory` / `face_memory` except the two time-token rows.  A step recomputes only the time
//     MLPs, the FiLM vectors, those two rows of keys / values, and the decoder stack.
//   * the guidance pair is ONE batch of 2 B clips (unconditional half first): every weight is streamed once per step.  The last launch of a
//     step (final_layer) multiplies both halves of a row tile and forms unc + (cond - unc) w, the clamp, pred_noise and the DDIM update in
//     its epilogue.
//   * a step is a plain chain of launches on one stream, captured once as a linear hipGraph.  The step's scalars live in a device record that
//     the FIRST launch of the chain (k_atom_advance, an ordinary one-thread kernel) copies from the step table: no in-launch hand-offs.
//   * the long sampler (diffusion.py:252-301: B half-overlapping windows as one batch) is the same chain: its per-step guidance weight comes
//     from a table k_atom_advance reads, its stitch x[b][w] <- x[b - 1][w + L / 2] is two stores of the DDIM epilogue.  The epilogue then must
//     not write the buffer it reads, so the sample has two buffers and even / odd steps are two graphs (x_io -> x_alt, x_alt -> x_io).
//
// Kernels: k_tok_linear (LayerNorm + rotary prologue, exact-f32 MFMA GEMM against [N][K] weights as the checkpoint stores them, bias /
// GELU / Mish / SiLU / FiLM / residual / guidance epilogues) and tok_attn.hip's k_tok_attn<512> (softmax attention of one head for 16
// queries, shared with hubert.hip; every key of a clip is in its one chunk).  Reference quirks that are behaviour are kept: see atom_build_step.
#include "plan_internal.h"
#include "tok_common.h"

namespace {
constexpr int ATT_KMAX = 512;      // keys per chunk of k_tok_attn here; create refuses more, so a workgroup sees one chunk (memory has 3 L + 2 keys: L <= 170)
constexpr int NFEAT = 204;         // 68 landmarks x 3 (model.py:402-410 hard-wires the 17 | 31 | 20 split)

enum { EPI_PLAIN = 0, EPI_RES = 1, EPI_FILM_RES = 2, EPI_FILM_SELF = 3, EPI_GUIDE = 4 };

struct AtomCur {                   // device record the guided final_layer epilogue reads (graph kernel arguments are frozen, this is not)
    DdimStep st;
    float gw;                      // guidance weight
    int ddim;                      // 0: write the guided output; 1: apply the DDIM update to x_io
    const float* noise;            // [n][B][L][204] in-loop draws
    long long n_per_draw;
};

struct TokLinArgs {
    const float* A;                // input rows, lda floats apart
    const float* A2;               // optional second addend (same addressing): norm3(face + lip)
    int lda;
    int M, K, N;                   // logical rows, reduction length (multiple of 4), output columns (multiple of 4)
    // logical row r: clip b = r / (L S), w = r % (L S), token position pos0 + w / S.  Input row = b in_bs + in_r0 + w, output row likewise.
    int L, S;
    int in_bs, in_r0, out_bs, out_r0;
    const float* W;                // [N][ldw]
    int ldw;
    const float* bias;             // [N]
    const float *ln_g, *ln_b;      // LayerNorm of the row over K (nullptr: none)
    const float* rot;              // [pos][K / 2][cos, sin] or nullptr; output columns < rot_cols multiply the rotated row
    int rot_cols, pos0;
    int act_in;                    // ACT_MISH: Mish on the input (DenseFiLM)
    int act;
    int epi;
    const float* res;              // residual, addressed like the output
    int ldres;
    const float* film;             // per clip: scale at [n], shift at [N + n]
    int film_bs;
    float* out;
    int ldo;
    int half_rows;                 // EPI_GUIDE: input row of the conditional half = row + half_rows
    const AtomCur* cur;
    float* x_io;                   // EPI_GUIDE with cur->ddim: the sample x_t, [M][N]
    float* x_out;                  // ... and where the updated sample goes: x_io itself (ddim_sample), the other buffer of the pair (long sampler)
    int stitch_L;                  // long sampler: clip length L (even); 0: no stitch
};

// 32 rows x 32 columns per workgroup; the four waves take the 16-wide K chunks round robin and meet in LDS (fixed order: results do not
// depend on the grid).  Lane (j, q) of a wave loads A[row j][16 c + 4 q ..+3] and W[col j][16 c + 4 q ..+3] as one 16-byte load each; the
// four MFMA steps of a chunk pair element i of both, so the K order inside a chunk is a permutation shared by A and B.
// (not hubert.hip's k_hub_gemm, where every wave walks all of K: the bits and the tile shapes differ by design)
template <int HALVES>
__global__ __launch_bounds__(256) void k_tok_linear(const TokLinArgs a) {
    __shared__ float s_stat[HALVES][32][2];
    __shared__ float s_red[4][HALVES][32][33];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const int LS = a.L * a.S;
    auto in_row = [&](int r) {
        const int b = r / LS, w = r - b * LS;
        return (size_t)(b * a.in_bs + a.in_r0 + w);
    };
    if (a.ln_g) {
        for (int i = wave; i < 32 * HALVES; i += 4) {
            const int h = i >> 5, rr = i & 31, r = m0 + rr;
            float mean = 0.0f, rstd = 0.0f;
            if (r < a.M) {
                const size_t ro = (in_row(r) + (size_t)h * a.half_rows) * a.lda;
                ln_row_stats(a.A, a.A2, ro, a.K, 1e-5f, lane, &mean, &rstd);
            }
            if (lane == 0) {
                s_stat[h][rr][0] = mean;
                s_stat[h][rr][1] = rstd;
            }
        }
        __syncthreads();
    }
    const int j = lane & 15, q = lane >> 4;
    const bool rot = a.rot != nullptr && n0 < a.rot_cols;
    size_t aoff[HALVES][2];
    float mean[HALVES][2], rstd[HALVES][2];
    const float* rotp[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int r = min(m0 + rb * 16 + j, a.M - 1);       // (rows past M repeat the last row; they are not stored)
        const int b = r / LS, w = r - b * LS;
        rotp[rb] = rot ? a.rot + (size_t)(a.pos0 + w / a.S) * a.K : nullptr;
#pragma unroll
        for (int h = 0; h < HALVES; ++h) {
            aoff[h][rb] = (in_row(r) + (size_t)h * a.half_rows) * a.lda;
            mean[h][rb] = a.ln_g ? s_stat[h][min(rb * 16 + j, a.M - 1 - m0)][0] : 0.0f;
            rstd[h][rb] = a.ln_g ? s_stat[h][min(rb * 16 + j, a.M - 1 - m0)][1] : 1.0f;
        }
    }
    size_t woff[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) woff[cb] = (size_t)min(n0 + cb * 16 + j, a.N - 1) * a.ldw;
    f32x4 acc[HALVES][2][2];
#pragma unroll
    for (int h = 0; h < HALVES; ++h)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[h][rb][cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int nch = (a.K + 15) >> 4;
    for (int c = wave; c < nch; c += 4) {
        const int k = 16 * c + 4 * q;
        // K is a multiple of 4: a lane's quad is inside or outside as a whole.  A quad past K (the last chunk of K = 204) multiplies zero weights:
        // every lane of the wave reaches the MFMAs, none branches around them.
        const bool kin = k < a.K;
        const f32x4 zero4{0.0f, 0.0f, 0.0f, 0.0f};
        f32x4 bw[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) bw[cb] = kin ? *reinterpret_cast<const f32x4*>(a.W + woff[cb] + k) : zero4;
        f32x4 g{1.0f, 1.0f, 1.0f, 1.0f}, be{0.0f, 0.0f, 0.0f, 0.0f};
        if (a.ln_g && kin) {
            g = *reinterpret_cast<const f32x4*>(a.ln_g + k);
            be = *reinterpret_cast<const f32x4*>(a.ln_b + k);
        }
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            f32x4 cs{1.0f, 0.0f, 1.0f, 0.0f};
            if (rot && kin) cs = *reinterpret_cast<const f32x4*>(rotp[rb] + k);      // (cos, sin) of pairs k / 2 and k / 2 + 1
#pragma unroll
            for (int h = 0; h < HALVES; ++h) {
                f32x4 x = kin ? *reinterpret_cast<const f32x4*>(a.A + aoff[h][rb] + k) : zero4;
                if (a.A2 && kin) x += *reinterpret_cast<const f32x4*>(a.A2 + aoff[h][rb] + k);
                if (a.ln_g) x = (x - mean[h][rb]) * rstd[h][rb] * g + be;
                if (a.act_in) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) x[i] = act_apply(x[i], a.act_in);
                }
                if (rot) {      // interleaved pairs: (x0, x1) -> (x0 cos - x1 sin, x1 cos + x0 sin)   (rotary_embedding_torch.py:39-59)
                    const f32x4 y = x;
                    x[0] = y[0] * cs[0] - y[1] * cs[1];
                    x[1] = y[1] * cs[0] + y[0] * cs[1];
                    x[2] = y[2] * cs[2] - y[3] * cs[3];
                    x[3] = y[3] * cs[2] + y[2] * cs[3];
                }
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[h][rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[i], bw[cb][i], acc[h][rb][cb], 0, 0, 0);
            }
        }
    }
    // C/D map of the 16x16 forms: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int h = 0; h < HALVES; ++h)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int i = 0; i < 4; ++i) s_red[wave][h][rb * 16 + q * 4 + i][cb * 16 + j] = acc[h][rb][cb][i];
    __syncthreads();
    const int rr = tid >> 3, c0 = (tid & 7) * 4, r = m0 + rr, n = n0 + c0;
    if (r >= a.M || n >= a.N) return;
    f32x4 y[HALVES];
#pragma unroll
    for (int h = 0; h < HALVES; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s = ((s_red[0][h][rr][c0 + i] + s_red[1][h][rr][c0 + i]) + s_red[2][h][rr][c0 + i]) + s_red[3][h][rr][c0 + i];
            y[h][i] = act_apply(s + a.bias[n + i], a.act);
        }
    const int b = r / LS, w = r - b * LS;
    const size_t orow = (size_t)(b * a.out_bs + a.out_r0 + w);
    f32x4 o = y[0];
    if (a.epi == EPI_RES) {
        o += *reinterpret_cast<const f32x4*>(a.res + orow * a.ldres + n);
    } else if (a.epi == EPI_FILM_RES || a.epi == EPI_FILM_SELF) {      // featurewise_affine (model.py:30-32): (scale + 1) y + shift
        const f32x4 sc = *reinterpret_cast<const f32x4*>(a.film + (size_t)b * a.film_bs + n);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(a.film + (size_t)b * a.film_bs + a.N + n);
        const f32x4 base = a.epi == EPI_FILM_SELF ? y[0] : *reinterpret_cast<const f32x4*>(a.res + orow * a.ldres + n);
        o = base + ((sc + 1.0f) * y[0] + sh);
    } else if (a.epi == EPI_GUIDE) {
        if constexpr (HALVES == 2) {
            const AtomCur cu = *a.cur;
            o = y[0] + (y[1] - y[0]) * cu.gw;                // model.py:385-389
            if (cu.ddim) {                                   // diffusion.py:131-140, 235-249
                const size_t idx = (size_t)r * a.N + n;
                const f32x4 xt = *reinterpret_cast<const f32x4*>(a.x_io + idx);
                f32x4 nz{0.0f, 0.0f, 0.0f, 0.0f};
                if (!cu.st.last) nz = *reinterpret_cast<const f32x4*>(cu.noise + (size_t)cu.st.noise_index * cu.n_per_draw + idx);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float x0 = fminf(fmaxf(o[i], -1.0f), 1.0f);
                    const float pn = __fdiv_rn(__fsub_rn(__fmul_rn(cu.st.sqrt_recip_ac, xt[i]), x0), cu.st.sqrt_recipm1_ac);
                    o[i] = cu.st.last ? x0
                                      : __fadd_rn(__fadd_rn(__fmul_rn(x0, cu.st.sqrt_ac_next), __fmul_rn(cu.st.c, pn)), __fmul_rn(cu.st.sigma, nz[i]));
                }
                // long_ddim_sample's stitch (diffusion.py:299-300) after every non-final step: x[b][w] <- x[b - 1][w + L / 2] for b >= 1, w < L / 2.
                // The row r + L / 2 IS (b + 1, w - L / 2): the owner of a second-half row stores it twice, the owner of a first-half row of a later
                // window stores nothing.  x_out is not x_io there, so no workgroup reads what another one writes in this launch.
                const int half = a.stitch_L >> 1;
                const bool stitch = a.stitch_L != 0 && !cu.st.last;
                const int w = stitch ? r % a.stitch_L : 0;
                if (!stitch || r < a.stitch_L || w >= half) *reinterpret_cast<f32x4*>(a.x_out + idx) = o;
                if (stitch && w >= half && r + half < a.M) *reinterpret_cast<f32x4*>(a.x_out + idx + (size_t)half * a.N) = o;
                return;
            }
        }
    }
    *reinterpret_cast<f32x4*>(a.out + orow * a.ldo + n) = o;
}

hipError_t launch_tok_linear(const TokLinArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.N + 31) / 32), (unsigned)((a.M + 31) / 32));
    if (a.epi == EPI_GUIDE) hipLaunchKernelGGL(k_tok_linear<2>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_tok_linear<1>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- small element-wise kernels
// SinusoidalPosEmb (utils.py:36-48): [sin(t f_i) | cos(t f_i)], f from the host's table
__global__ void k_atom_time_sin(const float* tv, const float* freqs, float* out, int nb, int half) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * half) return;
    const int b = i / half, f = i - b * half;
    const float ang = tv[b] * freqs[f];
    out[(size_t)b * 2 * half + f] = sinf(ang);
    out[(size_t)b * 2 * half + half + f] = cosf(ang);
}
__global__ void k_atom_times(const int64_t* t, float* tv, int nb, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb) tv[i] = (float)t[i % B];
}
// first launch of a sampler step: the step's scalars -> the record the final epilogue reads, its timestep -> every clip, counter + 1.
// gws (long sampler, else nullptr: the weight atom_write_cur wrote stays): the step's guidance weight from the table beside the steps.
__global__ void k_atom_advance(const DdimStep* steps, const float* gws, int* counter, AtomCur* cur, float* tv, int nb) {
    if (blockIdx.x || threadIdx.x) return;
    const int i = *counter;
    const DdimStep st = steps[i];
    cur->st = st;
    if (gws) cur->gw = gws[i];
    for (int b = 0; b < nb; ++b) tv[b] = (float)st.t;
    *counter = i + 1;
}
__global__ void k_atom_mean(const float* src, float* dst, int nb, int T, int D) {      // mean over the T tokens of a clip
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * D) return;
    const int b = i / D, c = i - b * D;
    float s = 0.0f;
    for (int t = 0; t < T; ++t) s += src[((size_t)b * T + t) * D + c];
    dst[i] = s / (float)T;
}
__global__ void k_atom_hid(const float* fh, const float* ch, float* out, int n) {      // the three in-place adds of model.py:454-460
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (fh[i] + fh[i]) + ch[i];
}
// input_projection_lip on cat(landmarks 0:17, 48:68) and input_projection_wo_lip on 17:48 (model.py:402-417) as ONE [2 D][204] matrix
// on the unsplit row: lip rows take columns 0..50 and 144..203, upper-face rows columns 51..143, the rest stays zero.
__global__ void k_atom_win(const float* wl, const float* wu, float* w, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D * NFEAT) return;
    const int n = i / NFEAT, c = i - n * NFEAT;
    w[(size_t)n * NFEAT + c] = c < 51 ? wl[n * 111 + c] : (c >= 144 ? wl[n * 111 + c - 93] : 0.0f);
    w[(size_t)(D + n) * NFEAT + c] = (c >= 51 && c < 144) ? wu[n * 93 + c - 51] : 0.0f;
}

// =====================================================================================================================================
struct AtomState {
    mtv_atom_config f;
    int D, L, Lm, Lf, nl, nbmax;
    std::map<std::string, float*> w;            // parameter name -> device copy (the checkpoint's own layout)
    float *Wfilm, *bfilm, *Win, *bin, *rot, *tfreq;
    bool tables = false;
    float *x_io, *x_alt, *X, *QKV, *ATT, *XT, *OUT;      // x_alt: the long sampler's second sample buffer (steps alternate x_io -> x_alt -> x_io)
    float *CT, *FT, *EQKV, *EATT, *EFF, *Cmem, *Cface, *pool, *hid1, *fh, *ch, *hid_add;
    float *tv, *tsin, *th, *tvec, *ttok, *film;
    std::vector<float*> KVm, KVf;
    AtomCur* cur;
    DdimStep* steps;
    float* gws;                                 // [steps_cap] per-step guidance weights of the long sampler, behind the step records
    int steps_cap;
    int* counter;
    float gw = 1.0f;
    AtomCur h_cur{};                            // host copies of what goes up asynchronously (they outlive the call)
    std::vector<DdimStep> h_steps;
    std::vector<float> h_gws;
};
AtomState* atom_of(mtv_ctx* c) { return c && c->kind == CTX_ATOM ? static_cast<AtomState*>(c->ext.get()) : nullptr; }

TokLinArgs lin(const float* A, int lda, int M, int K, const float* W, const float* bias, int N, float* out, int ldo) {
    TokLinArgs a{};
    a.A = A;
    a.lda = lda;
    a.M = M;
    a.K = K;
    a.N = N;
    a.L = M;
    a.S = 1;
    a.in_bs = a.out_bs = M;
    a.W = W;
    a.ldw = K;
    a.bias = bias;
    a.out = out;
    a.ldo = ldo;
    return a;
}
void per_clip(TokLinArgs& a, int L, int S) {
    a.L = L;
    a.S = S;
    a.in_bs = a.out_bs = L * S;
}
void with_ln(TokLinArgs& a, AtomState& A, const std::string& pre) {
    a.ln_g = A.w.at(pre + ".weight");
    a.ln_b = A.w.at(pre + ".bias");
}
void with_rot(TokLinArgs& a, AtomState& A, int cols, int pos0 = 0) {
    a.rot = A.rot;
    a.rot_cols = cols;
    a.pos0 = pos0;
}

// TransformerEncoderLayer (model.py:35-99, norm_first): x += sa(norm1 x); x += linear2(gelu(linear1(norm2 x))).  q and k see the rotated
// normalised row, v the unrotated one (model.py:84-94).
#define ACHK(expr)                         \
    do {                                   \
        hipError_t e_ = (expr);            \
        if (e_ != hipSuccess) return e_;   \
    } while (0)
hipError_t encoder_layer(AtomState& A, const std::string& pre, float* x, int nb, int T, hipStream_t s) {
    const int D = A.D, ff = A.f.ff_size, M = nb * T;
    TokLinArgs a = lin(x, D, M, D, A.w.at(pre + ".self_attn.in_proj_weight"), A.w.at(pre + ".self_attn.in_proj_bias"), 3 * D, A.EQKV, 3 * D);
    per_clip(a, T, 1);
    with_ln(a, A, pre + ".norm1");
    with_rot(a, A, 2 * D);
    ACHK(launch_tok_linear(a, s));
    TokAttnArgs t{};
    t.q = A.EQKV;
    t.k = A.EQKV + D;
    t.v = A.EQKV + 2 * D;
    t.o = A.EATT;
    t.q_bs = t.k_bs = (long long)T * 3 * D;
    t.q_rs = t.k_rs = 3 * D;
    t.o_bs = (long long)T * D;
    t.o_rs = D;
    t.Lq = t.Lk = T;
    t.H = A.f.num_heads;
    t.d = D / A.f.num_heads;
    t.S = 1;
    t.scale = 1.0f / std::sqrt((float)t.d);
    ACHK(launch_tok_attn(t, nb, ATT_KMAX, s));
    a = lin(A.EATT, D, M, D, A.w.at(pre + ".self_attn.out_proj.weight"), A.w.at(pre + ".self_attn.out_proj.bias"), D, x, D);
    a.epi = EPI_RES;
    a.res = x;
    a.ldres = D;
    ACHK(launch_tok_linear(a, s));
    a = lin(x, D, M, D, A.w.at(pre + ".linear1.weight"), A.w.at(pre + ".linear1.bias"), ff, A.EFF, ff);
    with_ln(a, A, pre + ".norm2");
    a.act = ACT_GELU;
    ACHK(launch_tok_linear(a, s));
    a = lin(A.EFF, ff, M, ff, A.w.at(pre + ".linear2.weight"), A.w.at(pre + ".linear2.bias"), D, x, D);
    a.epi = EPI_RES;
    a.res = x;
    a.ldres = D;
    return launch_tok_linear(a, s);
}

// non_attn_*_projection (model.py:348-359): LayerNorm, Linear, SiLU, Linear on nb pooled rows
hipError_t hidden_mlp(AtomState& A, const std::string& pre, const float* in, float* out, int nb, hipStream_t s) {
    const int D = A.D;
    TokLinArgs a = lin(in, D, nb, D, A.w.at(pre + ".1.weight"), A.w.at(pre + ".1.bias"), D, A.hid1, D);
    with_ln(a, A, pre + ".0");
    a.act = ACT_SILU;
    ACHK(launch_tok_linear(a, s));
    a = lin(A.hid1, D, nb, D, A.w.at(pre + ".3.weight"), A.w.at(pre + ".3.bias"), D, out, D);
    return launch_tok_linear(a, s);
}

enum { DROP_NONE = 0, DROP_ALL = 1, DROP_PAIR = 2 };      // cond_drop_prob 0 | 1 | the guidance pair (null half first, then the kept half)

// Everything of MotionDecoder.forward that does not depend on the timestep (model.py:419-466 minus the time rows), for nb = B or 2 B
// effective clips: clips [0, nnull) carry the null embeddings, clips [kb0, kb0 + B) the encoded conditions.
hipError_t atom_setup(AtomState& A, int B, int mode, const float* face, const float* cond, hipStream_t s) {
    const int D = A.D, L = A.L, Lm = A.Lm, Lf = A.Lf;
    const int nb = mode == DROP_PAIR ? 2 * B : B, nnull = mode == DROP_NONE ? 0 : B, kb0 = mode == DROP_PAIR ? B : 0, nkeep = mode == DROP_ALL ? 0 : B;
    hipLaunchKernelGGL(k_atom_win, dim3((unsigned)((D * NFEAT + 255) / 256)), dim3(256), 0, s, A.w.at("input_projection_lip.weight"),
                       A.w.at("input_projection_wo_lip.weight"), A.Win, D);
    ACHK(hipGetLastError());
    float* ct = A.CT + (size_t)kb0 * 2 * L * D;
    float* ft = A.FT + (size_t)kb0 * L * D;
    if (nkeep) {
        TokLinArgs a = lin(cond, A.f.cond_feature_dim, B * 2 * L, A.f.cond_feature_dim, A.w.at("cond_projection.weight"), A.w.at("cond_projection.bias"), D, ct, D);
        ACHK(launch_tok_linear(a, s));
        for (int i = 0; i < 2; ++i) ACHK(encoder_layer(A, "cond_encoder." + std::to_string(i), ct, B, 2 * L, s));
        a = lin(face, NFEAT, B * L, NFEAT, A.w.at("face_projection.weight"), A.w.at("face_projection.bias"), D, ft, D);
        ACHK(launch_tok_linear(a, s));
        for (int i = 0; i < 2; ++i) ACHK(encoder_layer(A, "face_encoder." + std::to_string(i), ft, B, L, s));
        hipLaunchKernelGGL(k_atom_mean, dim3((unsigned)((B * D + 255) / 256)), dim3(256), 0, s, ct, A.pool, B, 2 * L, D);
        ACHK(hipGetLastError());
        ACHK(hidden_mlp(A, "non_attn_cond_projection", A.pool, A.ch + (size_t)kb0 * D, B, s));
    }
    if (nnull) {      // torch.where(keep_mask, tokens, null) with an all-false mask (model.py:429-430, 448-449, 458-459)
        ACHK(launch_tok_copy(A.w.at("null_cond_embed"), 0, A.CT, (long long)2 * L * D, (long long)2 * L * D, nnull, s));
        ACHK(launch_tok_copy(A.w.at("face_null_cond_embed"), 0, A.FT, (long long)L * D, (long long)L * D, nnull, s));
        ACHK(launch_tok_copy(A.w.at("null_cond_hidden"), 0, A.ch, D, D, nnull, s));
    }
    hipLaunchKernelGGL(k_atom_mean, dim3((unsigned)((nb * D + 255) / 256)), dim3(256), 0, s, A.FT, A.pool, nb, L, D);
    ACHK(hipGetLastError());
    ACHK(hidden_mlp(A, "non_attn_face_projection", A.pool, A.fh, nb, s));
    hipLaunchKernelGGL(k_atom_hid, dim3((unsigned)((nb * D + 255) / 256)), dim3(256), 0, s, A.fh, A.ch, A.hid_add, nb * D);
    ACHK(hipGetLastError());
    // c = cat(cond_tokens, t_tokens, face_tokens), face_wo_lip_c = cat(t_tokens, face_tokens) (model.py:461-466); the time rows stay zero here
    ACHK(launch_tok_copy(A.CT, (long long)2 * L * D, A.Cmem, (long long)Lm * D, (long long)2 * L * D, nb, s));
    ACHK(launch_tok_copy(A.FT, (long long)L * D, A.Cmem + (size_t)(2 * L + 2) * D, (long long)Lm * D, (long long)L * D, nb, s));
    ACHK(launch_tok_copy(A.FT, (long long)L * D, A.Cface + (size_t)2 * D, (long long)Lf * D, (long long)L * D, nb, s));
    for (int l = 0; l < A.nl; ++l) {      // keys (rotated norm_cond row) | values (unrotated) of both cross-attentions (model.py:212-223)
        const std::string pre = "seqTransDecoder.stack." + std::to_string(l) + ".multihead_attn.";
        const float *W = A.w.at(pre + "in_proj_weight") + (size_t)D * D, *bias = A.w.at(pre + "in_proj_bias") + D;
        TokLinArgs a = lin(A.Cmem, D, nb * Lm, D, W, bias, 2 * D, A.KVm[l], 2 * D);
        per_clip(a, Lm, 1);
        with_ln(a, A, "norm_cond");
        with_rot(a, A, D);
        ACHK(launch_tok_linear(a, s));
        a = lin(A.Cface, D, nb * Lf, D, W, bias, 2 * D, A.KVf[l], 2 * D);
        per_clip(a, Lf, 1);
        with_ln(a, A, "norm_cond");
        with_rot(a, A, D);
        ACHK(launch_tok_linear(a, s));
    }
    return hipSuccess;
}

// The launch chain of one forward / one sampler step for nb effective clips (guided: nb = 2 B, the halves meet in final_layer).
//   x_src [B][L][204]: the landmarks (the sampler: the sample x_t).  x_out (sampler): where the DDIM update goes -- nullptr: x_src, in
//   place; with `stitch` (the long sampler) the other buffer of the pair.  Reference behaviour kept as is:
//   - lip_t, nonlip_t and t are ONE tensor (model.py:441-460): every FiLM sees t0 + 2 face_hidden + cond_hidden, film3's mean of the two is that vector;
//   - the norm_first decoder layer never runs linear1 / linear2; it ends x_tmp + affine(x_tmp, film3) -> linear3 (model.py:161-183);
//   - norm1 + self_attn serve both streams; norm2 + self_attn the face stream, norm2 + multihead_attn on memory the lip stream;
//     norm3 + multihead_attn again on face_memory for the sum.
void atom_build_step(AtomState* Ap, Plan* p, int B, bool guided, bool sampler, float* x_src, float* x_out = nullptr, bool stitch = false) {
    AtomState& A = *Ap;
    const int D = A.D, L = A.L, Lm = A.Lm, Lf = A.Lf, H = A.f.num_heads, d = D / H;
    const int nb = guided ? 2 * B : B, M = nb * L;
    auto add = [&](const std::string& name, std::function<hipError_t(hipStream_t)> fn) { p->ops.push_back(Op{std::move(fn), name}); };
    auto add_lin = [&](const std::string& name, const TokLinArgs& a) { add(name, [a](hipStream_t s) { return launch_tok_linear(a, s); }); };
    auto add_att = [&](const std::string& name, const TokAttnArgs& t, int n) { add(name, [t, n](hipStream_t s) { return launch_tok_attn(t, n, ATT_KMAX, s); }); };
    if (sampler)
        add("advance", [Ap, nb, stitch](hipStream_t s) {
            hipLaunchKernelGGL(k_atom_advance, dim3(1), dim3(64), 0, s, Ap->steps, stitch ? Ap->gws : (const float*)nullptr, Ap->counter, Ap->cur, Ap->tv, nb);
            return hipGetLastError();
        });
    add("time_sin", [Ap, nb, D](hipStream_t s) {
        hipLaunchKernelGGL(k_atom_time_sin, dim3((unsigned)((nb * D / 2 + 255) / 256)), dim3(256), 0, s, Ap->tv, Ap->tfreq, Ap->tsin, nb, D / 2);
        return hipGetLastError();
    });
    TokLinArgs a = lin(A.tsin, D, nb, D, A.w.at("time_mlp.1.weight"), A.w.at("time_mlp.1.bias"), 4 * D, A.th, 4 * D);
    a.act = ACT_MISH;
    add_lin("time_mlp", a);
    a = lin(A.th, 4 * D, nb, 4 * D, A.w.at("to_time_cond.0.weight"), A.w.at("to_time_cond.0.bias"), D, A.tvec, D);
    a.epi = EPI_RES;
    a.res = A.hid_add;
    a.ldres = D;
    add_lin("to_time_cond", a);
    a = lin(A.th, 4 * D, nb, 4 * D, A.w.at("to_time_tokens.0.weight"), A.w.at("to_time_tokens.0.bias"), 2 * D, A.ttok, 2 * D);
    add_lin("to_time_tokens", a);
    a = lin(A.tvec, D, nb, D, A.Wfilm, A.bfilm, A.nl * 6 * D, A.film, A.nl * 6 * D);      // DenseFiLM of all layers: Mish -> Linear (model.py:15-27)
    a.act_in = ACT_MISH;
    add_lin("film", a);
    for (int h = 0; h < nb / B; ++h) {      // both halves of the pair see the same landmarks
        a = lin(x_src, NFEAT, B * L, NFEAT, A.Win, A.bin, 2 * D, A.X + (size_t)h * B * L * 2 * D, 2 * D);
        add_lin("input_projection", a);
    }
    const int fbs = A.nl * 6 * D;
    for (int l = 0; l < A.nl; ++l) {
        const std::string pre = "seqTransDecoder.stack." + std::to_string(l) + ".", tag = "L" + std::to_string(l) + ".";
        const float *Wsa = A.w.at(pre + "self_attn.in_proj_weight"), *bsa = A.w.at(pre + "self_attn.in_proj_bias");
        const float *Wso = A.w.at(pre + "self_attn.out_proj.weight"), *bso = A.w.at(pre + "self_attn.out_proj.bias");
        const float *Wca = A.w.at(pre + "multihead_attn.in_proj_weight"), *bca = A.w.at(pre + "multihead_attn.in_proj_bias");
        const float *Wco = A.w.at(pre + "multihead_attn.out_proj.weight"), *bco = A.w.at(pre + "multihead_attn.out_proj.bias");
        const float* film = A.film + (size_t)l * 6 * D;
        // keys / values of the two time-token rows: rows 2 L, 2 L + 1 of memory, rows 0, 1 of face_memory
        for (int fm = 0; fm < 2; ++fm) {
            a = lin(A.ttok, D, nb * 2, D, Wca + (size_t)D * D, bca + D, 2 * D, fm ? A.KVf[l] : A.KVm[l], 2 * D);
            per_clip(a, 2, 1);
            a.out_bs = fm ? Lf : Lm;
            a.out_r0 = fm ? 0 : 2 * L;
            with_ln(a, A, "norm_cond");
            with_rot(a, A, D, fm ? 0 : 2 * L);
            add_lin(tag + (fm ? "time_kv_face" : "time_kv_mem"), a);
        }
        // ---- stage 1: self_attn(norm1) on both streams; X is [clip][token][lip | face][D]
        a = lin(A.X, D, M * 2, D, Wsa, bsa, 3 * D, A.QKV, 3 * D);
        per_clip(a, L, 2);
        with_ln(a, A, pre + "norm1");
        with_rot(a, A, 2 * D);
        add_lin(tag + "qkv1", a);
        TokAttnArgs t{};
        t.q = A.QKV;
        t.k = A.QKV + D;
        t.v = A.QKV + 2 * D;
        t.o = A.ATT;
        t.q_bs = t.k_bs = (long long)L * 6 * D;
        t.q_rs = t.k_rs = 6 * D;
        t.q_ss = t.k_ss = 3 * D;
        t.o_bs = (long long)L * 2 * D;
        t.o_rs = 2 * D;
        t.o_ss = D;
        t.Lq = t.Lk = L;
        t.H = H;
        t.d = d;
        t.S = 2;
        t.scale = 1.0f / std::sqrt((float)d);
        add_att(tag + "attn1", t, nb);
        a = lin(A.ATT, D, M * 2, D, Wso, bso, D, A.X, D);
        per_clip(a, L, 2);
        a.epi = EPI_FILM_RES;
        a.film = film;
        a.film_bs = fbs;
        a.res = A.X;
        a.ldres = D;
        add_lin(tag + "out1", a);
        // ---- stage 2: face = self_attn(norm2 face); lip = multihead_attn(norm2 lip, memory)
        a = lin(A.X + D, 2 * D, M, D, Wsa, bsa, 3 * D, A.QKV, 3 * D);
        per_clip(a, L, 1);
        with_ln(a, A, pre + "norm2");
        with_rot(a, A, 2 * D);
        add_lin(tag + "qkv2_face", a);
        float* Q = A.QKV + (size_t)M * 3 * D;
        a = lin(A.X, 2 * D, M, D, Wca, bca, D, Q, D);
        per_clip(a, L, 1);
        with_ln(a, A, pre + "norm2");
        with_rot(a, A, D);
        add_lin(tag + "q2_lip", a);
        t = TokAttnArgs{};
        t.q = A.QKV;
        t.k = A.QKV + D;
        t.v = A.QKV + 2 * D;
        t.o = A.ATT;
        t.q_bs = t.k_bs = (long long)L * 3 * D;
        t.q_rs = t.k_rs = 3 * D;
        t.o_bs = (long long)L * D;
        t.o_rs = D;
        t.Lq = t.Lk = L;
        t.H = H;
        t.d = d;
        t.S = 1;
        t.scale = 1.0f / std::sqrt((float)d);
        add_att(tag + "attn2_face", t, nb);
        TokAttnArgs u = t;
        u.q = Q;
        u.q_bs = (long long)L * D;
        u.q_rs = D;
        u.k = A.KVm[l];
        u.v = A.KVm[l] + D;
        u.k_bs = (long long)Lm * 2 * D;
        u.k_rs = 2 * D;
        u.Lk = Lm;
        u.o = A.ATT + (size_t)M * D;
        add_att(tag + "attn2_lip", u, nb);
        a = lin(A.ATT, D, M, D, Wso, bso, D, A.X + D, 2 * D);
        per_clip(a, L, 1);
        a.epi = EPI_FILM_RES;
        a.film = film + 2 * D;
        a.film_bs = fbs;
        a.res = A.X + D;
        a.ldres = 2 * D;
        add_lin(tag + "out2_face", a);
        a = lin(A.ATT + (size_t)M * D, D, M, D, Wco, bco, D, A.X, 2 * D);
        per_clip(a, L, 1);
        a.epi = EPI_FILM_RES;
        a.film = film + 2 * D;
        a.film_bs = fbs;
        a.res = A.X;
        a.ldres = 2 * D;
        add_lin(tag + "out2_lip", a);
        // ---- stage 3: x_tmp = multihead_attn(norm3(face + lip), face_memory); x_tmp += affine(x_tmp, film3); linear3
        a = lin(A.X, 2 * D, M, D, Wca, bca, D, Q, D);
        a.A2 = A.X + D;
        per_clip(a, L, 1);
        with_ln(a, A, pre + "norm3");
        with_rot(a, A, D);
        add_lin(tag + "q3", a);
        u.k = A.KVf[l];
        u.v = A.KVf[l] + D;
        u.k_bs = (long long)Lf * 2 * D;
        u.Lk = Lf;
        u.o = A.ATT;
        add_att(tag + "attn3", u, nb);
        a = lin(A.ATT, D, M, D, Wco, bco, D, A.XT, D);
        per_clip(a, L, 1);
        a.epi = EPI_FILM_SELF;
        a.film = film + 4 * D;
        a.film_bs = fbs;
        add_lin(tag + "out3", a);
        a = lin(A.XT, D, M, D, A.w.at(pre + "linear3.weight"), A.w.at(pre + "linear3.bias"), 2 * D, A.X, 2 * D);
        add_lin(tag + "linear3", a);
    }
    a = lin(A.X, 2 * D, guided ? B * L : M, 2 * D, A.w.at("final_layer.weight"), A.w.at("final_layer.bias"), NFEAT, A.OUT, NFEAT);
    if (guided) {
        a.epi = EPI_GUIDE;
        a.half_rows = B * L;
        a.cur = A.cur;
        a.x_io = sampler ? x_src : A.x_io;
        a.x_out = sampler && x_out ? x_out : a.x_io;
        a.stitch_L = stitch ? L : 0;
    }
    add_lin("final_layer", a);
}

// ATOM_LONG0 / ATOM_LONG1: a step of the long sampler reading x_io and writing x_alt / the reverse (even / odd steps of a call)
enum { ATOM_FORWARD = 0, ATOM_GUIDED = 1, ATOM_STEP = 2, ATOM_LONG0 = 3, ATOM_LONG1 = 4 };
int atom_plan(mtv_ctx* c, AtomState* A, int B, int mode, Plan** out) {
    auto it = c->plans.find({B, mode});
    if (it == c->plans.end()) {
        std::unique_ptr<Plan> p(new Plan());
        p->B = B;
        p->mode = mode;
        if (mode == ATOM_LONG0 || mode == ATOM_LONG1)
            atom_build_step(A, p.get(), B, true, true, mode == ATOM_LONG0 ? A->x_io : A->x_alt, mode == ATOM_LONG0 ? A->x_alt : A->x_io, true);
        else
            atom_build_step(A, p.get(), B, mode != ATOM_FORWARD, mode == ATOM_STEP, mode == ATOM_STEP ? A->x_io : A->OUT + (size_t)A->nbmax * A->L * NFEAT);
        it = c->plans.emplace(std::make_pair(B, mode), std::move(p)).first;
    }
    *out = it->second.get();
    return MTV_OK;
}
int atom_run(mtv_ctx* c, Plan* p, hipStream_t s) {
    if (c->eager) return run_ops(c, p, s);
    int rc;
    if (!p->g_forward && (rc = capture(c, p, &p->g_forward)) != MTV_OK) return rc;
    HIPCHK(hipGraphLaunch(p->g_forward, s));
    return MTV_OK;
}
int atom_ready(mtv_ctx* c, AtomState* A, int batch) {
    if (!A) return fail(MTV_ERR_INVALID, "not an AToM context");
    int rc = check_ready(c, batch);
    if (rc != MTV_OK) return rc;
    if (!A->tables) return fail(MTV_ERR_STATE, "mtv_atom_set_tables has not been called");
    return MTV_OK;
}
}  // namespace

extern "C" {

int mtv_atom_create(const mtv_atom_config* cfg, mtv_ctx** out) {
    if (!cfg || !out) return fail(MTV_ERR_INVALID, "null argument");
    const mtv_atom_config& f = *cfg;
    if (f.nfeats != NFEAT) return fail(MTV_ERR_INVALID, "nfeats must be 204 (68 landmarks x 3: the forward hard-wires the 17 | 31 | 20 split)");
    if (f.latent_dim < 32 || f.latent_dim % 32) return fail(MTV_ERR_INVALID, "latent_dim must be a multiple of 32");
    if (f.num_heads < 1 || f.latent_dim % f.num_heads) return fail(MTV_ERR_INVALID, "latent_dim must be divisible by num_heads");
    const int d = f.latent_dim / f.num_heads;
    if (d % 4 || d > 64) return fail(MTV_ERR_INVALID, "head dim must be a multiple of 4, at most 64");
    if (f.ff_size < 4 || f.ff_size % 4 || f.cond_feature_dim < 4 || f.cond_feature_dim % 4) return fail(MTV_ERR_INVALID, "ff_size and cond_feature_dim must be multiples of 4");
    if (f.seq_len < 1 || 3 * f.seq_len + 2 > ATT_KMAX) return fail(MTV_ERR_INVALID, "seq_len must be in [1, 170] (memory has 3 seq_len + 2 keys)");
    if (f.num_layers < 1 || f.max_batch < 1) return fail(MTV_ERR_INVALID, "bad sizes");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(MTV_ERR_HIP, "no HIP device available");
    std::unique_ptr<mtv_ctx> c(new mtv_ctx());
    c->cfg.max_batch = f.max_batch;
    int rc = ctx_init_common(c.get());
    if (rc != MTV_OK) return rc;
    auto st = std::make_shared<AtomState>();
    AtomState& A = *st;
    A.f = f;
    const int D = A.D = f.latent_dim, L = A.L = f.seq_len, nl = A.nl = f.num_layers, ff = f.ff_size;
    const int Lm = A.Lm = 3 * L + 2, Lf = A.Lf = L + 2, nb = A.nbmax = 2 * f.max_batch, B = f.max_batch;
    bool ok = true;
    auto W = [&](const std::string& key, std::vector<int64_t> shape) { ok = ok && (A.w[key] = c->wcopy(key, std::move(shape))) != nullptr; };
    auto WB = [&](const std::string& pre, int n, int k) { W(pre + ".weight", {n, k}); W(pre + ".bias", {n}); };
    auto LN = [&](const std::string& pre) { W(pre + ".weight", {D}); W(pre + ".bias", {D}); };
    auto MHA = [&](const std::string& pre) { W(pre + ".in_proj_weight", {3 * D, D}); W(pre + ".in_proj_bias", {3 * D}); WB(pre + ".out_proj", D, D); };
    // the keys the forward reads, in state_dict order (held but never run: input_projection, pos_projection, pos_encoder, non_attn_pos_projection,
    // face_mlp, to_face_cond, to_face_tokens and the decoder layers' linear1 / linear2 -- the Python holder keeps those)
    W("null_cond_embed", {1, 2 * L, D});
    W("null_cond_hidden", {1, D});
    W("face_null_cond_embed", {1, L, D});
    WB("time_mlp.1", 4 * D, D);
    WB("to_time_cond.0", D, 4 * D);
    WB("to_time_tokens.0", 2 * D, 4 * D);
    LN("norm_cond");
    A.bin = c->buf("a.bin", (size_t)2 * D);
    W("input_projection_lip.weight", {D, 111});
    c->slot("input_projection_lip.bias", {D}, ROLE_COPY, A.bin, 0);
    W("input_projection_wo_lip.weight", {D, 93});
    c->slot("input_projection_wo_lip.bias", {D}, ROLE_COPY, A.bin ? A.bin + D : nullptr, 0);
    for (const char* enc : {"cond_encoder.", "face_encoder."})
        for (int i = 0; i < 2; ++i) {
            const std::string pre = enc + std::to_string(i);
            MHA(pre + ".self_attn");
            WB(pre + ".linear1", ff, D);
            WB(pre + ".linear2", D, ff);
            LN(pre + ".norm1");
            LN(pre + ".norm2");
        }
    WB("cond_projection", D, f.cond_feature_dim);
    WB("face_projection", D, NFEAT);
    for (const char* pre : {"non_attn_cond_projection", "non_attn_face_projection"}) {
        LN(std::string(pre) + ".0");
        WB(std::string(pre) + ".1", D, D);
        WB(std::string(pre) + ".3", D, D);
    }
    A.Wfilm = c->buf("a.Wfilm", (size_t)nl * 6 * D * D);
    A.bfilm = c->buf("a.bfilm", (size_t)nl * 6 * D);
    ok = ok && A.bin && A.Wfilm && A.bfilm;
    for (int l = 0; ok && l < nl; ++l) {
        const std::string pre = "seqTransDecoder.stack." + std::to_string(l);
        MHA(pre + ".self_attn");
        MHA(pre + ".multihead_attn");
        WB(pre + ".linear3", 2 * D, D);
        LN(pre + ".norm1");
        LN(pre + ".norm2");
        LN(pre + ".norm3");
        for (int k = 0; k < 3; ++k) {      // the three DenseFiLM Linears of every layer side by side: ONE GEMM per step
            const std::string fk = pre + ".film" + std::to_string(k + 1) + ".block.1";
            c->slot(fk + ".weight", {2 * D, D}, ROLE_COPY, A.Wfilm + (size_t)(l * 3 + k) * 2 * D * D, 0);
            c->slot(fk + ".bias", {2 * D}, ROLE_COPY, A.bfilm + (size_t)(l * 3 + k) * 2 * D, 0);
        }
    }
    WB("final_layer", NFEAT, 2 * D);
    auto BUF = [&](float*& p, const char* name, size_t n) { ok = ok && (p = c->buf(name, n)) != nullptr; };
    BUF(A.Win, "a.Win", (size_t)2 * D * NFEAT);
    BUF(A.rot, "a.rot", (size_t)Lm * D);
    BUF(A.tfreq, "a.tfreq", (size_t)D / 2);
    BUF(A.x_io, "a.x_io", (size_t)B * L * NFEAT);
    BUF(A.x_alt, "a.x_alt", (size_t)B * L * NFEAT);
    BUF(A.X, "a.X", (size_t)nb * L * 2 * D);
    BUF(A.QKV, "a.QKV", (size_t)nb * L * 6 * D);
    BUF(A.ATT, "a.ATT", (size_t)nb * L * 2 * D);
    BUF(A.XT, "a.XT", (size_t)nb * L * D);
    BUF(A.OUT, "a.OUT", (size_t)(nb + B) * L * NFEAT);      // [nb clips of output | B clips of staged input]
    BUF(A.CT, "a.CT", (size_t)nb * 2 * L * D);
    BUF(A.FT, "a.FT", (size_t)nb * L * D);
    BUF(A.EQKV, "a.EQKV", (size_t)B * 2 * L * 3 * D);
    BUF(A.EATT, "a.EATT", (size_t)B * 2 * L * D);
    BUF(A.EFF, "a.EFF", (size_t)B * 2 * L * ff);
    BUF(A.Cmem, "a.Cmem", (size_t)nb * Lm * D);
    BUF(A.Cface, "a.Cface", (size_t)nb * Lf * D);
    BUF(A.pool, "a.pool", (size_t)nb * D);
    BUF(A.hid1, "a.hid1", (size_t)nb * D);
    BUF(A.fh, "a.fh", (size_t)nb * D);
    BUF(A.ch, "a.ch", (size_t)nb * D);
    BUF(A.hid_add, "a.hid_add", (size_t)nb * D);
    BUF(A.tv, "a.tv", (size_t)nb);
    BUF(A.tsin, "a.tsin", (size_t)nb * D);
    BUF(A.th, "a.th", (size_t)nb * 4 * D);
    BUF(A.tvec, "a.tvec", (size_t)nb * D);
    BUF(A.ttok, "a.ttok", (size_t)nb * 2 * D);
    BUF(A.film, "a.film", (size_t)nb * nl * 6 * D);
    A.KVm.resize(nl);
    A.KVf.resize(nl);
    for (int l = 0; l < nl; ++l) {
        BUF(A.KVm[l], ("a.KVm" + std::to_string(l)).c_str(), (size_t)nb * Lm * 2 * D);
        BUF(A.KVf[l], ("a.KVf" + std::to_string(l)).c_str(), (size_t)nb * Lf * 2 * D);
    }
    float* rec = nullptr;
    A.steps_cap = 1024;
    BUF(rec, "a.rec", (sizeof(AtomCur) + 64 + (size_t)A.steps_cap * sizeof(DdimStep)) / 4 + 16 + (size_t)A.steps_cap);
    if (!ok) return fail(MTV_ERR_HIP, "allocation failed");
    A.cur = reinterpret_cast<AtomCur*>(rec);
    A.counter = reinterpret_cast<int*>(rec + (sizeof(AtomCur) + 15) / 16 * 4);
    A.steps = reinterpret_cast<DdimStep*>(rec + (sizeof(AtomCur) + 15) / 16 * 4 + 16);
    A.gws = reinterpret_cast<float*>(A.steps + A.steps_cap);
    c->kind = CTX_ATOM;
    c->ext = st;
    *out = c.release();
    return MTV_OK;
}

int mtv_atom_destroy(mtv_ctx* c) {
    if (c && c->kind != CTX_ATOM) return fail(MTV_ERR_INVALID, "not an AToM context");
    delete c;
    return MTV_OK;
}

int mtv_atom_set_tables(mtv_ctx* c, const float* rot_tab, int n_pos, const float* time_freqs) {
    AtomState* A = atom_of(c);
    if (!A) return fail(MTV_ERR_INVALID, "not an AToM context");
    if (!rot_tab || !time_freqs) return fail(MTV_ERR_INVALID, "null table");
    if (n_pos != A->Lm) return fail(MTV_ERR_INVALID, "the rotary table must have 3 seq_len + 2 positions");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(A->rot, rot_tab, (size_t)A->Lm * A->D * sizeof(float), hipMemcpyDefault));
    HIPCHK(hipMemcpy(A->tfreq, time_freqs, (size_t)A->D / 2 * sizeof(float), hipMemcpyDefault));
    A->tables = true;
    return MTV_OK;
}

int mtv_atom_set_guidance(mtv_ctx* c, float w) {
    AtomState* A = atom_of(c);
    if (!A) return fail(MTV_ERR_INVALID, "not an AToM context");
    A->gw = w;
    return MTV_OK;
}

static int atom_write_cur(AtomState* A, float gw, int ddim, const float* noise, long long n_per, hipStream_t s) {
    AtomCur& h = A->h_cur;
    h = AtomCur{};
    h.gw = gw;
    h.ddim = ddim;
    h.noise = noise;
    h.n_per_draw = n_per;
    HIPCHK(hipMemcpyAsync(A->cur, &h, sizeof h, hipMemcpyHostToDevice, s));
    return MTV_OK;
}

int mtv_atom_forward(mtv_ctx* c, const float* x, const float* face, const float* cond, const int64_t* times, int drop, float* out, int batch,
                     void* stream) {
    AtomState* A = atom_of(c);
    int rc = atom_ready(c, A, batch);
    if (rc != MTV_OK) return rc;
    if (!x || !face || !cond || !times || !out) return fail(MTV_ERR_INVALID, "null tensor pointer");
    if (drop != 0 && drop != 1) return fail(MTV_ERR_INVALID, "cond_drop_prob must be exactly 0 or 1");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)batch * A->L * NFEAT;
    HIPCHK(hipMemcpyAsync(A->OUT + (size_t)A->nbmax * A->L * NFEAT, x, n * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(atom_setup(*A, batch, drop ? DROP_ALL : DROP_NONE, face, cond, s));
    hipLaunchKernelGGL(k_atom_times, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, times, A->tv, batch, batch);
    HIPCHK(hipGetLastError());
    Plan* p = nullptr;
    if ((rc = atom_plan(c, A, batch, ATOM_FORWARD, &p)) != MTV_OK || (rc = atom_run(c, p, s)) != MTV_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, A->OUT, n * 4, hipMemcpyDeviceToDevice, s));
    return MTV_OK;
}

int mtv_atom_guided_forward(mtv_ctx* c, const float* x, const float* face, const float* cond, const int64_t* times, float guidance_weight,
                            float* out, int batch, void* stream) {
    AtomState* A = atom_of(c);
    int rc = atom_ready(c, A, batch);
    if (rc != MTV_OK) return rc;
    if (!x || !face || !cond || !times || !out) return fail(MTV_ERR_INVALID, "null tensor pointer");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)batch * A->L * NFEAT;
    HIPCHK(hipMemcpyAsync(A->OUT + (size_t)A->nbmax * A->L * NFEAT, x, n * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(atom_setup(*A, batch, DROP_PAIR, face, cond, s));
    hipLaunchKernelGGL(k_atom_times, dim3((unsigned)((2 * batch + 255) / 256)), dim3(256), 0, s, times, A->tv, 2 * batch, batch);
    HIPCHK(hipGetLastError());
    if ((rc = atom_write_cur(A, guidance_weight, 0, nullptr, 0, s)) != MTV_OK) return rc;
    Plan* p = nullptr;
    if ((rc = atom_plan(c, A, batch, ATOM_GUIDED, &p)) != MTV_OK || (rc = atom_run(c, p, s)) != MTV_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, A->OUT, n * 4, hipMemcpyDeviceToDevice, s));
    return MTV_OK;
}

// the argument checks both samplers share; nothing has been launched when they fail
static int atom_check_sample(AtomState* A, const float* x_io, const float* face, const float* cond, const float* noise, int n_noise,
                             const mtv_ddim_step* steps, int n_steps) {
    static_assert(sizeof(DdimStep) == sizeof(mtv_ddim_step), "step layout");
    if (!x_io || !face || !cond || !steps) return fail(MTV_ERR_INVALID, "null tensor pointer");
    if (n_steps < 1 || n_steps > A->steps_cap) return fail(MTV_ERR_INVALID, "n_steps outside [1, 1024]");
    for (int i = 0; i < n_steps; ++i) {
        if (!steps[i].last && (steps[i].noise_index < 0 || steps[i].noise_index >= n_noise || !noise))
            return fail(MTV_ERR_INVALID, "step " + std::to_string(i) + " needs a noise draw the caller did not supply");
        if (!(steps[i].sqrt_recipm1_ac > 0.0f)) return fail(MTV_ERR_INVALID, "sqrt_recipm1_ac must be positive (pred_noise divides by it)");
    }
    return MTV_OK;
}

int mtv_atom_ddim_sample(mtv_ctx* c, float* x_io, const float* face, const float* cond, const float* noise, int n_noise,
                         const mtv_ddim_step* steps, int n_steps, int batch, void* stream) {
    AtomState* A = atom_of(c);
    int rc = atom_ready(c, A, batch);
    if (rc != MTV_OK) return rc;
    if ((rc = atom_check_sample(A, x_io, face, cond, noise, n_noise, steps, n_steps)) != MTV_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)batch * A->L * NFEAT;
    HIPCHK(hipMemcpyAsync(A->x_io, x_io, n * 4, hipMemcpyDeviceToDevice, s));
    A->h_steps.resize(n_steps);
    std::memcpy(A->h_steps.data(), steps, (size_t)n_steps * sizeof(DdimStep));
    HIPCHK(hipMemcpyAsync(A->steps, A->h_steps.data(), (size_t)n_steps * sizeof(DdimStep), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(A->counter, 0, sizeof(int), s));
    if ((rc = atom_write_cur(A, A->gw, 1, noise, (long long)n, s)) != MTV_OK) return rc;
    HIPCHK(atom_setup(*A, batch, DROP_PAIR, face, cond, s));
    Plan* p = nullptr;
    if ((rc = atom_plan(c, A, batch, ATOM_STEP, &p)) != MTV_OK) return rc;
    for (int i = 0; i < n_steps; ++i)
        if ((rc = atom_run(c, p, s)) != MTV_OK) return rc;
    HIPCHK(hipMemcpyAsync(x_io, A->x_io, n * 4, hipMemcpyDeviceToDevice, s));
    return MTV_OK;
}

int mtv_atom_long_ddim_sample(mtv_ctx* c, float* x_io, const float* face, const float* cond, const float* noise, int n_noise,
                              const mtv_ddim_step* steps, int n_steps, const float* weights, int batch, void* stream) {
    AtomState* A = atom_of(c);
    int rc = atom_ready(c, A, batch);
    if (rc != MTV_OK) return rc;
    if (batch < 2) return fail(MTV_ERR_INVALID, "the long sampler needs at least 2 windows (one window is mtv_atom_ddim_sample)");
    if (A->L % 2) return fail(MTV_ERR_INVALID, "the long sampler needs an even seq_len (windows overlap by half)");
    if ((rc = atom_check_sample(A, x_io, face, cond, noise, n_noise, steps, n_steps)) != MTV_OK) return rc;
    if (!weights) return fail(MTV_ERR_INVALID, "null guidance weight table");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)batch * A->L * NFEAT;
    HIPCHK(hipMemcpyAsync(A->x_io, x_io, n * 4, hipMemcpyDeviceToDevice, s));
    A->h_steps.resize(n_steps);
    std::memcpy(A->h_steps.data(), steps, (size_t)n_steps * sizeof(DdimStep));
    HIPCHK(hipMemcpyAsync(A->steps, A->h_steps.data(), (size_t)n_steps * sizeof(DdimStep), hipMemcpyHostToDevice, s));
    A->h_gws.assign(weights, weights + n_steps);
    HIPCHK(hipMemcpyAsync(A->gws, A->h_gws.data(), (size_t)n_steps * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(A->counter, 0, sizeof(int), s));
    if ((rc = atom_write_cur(A, 0.0f, 1, noise, (long long)n, s)) != MTV_OK) return rc;      // (gw: k_atom_advance writes the step's)
    HIPCHK(atom_setup(*A, batch, DROP_PAIR, face, cond, s));
    Plan* p[2] = {nullptr, nullptr};
    if ((rc = atom_plan(c, A, batch, ATOM_LONG0, &p[0])) != MTV_OK || (rc = atom_plan(c, A, batch, ATOM_LONG1, &p[1])) != MTV_OK) return rc;
    for (int i = 0; i < n_steps; ++i)      // step i reads the buffer step i - 1 wrote
        if ((rc = atom_run(c, p[i & 1], s)) != MTV_OK) return rc;
    HIPCHK(hipMemcpyAsync(x_io, n_steps & 1 ? A->x_alt : A->x_io, n * 4, hipMemcpyDeviceToDevice, s));
    return MTV_OK;
}

int mtv_atom_long_num_launches(mtv_ctx* c, int batch, int* per_step) {
    AtomState* A = atom_of(c);
    if (!A || !per_step) return fail(MTV_ERR_INVALID, "not an AToM context");
    Plan* p = nullptr;
    int rc = atom_plan(c, A, batch, ATOM_LONG0, &p);
    if (rc != MTV_OK) return rc;
    *per_step = (int)p->ops.size();
    return MTV_OK;
}

int mtv_atom_num_launches(mtv_ctx* c, int batch, int* per_step) {
    AtomState* A = atom_of(c);
    if (!A || !per_step) return fail(MTV_ERR_INVALID, "not an AToM context");
    Plan* p = nullptr;
    int rc = atom_plan(c, A, batch, ATOM_STEP, &p);
    if (rc != MTV_OK) return rc;
    *per_step = (int)p->ops.size();
    return MTV_OK;
}

}  // extern "C"
