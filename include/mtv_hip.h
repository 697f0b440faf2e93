/*
 * mtv_hip.h -- C ABI of libmtv_hip.so: the MI355X (gfx950) denoising step of MoDiTalker's MToV
 * latent-video diffusion sampler (tri-plane UNet forward + eta=1 DDIM update) as hand-written HIP.
 *
 * The reference has NO FFI / plugin interface for this path: its boundary is three Python classes
 * (SURVEY.md section 8b).  This header is therefore the build's own C boundary *under* the Python
 * look-alikes in moditalker_amd/{unet,ddpm}.py; each entry point cites the reference code whose
 * work it replaces.  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C, no torch types: device pointers are raw `float*` / `int64_t*` (Tensor.data_ptr()),
 *     BORROWED for the duration of the call (the caller keeps ownership and keeps them alive until
 *     the stream has drained); sizes are ints.
 *   - every function returns MTV_OK (0) or a negative error code; mtv_last_error() gives the text
 *     of the last failure on the calling thread.  No C++ exception crosses the ABI.
 *   - a context is bound to the HIP device that was current at mtv_create() and is NOT re-entrant:
 *     one caller at a time, launches go to the `stream` argument (pass torch's current stream so
 *     torch ordering holds).  `stream` is a hipStream_t passed as void*.
 *   - all tensors fp32.  External activations use the reference's layout, channel-major
 *     [B, C, L] with L = R*R + 2*T*R (xy plane | yt plane | xt plane, unet.py:1027-1029).
 */
#ifndef MTV_HIP_H
#define MTV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTV_OK 0
#define MTV_ERR_INVALID (-1)     /* bad argument / unsupported configuration */
#define MTV_ERR_HIP (-2)         /* a HIP runtime call failed                 */
#define MTV_ERR_WEIGHT (-3)      /* unknown key, wrong shape, or weights missing at forward time */
#define MTV_ERR_STATE (-4)       /* call sequence error (e.g. batch > max_batch) */
#define MTV_IGNORED 1            /* mtv_load_weight: key accepted but unused (output_bg_*) */

#define MTV_MAX_LEVELS 8

/* UNet hyper-parameters: the subset of UNetModel.__init__ kwargs (unet.py:631-659) the hot path
 * depends on, plus the tri-plane geometry the reference hard-wires to (32,16) (unet.py:1027-1029). */
typedef struct mtv_config {
    int32_t model_channels;                       /* unet_config.model_channels (128)            */
    int32_t num_res_blocks;                       /* (2)                                         */
    int32_t num_heads;                            /* (8) heads in every attention block          */
    int32_t n_levels;                             /* len(channel_mult)                           */
    int32_t channel_mult[MTV_MAX_LEVELS];         /* ([1,2,4,4])                                 */
    int32_t n_attention_resolutions;
    int32_t attention_resolutions[MTV_MAX_LEVELS];/* ([4,2,1]) downsample rates with 2-D attention */
    int32_t use_scale_shift_norm;                 /* (1) FiLM: GN(h)*(1+s)+b ; 0: h+emb then GN  */
    int32_t out_channels;                         /* (4)                                         */
    int32_t res;                                  /* R: xy plane is R x R                        */
    int32_t frames;                               /* T: yt / xt planes are T x R                 */
    int32_t max_batch;                            /* workspace is sized for this many clips      */
} mtv_config;

typedef struct mtv_ctx mtv_ctx;

const char* mtv_last_error(void);
int mtv_version(void);

/* Replaces UNetModel.__init__ (unet.py:631-975): builds the block list, allocates the
 * token-major channels-last workspace [B, L, C] per tensor and the im2col gather tables. */
int mtv_create(const mtv_config* cfg, mtv_ctx** out);
int mtv_destroy(mtv_ctx* ctx);

/* Checkpoint interface -- replaces `load_state_dict` (sample.py:229-230).
 * Keys are the reference's state_dict names WITHOUT the `diffusion_model.` prefix, e.g.
 * "input_blocks.4.0.in_layers.2.weight" [256,128,3,3].  `data` may be a host or a device pointer
 * (fp32, contiguous, PyTorch layout: OIHW conv, [O,I,1] conv1d, [O,I] linear); the library repacks
 * into its device layout ([tap][Cin][Cout] etc.).  Keys under output_bg_blocks./output_bg_attns.
 * (dead in the reference forward, unet.py:859-968) are accepted and return MTV_IGNORED. */
int mtv_num_weights(const mtv_ctx* ctx);
int mtv_weight_info(const mtv_ctx* ctx, int index, char* key_out, int key_cap, int* ndim_out, int64_t shape_out[4]);
int mtv_load_weight(mtv_ctx* ctx, const char* key, const float* data, int ndim, const int64_t* shape);
int mtv_weights_missing(const mtv_ctx* ctx);   /* number of required keys not loaded yet */

/* Replaces UNetModel.forward / DiffusionWrapper.forward (unet.py:995-1117, 41-44):
 *   x [B,4,L], cond [B,8,L], image_cond [B,4,image_cond_len] (only the first R*R tokens are
 *   used, the yt/xt planes of image_cond are zeros: unet.py:1022-1025), timesteps [B] int64 on the
 *   device, eps_out [B,out_channels,L].  All device pointers. */
int mtv_forward(mtv_ctx* ctx, const float* x, const float* cond, const float* image_cond,
                int image_cond_len, const int64_t* timesteps, float* eps_out, int batch, void* stream);

/* One entry per DDIM step, computed by the host exactly as ddpm.py:390-394 does (fp32). */
typedef struct mtv_ddim_step {
    int32_t t;                 /* timestep fed to the UNet (ddpm.py:383)                          */
    int32_t last;              /* 1: time_next < 0 -> result is clamped x0 (ddpm.py:386-388)      */
    float sqrt_recip_ac;       /* sqrt(1/alphas_cumprod[t])        (ddpm.py:278-282)              */
    float sqrt_recipm1_ac;     /* sqrt(1/alphas_cumprod[t] - 1)                                   */
    float sqrt_ac_next;        /* alphas_cumprod[t_next].sqrt()    (ddpm.py:398)                  */
    float c;                   /* (1 - alpha_next - sigma^2).sqrt()                               */
    float sigma;               /* eta * ((1-a/a_next)(1-a_next)/(1-a)).sqrt()                     */
    int32_t noise_index;       /* which [B,4,L] slab of `noise` this step adds (-1: none)         */
} mtv_ddim_step;

/* Replaces the loop body of DDPM.ddim_sample / ddim_sample_noised_start (ddpm.py:382-398,
 * 434-448) for `n_steps` consecutive steps: eps = UNet(x_t, cond, image_cond, t);
 * x0 = clamp(sqrt_recip*x_t - sqrt_recipm1*eps, -1, 1); x <- x0*sqrt_ac_next + c*eps + sigma*noise.
 *   x_io      [B,4,L]  in: x_T (or the q_sample'd start); out: the clamped x0 of the last step
 *   noise     [n_noise,B,4,L] explicit N(0,1) draws (the reference draws them from torch's global
 *             generator inside the loop; the Python wrapper owns that RNG)
 * A step is ONE hipGraph replay and consists of the UNet's launches only: the FiLM rows of all steps are computed
 * once per call, the DDIM update and the hand-over to the next step (step counter, packed input, FiLM row,
 * statistics arena) run inside the head conv; steps are device-resident (no host synchronisation in the loop). */
int mtv_ddim_sample(mtv_ctx* ctx, float* x_io, const float* cond, const float* image_cond,
                    int image_cond_len, const float* noise, int n_noise,
                    const mtv_ddim_step* steps, int n_steps, int batch, void* stream);

/* Fault state of the in-launch hand-offs.  Some launches of a step exchange data between their own workgroups (k_deep_block's clusters, the
 * tagged completion of a deep tensor: csrc/block.hip, csrc/deep.hip); a poll that is not served within 2^21 retries (seconds) raises a
 * host-visible fault word and falls through -- never a hang, but the call's output is then garbage.  The reference raises Python exceptions
 * synchronously (unet.py:995-1117 is plain torch); here launches are asynchronous, so:
 *   - mtv_check_fault(ctx) reads the word: MTV_OK, or MTV_ERR_STATE with the explanation in mtv_last_error().  It is meaningful for a call
 *     once the stream that call ran on has drained -- call it after the synchronisation point you have anyway (it does not synchronise);
 *   - every later entry point of a faulted context refuses to run (MTV_ERR_STATE): a fault is sticky, destroy the context.
 * moditalker_amd.DDPM.sample(..., strict=True) / UNetModel.forward(..., strict=True) synchronise the stream and check before returning. */
int mtv_check_fault(mtv_ctx* ctx);
/* CUs this context counts on being resident together (the device's multiProcessorCount unless overridden): every grid whose workgroups wait
 * for each other is planned within it (k_deep_block: half of it; tagged completion: all of it), larger ones fall back to the forms without
 * in-launch hand-offs (three-launch attention block, k_deep_finalize pass).  A stream whose CU mask (hipExtStreamCreateWithCUMask) leaves
 * fewer CUs is refused by mtv_forward / mtv_ddim_sample with MTV_ERR_STATE. */
int mtv_resident_cus(const mtv_ctx* ctx);

/* Introspection for bench.py / DESIGN.md: algorithmic work of one forward at batch 1. */
typedef struct mtv_work {
    double flops_conv3x3, flops_1x1, flops_attn_core, flops_linear;
    double bytes_weights_conv, bytes_weights_other, bytes_act_conv_path;
    int32_t n_launches;        /* launches of one mtv_forward (time-embedding chain + packing + UNet) */
    int32_t n_launches_step;   /* launches of one sampler step inside mtv_ddim_sample (UNet launches only) */
} mtv_work;
int mtv_get_work(const mtv_ctx* ctx, mtv_work* out);

/* Per-launch timing of one UNet forward, measured with hipEvents on `stream` around every launch
 * of the plan (plain launches, averaged over `iters` passes).  Call with out == NULL to get the
 * number of launches in *n_out.  flops/bytes are the algorithmic figures of that launch. */
typedef struct mtv_op_time {
    char name[96];
    float ms;
    double flops;
    double bytes;
} mtv_op_time;
int mtv_profile_forward(mtv_ctx* ctx, int batch, int iters, mtv_op_time* out, int cap, int* n_out, void* stream);
/* The same for one SAMPLER STEP (the launch sequence mtv_ddim_sample replays per step: UNet launches only, the
 * DDIM update inside the head conv).  Runs on the context's own staging buffers with a one-entry step table. */
int mtv_profile_step(mtv_ctx* ctx, int batch, int iters, mtv_op_time* out, int cap, int* n_out, void* stream);

/* 0: replay the step as a hipGraph (default); 1: plain launches (profiling / debugging). */
int mtv_set_eager(mtv_ctx* ctx, int eager);

/* ------------------------------------------------------------------------------------------------
 * The autoencoder steps either side of the denoising loop.
 * Replaces ViTAutoencoder.decode_from_sample / .extract (MToV/models/autoencoder/autoencoder_vit.py:257-275, 212-255;
 * called at MToV/sample.py:328-332,369,386).  A separate context of the same opaque type: weights go in through
 * mtv_num_weights / mtv_weight_info / mtv_load_weight / mtv_weights_missing with the reference's state_dict keys
 * (e.g. "decoder.layers.0.0.fn.to_qkv.weight" [1536,384], "to_pixel.1.weight" [384,3,8,8]).
 * ------------------------------------------------------------------------------------------------ */
typedef struct mtv_ae_config {
    int32_t channels;      /* ddconfig.channels (384)                                                    */
    int32_t resolution;    /* ddconfig.resolution (256)                                                  */
    int32_t frames;        /* ddconfig.timesteps / splits (16)                                           */
    int32_t patch;         /* 8 (4 at resolution 128: autoencoder_vit.py:105-107)                        */
    int32_t embed_dim;     /* 4                                                                          */
    int32_t depth;         /* 8 TimeSformer layers per coder (autoencoder_vit.py:110-116)                */
    int32_t heads;         /* 8                                                                          */
    int32_t dim_head;      /* 64                                                                         */
    int32_t max_batch;
} mtv_ae_config;

int mtv_ae_create(const mtv_ae_config* cfg, mtv_ctx** out);
int mtv_ae_destroy(mtv_ctx* ctx);
/* Rotary tables, computed by the host exactly as RotaryEmbedding / AxialRotaryEmbedding.forward do
 * (vit_modules.py:29-49,57-62): time_tab [frames][2][dim_head], space_tab [(res/patch)^2][2][dim_head]; row 0 = sin,
 * row 1 = cos.  Host or device pointers. */
int mtv_ae_set_rotary(mtv_ctx* ctx, const float* time_tab, const float* space_tab);
/* latents [B, embed_dim, r*r + 2*frames*r] (r = resolution/patch; the sampler's output) -> frames
 * [B*frames, 3, resolution, resolution] in (-1, 1).  Device pointers. */
int mtv_ae_decode(mtv_ctx* ctx, const float* latents, float* frames_out, int batch, void* stream);
/* video [B, 3, frames, resolution, resolution] in [-1, 1] -> latents [B, embed_dim, r*r + 2*frames*r] (tanh outputs). */
int mtv_ae_extract(mtv_ctx* ctx, const float* video, float* latents_out, int batch, void* stream);
/* Per-launch hipEvent timing of decode (extract != 0: of extract), like mtv_profile_forward. */
int mtv_ae_profile(mtv_ctx* ctx, int batch, int extract, int iters, mtv_op_time* out, int cap, int* n_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CrossAttention (unet.py:429-467) as a stand-alone operator: the one usable piece of the
 * reference's dormant cross-attention conditioning (SpatialTransformer cannot be constructed there, unet.py:470-489,513).
 * Weights through mtv_load_weight with the module's keys: "to_q.weight" [H*d, query_dim], "to_k.weight" / "to_v.weight"
 * [H*d, context_dim], "to_out.0.weight" [query_dim, H*d], "to_out.0.bias" [query_dim].
 * ------------------------------------------------------------------------------------------------ */
typedef struct mtv_xattn_config {
    int32_t query_dim, context_dim, heads, dim_head;
    int32_t max_batch, max_queries, max_keys;
} mtv_xattn_config;
int mtv_xattn_create(const mtv_xattn_config* cfg, mtv_ctx** out);
int mtv_xattn_destroy(mtv_ctx* ctx);
/* x [B, n_queries, query_dim]; context [B, n_keys, context_dim] or NULL (= x: self-attention); mask [B, n_keys] bytes or
 * NULL (0 = key masked out, unet.py:452-456); out [B, n_queries, query_dim].  Device pointers. */
int mtv_xattn_forward(mtv_ctx* ctx, const float* x, const float* context, const unsigned char* mask, float* out, int batch,
                      int n_queries, int n_keys, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The audio-to-motion stage in front of MToV: AToM's MotionDecoder and its DDIM sampler (csrc/atom.hip).
 * Replaces MotionDecoder.forward / guided_forward (AToM/model/model.py:385-470) and the loop of
 * GaussianDiffusion.ddim_sample (AToM/model/diffusion.py:212-250).  A separate context of the same opaque type:
 * weights go in through mtv_num_weights / mtv_weight_info / mtv_load_weight / mtv_weights_missing with the
 * reference's state_dict keys (e.g. "seqTransDecoder.stack.0.multihead_attn.in_proj_weight" [3 D, D]); the context
 * lists only the keys its forward reads (the reference holds several modules it never runs).
 * Tensors: x [B, seq_len, 204] landmarks, face [B, seq_len, 204], cond [B, 2 seq_len, cond_feature_dim], times [B]
 * int64; all device pointers.  x_pos of the reference is accepted by the Python class and unused there as here.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mtv_atom_config {
    int32_t nfeats;            /* 204                                                        */
    int32_t seq_len;           /* 156 (memory has 3 seq_len + 2 keys: at most 170)           */
    int32_t latent_dim;        /* 512; multiple of 32                                        */
    int32_t ff_size;           /* 1024                                                       */
    int32_t num_layers;        /* 8 FiLM decoder layers                                      */
    int32_t num_heads;         /* 8; head dim a multiple of 4, at most 64                    */
    int32_t cond_feature_dim;  /* 1024 (HuBERT)                                              */
    int32_t max_batch;
} mtv_atom_config;
int mtv_atom_create(const mtv_atom_config* cfg, mtv_ctx** out);
int mtv_atom_destroy(mtv_ctx* ctx);
/* Tables the host computes exactly as the reference does: rot_tab [n_pos = 3 seq_len + 2][latent_dim / 2][cos, sin] of
 * position * rotary.freqs (rotary_embedding_torch.py:117-132), time_freqs [latent_dim / 2] of SinusoidalPosEmb
 * (utils.py:41-48).  Host or device pointers. */
int mtv_atom_set_tables(mtv_ctx* ctx, const float* rot_tab, int n_pos, const float* time_freqs);
/* One forward with every clip's condition kept (drop = 0) or replaced by the null embeddings (drop = 1):
 * cond_drop_prob of model.py:391-399 restricted to the two values inference uses.  out [B, seq_len, 204]. */
int mtv_atom_forward(mtv_ctx* ctx, const float* x, const float* face, const float* cond, const int64_t* times, int drop,
                     float* out, int batch, void* stream);
/* unc + (cond - unc) * guidance_weight (model.py:385-389): both passes as one batch of 2 B clips. */
int mtv_atom_guided_forward(mtv_ctx* ctx, const float* x, const float* face, const float* cond, const int64_t* times,
                            float guidance_weight, float* out, int batch, void* stream);
/* Guidance weight of the sampler below (GaussianDiffusion.guidance_weight, diffusion.py:77,131-133); default 1. */
int mtv_atom_set_guidance(mtv_ctx* ctx, float guidance_weight);
/* The loop of ddim_sample for `n_steps` consecutive steps: x_start = clamp(guided_forward(x_t, t), -1, 1);
 * pred_noise = (sqrt_recip_ac x_t - x_start) / sqrt_recipm1_ac; x <- x_start sqrt_ac_next + c pred_noise + sigma noise;
 * the last step leaves x_start.  x_io [B, seq_len, 204] in: x_T, out: the sample; noise [n_noise, B, seq_len, 204].
 * The timestep-invariant part of the model (condition encoders, cross-attention keys / values) runs once per call,
 * every step is one replay of a linear hipGraph; no host synchronisation in the loop. */
int mtv_atom_ddim_sample(mtv_ctx* ctx, float* x_io, const float* face, const float* cond, const float* noise, int n_noise,
                         const mtv_ddim_step* steps, int n_steps, int batch, void* stream);
/* Launches of one sampler step at this batch size (introspection for tools/atom_bench.py). */
int mtv_atom_num_launches(mtv_ctx* ctx, int batch, int* per_step);
/* The loop of GaussianDiffusion.long_ddim_sample (AToM/model/diffusion.py:252-301), the EDGE-style sampler for motion
 * longer than one horizon: `batch` >= 2 half-overlapping windows denoised as one batch.  As mtv_atom_ddim_sample, plus
 *   - step i runs with guidance weight weights[i] (host array of n_steps floats; the reference's ramp
 *     np.clip(np.linspace(0, 2 w, 50), None, w), rounded to fp32, step 0 exactly 0) instead of mtv_atom_set_guidance's;
 *   - after the update of every step that is not `last`: x[b][w] <- x[b - 1][w + seq_len / 2] for b >= 1,
 *     w < seq_len / 2 (the values just computed); the `last` step leaves the clamped x_start unstitched, as the reference.
 * The stitch is part of the last launch of a step: the sample lives in two buffers and steps alternate between them,
 * so no launch reads what it writes.  seq_len must be even.  Running the first n_steps < 50 records returns x_t there
 * (after the update and the stitch).  Errors are reported before any launch. */
int mtv_atom_long_ddim_sample(mtv_ctx* ctx, float* x_io, const float* face, const float* cond, const float* noise, int n_noise,
                              const mtv_ddim_step* steps, int n_steps, const float* weights, int batch, void* stream);
/* Launches of one step of the long sampler at this batch size: the same chain as mtv_atom_num_launches reports. */
int mtv_atom_long_num_launches(mtv_ctx* ctx, int batch, int* per_step);

/* ------------------------------------------------------------------------------------------------
 * The stage in front of AToM: HuBERT audio features (csrc/hubert.hip).  Replaces the HubertModel.forward calls and the
 * Wav2Vec2FeatureExtractor normalisation of data/data_utils/preprocess/process_audio.py:9-55: a 16 kHz waveform in,
 * last_hidden_state [batch, T, hidden] out.  The stable-layer-norm form with layer-normed conv layers (the "large" family):
 * conv feature encoder -> LayerNorm + projection -> x + GELU(grouped positional conv(x)) -> n_layers of
 * x += attn(LN x); x += W2 gelu(W1 LN x) -> LayerNorm.  A separate context of the same opaque type: weights go in through
 * mtv_num_weights / mtv_weight_info / mtv_load_weight / mtv_weights_missing with transformers' HubertModel state_dict keys
 * (e.g. "encoder.layers.0.attention.q_proj.weight" [hidden, hidden]; the positional conv as
 * "encoder.pos_conv_embed.conv.parametrizations.weight.original0" [1, 1, taps] (g) and "...original1" [hidden, hidden / groups, taps]
 * (v): the effective weight v g / |v| is formed once after a load, not per call).  All tensors are device pointers.
 * ------------------------------------------------------------------------------------------------ */
#define MTV_HUBERT_MAX_CONV 8
typedef struct mtv_hubert_config {
    int32_t hidden;                             /* 1024; multiple of 4                                      */
    int32_t n_layers;                           /* 24                                                       */
    int32_t heads;                              /* 16; head dim a multiple of 4, at most 64                 */
    int32_t intermediate;                       /* 4096; multiple of 4                                      */
    int32_t n_conv;                             /* 7                                                        */
    int32_t conv_dim[MTV_HUBERT_MAX_CONV];      /* 512 each; multiples of 4                                 */
    int32_t conv_kernel[MTV_HUBERT_MAX_CONV];   /* 10, 3, 3, 3, 3, 2, 2                                     */
    int32_t conv_stride[MTV_HUBERT_MAX_CONV];   /* 5, 2, 2, 2, 2, 2, 2                                      */
    int32_t pos_taps;                           /* 128 (an even count drops the last output: T rows out)    */
    int32_t pos_groups;                         /* 16; hidden / groups a multiple of 4                      */
    float eps;                                  /* 1e-5: feature projection and encoder LayerNorms          */
    int32_t max_samples;                        /* longest clip a forward may be given (320080)             */
    int32_t max_batch;
} mtv_hubert_config;
int mtv_hubert_create(const mtv_hubert_config* cfg, mtv_ctx** out);
int mtv_hubert_destroy(mtv_ctx* ctx);
/* Wav2Vec2FeatureExtractor's do_normalize: out = (wave - mean) / sqrt(var + 1e-7) over all n samples (biased variance), any n >= 1.
 * Two fixed-order reduction passes (fp64 partial sums, no atomics), then the map: a repeated call is bit-equal.  out may be wave. */
int mtv_hubert_normalize(mtv_ctx* ctx, const float* wave, int64_t n, float* out, void* stream);
/* Frames of a clip of n_samples: (n - k) / s + 1 through every conv layer; 0 when a layer has no valid window.  The context-free
 * form below is the published geometry (10,3,3,3,3,2,2 / 5,2,2,2,2,2,2). */
int mtv_hubert_frames(const mtv_ctx* ctx, int n_samples);
int mtv_hubert_num_frames(int n_samples);
/* wave [batch, n_samples] (normalised; clips of one length) -> out [batch, T, hidden], T = mtv_hubert_frames(n_samples).
 * One linear chain of launches on `stream`; argument errors (T = 0, n_samples > max_samples, batch > max_batch, missing weights)
 * are reported before anything is launched. */
int mtv_hubert_forward(mtv_ctx* ctx, const float* wave, int n_samples, int batch, float* out, void* stream);
/* Launches of one forward at this clip length and batch. */
int mtv_hubert_num_launches(mtv_ctx* ctx, int n_samples, int batch, int* n_out);
/* Per-launch hipEvent timing of that forward, like mtv_ae_profile (out == NULL: only the count); the result is discarded. */
int mtv_hubert_profile(mtv_ctx* ctx, const float* wave, int n_samples, int batch, int iters, mtv_op_time* out, int cap, int* n_out,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Both ends of the MToV chunk loop (csrc/frames.hip): what MToV/sample.py:305-400 and MToV/tools/dataloader_sample.py:130-247 do on
 * the host around the extracts, the sampler and the decode.  Three context-free calls: they launch on the current device into
 * `stream`, all tensors are contiguous device pointers, every argument is checked before anything is launched.  All three are
 * gathers (a thread computes whole output elements from clipped source coordinates; no input value takes part in a store address,
 * no atomics).  Sides (res, canvas) are multiples of 4 up to 8192, batch and frames at most 4096; float tensors are 16-byte
 * aligned, 8-bit outputs and integer tables 4-byte aligned.
 * ------------------------------------------------------------------------------------------------ */
/* resize_crop (MToV/tools/data_utils.py:73-98) and `x / 127.5 - 1` with the b t c -> b c t transpose (sample.py:323-326):
 *   src [B, frames_in, 3, height, width] 8-bit, frames_in = frames or 1 (one frame repeated over `frames`: how x_ref is built)
 *   mask_start [B, frames] int32 or NULL: source rows >= mask_start[b][t] (row numbers of the uncropped frame) read as 0, i.e.
 *              _crop_lower_half (dataloader_sample.py:130-139) applied before the resize, the reference's order
 *   out [B, 3, frames, res, res] fp32.
 * Per output pixel: centre crop to the square S x S of the short side (half = (long - short) / 2 rounded down, for either
 * orientation), bilinear resize with align_corners = False and no antialiasing in ATen's float arithmetic --
 * scale = float(S) / res; src = scale * (dst + 0.5) - 0.5, below 0 -> 0; i0 = int(src); i1 = i0 + (i0 < S - 1); lambda1 = src - i0;
 * lambda0 = 1 - lambda1; value = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d) without fused multiply-adds -- then
 * value / 127.5 - 1, two roundings, in the form `division` names:
 *   MTV_FRAMES_DIV_IEEE        an IEEE division: what torch computes for x / 127.5 - 1 on the host;
 *   MTV_FRAMES_DIV_RECIPROCAL  value * fp32(1 / 127.5): what torch computes on a HIP device, where a division by a scalar becomes a
 *                              multiplication by its reciprocal -- the form sample.py:318-326 gets, its tensors being on the device by
 *                              then.  It differs from the division in the last bit for 111 of the 256 byte values.
 * With height == width == res the weights are exactly 1 and 0 and the result is bit-equal to that form of byte / 127.5 - 1. */
#define MTV_FRAMES_DIV_IEEE 0
#define MTV_FRAMES_DIV_RECIPROCAL 1
int mtv_frames_prep(const uint8_t* src, const int32_t* mask_start, float* out, int batch, int frames_in, int frames, int height,
                    int width, int res, int division, void* stream);
/* The landmark video (_change_np_img_size, dataloader_sample.py:153-179, in model range):
 *   centres [B, frames, points, 2] int32 (x, y) disc centres on the canvas, any value (off-canvas parts clip); points <= 1024
 *   half_width [2 * radius + 1] int32: row cy + dy of a disc spans cx - half_width[dy + radius] .. cx + half_width[dy + radius]
 *              (negative: no pixel in that row); radius <= 31.  The caller states the scan-conversion rule (OpenCV's for cv2.circle).
 *   out [B, 3, frames, canvas, canvas] fp32: +1 inside any disc, -1 outside, the three channels equal. */
int mtv_frames_discs(const int32_t* centres, const int32_t* half_width, float* out, int batch, int frames, int points, int radius,
                     int canvas, void* stream);
/* Decoded frames to what the loop stores and chains (sample.py:385-398, 402, 349-360):
 *   decoded [B * frames, 3, res, res] fp32, unclamped (mtv_ae_decode's output); s = (1 + min(max(v, -1), 1)) * 127.5 (a NaN reads as -1)
 *   frames_u8 [B, frames, res, res, 3]: s truncated to 8 bits
 *   last_u8 [B, res, res, 3] or NULL: the last frame of every clip, s rounded half to even (np.rint) and clipped to 0..255
 *   next_ref [B, 3, frames, res, res] fp32 or NULL: last_u8 / 255 * 2 - 1 (IEEE division) repeated over the frames: the video
 *            whose extract is the next chunk's image_cond.
 * last_u8 and next_ref are requested together or not at all. */
int mtv_frames_finish(const float* decoded, uint8_t* frames_u8, uint8_t* last_u8, float* next_ref, int batch, int frames, int res,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTV_HIP_H */
