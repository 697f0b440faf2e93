/* mtv_hip_debug.h -- testing, self-test and diagnostic entry points of libmtv_hip.so (product surface: mtv_hip.h).  The MTV_* variables of README.md
 * "Run-time switches" and the process-wide setters below are read ONCE PER CONTEXT, at its creation: setter, then environment, then default.  A setter
 * acts on contexts created afterwards (mutex-guarded); its "off" value clears the override.  A context never changes its options. */
#ifndef MTV_HIP_DEBUG_H
#define MTV_HIP_DEBUG_H

#include "mtv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A context's options as NAME=value lines in the order of README.md's table (a forced tile as "MT,NT,KS", 0 = off).  ctx == NULL: what a context
 * created now would get (needs no device).  MTV_ERR_INVALID when the text and its terminating 0 do not fit into `cap` bytes. */
int mtv_debug_options_dump(const mtv_ctx* ctx, char* buf, int cap);

/* Testing aids: contexts created after mtv_debug_resident_cus(n) plan for n co-resident CUs (0 = the device's count / MTV_RESIDENT_CUS);
 * mtv_debug_arm_fault makes the NEXT mtv_forward / mtv_ddim_sample on this context end with a launch that raises the fault word exactly as a
 * timed-out poll does (the caller-side path -- same-call detection with strict=True, stickiness -- is then testable without a real time-out). */
int mtv_debug_resident_cus(int n);
int mtv_debug_arm_fault(mtv_ctx* ctx);
/* Test/debug: copy an internal activation (token-major [B, L_level, C]) to `dst` (device or host).
 * Names: "in<i>", "mid", "out<i>" = result after the cross-plane attention of that stage. */
int mtv_debug_tap(mtv_ctx* ctx, const char* name, float* dst, int64_t dst_cap_floats, int* tokens_out, int* channels_out);
/* Diagnostic build only (conv.hip compiled with -DMTV_ABLATE=64, MTV_STAMPS=1 in the environment): one sampler step
 * with plain launches; the in-kernel phase timestamps of four sampled workgroups per conv are written to `path`. */
int mtv_debug_stamps(mtv_ctx* ctx, int batch, const char* path, void* stream);

/* Forced tiles (testing aids): every conv the family can run uses that tile instead of the tuned choice; mt / wm = 0 = off again.
 *   lds  k_conv_lds<wm, wn> (csrc/conv.hip: wave tile 16 wm x 16 wn, workgroup 2 x 2 waves);
 *   b3   the split-bf16 pair k_x3_prep + k_conv_x3<mt, nt> (csrc/conv_x3.hip: workgroup tile 32 mt x 64 nt) with ks = 1 | 2 | 4 | 8 K slices (convs with
 *        fewer than 6 ks 32-channel chunks keep one slice), any row count;
 *   win  every 3x3 conv (ResBlock in_layers / out_layers, unet.py:131-167) on k_conv_win<mt, nt> (csrc/deep.hip: row tile 16 mt x column tile 16 nt, the
 *        transformed input window staged in LDS once), ks = 1 | 2 | 4 K slices that meet in the plan's split-K slab on the convs that can take them;
 *   pw   every 1x1 conv on identity rows (the attention blocks' qkv / proj_out, unet.py:234,253) on k_conv_pw<mt, ntw> (csrc/deep.hip: 16 mt rows
 *        normalised once into LDS, ntw = 1 | 2), `waves` of its 8 waves multiplying (8, or 6 / 4 / 2 at ntw = 1: column tiles of 16 ntw waves). */
int mtv_debug_force_lds(int wm, int wn);
int mtv_debug_force_b3(int mt, int nt, int ks);
int mtv_debug_force_win(int mt, int nt);
int mtv_debug_force_win_ks(int mt, int nt, int ks);
int mtv_debug_force_pw(int mt, int ntw);
int mtv_debug_force_pw_waves(int mt, int ntw, int waves);
/* QK^T of k_attention on the bf16 matrix pipe through a three-term split of q and k at f32 accuracy (QB = 1: the 8-wave shapes of d = 16 / 32 / 64; PV
 * stays on the f32 instruction): 1 on, 0 off, -1 back to the default / MTV_ATT_QB. */
int mtv_debug_attention_qb(int mode);
/* Which convolution kernels the levels of at most 128 tokens per clip run on (batch <= 2): 1 = the K-sliced kernels of csrc/deep.hip (k_deep_conv: the
 * consumers add the producers' partial slabs and compute the GroupNorm statistics themselves), 0 = k_conv everywhere, -1 = back to the default (on) /
 * MTV_DEEP.  Replaces the same reference code either way (MToV/models/ddpm/unet.py:178-207, 234, 253).  The parity tests run both. */
int mtv_debug_deep(int mode);
/* Variants of the deep levels' dataflow (every variant meets the parity bars, the default is the fastest measured): a bit mask of
 *   MTV_DEEP_OPT_NO_FUSED_ATTN  k_attention + a proj_out conv instead of the fused k_deep_attn (implies the three-launch form below);
 *   MTV_DEEP_OPT_NO_BLOCK       k_deep_finalize + qkv conv + k_deep_attn instead of the one-launch k_deep_block (csrc/block.hip);
 *   MTV_DEEP_OPT_BLOCK_ALL      k_deep_block for EVERY attention block of the deep levels it can run, not only where it measures faster
 *                               (by default: 32-token blocks and [128 x 256]; at [128 x 512] the three-launch form is faster);
 *   MTV_DEEP_OPT_FIN_PASS       a separate k_deep_finalize pass wherever a consumer needs a deep tensor as ONE plain tensor, instead of the
 *                               completion inside the producing kernel by data-tagged granules;
 * -1 = back to the defaults / MTV_DEEP_NO_ATTN, MTV_DEEP_NO_BLOCK, MTV_DEEP_BLOCK_ALL, MTV_DEEP_FIN_PASS.  Bits 1, 2 and 4 named three variants
 * that measured slower and are retired (their measurements stay in profiles/ and in git log): a mask with one of them is MTV_ERR_INVALID. */
#define MTV_DEEP_OPT_NO_FUSED_ATTN 8
#define MTV_DEEP_OPT_NO_BLOCK 16
#define MTV_DEEP_OPT_BLOCK_ALL 32
#define MTV_DEEP_OPT_FIN_PASS 64
int mtv_debug_deep_options(int mask);
/* Form of the fused attention + proj_out kernel k_deep_attn: 1 = one head per workgroup with 128-column proj slices wherever that form exists (C a
 * multiple of 128, at most 8 heads, a power of two), 2 = head groups everywhere (what MTV_DEEP_ATTN_HPW=2 selects), -1 = back to the environment /
 * the rule: one head per workgroup at the 128-token blocks of 64-wide heads, head groups elsewhere. */
int mtv_debug_deep_attn_form(int form);

/* Host-only self-test (needs no device): the conv kernels compute their 3x3 / nearest-upsample gather indices arithmetically on the tri-plane grid
 * (planes xy R x R | yt T x R | xt T x R per level, i.e. the slicing of unet.py:1039-1053 and the Upsample/conv padding of unet.py:531-598); this
 * checks that arithmetic against explicitly constructed index tables for every level of a (res, frames, n_levels) geometry. Returns 0 when all agree,
 * else 1 + the first level that does not (<0: bad arguments). */
int mtv_selftest_geometry(int res, int frames, int n_levels);
/* Host-only self-test (needs no device) of the row tables of the deep levels (csrc/deep.hip: levels of at most 128 tokens per clip, whose convs stage
 * a whole row group of a channel slice in LDS and address it through a per-launch table of LDS rows): every entry -- all row groupings, 3x3 and 1x1,
 * same-level and nearest-upsampled source -- is checked against the explicitly constructed im2col tables (unet.py:178-207 ResBlock convs incl. the
 * Upsample of :531-598). 0 = all agree, else 1 + the first level that does not (<0: bad arguments). */
int mtv_selftest_deep(int res, int frames, int n_levels);
/* Host-only self-test of k_deep_block's work split (csrc/block.hip: one attention block of a deep level -- unet.py:210-300, 303-326 -- in one launch):
 * for a level of `tokens` tokens (<= 128), `channels`, `heads`, `batch` clips it configures the cluster (K slices x row groups), and checks that the
 * grid stays within the residency bound, LDS within 160 KB, that stage 2 deals every row pair to exactly one workgroup and stage 3 every (query tile,
 * column part) to exactly one, and that every granule offset of the three scratch buffers lies inside its allocation. Returns 0 when all hold, 1 when
 * the shape is (legitimately) not configurable, > 1 on a violated invariant, < 0 on bad arguments. */
int mtv_selftest_block(int tokens, int channels, int heads, int batch);
/* Host-only self-test of k_conv_win's window arithmetic (csrc/deep.hip: the contiguous range of source tokens a row tile of a 3x3 conv stages in LDS):
 * for row tiles of 16 and 32 tokens at every level, same-level and nearest-upsampled source, the window lies inside the source tensor and contains the
 * source token of every tap of every output row (the taps of mtv_debug_gather_index). 0 = ok, else 1 + the first level that fails (<0: bad arguments). */
int mtv_selftest_win(int res, int frames, int n_levels);
/* Host-only self-test of k_conv_win's packed weight operand (csrc/deep.hip, csrc/mtv_internal.h WinPack: the 3x3 conv matrix -- unet.py:131-167
 * in_layers / out_layers, with the fused 1x1 skip_connection of :169-176 -- rewritten per (column tile, K slice, wave) in the order the kernel's K
 * loop consumes it). For the tile <mt, nt> with ks K slices and a conv of cmain tapped + cskip fused-skip input channels and n output channels: the
 * packed-index -> (row, column) map reaches every element of the matrix exactly once, every other packed position is zero padding (the chunks past a
 * wave's last), and the offsets the kernel computes land on the elements its MFMA operand registers expect. 0 = ok, > 0: the violated invariant, < 0:
 * bad arguments (a tile that does not exist, a shape it cannot slice). */
int mtv_selftest_win_pack(int mt, int nt, int ks, int cmain, int cskip, int n);
/* The arithmetic itself, for tests: source token of tap (ky, kx in 0..2) at output token `tok` of a level with planes res x res | frames x res |
 * frames x res; up != 0: the source is the (res/2, frames/2) level under a nearest x2 upsample. Returns -1 for zero padding, else source_token | plane
 * << 28. */
int mtv_debug_gather_index(int res, int frames, int tok, int ky, int kx, int up);

/* keep != 0: every later forward also keeps copies of two tensors it otherwise updates in place ("after_pos_conv", "layer_0").
 * mtv_hubert_debug_tap reads a tensor of the LAST forward: those two, or "extract_features" (the conv encoder's output,
 * [batch, T, conv_dim[n_conv - 1]]).  dst: host or device, cap floats; rows_out = batch T of that forward. */
int mtv_hubert_debug_keep(mtv_ctx* ctx, int keep);
int mtv_hubert_debug_tap(mtv_ctx* ctx, const char* name, float* dst, int64_t cap, int* rows_out, int* channels_out);

#ifdef __cplusplus
}
#endif
#endif /* MTV_HIP_DEBUG_H */
