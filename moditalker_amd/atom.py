"""AToM, the audio-to-motion stage in front of MToV, on the HIP library: look-alikes of the reference's MotionDecoder
(AToM/model/model.py:242-470) and GaussianDiffusion (AToM/model/diffusion.py:40-250, 462-550).

HuBERT features [B, 2 L, cond_feature_dim] and first-frame landmarks repeated over the horizon [B, L, 204] in, a landmark
residual sequence [B, L, 204] out.  Both classes are parameter holders with the reference's state_dict keys and shapes (a
reference checkpoint loads with strict=True); the arithmetic runs in libmtv_hip.so (csrc/atom.hip): `mtv_atom_forward`,
`mtv_atom_guided_forward`, `mtv_atom_ddim_sample`, `mtv_atom_long_ddim_sample` (motion longer than one horizon:
diffusion.py:252-301).  Inference only: training, the ancestral loop and cond_drop_prob other than 0 or 1 raise.  No CPU fallback.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._context import HipContextMixin
from .ddpm import ddim_step_table, ddim_time_pairs

NFEATS = 204                      # 68 landmarks x 3; forward() splits them 0:17 | 17:48 | 48:68
DDIM_STEPS = 50                   # diffusion.py:213-219 hard-wires 50 sampling steps, eta = 1


def make_beta_schedule(schedule: str, n_timestep: int, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3) -> np.ndarray:
    """AToM/model/utils.py:67-99 (fp64).  Unlike MToV's, "cosine" divides alpha_bar by (1 + s) BEFORE the pi / 2 factor in one
    expression and clips to [0, 0.999]; the four names mean the same ramps."""
    ramp = dict(steps=n_timestep, dtype=torch.float64)
    if schedule == "linear":
        betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, **ramp) ** 2
    elif schedule == "cosine":
        ts = torch.arange(n_timestep + 1, dtype=torch.float64) / n_timestep + cosine_s
        abar = torch.cos(ts / (1 + cosine_s) * np.pi / 2).pow(2)
        abar = abar / abar[0]
        betas = (1 - abar[1:] / abar[:-1]).clamp(0, 0.999)
    elif schedule == "sqrt_linear":
        betas = torch.linspace(linear_start, linear_end, **ramp)
    elif schedule == "sqrt":
        betas = torch.linspace(linear_start, linear_end, **ramp) ** 0.5
    else:
        raise ValueError(f"schedule '{schedule}' unknown.")
    return betas.numpy()


# ------------------------------------------------------------------------------------------------------------------
# parameter holders: the module tree whose state_dict() is the reference's, key for key
# ------------------------------------------------------------------------------------------------------------------
class _Rotary(nn.Module):
    def __init__(self, dim: int, theta: float = 10000.0):
        super().__init__()
        self.register_buffer("freqs", 1.0 / (theta ** (torch.arange(0, dim, 2)[: dim // 2].float() / dim)))


def _slots(*mods):
    """nn.Sequential whose parameter-free positions (activations, the sinusoid, Rearrange) are placeholders."""
    return nn.Sequential(*[nn.Identity() if m is None else m for m in mods])


class _EncoderLayer(nn.Module):
    def __init__(self, d, heads, ff, rotary):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, heads, batch_first=True)
        self.linear1 = nn.Linear(d, ff)
        self.linear2 = nn.Linear(ff, d)
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)
        self.rotary = rotary


class _FiLM(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.block = _slots(None, nn.Linear(d, 2 * d))


class _DecoderLayer(nn.Module):
    def __init__(self, d, heads, ff, rotary):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, heads, batch_first=True)
        self.multihead_attn = nn.MultiheadAttention(d, heads, batch_first=True)
        self.linear1 = nn.Linear(d, ff)        # held, never run: the norm_first path has no feed-forward block
        self.linear2 = nn.Linear(ff, d)
        self.linear3 = nn.Linear(d, 2 * d)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d), nn.LayerNorm(d), nn.LayerNorm(d)
        self.film1, self.film2, self.film3 = _FiLM(d), _FiLM(d), _FiLM(d)
        self.rotary = rotary


class _Stack(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.stack = nn.ModuleList(layers)


class MotionDecoder(HipContextMixin, nn.Module):
    """Same constructor kwargs and state_dict as the reference's MotionDecoder; forward / guided_forward run on the HIP library."""

    _destroy = "mtv_atom_destroy"

    def __init__(self, nfeats: int, seq_len: int = 150, latent_dim: int = 256, ff_size: int = 1024, num_layers: int = 4,
                 num_heads: int = 4, dropout: float = 0.1, cond_feature_dim: int = 1024, activation=None, use_rotary=True,
                 max_batch: int = 1, **kwargs) -> None:
        super().__init__()
        if not use_rotary:
            raise NotImplementedError("use_rotary=False (absolute positional encoding) is not built: every shipped AToM configuration is rotary")
        if activation is not None and getattr(activation, "__name__", "") != "gelu":
            raise NotImplementedError("activation must be F.gelu (exact erf), the reference's default and only configuration")
        if nfeats != NFEATS:
            raise NotImplementedError("nfeats must be 204: forward() splits 68 x 3 landmarks")
        d = latent_dim
        self.cfg = dict(nfeats=nfeats, seq_len=seq_len, latent_dim=d, ff_size=ff_size, num_layers=num_layers, num_heads=num_heads,
                        cond_feature_dim=cond_feature_dim)
        self.dropout_p = float(dropout)      # identity in eval; forward() refuses training mode with dropout
        self.max_batch = int(max_batch)
        self.rotary = _Rotary(d)
        self.time_mlp = _slots(None, nn.Linear(d, 4 * d), None)
        self.to_time_cond = _slots(nn.Linear(4 * d, d))
        self.to_time_tokens = _slots(nn.Linear(4 * d, 2 * d), None)
        self.face_mlp = _slots(nn.Linear(96, 4 * d), None)             # face_mlp / to_face_*: held, never run
        self.to_face_cond = _slots(nn.Linear(4 * d, d))
        self.to_face_tokens = _slots(nn.Linear(4 * d, 2 * d), None)
        self.null_cond_embed = nn.Parameter(torch.randn(1, 2 * seq_len, d))
        self.null_cond_hidden = nn.Parameter(torch.randn(1, d))
        self.face_null_cond_embed = nn.Parameter(torch.randn(1, seq_len, d))
        self.norm_cond = nn.LayerNorm(d)
        self.input_projection = nn.Linear(nfeats, d)                   # held, never run
        self.input_projection_lip = nn.Linear(37 * 3, d)
        self.input_projection_wo_lip = nn.Linear(31 * 3, d)
        enc = lambda: nn.Sequential(*[_EncoderLayer(d, num_heads, ff_size, self.rotary) for _ in range(2)])
        self.cond_encoder, self.face_encoder, self.pos_encoder = enc(), enc(), enc()      # pos_*: held, never run
        self.cond_projection = nn.Linear(cond_feature_dim, d)
        self.face_projection = nn.Linear(nfeats, d)
        self.pos_projection = nn.Linear(198, d)
        hid = lambda: _slots(nn.LayerNorm(d), nn.Linear(d, d), None, nn.Linear(d, d))
        self.non_attn_cond_projection, self.non_attn_face_projection, self.non_attn_pos_projection = hid(), hid(), hid()
        self.seqTransDecoder = _Stack([_DecoderLayer(d, num_heads, ff_size, self.rotary) for _ in range(num_layers)])
        self.final_layer = nn.Linear(2 * d, nfeats)
        self._ctx: Optional[C.c_void_p] = None
        self._key = None
        self._fingerprint = None

    def tables(self):
        """(rot [3 L + 2, D / 2, 2] cos | sin, time_freqs [D / 2]) in fp32 on the CPU, evaluated as the reference does:
        position.float() * freqs (rotary_embedding_torch.py:117-132) and exp(arange * -log(10000) / (half - 1)) (utils.py:41-48)."""
        d, L = self.cfg["latent_dim"], self.cfg["seq_len"]
        freqs = self.rotary.freqs.detach().float().cpu()
        ang = torch.arange(3 * L + 2).type(freqs.dtype)[:, None] * freqs[None, :]
        rot = torch.stack((ang.cos(), ang.sin()), dim=-1).contiguous()
        half = d // 2
        tf = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1))).float().contiguous()
        return rot, tf

    def _context(self, device, B):
        if device.type != "cuda":
            raise _lib.MtvError("MotionDecoder runs only on a HIP device (tensor is on %s); there is no CPU fallback" % device)
        if self.training and self.dropout_p != 0.0:
            raise NotImplementedError("dropout != 0 in training mode is the training path; call .eval()")
        lib = _lib.load()
        if self._ctx is None or self._key is None or self._key[0] != device or B > self._key[1]:
            self._release()
            cap = max(B, self.max_batch)
            cfg = _lib.MtvAtomConfig(self.cfg["nfeats"], self.cfg["seq_len"], self.cfg["latent_dim"], self.cfg["ff_size"],
                                     self.cfg["num_layers"], self.cfg["num_heads"], self.cfg["cond_feature_dim"], cap)
            with torch.cuda.device(device):
                ctx = C.c_void_p()
                _lib.check(lib.mtv_atom_create(C.byref(cfg), C.byref(ctx)), "mtv_atom_create")
            self._ctx, self._key, self._fingerprint = ctx, (device, cap), None
        fp = self._weights_fingerprint()
        if fp != self._fingerprint:
            self._upload_weights(self._ctx, device)
            with torch.cuda.device(device):
                rot, tf = self.tables()
                _lib.check(lib.mtv_atom_set_tables(self._ctx, C.c_void_p(rot.data_ptr()), rot.shape[0], C.c_void_p(tf.data_ptr())),
                           "mtv_atom_set_tables")
            self._fingerprint = fp
        return self._ctx

    def check_inputs(self, x, face, cond_embed):
        """ValueError for a wrong-shaped tensor, before any launch."""
        L, cf = self.cfg["seq_len"], self.cfg["cond_feature_dim"]
        if x.dim() != 3 or tuple(x.shape[1:]) != (L, NFEATS):
            raise ValueError(f"x must be [B,{L},{NFEATS}]; got {tuple(x.shape)}")
        B = x.shape[0]
        if tuple(face.shape) != (B, L, NFEATS):
            raise ValueError(f"face must be [{B},{L},{NFEATS}]; got {tuple(face.shape)}")
        if tuple(cond_embed.shape) != (B, 2 * L, cf):
            raise ValueError(f"cond_embed must be [{B},{2 * L},{cf}]; got {tuple(cond_embed.shape)}")
        return B

    def _prep(self, x, face, cond_embed, times):
        B = self.check_inputs(x, face, cond_embed)
        if times.dim() != 1 or times.shape[0] != B:
            raise ValueError(f"times must be [{B}]; got {tuple(times.shape)}")
        dev = x.device
        ctx = self._context(dev, B)
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
        return B, dev, ctx, f32(x), f32(face), f32(cond_embed), times.to(device=dev, dtype=torch.int64).contiguous()

    @torch.no_grad()
    def forward(self, x_pos, x, face, cond_embed, times, cond_drop_prob: float = 0.0):
        """model.py:391-470.  x_pos is accepted and unused, as in the reference."""
        if cond_drop_prob not in (0, 1):
            raise NotImplementedError("cond_drop_prob must be exactly 0 or 1: a random keep mask is the training path")
        B, dev, ctx, xf, ff, cf, tt = self._prep(x, face, cond_embed, times)
        out = torch.empty(B, self.cfg["seq_len"], NFEATS, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mtv_atom_forward(ctx, xf.data_ptr(), ff.data_ptr(), cf.data_ptr(), tt.data_ptr(), int(cond_drop_prob),
                                                    out.data_ptr(), B, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mtv_atom_forward")
        return out.type(x.dtype)

    @torch.no_grad()
    def guided_forward(self, x_pos, x, face, cond_embed, times, guidance_weight):
        """model.py:385-389: unc + (conditioned - unc) * guidance_weight, both passes as one batch."""
        B, dev, ctx, xf, ff, cf, tt = self._prep(x, face, cond_embed, times)
        out = torch.empty(B, self.cfg["seq_len"], NFEATS, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mtv_atom_guided_forward(ctx, xf.data_ptr(), ff.data_ptr(), cf.data_ptr(), tt.data_ptr(), float(guidance_weight),
                                                           out.data_ptr(), B, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                       "mtv_atom_guided_forward")
        return out.type(x.dtype)


class GaussianDiffusion(nn.Module):
    """diffusion.py:40-114 (constructor, schedule buffers) and the sampling entry points ddim_sample / render_sample."""

    def __init__(self, model, horizon, repr_dim, n_timestep=1000, schedule="linear", loss_type="l1", clip_denoised=True,
                 predict_epsilon=True, guidance_weight=3, use_p2=False, cond_drop_prob=0.2):
        super().__init__()
        self.horizon = horizon
        self.transition_dim = repr_dim
        self.model = model
        self.master_model = copy.deepcopy(model)      # the EMA copy: part of the reference's state_dict, not used when sampling
        self.cond_drop_prob = cond_drop_prob
        betas = torch.Tensor(make_beta_schedule(schedule=schedule, n_timestep=n_timestep))      # fp32 from here on, as the reference
        alphas = 1.0 - betas
        ac = torch.cumprod(alphas, axis=0)
        ac_prev = torch.cat([torch.ones(1), ac[:-1]])
        self.n_timestep = int(n_timestep)
        self.clip_denoised = clip_denoised
        self.predict_epsilon = predict_epsilon
        self.guidance_weight = guidance_weight
        reg = self.register_buffer
        reg("betas", betas)
        reg("alphas_cumprod", ac)
        reg("alphas_cumprod_prev", ac_prev)
        reg("sqrt_alphas_cumprod", torch.sqrt(ac))
        reg("sqrt_one_minus_alphas_cumprod", torch.sqrt(1.0 - ac))
        reg("log_one_minus_alphas_cumprod", torch.log(1.0 - ac))
        reg("sqrt_recip_alphas_cumprod", torch.sqrt(1.0 / ac))
        reg("sqrt_recipm1_alphas_cumprod", torch.sqrt(1.0 / ac - 1))
        pv = betas * (1.0 - ac_prev) / (1.0 - ac)
        reg("posterior_variance", pv)
        reg("posterior_log_variance_clipped", torch.log(torch.clamp(pv, min=1e-20)))
        # (numpy's sqrt, as the reference: torch.sqrt rounds a few of these differently and the buffers are pinned bit for bit)
        reg("posterior_mean_coef1", betas * torch.from_numpy(np.sqrt(ac_prev.numpy())) / (1.0 - ac))
        reg("posterior_mean_coef2", (1.0 - ac_prev) * torch.from_numpy(np.sqrt(alphas.numpy())) / (1.0 - ac))
        self.p2_loss_weight_k = 1
        self.p2_loss_weight_gamma = 0.5 if use_p2 else 0
        reg("p2_loss_weight", (self.p2_loss_weight_k + ac / (1 - ac)) ** -self.p2_loss_weight_gamma)
        self.loss_type = loss_type

    def step_table(self):
        """The 50 DDIM steps' scalars (diffusion.py:221-245) as the library's step records; returns (steps, n_draws)."""
        pairs = ddim_time_pairs(self.n_timestep, DDIM_STEPS)
        return ddim_step_table(self.alphas_cumprod, self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod, pairs, 1.0)

    @torch.no_grad()
    def ddim_sample(self, shape, face, x_pos, cond, noise=None, strict=None, **kwargs):
        """diffusion.py:212-250.  `noise` (appended kwarg, as in DDPM.sample): x_T first, then one draw per non-final step --
        a list / tensor [1 + 49, *shape]; None draws them from torch's generator in that order.  `strict` is accepted for
        signature parity with DDPM.sample: this path has no in-launch hand-offs to check."""
        if not self.clip_denoised:
            raise NotImplementedError("clip_denoised=False is not built (every AToM configuration clamps x_start)")
        dev = self.betas.device
        model = self.model
        shape = tuple(int(s) for s in shape)
        steps, n_draws = self.step_table()
        noise = self._noise(shape, noise, n_draws, dev)
        face, cond = face.to(dev), cond.to(dev)
        x = noise[0].clone()
        B = model.check_inputs(x, face, cond)
        ctx = model._context(dev, B)
        ff = face.to(torch.float32).contiguous()
        cf = cond.to(torch.float32).contiguous()
        draws = noise[1:]
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(lib.mtv_atom_set_guidance(ctx, float(self.guidance_weight)), "mtv_atom_set_guidance")
            _lib.check(lib.mtv_atom_ddim_sample(ctx, x.data_ptr(), ff.data_ptr(), cf.data_ptr(), draws.data_ptr() if n_draws else None, int(draws.shape[0]),
                                                steps, len(steps), B, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mtv_atom_ddim_sample")
        return x

    @staticmethod
    def _noise(shape, noise, n_draws, dev):
        """The samplers' `noise` argument as one fp32 tensor [>= 1 + n_draws, *shape] on `dev`; ValueError for any other shape."""
        if noise is None:
            noise = [torch.randn(shape, device=dev) for _ in range(1 + n_draws)]
        if isinstance(noise, (list, tuple)):
            noise = torch.stack([n.to(dev) for n in list(noise)[: 1 + n_draws]])
        noise = noise.to(device=dev, dtype=torch.float32).contiguous()
        if noise.shape[0] < 1 + n_draws or tuple(noise.shape[1:]) != shape:
            raise ValueError(f"noise must be [{1 + n_draws},{','.join(map(str, shape))}] (x_T, then one draw per non-final step); got {tuple(noise.shape)}")
        return noise

    def long_guidance_weights(self) -> np.ndarray:
        """diffusion.py:269: the guidance weight of each of the 50 steps of long_ddim_sample, a ramp from 0 that reaches
        guidance_weight half way.  float32: the reference multiplies an fp32 tensor by the (fp64) scalar, which rounds it so."""
        return np.clip(np.linspace(0, self.guidance_weight * 2, DDIM_STEPS), None, self.guidance_weight).astype(np.float32)

    @torch.no_grad()
    def long_ddim_sample(self, shape, face, x_pos, cond, noise=None, strict=None, n_steps=None, **kwargs):
        """diffusion.py:252-301, the EDGE-style sampler for motion longer than one horizon, with the signature of ddim_sample
        (the reference's own method predates `face` / `x_pos` and cannot be called as written).  shape [B, L, 204]: B windows that
        overlap their neighbours by L / 2 frames are denoised as one batch; after every step but the last, the first half of
        window b is overwritten with the second half of window b - 1, and the guidance weight ramps up over the first 25 steps
        (long_guidance_weights).  B == 1 is ddim_sample (:262-263).  `noise` as in ddim_sample: [1 + 49, B, L, 204], x_T first.
        `n_steps` (appended kwarg, for diagnosis and tests): run only the first n_steps < 50 steps and return x_t there, after
        the update and the stitch."""
        shape = tuple(int(s) for s in shape)
        if shape[0] == 1:
            if n_steps is not None:
                raise ValueError("n_steps is an argument of the multi-window sampler; one window is ddim_sample")
            return self.ddim_sample(shape, face, x_pos, cond, noise=noise, strict=strict, **kwargs)
        if not self.clip_denoised:
            raise NotImplementedError("clip_denoised=False is not built (every AToM configuration clamps x_start)")
        if len(shape) != 3 or shape[1] % 2:
            raise ValueError(f"long_ddim_sample needs an even horizon (windows overlap by half, diffusion.py:276-277); got shape {shape}")
        dev = self.betas.device
        model = self.model
        steps, n_draws = self.step_table()
        n_run = len(steps) if n_steps is None else int(n_steps)
        if not 1 <= n_run <= len(steps):
            raise ValueError(f"n_steps must be in [1, {len(steps)}]; got {n_steps}")
        noise = self._noise(shape, noise, n_draws, dev)
        face, cond = face.to(dev), cond.to(dev)
        x = noise[0].clone()
        B = model.check_inputs(x, face, cond)
        weights = np.ascontiguousarray(self.long_guidance_weights())
        ctx = model._context(dev, B)
        ff = face.to(torch.float32).contiguous()
        cf = cond.to(torch.float32).contiguous()
        draws = noise[1:]
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mtv_atom_long_ddim_sample(
                ctx, x.data_ptr(), ff.data_ptr(), cf.data_ptr(), draws.data_ptr(), int(draws.shape[0]), steps, n_run,
                weights.ctypes.data_as(C.POINTER(C.c_float)), B, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mtv_atom_long_ddim_sample")
        return x

    @torch.no_grad()
    def render_sample(self, face3d_helper, shape, kpt, front, x_pos, gt, cond, epoch, render_out, fk_out=None, name=None, sound=True,
                      mode="normal", noise=None, constraint=None, sound_folder="ood_sliced", start_point=None, render=True, filename=None,
                      checkpoint=None, slice=None):
        """diffusion.py:462-550: the live part is ddim_sample(shape, kpt, x_pos, cond) moved to the CPU."""
        return self.ddim_sample(shape, kpt, x_pos, cond, noise=noise).detach().cpu()

    def _training(self, *a, **k):
        raise NotImplementedError("moditalker_amd.GaussianDiffusion is the sampling path (ddim_sample / long_ddim_sample / render_sample); training, "
                                  "q_sample losses and the ancestral p_sample loop are not built")

    forward = loss = p_losses = p_sample = p_sample_loop = inpaint_loop = long_inpaint_loop = conditional_sample = _training
