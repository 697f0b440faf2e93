"""HuBERT audio features on the HIP library: a look-alike of transformers' HubertModel for the configuration the reference
uses (data/data_utils/preprocess/process_audio.py:9-55 loads facebook/hubert-large-ls960-ft).

A normalised 16 kHz waveform [B, n] in, `last_hidden_state` [B, T, hidden] out: seven layer-normed Conv1d layers, LayerNorm +
projection, the weight-normed grouped positional conv, the stable-layer-norm transformer stack.  The class is a parameter
holder with transformers' state_dict keys and shapes (tests/golden/hubert_large_keys.txt), so `load_state_dict` takes a
HubertModel state dict; `load_checkpoint_dict` takes a published checkpoint's dict as it is.  The arithmetic runs in
libmtv_hip.so (csrc/hubert.hip): `mtv_hubert_forward`, `mtv_hubert_normalize`.  Inference only; what is not built raises
NotImplementedError with the reason.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._context import HipContextMixin

# The published config.json of facebook/hubert-large-ls960-ft, WRITTEN FROM MEMORY: the file cannot be fetched where this was
# written.  Every value the forward depends on lives in this one dict; compare it with the checkpoint's own config.json
# before trusting features from real weights (a wrong shape fails at load_state_dict, a wrong eps or flag does not).
HUBERT_LARGE_CONFIG = dict(
    hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
    conv_dim=(512, 512, 512, 512, 512, 512, 512), conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2),
    feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True, feat_proj_layer_norm=True,
    num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
    hidden_act="gelu", feat_extract_activation="gelu",
)
CLIP_SAMPLES = 320 * 1000 - 320 + 400      # process_audio.py:24-36: the longest clip the reference's loop hands the model

BaseModelOutput = namedtuple("BaseModelOutput", ["last_hidden_state", "extract_features"])


def num_frames(n_samples: int, conv_kernel=HUBERT_LARGE_CONFIG["conv_kernel"], conv_stride=HUBERT_LARGE_CONFIG["conv_stride"]) -> int:
    """Frames of a clip: (n - k) // s + 1 through every conv layer; 0 when a layer has no valid window."""
    n = int(n_samples)
    for k, s in zip(conv_kernel, conv_stride):
        if n < k:
            return 0
        n = (n - k) // s + 1
    return n


def convert_checkpoint_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A published checkpoint's dict -> this class's keys: a leading `hubert.` goes, `lm_head.*` and `masked_spec_embed` are
    dropped, the positional conv's `weight_g` / `weight_v` (torch.nn.utils.weight_norm) become
    `parametrizations.weight.original0` / `original1` (torch.nn.utils.parametrizations.weight_norm: same tensors, new names)."""
    out = {}
    for k, v in sd.items():
        if k.startswith("hubert."):
            k = k[len("hubert."):]
        if k.startswith("lm_head.") or k == "masked_spec_embed":
            continue
        if k.endswith(".conv.weight_g"):
            k = k[: -len("weight_g")] + "parametrizations.weight.original0"
        elif k.endswith(".conv.weight_v"):
            k = k[: -len("weight_v")] + "parametrizations.weight.original1"
        out[k] = v
    return out


# ------------------------------------------------------------------------------------------------------------------
# parameter holders: the module tree whose state_dict() is transformers', key for key
# ------------------------------------------------------------------------------------------------------------------
class _ConvLayer(nn.Module):
    def __init__(self, cin, cout, k, s):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, kernel_size=k, stride=s, bias=True)
        self.layer_norm = nn.LayerNorm(cout)


class _FeatureEncoder(nn.Module):
    def __init__(self, dims, kernels, strides):
        super().__init__()
        self.conv_layers = nn.ModuleList([_ConvLayer(dims[i - 1] if i else 1, dims[i], kernels[i], strides[i]) for i in range(len(dims))])


class _FeatureProjection(nn.Module):
    def __init__(self, cin, hidden, eps):
        super().__init__()
        self.layer_norm = nn.LayerNorm(cin, eps=eps)
        self.projection = nn.Linear(cin, hidden)


class _PosConv(nn.Module):
    def __init__(self, hidden, taps, groups):
        super().__init__()
        self.conv = nn.utils.parametrizations.weight_norm(nn.Conv1d(hidden, hidden, kernel_size=taps, padding=taps // 2, groups=groups),
                                                          name="weight", dim=2)


class _Attention(nn.Module):
    def __init__(self, hidden):
        super().__init__()
        self.k_proj, self.v_proj = nn.Linear(hidden, hidden), nn.Linear(hidden, hidden)
        self.q_proj, self.out_proj = nn.Linear(hidden, hidden), nn.Linear(hidden, hidden)


class _FeedForward(nn.Module):
    def __init__(self, hidden, inter):
        super().__init__()
        self.intermediate_dense = nn.Linear(hidden, inter)
        self.output_dense = nn.Linear(inter, hidden)


class _EncoderLayer(nn.Module):
    def __init__(self, hidden, inter, eps):
        super().__init__()
        self.attention = _Attention(hidden)
        self.layer_norm = nn.LayerNorm(hidden, eps=eps)
        self.feed_forward = _FeedForward(hidden, inter)
        self.final_layer_norm = nn.LayerNorm(hidden, eps=eps)


class _Encoder(nn.Module):
    def __init__(self, hidden, inter, layers, taps, groups, eps):
        super().__init__()
        self.pos_conv_embed = _PosConv(hidden, taps, groups)
        self.layer_norm = nn.LayerNorm(hidden, eps=eps)
        self.layers = nn.ModuleList([_EncoderLayer(hidden, inter, eps) for _ in range(layers)])


class HubertModel(HipContextMixin, nn.Module):
    """HubertModel(**HUBERT_LARGE_CONFIG): transformers' HubertConfig keywords.  forward(input_values).last_hidden_state runs on
    the HIP library.  `max_samples` / `max_batch` size the workspace (a longer clip or larger batch rebuilds it)."""

    _destroy = "mtv_hubert_destroy"

    def __init__(self, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), feat_extract_norm="group",
                 conv_bias=False, do_stable_layer_norm=False, feat_proj_layer_norm=True, num_conv_pos_embeddings=128,
                 num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5, hidden_act="gelu", feat_extract_activation="gelu",
                 hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.0, layerdrop=0.1,
                 apply_spec_augment=True, max_samples: int = CLIP_SAMPLES, max_batch: int = 1, **kwargs) -> None:
        super().__init__()
        if not do_stable_layer_norm or feat_extract_norm != "layer":
            raise NotImplementedError('do_stable_layer_norm=False / feat_extract_norm="group" is the base model; only the stable-layer-norm, '
                                      "layer-normed-conv form of the large checkpoints is built")
        if not conv_bias or not feat_proj_layer_norm:
            raise NotImplementedError("conv_bias=False / feat_proj_layer_norm=False are not built (the large checkpoints set both)")
        if hidden_act != "gelu" or feat_extract_activation != "gelu":
            raise NotImplementedError("only exact-erf GELU is built, the checkpoints' activation")
        if kwargs.get("conv_pos_batch_norm"):
            raise NotImplementedError("conv_pos_batch_norm is not built (the checkpoints use the weight-normed positional conv)")
        if not (len(conv_dim) == len(conv_kernel) == len(conv_stride)) or not 1 <= len(conv_dim) <= 8:
            raise ValueError("conv_dim, conv_kernel and conv_stride must have the same length, at most 8")
        self.cfg = dict(hidden=int(hidden_size), n_layers=int(num_hidden_layers), heads=int(num_attention_heads), intermediate=int(intermediate_size),
                        conv_dim=tuple(int(v) for v in conv_dim), conv_kernel=tuple(int(v) for v in conv_kernel),
                        conv_stride=tuple(int(v) for v in conv_stride), pos_taps=int(num_conv_pos_embeddings),
                        pos_groups=int(num_conv_pos_embedding_groups), eps=float(layer_norm_eps))
        self.dropouts = tuple(float(p) for p in (hidden_dropout, attention_dropout, activation_dropout, feat_proj_dropout, layerdrop))
        self.apply_spec_augment = bool(apply_spec_augment)      # acts in training mode only, which forward() refuses
        self.max_samples, self.max_batch = int(max_samples), int(max_batch)
        self.debug_taps = False                                 # True: forward also keeps "after_pos_conv" and "layer_0" for tap()
        c = self.cfg
        self.masked_spec_embed = nn.Parameter(torch.zeros(c["hidden"]))      # spec-augment's fill vector: held for the state_dict, never read
        self.feature_extractor = _FeatureEncoder(c["conv_dim"], c["conv_kernel"], c["conv_stride"])
        self.feature_projection = _FeatureProjection(c["conv_dim"][-1], c["hidden"], c["eps"])
        self.encoder = _Encoder(c["hidden"], c["intermediate"], c["n_layers"], c["pos_taps"], c["pos_groups"], c["eps"])
        self._ctx: Optional[C.c_void_p] = None
        self._key = None
        self._fingerprint = None

    def load_checkpoint_dict(self, sd, strict: bool = True):
        """load_state_dict for a published checkpoint's dict as it is (see convert_checkpoint_dict)."""
        sd = convert_checkpoint_dict(sd)
        sd["masked_spec_embed"] = self.masked_spec_embed.detach().clone()      # (ignored in the checkpoint: the forward never reads it)
        return self.load_state_dict(sd, strict=strict)

    def num_frames(self, n_samples: int) -> int:
        return num_frames(n_samples, self.cfg["conv_kernel"], self.cfg["conv_stride"])

    def _context(self, device, B, n):
        if device.type != "cuda":
            raise _lib.MtvError("HubertModel runs only on a HIP device (tensor is on %s); there is no CPU fallback" % device)
        if self.training and (any(p != 0.0 for p in self.dropouts) or self.apply_spec_augment):
            raise NotImplementedError("dropout / layerdrop / spec-augment in training mode are the training path; call .eval()")
        lib = _lib.load()
        if self._ctx is None or self._key is None or self._key[0] != device or B > self._key[1] or n > self._key[2]:
            self._release()
            cap_b, cap_n = max(B, self.max_batch), max(n, self.max_samples)
            c = self.cfg
            cfg = _lib.MtvHubertConfig()
            cfg.hidden, cfg.n_layers, cfg.heads, cfg.intermediate, cfg.n_conv = c["hidden"], c["n_layers"], c["heads"], c["intermediate"], len(c["conv_dim"])
            for i in range(len(c["conv_dim"])):
                cfg.conv_dim[i], cfg.conv_kernel[i], cfg.conv_stride[i] = c["conv_dim"][i], c["conv_kernel"][i], c["conv_stride"][i]
            cfg.pos_taps, cfg.pos_groups, cfg.eps, cfg.max_samples, cfg.max_batch = c["pos_taps"], c["pos_groups"], c["eps"], cap_n, cap_b
            with torch.cuda.device(device):
                ctx = C.c_void_p()
                _lib.check(lib.mtv_hubert_create(C.byref(cfg), C.byref(ctx)), "mtv_hubert_create")
            self._ctx, self._key, self._fingerprint = ctx, (device, cap_b, cap_n), None
        fp = self._weights_fingerprint()
        if fp != self._fingerprint:
            self._upload_weights(self._ctx, device)
            self._fingerprint = fp
        _lib.check(lib.mtv_hubert_debug_keep(self._ctx, int(self.debug_taps)), "mtv_hubert_debug_keep")
        return self._ctx

    @torch.no_grad()
    def normalize(self, speech) -> torch.Tensor:
        """Wav2Vec2FeatureExtractor's do_normalize on the device: (x - mean) / sqrt(var + 1e-7) over the whole 1-D utterance."""
        dev = next(self.parameters()).device
        x = torch.as_tensor(np.asarray(speech, dtype=np.float32) if not torch.is_tensor(speech) else speech).to(device=dev, dtype=torch.float32).contiguous()
        if x.dim() != 1 or x.numel() < 1:
            raise ValueError(f"normalize takes one utterance [n >= 1]; got {tuple(x.shape)}")
        ctx = self._context(dev, 1, 1)
        out = torch.empty_like(x)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mtv_hubert_normalize(ctx, x.data_ptr(), x.numel(), out.data_ptr(),
                                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mtv_hubert_normalize")
        return out

    @torch.no_grad()
    def forward(self, input_values, attention_mask=None, mask_time_indices=None, output_attentions=None, output_hidden_states=None,
                return_dict=None, **kwargs):
        """input_values [B, n] (clips of one length, normalised) -> BaseModelOutput with last_hidden_state [B, T, hidden]."""
        if attention_mask is not None:
            raise NotImplementedError("attention masks / padded batches are not built: batch clips of equal length (the reference's loop does)")
        if mask_time_indices is not None:
            raise NotImplementedError("mask_time_indices is spec-augment, the training path")
        if output_attentions or output_hidden_states:
            raise NotImplementedError("output_attentions / output_hidden_states are not built (tap() reads three intermediate tensors)")
        if input_values.dim() != 2:
            raise ValueError(f"input_values must be [B, n_samples]; got {tuple(input_values.shape)}")
        B, n = int(input_values.shape[0]), int(input_values.shape[1])
        T = self.num_frames(n)
        if B < 1 or T < 1:
            raise ValueError(f"input_values [{B}, {n}]: a clip needs at least {self.min_samples()} samples for one frame")
        dev = input_values.device
        ctx = self._context(dev, B, n)
        x = input_values.to(dtype=torch.float32).contiguous()
        out = torch.empty(B, T, self.cfg["hidden"], device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mtv_hubert_forward(ctx, x.data_ptr(), n, B, out.data_ptr(),
                                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mtv_hubert_forward")
        out = out.type(input_values.dtype) if input_values.is_floating_point() else out
        return BaseModelOutput(last_hidden_state=out, extract_features=None) if return_dict is not False else (out,)

    def min_samples(self) -> int:
        n = 1
        for k, s in zip(reversed(self.cfg["conv_kernel"]), reversed(self.cfg["conv_stride"])):
            n = (n - 1) * s + k
        return n

    def tap(self, name: str) -> torch.Tensor:
        """A tensor of the LAST forward, [B T, channels] on the CPU: "extract_features", or with debug_taps set before that
        forward "after_pos_conv" / "layer_0"."""
        if self._ctx is None:
            raise _lib.MtvError("no forward has run yet")
        lib = _lib.load()
        rows, ch = C.c_int(0), C.c_int(0)
        _lib.check(lib.mtv_hubert_debug_tap(self._ctx, name.encode(), None, 0, C.byref(rows), C.byref(ch)), "mtv_hubert_debug_tap")
        out = torch.empty(rows.value, ch.value, dtype=torch.float32)
        _lib.check(lib.mtv_hubert_debug_tap(self._ctx, name.encode(), C.c_void_p(out.data_ptr()), out.numel(), None, None), "mtv_hubert_debug_tap")
        return out
