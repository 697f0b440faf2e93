"""Both ends of the MToV chunk loop on the device: thin wrappers over the three context-free calls of csrc/frames.hip
(include/mtv_hip.h: mtv_frames_prep / mtv_frames_discs / mtv_frames_finish) and the two host helpers that resolve the
reference's Python semantics once, so that only integers go up.

  MToV/tools/data_utils.py:73-98             resize_crop: centre crop, bilinear resize          -> prepare_frames
  MToV/tools/dataloader_sample.py:130-139    _crop_lower_half: rows from landmark 33's y zeroed -> mask_start + prepare_frames
  MToV/tools/dataloader_sample.py:153-179    _change_np_img_size: 68 filled discs per frame     -> disc_centres + landmark_frames
  MToV/sample.py:385-398,402,349-360         clamp, 8-bit frames, 8-bit last frame, next ref    -> finish_frames

The wrappers check dtype, shape, contiguity and that the tensors share a device (ValueError) before anything reaches the
library.  There is no CPU fallback: tensors that are not on a HIP device raise MtvError.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

CANVAS = 256            # dataloader_sample.py:163: the landmark canvas is hard-wired, whatever WH is
_INT32 = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------------------------
# host helpers
# ------------------------------------------------------------------------------------------------------------------
def mask_start(y33, h: int) -> np.ndarray:
    """First zeroed source row of `crop_lower_half` for landmark-33 y values of any shape: `mask[int(y):] = 0` on h rows.
    int() truncates towards zero; a negative start counts from the end as the slice does (max(h + y, 0)); values >= h mask
    nothing (h).  Returns int32 of y33's shape, every value in [0, h]."""
    y = np.asarray(y33, dtype=np.float64)
    if not np.all(np.isfinite(y)):
        raise ValueError("mask_start: landmark y values must be finite")
    s = np.trunc(y)
    s = np.where(s < 0, np.maximum(h + s, 0), np.minimum(s, h))
    return s.astype(np.int32)


def disc_centres(lm, WH: int) -> np.ndarray:
    """Disc centres of `landmarks_to_images`: lm [..., 68, 3] (normalised 3-D: (lm * WH / 2 + WH / 2).astype(int), first two
    columns) or [..., 68, 2] (image-sized: astype(int)), then int(x / WH * 256.0) in float64 as the reference's Python does.
    Returns int32 [..., 68, 2] (x, y); values beyond int32 (such centres touch no canvas) are clipped to its range."""
    lm = np.asarray(lm)
    if lm.ndim < 2 or lm.shape[-1] not in (2, 3):
        raise ValueError(f"disc_centres: landmarks must be [..., points, 2 or 3]; got {lm.shape}")
    if lm.shape[-1] == 3:
        lm2d = (lm * WH / 2 + WH / 2).astype(int)[..., :2]
    else:
        lm2d = lm.astype(int)
    c = np.trunc(lm2d / WH * 256.0)                       # int() of a float64: towards zero
    return np.clip(c, -_INT32, _INT32).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------
# device wrappers
# ------------------------------------------------------------------------------------------------------------------
def _want(t, name: str, dtype: torch.dtype, ndim: int) -> None:
    if not torch.is_tensor(t):
        raise ValueError(f"{name} must be a torch tensor; got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}; got {t.dtype}")
    if t.dim() != ndim:
        raise ValueError(f"{name} must have {ndim} dimensions; got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _same_device(ref: torch.Tensor, t: torch.Tensor, name: str) -> None:
    if t.device != ref.device:
        raise ValueError(f"{name} is on {t.device}, the input on {ref.device}")


def _hip(t: torch.Tensor, what: str) -> None:
    if t.device.type != "cuda":
        raise _lib.MtvError(f"{what} runs only on a HIP device (tensor is on {t.device}); there is no CPU fallback")


def _stream(dev: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _side(n, name: str) -> int:
    if not isinstance(n, int) or n < 4 or n > 8192 or n % 4:
        raise ValueError(f"{name} must be a multiple of 4 in 4..8192; got {n}")
    return n


DIVISIONS = {"ieee": 0, "reciprocal": 1}        # MTV_FRAMES_DIV_IEEE / MTV_FRAMES_DIV_RECIPROCAL


def prepare_frames(src_u8: torch.Tensor, res: int, frames: Optional[int] = None, mask_start: Optional[torch.Tensor] = None,
                   division: str = "ieee") -> torch.Tensor:
    """8-bit source frames [B, Tin, 3, h, w] -> float32 [B, 3, T, res, res] in model range: centre crop to the short side,
    bilinear resize (align_corners=False, no antialiasing: F.interpolate's arithmetic), v / 127.5 - 1.  Tin is T or 1 (one
    frame repeated over `frames`); mask_start int32 [B, T] on the same device, each in [0, h] (see mask_start()): source rows
    from there on read as 0, before the resize.  `division`: "ieee", an IEEE division: `to_model_range` of a host tensor; or
    "reciprocal", v * fp32(1 / 127.5): `to_model_range` of a tensor on a HIP device, where torch divides by a scalar that way
    (one ulp apart for 111 of the 256 byte values)."""
    _want(src_u8, "src_u8", torch.uint8, 5)
    B, Tin, ch, h, w = src_u8.shape
    T = Tin if frames is None else frames
    if ch != 3 or B < 1 or B > 4096 or h < 1 or w < 1 or h > 8192 or w > 8192:
        raise ValueError(f"src_u8 must be [1..4096, Tin, 3, 1..8192, 1..8192]; got {tuple(src_u8.shape)}")
    if not isinstance(T, int) or T < 1 or T > 4096 or Tin not in (1, T):
        raise ValueError(f"src_u8 holds {Tin} frames, which must be 1 or frames = {T} (1..4096)")
    _side(res, "res")
    if division not in DIVISIONS:
        raise ValueError(f"division must be one of {sorted(DIVISIONS)}; got {division!r}")
    if mask_start is not None:
        _want(mask_start, "mask_start", torch.int32, 2)
        if tuple(mask_start.shape) != (B, T):
            raise ValueError(f"mask_start must be [{B}, {T}]; got {tuple(mask_start.shape)}")
        _same_device(src_u8, mask_start, "mask_start")
    _hip(src_u8, "prepare_frames")
    dev = src_u8.device
    out = torch.empty(B, 3, T, res, res, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mtv_frames_prep(src_u8.data_ptr(), mask_start.data_ptr() if mask_start is not None else None,
                                               out.data_ptr(), B, Tin, T, h, w, res, DIVISIONS[division], _stream(dev)), "mtv_frames_prep")
    return out


_HALF_WIDTHS = {}        # (device, radius) -> int32 [2 radius + 1] on the device


def half_width_table(radius: int) -> np.ndarray:
    """pipeline._disc_rows(radius) as the table the kernel reads: entry dy + radius is the half width of row cy + dy, -1 for
    a row the scan conversion does not touch.  OpenCV's rule itself stays in pipeline._disc_rows."""
    from .pipeline import _disc_rows
    tab = np.full(2 * radius + 1, -1, dtype=np.int32)
    for dy, hw in _disc_rows(radius):
        tab[dy + radius] = max(tab[dy + radius], hw)
    return tab


def landmark_frames(centres: torch.Tensor, radius: int = 3, canvas: int = CANVAS) -> torch.Tensor:
    """Disc centres int32 [B, T, P, 2] (x, y; see disc_centres()) -> float32 [B, 3, T, 256, 256]: +1 inside any filled disc
    of `radius` (cv2.circle's scan conversion), -1 outside, i.e. to_model_range(landmarks_to_images(...)).  Centres off the
    canvas clip.  The canvas is the reference's hard-wired 256."""
    _want(centres, "centres", torch.int32, 4)
    B, T, P, two = centres.shape
    if two != 2 or not (1 <= B <= 4096 and 1 <= T <= 4096 and 1 <= P <= 1024):
        raise ValueError(f"centres must be [1..4096, 1..4096, 1..1024, 2]; got {tuple(centres.shape)}")
    if not isinstance(radius, int) or radius < 0 or radius > 31:
        raise ValueError(f"radius must be 0..31; got {radius}")
    if canvas != CANVAS:
        raise ValueError(f"the landmark canvas is the reference's hard-wired {CANVAS}; got {canvas}")
    _hip(centres, "landmark_frames")
    dev = centres.device
    key = (dev, radius)
    if key not in _HALF_WIDTHS:
        _HALF_WIDTHS[key] = torch.from_numpy(half_width_table(radius)).to(dev)
    out = torch.empty(B, 3, T, canvas, canvas, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mtv_frames_discs(centres.data_ptr(), _HALF_WIDTHS[key].data_ptr(), out.data_ptr(), B, T, P, radius,
                                                canvas, _stream(dev)), "mtv_frames_discs")
    return out


def finish_frames(decoded: torch.Tensor, batch: int, want_next_ref: bool = False,
                  out: Optional[Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]] = None):
    """decode_from_sample's output [B * T, 3, res, res] float32 (unclamped) -> (frames_u8, last_u8, next_ref):
      frames_u8 uint8 [B, T, res, res, 3]   clamp(-1, 1), (1 + v) * 127.5, truncated: frames_to_uint8 of sample_chunk's frames
      last_u8   uint8 [B, res, res, 3]      the last frame of every clip through rint and a clip to 0..255: last_frame_to_uint8
      next_ref  float32 [B, 3, T, res, res] last_u8 / 255 * 2 - 1 repeated over T: reference_from_uint8
    The last two are None unless want_next_ref.  `out`: the three tensors to write into (the last two may be None when not
    wanted; they are never touched then)."""
    _want(decoded, "decoded", torch.float32, 4)
    N, ch, res, res2 = decoded.shape
    if not isinstance(batch, int) or batch < 1 or batch > 4096 or N % batch or N // batch < 1 or N // batch > 4096:
        raise ValueError(f"decoded holds {N} frames, which must be batch = {batch} (1..4096) clips of 1..4096 frames")
    if ch != 3 or res != res2:
        raise ValueError(f"decoded must be [B * T, 3, res, res]; got {tuple(decoded.shape)}")
    _side(res, "res")
    T = N // batch
    shapes = ((batch, T, res, res, 3), (batch, res, res, 3), (batch, 3, T, res, res))
    dtypes = (torch.uint8, torch.uint8, torch.float32)
    names = ("frames_u8", "last_u8", "next_ref")
    if out is not None:
        if len(out) != 3:
            raise ValueError("out must be (frames_u8, last_u8, next_ref)")
        for i, t in enumerate(out):
            if t is None and (i == 0 or want_next_ref):
                raise ValueError(f"out: {names[i]} is needed")
            if t is not None:
                _want(t, names[i], dtypes[i], len(shapes[i]))
                if tuple(t.shape) != shapes[i]:
                    raise ValueError(f"{names[i]} must be {shapes[i]}; got {tuple(t.shape)}")
                _same_device(decoded, t, names[i])
    _hip(decoded, "finish_frames")
    dev = decoded.device
    bufs = list(out) if out is not None else [None, None, None]
    for i in range(3):
        if bufs[i] is None and (i == 0 or want_next_ref):
            bufs[i] = torch.empty(shapes[i], device=dev, dtype=dtypes[i])
    last, ref = (bufs[1], bufs[2]) if want_next_ref else (None, None)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mtv_frames_finish(decoded.data_ptr(), bufs[0].data_ptr(), last.data_ptr() if last is not None else None,
                                                 ref.data_ptr() if ref is not None else None, batch, T, res, _stream(dev)), "mtv_frames_finish")
    return bufs[0], last, ref
