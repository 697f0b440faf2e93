"""The callers and data formats either side of the denoising loop: the reference's
per-identity sampling loop as a library, driving the HIP sampler (moditalker_amd.DDPM) and the HIP autoencoder
(moditalker_amd.ViTAutoencoder).

Restates, step for step,
  MToV/sample.py:305-400                      the 16-frame chunk loop: conditioning assembly -> DDPM.sample -> decode -> frames
  MToV/sample.py:344-362,388-398              --use_last_as_reference chaining (last decoded frame, through an 8-bit image,
                                              becomes the next chunk's image_cond)
  MToV/sample.py:79-104                       frames/NNNN.png output (save_image_at_folder)
  MToV/tools/dataloader_sample.py:130-139     masked_x: rows from landmark 33's y downwards zeroed
  MToV/tools/dataloader_sample.py:153-179     x_l: 68 landmarks drawn as filled radius-3 discs on black 256x256
  data/data_utils/motion_align/align_face_recon.py:347   aligned_npy/<id>/NNNNN.npy: one [68, 2] landmark array per frame

This is host logic (numpy / PIL for the image formats, torch for device tensors); every model call goes to the HIP library.
`sample.py` itself is not importable (module-level argparse, hard-wired paths, cv2 / torchvision / omegaconf) and the disc
rasteriser it uses, cv2.circle, is not installed here: `_disc_rows` produces the row spans of OpenCV's filled-circle scan
conversion (modules/imgproc/src/drawing.cpp, Circle(), OpenCV 4.x).  It is checked bit for bit against golden bitmaps and
against the test suite's statement-for-statement restatement of Circle() incl. its clipping path
(tests/test_pipeline_host.py); cv2 itself never ran here, see DESIGN.md section 4.
"""
from __future__ import annotations

import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------------------------
# conditioning assembly (dataloader_sample.py)
# ------------------------------------------------------------------------------------------------------------------
def _disc_rows(radius: int) -> List[Tuple[int, int]]:
    """(dy, half_width) rows of cv2.circle(..., radius, thickness=-1): OpenCV's midpoint scan conversion.
    radius 3 -> half widths 3,2,2,0 at |dy| = 0,1,2,3."""
    rows = {}
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        rows[dy] = max(rows.get(dy, -1), dx)       # rows cy +- dy span cx +- dx
        rows[dx] = max(rows.get(dx, -1), dy)       # rows cy +- dx span cx +- dy
        dy += 1
        err += plus
        plus += 2
        mask = -1 if err > 0 else 0                # (err <= 0) - 1
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    out = []
    for d, hw in rows.items():
        out.append((d, hw))
        if d:
            out.append((-d, hw))
    return out


def _draw_disc(img: np.ndarray, cx: int, cy: int, rows: Sequence[Tuple[int, int]], value: int = 255) -> None:
    """One filled disc, clipped to the image ([H, W] or [H, W, C], in place): row cy + dy spans cx - hw .. cx + hw."""
    h, w = img.shape[:2]
    for dy, hw in rows:
        yy = cy + dy
        if 0 <= yy < h:
            x0, x1 = max(cx - hw, 0), min(cx + hw, w - 1)
            if x0 <= x1:
                img[yy, x0:x1 + 1] = value


def landmarks_to_images(lm: np.ndarray, WH: int = 256, flip: bool = False) -> np.ndarray:
    """dataloader_sample.py:153-179 `_change_np_img_size`: lm [T, 68, 2] (image-sized ints) or [T, 68, 3] (normalised
    3-D) -> uint8 [T, 256, 256, 3], white filled radius-3 discs on black; optional vertical flip."""
    lm = np.asarray(lm)
    T = lm.shape[0]
    if lm.shape[-1] == 3:
        lm2d = (lm * WH / 2 + WH / 2).astype(int)[:, :, :2]
    else:
        lm2d = lm.astype(int)
    img = np.zeros([T, 256, 256, 3], dtype=np.uint8)
    rows = _disc_rows(3)
    for b in range(T):
        for x, y in lm2d[b]:
            _draw_disc(img[b], int(x / WH * 256.0), int(y / WH * 256.0), rows)
    if flip:
        img = img[:, ::-1].copy()
    return img


def crop_lower_half(img: np.ndarray, landmarks: np.ndarray) -> np.ndarray:
    """dataloader_sample.py:130-139: zero every row from landmark 33's y downwards. img [C, H, W] (0..255)."""
    mask = np.ones(img.shape[-2:])
    mask[int(landmarks[33][1]):, :] = 0.0
    return (img * mask[None]).astype(np.uint8)


def load_aligned_landmarks(folder: str, start: int, count: int) -> np.ndarray:
    """aligned_npy/<id>/NNNNN.npy (align_face_recon.py:347): frames start .. start+count-1 -> [count, 68, 2]."""
    return np.stack([np.load(os.path.join(folder, f"{str(i).zfill(5)}.npy")) for i in range(start, start + count)], axis=0)


def to_model_range(x: torch.Tensor) -> torch.Tensor:
    """sample.py:321-325: [B, T, C, H, W] in 0..255 -> [B, C, T, H, W] in [-1, 1]."""
    return (x / 127.5 - 1).permute(0, 2, 1, 3, 4).contiguous()


# ------------------------------------------------------------------------------------------------------------------
# on-disk formats (sample.py)
# ------------------------------------------------------------------------------------------------------------------
def frames_to_uint8(fake: torch.Tensor) -> np.ndarray:
    """sample.py:402 / :97-99: frames in 0..255 float -> uint8 the way the reference stores them (`fake.type(torch.uint8)`:
    truncation, then the no-op rint/clip of save_image_at_folder)."""
    return fake.to(torch.uint8).cpu().numpy()


def save_frames(start_iter: int, frames_u8: np.ndarray, folder: str) -> List[str]:
    """sample.py:79-104 save_image_at_folder for one identity column: frames_u8 [T, H, W, 3] -> <folder>/NNNN.png."""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    names = []
    for i in range(frames_u8.shape[0]):
        name = os.path.join(folder, f"{start_iter + i}".zfill(4) + ".png")
        Image.fromarray(frames_u8[i], "RGB").save(name)
        names.append(name)
    return names


def save_gif(frames_u8: np.ndarray, fname: str, duration_ms: int = 100) -> str:
    """sample.py:55-76 save_image_grid's output format: frames_u8 [T, H, W, 3] -> an animated GIF (PIL: `save_all`, 100 ms per
    frame, loop forever, the reference's arguments)."""
    from PIL import Image
    imgs = [Image.fromarray(f, "RGB") for f in frames_u8]
    imgs[0].save(fname, quality=95, save_all=True, append_images=imgs[1:], duration=duration_ms, loop=0)
    return fname


def make_video(result_frames, audio_path: Optional[str], save_path: str, fps: int = 25) -> str:
    """sample.py:107-116: frames -> <save_path minus .mp4>no_audio.mp4 (imageio / ffmpeg writer at `fps`), then ffmpeg muxes the
    driving audio in (`-map 0:v -map 1:a -c:v copy -shortest`) and the silent file is removed.  Host-only and after the path;
    imageio and the ffmpeg binary are the reference's own dependencies and are not part of this image: without them this raises
    a RuntimeError that says so (no silent fallback), `audio_path=None` skips the mux."""
    import shutil
    import subprocess
    try:
        import imageio
    except ImportError as e:
        raise RuntimeError("make_video needs imageio (+ imageio-ffmpeg), as MToV/sample.py does; PNG frames and GIFs need only PIL") from e
    if audio_path and not save_path.endswith(".mp4"):
        # (the reference forms the silent name with .replace('.mp4', ...): without that suffix ffmpeg would read and write the SAME
        # file and the final os.remove would delete the result)
        raise ValueError("make_video: save_path must end in .mp4 when an audio track is muxed in (sample.py:107-116)")
    silent = os.path.splitext(save_path)[0] + "no_audio.mp4" if audio_path else save_path
    imageio.mimwrite(silent, list(result_frames), fps=fps, output_params=["-vf", f"fps={fps}"])
    if audio_path:
        if shutil.which("ffmpeg") is None:
            raise RuntimeError("make_video: the ffmpeg binary is needed to mux the audio track (sample.py:110-113)")
        subprocess.run(["ffmpeg", "-y", "-i", silent, "-i", audio_path, "-map", "0:v", "-map", "1:a", "-c:v", "copy", "-shortest", save_path], check=True)
        os.remove(silent)
    return save_path


def last_frame_to_uint8(fake: torch.Tensor) -> np.ndarray:
    """sample.py:391-398: the last frame of every clip as stored in references/<n>/<idx>.png: rint, clip, uint8
    (the BGR<->RGB swaps of cvtColor + imwrite cancel).  fake [B, T, H, W, 3] in 0..255 -> [B, H, W, 3] uint8."""
    return np.rint(np.asarray(fake[:, -1].cpu(), dtype=np.float32)).clip(0, 255).astype(np.uint8)


def reference_from_uint8(last_u8: np.ndarray, frames: int = 16) -> torch.Tensor:
    """sample.py:349-360: an 8-bit RGB frame per clip -> ToTensor (/255) -> *2-1 -> repeated over `frames` frames:
    [B, 3, frames, H, W] in [-1, 1], the input of extract() for the chained image_cond."""
    t = torch.from_numpy(last_u8).float().div(255.0).permute(0, 3, 1, 2) * 2.0 - 1.0      # [B, 3, H, W]
    return t.unsqueeze(2).expand(-1, -1, frames, -1, -1).contiguous()


# ------------------------------------------------------------------------------------------------------------------
# the stage in front: audio -> motion (AToM/inference.py:101-164)
# ------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def audio_to_motion(hubert, first_frame_kpts, diffusion, key_mean_shape, save_dir: Optional[str] = None, chunk: int = 0,
                    noise=None) -> np.ndarray:
    """One horizon of AToM sampling as AToM/inference.py:113-164 runs it, on moditalker_amd.GaussianDiffusion.
      hubert            [T, cond_feature_dim] HuBERT features of the driving audio (two per video frame); rows
                        [chunk * horizon, chunk * horizon + 2 * horizon) condition this chunk
      first_frame_kpts  the identity's first-frame landmarks, 204 values in any shape ([68, 3], [1, 1, 204], ...)
      key_mean_shape    the 3DMM mean landmark shape (Face3DHelper.key_mean_shape), 204 values
    `face` is the first-frame landmarks repeated over the horizon (AToM.py:158-164, 214-220); the sampler's output is a
    residual on them, the sum is /10 + the mean shape.  Returns [horizon, 68, 3] float32 and, with save_dir, writes
    <save_dir>/atom_<chunk>.npy."""
    horizon = int(diffusion.horizon)
    dev = diffusion.betas.device
    kp = torch.as_tensor(np.asarray(first_frame_kpts), dtype=torch.float32).reshape(1, 1, -1)
    if kp.shape[-1] != 204:
        raise ValueError(f"first_frame_kpts must hold 68 x 3 values; got {kp.shape[-1]}")
    face = kp.repeat(1, horizon, 1)
    cond = torch.as_tensor(np.asarray(hubert), dtype=torch.float32)
    if cond.dim() != 2:
        raise ValueError(f"hubert must be [T, feature_dim]; got {tuple(cond.shape)}")
    cond = cond[chunk * horizon: chunk * horizon + 2 * horizon].unsqueeze(0)
    if cond.shape[1] != 2 * horizon:
        raise ValueError(f"chunk {chunk} needs {2 * horizon} HuBERT rows from {chunk * horizon}; the file has {int(np.asarray(hubert).shape[0])}")
    pos = torch.zeros(1, horizon, 3)
    out = diffusion.render_sample(None, [1, horizon, 204], face.to(dev), None, pos, None, cond.to(dev), 0, "", noise=noise)[0]
    out = (out.reshape(horizon, 204).float() + face[0]) / 10 + torch.as_tensor(np.asarray(key_mean_shape), dtype=torch.float32).reshape(1, 204)
    out = out.reshape(horizon, 68, 3).numpy().astype(np.float32)
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        np.save(os.path.join(save_dir, f"atom_{chunk}.npy"), out)
    return out


def hubert_windows(hubert, horizon: int) -> np.ndarray:
    """HuBERT features [rows, feat] (two rows per video frame) of audio of any length -> [B, 2 horizon, feat], the
    conditions of B half-overlapping windows of `horizon` frames: window b = rows [b horizon, b horizon + 2 horizon), the
    slicing of AToM/inference.py:130 at a stride of half a horizon of frames.  F = rows // 2 frames need
    B = 1 + ceil(max(0, F - horizon) / (horizon / 2)) windows; the (B + 1) horizon rows they read are made by repeating the
    last row."""
    h = np.asarray(hubert)
    horizon = int(horizon)
    if h.ndim != 2 or h.shape[0] < 2:
        raise ValueError(f"hubert must be [rows >= 2, feature_dim]; got {h.shape}")
    if horizon < 2 or horizon % 2:
        raise ValueError(f"the horizon must be even (windows overlap by half); got {horizon}")
    F = h.shape[0] // 2
    B = 1 + -(-max(0, F - horizon) // (horizon // 2))
    need = (B + 1) * horizon
    if h.shape[0] < need:
        h = np.concatenate([h, np.repeat(h[-1:], need - h.shape[0], axis=0)], axis=0)
    return np.stack([h[b * horizon: b * horizon + 2 * horizon] for b in range(B)], axis=0)


def merge_windows(samples) -> np.ndarray:
    """[B, H, 204] half-overlapping windows -> one sequence [(B + 1) H / 2, 204]: the first half of window 0 and the last
    half of window B - 1 as they are, every overlap a linear cross-fade, np.linspace(1, 0, H / 2) on the outgoing window and
    np.linspace(0, 1, H / 2) on the incoming one.  The reference has no merge (its driver never reaches the long sampler); this
    is EDGE's rule for positional channels, and landmarks are positions.  The sampler has already forced the overlaps to
    agree at every step but the last, so the fade only blends what the final step changed."""
    x = np.asarray(samples, dtype=np.float32)
    if x.ndim != 3 or x.shape[1] % 2:
        raise ValueError(f"samples must be [B, even H, C]; got {x.shape}")
    B, H, _ = x.shape
    half = H // 2
    out = np.empty(((B + 1) * half, x.shape[2]), dtype=np.float32)
    out[:half] = x[0, :half]
    out[B * half:] = x[B - 1, half:]
    fade_out = np.linspace(1, 0, half, dtype=np.float32)[:, None]
    fade_in = np.linspace(0, 1, half, dtype=np.float32)[:, None]
    for b in range(1, B):
        out[b * half: (b + 1) * half] = x[b - 1, half:] * fade_out + x[b, :half] * fade_in
    return out


@torch.no_grad()
def audio_to_motion_long(hubert, first_frame_kpts, diffusion, key_mean_shape, save_dir: Optional[str] = None, noise=None) -> np.ndarray:
    """AToM for audio of any length: hubert_windows -> GaussianDiffusion.long_ddim_sample (AToM/model/diffusion.py:252-301)
    -> merge_windows -> the arithmetic of audio_to_motion ((sample + face) / 10 + mean shape), trimmed to the
    F = rows // 2 frames the audio has.  Arguments as audio_to_motion; `noise` is [1 + 49, B, horizon, 204] for the
    B windows hubert_windows makes.  Returns [F, 68, 3] float32 and, with save_dir, writes <save_dir>/atom_long.npy."""
    horizon = int(diffusion.horizon)
    dev = diffusion.betas.device
    kp = torch.as_tensor(np.asarray(first_frame_kpts), dtype=torch.float32).reshape(1, 1, -1)
    if kp.shape[-1] != 204:
        raise ValueError(f"first_frame_kpts must hold 68 x 3 values; got {kp.shape[-1]}")
    cond = torch.from_numpy(np.ascontiguousarray(hubert_windows(hubert, horizon), dtype=np.float32))
    B, F = cond.shape[0], int(np.asarray(hubert).shape[0]) // 2
    face = kp.repeat(B, horizon, 1)
    pos = torch.zeros(B, horizon, 3)
    out = diffusion.long_ddim_sample((B, horizon, 204), face.to(dev), pos, cond.to(dev), noise=noise).detach().cpu().float()
    out = torch.from_numpy(merge_windows(out.numpy()))[:F]
    out = (out + kp[0]) / 10 + torch.as_tensor(np.asarray(key_mean_shape), dtype=torch.float32).reshape(1, 204)
    out = out.reshape(F, 68, 3).numpy().astype(np.float32)
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        np.save(os.path.join(save_dir, "atom_long.npy"), out)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the stage in front of the stage in front: waveform -> HuBERT features (data/data_utils/preprocess/process_audio.py:9-55)
# ------------------------------------------------------------------------------------------------------------------
HUBERT_KERNEL, HUBERT_STRIDE = 400, 320                  # receptive field and hop of the conv encoder, in samples
HUBERT_CLIP_LENGTH = HUBERT_STRIDE * 1000                 # process_audio.py:26: 20 s of 16 kHz audio per clip


@torch.no_grad()
def audio_to_hubert(speech, model, save_path: Optional[str] = None) -> np.ndarray:
    """get_hubert_from_speech (process_audio.py:9-55) step for step, on moditalker_amd.HubertModel.
      speech   the utterance at 16 kHz, [N] or [N, channels] (channel 0 is kept).  Resampling to 16 kHz is ffmpeg in the
               reference (process_audio.py:57-64) and stays with the caller.
      model    anything with HubertModel's forward: forward(input_values [B, n]).last_hidden_state is [B, T, hidden].  If it
               has `normalize` (HubertModel: the device reduction) that normalises the utterance, else the same formula in
               numpy -- which is there so that the windowing can be tested on the CPU with a stub, not as a product path.
    The WHOLE utterance is normalised first ((x - mean) / sqrt(var + 1e-7), Wav2Vec2FeatureExtractor); clip i is samples
    [i 320000, i 320000 + 320080), the remainder starts at num_iter 320000 and is skipped below 400 samples; the clips'
    features are concatenated and padded with zero rows or trimmed to expected_T = (N - 80) // 320, ValueError when they
    differ by more than one row (the reference's assert).  Clips of equal length go through the model as one batch of up to
    model.max_batch clips (every kernel works per clip: the rows are those of one-by-one calls).
    Returns [expected_T, hidden] float32 -- what audio_to_motion / audio_to_motion_long take -- and, with save_path, np.save's it."""
    x = np.asarray(speech.detach().cpu() if torch.is_tensor(speech) else speech)
    if x.ndim == 2:
        x = x[:, 0]
    if x.ndim != 1 or x.shape[0] < 1:
        raise ValueError(f"speech must be [N] or [N, channels]; got {x.shape}")
    x = np.ascontiguousarray(x, dtype=np.float32)
    if hasattr(model, "normalize"):
        values = torch.as_tensor(model.normalize(x))
    else:
        values = torch.from_numpy(((x - x.mean()) / np.sqrt(x.var() + 1e-7)).astype(np.float32))
    N = int(values.shape[0])
    num_iter = N // HUBERT_CLIP_LENGTH
    expected_T = (N - (HUBERT_KERNEL - HUBERT_STRIDE)) // HUBERT_STRIDE
    spans = [(i * HUBERT_CLIP_LENGTH, min(N, i * HUBERT_CLIP_LENGTH + HUBERT_CLIP_LENGTH - HUBERT_STRIDE + HUBERT_KERNEL)) for i in range(num_iter)]
    rest = (num_iter * HUBERT_CLIP_LENGTH, N)
    if rest[1] - rest[0] >= HUBERT_KERNEL:             # a remainder shorter than the receptive field is skipped
        spans.append(rest)
    cap = max(1, int(getattr(model, "max_batch", 1)))
    res: List[torch.Tensor] = []
    i = 0
    while i < len(spans):
        j = i + 1
        while j < len(spans) and j - i < cap and spans[j][1] - spans[j][0] == spans[i][1] - spans[i][0]:
            j += 1
        batch = torch.stack([values[a:b] for a, b in spans[i:j]])
        hidden = model.forward(batch).last_hidden_state
        res.extend(torch.as_tensor(hidden[b]).detach().cpu().float() for b in range(j - i))
        i = j
    if not res:
        raise ValueError(f"speech has {N} samples; one feature row needs {HUBERT_KERNEL}")
    ret = torch.cat(res, dim=0)
    if abs(ret.shape[0] - expected_T) > 1:
        raise ValueError(f"the clips gave {ret.shape[0]} rows, {expected_T} expected from {N} samples")
    if ret.shape[0] < expected_T:
        ret = torch.nn.functional.pad(ret, (0, 0, 0, expected_T - ret.shape[0]))
    else:
        ret = ret[:expected_T]
    out = ret.numpy().astype(np.float32)
    if save_path is not None:
        os.makedirs(os.path.dirname(os.path.abspath(save_path)), exist_ok=True)
        np.save(save_path, out)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the chunk loop (sample.py:305-400)
# ------------------------------------------------------------------------------------------------------------------
_DIVISION_ON = {}          # device -> form of x / 127.5 - 1 that to_model_range takes there (MToVSampler._model_range_division)


class MToVSampler:
    """diffusion_model: moditalker_amd.DDPM; first_stage_model / first_stage_model_ldmk: moditalker_amd.ViTAutoencoder
    (the reference loads two checkpoints of the same architecture, sample.py:206-218)."""

    def __init__(self, diffusion_model, first_stage_model, first_stage_model_ldmk=None, latent_res: int = 32):
        self.dm = diffusion_model
        self.ae = first_stage_model
        self.ae_ldmk = first_stage_model_ldmk if first_stage_model_ldmk is not None else first_stage_model
        self.n_xy = latent_res * latent_res                 # the reference hard-wires 32 * 32 (sample.py:332)

    @torch.no_grad()
    def conditioning(self, x_ref, x, x_l, masked_x):
        """sample.py:321-332,366: inputs [B, T, C, H, W] in 0..255 on the device -> dict of latents."""
        x_ref, x, x_l, masked_x = (to_model_range(t) for t in (x_ref, x, x_l, masked_x))
        z_ = self.ae.extract(x)
        image_cond_ = self.ae.extract(x_ref)
        z_l = self.ae_ldmk.extract(x_l)
        masked_z = self.ae.extract(masked_x)
        return dict(z_=z_, image_cond_=image_cond_, image_cond=image_cond_[:, :, 0:self.n_xy],
                    c=torch.cat([z_l, masked_z], dim=1))

    @torch.no_grad()
    def sample_chunk(self, cond: dict, image_cond: Optional[torch.Tensor] = None, x_noisy_start: bool = False,
                     refvid_noisy_start: bool = False, ratio_: Optional[float] = None, fix_noise: bool = False, noise=None):
        """sample.py:366-387 -> (z [B,4,L], fake [B,T,H,W,3] float in 0..255 on the CPU like the reference)."""
        k = cond["c"].shape[0]
        noised_start = None
        if x_noisy_start:
            noised_start = cond["image_cond_"].float()
        elif refvid_noisy_start:
            noised_start = cond["z_"].float()
        z = self.dm.sample(batch_size=k, cond=cond["c"].float(),
                           image_cond=(image_cond if image_cond is not None else cond["image_cond"]).float(),
                           noised_start=noised_start, ratio_=ratio_, fix_noise=fix_noise, noise=noise)
        fake = self.ae.decode_from_sample(z).clamp(-1, 1).cpu()
        T = fake.shape[0] // k
        fake = (1 + fake.reshape(k, T, *fake.shape[1:]).permute(0, 1, 3, 4, 2)) * 127.5
        return z, fake

    @torch.no_grad()
    def chained_image_cond(self, fake: torch.Tensor, out_dir: Optional[str] = None, ldmk_end: int = 0) -> torch.Tensor:
        """sample.py:344-362,388-398: the next chunk's image_cond from this chunk's last frame (8-bit round trip; written
        to <out_dir>/references/<ldmk_end>/<idx>.png and read back when out_dir is given, exactly as the reference does)."""
        u8 = last_frame_to_uint8(fake)
        if out_dir is not None:
            from PIL import Image
            folder = os.path.join(out_dir, "references", str(ldmk_end))
            os.makedirs(folder, exist_ok=True)
            for idx in range(u8.shape[0]):
                Image.fromarray(u8[idx], "RGB").save(os.path.join(folder, f"{idx}.png"))
            # read back exactly what was just written, in clip order.  (sample.py:347-348 lists and sorts the folder: stale
            # PNGs of an earlier, larger batch would join the batch there, and "10.png" sorts before "2.png".)
            u8 = np.stack([np.asarray(Image.open(os.path.join(folder, f"{idx}.png")).convert("RGB")) for idx in range(u8.shape[0])], axis=0)
        dev = next(self.ae.parameters()).device
        ref = reference_from_uint8(u8, frames=self.ae.s).to(dev)
        return self.ae.extract(ref)[:, :, 0:self.n_xy]

    @torch.no_grad()
    def run_identity(self, chunks: Iterable[Sequence[torch.Tensor]], use_last_as_reference: bool = False,
                     out_dir: Optional[str] = None, noise_per_chunk: Optional[Sequence] = None, overlap: bool = False,
                     num_frames: Optional[int] = None, **sample_kw):
        """The per-identity loop (sample.py:305-432): chunks yield (x_ref, x, x_l, masked_x) in 0..255, [B,T,C,H,W].
        Chunks of one identity are sequential when chained (chunk k+1 needs chunk k's last frame): shard by identity.
        Returns the list of uint8 frame arrays [B, T, H, W, 3]; when out_dir is given writes frames/NNNN.png with the B clips
        of the batch side by side ([H, B*W, 3] per frame), the reference's grid_size=(k, 1) layout (sample.py:79-104).

        `overlap` (sample_crossID.py:185,343-348, the cross-identity script's `--overlap`): chunks start every T/2 frames instead of
        every T -- chunk `it` covers frames [it T/2, it T/2 + T), its frame files overwrite the second half of the chunk before, and
        with `use_last_as_reference` its reference is the last frame of the chunk that ENDED where it starts (the folder
        `references/<ldmk_srt>` there: chunk it - 2; the first two chunks find none and keep their own x_ref, sample_crossID.py:394-396).
        `num_frames` (sample_crossID.py:352-353): stop before the first chunk that starts past it."""
        results = []
        T = self.ae.s
        stride = T // 2 if overlap else T
        chained = {}                                  # frame index a chunk ended at -> image_cond made from its last frame
        for it, (x_ref, x, x_l, masked_x) in enumerate(chunks):
            ldmk_srt = it * stride
            if num_frames is not None and num_frames < ldmk_srt:
                break
            cond = self.conditioning(x_ref, x, x_l, masked_x)
            nz = noise_per_chunk[it] if noise_per_chunk is not None else None
            z, fake = self.sample_chunk(cond, image_cond=chained.get(ldmk_srt) if use_last_as_reference else None, noise=nz, **sample_kw)
            if use_last_as_reference:
                chained[ldmk_srt + T] = self.chained_image_cond(fake, out_dir, ldmk_srt + T)
                chained.pop(ldmk_srt - stride, None)  # (no longer reachable: keeps at most two latents alive)
            u8 = frames_to_uint8(fake)
            results.append(u8)
            if out_dir is not None:
                save_frames(ldmk_srt, np.concatenate(list(u8), axis=2), os.path.join(out_dir, "frames"))
        return results

    # --------------------------------------------------------------------------------------------------------------
    # the same loop with both ends on the device (moditalker_amd.frames, csrc/frames.hip): source frames go up as 8-bit,
    # landmarks as integers, frames come down as 8-bit, the chained reference never leaves the GPU
    # --------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _model_range_division(self, dev) -> str:
        """Which form of x / 127.5 - 1 `to_model_range` takes on `dev`, where `conditioning` evaluates it (sample.py:318-326 moves
        the tensors to the device first, too): "ieee" or "reciprocal" (moditalker_amd.frames.prepare_frames).  Found by evaluating
        it there on the 256 byte values, once per device."""
        key = str(dev)
        if key not in _DIVISION_ON:
            x = torch.arange(256, dtype=torch.float32).reshape(1, 1, 1, 16, 16)
            there = to_model_range(x.to(dev)).cpu()
            forms = {"ieee": to_model_range(x),
                     "reciprocal": (x * (torch.tensor(1.0) / 127.5) - 1).permute(0, 2, 1, 3, 4).contiguous()}
            match = [k for k, v in forms.items() if torch.equal(v, there)]
            if not match:
                from ._lib import MtvError
                raise MtvError(f"x / 127.5 - 1 on {dev} is neither an IEEE division nor a multiplication by the fp32 reciprocal: "
                               "k_frames_prep has no form for it; pass division= explicitly")
            _DIVISION_ON[key] = match[0]
        return _DIVISION_ON[key]

    @torch.no_grad()
    def conditioning_device(self, ref_u8, vid_u8, landmarks, y33, WH: Optional[int] = None, division: Optional[str] = None):
        """`conditioning` from what the reference's loader starts with (dataloader_sample.py:181-247) instead of four float videos:
          ref_u8     uint8 [B, 1, 3, h, w] (the identity's first frame, repeated over T on the device) or [B, T, 3, h, w]
          vid_u8     uint8 [B, T, 3, h, w] source frames of any size (centre crop + bilinear resize happen on the device)
          landmarks  [B, T, 68, 2] image-sized or [B, T, 68, 3] normalised, as `landmarks_to_images` takes them per clip
          y33        [B, T] landmark 33's y in source rows: rows from int(y) downwards are zeroed in masked_x (`crop_lower_half`)
          WH         the landmarks' image size, default the source width (dataloader_sample.py:224-225)
          division   the form of x / 127.5 - 1 (prepare_frames): default the one `to_model_range` takes on the device, which is
                     what `conditioning` computes; "ieee" is the host's
        Tensors may be on the host (they are uploaded as they are, 8-bit) or on the device.  Returns the dict `conditioning` returns.
        The loader's half-length branch (dataloader_sample.py:234-239: a clip of nframes / 2 frames is padded with zero frames in
        front) is not built: clips have T frames."""
        from . import frames as F
        dev = next(self.ae.parameters()).device
        T, res = self.ae.s, self.ae.res
        if self.ae_ldmk.res != F.CANVAS:
            raise ValueError(f"the landmark canvas is {F.CANVAS} x {F.CANVAS} (dataloader_sample.py:163); the landmark autoencoder takes {self.ae_ldmk.res}")
        vid_u8, ref_u8 = torch.as_tensor(vid_u8), torch.as_tensor(ref_u8)
        if vid_u8.dim() != 5 or vid_u8.shape[1] != T:
            raise ValueError(f"vid_u8 must be [B, {T}, 3, h, w]; got {tuple(vid_u8.shape)}")
        B, h, w = vid_u8.shape[0], vid_u8.shape[3], vid_u8.shape[4]
        if ref_u8.dim() != 5 or ref_u8.shape[0] != B or tuple(ref_u8.shape[2:]) != (3, h, w):
            raise ValueError(f"ref_u8 must be [{B}, 1 or {T}, 3, {h}, {w}]; got {tuple(ref_u8.shape)}")
        centres = F.disc_centres(landmarks, w if WH is None else WH)
        start = F.mask_start(y33, h)
        if centres.ndim != 4 or centres.shape[:2] != (B, T) or start.shape != (B, T):
            raise ValueError(f"landmarks must be [{B}, {T}, points, 2 or 3] and y33 [{B}, {T}]; got {centres.shape[:-1]} and {start.shape}")
        vid_u8, ref_u8 = vid_u8.to(dev).contiguous(), ref_u8.to(dev).contiguous()
        division = self._model_range_division(dev) if division is None else division
        x = F.prepare_frames(vid_u8, res, division=division)
        x_ref = F.prepare_frames(ref_u8, res, frames=T, division=division)
        masked_x = F.prepare_frames(vid_u8, res, mask_start=torch.from_numpy(start).to(dev), division=division)
        x_l = F.landmark_frames(torch.from_numpy(np.ascontiguousarray(centres)).to(dev))
        z_ = self.ae.extract(x)
        image_cond_ = self.ae.extract(x_ref)
        z_l = self.ae_ldmk.extract(x_l)
        masked_z = self.ae.extract(masked_x)
        return dict(z_=z_, image_cond_=image_cond_, image_cond=image_cond_[:, :, 0:self.n_xy],
                    c=torch.cat([z_l, masked_z], dim=1))

    @torch.no_grad()
    def sample_chunk_device(self, cond: dict, image_cond: Optional[torch.Tensor] = None, x_noisy_start: bool = False,
                            refvid_noisy_start: bool = False, ratio_: Optional[float] = None, fix_noise: bool = False, noise=None,
                            want_next_ref: bool = False):
        """`sample_chunk` without the host: -> (z [B,4,L], frames_u8 uint8 [B,T,H,W,3], last_u8 uint8 [B,H,W,3], next_ref
        [B,3,T,H,W]), all on the device.  frames_u8 is frames_to_uint8 of sample_chunk's frames; last_u8 / next_ref
        (None unless want_next_ref) are last_frame_to_uint8 and reference_from_uint8 of them."""
        from . import frames as F
        k = cond["c"].shape[0]
        noised_start = None
        if x_noisy_start:
            noised_start = cond["image_cond_"].float()
        elif refvid_noisy_start:
            noised_start = cond["z_"].float()
        z = self.dm.sample(batch_size=k, cond=cond["c"].float(),
                           image_cond=(image_cond if image_cond is not None else cond["image_cond"]).float(),
                           noised_start=noised_start, ratio_=ratio_, fix_noise=fix_noise, noise=noise)
        frames_u8, last_u8, next_ref = F.finish_frames(self.ae.decode_from_sample(z).float().contiguous(), k, want_next_ref=want_next_ref)
        return z, frames_u8, last_u8, next_ref

    @torch.no_grad()
    def run_identity_device(self, chunks, use_last_as_reference: bool = False, out_dir: Optional[str] = None,
                            noise_per_chunk: Optional[Sequence] = None, overlap: bool = False, num_frames: Optional[int] = None,
                            WH: Optional[int] = None, division: Optional[str] = None, **sample_kw):
        """`run_identity` on conditioning_device / sample_chunk_device: chunks yield (ref_u8, vid_u8, landmarks, y33) (see
        conditioning_device).  Same keyword arguments (`WH` and `division` are passed on to conditioning_device), same returned list of uint8 arrays
        [B, T, H, W, 3], same files under out_dir: frames/NNNN.png, and with `use_last_as_reference` references/<n>/<idx>.png from
        last_u8.  The chained image_cond is the extract of next_ref, which never passes through the host (the PNG is written, not
        read back: it holds exactly the bytes next_ref was made from).  The only downloads are the 8-bit frames."""
        results = []
        T = self.ae.s
        stride = T // 2 if overlap else T
        chained = {}
        for it, (ref_u8, vid_u8, landmarks, y33) in enumerate(chunks):
            ldmk_srt = it * stride
            if num_frames is not None and num_frames < ldmk_srt:
                break
            cond = self.conditioning_device(ref_u8, vid_u8, landmarks, y33, WH=WH, division=division)
            nz = noise_per_chunk[it] if noise_per_chunk is not None else None
            z, frames_u8, last_u8, next_ref = self.sample_chunk_device(
                cond, image_cond=chained.get(ldmk_srt) if use_last_as_reference else None, noise=nz,
                want_next_ref=use_last_as_reference, **sample_kw)
            if use_last_as_reference:
                chained[ldmk_srt + T] = self.ae.extract(next_ref)[:, :, 0:self.n_xy]
                chained.pop(ldmk_srt - stride, None)
                if out_dir is not None:
                    from PIL import Image
                    folder = os.path.join(out_dir, "references", str(ldmk_srt + T))
                    os.makedirs(folder, exist_ok=True)
                    for idx, img in enumerate(last_u8.cpu().numpy()):
                        Image.fromarray(img, "RGB").save(os.path.join(folder, f"{idx}.png"))
            u8 = frames_u8.cpu().numpy()
            results.append(u8)
            if out_dir is not None:
                save_frames(ldmk_srt, np.concatenate(list(u8), axis=2), os.path.join(out_dir, "frames"))
        return results
