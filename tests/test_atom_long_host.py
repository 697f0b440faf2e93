"""Host-side checks of AToM's long-form path: the windowing and merge helpers of moditalker_amd/pipeline.py, the per-step
guidance weights of GaussianDiffusion.long_ddim_sample against the ones the REFERENCE's loop used
(tests/golden/atom_long.npz, written by tests/golden/make_golden_atom_long.py), the argument checks and the C ABI's exports.
No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

NARROW = dict(nfeats=204, seq_len=20, latent_dim=64, ff_size=128, num_layers=2, num_heads=2, cond_feature_dim=32)
DIFFUSION = dict(schedule="cosine", n_timestep=1000, predict_epsilon=False, loss_type="l2", use_p2=False, cond_drop_prob=0.25, guidance_weight=2)


def _diffusion(**over):
    from moditalker_amd import GaussianDiffusion, MotionDecoder
    cfg = dict(NARROW, **over)
    return GaussianDiffusion(MotionDecoder(**cfg).eval(), cfg["seq_len"], 204, **DIFFUSION)


# H = 20: F below, at, just above and well above one horizon (rows = 2 F, one case with an odd row count)
@pytest.mark.parametrize("rows,want_B", [(14, 1), (40, 1), (42, 2), (43, 2), (60, 2), (62, 3), (100, 4), (250, 12)])
def test_hubert_windows_count_padding_and_slices(rows, want_B):
    from moditalker_amd import pipeline
    H = 20
    hub = np.arange(rows * 3, dtype=np.float32).reshape(rows, 3)
    win = pipeline.hubert_windows(hub, H)
    F = rows // 2
    assert want_B == 1 + int(np.ceil(max(0, F - H) / (H / 2)))
    assert win.shape == (want_B, 2 * H, 3)
    assert (want_B + 1) * (H // 2) >= F                      # the merged windows cover every frame
    need = (want_B + 1) * H
    padded = np.concatenate([hub, np.repeat(hub[-1:], max(0, need - rows), axis=0)], axis=0)
    for b in range(want_B):
        np.testing.assert_array_equal(win[b], padded[b * H: b * H + 2 * H])


def test_hubert_windows_refuses_an_odd_horizon_and_a_wrong_rank():
    from moditalker_amd import pipeline
    with pytest.raises(ValueError):
        pipeline.hubert_windows(np.zeros((80, 4), np.float32), 21)
    with pytest.raises(ValueError):
        pipeline.hubert_windows(np.zeros((80,), np.float32), 20)


def test_merge_windows_length_identity_and_outer_halves():
    from moditalker_amd import pipeline
    B, H, half = 4, 20, 10
    rng = np.random.default_rng(5)
    seq = rng.standard_normal(((B + 1) * half, 204)).astype(np.float32)
    agree = np.stack([seq[b * half: b * half + H] for b in range(B)])      # windows that already agree in their overlaps
    out = pipeline.merge_windows(agree)
    assert out.shape == ((B + 1) * half, 204) and out.dtype == np.float32
    np.testing.assert_allclose(out, seq, rtol=0, atol=1e-6)                # (the two fades sum to 1 up to an fp32 rounding)
    x = rng.standard_normal((B, H, 204)).astype(np.float32)               # windows that disagree
    out = pipeline.merge_windows(x)
    np.testing.assert_array_equal(out[:half], x[0, :half])
    np.testing.assert_array_equal(out[B * half:], x[B - 1, half:])
    # an overlap starts on the outgoing window and ends on the incoming one
    np.testing.assert_array_equal(out[half], x[0, half])
    np.testing.assert_array_equal(out[2 * half - 1], x[1, half - 1])
    fo, fi = np.linspace(1, 0, half, dtype=np.float32)[:, None], np.linspace(0, 1, half, dtype=np.float32)[:, None]
    np.testing.assert_array_equal(out[2 * half: 3 * half], x[1, half:] * fo + x[2, :half] * fi)
    with pytest.raises(ValueError):
        pipeline.merge_windows(np.zeros((2, 21, 204), np.float32))


def test_guidance_weight_table_is_the_references_bit_for_bit():
    gold = np.load(os.path.join(GOLDEN, "atom_long.npz"))
    w = _diffusion().long_guidance_weights()
    assert w.dtype == np.float32 and w.shape == (50,)
    np.testing.assert_array_equal(w, gold["weights"].astype(np.float32))
    assert w[0] == 0.0 and w[-1] == 2.0 and np.all(np.diff(w) >= 0)


def _args(B, L):
    return torch.zeros(B, L, 204), torch.zeros(B, L, 3), torch.zeros(B, 2 * L, 32)


def test_bad_arguments_raise_before_any_launch():
    L = NARROW["seq_len"]
    dif = _diffusion()
    face, pos, cond = _args(3, L)
    with pytest.raises(ValueError):                          # wrong noise shape (the windows of another batch size)
        dif.long_ddim_sample((3, L, 204), face, pos, cond, noise=torch.zeros(50, 2, L, 204))
    with pytest.raises(ValueError):                          # too few draws
        dif.long_ddim_sample((3, L, 204), face, pos, cond, noise=torch.zeros(10, 3, L, 204))
    with pytest.raises(ValueError):
        dif.long_ddim_sample((3, L, 204), face, pos, cond, noise=torch.zeros(50, 3, L, 204), n_steps=0)
    odd = _diffusion(seq_len=21)                             # diffusion.py:276
    face, pos, cond = _args(2, 21)
    with pytest.raises(ValueError):
        odd.long_ddim_sample((2, 21, 204), face, pos, cond, noise=torch.zeros(50, 2, 21, 204))
    dif.clip_denoised = False
    face, pos, cond = _args(3, L)
    with pytest.raises(NotImplementedError):
        dif.long_ddim_sample((3, L, 204), face, pos, cond, noise=torch.zeros(50, 3, L, 204))
    with pytest.raises(NotImplementedError):                 # one window is ddim_sample, which refuses it too
        dif.long_ddim_sample((1, L, 204), face[:1], pos[:1], cond[:1], noise=torch.zeros(50, 1, L, 204))


def test_no_cpu_fallback():
    from moditalker_amd import MtvError
    L = NARROW["seq_len"]
    dif = _diffusion()
    face, pos, cond = _args(3, L)
    with pytest.raises(MtvError):
        dif.long_ddim_sample((3, L, 204), face, pos, cond, noise=torch.zeros(50, 3, L, 204))


def test_library_exports_the_long_sampler():
    from moditalker_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mtv_atom_long_ddim_sample", "mtv_atom_long_num_launches"):
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in _lib.SYMBOLS), name


def test_audio_to_motion_long_windows_merges_and_trims(tmp_path, monkeypatch):
    from moditalker_amd import pipeline
    L = 20
    dif = _diffusion()
    seen = {}

    def fake_long(shape, face, x_pos, cond, noise=None, **kw):
        seen.update(shape=tuple(shape), face=face.clone(), cond=cond.clone())
        return torch.full(tuple(shape), 0.5)

    monkeypatch.setattr(dif, "long_ddim_sample", fake_long)
    kpts = np.arange(204, dtype=np.float32).reshape(68, 3) / 204
    mean = np.linspace(-1, 1, 204, dtype=np.float32)
    hub = np.random.default_rng(2).standard_normal((101, 32)).astype(np.float32)      # F = 50 frames = 2.5 horizons -> 4 windows
    out = pipeline.audio_to_motion_long(hub, kpts, dif, mean, save_dir=str(tmp_path))
    assert seen["shape"] == (4, L, 204)
    np.testing.assert_array_equal(seen["cond"].numpy(), pipeline.hubert_windows(hub, L))
    assert torch.equal(seen["face"], torch.from_numpy(kpts).reshape(1, 1, 204).repeat(4, L, 1))
    assert out.shape == (50, 68, 3) and out.dtype == np.float32
    np.testing.assert_array_equal(np.load(tmp_path / "atom_long.npy"), out)
    np.testing.assert_allclose(out[33].reshape(-1), (0.5 + kpts.reshape(-1)) / 10 + mean, rtol=0, atol=1e-6)
