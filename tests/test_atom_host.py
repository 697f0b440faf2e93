"""Host-side checks of the audio-to-motion stage (moditalker_amd/atom.py): state_dict parity with the reference, the
schedule and the 50-step DDIM table against values the reference produced (tests/golden/atom.npz, written by
tests/golden/make_golden_atom.py), argument checks, the C ABI's exports and the pipeline glue.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

NARROW = dict(nfeats=204, seq_len=20, latent_dim=64, ff_size=128, num_layers=2, num_heads=2, cond_feature_dim=32)
TRUE_SHAPE = dict(nfeats=204, seq_len=156, latent_dim=512, ff_size=1024, num_layers=1, num_heads=8, cond_feature_dim=1024)
DIFFUSION = dict(schedule="cosine", n_timestep=1000, predict_epsilon=False, loss_type="l2", use_p2=False, cond_drop_prob=0.25, guidance_weight=2)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "atom.npz"))


@pytest.mark.parametrize("tag,cfg", [("narrow", NARROW), ("true_shape", TRUE_SHAPE)])
def test_state_dict_matches_reference(gold, tag, cfg):
    from moditalker_amd import MotionDecoder
    sd = MotionDecoder(dropout=0.1, **cfg).state_dict()
    assert list(sd.keys()) == list(gold[f"{tag}_keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(gold[f"{tag}_shapes"])


def test_rotary_freqs_are_the_references():
    from moditalker_amd import MotionDecoder
    m = MotionDecoder(**NARROW)
    d = NARROW["latent_dim"]
    want = 1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))
    assert torch.equal(m.rotary.freqs, want)
    rot, tf = m.tables()
    assert rot.shape == (3 * NARROW["seq_len"] + 2, d // 2, 2) and tf.shape == (d // 2,)
    assert float(rot[0, :, 0].min()) == 1.0 and float(rot[0, :, 1].abs().max()) == 0.0      # position 0: cos 1, sin 0


def test_schedule_buffers_match_reference(gold):
    from moditalker_amd import GaussianDiffusion, MotionDecoder
    dif = GaussianDiffusion(MotionDecoder(**NARROW), NARROW["seq_len"], 204, **DIFFUSION)
    names = [k[len("sched_"):] for k in gold.files if k.startswith("sched_")]
    assert len(names) == 13
    assert [n for n, _ in dif.named_buffers() if "." not in n] == names
    for n in names:
        np.testing.assert_array_equal(getattr(dif, n).numpy(), gold[f"sched_{n}"], err_msg=n)


def test_beta_schedule_is_atoms_not_mtovs():
    from moditalker_amd import atom, ddpm
    for name in ("linear", "cosine", "sqrt_linear", "sqrt"):
        b = atom.make_beta_schedule(name, 1000)
        assert b.dtype == np.float64 and b.shape == (1000,)
    assert atom.make_beta_schedule("cosine", 1000).max() == 0.999
    with pytest.raises(ValueError):
        atom.make_beta_schedule("quadratic", 10)
    # same default ramp end points as MToV's function, but AToM's constructor passes no overrides: linear starts at 1e-4
    assert atom.make_beta_schedule("linear", 1000)[0] == pytest.approx(1e-4) and ddpm.make_beta_schedule("linear", 1000)[0] == pytest.approx(1e-4)


def test_ddim_step_table_matches_reference(gold):
    from moditalker_amd import GaussianDiffusion, MotionDecoder
    dif = GaussianDiffusion(MotionDecoder(**NARROW), NARROW["seq_len"], 204, **DIFFUSION)
    steps, n_draws = dif.step_table()
    assert len(steps) == 50 and n_draws == 49
    np.testing.assert_array_equal(np.array([s.t for s in steps], dtype=np.int32), gold["steps_t"])
    np.testing.assert_array_equal(np.array([s.c for s in steps], dtype=np.float32), gold["steps_c"])
    np.testing.assert_array_equal(np.array([s.sigma for s in steps], dtype=np.float32), gold["steps_sigma"])
    assert [s.last for s in steps] == [0] * 49 + [1]
    assert [s.noise_index for s in steps] == list(range(49)) + [-1]
    assert all(s.sqrt_recipm1_ac > 0 for s in steps)      # pred_noise divides by it
    assert steps[0].sqrt_recipm1_ac == float(dif.sqrt_recipm1_alphas_cumprod[999])


def test_training_paths_raise():
    from moditalker_amd import GaussianDiffusion, MotionDecoder
    m = MotionDecoder(**NARROW)
    B, L = 1, NARROW["seq_len"]
    x, cond, t = torch.zeros(B, L, 204), torch.zeros(B, 2 * L, 32), torch.zeros(B, dtype=torch.long)
    with pytest.raises(NotImplementedError):
        m(None, x, x, cond, t, cond_drop_prob=0.3)
    with pytest.raises(NotImplementedError):
        MotionDecoder(use_rotary=False, **NARROW)
    dif = GaussianDiffusion(m, L, 204, **DIFFUSION)
    for call in (lambda: dif(None, x, x, cond), lambda: dif.p_sample_loop((B, L, 204), cond), lambda: dif.loss(x, None, x, cond)):
        with pytest.raises(NotImplementedError):
            call()


def test_wrong_shapes_raise_before_the_device_is_touched():
    from moditalker_amd import MotionDecoder
    m = MotionDecoder(**NARROW)
    L = NARROW["seq_len"]
    x, cond, t = torch.zeros(2, L, 204), torch.zeros(2, 2 * L, 32), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError):
        m(None, x, torch.zeros(2, L + 1, 204), cond, t)
    with pytest.raises(ValueError):
        m.guided_forward(None, x, x, torch.zeros(2, 2 * L, 33), t, 2.0)
    with pytest.raises(ValueError):
        m(None, x, x, cond, torch.zeros(3, dtype=torch.long))


def test_no_cpu_fallback():
    from moditalker_amd import MotionDecoder, MtvError
    m = MotionDecoder(**NARROW).eval()
    L = NARROW["seq_len"]
    with pytest.raises(MtvError):
        m(None, torch.zeros(1, L, 204), torch.zeros(1, L, 204), torch.zeros(1, 2 * L, 32), torch.zeros(1, dtype=torch.long))


def test_reference_style_checkpoint_loads_strict(gold):
    from moditalker_amd import MotionDecoder
    m = MotionDecoder(**NARROW)
    sd = {k: torch.zeros([int(s) for s in shp.split(",")]) for k, shp in zip(gold["narrow_keys"], gold["narrow_shapes"])}
    m.load_state_dict(sd, strict=True)


def test_library_exports_atom_symbols():
    from moditalker_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mtv_atom_create", "mtv_atom_destroy", "mtv_atom_set_tables", "mtv_atom_forward", "mtv_atom_guided_forward",
                 "mtv_atom_set_guidance", "mtv_atom_ddim_sample"):
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in _lib.SYMBOLS), name


def test_audio_to_motion_writes_the_references_file(tmp_path, monkeypatch):
    from moditalker_amd import GaussianDiffusion, MotionDecoder, pipeline
    L = 156
    dif = GaussianDiffusion(MotionDecoder(**dict(NARROW, seq_len=L)), L, 204, **DIFFUSION)
    seen = {}

    def fake_ddim(shape, face, x_pos, cond, noise=None, **kw):
        seen.update(shape=tuple(shape), face=face.clone(), cond=tuple(cond.shape))
        return torch.full(tuple(shape), 0.5)

    monkeypatch.setattr(dif, "ddim_sample", fake_ddim)
    kpts = np.arange(204, dtype=np.float32).reshape(68, 3) / 204
    mean = np.linspace(-1, 1, 204, dtype=np.float32)
    out = pipeline.audio_to_motion(np.zeros((400, 32), np.float32), kpts, dif, mean, save_dir=str(tmp_path))
    assert seen["shape"] == (1, L, 204) and seen["cond"] == (1, 2 * L, 32)
    assert torch.equal(seen["face"], torch.from_numpy(kpts).reshape(1, 1, 204).repeat(1, L, 1))      # first frame repeated over the horizon
    saved = np.load(tmp_path / "atom_0.npy")
    assert saved.shape == (156, 68, 3) and saved.dtype == np.float32
    np.testing.assert_array_equal(saved, out)
    np.testing.assert_allclose(saved[7].reshape(-1), (0.5 + kpts.reshape(-1)) / 10 + mean, rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        pipeline.audio_to_motion(np.zeros((100, 32), np.float32), kpts, dif, mean)
