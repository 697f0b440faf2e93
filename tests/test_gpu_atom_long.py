"""AToM's long-form sampler on the GPU (mtv_atom_long_ddim_sample behind GaussianDiffusion.long_ddim_sample) against what the
REFERENCE's own long_ddim_sample computed (tests/golden/atom_long.npz, tests/golden/make_golden_atom_long.py): the final
sample of 3 half-overlapping windows and the x entering steps 1, 25 and 49.  82 % of the final sample sits on the +-1 clamp,
so the noise-mixed intermediates carry most of the evidence.  Every bar is read from the golden file (1e-3, the sampler bar:
the reference's fp32-vs-fp64 drift is at most 1.4e-5 on each tensor; tests/golden/PIN_REPORT_atom_long.txt).

Equalities asserted bit for bit hold because every kernel of the path computes an output element from its own row and clip
in an order fixed by the weights' shapes (see test_gpu_atom.py), and the stitch copies values: window 0 is never written by
the stitch and attention is per clip, so neither the number of windows nor a repeated call can change one of its bits."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, report

pytestmark = pytest.mark.gpu

NARROW = dict(nfeats=204, seq_len=20, latent_dim=64, ff_size=128, num_layers=2, num_heads=2, cond_feature_dim=32)
TRUE_SHAPE = dict(nfeats=204, seq_len=156, latent_dim=512, ff_size=1024, num_layers=1, num_heads=8, cond_feature_dim=1024)
DIFFUSION = dict(schedule="cosine", n_timestep=1000, predict_epsilon=False, loss_type="l2", use_p2=False, cond_drop_prob=0.25, guidance_weight=2)
SEED = 71
B, L = 3, NARROW["seq_len"]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "atom_long.npz"))


def _model(cfg, max_batch):
    from moditalker_amd import MotionDecoder, filler
    m = MotionDecoder(dropout=0.1, max_batch=max_batch, **cfg).eval()
    freqs = m.rotary.freqs.clone()
    filler.fill_module_(m, seed=SEED)
    m.rotary.freqs.copy_(freqs)
    return m.to(DEV)


@pytest.fixture(scope="module")
def long():
    """The golden's case (make_golden_atom_long.py `inputs`) and every sampler output the tests below share."""
    from moditalker_amd import GaussianDiffusion, filler, pipeline
    m = _model(NARROW, B)
    dif = GaussianDiffusion(m, L, 204, **DIFFUSION).to(DEV)
    face = filler.uniform_pm1("atom.long.face", (1, 1, 204), SEED).repeat(B, L, 1).to(DEV)
    hub = filler.uniform_pm1("atom.long.hubert", ((B + 1) * L, 32), SEED).numpy()
    cond = torch.from_numpy(pipeline.hubert_windows(hub, L)).to(DEV)
    noise = torch.stack(filler.noise_list(50, (B, L, 204), SEED, tag="atom.long.noise")).to(DEV)
    run = lambda n=None: dif.long_ddim_sample((B, L, 204), face, None, cond, noise=noise, n_steps=n)
    out = {None: run()}
    for n in (1, 7, 25, 49):
        out[n] = run(n)
    return dict(m=m, dif=dif, face=face, cond=cond, noise=noise, out=out, run=run)


def _check(name, got, gold, key):
    bar = float(gold[key + "_bar"])
    d = report(name, float((got.cpu().double() - torch.from_numpy(gold[key]).double()).abs().max()), bar)
    print(f"{name}: max-abs {d:.3e}  bar {bar:.3e}")
    assert d <= bar, (name, d, bar)


def test_golden_final_sample(gold, long):
    _check("atom long 50-step sample, 3 windows", long["out"][None], gold, "sample")


@pytest.mark.parametrize("n", [1, 25, 49])
def test_golden_intermediates(gold, long, n):
    _check(f"atom long x entering step {n}", long["out"][n], gold, f"x_step{n}")


def test_stitch_invariant(long):
    x = long["out"][7]
    assert torch.equal(x[1:, :L // 2], x[:-1, L // 2:])
    # ... and the final step is not stitched (diffusion.py:285-287): the windows' x_start differ in their overlaps
    fin = long["out"][None]
    assert not torch.equal(fin[1:, :L // 2], fin[:-1, L // 2:])


@pytest.mark.parametrize("n", [7, None])
def test_window_zero_does_not_depend_on_the_number_of_windows(long, n):
    g = long
    two = g["dif"].long_ddim_sample((2, L, 204), g["face"][:2], None, g["cond"][:2], noise=g["noise"][:, :2].contiguous(), n_steps=n)
    assert torch.equal(two[0], g["out"][n][0])


def test_true_geometry_equals_a_loop_of_guided_forwards():
    """seq_len 156: L / 2 = 78 is no multiple of the 32-row tile, window boundaries fall inside tiles, M = 312 is no tile multiple.
    The same 3 steps driven from Python: one mtv_atom_guided_forward per step with the ramped weight, then the DDIM update and the
    stitch in torch as diffusion.py:289-300 writes them; held to the tolerance of test_hoisted_sample_equals_a_loop_of_guided_forwards."""
    from moditalker_amd import GaussianDiffusion, filler
    nb, Lt, half = 2, TRUE_SHAPE["seq_len"], TRUE_SHAPE["seq_len"] // 2
    m = _model(TRUE_SHAPE, nb)
    dif = GaussianDiffusion(m, Lt, 204, **DIFFUSION).to(DEV)
    face = filler.uniform_pm1("atom.long.true.face", (1, 1, 204), SEED).repeat(nb, Lt, 1).to(DEV)
    cond = filler.uniform_pm1("atom.long.true.cond", (nb, 2 * Lt, 1024), SEED).to(DEV)
    noise = torch.stack(filler.noise_list(50, (nb, Lt, 204), SEED, tag="atom.long.true.noise")).to(DEV)
    got = dif.long_ddim_sample((nb, Lt, 204), face, None, cond, noise=noise, n_steps=3)
    steps, _ = dif.step_table()
    w = dif.long_guidance_weights()
    x = noise[0].clone()
    for i in range(3):
        s = steps[i]
        t = torch.full((nb,), s.t, dtype=torch.long, device=DEV)
        x0 = m.guided_forward(None, x, face, cond, t, float(w[i])).clamp(-1.0, 1.0)
        pn = (s.sqrt_recip_ac * x - x0) / s.sqrt_recipm1_ac
        x = x0 * s.sqrt_ac_next + s.c * pn + s.sigma * noise[1 + s.noise_index]
        x[1:, :half] = x[:-1, half:].clone()
    bar = float(np.load(os.path.join(GOLDEN, "atom.npz"))["narrow_sample_bar"])
    d = report("atom long sampler, true geometry, vs loop of guided forwards", float((x - got).abs().max()), bar)
    print(f"true geometry, fused vs looped: max-abs {d:.3e}  bar {bar:.3e}")
    assert torch.equal(got[1, :half], got[0, half:])
    assert d <= bar


def test_sample_is_bit_reproducible(long):
    assert torch.equal(long["run"](), long["out"][None])
    assert torch.equal(long["run"](7), long["out"][7])


def test_constant_weight_sampler_is_not_disturbed(long):
    g = long
    args = ((2, L, 204), g["face"][:2], None, g["cond"][:2])
    nz = g["noise"][:, :2].contiguous()
    before = g["dif"].ddim_sample(*args, noise=nz)
    g["run"](7)
    after = g["dif"].ddim_sample(*args, noise=nz)
    assert torch.equal(before, after)


def test_one_window_is_ddim_sample(long):
    g = long
    args = ((1, L, 204), g["face"][:1], None, g["cond"][:1])
    nz = g["noise"][:, :1].contiguous()
    assert torch.equal(g["dif"].long_ddim_sample(*args, noise=nz), g["dif"].ddim_sample(*args, noise=nz))


def test_launches_per_step_equal_the_constant_weight_samplers(long):
    """The stitch and the per-step weight ride in launches the step already has."""
    from moditalker_amd import _lib
    lib, ctx = _lib.load(), long["m"]._context(torch.device(DEV), B)
    a, b = C.c_int(), C.c_int()
    _lib.check(lib.mtv_atom_num_launches(ctx, B, C.byref(a)), "mtv_atom_num_launches")
    _lib.check(lib.mtv_atom_long_num_launches(ctx, B, C.byref(b)), "mtv_atom_long_num_launches")
    print(f"launches per step at B = {B}: ddim_sample {a.value}, long_ddim_sample {b.value}")
    assert a.value == b.value > 0


def test_library_refuses_one_window_before_any_launch(long):
    from moditalker_amd import _lib
    g = long
    lib, ctx = _lib.load(), g["m"]._context(torch.device(DEV), B)
    steps, _ = g["dif"].step_table()
    w = np.ascontiguousarray(g["dif"].long_guidance_weights())
    x = g["noise"][0, :1].clone()
    keep = x.clone()
    rc = lib.mtv_atom_long_ddim_sample(ctx, x.data_ptr(), g["face"].data_ptr(), g["cond"].data_ptr(), g["noise"][1:].data_ptr(), 49, steps, 50,
                                       w.ctypes.data_as(C.POINTER(C.c_float)), 1, None)
    torch.cuda.synchronize()
    assert rc < 0 and b"2 windows" in lib.mtv_last_error()
    assert torch.equal(x, keep)


def test_audio_to_motion_long(long, tmp_path):
    from moditalker_amd import filler, pipeline
    hub = filler.uniform_pm1("atom.long.pipeline.hubert", (5 * L, 32), SEED).numpy()      # F = 50 frames = 2.5 horizons: 4 windows
    kpts = filler.uniform_pm1("atom.long.face", (68, 3), SEED).numpy()
    mean = np.linspace(-1, 1, 204, dtype=np.float32)
    out = pipeline.audio_to_motion_long(hub, kpts, long["dif"], mean, save_dir=str(tmp_path))
    assert out.shape == (50, 68, 3) and out.dtype == np.float32 and np.isfinite(out).all()
    np.testing.assert_array_equal(np.load(tmp_path / "atom_long.npy"), out)
