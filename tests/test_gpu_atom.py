"""The audio-to-motion stage on the GPU (csrc/atom.hip behind moditalker_amd.MotionDecoder / GaussianDiffusion) against
what the REFERENCE computed (tests/golden/atom.npz, tests/golden/make_golden_atom.py).

Tolerances are read from the golden file: for a single forward 10 x the max-abs difference between the reference's own
fp32 and fp64 runs of that call; for the 50-step sample the project's sampler bar 1e-3 (the reference's own fp32-vs-fp64
drift over the 50 steps is 1.0e-5, below the 1e-4 at which the bar would widen); tests/golden/PIN_REPORT_atom.txt lists both.

Equalities asserted bit for bit, and why they must hold: every kernel of this path computes an output element from its own
row and clip with a summation order fixed by the shapes of the weights (k_tok_linear: K chunks dealt to four waves, added
in wave order; k_tok_attn: keys in index order), no atomics -- so neither a repeated call nor the batch size can change a bit."""
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


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "atom.npz"))


def _inputs(tag, cfg, B):
    from moditalker_amd import filler
    L = cfg["seq_len"]
    return (filler.uniform_pm1(f"atom.{tag}.x", (B, L, 204), SEED), filler.uniform_pm1(f"atom.{tag}.face", (B, 1, 204), SEED).repeat(1, L, 1),
            filler.uniform_pm1(f"atom.{tag}.cond", (B, 2 * L, cfg["cond_feature_dim"]), SEED))


def _model(cfg, max_batch):
    from moditalker_amd import MotionDecoder, filler
    m = MotionDecoder(dropout=0.1, max_batch=max_batch, **cfg).eval()
    freqs = m.rotary.freqs.clone()
    filler.fill_module_(m, seed=SEED)
    m.rotary.freqs.copy_(freqs)
    return m.to("cuda:0")


@pytest.fixture(scope="module")
def narrow():
    from moditalker_amd import GaussianDiffusion, filler
    m = _model(NARROW, 2)
    dif = GaussianDiffusion(m, NARROW["seq_len"], 204, **DIFFUSION).to("cuda:0")
    x, face, cond = (t.to("cuda:0") for t in _inputs("narrow", NARROW, 2))
    noise = torch.stack(filler.noise_list(50, (2, NARROW["seq_len"], 204), SEED, tag="atom.narrow.noise")).to("cuda:0")
    sample = dif.ddim_sample((2, NARROW["seq_len"], 204), face, None, cond, noise=noise)
    return dict(m=m, dif=dif, x=x, face=face, cond=cond, noise=noise, sample=sample)


def _check(name, got, gold, key):
    d = report(name, float((got.cpu().double() - torch.from_numpy(gold[key]).double()).abs().max()), float(gold[key + "_bar"]))
    print(f"{name}: max-abs {d:.3e}  bar {float(gold[key + '_bar']):.3e}")
    assert d <= float(gold[key + "_bar"]), (name, d, float(gold[key + "_bar"]))


@pytest.mark.parametrize("t", [999, 0])
@pytest.mark.parametrize("drop", [0, 1])
def test_narrow_forward(gold, narrow, t, drop):
    n = narrow
    out = n["m"](None, n["x"], n["face"], n["cond"], torch.full((2,), t, dtype=torch.long, device="cuda:0"), cond_drop_prob=drop)
    _check(f"atom narrow forward t={t} drop={drop}", out, gold, f"narrow_forward_t{t}_drop{drop}")


def test_narrow_guided_forward(gold, narrow):
    n = narrow
    out = n["m"].guided_forward(None, n["x"], n["face"], n["cond"], torch.tensor([999, 400], device="cuda:0"), 2.0)
    _check("atom narrow guided_forward w=2", out, gold, "narrow_guided_t999_w2")


def test_true_shape_guided_forward(gold):
    m = _model(TRUE_SHAPE, 1)
    x, face, cond = (t.to("cuda:0") for t in _inputs("true_shape", TRUE_SHAPE, 1))
    out = m.guided_forward(None, x, face, cond, torch.full((1,), 500, dtype=torch.long, device="cuda:0"), 2.0)
    _check("atom true_shape guided_forward t=500 (keys 156 / 470 / 158, d = 64)", out, gold, "true_shape_guided_t500_w2")


def test_narrow_sample(gold, narrow):
    _check("atom narrow 50-step ddim_sample", narrow["sample"], gold, "narrow_sample")


def test_hoisted_sample_equals_a_loop_of_guided_forwards(gold, narrow):
    """The sampler runs the timestep-invariant part once and the DDIM update in final_layer's epilogue; here the same 50 steps are driven
    from Python, one mtv_atom_guided_forward (which recomputes everything) per step, the update in torch as diffusion.py:235-249 writes it."""
    n, dif = narrow, narrow["dif"]
    steps, _ = dif.step_table()
    x = n["noise"][0].clone()
    for s in steps:
        t = torch.full((2,), s.t, dtype=torch.long, device="cuda:0")
        x0 = n["m"].guided_forward(None, x, n["face"], n["cond"], t, 2.0).clamp(-1.0, 1.0)
        if s.last:
            x = x0
            break
        pn = (s.sqrt_recip_ac * x - x0) / s.sqrt_recipm1_ac
        x = x0 * s.sqrt_ac_next + s.c * pn + s.sigma * n["noise"][1 + s.noise_index]
    bar = float(gold["narrow_sample_bar"])
    d = report("atom hoisted sampler vs loop of guided forwards", float((x - n["sample"]).abs().max()), bar)
    print(f"hoisted vs looped: max-abs {d:.3e}  bar {bar:.3e}")
    assert d <= bar


def test_sample_is_bit_reproducible(narrow):
    n = narrow
    again = n["dif"].ddim_sample((2, NARROW["seq_len"], 204), n["face"], None, n["cond"], noise=n["noise"])
    assert torch.equal(again, n["sample"])


def test_batch_two_equals_two_batch_one_runs(narrow):
    n = narrow
    t = torch.tensor([999, 400], device="cuda:0")
    both = n["m"].guided_forward(None, n["x"], n["face"], n["cond"], t, 2.0)
    for b in range(2):
        one = n["m"].guided_forward(None, n["x"][b:b + 1], n["face"][b:b + 1], n["cond"][b:b + 1], t[b:b + 1], 2.0)
        assert torch.equal(one[0], both[b]), b
    for b in range(2):
        one = n["dif"].ddim_sample((1, NARROW["seq_len"], 204), n["face"][b:b + 1], None, n["cond"][b:b + 1], noise=n["noise"][:, b:b + 1])
        assert torch.equal(one[0], n["sample"][b]), b


def test_wrong_shapes_raise_before_any_launch(narrow):
    n, L = narrow, NARROW["seq_len"]
    t = torch.zeros(2, dtype=torch.long, device="cuda:0")
    with pytest.raises(ValueError):
        n["m"](None, n["x"], n["face"][:, :L - 1], n["cond"], t)
    with pytest.raises(ValueError):
        n["m"].guided_forward(None, n["x"], n["face"], n["cond"][:, :, :16], t, 2.0)
    with pytest.raises(ValueError):
        n["dif"].ddim_sample((2, L, 204), n["face"], None, n["cond"][:, :L], noise=n["noise"])
    with pytest.raises(ValueError):
        n["dif"].ddim_sample((2, L, 204), n["face"], None, n["cond"], noise=n["noise"][:10])
