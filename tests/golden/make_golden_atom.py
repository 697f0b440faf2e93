#!/usr/bin/env python3
"""Golden vectors for the audio-to-motion stage from the REFERENCE itself: AToM's MotionDecoder and GaussianDiffusion
(AToM/model/{model,utils,rotary_embedding_torch,diffusion}.py), imported unmodified.  Build container only (needs the
reference checkout; never on the GPU box).

Harness-side shims, none of them in the arithmetic: `p_tqdm` and `cv2` (imported by diffusion.py, not used when
sampling) are stubbed when absent; the reference's ddim_sample draws x_T and the in-loop noise from torch's global
generator, so torch.randn / torch.randn_like hand out an explicit, recipe-made list while it runs.

Weights: filler.fill_module_(m, seed) -- rotary.freqs keeps the value the reference computes.  Inputs: filler.uniform_pm1.

Cases
  narrow      latent_dim 64, 2 heads (d = 32), ff 128, 2 layers, seq_len 20 (keys 20 / 62 / 22), cond_feature_dim 32, B = 2:
              forward at cond_drop_prob 0 and 1 for t = 999 and 0, guided_forward with w = 2, a 50-step ddim_sample.
  true_shape  latent_dim 512, 8 heads (d = 64), ff 1024, 1 layer, seq_len 156 (keys 156 / 470 / 158), cond_feature_dim 1024,
              B = 1: one guided_forward at t = 500.
Every stored call is also run in float64 (model.double(), default dtype float64); the tolerance of a single forward is
10 x max|fp32 - fp64| of the reference on that call, the tolerance of the sample is 1e-3 (the project's sampler bar) unless
the reference's own fp32-vs-fp64 drift over the 50 steps exceeds 1e-4, then 10 x that.

Output: tests/golden/atom.npz (outputs, bars, schedule buffers, step table, state-dict key / shape lists -- data only) and
tests/golden/PIN_REPORT_atom.txt."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
from moditalker_amd import filler  # noqa: E402

REF = "/root/reference/AToM"
SEED = 71
CASES = {
    "narrow": dict(cfg=dict(nfeats=204, seq_len=20, latent_dim=64, ff_size=128, num_layers=2, num_heads=2, cond_feature_dim=32), B=2),
    "true_shape": dict(cfg=dict(nfeats=204, seq_len=156, latent_dim=512, ff_size=1024, num_layers=1, num_heads=8, cond_feature_dim=1024), B=1),
}


def import_reference():
    for name in ("p_tqdm", "cv2"):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.p_map = None
            sys.modules[name] = m
    sys.path.insert(0, REF)
    from model.diffusion import GaussianDiffusion
    from model.model import MotionDecoder
    return MotionDecoder, GaussianDiffusion


def inputs(tag, cfg, B):
    L = cfg["seq_len"]
    return (filler.uniform_pm1(f"atom.{tag}.x", (B, L, 204), SEED), filler.uniform_pm1(f"atom.{tag}.face", (B, 1, 204), SEED).repeat(1, L, 1),
            filler.uniform_pm1(f"atom.{tag}.cond", (B, 2 * L, cfg["cond_feature_dim"]), SEED))


def sample_noise(tag, cfg, B):
    return filler.noise_list(50, (B, cfg["seq_len"], 204), SEED, tag=f"atom.{tag}.noise")


class explicit_noise:
    """torch.randn / randn_like hand out the given draws in order while active (the harness owns the RNG)."""

    def __init__(self, draws):
        self.draws = list(draws)

    def __enter__(self):
        self.saved = (torch.randn, torch.randn_like)
        torch.randn = lambda *a, **k: self.draws.pop(0).to(torch.get_default_dtype())
        torch.randn_like = lambda t, **k: self.draws.pop(0).to(t.dtype)

    def __exit__(self, *a):
        torch.randn, torch.randn_like = self.saved
        assert not self.draws, "the loop did not consume every draw"


def build(MotionDecoder, cfg, double):
    import torch.nn.functional as F
    m = MotionDecoder(dropout=0.1, activation=F.gelu, **cfg).eval()
    freqs = m.rotary.freqs.clone()
    filler.fill_module_(m, seed=SEED)
    m.rotary.freqs.copy_(freqs)
    return m.double() if double else m


def run_case(MotionDecoder, GaussianDiffusion, tag, double):
    spec = CASES[tag]
    cfg, B = spec["cfg"], spec["B"]
    torch.set_default_dtype(torch.float64 if double else torch.float32)
    try:
        m = build(MotionDecoder, cfg, double)
        x, face, cond = (t.double() if double else t for t in inputs(tag, cfg, B))
        out = {}
        with torch.no_grad():
            if tag == "narrow":
                for t in (999, 0):
                    for drop in (0, 1):
                        out[f"forward_t{t}_drop{drop}"] = m(None, x, face, cond, torch.full((B,), t, dtype=torch.long), cond_drop_prob=drop)
                out["guided_t999_w2"] = m.guided_forward(None, x, face, cond, torch.tensor([999, 400][:B]), 2.0)
                dif = GaussianDiffusion(m, cfg["seq_len"], 204, schedule="cosine", n_timestep=1000, predict_epsilon=False, loss_type="l2",
                                        use_p2=False, cond_drop_prob=0.25, guidance_weight=2)
                if double:
                    dif = dif.double()
                with explicit_noise(sample_noise(tag, cfg, B)):
                    out["sample"] = dif.ddim_sample((B, cfg["seq_len"], 204), face, None, cond)
                if not double:
                    out["_diffusion"] = dif
            else:
                out["guided_t500_w2"] = m.guided_forward(None, x, face, cond, torch.full((B,), 500, dtype=torch.long), 2.0)
        if not double:
            sd = m.state_dict()
            out["_keys"] = np.array(list(sd.keys()))
            out["_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        return out
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    MotionDecoder, GaussianDiffusion = import_reference()
    torch.manual_seed(0)
    out, lines = {}, []
    for tag in CASES:
        r32 = run_case(MotionDecoder, GaussianDiffusion, tag, False)
        r64 = run_case(MotionDecoder, GaussianDiffusion, tag, True)
        out[f"{tag}_keys"], out[f"{tag}_shapes"] = r32.pop("_keys"), r32.pop("_shapes")
        dif = r32.pop("_diffusion", None)
        for k, v in r32.items():
            drift = float((v.double() - r64[k]).abs().max())
            if k == "sample":
                bar = 1e-3 if drift <= 1e-4 else 10.0 * drift
                note = "sampler bar 1e-3" if drift <= 1e-4 else "drift > 1e-4: 10 x drift"
            else:
                bar, note = 10.0 * drift, "10 x drift"
            out[f"{tag}_{k}"] = v.float().numpy()
            out[f"{tag}_{k}_f64"] = r64[k].numpy()
            out[f"{tag}_{k}_bar"] = np.float64(bar)
            lines.append(f"{tag + ' ' + k:36s} max|fp32-fp64| {drift:.3e}   bar {bar:.3e}   ({note}; max|out| {float(v.abs().max()):.3f})")
        if dif is not None:      # schedule buffers and the 50-step table of the configuration AToM.py:70-81 builds (cosine, 1000 steps)
            for name, buf in dif.named_buffers():
                if "." not in name:
                    out[f"sched_{name}"] = buf.numpy()
            times = list(reversed(torch.linspace(-1, 999, steps=51).int().tolist()))
            tab = []
            for t, tn in zip(times[:-1], times[1:]):
                if tn < 0:
                    tab.append((t, 0.0, 0.0))
                    continue
                a, an = dif.alphas_cumprod[t], dif.alphas_cumprod[tn]
                sigma = 1 * ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
                tab.append((t, float((1 - an - sigma ** 2).sqrt()), float(sigma)))
            out["steps_t"] = np.array([r[0] for r in tab], dtype=np.int32)
            out["steps_c"] = np.array([r[1] for r in tab], dtype=np.float32)
            out["steps_sigma"] = np.array([r[2] for r in tab], dtype=np.float32)
    np.savez_compressed(os.path.join(HERE, "atom.npz"), **out)
    with open(os.path.join(HERE, "PIN_REPORT_atom.txt"), "w") as f:
        f.write("AToM goldens (make_golden_atom.py): the reference's own fp32 vs fp64 runs, and the bars the tests read from atom.npz\n")
        for ln in lines:
            f.write(ln + "\n")
            print(ln)
    print("atom.npz written:", os.path.getsize(os.path.join(HERE, "atom.npz")), "bytes")


if __name__ == "__main__":
    main()
