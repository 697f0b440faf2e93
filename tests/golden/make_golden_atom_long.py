#!/usr/bin/env python3
"""Golden vectors for AToM's long-form sampler from the REFERENCE itself: GaussianDiffusion.long_ddim_sample
(AToM/model/diffusion.py:252-301), imported unmodified the way make_golden_atom.py imports it (that module's `build`,
`explicit_noise`, model configuration and seed are reused by import).  Build container only.

The reference's method was never updated when model_predictions gained `x_pos` and `face`: :283 passes three positionals.
Its loop body is intact, so the one harness-side shim binds those two arguments,
    orig = dif.model_predictions
    dif.model_predictions = lambda x, c, t, weight=None, clip_x_start=False: orig(None, x, face, c, t, weight, clip_x_start)
and the reference's own long_ddim_sample((B, L, 204), cond) runs as written.  The same wrapper records the guidance
weight of every step and the x entering steps 1, 25 and 49.

Case: the narrow model of make_golden_atom.py, B = 3 windows (a sender, a sender and receiver, a receiver); face is one
filler row repeated; the conditions are one [(B + 1) L, 32] filler array cut by moditalker_amd.pipeline.hubert_windows;
50 filler draws of [3, 20, 204]; guidance_weight 2, cosine schedule.  Run in fp32 and in fp64.

Bars, per tensor, by make_golden_atom.py's sampler rule: 1e-3 where the reference's own fp32-vs-fp64 drift is at most
1e-4, else 10 x the drift.  With filler weights most of the final sample sits on the +-1 clamp, which would hide most
errors; the noise-mixed intermediates do not saturate, which is why they are pinned too.

Output: tests/golden/atom_long.npz (data only) and tests/golden/PIN_REPORT_atom_long.txt."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_golden_atom as base  # noqa: E402
from moditalker_amd import filler  # noqa: E402
from moditalker_amd.pipeline import hubert_windows  # noqa: E402

SEED = base.SEED
CFG = base.CASES["narrow"]["cfg"]
B = 3
TAPS = (1, 25, 49)      # x entering these steps (0-based) = x after that many steps


def inputs():
    L = CFG["seq_len"]
    face = filler.uniform_pm1("atom.long.face", (1, 1, 204), SEED).repeat(B, L, 1)
    hub = filler.uniform_pm1("atom.long.hubert", ((B + 1) * L, CFG["cond_feature_dim"]), SEED).numpy()
    cond = torch.from_numpy(hubert_windows(hub, L))
    assert tuple(cond.shape) == (B, 2 * L, CFG["cond_feature_dim"])
    return face, cond, filler.noise_list(50, (B, L, 204), SEED, tag="atom.long.noise")


def run(MotionDecoder, GaussianDiffusion, double):
    torch.set_default_dtype(torch.float64 if double else torch.float32)
    try:
        L = CFG["seq_len"]
        m = base.build(MotionDecoder, CFG, double)
        face, cond, noise = inputs()
        if double:
            face, cond = face.double(), cond.double()
        dif = GaussianDiffusion(m, L, 204, schedule="cosine", n_timestep=1000, predict_epsilon=False, loss_type="l2", use_p2=False,
                                cond_drop_prob=0.25, guidance_weight=2)
        if double:
            dif = dif.double()
        orig = dif.model_predictions
        seen_w, seen_x = [], {}

        def bound(x, c, t, weight=None, clip_x_start=False):
            if len(seen_w) in TAPS:
                seen_x[len(seen_w)] = x.clone()
            seen_w.append(weight)
            return orig(None, x, face, c, t, weight, clip_x_start)

        dif.model_predictions = bound
        with torch.no_grad(), base.explicit_noise(noise):
            out = {"sample": dif.long_ddim_sample((B, L, 204), cond)}
        assert len(seen_w) == 50 and sorted(seen_x) == list(TAPS)
        for k in TAPS:
            out[f"x_step{k}"] = seen_x[k]
        return out, np.array([float(w) for w in seen_w], dtype=np.float64)
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    MotionDecoder, GaussianDiffusion = base.import_reference()
    torch.manual_seed(0)
    r32, w32 = run(MotionDecoder, GaussianDiffusion, False)
    r64, w64 = run(MotionDecoder, GaussianDiffusion, True)
    assert np.array_equal(w32, w64)
    out = {"weights": w32, "B": np.int32(B)}
    lines = []
    for k, v in r32.items():
        drift = float((v.double() - r64[k]).abs().max())
        bar = 1e-3 if drift <= 1e-4 else 10.0 * drift
        note = "sampler bar 1e-3" if drift <= 1e-4 else "drift > 1e-4: 10 x drift"
        sat = float((v.abs() >= 1.0).double().mean())
        out[k] = v.float().numpy()
        out[k + "_f64"] = r64[k].numpy()
        out[k + "_bar"] = np.float64(bar)
        lines.append(f"long {k:10s} max|fp32-fp64| {drift:.3e}   bar {bar:.3e}   ({note}; saturated share {100 * sat:.1f} %; max|x| {float(v.abs().max()):.3f})")
    lines.append("guidance weights seen by model_predictions: " + " ".join(f"{w:.6g}" for w in w32[:3]) + " ... " + " ".join(f"{w:.6g}" for w in w32[23:27])
                 + f" ... {w32[-1]:.6g}")
    np.savez_compressed(os.path.join(HERE, "atom_long.npz"), **out)
    with open(os.path.join(HERE, "PIN_REPORT_atom_long.txt"), "w") as f:
        f.write("AToM long-sampler goldens (make_golden_atom_long.py): the reference's own long_ddim_sample, 3 windows of the narrow model,\n"
                "fp32 vs fp64, and the bars the tests read from atom_long.npz\n")
        for ln in lines:
            f.write(ln + "\n")
            print(ln)
    print("atom_long.npz written:", os.path.getsize(os.path.join(HERE, "atom_long.npz")), "bytes")


if __name__ == "__main__":
    main()
