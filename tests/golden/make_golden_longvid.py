#!/usr/bin/env python3
"""Golden vectors of the 128-wide-head geometries, produced by running the REFERENCE itself (the method of make_golden.py:
the reference imported unmodified with the two documented shims, weights / inputs / noise from moditalker_amd/filler.py,
oracle/ref_unet.py + oracle/ref_ddpm.py cross-checked on every case, results appended to PIN_REPORT_longvid.txt -- a report of its own
next to PIN_REPORT.txt, which make_golden.py rewrites).

  slim128.npz   model_channels=64, 2 heads, channel_mult [1,2,4,4]: head dims 32 / 64 / 128 / 128 at C = 64 .. 256 (52 M
                parameters).  eps at t = 999 / 500 / 0 (B = 1), a B = 2 forward at t = [977, 13] with the 25 taps
                subsampled [..., ::7], the 4-step sample.
  longvid.npz   MToV/configs/latent-diffusion/base_longvid.yaml exactly (model_channels=256, 8 heads, cond_model=True; 805
                keys): key / shape manifest, eps at t = 999 and 0, the 4-step sample.

Runs only where the reference tree is present (never on the GPU box).  Usage: python tests/golden/make_golden_longvid.py [--slim-only]
Outputs are data only (fp32, compressed .npz)."""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402  (import_reference / injected_noise / build: the shared method)
from moditalker_amd import LONGVID_UNET_CONFIG, filler  # noqa: E402
from oracle import ref_ddpm, ref_unet  # noqa: E402

SLIM128_CFG = dict(image_size=32, in_channels=4, out_channels=4, model_channels=64, attention_resolutions=[4, 2, 1],
                   num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=2, use_scale_shift_norm=True,
                   resblock_updown=True, cond_model=False)
R, T = 32, 16
L = R * R + 2 * T * R


def save_parts(tag, out, budget=900 * 1024):
    """<tag>.npz holds everything but the taps and as many taps (in key order) as fit under `budget` compressed bytes; the rest go to
    <tag>_taps1.npz, <tag>_taps2.npz, ... under the same budget (no committed file above 1 MiB).  Readers merge <tag>.npz + <tag>_taps*.npz."""
    def size(v):
        b = io.BytesIO()
        np.savez_compressed(b, a=v)
        return len(b.getvalue())

    parts = [{k: v for k, v in out.items() if not k.startswith("tap_")}]
    used = sum(size(v) for v in parts[0].values())
    for k, v in out.items():
        if not k.startswith("tap_"):
            continue
        s = size(v)
        if used + s > budget:
            parts.append({})
            used = 0
        parts[-1][k] = v
        used += s
    for i, p in enumerate(parts):
        name = f"{tag}.npz" if i == 0 else f"{tag}_taps{i}.npz"
        np.savez_compressed(os.path.join(HERE, name), **p)
        print(f"{name} written ({len(p)} arrays, {os.path.getsize(os.path.join(HERE, name))} bytes)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slim-only", action="store_true", help="skip the full-width long-video model")
    args = ap.parse_args()
    torch.set_num_threads(os.cpu_count() or 8)
    UNetModel, DiffusionWrapper, D = mg.import_reference()
    report = []

    def check(name, a, b, tol):
        d = float((a - b).abs().max())
        report.append((name, d))
        print(f"  oracle vs reference  {name:38s} max-abs {d:.3e}")
        assert d <= tol, (name, d)

    def sample4(net, sd, cfg, cond, ic, B, seed, tag):
        S = 4
        with contextlib.redirect_stdout(io.StringIO()):
            dm = D.DDPM(net, channels=4, image_size=32, sampling_timesteps=S, w=0.0)
        noise = filler.noise_list(ref_ddpm.num_noise_draws(S, None), (B, 4, L), seed=seed, tag=f"{tag}.S{S}")
        with mg.injected_noise(noise) as (q, seeds), contextlib.redirect_stdout(io.StringIO()):
            z = dm.sample(batch_size=B, cond=cond, image_cond=ic)
        assert len(q) == 0 and seeds == [], (len(q), seeds)
        zo = ref_ddpm.ddim_sample(lambda a, b, c, d: ref_unet.unet_forward(sd, cfg, a, b, c, d, R, T), cond, ic, noise, S)
        check(f"{tag} sample_S{S}", zo, z, 1e-4)
        return z

    # ---------------------------------------------------------------- slim128
    tag, cfg, seed = "slim128", SLIM128_CFG, 21
    t0 = time.time()
    net = mg.build(UNetModel, DiffusionWrapper, cfg, seed)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    print(f"{tag} built+filled in {time.time() - t0:.1f}s ({sum(v.numel() for v in sd.values()) / 1e6:.1f} M params)")
    out = dict(seed=np.int64(seed))
    x, cond, ic = filler.synthetic_inputs(1, R, T, seed=seed, tag=tag)
    for tv in (999, 500, 0):
        t = torch.tensor([tv], dtype=torch.long)
        with torch.no_grad():
            eps = net(x, cond, ic, t)
        check(f"{tag} forward t={tv}", ref_unet.unet_forward(sd, cfg, x, cond, ic, t, R, T), eps, 2e-5)
        out[f"eps_t{tv}"] = eps.numpy()
    out["sample_S4"] = sample4(net, sd, cfg, cond, ic, 1, seed, tag).numpy()
    x2, cond2, ic2 = filler.synthetic_inputs(2, R, T, seed=seed, tag=tag + ".b2")
    t2 = torch.tensor([977, 13], dtype=torch.long)
    taps_ref, hooks, um = {}, [], net.diffusion_model
    for i, m in enumerate(um.input_attns):
        hooks.append(m.register_forward_hook(lambda mod, inp, o, i=i: taps_ref.__setitem__(f"in{i}", o.detach().clone())))
    hooks.append(um.mid_attn.register_forward_hook(lambda mod, inp, o: taps_ref.__setitem__("mid", o.detach().clone())))
    for i, m in enumerate(um.output_attns):
        hooks.append(m.register_forward_hook(lambda mod, inp, o, i=i: taps_ref.__setitem__(f"out{i}", o.detach().clone())))
    with torch.no_grad():
        eps2 = net(x2, cond2, ic2, t2)
    for h in hooks:
        h.remove()
    taps = {}
    check(f"{tag} B2 forward eps", ref_unet.unet_forward(sd, cfg, x2, cond2, ic2, t2, R, T, taps=taps), eps2, 2e-5)
    assert len(taps_ref) == 25, len(taps_ref)
    for k in taps_ref:
        check(f"{tag} B2 tap {k}", taps[k], taps_ref[k], 2e-5)
        out["tap_" + k] = taps_ref[k][..., ::7].contiguous().numpy()
    out["eps_b2"] = eps2.numpy()
    out["t_b2"] = t2.numpy()
    print(f"  {tag}: |eps| <= {max(float(np.abs(out[k]).max()) for k in ('eps_t999', 'eps_t500', 'eps_t0', 'eps_b2')):.2f}, "
          f"|tap| <= {max(float(v.abs().max()) for v in taps_ref.values()):.2f}")
    save_parts(tag, out)

    # ---------------------------------------------------------------- the shipped long-video config
    if not args.slim_only:
        tag, cfg, seed = "longvid", dict(LONGVID_UNET_CONFIG), 7
        t0 = time.time()
        net = mg.build(UNetModel, DiffusionWrapper, cfg, seed)
        sd = {k: v for k, v in net.state_dict().items()}
        assert len(sd) == 805, len(sd)
        print(f"{tag} built+filled in {time.time() - t0:.1f}s ({sum(v.numel() for v in sd.values()) / 1e6:.1f} M params)")
        out = dict(seed=np.int64(seed))
        out["keys"] = np.array(list(sd.keys()))
        out["shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        x, cond, ic = filler.synthetic_inputs(1, R, T, seed=seed, tag=tag)
        for tv in (999, 0):
            t = torch.tensor([tv], dtype=torch.long)
            with torch.no_grad():
                eps = net(x, cond, ic, t)
            check(f"{tag} forward t={tv}", ref_unet.unet_forward(sd, cfg, x, cond, ic, t, R, T), eps, 2e-5)
            out[f"eps_t{tv}"] = eps.numpy()
        out["sample_S4"] = sample4(net, sd, cfg, cond, ic, 1, seed, tag).numpy()
        np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **out)
        print(f"{tag}.npz written")

    with open(os.path.join(HERE, "PIN_REPORT_longvid.txt"), "a") as f:
        f.write(f"# make_golden_longvid.py{' --slim-only' if args.slim_only else ''}: torch {torch.__version__}, {torch.get_num_threads()} threads\n")
        for k, d in report:
            f.write(f"{k:44s} {d:.3e}\n")


if __name__ == "__main__":
    main()
