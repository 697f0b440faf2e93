#!/usr/bin/env python3
"""The shipped long-video UNet (LONGVID_UNET_CONFIG: model_channels 256, 8 heads, cond_model; 830 M parameters) at full width on the GPU:
parity against tests/golden/longvid.npz (eps at t = 999 / 0 at 2e-4, the 4-step sample at 1e-3) and the per-op table of one sampler step,
with the fused d = 128 attention (k_deep_attn<128>) and with the fallback form of the same build (MTV_DEEP_OPT_NO_FUSED_ATTN: finalize +
qkv conv + k_attention + proj_out conv).  Too slow for the suite (about 20 s of host time to build and fill the model), so it is a tool.
Exits non-zero on a parity miss.  Usage: python tools/longvid_check.py [--reps N]   (profiles/r07_longvid_check.txt is its output)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moditalker_amd import DDPM, LONGVID_UNET_CONFIG, DiffusionWrapper, UNetModel, _lib, filler  # noqa: E402

FWD_TOL, SAMPLE_TOL, SEED = 2e-4, 1e-3, 7


def block_ops(table):
    """{attention block: its launches} for the d = 128 blocks of the 128- and 32-token levels (fin:<nm>.in, <nm>.qkv, attn:<nm>, <nm>.proj)."""
    blocks = {}
    for p in table:
        n = p["name"]
        if n.startswith("attn:") and " d128 " in n and ("[L128 " in n or "[L32 " in n):
            blocks[n[5:n.index("[")]] = []
    for p in table:
        for nm, ops in blocks.items():
            if nm + "[" in p["name"] or nm + "." in p["name"]:
                ops.append(p)
    return blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="repeats of every timing (the spread is printed)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(ROOT, "tests", "golden", "longvid.npz"))
    lib = _lib.load()
    t0 = time.time()
    host = DiffusionWrapper(UNetModel(**LONGVID_UNET_CONFIG, frames=16, max_batch=1)).eval()
    t1 = time.time()
    filler.fill_module_(host, seed=SEED, skip_prefixes=("output_bg_",))
    sd = {k: v.detach().clone() for k, v in host.state_dict().items()}
    print(f"long-video UNet: {len(sd)} keys, {sum(v.numel() for v in sd.values()) / 1e6:.1f} M parameters; built in {t1 - t0:.1f} s, filled in {time.time() - t1:.1f} s")
    assert [str(k) for k in g["keys"]] == list(sd.keys()), "state-dict keys differ from the reference manifest"
    del host
    x, cond, ic = (v.to(dev) for v in filler.synthetic_inputs(1, 32, 16, seed=SEED, tag="longvid"))
    S = 4
    noise = [z.to(dev) for z in filler.noise_list(S, (1, 4, 2048), seed=SEED, tag=f"longvid.S{S}")]
    bad = 0
    results = {}
    for what, mask in (("fused d128 attention (default)", -1), ("fallback: k_attention + proj_out conv (MTV_DEEP_OPT_NO_FUSED_ATTN)", 8)):
        _lib.check(lib.mtv_debug_deep_options(mask), "mtv_debug_deep_options")
        try:
            net = DiffusionWrapper(UNetModel(**LONGVID_UNET_CONFIG, frames=16, max_batch=1)).eval()
            net.load_state_dict(sd)
            net = net.to(dev)
            print(f"\n==== {what}")
            for tv in (999, 0):
                e = float((net(x, cond, ic, torch.tensor([tv], device=dev)).cpu() - torch.from_numpy(g[f"eps_t{tv}"])).abs().max())
                ok = e <= FWD_TOL
                bad += not ok
                print(f"eps t={tv:<3d} vs reference golden: max-abs {e:.3e} (tol {FWD_TOL:.0e})  {'PASS' if ok else 'FAIL'}")
            dm = DDPM(net, channels=4, image_size=32, sampling_timesteps=S, w=0.0).to(dev)
            z = dm.sample(batch_size=1, cond=cond, image_cond=ic, noise=noise)
            e = float((z.cpu() - torch.from_numpy(g[f"sample_S{S}"])).abs().max())
            ok = e <= SAMPLE_TOL
            bad += not ok
            print(f"{S}-step sample vs reference golden: max-abs {e:.3e} (tol {SAMPLE_TOL:.0e})  {'PASS' if ok else 'FAIL'}")
            # per-op table of one sampler step (plain launches, hipEvent per launch), `reps` times: medians per op
            runs = [net.diffusion_model.profile_forward(1, 5, dev, step=True) for _ in range(args.reps)]
            table = [dict(p, ms=float(np.median([r[i]["ms"] for r in runs]))) for i, p in enumerate(runs[0])]
            print(f"per-op table of one sampler step ({len(table)} launches; median of {args.reps} x 5 iterations, us):")
            for p in table:
                print(f"  {p['ms'] * 1e3:9.2f}  {p['name']}")
            blocks = block_ops(table)
            sums = [sum(p["ms"] for nm in block_ops(r) for p in block_ops(r)[nm]) * 1e3 for r in runs]
            by_level = {lv: sum(p["ms"] for ops in blocks.values() for p in ops if any(f"[{lv} " in q["name"] for q in ops if q["name"].startswith("attn:"))) * 1e3
                        for lv in ("L128", "L32")}
            steps = [sum(p["ms"] for p in r) * 1e3 for r in runs]
            # the step as DDPM.sample replays it (one graph per step): wall time of a 20-step sample / 20
            dm20 = DDPM(net, channels=4, image_size=32, sampling_timesteps=20, w=0.0).to(dev)
            n20 = [z.to(dev) for z in filler.noise_list(20, (1, 4, 2048), seed=SEED, tag="longvid.S20")]
            dm20.sample(batch_size=1, cond=cond, image_cond=ic, noise=n20)
            walls = []
            for _ in range(args.reps):
                torch.cuda.synchronize(dev)
                w0 = time.perf_counter()
                dm20.sample(batch_size=1, cond=cond, image_cond=ic, noise=n20)
                torch.cuda.synchronize(dev)
                walls.append((time.perf_counter() - w0) / 20 * 1e3)
            results[what] = (sums, steps, walls, by_level, len(blocks))
            print(f"d128 attention blocks of the deep levels: {len(blocks)} blocks, {sum(len(o) for o in blocks.values())} launches")
            print(f"  sum of their launches, us per step: " + " ".join(f"{v:.1f}" for v in sums) + f"   (128 tokens {by_level['L128']:.1f}, 32 tokens {by_level['L32']:.1f})")
            print(f"  sum of all launches, us per step:   " + " ".join(f"{v:.1f}" for v in steps))
            print(f"  sampler step, ms (20-step sample / 20): " + " ".join(f"{v:.3f}" for v in walls))
            del net, dm, dm20
            torch.cuda.empty_cache()
        finally:
            lib.mtv_debug_deep_options(-1)
    print("\n==== fused against fallback (same build, same box; median [min .. max])")
    for what, (sums, steps, walls, by_level, nb) in results.items():
        print(f"{what}:")
        print(f"  d128 attention blocks ({nb}): {np.median(sums):.1f} us [{min(sums):.1f} .. {max(sums):.1f}]   128 tokens {by_level['L128']:.1f} us, 32 tokens {by_level['L32']:.1f} us")
        print(f"  sampler step: {np.median(walls):.3f} ms [{min(walls):.3f} .. {max(walls):.3f}]")
    print("\nLONGVID CHECK " + ("FAILED" if bad else "OK"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
