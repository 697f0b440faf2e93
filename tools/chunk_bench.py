#!/usr/bin/env python3
"""Time the per-chunk glue around the MToV loop: pipeline.MToVSampler.run_identity (host-built float conditioning videos,
host frame finishing) against run_identity_device (8-bit frames and integer landmarks up, 8-bit frames down, csrc/frames.hip) on
the same build.  Two chained chunks (use_last_as_reference) of one clip at full size: 256 x 256 autoencoder, the base UNet at
R = 32, filler weights, source frames of 256 x 256 and of one larger size.  No speed bar: the record says what came out.

  python tools/chunk_bench.py --gpu [--out FILE] [--steps S] [--big 634]

Both paths start from the same 8-bit source frames, landmark arrays and noise, and each is timed end to end with the wall clock
(the host stages are the point), after one untimed pass.  The host path builds x_ref / x / x_l / masked_x as the reference's
loader does: crop_lower_half per frame, landmarks_to_images, and -- for sources that are not 256 x 256 -- the centre crop and
F.interpolate of resize_crop on the CPU with torch, which the project itself does not have; that stage is timed separately
(`host_build_ms`) from the loop (`loop_ms`, upload included).  The record (default profiles/chunk_loop.json) also says whether the
two paths' frames agree."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "chunk_loop.json")
SEED = 61


def host_inputs(P, torch, np, TF, ref, vid, lm, res):
    """(x_ref, x, x_l, masked_x) in 0..255 float [1, T, 3, res, res] on the host, the loader's way (dataloader_sample.py:181-247)."""
    T, h, w = vid.shape[1], vid.shape[3], vid.shape[4]

    def resize_crop(v):                                                  # data_utils.py:73-98 on [T, 3, h, w] float
        if (h, w) == (res, res):
            return v
        if h > w:
            v = v[:, :, (h - w) // 2:(h - w) // 2 + w]
        else:
            v = v[:, :, :, (w - h) // 2:(w - h) // 2 + h]
        return TF.interpolate(v, size=res, mode="bilinear", align_corners=False)
    x = resize_crop(vid[0].float())[None]
    x_ref = resize_crop(ref[0].float().expand(T, -1, -1, -1))[None].contiguous()
    masked = torch.from_numpy(np.stack([P.crop_lower_half(vid[0, f].float().numpy(), lm[f]) for f in range(T)])).float()
    masked_x = resize_crop(masked)[None]
    x_l = torch.from_numpy(P.landmarks_to_images(lm, WH=w)).float().permute(0, 3, 1, 2)[None].contiguous()
    return x_ref, x, x_l, masked_x


def gpu_child(args):
    import numpy as np
    import torch
    import torch.nn.functional as TF
    from moditalker_amd import BASE_AE_DDCONFIG, BASE_UNET_CONFIG, DDPM, DiffusionWrapper, UNetModel, ViTAutoencoder, filler
    from moditalker_amd import pipeline as P
    dev = torch.device("cuda:0")
    R, T, res, S = 32, 16, 256, args.steps
    net = DiffusionWrapper(UNetModel(**BASE_UNET_CONFIG, frames=T, max_batch=1)).eval()
    filler.fill_module_(net, seed=SEED, skip_prefixes=("output_bg_",))
    ae = ViTAutoencoder(4, dict(BASE_AE_DDCONFIG, resolution=res), max_batch=1).eval()
    filler.fill_autoencoder_(ae, seed=SEED + 1)
    net, ae = net.to(dev), ae.to(dev)
    dm = DDPM(net, channels=4, image_size=R, sampling_timesteps=S, w=0.0).to(dev)
    sampler = P.MToVSampler(dm, ae, latent_res=R)
    L = R * R + 2 * T * R
    noises = [[n.to(dev) for n in filler.noise_list(S, (1, 4, L), seed=SEED + it, tag="chunkbench.noise")] for it in range(2)]
    rec = dict(what="two chained chunks (use_last_as_reference) of one clip: run_identity (host glue) vs run_identity_device, wall clock, ms",
               device=torch.cuda.get_device_name(0), sampling_steps=S, frames=T, resolution=res, repeats=args.iters)
    for side in (256, args.big):
        g = torch.Generator().manual_seed(side)
        chunks = []
        for it in range(2):
            vid = torch.randint(0, 256, (1, T, 3, side, side), generator=g, dtype=torch.uint8)
            lm = np.stack([np.stack([np.array([0.2 * side + 0.07 * side * (i % 9) + f + it, 0.25 * side + 0.06 * side * (i // 9) + f])
                                     for i in range(68)]) for f in range(T)])
            chunks.append((vid[:, :1].contiguous(), vid, lm))

        def host_path():
            t0 = time.perf_counter()
            built = [host_inputs(P, torch, np, TF, ref, vid, lm, res) for ref, vid, lm in chunks]
            t1 = time.perf_counter()
            out = sampler.run_identity((tuple(t.to(dev) for t in c) for c in built), use_last_as_reference=True, noise_per_chunk=noises)
            torch.cuda.synchronize()
            return out, 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)

        def device_path():
            t0 = time.perf_counter()
            out = sampler.run_identity_device(((ref, vid, lm[None], lm[None, :, 33, 1]) for ref, vid, lm in chunks),
                                              use_last_as_reference=True, noise_per_chunk=noises)
            torch.cuda.synchronize()
            return out, 0.0, 1e3 * (time.perf_counter() - t0)

        r = {}
        outs = {}
        for name, fn in (("host", host_path), ("device", device_path)):
            fn()                                                        # untimed pass: contexts, weights, graphs, allocator
            runs = [fn() for _ in range(args.iters)]
            outs[name] = np.stack(runs[-1][0])
            build = sorted(x[1] for x in runs)
            loop = sorted(x[2] for x in runs)
            total = sorted(x[1] + x[2] for x in runs)
            r[name] = dict(host_build_ms=build[len(build) // 2], loop_ms=loop[len(loop) // 2], total_ms_median=total[len(total) // 2],
                           total_ms_min=total[0], total_ms_max=total[-1])
        d = np.abs(outs["host"].astype(np.int32) - outs["device"].astype(np.int32))
        r["frames_differ"] = int((d != 0).sum())
        r["frames_values"] = int(d.size)
        r["frames_max_count_gap"] = int(d.max())
        r["device_over_host_total"] = r["device"]["total_ms_median"] / r["host"]["total_ms_median"]
        rec[f"source_{side}"] = r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--steps", type=int, default=50, help="DDIM steps per chunk")
    ap.add_argument("--big", type=int, default=634, help="side of the larger source frames")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU measurement may take")
    args = ap.parse_args()
    if args.child:
        return gpu_child(args)
    if args.gpu:      # the GPU step runs in a fresh process under its own time limit
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--out", args.out,
               "--steps", str(args.steps), "--big", str(args.big), "--iters", str(args.iters)]
        rc = subprocess.run(cmd).returncode
        if rc:
            sys.exit(rc)


if __name__ == "__main__":
    main()
