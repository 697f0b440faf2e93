#!/usr/bin/env python3
"""Time one 50-step AToM sample at the full configuration (moditalker_amd.ATOM_CONFIG: 156 frames, d_model 512, 8 layers,
guidance pair) and record it beside the reference's own time on the CPU.  Two numbers, no comparison claimed: there is no
earlier GPU path for this stage.

  python tools/atom_bench.py --gpu [--out FILE]                  the HIP path, hipEvents around whole samples after warm-up; the
                                                                 measurement runs in a child process under its own `timeout`
  python tools/atom_bench.py --reference-cpu PATH [--out FILE]   the reference (PATH = its AToM directory) on the CPU at 8 threads

Each mode merges its record into the JSON file (default profiles/atom_sample.json)."""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "atom_sample.json")
SEED = 5


def inputs(cfg, B):
    from moditalker_amd import filler
    L = cfg["seq_len"]
    face = filler.uniform_pm1("atom.bench.face", (B, 1, 204), SEED).repeat(1, L, 1)
    cond = filler.uniform_pm1("atom.bench.cond", (B, 2 * L, cfg["cond_feature_dim"]), SEED)
    return face, cond


def merge(path, key, rec):
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = rec
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({key: rec}))


def gpu_child(args):
    import ctypes as C
    import torch
    from moditalker_amd import ATOM_CONFIG, ATOM_DIFFUSION_CONFIG, GaussianDiffusion, MotionDecoder, _lib, filler
    dev = torch.device("cuda:0")
    m = MotionDecoder(max_batch=args.batch, **ATOM_CONFIG).eval()
    freqs = m.rotary.freqs.clone()
    filler.fill_module_(m, seed=SEED)
    m.rotary.freqs.copy_(freqs)
    dif = GaussianDiffusion(m, ATOM_CONFIG["seq_len"], 204, **ATOM_DIFFUSION_CONFIG).to(dev)
    face, cond = (t.to(dev) for t in inputs(ATOM_CONFIG, args.batch))
    shape = (args.batch, ATOM_CONFIG["seq_len"], 204)
    noise = torch.stack(filler.noise_list(50, shape, SEED, tag="atom.bench.noise")).to(dev)
    for _ in range(args.warmup):
        out = dif.ddim_sample(shape, face, None, cond, noise=noise)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = dif.ddim_sample(shape, face, None, cond, noise=noise)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    n = C.c_int(0)
    _lib.check(_lib.load().mtv_atom_num_launches(m._ctx, args.batch, C.byref(n)), "mtv_atom_num_launches")
    ms.sort()
    merge(args.out, "hip_mi355x", dict(what="one 50-step ddim_sample, guidance pair as one batch, hipEvents around the whole call (set-up + 50 graph replays)",
                                       device=torch.cuda.get_device_name(0), batch=args.batch, warmup=args.warmup, iters=args.iters,
                                       ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1], launches_per_step=n.value,
                                       finite=bool(torch.isfinite(out).all()), out_abs_max=float(out.abs().max())))


def reference_cpu(args):
    import torch
    import torch.nn.functional as F
    from moditalker_amd import ATOM_CONFIG, ATOM_DIFFUSION_CONFIG, filler
    for name in ("p_tqdm", "cv2"):      # imported by the reference's diffusion.py, unused when sampling
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].p_map = None
    sys.path.insert(0, args.reference_cpu)
    from model.diffusion import GaussianDiffusion
    from model.model import MotionDecoder
    torch.set_num_threads(args.threads)
    m = MotionDecoder(activation=F.gelu, **ATOM_CONFIG).eval()
    freqs = m.rotary.freqs.clone()
    filler.fill_module_(m, seed=SEED)
    m.rotary.freqs.copy_(freqs)
    dif = GaussianDiffusion(m, ATOM_CONFIG["seq_len"], 204, **ATOM_DIFFUSION_CONFIG)
    face, cond = inputs(ATOM_CONFIG, args.batch)
    shape = (args.batch, ATOM_CONFIG["seq_len"], 204)
    s = []
    for i in range(1 + args.iters):      # first run: warm-up
        t0 = time.perf_counter()
        dif.ddim_sample(shape, face, None, cond)
        s.append(time.perf_counter() - t0)
    s = sorted(s[1:])
    merge(args.out, "reference_cpu", dict(what="the reference's GaussianDiffusion.ddim_sample (PyTorch eager, fp32) on the CPU", threads=args.threads,
                                          torch=torch.__version__, batch=args.batch, iters=args.iters, ms_median=1e3 * s[len(s) // 2], ms_min=1e3 * s[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--reference-cpu", metavar="PATH")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=240, help="seconds the GPU measurement may take")
    args = ap.parse_args()
    if args.child:
        return gpu_child(args)
    if args.gpu:      # the GPU step runs in a fresh process under its own time limit
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--out", args.out,
               "--batch", str(args.batch), "--warmup", str(args.warmup), "--iters", str(args.iters)]
        rc = subprocess.run(cmd).returncode
        if rc:
            sys.exit(rc)
    if args.reference_cpu:
        reference_cpu(args)


if __name__ == "__main__":
    main()
