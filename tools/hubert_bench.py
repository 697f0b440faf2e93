#!/usr/bin/env python3
"""Time HuBERT feature extraction at the full configuration (moditalker_amd.HUBERT_LARGE_CONFIG: 24 layers of width 1024,
filler weights) on one full 20-second clip (320080 samples -> 1000 frames) and on a batch of 3 such clips, and record it.
No speed bar and no comparison: there is no earlier GPU path for this stage.

  python tools/hubert_bench.py --gpu [--out FILE]     hipEvents around whole forwards after warm-up, then one per-launch pass
                                                      (mtv_hubert_profile); the measurement runs in a child process under its
                                                      own `timeout`

The record (default profiles/hubert_extract.json) carries the ms figures, the FLOP count of the launch chain (2 M K N per
GEMM, 4 T^2 hidden per attention, 2 k per conv-1 output; LayerNorm / GELU not counted), the floor that count implies at the
exact-f32 MFMA peak (157.3 TFLOP/s, the MI355X's FP32 matrix rate), and the per-launch table of the one-clip forward."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "hubert_extract.json")
SEED = 5
F32_MFMA_PEAK = 157.3e12
CLIP = 320080


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
    print(json.dumps({key: {k: v for k, v in rec.items() if k != "per_launch"}}))


def gpu_child(args):
    import ctypes as C
    import torch
    from moditalker_amd import HUBERT_LARGE_CONFIG, HubertModel, _lib, filler
    dev = torch.device("cuda:0")
    m = HubertModel(max_batch=3, **HUBERT_LARGE_CONFIG).eval()
    filler.fill_module_(m, seed=SEED)
    m = m.to(dev)
    lib = _lib.load()
    rec = dict(what="HubertModel.forward on full 20 s clips (320080 samples -> 1000 frames), filler weights, hipEvents around the whole call",
               device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, f32_mfma_peak_tflops=F32_MFMA_PEAK / 1e12)
    for B in (1, 3):
        x = filler.uniform_pm1("hubert.bench.wave", (B, CLIP), SEED).to(dev)
        for _ in range(args.warmup):
            out = m(x).last_hidden_state
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = m(x).last_hidden_state
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        n = C.c_int(0)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.mtv_hubert_profile(m._ctx, x.data_ptr(), CLIP, B, 1, None, 0, C.byref(n), stream), "mtv_hubert_profile")
        tab = (_lib.MtvOpTime * n.value)()
        _lib.check(lib.mtv_hubert_profile(m._ctx, x.data_ptr(), CLIP, B, args.iters, tab, n.value, C.byref(n), stream), "mtv_hubert_profile")
        flops = sum(t.flops for t in tab)
        r = dict(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1], launches=n.value, gflop=flops / 1e9,
                 f32_mfma_floor_ms=1e3 * flops / F32_MFMA_PEAK, tflops_at_median=flops / (ms[len(ms) // 2] * 1e-3) / 1e12,
                 finite=bool(torch.isfinite(out).all()), out_abs_max=float(out.abs().max()))
        if B == 1:      # per-launch table: layers 1.. repeat layer 0's shapes, so they are summed under one name
            rows = {}
            for t in tab:
                name = t.name.decode()
                parts = name.split(".")
                if parts[0].startswith("L") and parts[0][1:].isdigit() and parts[0] != "L0":
                    name = "L1..L23." + parts[1]
                a = rows.setdefault(name, dict(ms=0.0, gflop=0.0, launches=0))
                a["ms"] += t.ms
                a["gflop"] += t.flops / 1e9
                a["launches"] += 1
            r["per_launch"] = [dict(name=k, **v) for k, v in rows.items()]
        rec[f"batch{B}"] = r
    merge(args.out, "hip_mi355x", rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU measurement may take")
    args = ap.parse_args()
    if args.child:
        return gpu_child(args)
    if args.gpu:      # the GPU step runs in a fresh process under its own time limit
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--out", args.out,
               "--warmup", str(args.warmup), "--iters", str(args.iters)]
        rc = subprocess.run(cmd).returncode
        if rc:
            sys.exit(rc)


if __name__ == "__main__":
    main()
