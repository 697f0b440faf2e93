#!/usr/bin/env python3
"""Golden vectors for the HuBERT stage from the library the reference calls: transformers' HubertModel
(data/data_utils/preprocess/process_audio.py:16 loads it) built offline from a HubertConfig, and
Wav2Vec2FeatureExtractor's normalisation.  CPU only; the reference tree is not imported.

Weights: filler.fill_module_(m, seed) by state-dict key (moditalker_amd.HubertModel has the same keys, so the tests fill
the same values).  Inputs: filler.uniform_pm1.  hubert.npz holds outputs and bars, never weights.

Cases
  norm        5000 samples with mean 0.25: the extractor's (x - mean) / sqrt(var + 1e-7).
  narrow      hidden 64, 2 layers, 2 heads, ff 128, conv dims 32 x 7, positional conv k = 16 in 4 groups:
              400 samples (1 frame), 4000 (12), 12240 (38; two clips, also run as a batch of 2): output and the taps
              extract_features / after_pos_conv / layer_0; the utterance of 645000 samples clip by clip as
              get_hubert_from_speech cuts it (320080 | 320080 | 5000 samples -> 1000 + 1000 + 15 rows; its first clip is the
              320080-sample case).
  true_width  hidden 1024, 16 heads of 64, ff 4096, 1 layer, conv dims 512 x 7, positional conv k = 128 in 16 groups,
              16080 samples -> 50 frames.
Every stored call is also run in float64 (model.double()); its bar is 10 x max|fp32 - fp64| of that call (the rule atom.npz
uses for a single forward: the margin is for a different summation order), stored as <key>_bar and listed in
PIN_REPORT_hubert.txt.  Also written: hubert_large_keys.txt, the names and shapes of the large model's state dict (built on
the meta device)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
from moditalker_amd import filler  # noqa: E402
from moditalker_amd.hubert import HUBERT_LARGE_CONFIG  # noqa: E402

SEED = 83
NARROW = dict(HUBERT_LARGE_CONFIG, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, conv_dim=(32,) * 7,
              num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
TRUE_WIDTH = dict(HUBERT_LARGE_CONFIG, num_hidden_layers=1)
PIPE_N = 645000


def wave(tag, n):
    return filler.uniform_pm1(f"hubert.{tag}", (n,), SEED)


def utterance():
    """The raw 645000-sample utterance of the pipeline case (mean 0.1, not unit variance: the normalisation has work to do)."""
    return (0.3 * wave("pipe", PIPE_N) + 0.1).numpy()


def normalise(x):
    return (x - x.mean()) / np.sqrt(x.var() + 1e-7)


def build(cfg, double):
    from transformers import HubertConfig, HubertModel
    m = HubertModel(HubertConfig(**cfg)).eval()
    filler.fill_module_(m, seed=SEED)
    return m.double() if double else m


@torch.no_grad()
def run(m, x):
    """x [B, n] -> dict(out, extract_features, after_pos_conv, layer_0), rows flattened over the batch."""
    got = {}
    h = m.encoder.layers[0].register_forward_hook(lambda mod, a, o: got.__setitem__("layer_0", o[0]))
    try:
        r = m(x.to(next(m.parameters()).dtype), output_hidden_states=True)
    finally:
        h.remove()
    feat = m.feature_extractor(x.to(next(m.parameters()).dtype)).transpose(1, 2)
    flat = lambda t: t.reshape(-1, t.shape[-1])
    return dict(out=flat(r.last_hidden_state), extract_features=flat(feat), after_pos_conv=flat(r.hidden_states[0]), layer_0=flat(got["layer_0"]))


def main():
    out, lines = {}, []

    def store(key, v32, v64, note=""):
        drift = float((v32.double() - v64).abs().max())
        out[key] = v32.float().numpy()
        out[key + "_bar"] = np.float64(10.0 * drift)
        lines.append(f"{key:40s} max|fp32-fp64| {drift:.3e}   bar {10.0 * drift:.3e}   (10 x drift; max|out| {float(v32.abs().max()):.3f}{note})")

    # ---- normalisation: the extractor itself in fp32, the formula in fp64
    from transformers import Wav2Vec2FeatureExtractor
    x = (0.5 * wave("norm", 5000) + 0.25).numpy()
    ext = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=True)
    e32 = torch.from_numpy(np.asarray(ext(x, sampling_rate=16000, return_tensors="np").input_values[0], dtype=np.float32))
    f32 = torch.from_numpy(normalise(x).astype(np.float32))
    lines.append(f"extractor vs formula (fp32)              max-abs {float((e32 - f32).abs().max()):.3e}")
    store("norm", e32, torch.from_numpy(normalise(x.astype(np.float64))))

    # ---- narrow
    m32, m64 = build(NARROW, False), build(NARROW, True)
    for n in (400, 4000):
        x = wave(f"narrow.n{n}", n)[None]
        r32, r64 = run(m32, x), run(m64, x)
        for k in r32:
            store(f"narrow_n{n}_{k}", r32[k], r64[k])
    x = torch.stack([wave("narrow.n12240.0", 12240), wave("narrow.n12240.1", 12240)])
    r32 = [run(m32, x[b:b + 1]) for b in range(2)]      # clip by clip: the batch test compares against these
    r64 = [run(m64, x[b:b + 1]) for b in range(2)]
    for k in r32[0]:
        store(f"narrow_n12240_{k}", torch.cat([r32[0][k], r32[1][k]]), torch.cat([r64[0][k], r64[1][k]]), "; clips 0 | 1")
    u = utterance()
    v32 = torch.from_numpy(normalise(u).astype(np.float32))
    v64 = torch.from_numpy(normalise(u.astype(np.float64)))
    spans = [(0, 320080), (320000, 640080), (640000, PIPE_N)]
    p32 = [run(m32, v32[a:b][None])["out"] for a, b in spans]
    p64 = [run(m64, v64[a:b][None])["out"] for a, b in spans]
    assert [int(t.shape[0]) for t in p32] == [1000, 1000, 15]
    store("narrow_pipe645000", torch.cat(p32), torch.cat(p64), "; 1000 | 1000 | 15 rows, normalised utterance")
    drift = float((p32[0].double() - p64[0]).abs().max())
    out["narrow_n320080_bar"] = np.float64(10.0 * drift)      # (the output is rows 0..999 of narrow_pipe645000)
    lines.append(f"{'narrow_n320080 (= pipe rows 0..999)':40s} max|fp32-fp64| {drift:.3e}   bar {10.0 * drift:.3e}   (10 x drift)")

    # ---- true width, one layer
    m32, m64 = build(TRUE_WIDTH, False), build(TRUE_WIDTH, True)
    x = wave("true_width.n16080", 16080)[None]
    store("true_width_n16080_out", run(m32, x)["out"], run(m64, x)["out"])

    np.savez_compressed(os.path.join(HERE, "hubert.npz"), **out)
    with open(os.path.join(HERE, "PIN_REPORT_hubert.txt"), "w") as f:
        f.write("HuBERT goldens (make_golden_hubert.py): transformers' own fp32 vs fp64 runs, and the bars the tests read from hubert.npz\n")
        for ln in lines:
            f.write(ln + "\n")
            print(ln)
    from transformers import HubertConfig, HubertModel
    with torch.device("meta"):
        big = HubertModel(HubertConfig(**HUBERT_LARGE_CONFIG))
    with open(os.path.join(HERE, "hubert_large_keys.txt"), "w") as f:
        for k, v in big.state_dict().items():
            f.write(f"{k} {','.join(map(str, v.shape))}\n")
    print("hubert.npz written:", os.path.getsize(os.path.join(HERE, "hubert.npz")), "bytes")


if __name__ == "__main__":
    main()
