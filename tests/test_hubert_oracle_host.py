"""The HuBERT oracle (oracle/ref_hubert.py) in fp64 against what transformers' HubertModel and Wav2Vec2FeatureExtractor
computed (tests/golden/hubert.npz, written by tests/golden/make_golden_hubert.py): every stored array, each within the bar
stored beside it (10 x that call's own fp32-vs-fp64 drift).  This is the oracle's pin -- the relation test_oracle_golden.py
establishes for the UNet oracle -- and what lets tests/test_gpu_hubert_edges.py trust it at shapes the goldens do not cover.
CPU only."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from moditalker_amd import HUBERT_LARGE_CONFIG, filler
from oracle import ref_hubert

SEED = 83
NARROW = dict(HUBERT_LARGE_CONFIG, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, conv_dim=(32,) * 7,
              num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
TRUE_WIDTH = dict(HUBERT_LARGE_CONFIG, num_hidden_layers=1)
TAPS = ("extract_features", "after_pos_conv", "layer_0")
PIPE_N = 645000


def filler_state_dict(cfg, seed=SEED):
    """The state dict filler.fill_module_ gives moditalker_amd.HubertModel(**cfg), without building the module's tensors twice."""
    from moditalker_amd import HubertModel
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in HubertModel(**cfg).state_dict().items()}
    return {k: filler.fill_tensor(k, s, seed) for k, s in shapes.items()}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "hubert.npz"))


@pytest.fixture(scope="module")
def narrow_sd():
    return filler_state_dict(NARROW)


def _wave(tag, n):
    return filler.uniform_pm1(f"hubert.{tag}", (n,), SEED)


def _within(gold, key, got, rows=None, bar_key=None):
    want = torch.from_numpy(gold[key]).double()
    want = want if rows is None else want[rows]
    bar = float(gold[(bar_key or key) + "_bar"])
    assert tuple(got.shape) == tuple(want.shape), (key, tuple(got.shape), tuple(want.shape))
    d = float((got.double() - want).abs().max())
    print(f"{key}: oracle fp64 vs golden max-abs {d:.3e}  bar {bar:.3e}")
    assert d <= bar, (key, d, bar)


def test_normalize(gold):
    x = 0.5 * _wave("norm", 5000) + 0.25
    _within(gold, "norm", ref_hubert.normalize(x))
    assert ref_hubert.normalize(x, torch.float32).dtype == torch.float32
    assert float(ref_hubert.normalize(torch.tensor([0.7]))[0]) == 0.0


@pytest.mark.parametrize("n,frames", [(400, 1), (4000, 12)])
def test_narrow_forward_and_taps(gold, narrow_sd, n, frames):
    taps = {}
    out = ref_hubert.hubert_forward(narrow_sd, NARROW, _wave(f"narrow.n{n}", n)[None], taps=taps)
    assert tuple(out.shape) == (1, frames, 64) and out.dtype == torch.float64
    _within(gold, f"narrow_n{n}_out", out[0])
    for tap in TAPS:
        _within(gold, f"narrow_n{n}_{tap}", taps[tap])


def test_narrow_two_clips_as_a_batch(gold, narrow_sd):
    """The golden holds the two clips run singly; the oracle's batch of 2 must give the same rows (no leak across clips)."""
    x = torch.stack([_wave("narrow.n12240.0", 12240), _wave("narrow.n12240.1", 12240)])
    taps = {}
    out = ref_hubert.hubert_forward(narrow_sd, NARROW, x, taps=taps)
    assert tuple(out.shape) == (2, 38, 64)
    _within(gold, "narrow_n12240_out", out.reshape(76, 64))
    for tap in TAPS:
        _within(gold, f"narrow_n12240_{tap}", taps[tap])


def test_narrow_pipeline_case_clip_by_clip(gold, narrow_sd):
    """The 645000-sample utterance, normalised as a whole and cut as get_hubert_from_speech cuts it: 1000 + 1000 + 15 rows.  Rows
    0..999 (the full 320080-sample clip) also carry a bar of their own."""
    v = ref_hubert.normalize(0.3 * _wave("pipe", PIPE_N) + 0.1)
    outs = [ref_hubert.hubert_forward(narrow_sd, NARROW, v[None, a:b])[0] for a, b in ((0, 320080), (320000, 640080), (640000, PIPE_N))]
    assert [int(o.shape[0]) for o in outs] == [1000, 1000, 15]
    _within(gold, "narrow_pipe645000", torch.cat(outs))
    _within(gold, "narrow_pipe645000", outs[0], rows=slice(0, 1000), bar_key="narrow_n320080")


def test_true_width_one_layer(gold):
    out = ref_hubert.hubert_forward(filler_state_dict(TRUE_WIDTH), TRUE_WIDTH, _wave("true_width.n16080", 16080)[None])
    assert tuple(out.shape) == (1, 50, 1024)
    _within(gold, "true_width_n16080_out", out[0])


def test_num_frames_agrees_with_the_package():
    from moditalker_amd import hubert
    for n in (1, 399, 400, 719, 720, 12240, 320080):
        assert ref_hubert.num_frames(n, NARROW["conv_kernel"], NARROW["conv_stride"]) == hubert.num_frames(n)
    assert ref_hubert.num_frames(5, (2,), (3,)) == 2 and ref_hubert.num_frames(1, (2,), (3,)) == 0
