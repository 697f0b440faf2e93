"""The HuBERT stage on the GPU (csrc/hubert.hip behind moditalker_amd.HubertModel and pipeline.audio_to_hubert) against what
transformers' HubertModel and Wav2Vec2FeatureExtractor computed (tests/golden/hubert.npz, tests/golden/make_golden_hubert.py).

Every bar is read from the golden file: 10 x the max-abs difference between the library's own fp32 and fp64 runs of that
call (tests/golden/PIN_REPORT_hubert.txt lists them; 1.5e-5 .. 3.2e-5 on outputs of magnitude 2 .. 5).

Equalities asserted bit for bit, and why they must hold: k_hub_gemm computes an output element from its own row, its column
and the weights with K walked in index order by one wave; k_hub_ln and k_tok_attn work per row / per (clip, head, query
tile) with keys in index order; the normalisation adds fixed partial sums in index order.  No atomics anywhere, so neither
a repeated call nor the batch size can change a bit."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, report

pytestmark = pytest.mark.gpu

SEED = 83
NARROW = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, conv_dim=(32,) * 7,
              num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
TAPS = ("extract_features", "after_pos_conv", "layer_0")
PIPE_N = 645000


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "hubert.npz"))


def _model(over, **kw):
    from moditalker_amd import HUBERT_LARGE_CONFIG, HubertModel, filler
    m = HubertModel(**dict(HUBERT_LARGE_CONFIG, **over), **kw).eval()
    filler.fill_module_(m, seed=SEED)
    return m.to("cuda:0")


@pytest.fixture(scope="module")
def narrow():
    m = _model(NARROW, max_batch=2)
    m.debug_taps = True
    return m


def _wave(tag, n):
    from moditalker_amd import filler
    return filler.uniform_pm1(f"hubert.{tag}", (n,), SEED)


def _utterance():
    return (0.3 * _wave("pipe", PIPE_N) + 0.1).numpy()


def _check(name, got, gold, key, want=None, bar_key=None):
    want = torch.from_numpy(gold[key]) if want is None else want
    bar = float(gold[(bar_key or key) + "_bar"])
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    d = report(name, float((got.cpu().double() - want.double()).abs().max()), bar)
    print(f"{name}: max-abs {d:.3e}  bar {bar:.3e}")
    assert d <= bar, (name, d, bar)


def test_normalize(gold, narrow):
    x = (0.5 * _wave("norm", 5000) + 0.25).to("cuda:0")
    a = narrow.normalize(x)
    _check("hubert normalise 5000 samples, mean 0.25", a, gold, "norm")
    assert torch.equal(narrow.normalize(x), a)


@pytest.mark.parametrize("n,frames", [(400, 1), (4000, 12)])
def test_narrow_forward_and_taps(gold, narrow, n, frames):
    x = _wave(f"narrow.n{n}", n)[None].to("cuda:0")
    out = narrow(x).last_hidden_state
    assert tuple(out.shape) == (1, frames, 64)
    _check(f"hubert narrow n={n} output", out[0], gold, f"narrow_n{n}_out")
    for tap in TAPS:
        _check(f"hubert narrow n={n} {tap}", narrow.tap(tap), gold, f"narrow_n{n}_{tap}")


@pytest.fixture(scope="module")
def batch2(narrow):
    x = torch.stack([_wave("narrow.n12240.0", 12240), _wave("narrow.n12240.1", 12240)]).to("cuda:0")
    both = narrow(x).last_hidden_state
    taps = {t: narrow.tap(t) for t in TAPS}
    return x, both, taps


def test_narrow_38_frames_single_clip(gold, narrow, batch2):
    """38 frames: no multiple of a 16-, 32- or 64-row tile, and shorter than the positional conv's reach on both sides."""
    x = batch2[0]
    out = narrow(x[:1]).last_hidden_state
    assert tuple(out.shape) == (1, 38, 64)
    _check("hubert narrow n=12240 output (clip 0)", out[0], gold, "narrow_n12240_out", want=torch.from_numpy(gold["narrow_n12240_out"][:38]))
    for tap in TAPS:
        _check(f"hubert narrow n=12240 {tap} (clip 0)", narrow.tap(tap), gold, f"narrow_n12240_{tap}", want=torch.from_numpy(gold[f"narrow_n12240_{tap}"][:38]))


def test_batch_of_two_equals_golden_and_single_runs(gold, narrow, batch2):
    x, both, taps = batch2
    assert tuple(both.shape) == (2, 38, 64)
    _check("hubert narrow batch of 2 x 12240 output", both.reshape(76, 64), gold, "narrow_n12240_out")
    for tap in TAPS:
        _check(f"hubert narrow batch of 2 x 12240 {tap}", taps[tap], gold, f"narrow_n12240_{tap}")
    for b in range(2):      # bit-equal to the clips run singly: with the golden above, the positional conv's zero padding does not leak across clips
        one = narrow(x[b:b + 1]).last_hidden_state
        assert torch.equal(one[0], both[b]), b


@pytest.fixture(scope="module")
def pipe(narrow):
    from moditalker_amd import pipeline
    return pipeline.audio_to_hubert(_utterance(), narrow)


def test_pipeline_end_to_end(gold, narrow, pipe):
    """N = 645000: clips of 320080 | 320080 (one batch of 2) | 5000 samples -> 1000 + 1000 + 15 rows, normalised on the device first."""
    assert pipe.shape == (2015, 64) and pipe.dtype == np.float32
    _check("hubert pipeline N=645000 (2015 rows)", torch.from_numpy(pipe), gold, "narrow_pipe645000")


def test_narrow_full_clip_1000_frames(gold, narrow):
    """320080 samples: the first conv's 64015-row output, attention over 1000 keys (four key chunks, the last of 232)."""
    v = narrow.normalize(_utterance())
    out = narrow(v[None, :320080]).last_hidden_state
    assert tuple(out.shape) == (1, 1000, 64)
    _check("hubert narrow n=320080 output", out[0], gold, "narrow_pipe645000", want=torch.from_numpy(gold["narrow_pipe645000"][:1000]), bar_key="narrow_n320080")


def test_true_width_one_layer(gold):
    """hidden 1024, 16 heads of 64, ff 4096, conv dims 512, positional conv k = 128 in 16 groups (K = 8192 per group), K = 1536 convs."""
    m = _model(dict(num_hidden_layers=1), max_samples=16080)
    x = _wave("true_width.n16080", 16080)[None].to("cuda:0")
    out = m(x).last_hidden_state
    assert tuple(out.shape) == (1, 50, 1024)
    _check("hubert true width, 1 layer, n=16080 output", out[0], gold, "true_width_n16080_out")


def test_loader_spellings_give_the_same_bits(narrow):
    from moditalker_amd import HUBERT_LARGE_CONFIG, HubertModel
    x = _wave("narrow.n4000", 4000)[None].to("cuda:0")
    want = narrow(x).last_hidden_state
    ck = {}
    for k, v in narrow.state_dict().items():
        k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
        ck["hubert." + k] = v.detach().cpu().clone()
    ck["lm_head.weight"] = torch.zeros(32, 64)
    m = HubertModel(**dict(HUBERT_LARGE_CONFIG, **NARROW), max_samples=4000).eval()
    m.load_checkpoint_dict(ck)
    assert torch.equal(m.to("cuda:0")(x).last_hidden_state, want)


def test_argument_errors_come_before_any_launch(narrow):
    from moditalker_amd import MtvError
    with pytest.raises(ValueError):
        narrow(torch.zeros(1, 399, device="cuda:0"))
    with pytest.raises(NotImplementedError):
        narrow(torch.zeros(1, 4000, device="cuda:0"), attention_mask=torch.ones(1, 4000, device="cuda:0"))
    with pytest.raises(MtvError):
        narrow.tap("no_such_tap")
