"""Host-side checks of the HuBERT stage (moditalker_amd/hubert.py, pipeline.audio_to_hubert): state_dict parity with
transformers' large model (tests/golden/hubert_large_keys.txt, written by tests/golden/make_golden_hubert.py), the
checkpoint-dict loader, the frame arithmetic, the windowing of get_hubert_from_speech
(data/data_utils/preprocess/process_audio.py:9-55) with a stub forward, the C ABI's exports.  No GPU."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN

NARROW = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, conv_dim=(32,) * 7,
              num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)


def _narrow_cfg():
    from moditalker_amd import HUBERT_LARGE_CONFIG
    return dict(HUBERT_LARGE_CONFIG, **NARROW)


def test_large_state_dict_matches_transformers_manifest():
    from moditalker_amd import HUBERT_LARGE_CONFIG, HubertModel
    with open(os.path.join(GOLDEN, "hubert_large_keys.txt")) as f:
        want = [ln.split() for ln in f.read().splitlines() if ln]
    with torch.device("meta"):
        sd = HubertModel(**HUBERT_LARGE_CONFIG).state_dict()
    assert len(want) == 422
    assert list(sd.keys()) == [k for k, _ in want]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [s for _, s in want]


def test_large_config_values():
    from moditalker_amd import HUBERT_LARGE_CONFIG as c
    assert (c["hidden_size"], c["num_hidden_layers"], c["num_attention_heads"], c["intermediate_size"]) == (1024, 24, 16, 4096)
    assert c["feat_extract_norm"] == "layer" and c["conv_bias"] and c["do_stable_layer_norm"] and c["feat_proj_layer_norm"]
    assert (c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"], c["layer_norm_eps"]) == (128, 16, 1e-5)
    assert c["conv_kernel"] == (10, 3, 3, 3, 3, 2, 2) and c["conv_stride"] == (5, 2, 2, 2, 2, 2, 2)


@pytest.mark.parametrize("spelling", ["weight_g", "parametrizations"])
@pytest.mark.parametrize("prefix", ["", "hubert."])
def test_checkpoint_dict_loader(spelling, prefix):
    from moditalker_amd import HubertModel, filler
    cfg = _narrow_cfg()
    src = HubertModel(**cfg)
    filler.fill_module_(src, seed=3)
    ck = {}
    for k, v in src.state_dict().items():
        if spelling == "weight_g":
            k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
        ck[prefix + k] = v.clone()
    ck[prefix + "masked_spec_embed"] = torch.full((64,), 7.0)      # ignored
    ck["lm_head.weight"] = torch.zeros(32, 64)                     # ignored
    ck["lm_head.bias"] = torch.zeros(32)
    dst = HubertModel(**cfg)
    res = dst.load_checkpoint_dict(ck)
    assert not res.missing_keys and not res.unexpected_keys
    a, b = src.state_dict(), dst.state_dict()
    for k in a:
        if k != "masked_spec_embed":
            assert torch.equal(a[k], b[k]), k
    assert float(dst.masked_spec_embed.detach().abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        dst.load_checkpoint_dict({k: v for k, v in ck.items() if "k_proj" not in k})      # a missing tensor is not ignored


def _frames(n):
    for k, s in zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)):
        if n < k:
            return 0
        n = (n - k) // s + 1
    return n


@pytest.mark.parametrize("n,want", [(399, 0), (400, 1), (719, 1), (720, 2), (320080, 1000)])
def test_num_frames(n, want):
    from moditalker_amd import _lib, hubert
    assert _frames(n) == want
    assert _lib.load().mtv_hubert_num_frames(n) == want
    assert hubert.num_frames(n) == want


def test_not_built_configurations_raise():
    from moditalker_amd import HubertModel, MtvError
    cfg = _narrow_cfg()
    with pytest.raises(NotImplementedError):
        HubertModel(**dict(cfg, do_stable_layer_norm=False))
    with pytest.raises(NotImplementedError):
        HubertModel(**dict(cfg, feat_extract_norm="group"))
    m = HubertModel(**cfg).eval()
    x = torch.zeros(1, 4000)
    with pytest.raises(NotImplementedError):
        m(x, attention_mask=torch.ones(1, 4000, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        m(x, mask_time_indices=torch.zeros(1, 12, dtype=torch.bool))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 399))
    with pytest.raises(MtvError):      # no CPU fallback
        m(x)


class _Stub:
    """forward returns, per frame, (clip's first sample, frame index, samples in the clip); it records every call."""

    def __init__(self, extra_rows=0):
        self.calls, self.extra = [], extra_rows

    def forward(self, input_values):
        B, n = input_values.shape
        self.calls.append((int(B), int(n)))
        T = _frames(int(n)) + self.extra
        out = torch.zeros(B, T, 3)
        out[:, :, 0] = input_values[:, :1]
        out[:, :, 1] = torch.arange(T, dtype=torch.float32)[None]
        out[:, :, 2] = float(n)
        return SimpleNamespace(last_hidden_state=out)


def _ramp(N):
    return np.arange(N, dtype=np.float64) / N - 0.25


def _norm(x):
    x = x.astype(np.float32)
    return (x - x.mean()) / np.sqrt(x.var() + 1e-7)


@pytest.mark.parametrize("N,clips", [
    (5000, [(0, 5000)]),                                              # no full clip
    (645000, [(0, 320080), (320000, 640080), (640000, 645000)]),      # two clips plus remainder: 2015 rows
    (640399, [(0, 320080), (320000, 640080)]),                        # remainder of 399 samples skipped
    (320050, [(0, 320050)]),                                          # the one full clip is cut short by the end of the file
])
def test_audio_to_hubert_windowing(N, clips, tmp_path):
    from moditalker_amd import pipeline
    stub = _Stub()
    x = _ramp(N)
    out = pipeline.audio_to_hubert(x, stub, save_path=str(tmp_path / "h" / "a.npy"))
    expected_T = (N - 80) // 320
    assert out.shape == (expected_T, 3) and out.dtype == np.float32
    assert sorted(n for B, n in stub.calls for _ in range(B)) == sorted(b - a for a, b in clips)
    v = _norm(x)
    rows = []
    for a, b in clips:
        rows += [(v[a], t, b - a) for t in range(_frames(b - a))]
    # whatever N: the clips' rows differ from expected_T by at most one, made up by a zero row or a trim
    assert abs(len(rows) - expected_T) <= 1
    rows = (rows + [(0.0, 0.0, 0.0)])[:expected_T]
    np.testing.assert_array_equal(out, np.array(rows, dtype=np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "h" / "a.npy"), out)
    if N == 645000:
        assert out.shape[0] == 2015
    if N == 320050:
        # 320050 samples give 999 frames (64009, 32004, 16001, 8000, 3999, 1999, 999 through the convs) = expected_T: nothing to trim
        assert len(rows) == 999 and _frames(320050) == 999


def test_audio_to_hubert_pads_trims_and_refuses():
    from moditalker_amd import pipeline
    x = _ramp(5000)
    out = pipeline.audio_to_hubert(x, _Stub(extra_rows=1))      # 16 rows for 15 expected: trimmed
    assert out.shape == (15, 3) and out[-1, 1] == 14.0
    out = pipeline.audio_to_hubert(x, _Stub(extra_rows=-1))     # 14 rows: one zero row appended
    assert out.shape == (15, 3) and out[-2, 1] == 13.0 and not out[-1].any()
    with pytest.raises(ValueError):
        pipeline.audio_to_hubert(x, _Stub(extra_rows=2))
    with pytest.raises(ValueError):
        pipeline.audio_to_hubert(np.zeros(399), _Stub())


def test_audio_to_hubert_batches_equal_clips_and_keeps_channel_0():
    from moditalker_amd import pipeline
    stub = _Stub()
    stub.max_batch = 2
    x = _ramp(645000)
    stereo = np.stack([x, -x], axis=1)
    out = pipeline.audio_to_hubert(stereo, stub)
    assert stub.calls == [(2, 320080), (1, 5000)]
    one = _Stub()
    np.testing.assert_array_equal(out, pipeline.audio_to_hubert(x, one))
    assert one.calls == [(1, 320080), (1, 320080), (1, 5000)]


def test_library_exports_hubert_symbols():
    from moditalker_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mtv_hubert_create", "mtv_hubert_destroy", "mtv_hubert_normalize", "mtv_hubert_forward", "mtv_hubert_num_frames",
                 "mtv_hubert_frames", "mtv_hubert_num_launches", "mtv_hubert_profile", "mtv_hubert_debug_keep", "mtv_hubert_debug_tap"):
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in _lib.SYMBOLS), name
