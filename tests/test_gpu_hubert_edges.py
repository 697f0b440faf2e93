"""The HuBERT stage on the GPU (csrc/hubert.hip behind moditalker_amd.HubertModel) against the fp64 oracle (oracle/ref_hubert.py,
pinned to transformers' outputs by tests/test_hubert_oracle_host.py) at the shapes the goldens cannot reach: k_hub_gemm's K / N
/ M tails as a Linear, as a conv whose 16-wide K chunk spans several taps, and as the positional conv (4-channel groups, an odd
tap count, padding longer than the clip, three clips); k_tok_attn at head dims 4 / 20 / 64, on both sides of the 256-key chunk
and with a peaked softmax; the waveform normalisation across its grid-stride wrap, in place and on a signal whose mean dwarfs
its spread; a layer_norm_eps that differs from the conv layers' fixed 1e-5.

Bar of every forward comparison: 10 x max|oracle(fp32) - oracle(fp64)| of that same call and tensor, computed here on the CPU
-- the rule of tests/golden/PIN_REPORT_hubert.txt, measured on the reference and never on the code under test.  The
normalisation computes in fp64 and rounds once, so its bar is derived: 2 fp32 ulps of the fp64 reference, elementwise."""
import ctypes as C

import pytest
import torch

from conftest import report

pytestmark = pytest.mark.gpu

SEED = 83
TAPS = ("extract_features", "after_pos_conv", "layer_0")
NARROW = dict(hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128, conv_dim=(32,) * 7,
              num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
# n = 20 T + 10.  conv1: K = 3 x 36 = 108 (a 16-wide chunk spans taps; K tail), N = 20; conv2: K = 40, N = 44; projection: LayerNorm
# over K = 44; positional conv: 15 taps (odd), Cg = 20; encoder: K = 100, N = 300 / 132 / 100; 5 heads of 20; eps 1e-3 != 1e-5
ODD = dict(hidden_size=100, num_hidden_layers=1, num_attention_heads=5, intermediate_size=132, conv_dim=(36, 20, 44), conv_kernel=(10, 3, 2),
           conv_stride=(5, 2, 2), num_conv_pos_embeddings=15, num_conv_pos_embedding_groups=5, layer_norm_eps=1e-3)
# n = 3 T + 4.  Positional conv: Cg = 4 (every quad its own tap, 4 valid columns of a 64-wide tile), pad 20; 16 heads of 4; a conv of kernel 1
CG4 = dict(hidden_size=64, num_hidden_layers=1, num_attention_heads=16, intermediate_size=68, conv_dim=(32, 32), conv_kernel=(7, 1),
           conv_stride=(3, 1), num_conv_pos_embeddings=40, num_conv_pos_embedding_groups=16)
# n = 3 T - 1.  One conv layer (projection straight after conv0), stride > kernel; 2 heads of 64; positional conv K = 128 x 64
D64 = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, conv_dim=(64,), conv_kernel=(2,),
           conv_stride=(3,), num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=2)
CONV8 = dict(NARROW, conv_dim=(32,) * 8, conv_kernel=(10, 3, 3, 3, 3, 2, 2, 1), conv_stride=(5, 2, 2, 2, 2, 2, 2, 1))
# q_proj / k_proj weights times PEAK_GAIN: the logits grow by its square.  The smallest whole gain at which the oracle's median
# (over head and query) largest softmax weight exceeds 0.5 in every case below: 0.83 at T = 513, 0.78 at T = 514 and 0.73 at T = 257,
# where gain 3 gives 0.53 and 0.49 at the first two and filler weights alone 0.008.
PEAK_GAIN = 4.0


class _Case:
    """One configuration: the HIP model, its weights for the oracle, and one context sized for the largest case."""

    def __init__(self, over, max_samples, max_batch=1, edit=None):
        from moditalker_amd import HUBERT_LARGE_CONFIG, HubertModel, filler
        self.cfg = dict(HUBERT_LARGE_CONFIG, **over)
        m = HubertModel(**self.cfg, max_samples=max_samples, max_batch=max_batch).eval()
        filler.fill_module_(m, seed=SEED)
        if edit:
            edit(m)
        self.sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        self.model = m.to("cuda:0")
        self.model.debug_taps = True

    def wave(self, tag, B, n):
        from moditalker_amd import filler
        return filler.uniform_pm1(f"hubert.edges.{tag}", (B, n), SEED)

    def oracle(self, x):
        """{name: (fp64 value, bar)} for the output and the three taps; taps64 also keeps the softmax weights."""
        from oracle import ref_hubert
        t64, t32 = {}, {}
        t64["out"] = ref_hubert.hubert_forward(self.sd, self.cfg, x, torch.float64, taps=t64).flatten(0, 1)
        t32["out"] = ref_hubert.hubert_forward(self.sd, self.cfg, x, torch.float32, taps=t32).flatten(0, 1)
        return {k: (t64[k], 10.0 * float((t32[k].double() - t64[k]).abs().max())) for k in ("out",) + TAPS}, t64

    def run(self, x):
        out = self.model(x.to("cuda:0")).last_hidden_state
        return out, dict({t: self.model.tap(t) for t in TAPS}, out=out.flatten(0, 1).cpu())

    def check(self, name, x, frames):
        want, t64 = self.oracle(x)
        out, got = self.run(x)
        assert tuple(out.shape) == (x.shape[0], frames, self.cfg["hidden_size"]), tuple(out.shape)
        fails = []
        for k, (ref, bar) in want.items():
            assert tuple(got[k].shape) == tuple(ref.shape), (name, k, tuple(got[k].shape), tuple(ref.shape))
            assert bar > 0.0, (name, k)
            d = report(f"hubert edges {name} {k}", float((got[k].double() - ref).abs().max()), bar)
            print(f"{name} {k}: max-abs {d:.3e}  bar {bar:.3e}")
            if not d <= bar:
                fails.append((k, d, bar))
        assert not fails, (name, fails)
        return out, got, t64


@pytest.fixture(scope="module")
def odd():
    return _Case(ODD, max_samples=20 * 513 + 10, max_batch=3)


@pytest.fixture(scope="module")
def cg4():
    return _Case(CG4, max_samples=3 * 300 + 4)


@pytest.fixture(scope="module")
def d64():
    return _Case(D64, max_samples=3 * 257 - 1)


@pytest.mark.parametrize("T", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513])
def test_odd_single_clip(odd, T):
    """Tile edges of the 16-query attention tile and the 64-row GEMM tile, and key counts around the 256-key chunk (at 257 the
    second chunk holds one key)."""
    odd.check(f"ODD T={T}", odd.wave(f"odd.T{T}", 1, 20 * T + 10), T)


@pytest.mark.parametrize("T", [17, 65])
def test_odd_batch_of_three(odd, T):
    """64-row tiles straddle clips (3 x 17 rows in one tile; 65 rows per clip), the conv buffers ping-pong with three clips, and
    the positional conv's padding must not read the neighbouring clip: against the oracle, and bit-equal to the clips run singly."""
    x = odd.wave(f"odd.B3.T{T}", 3, 20 * T + 10)
    both, got, _ = odd.check(f"ODD B=3 T={T}", x, T)
    for b in range(3):
        one, taps = odd.run(x[b:b + 1])
        assert torch.equal(one[0], both[b]), b
        for t in TAPS:
            assert torch.equal(taps[t], got[t][b * T:(b + 1) * T]), (b, t)


@pytest.mark.parametrize("T", [1, 17, 300])
def test_cg4(cg4, T):
    """T = 1 and 17: the positional conv's padding (20) is longer than the clip on both sides.  T = 300: a last key chunk of 44."""
    cg4.check(f"CG4 T={T}", cg4.wave(f"cg4.T{T}", 1, 3 * T + 4), T)


@pytest.mark.parametrize("T", [16, 257])
def test_d64(d64, T):
    d64.check(f"D64 T={T}", d64.wave(f"d64.T{T}", 1, 3 * T - 1), T)


def test_eight_conv_layers():
    case = _Case(CONV8, max_samples=4000)
    case.check("8 conv layers T=12", case.wave("conv8", 1, 4000), 12)


@pytest.fixture(scope="module")
def peaked():
    def sharpen(m):
        with torch.no_grad():
            m.encoder.layers[0].attention.q_proj.weight.mul_(PEAK_GAIN)
            m.encoder.layers[0].attention.k_proj.weight.mul_(PEAK_GAIN)

    return _Case(NARROW, max_samples=164560, edit=sharpen)


@pytest.mark.parametrize("n,T,roll", [(164240, 513, 0), (164560, 514, 0), (82320, 257, 23360)])
def test_peaked_softmax_across_key_chunks(peaked, n, T, roll):
    """Filler weights give near-uniform attention, which a wrong rescale of the running sum barely moves.  Here most queries put
    more than half their weight on one key, and the running max changes between the chunks of 256 | 256 | 1 (or 2) keys.
    At T = 257 no query of any unrolled clip tried has its strongest key in the one-key second chunk, so a rescale that is wrong
    only when that key raises the maximum would pass: the clip is rolled by 73 frames, which puts the key most queries prefer
    (frame 183) last.  The oracle says whether that worked."""
    case = peaked
    x = torch.roll(case.wave(f"peaked.{T}", 1, n), roll, dims=1)
    _, _, t64 = case.check(f"PEAKED gain {PEAK_GAIN:g} T={T}", x, T)
    if roll:
        late = int((t64["attention_0"].argmax(dim=-1) == T - 1).sum())
        print(f"PEAKED T={T}: {late} (head, query) pairs have their strongest key alone in the last chunk")
        assert late >= 16, late
    peak = float(t64["attention_0"].amax(dim=-1).median())
    print(f"PEAKED: median over (head, query) of the largest softmax weight {peak:.3f}")
    assert peak > 0.5, peak


# ---- waveform normalisation
def _norm_input(n, kind):
    from moditalker_amd import filler
    u = filler.uniform_pm1(f"hubert.edges.norm.{n}", (n,), SEED)
    return 0.5 * u + 0.25 if kind == "offset" else 1000.0 + 0.01 * u


@pytest.mark.parametrize("n,kind", [(1, "offset"), (2, "offset"), (255, "offset"), (256, "offset"), (257, "offset"), (65535, "offset"),
                                    (65536, "offset"), (65537, "offset"), (200001, "offset"), (200001, "large_mean")])
def test_normalize(cg4, n, kind):
    """One workgroup's worth, the partial passes' grid-stride wrap at 65536 samples, and a mean 1e5 times the spread (what the two
    fp64 passes are for).  The kernel rounds an fp64 result once: 2 fp32 ulps of the fp64 reference, elementwise."""
    from moditalker_amd import _lib
    from oracle import ref_hubert
    m = cg4.model
    x = _norm_input(n, kind)
    ref = ref_hubert.normalize(x, torch.float64)
    xd = x.to("cuda:0")
    got = m.normalize(xd)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
    assert torch.equal(xd.cpu(), x)                                         # out of place: the input is left alone
    ulp = 2.0 ** -23 * ref.abs().clamp_min(2.0 ** -126)
    d = report(f"hubert edges normalise n={n} {kind} (fp32 ulps of the fp64 reference)", float(((got.cpu().double() - ref).abs() / ulp).max()), 2.0)
    print(f"normalise n={n} {kind}: {d:.3f} ulps  bar 2")
    assert d <= 2.0, (n, kind, d)
    if n == 1:
        assert float(got[0]) == 0.0
    assert torch.equal(m.normalize(xd), got)                                # a repeated call
    inplace = xd.clone()                                                    # the documented in-place form of the C ABI
    with torch.cuda.device(0):
        _lib.check(_lib.load().mtv_hubert_normalize(m._ctx, inplace.data_ptr(), n, inplace.data_ptr(),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mtv_hubert_normalize")
    assert torch.equal(inplace, got)


# ---- shapes the kernels cannot take are refused at context creation
@pytest.mark.parametrize("what,over", [
    ("hidden 66 (no multiple of 4)", dict(ODD, hidden_size=66, num_attention_heads=2, intermediate_size=132, num_conv_pos_embedding_groups=2)),
    ("head dim 68", dict(ODD, hidden_size=136, num_attention_heads=2, num_conv_pos_embedding_groups=2)),
    ("hidden / groups = 6", dict(ODD, hidden_size=96, num_attention_heads=2, num_conv_pos_embedding_groups=16)),
    ("conv_dim 30", dict(ODD, conv_dim=(36, 30, 44))),
])
def test_unsupported_shapes_raise_before_any_launch(what, over):
    from moditalker_amd import HUBERT_LARGE_CONFIG, HubertModel, MtvError, filler
    m = None
    with pytest.raises((MtvError, ValueError)):
        m = HubertModel(**dict(HUBERT_LARGE_CONFIG, **over), max_samples=350).eval()
        filler.fill_module_(m, seed=SEED)
        m = m.to("cuda:0")
        m(torch.zeros(1, 350, device="cuda:0"))
    assert m is None or m._ctx is None, what
