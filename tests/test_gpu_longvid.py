"""128-wide heads on the deep levels (the long-video UNet's 128- and 32-token levels): k_deep_attn<128> through the slim net against the
reference's golden (tests/golden/slim128*.npz), the op names of its plan, the k_attention + proj_out fallback, bit-equal repeats, and the
kernel itself against deep_bench's double-precision CPU restatement.  Only the slim net (52 M parameters) is built here; the shipped
config at full width is tools/longvid_check.py."""
import os
import subprocess

import pytest
import torch

from conftest import GOLDEN, report
from test_gpu_parity import FWD_TOL, SAMPLE_TOL, _build, _dev, _maxabs
from test_longvid_host import SLIM128_CFG, SLIM128_SEED, slim128_golden
from moditalker_amd import DDPM, filler

pytestmark = pytest.mark.gpu

TAP_TOL = FWD_TOL      # the bar test_gpu_parity.py holds the taps of the narrow / shallow nets to
_G = {}


def _g():
    if not _G:
        _G.update(slim128_golden())
    return _G


def _parity(what):
    """eps at t = 999 / 500 / 0, the 25 taps of a two-clip forward and the 4-step sample of the slim net against the reference golden."""
    g, dev = _g(), _dev()
    net = _build(SLIM128_CFG, SLIM128_SEED)
    x, cond, ic = filler.synthetic_inputs(1, 32, 16, seed=SLIM128_SEED, tag="slim128")
    for tv in (999, 500, 0):
        eps = net(x.to(dev), cond.to(dev), ic.to(dev), torch.tensor([tv], device=dev))
        e = report(f"{what}: slim128 eps t={tv} vs reference golden", _maxabs(eps, g[f"eps_t{tv}"]), FWD_TOL)
        assert e <= FWD_TOL, (what, tv, e)
    x2, cond2, ic2 = filler.synthetic_inputs(2, 32, 16, seed=SLIM128_SEED, tag="slim128.b2")
    eps2 = net(x2.to(dev), cond2.to(dev), ic2.to(dev), torch.from_numpy(g["t_b2"]).to(dev))
    worst = {k: _maxabs(net.diffusion_model.debug_tap(k[4:], 2)[..., ::7], g[k]) for k in g if k.startswith("tap_")}
    assert len(worst) == 25
    report(f"{what}: slim128 worst of {len(worst)} taps vs reference golden", max(worst.values()), TAP_TOL)
    bad = {k: v for k, v in worst.items() if not v <= TAP_TOL}
    assert not bad, f"taps off: {bad} (all: {worst})"
    assert report(f"{what}: slim128 B=2 eps vs reference golden", _maxabs(eps2, g["eps_b2"]), FWD_TOL) <= FWD_TOL
    S = 4
    dm = DDPM(net, channels=4, image_size=32, sampling_timesteps=S, w=0.0).to(dev)
    noise = [z.to(dev) for z in filler.noise_list(S, (1, 4, 2048), seed=SLIM128_SEED, tag=f"slim128.S{S}")]
    z = dm.sample(batch_size=1, cond=cond.to(dev), image_cond=ic.to(dev), noise=noise)
    assert report(f"{what}: slim128 {S}-step sample vs reference golden", _maxabs(z, g[f"sample_S{S}"]), SAMPLE_TOL) <= SAMPLE_TOL
    return net


def _d128(names):
    return [n for n in names if n.startswith("attn") and " d128 " in n and ("[L128 " in n or "[L32 " in n)]


def test_slim128_vs_reference_golden():
    _parity("default plan")


def test_d128_attention_blocks_of_the_deep_levels_are_fused():
    """Every d = 128 attention op of the 128- and 32-token levels is the fused attention + proj_out launch: 17 of the 18 blocks of those levels
    (the 1-D block behind the down-sample into the 128-token level still has 128 channels: d = 64)."""
    net = _build(SLIM128_CFG, SLIM128_SEED)
    names = [p["name"] for p in net.diffusion_model.profile_forward(1, 1, _dev(), step=True)]
    ops = _d128(names)
    assert len(ops) == 17, ops
    assert all("+proj h1,c" in n for n in ops), ops


def test_slim128_fallback_form_vs_reference_golden():
    """MTV_DEEP_OPT_NO_FUSED_ATTN: finalize + qkv conv + k_attention<128> + proj_out conv -- what a plan keeps where the fused form is not taken."""
    from moditalker_amd import _lib
    lib = _lib.load()
    _lib.check(lib.mtv_debug_deep_options(8), "mtv_debug_deep_options")
    try:
        net = _parity("no fused attention")
        ops = _d128([p["name"] for p in net.diffusion_model.profile_forward(1, 1, _dev(), step=True)])
        assert len(ops) == 17 and not any("+proj" in n or " blk " in n for n in ops), ops
    finally:
        lib.mtv_debug_deep_options(-1)


def test_slim128_repeated_two_clip_forwards_are_bit_equal():
    dev = _dev()
    net = _build(SLIM128_CFG, SLIM128_SEED)
    x, cond, ic = (v.to(dev) for v in filler.synthetic_inputs(2, 32, 16, seed=SLIM128_SEED, tag="slim128.b2"))
    t = torch.tensor([977, 13], device=dev)
    a = net(x, cond, ic, t).clone()
    for _ in range(5):
        assert torch.equal(net(x, cond, ic, t), a)


def test_deep_bench_attn128():
    exe = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "ubench", "deep_bench")
    if not os.path.exists(exe):
        pytest.skip("tools/ubench/deep_bench not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run([exe, "attn128"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ATTN128 CHECK OK" in out.stdout, out.stdout[-3000:] + out.stderr[-500:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("attn+proj")]
    assert len(lines) == 30 and all(ln.rstrip().endswith("PASS") for ln in lines), out.stdout[-3000:]
    assert all(" d128 " in ln for ln in lines)
    assert sum("L128 C1024 d128" in ln and "HPW1 NC128 -> 8 slabs, 512 WGs" in ln for ln in lines) == 1, lines
