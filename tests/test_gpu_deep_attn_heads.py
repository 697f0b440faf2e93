"""k_deep_attn with ONE head per workgroup and 128-column proj slices read lane-linear from the packed proj_out matrix
(csrc/deep.hip; DeepAttnArgs::form / Wpk, MTV_DEEP_ATTN_HPW, mtv_debug_deep_attn_form): the kernel on its own against the CPU
restatement of tools/ubench/deep_bench, and through the base UNet against the reference golden in both forms."""
import os
import re
import subprocess

import pytest
import torch

from test_gpu_parity import (FWD_TOL, GOLDEN, SAMPLE_TOL, SHALLOW_CFG, _base_eps_and_sample, _build, _dev)
from moditalker_amd import filler

pytestmark = pytest.mark.gpu


def test_deep_bench_attn_covers_packed_weights_and_one_head_per_workgroup():
    """deep_bench attn: besides the nine LDS-staged cases, every shape of the list below with the packed matrix in the rule's head-group
    form and with one head per workgroup forced -- same double-precision CPU restatement, same bar (1e-4 x max(1, |ref|)) as the
    staged cases.  [128 x 512] d = 64 1-D / per plane with 1 and 8 residual slabs (the product shape: one proj tile per wave), ragged
    planes 36 | 18 | 18 at d = 32 (a query tile across a plane border, 5 key tiles), 15 tokens (less than a key tile), two clips at
    d = 16 (a K slice of one 16-channel chunk), and C = 64, where no 128-column slice exists and the forced form must fall back."""
    exe = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "ubench", "deep_bench")
    assert os.path.exists(exe), "tools/ubench/deep_bench not built (python -c 'import __graft_entry__ as g; g.build()')"
    out = subprocess.run([exe, "attn"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ATTN CHECK OK" in out.stdout, out.stdout[-3000:] + out.stderr[-500:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("attn+proj")]
    assert all(ln.rstrip().endswith("PASS") for ln in lines), out.stdout[-3000:]
    heads = [ln for ln in lines if " packed/heads " in ln]
    packed = [ln for ln in lines if " packed " in ln]
    assert len(heads) == 8 and len(packed) == 8 and len(lines) == 25, (len(heads), len(packed), len(lines))
    # forced: one head per workgroup wherever C is a multiple of 128; the product shape gets 8 slabs from 8 x 8 x 4 workgroups
    assert sum("HPW1 NC128" in ln for ln in heads) == 7, heads
    assert sum(bool(re.search(r"L128 C512 d64 .* HPW1 NC128 -> 8 slabs, 256 WGs", ln)) for ln in heads) == 4, heads
    fallback = [ln for ln in heads if " C64 " in ln]
    assert len(fallback) == 1 and "NC16" in fallback[0], fallback
    assert not any("NC128" in ln for ln in packed), packed


def _attn_tags(names):
    return [n for n in names if n.startswith("attn") and "+proj" in n and "[L128 d64" in n]


@pytest.mark.parametrize("form,tag", [(-1, "h1,c128]"), (2, "h2,c64]")])
def test_base_unet_in_both_attention_forms_vs_reference_golden(form, tag):
    """The default plan runs the ten [128 x 512] attention blocks with one head per workgroup (op names `+proj h1,c128`);
    mtv_debug_deep_attn_form(2) -- what MTV_DEEP_ATTN_HPW=2 selects -- keeps round 6's head groups (`h2,c64`), on packed weights too.
    Either way: eps at t = 999 / 500 / 0 and the 4-step sample against the reference golden at the project's bars, 10 fused and 8
    one-launch blocks, and five repeated forwards of the shallow two-clip net bit-equal (the arrival order of the head groups -- 8 of
    them in the new form -- must not matter)."""
    from moditalker_amd import _lib
    lib = _lib.load()
    _lib.check(lib.mtv_debug_deep_attn_form(form), "mtv_debug_deep_attn_form")
    try:
        names = []
        e, s = _base_eps_and_sample(lib, names, what=f"deep attention form {form}")
        assert e <= FWD_TOL and s <= SAMPLE_TOL, (form, e, s)
        fused = [n for n in names if n.startswith("attn") and "+proj" in n]
        blocks = [n for n in names if n.startswith("attn") and " blk " in n]
        assert len(fused) == 10 and len(blocks) == 8, (len(fused), len(blocks))
        big = _attn_tags(names)
        assert len(big) == 10 and all(n.endswith(tag) for n in big), big
        net = _build(SHALLOW_CFG, 12)
        dev = _dev()
        x, cond, ic = filler.synthetic_inputs(2, 32, 16, seed=12, tag="shallow")
        t = torch.tensor([321, 9], device=dev)
        a = net(x.to(dev), cond.to(dev), ic.to(dev), t)
        for _ in range(5):
            assert torch.equal(net(x.to(dev), cond.to(dev), ic.to(dev), t), a)
    finally:
        lib.mtv_debug_deep_attn_form(-1)


def test_one_head_per_workgroup_forced_everywhere_vs_reference_golden():
    """mtv_debug_deep_attn_form(1) with the three-launch block everywhere (MTV_DEEP_OPT_NO_BLOCK): all 18 attention blocks of the deep
    levels run the new form (32 and 128 tokens, 1-D and per plane), tagged completion over 8 head groups included."""
    from moditalker_amd import _lib
    lib = _lib.load()
    _lib.check(lib.mtv_debug_deep_attn_form(1), "mtv_debug_deep_attn_form")
    _lib.check(lib.mtv_debug_deep_options(16), "mtv_debug_deep_options")
    try:
        names = []
        e, s = _base_eps_and_sample(lib, names, what="deep attention form 1, no block")
        assert e <= FWD_TOL and s <= SAMPLE_TOL, (e, s)
        fused = [n for n in names if n.startswith("attn") and "+proj" in n]
        assert len(fused) == 18 and all(n.endswith("h1,c128]") for n in fused), fused
    finally:
        lib.mtv_debug_deep_options(-1)
        lib.mtv_debug_deep_attn_form(-1)
