"""k_conv_win on its packed 3x3 weights (csrc/deep.hip, ConvArgs::Wwin: the conv matrix rewritten per (column tile, K slice, wave) in the order the K loop
consumes it) against the same kernel on the legacy [krow][ldw] matrix: same MFMA order, same sums -- the outputs must be bit-equal.  MTV_WIN_PACKED=0 is
read when a context is created (a module's first forward), so one process holds a context of each form."""
import os
import re

import pytest
import torch

from moditalker_amd import _lib, filler
from test_gpu_parity import BASE_CFG, RAGGED_CFG, _build, _dev, _ragged_case

pytestmark = pytest.mark.gpu

TILES = [(1, 2), (1, 4), (2, 2), (2, 4)]
TAG = re.compile(r"^conv3:(?P<name>\S+?)\[(?P<L>\d+)x(?P<N>\d+) k(?P<K>\d+) t(?P<mt>\d+),(?P<nt>\d+),80,(?P<ks>\d+)x?\]$")


def _restore(lib, old):
    lib.mtv_debug_force_win_ks(0, 0, 1)
    if old is None:
        os.environ.pop("MTV_WIN_PACKED", None)
    else:
        os.environ["MTV_WIN_PACKED"] = old


def _win_launches(net, B):
    names = [p["name"] for p in net.diffusion_model.profile_forward(B, 1, _dev())]
    return [m.groupdict() for m in map(TAG.match, names) if m]


def _run_pair(cfg, seed, frames, B, mt, nt, ks, inputs, t):
    """eps of the legacy plan and of the packed plan on the same inputs (plans are built by the first forward, under the switch of their net), and the
    k_conv_win launches of the packed plan."""
    lib = _lib.load()
    _lib.check(lib.mtv_debug_force_win_ks(mt, nt, ks), "mtv_debug_force_win_ks")
    old = os.environ.get("MTV_WIN_PACKED")
    dev = _dev()
    x, cond, ic = (v.to(dev) for v in inputs)
    out, nets, wins = [], [], None
    try:
        for packed in ("0", "1"):
            os.environ["MTV_WIN_PACKED"] = packed
            net = _build(cfg, seed, frames=frames, max_batch=B)
            out.append(net(x, cond, ic, t.to(dev)).clone())
            wins = _win_launches(net, B)
            nets.append(net)
    finally:
        _restore(lib, old)
    return out, nets, wins


def _on_tile(wins, mt, nt, ks=None):
    return [w for w in wins if (int(w["mt"]), int(w["nt"])) == (mt, nt) and (ks is None or int(w["ks"]) == ks)]


@pytest.mark.parametrize("ks", [1, 2, 4])
@pytest.mark.parametrize("mt,nt", TILES)
def test_packed_weights_bit_equal_legacy_ragged_two_clips(mt, nt, ks):
    """The ragged two-clip geometry (24, 8): row tiles that straddle planes, windows clipped by plane borders, partial last tiles.  Every eligible 3x3 conv
    is forced onto k_conv_win<mt, nt> with ks K slices where conv_win_can_run admits them (the others run unsliced, also packed).  The plan must hold a conv
    with a fused skip conv on two concatenated sources (K = 9 Cmain + Cskip, the decoder's ResBlocks) and one on an upsampled source (the first conv of a
    block's last ResBlock, whose output level is finer than the block's others)."""
    x, cond, ic, t, _ = _ragged_case(2)
    (legacy, packed), _, wins = _run_pair(RAGGED_CFG, 21, 8, 2, mt, nt, ks, (x, cond, ic), t)
    assert torch.equal(legacy, packed), float((legacy - packed).abs().max())
    assert len(_on_tile(wins, mt, nt)) >= 20, wins
    assert _on_tile(wins, mt, nt, ks), f"no conv took {ks} K slices"
    fused = [w for w in _on_tile(wins, mt, nt) if w["name"].startswith("out") and int(w["K"]) > 9 * int(w["N"]) and w["name"].endswith("conv2")]
    assert fused, "no conv with a fused skip conv on concatenated sources ran on the tile"
    by_block = {}
    for w in _on_tile(wins, mt, nt):
        if w["name"].startswith("out"):
            by_block.setdefault(w["name"].split(".")[0], []).append(w)
    ups = [w for ws in by_block.values() for w in ws if w["name"].endswith("conv1") and int(w["L"]) > min(int(v["L"]) for v in ws)]
    assert ups, "no conv on an upsampled source ran on the tile"


@pytest.mark.parametrize("mt,nt,ks", [(1, 2, 1), (1, 4, 2), (2, 2, 4), (2, 4, 1)])
def test_packed_weights_bit_equal_legacy_at_the_128_token_level(mt, nt, ks):
    """Base geometry (32, 16), one clip: besides the 2048- and 512-token convs, the 3x3 convs of the 128-token level that the deep-level kernels leave to
    the large-level ones run on the forced tile."""
    inputs = filler.synthetic_inputs(1, 32, 16, seed=7, tag="base")
    (legacy, packed), _, wins = _run_pair(BASE_CFG, 7, 16, 1, mt, nt, ks, inputs, torch.tensor([500]))
    assert torch.equal(legacy, packed), float((legacy - packed).abs().max())
    assert [w for w in _on_tile(wins, mt, nt) if int(w["L"]) == 128], "no 128-token conv ran on the tile"
    assert {int(w["L"]) for w in _on_tile(wins, mt, nt)} >= {2048, 512, 128}


def test_packed_copy_is_remade_when_weights_are_reloaded():
    """load_state_dict with other weights: the packed plan's output follows (equal to the legacy plan's again, different from before)."""
    x, cond, ic, t, _ = _ragged_case(2)
    dev = _dev()
    (legacy, packed), (net0, net1), wins = _run_pair(RAGGED_CFG, 21, 8, 2, 1, 4, 2, (x, cond, ic), t)
    assert torch.equal(legacy, packed) and _on_tile(wins, 1, 4)
    sd = {k: (v * 0.5 if k.endswith("in_layers.2.weight") or k.endswith("out_layers.3.weight") else v) for k, v in net0.state_dict().items()}
    for net in (net0, net1):
        net.load_state_dict(sd)
    a, b = (net(x.to(dev), cond.to(dev), ic.to(dev), t.to(dev)) for net in (net0, net1))
    assert torch.equal(a, b), float((a - b).abs().max())
    assert not torch.equal(a, legacy), "the reloaded weights changed nothing: the test shows nothing"
