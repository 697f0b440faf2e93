"""A library context takes its options (csrc/options.h: MTV_* environment, mtv_debug_* overrides) once, when it is created, and keeps them: plans it
builds later -- another batch size, after a setter's reset -- run under them, and two live contexts of one process can differ.  The first test runs
the shallow three-level UNet at (32, 16), the smallest configuration whose default plan has deep-level launches (its 128-token level); the bit-equality
tests run the base UNet at one clip, whose every conv shape is in the committed tile table: two default contexts then hold the same plan (shapes the
table does not list are timed per context, and two contexts may settle on different split-K tiles)."""
import ctypes
import functools

import torch

from conftest import BASE_CFG, SHALLOW_CFG
from moditalker_amd import _lib, filler
from test_gpu_parity import FWD_TOL, _build, _dev, _golden, _maxabs

import pytest

pytestmark = pytest.mark.gpu

SEED = 12


@functools.lru_cache(maxsize=None)
def _case():
    """Two clips and the CPU oracle's eps for them, once per session (clips are independent: clip 0 alone is the B = 1 reference)."""
    from oracle import ref_unet
    net = _build(SHALLOW_CFG, SEED)
    x, cond, ic = filler.synthetic_inputs(2, 32, 16, seed=SEED, tag="options")
    t = torch.tensor([640, 7])
    ref = ref_unet.unet_forward({k: v.cpu() for k, v in net.state_dict().items()}, SHALLOW_CFG, x, cond, ic, t, 32, 16)
    return x, cond, ic, t, ref


def _forward(net, B):
    x, cond, ic, t, _ = _case()
    dev = _dev()
    return net(x[:B].to(dev), cond[:B].to(dev), ic[:B].to(dev), t[:B].to(dev)).clone()


def _base_forward(net):
    dev = _dev()
    x, cond, ic = filler.synthetic_inputs(1, 32, 16, seed=7, tag="base")
    return net(x.to(dev), cond.to(dev), ic.to(dev), torch.tensor([999], device=dev)).clone()


def _names(net, B):
    return [p["name"] for p in net.diffusion_model.profile_forward(B, 1, _dev())]


def _deep(names):
    return [n for n in names if (n.startswith("conv") and " d" in n.split("[")[-1]) or "+proj" in n or " blk " in n or n.startswith("fin")]


def _on_win_1x2(names):
    return [n for n in names if "t1,2,80,1" in n]


def _dump(net):
    buf = ctypes.create_string_buffer(4096)
    _lib.check(_lib.load().mtv_debug_options_dump(net.diffusion_model._ctx, buf, len(buf)), "mtv_debug_options_dump")
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


def test_a_context_keeps_the_options_it_was_created_with():
    """mtv_debug_deep(0), a net, its first forward (B = 1), the reset, then the net's B = 2 plan -- built after the reset: still no deep kernel, both
    outputs at the oracle.  A net built after the reset does run them."""
    lib = _lib.load()
    ref = _case()[4]
    _lib.check(lib.mtv_debug_deep(0), "mtv_debug_deep")
    try:
        net = _build(SHALLOW_CFG, SEED, max_batch=2)
        e1 = _forward(net, 1)
    finally:
        lib.mtv_debug_deep(-1)
    e2 = _forward(net, 2)
    assert not _deep(_names(net, 2)), "a plan built after the reset took the process's new setting"
    assert not _deep(_names(net, 1))
    assert _maxabs(e1, ref[:1]) <= FWD_TOL and _maxabs(e2, ref) <= FWD_TOL, (_maxabs(e1, ref[:1]), _maxabs(e2, ref))
    assert _dump(net)["MTV_DEEP"] == "0"
    fresh = _build(SHALLOW_CFG, SEED, max_batch=2)
    assert _maxabs(_forward(fresh, 2), ref) <= FWD_TOL
    assert _deep(_names(fresh, 2)) and _dump(fresh)["MTV_DEEP"] == "1"


@pytest.fixture(scope="module")
def pair():
    """Net A created under a forced k_conv_win tile, net B after the reset, and their first outputs (a context is created by the first forward); the two
    tests below only read them, and both contexts are freed when the module is done."""
    lib = _lib.load()
    _lib.check(lib.mtv_debug_force_win_ks(1, 2, 1), "mtv_debug_force_win_ks")
    try:
        a = _build(BASE_CFG, 7, max_batch=1)
        a1 = _base_forward(a)
    finally:
        lib.mtv_debug_force_win(0, 0)
    b = _build(BASE_CFG, 7, max_batch=1)
    yield a, b, a1, _base_forward(b)
    for net in (a, b):
        net.diffusion_model._release()


def test_two_live_contexts_with_two_option_sets(pair):
    """Forwards interleaved A, B, A, B on the same inputs: A's plan carries the forced tile, B's is the default plan and computes the default
    net's bits."""
    default = _build(BASE_CFG, 7, max_batch=1)
    want = _base_forward(default)
    a, b, a1, b1 = pair
    a2 = _base_forward(a)
    b2 = _base_forward(b)
    names_a, names_b = _names(a, 1), _names(b, 1)
    assert len(_on_win_1x2(names_a)) >= 10 and all("t1,2,80," in n for n in names_a if ",80," in n), names_a
    assert names_b == _names(default, 1) and names_b != names_a
    assert torch.equal(b1, want) and torch.equal(b2, want)
    assert torch.equal(a1, a2)
    assert _maxabs(a1, _golden("base")["eps_t999"]) <= FWD_TOL and _maxabs(b1, _golden("base")["eps_t999"]) <= FWD_TOL


def test_options_dump_of_a_context_shows_its_snapshot(pair):
    """After the setter's reset, mtv_debug_options_dump(ctx) of net A still shows the forced tile and of net B shows it off."""
    a, b, _, _ = pair
    assert _dump(a)["MTV_FORCE_WIN"] == "1,2,1" and _dump(b)["MTV_FORCE_WIN"] == "0"
    assert {k: v for k, v in _dump(a).items() if k != "MTV_FORCE_WIN"} == {k: v for k, v in _dump(b).items() if k != "MTV_FORCE_WIN"}
