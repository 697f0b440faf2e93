"""The long-video UNet (MToV/configs/latent-diffusion/base_longvid.yaml: model_channels 256, 8 heads, cond_model -- head dims
32 / 64 / 128 / 128) on the host: the checkpoint layout of LONGVID_UNET_CONFIG against the reference's manifest, and the oracle's pin on
the slim 128-wide-head net (tests/golden/slim128*.npz, written by tests/golden/make_golden_longvid.py).  CPU only."""
import glob
import os

import numpy as np
import torch

from conftest import GOLDEN
from moditalker_amd import LONGVID_UNET_CONFIG, DiffusionWrapper, UNetModel, filler
from oracle import ref_unet

# the smallest net with the long-video model's head dims: 32 / 64 / 128 / 128 at C = 64 / 128 / 256 / 256, two heads
SLIM128_CFG = dict(image_size=32, in_channels=4, out_channels=4, model_channels=64, attention_resolutions=[4, 2, 1],
                   num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=2, use_scale_shift_norm=True,
                   resblock_updown=True, cond_model=False)
SLIM128_SEED = 21


def slim128_golden():
    """slim128.npz and its tap parts (slim128_taps*.npz: no committed file above 1 MiB), merged."""
    g = {}
    for p in [os.path.join(GOLDEN, "slim128.npz")] + sorted(glob.glob(os.path.join(GOLDEN, "slim128_taps*.npz"))):
        g.update(np.load(p))
    return g


def test_longvid_state_dict_layout_matches_the_reference_manifest():
    g = np.load(os.path.join(GOLDEN, "longvid.npz"))
    with torch.device("meta"):
        net = DiffusionWrapper(UNetModel(**LONGVID_UNET_CONFIG))
    sd = net.state_dict()
    want = {str(k): tuple(int(x) for x in str(s).split(",")) if str(s) else () for k, s in zip(g["keys"], g["shapes"])}
    assert len(want) == 805 and "diffusion_model.zeros" in want        # cond_model=True: one buffer more than the base layout
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert {k: tuple(v.shape) for k, v in sd.items()} == want


def test_oracle_reproduces_slim128_eps():
    g = slim128_golden()
    assert sum(k.startswith("tap_") for k in g) == 25
    with torch.device("meta"):
        m = UNetModel(**SLIM128_CFG)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = {k: filler.fill_tensor("diffusion_model." + k, shapes[k], SLIM128_SEED) for k in ref_unet.used_keys(SLIM128_CFG)}
    x, cond, ic = filler.synthetic_inputs(1, 32, 16, seed=SLIM128_SEED, tag="slim128")
    for tv in (999, 500, 0):
        eps = ref_unet.unet_forward(sd, SLIM128_CFG, x, cond, ic, torch.tensor([tv]), 32, 16)
        assert float((eps - torch.from_numpy(g[f"eps_t{tv}"])).abs().max()) <= 2e-5, tv
