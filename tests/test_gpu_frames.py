"""GPU checks of the device chunk loop (csrc/frames.hip through moditalker_amd.frames and the *_device methods of
pipeline.MToVSampler).  Comparators are the project's host functions (landmarks_to_images, crop_lower_half, to_model_range,
frames_to_uint8, last_frame_to_uint8, reference_from_uint8, run_identity) and torch.nn.functional.interpolate on the CPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import GOLDEN, SHALLOW_CFG, report
from moditalker_amd import BASE_AE_DDCONFIG, DDPM, DiffusionWrapper, UNetModel, ViTAutoencoder, filler, frames as F
from moditalker_amd import pipeline as P

pytestmark = pytest.mark.gpu

TOL = 1e-3      # BASELINE.json north_star: <= 1e-3 max-abs in fp32 (model range is [-1, 1])


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------ discs
def _disc_landmarks():
    """[B = 2, T = 3, 75, 2]: the 68-point grid of the chained-run test (test_gpu_autoencoder.py) moving with the frame, points on
    and beyond all four borders, two overlapping discs."""
    lm = np.zeros((2, 3, 75, 2), dtype=np.int64)
    for b in range(2):
        for f in range(3):
            lm[b, f, :68] = [[4 * (20 + 3 * (i % 8) + f) + 17 * b, 4 * (20 + 4 * (i // 8))] for i in range(68)]
            lm[b, f, 68:73] = [[0, 0], [255, 255], [-2, 1], [257, 128], [-1000, 10 ** 6]]
            lm[b, f, 73:] = [[40 + f, 30], [43 + f, 32 + b]]
    return lm


def _host_discs(lm, radius):
    img = np.zeros(lm.shape[:2] + (256, 256, 3), dtype=np.uint8)
    rows = P._disc_rows(radius)
    for b in range(lm.shape[0]):
        for f in range(lm.shape[1]):
            for x, y in lm[b, f]:
                P._draw_disc(img[b, f], int(x), int(y), rows)
    return img


def test_discs_bit_equal_landmarks_to_images():
    lm = _disc_landmarks()
    want = P.to_model_range(torch.from_numpy(np.stack([P.landmarks_to_images(lm[b], WH=256) for b in range(2)])).float().permute(0, 1, 4, 2, 3))
    got = F.landmark_frames(torch.from_numpy(F.disc_centres(lm, 256)).to(_dev())).cpu()
    assert got.shape == (2, 3, 3, 256, 256) and torch.equal(got, want)
    assert 0 < int((got == 1).sum()) < got.numel() // 10 and bool(((got == 1) | (got == -1)).all())


def test_discs_radius_6_follow_the_golden_rule():
    lm = _disc_landmarks()
    want = P.to_model_range(torch.from_numpy(_host_discs(lm, 6)).float().permute(0, 1, 4, 2, 3))
    got = F.landmark_frames(torch.from_numpy(F.disc_centres(lm, 256)).to(_dev()), radius=6).cpu()
    assert torch.equal(got, want)
    # one whole disc against the committed bitmap of OpenCV's Circle()
    title, bitmap = open(os.path.join(GOLDEN, "circle_r6.txt")).read().split("\n", 1)
    assert re.match(r"# radius 6, centre \(6,6\), 13x13", title)
    bm = torch.tensor([[1.0 if ch == "X" else -1.0 for ch in line] for line in bitmap.split()])
    one = F.landmark_frames(torch.tensor([[[[100, 200]]]], dtype=torch.int32, device=_dev()), radius=6).cpu()
    assert torch.equal(one[0, 1, 0, 194:207, 94:107], bm) and int((one[0, 0] == 1).sum()) == 113


# ------------------------------------------------------------------------------------------------------------------ prep
def test_prep_identity_size_is_to_model_range():
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 256, (2, 3, 3, 64, 64), generator=g, dtype=torch.uint8)
    src[0, 0, 0, 0, :256 // 4] = torch.arange(0, 256, 4, dtype=torch.uint8)
    src[0, 0, 1].view(-1)[:256] = torch.arange(256, dtype=torch.uint8)            # every byte value is there
    assert torch.equal(F.prepare_frames(src.to(dev), 64).cpu(), P.to_model_range(src.float()))
    # the other form: a multiplication by the fp32 reciprocal, composed on the host; it is what to_model_range gives on this device
    recip = (src.float() * (torch.tensor(1.0) / 127.5) - 1).permute(0, 2, 1, 3, 4).contiguous()
    got_r = F.prepare_frames(src.to(dev), 64, division="reciprocal").cpu()
    assert torch.equal(got_r, recip) and not torch.equal(recip, P.to_model_range(src.float()))
    print("prep: to_model_range on the device equals the reciprocal form:", torch.equal(P.to_model_range(src.float().to(dev)).cpu(), recip),
          "the IEEE form:", torch.equal(P.to_model_range(src.float().to(dev)).cpu(), P.to_model_range(src.float())))
    ms = torch.tensor([[0, 1, 31], [64, 31, 1]], dtype=torch.int32)
    lm = np.zeros((68, 2))
    masked = torch.zeros(2, 3, 3, 64, 64)
    for b in range(2):
        for t in range(3):
            lm[33, 1] = int(ms[b, t])
            masked[b, t] = torch.from_numpy(P.crop_lower_half(src[b, t].float().numpy(), lm)).float()
    got = F.prepare_frames(src.to(dev), 64, mask_start=ms.to(dev)).cpu()
    assert torch.equal(got, P.to_model_range(masked))
    assert bool((got[0, :, 0] == -1).all()) and torch.equal(got[1, :, 0], P.to_model_range(src.float())[1, :, 0])
    # Tin = 1 broadcasts one frame over T
    one = src[:, :1].contiguous()
    assert torch.equal(F.prepare_frames(one.to(dev), 64, frames=3).cpu(), P.to_model_range(one.expand(-1, 3, -1, -1, -1).float()))
    # a source that is not 4-byte aligned takes the general path: the same values (weights exactly 0 and 1)
    flat = torch.zeros(src.numel() + 1, dtype=torch.uint8, device=dev)
    flat[1:] = src.to(dev).view(-1)
    assert flat[1:].data_ptr() % 4 == 1
    assert torch.equal(F.prepare_frames(flat[1:].view(src.shape), 64, mask_start=ms.to(dev)).cpu(), got)


def _host_resize(src, ms, res):
    """mask -> centre crop -> F.interpolate(bilinear, align_corners=False) -> / 127.5 - 1, the order of dataloader_sample.py:210-232."""
    B, T, _, h, w = src.shape
    x = src.float().clone()
    if ms is not None:
        for b in range(B):
            for t in range(T):
                x[b, t, :, int(ms[b, t]):] = 0
    if h > w:
        half = (h - w) // 2
        x = x[:, :, :, half:half + w]
    else:
        half = (w - h) // 2
        x = x[:, :, :, :, half:half + h]
    y = TF.interpolate(x.reshape(B * T, 3, *x.shape[-2:]), size=res, mode="bilinear", align_corners=False)
    return P.to_model_range(y.reshape(B, T, 3, res, res))


@pytest.mark.parametrize("h,w", [(37, 50), (50, 37), (20, 20), (97, 97)])
def test_prep_resizing_vs_interpolate(h, w):
    dev, res = _dev(), 24
    src = torch.randint(0, 256, (2, 2, 3, h, w), generator=torch.Generator().manual_seed(h * 100 + w), dtype=torch.uint8)
    S, y_off = min(h, w), (h - w) // 2 if h > w else 0
    # a first masked row BETWEEN the two taps of output row 5: its upper tap is kept, its lower tap reads 0
    cut = y_off + int(S / res * 5.5 - 0.5) + 1
    ms = torch.tensor([[cut, h], [0, cut + 3]], dtype=torch.int32)
    for tag, m in (("plain", None), ("masked", ms)):
        got = F.prepare_frames(src.to(dev), res, mask_start=None if m is None else m.to(dev)).cpu()
        want = _host_resize(src, m, res)
        d = report(f"frame prep {h}x{w} -> {res} ({tag}) vs F.interpolate on the CPU", float((got - want).abs().max()), TOL)
        print(f"prep {h}x{w}->{res} {tag}: max-abs {d:.3e}")
        assert d <= TOL, d
    assert not torch.equal(_host_resize(src, ms, res)[0, :, 0, 5], _host_resize(src, None, res)[0, :, 0, 5])     # the cut does fall inside row 5
    # the reciprocal form of the same pixels: q = v / 127.5 <= 2 carries one rounding (2^-24 relative) as a division and two
    # (the reciprocal's and the product's) as a multiplication, so the forms are at most 3 * 2^-24 * 2 = 3.6e-7 apart before
    # the subtraction, which adds at most half an ulp of a result below 1 (3e-8) to each: 4.2e-7
    d = float((F.prepare_frames(src.to(dev), res, mask_start=ms.to(dev), division="reciprocal").cpu() - got).abs().max())
    print(f"prep {h}x{w}->{res}: reciprocal form vs IEEE form max-abs {d:.3e}")
    assert d <= 4.2e-7, d
    one = src[:, :1].contiguous()
    assert torch.equal(F.prepare_frames(one.to(dev), res, frames=2).cpu()[:, :, 1], F.prepare_frames(src.to(dev), res).cpu()[:, :, 0])


# ------------------------------------------------------------------------------------------------------------------ finish
def _decoded():
    dec = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(9)) * 0.8          # some beyond +-1 by themselves
    special = [-3.0, -1.0000001, -1.0, 1.0, 1.0000001, 2.5, 0.0] + [k / 127.5 - 1 for k in (0.5, 1.5, 2.5, 254.5)]
    # in fp32 only the last of those scales to k exactly; add values that do land on .5, below an even and below an odd count
    v = torch.arange(256, dtype=torch.float32).add(0.5) / 127.5 - 1
    on_half = [int(k) for k in torch.nonzero((1 + v) * 127.5 == torch.arange(256).add(0.5)).flatten()]
    even, odd = [k for k in on_half if k % 2 == 0 and k != 254], [k for k in on_half if k % 2]
    assert even and odd, on_half
    special += [float(v[even[0]]), float(v[odd[0]])]
    for n in range(4):                                                  # in every frame (the last frames are n = 1 and n = 3), every channel
        for c in range(3):
            dec[n, c, c, :len(special)] = torch.tensor(special)
    return dec


def _host_finish(dec, B):
    T = dec.shape[0] // B
    fake = (1 + dec.clamp(-1, 1).reshape(B, T, *dec.shape[1:]).permute(0, 1, 3, 4, 2)) * 127.5          # sample_chunk's arithmetic
    last = P.last_frame_to_uint8(fake)
    return P.frames_to_uint8(fake), last, P.reference_from_uint8(last, frames=T)


def test_finish_bit_equal_host_functions():
    dec = _decoded()
    u8, last, ref = _host_finish(dec, 2)
    halves = (1 + dec[1, 0, 0, 7:13].clamp(-1, 1)) * 127.5
    print("finish: the constructed .5 values scale to", halves.tolist())
    got_u8, got_last, got_ref = F.finish_frames(dec.to(_dev()), 2, want_next_ref=True)
    assert got_u8.dtype == torch.uint8 and tuple(got_u8.shape) == (2, 2, 16, 16, 3)
    assert np.array_equal(got_u8.cpu().numpy(), u8)
    assert np.array_equal(got_last.cpu().numpy(), last)
    assert torch.equal(got_ref.cpu(), ref)
    assert not np.array_equal(last, u8[:, -1])                          # rint and truncation do differ on this input


def test_finish_leaves_unrequested_outputs_alone():
    dev = _dev()
    dec = _decoded()
    u8, _, _ = _host_finish(dec, 2)
    n, guard = u8.size, 4096
    big = torch.full((n + 2 * guard,), 77, dtype=torch.uint8, device=dev)
    last = torch.full((2, 16, 16, 3), 77, dtype=torch.uint8, device=dev)
    ref = torch.full((2, 3, 2, 16, 16), 7.0, device=dev)
    out = big[guard:guard + n].view(u8.shape)
    got = F.finish_frames(dec.to(dev), 2, want_next_ref=False, out=(out, last, ref))
    assert got[0] is out and got[1] is None and got[2] is None
    assert np.array_equal(out.cpu().numpy(), u8)
    assert bool((big[:guard] == 77).all()) and bool((big[guard + n:] == 77).all())
    assert bool((last == 77).all()) and bool((ref == 7.0).all())
    without = F.finish_frames(dec.to(dev), 2)
    assert without[1] is None and without[2] is None and torch.equal(without[0], out)


# ------------------------------------------------------------------------------------------------------------------ the whole loop
def _png_bytes(folder):
    return {os.path.relpath(os.path.join(d, f), folder): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(folder) for f in fs}


class _HostDivisionSampler(P.MToVSampler):
    """The existing loop with ONE difference: to_model_range runs on the host, before the upload.  (MToVSampler.conditioning
    applies it to device tensors, where torch divides by a scalar by multiplying with its reciprocal.)"""

    def conditioning(self, x_ref, x, x_l, masked_x):
        dev = next(self.ae.parameters()).device
        x_ref, x, x_l, masked_x = (P.to_model_range(t.cpu()).to(dev) for t in (x_ref, x, x_l, masked_x))
        image_cond_ = self.ae.extract(x_ref)
        return dict(z_=self.ae.extract(x), image_cond_=image_cond_, image_cond=image_cond_[:, :, 0:self.n_xy],
                    c=torch.cat([self.ae_ldmk.extract(x_l), self.ae.extract(masked_x)], dim=1))


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    """Two chained chunks (use_last_as_reference, out_dir set) at full size, computed once: full-size autoencoder with filler
    weights, SHALLOW_CFG UNet at R = 32, S = 2, 256 x 256 sources so that the prep is exact.  The existing path twice, the
    existing path with the division on the host, the device path in both forms of the division."""
    dev = _dev()
    tmp = tmp_path_factory.mktemp("loop")
    R, T, S, res = 32, 16, 2, 256
    cfg = dict(SHALLOW_CFG, image_size=R)
    net = DiffusionWrapper(UNetModel(**cfg, frames=T, max_batch=1)).eval()
    filler.fill_module_(net, seed=51, skip_prefixes=("output_bg_",))
    net = net.to(dev)
    ae = ViTAutoencoder(4, dict(BASE_AE_DDCONFIG, resolution=res), max_batch=1).eval()
    filler.fill_autoencoder_(ae, seed=52)
    ae = ae.to(dev)
    L = R * R + 2 * T * R
    dm = DDPM(net, channels=4, image_size=R, sampling_timesteps=S, w=0.0).to(dev)
    sampler, hostdiv = P.MToVSampler(dm, ae, latent_res=R), _HostDivisionSampler(dm, ae, latent_res=R)
    host_chunks, dev_chunks, noises = [], [], []
    for it in range(2):
        vid = ((filler.uniform_pm1(f"loop.vid{it}", (1, T, 3, res, res), 51) + 1) * 127.5).round().clamp(0, 255).to(torch.uint8)
        ref = vid[:, :1].contiguous()
        lm = np.stack([np.stack([np.array([60 + 14 * (i % 9) + 2 * f + it, 70.5 + 13 * (i // 9) + f]) for i in range(68)]) for f in range(T)])
        x_l = torch.from_numpy(P.landmarks_to_images(lm, WH=res)).float().permute(0, 3, 1, 2)[None].contiguous()
        masked = torch.from_numpy(np.stack([P.crop_lower_half(vid[0, f].float().numpy(), lm[f]) for f in range(T)])).float()[None]
        host_chunks.append((ref.expand(-1, T, -1, -1, -1).float().contiguous(), vid.float(), x_l, masked))
        dev_chunks.append((ref, vid, lm[None], lm[None, :, 33, 1]))
        noises.append([n.to(dev) for n in filler.noise_list(S, (1, 4, L), seed=51 + it, tag="loop.noise")])
    up = [tuple(t.to(dev) for t in c) for c in host_chunks]
    r = dict(T=T, res=res)
    r["cond_host"] = sampler.conditioning(*up[0])
    r["cond_hostdiv"] = hostdiv.conditioning(*up[0])
    r["cond_device"] = sampler.conditioning_device(*dev_chunks[0])
    r["cond_device_ieee"] = sampler.conditioning_device(*dev_chunks[0], division="ieee")
    for tag, s in (("host_a", sampler), ("host_b", sampler), ("hostdiv", hostdiv)):
        out = s.run_identity(up, use_last_as_reference=True, out_dir=str(tmp / tag), noise_per_chunk=noises)
        r[tag] = (np.stack(out), _png_bytes(tmp / tag))
    out = sampler.run_identity_device(dev_chunks, use_last_as_reference=True, out_dir=str(tmp / "device"), noise_per_chunk=noises)
    r["device"] = (np.stack(out), _png_bytes(tmp / "device"))
    out = sampler.run_identity_device(dev_chunks, use_last_as_reference=True, out_dir=str(tmp / "device_ieee"), noise_per_chunk=noises,
                                      division="ieee")
    r["device_ieee"] = (np.stack(out), _png_bytes(tmp / "device_ieee"))
    return r


def test_whole_loop_equals_the_loop_with_host_division(loop):
    """The device loop with division="ieee" against the existing loop composed with to_model_range on the host (the arithmetic
    k_frames_prep follows by default): conditioning torch.equal, frames and every written PNG byte for byte."""
    for k, v in loop["cond_hostdiv"].items():
        assert torch.equal(v, loop["cond_device_ieee"][k]), k
    got, got_png = loop["device_ieee"]
    want, want_png = loop["hostdiv"]
    assert got.shape == want.shape and sorted(got_png) == sorted(want_png)
    assert np.array_equal(got, want)
    assert got_png == want_png


def test_whole_loop_equals_run_identity(loop):
    """conditioning_device torch.equal to conditioning fed the host-built tensors, run_identity_device's frames and PNG bytes
    equal to run_identity's: the existing path runs twice first; if those two runs are bit-equal, equality with the device path
    is required, else the device path must lie within their spread.

    (MToVSampler.conditioning applies to_model_range to tensors that are already on the device, where torch divides by a scalar
    by multiplying with its reciprocal: 111 of the 256 byte values come out one ulp away from the host's division.
    conditioning_device therefore asks k_frames_prep for the form to_model_range takes on the device.  With the host's form
    instead, measured on an MI355X: conditioning differs by at most 1.5e-6, 8106 to 14536 of the 6291456 frame values by one
    count, and all 34 PNG files differ.)"""
    cond_h, cond_d = loop["cond_host"], loop["cond_device"]
    cond_gap = {k: float((cond_h[k] - cond_d[k]).abs().max()) for k in cond_h}
    print("whole loop: conditioning_device vs conditioning, max-abs per entry:", cond_gap)
    (a, a_png), (b, b_png), (got, got_png) = loop["host_a"], loop["host_b"], loop["device"]
    T, res = loop["T"], loop["res"]
    assert got.shape == a.shape == (2, 1, T, res, res, 3) and got.dtype == np.uint8
    assert sorted(got_png) == sorted(a_png) and len(got_png) == 2 * T + 2
    gap = np.abs(got.astype(np.int32) - a.astype(np.int32))
    print(f"whole loop: host run a vs b differ in {int((a != b).sum())} of {a.size} values; device vs host a: {int((gap != 0).sum())} "
          f"values differ, max {int(gap.max())} counts; PNG files that differ: {sum(got_png[k] != a_png[k] for k in got_png)}")
    for k in cond_h:
        assert torch.equal(cond_h[k], cond_d[k]), (k, cond_gap[k])
    if np.array_equal(a, b) and a_png == b_png:
        assert np.array_equal(got, a), (int((gap != 0).sum()), int(gap.max()))
        assert got_png == a_png
    else:
        print("WHOLE LOOP: THE EXISTING PATH IS NOT BIT-REPRODUCIBLE HERE; the device path is held to the spread of its two runs")
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        assert bool(((got >= lo) & (got <= hi)).all())
