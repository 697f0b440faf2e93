"""Host side of the device chunk loop (moditalker_amd/frames.py, csrc/frames.hip; no GPU): the library exports the three
calls, the two helpers that resolve the reference's Python semantics agree with the project's host functions, and the wrappers
refuse wrong arguments before anything reaches the library."""
import numpy as np
import pytest
import torch

from moditalker_amd import MtvError, _lib, frames as F
from moditalker_amd import pipeline as P


def test_library_exports_the_frame_calls():
    lib = _lib.load()
    for name in ("mtv_frames_prep", "mtv_frames_discs", "mtv_frames_finish"):
        assert any(s[0] == name for s in _lib.SYMBOLS), name
        assert getattr(lib, name) is not None


def test_entry_points_refuse_bad_arguments_before_launching():
    """Null pointers and bad sizes come back as MTV_ERR_INVALID with a text: nothing is launched (there is no device here)."""
    lib = _lib.load()
    p = 4096                                   # a non-null, aligned value that is never dereferenced: every call below fails first
    assert lib.mtv_frames_prep(None, None, p, 1, 1, 1, 8, 8, 8, 0, None) == -1
    assert lib.mtv_frames_prep(p, None, p, 1, 2, 3, 8, 8, 8, 0, None) == -1        # frames_in neither 1 nor frames
    assert lib.mtv_frames_prep(p, None, p, 1, 1, 1, 8, 8, 6, 0, None) == -1        # res not a multiple of 4
    assert lib.mtv_frames_prep(p, None, p + 4, 1, 1, 1, 8, 8, 8, 0, None) == -1    # out not 16-byte aligned
    assert lib.mtv_frames_prep(p, None, p, 1, 1, 1, 8, 8, 8, 2, None) == -1        # no such form of the division
    assert lib.mtv_frames_discs(p, None, p, 1, 1, 68, 3, 256, None) == -1
    assert lib.mtv_frames_discs(p, p, p, 1, 1, 2000, 3, 256, None) == -1
    assert lib.mtv_frames_discs(p, p, p, 1, 1, 68, 32, 256, None) == -1
    assert lib.mtv_frames_finish(p, None, None, None, 1, 1, 8, None) == -1
    assert lib.mtv_frames_finish(p, p, p, None, 1, 1, 8, None) == -1            # last_u8 without next_ref
    assert lib.mtv_frames_finish(p, p, None, None, 0, 1, 8, None) == -1
    assert b"mtv_frames_finish" in lib.mtv_last_error()


@pytest.mark.parametrize("y", [-300, -5, 0, 7.9, 39, 40, 90])          # h - 1, h and h + 50 at h = 40
def test_mask_start_is_crop_lower_half(y):
    h, w = 40, 12
    img = np.random.default_rng(3).integers(1, 256, size=(3, h, w)).astype(np.float64)      # no zero: every kept row shows
    lm = np.zeros((68, 2))
    lm[33, 1] = y
    want = P.crop_lower_half(img, lm)
    s = int(F.mask_start(y, h))
    assert 0 <= s <= h
    got = img.astype(np.uint8).copy()
    got[:, s:] = 0
    assert np.array_equal(got, want), (y, s)
    assert F.mask_start(np.full((2, 3), y), h).shape == (2, 3) and F.mask_start(np.full((2, 3), y), h).dtype == np.int32


def _centres_from_images(lm, WH):
    """The centres `landmarks_to_images` used, read off its picture: one point at a time: a whole disc reaches 3 pixels to every side of its centre."""
    out = np.zeros(lm.shape[:2] + (2,), dtype=np.int64)
    for t in range(lm.shape[0]):
        for p in range(lm.shape[1]):
            img = P.landmarks_to_images(lm[t:t + 1, p:p + 1], WH=WH)[0, :, :, 0]
            ys, xs = np.nonzero(img)
            assert len(ys) == 29, (t, p, len(ys))               # a whole radius-3 disc: the test keeps its points inside the canvas
            out[t, p] = (xs.min() + 3, ys.min() + 3)
    return out


@pytest.mark.parametrize("WH", [256, 634])
def test_disc_centres_image_sized(WH):
    rng = np.random.default_rng(WH)
    lm = rng.uniform(0.03 * WH, 0.97 * WH, size=(2, 68, 2))
    c = F.disc_centres(lm, WH)
    assert c.dtype == np.int32 and c.shape == (2, 68, 2)
    assert np.array_equal(c, _centres_from_images(lm, WH))
    # ... and the pictures themselves, all points at once
    img = np.zeros((2, 256, 256, 3), dtype=np.uint8)
    for t in range(2):
        for x, y in c[t]:
            P._draw_disc(img[t], int(x), int(y), P._disc_rows(3))
    assert np.array_equal(img, P.landmarks_to_images(lm, WH=WH))


def test_disc_centres_normalised_with_negative_values():
    rng = np.random.default_rng(5)
    lm = rng.uniform(-0.9, 0.9, size=(2, 68, 3))
    lm[0, 0] = (-0.5, -0.25, -3.0)
    for WH in (256, 634):
        c = F.disc_centres(lm, WH)
        assert np.array_equal(c, _centres_from_images(lm, WH))
    # beyond the canvas on the negative side: the astype(int) and int() truncations both go towards zero
    far = np.array([[[-1.004, -2.5, 0.0], [1.5, -1.0, 0.0]]])
    want = [[int(int(v * 634 / 2 + 634 / 2) / 634 * 256.0) for v in p[:2]] for p in far[0]]
    assert F.disc_centres(far, 634).tolist() == [want]
    with pytest.raises(ValueError):
        F.disc_centres(np.zeros((2, 68, 4)), 256)


def test_half_width_table_is_disc_rows():
    assert F.half_width_table(3).tolist() == [0, 2, 2, 3, 2, 2, 0]
    for r in (0, 1, 6, 31):
        tab = F.half_width_table(r)
        assert len(tab) == 2 * r + 1 and sorted(set(d for d, _ in P._disc_rows(r))) == list(range(-r, r + 1)) and tab.min() >= 0


def test_wrappers_refuse_wrong_arguments_without_calling_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", boom)
    u8 = torch.zeros(1, 2, 3, 8, 8, dtype=torch.uint8)
    bad_prep = [
        dict(src_u8=u8.float(), res=8),                                                      # dtype
        dict(src_u8=u8[0], res=8),                                                           # shape
        dict(src_u8=u8[:, :, :, :, ::2], res=8),                                             # contiguity
        dict(src_u8=u8, res=6),                                                              # res not a multiple of 4
        dict(src_u8=u8, res=8, frames=3),                                                    # 2 frames are neither 1 nor 3
        dict(src_u8=u8, res=8, division="fast"),                                             # no such form of the division
        dict(src_u8=u8, res=8, mask_start=torch.zeros(1, 2, dtype=torch.int64)),             # dtype
        dict(src_u8=u8, res=8, mask_start=torch.zeros(2, 2, dtype=torch.int32)),             # shape
        dict(src_u8=u8, res=8, mask_start=torch.zeros(1, 2, dtype=torch.int32, device="meta")),   # device
    ]
    for kw in bad_prep:
        with pytest.raises(ValueError):
            F.prepare_frames(**kw)
    c = torch.zeros(1, 2, 68, 2, dtype=torch.int32)
    for args in ((c.long(),), (c[0],), (c[..., :1],), (c, 32), (c, 3, 128)):
        with pytest.raises(ValueError):
            F.landmark_frames(*args)
    d = torch.zeros(4, 3, 8, 8)
    o8, l8, nr = torch.zeros(2, 2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 3, 2, 8, 8)
    bad_finish = [
        dict(decoded=d.double(), batch=2), dict(decoded=d[0], batch=2), dict(decoded=d, batch=3), dict(decoded=d[:, :, :, :6], batch=2),
        dict(decoded=d, batch=2, out=(o8.float(), None, None)),
        dict(decoded=d, batch=2, want_next_ref=True, out=(o8, l8, None)),
        dict(decoded=d, batch=2, want_next_ref=True, out=(o8, l8[:1], nr)),
        dict(decoded=d, batch=2, out=(o8.to("meta"), None, None)),
    ]
    for kw in bad_finish:
        with pytest.raises(ValueError):
            F.finish_frames(**kw)
    # right arguments, wrong place: there is no CPU fallback
    for call in (lambda: F.prepare_frames(u8, 8), lambda: F.landmark_frames(c), lambda: F.finish_frames(d, 2)):
        with pytest.raises(MtvError):
            call()
