"""k_conv_win's packed 3x3 weight operand (csrc/mtv_internal.h WinPack, csrc/deep.hip k_win_repack; no GPU): the packed-index -> (row, column)
map that the repack kernel writes by and the kernel's loads invert.  mtv_selftest_win_pack walks that one shared function on the host."""
import pytest

from moditalker_amd import _lib

TILES = [(1, 2), (1, 4), (2, 2), (2, 4)]          # every instantiated k_conv_win<MT, NT>


def _sliceable(ks, cmain, cskip):
    """conv_win_eligible's rule for K slices: whole 16-channel chunks of the tapped and of the skip channels per slice."""
    return (cmain // 16) % ks == 0 and (cskip // 16) % ks == 0


@pytest.mark.parametrize("mt,nt", TILES)
@pytest.mark.parametrize("ks", [1, 2, 4])
def test_packed_map_reaches_every_element_once_and_pads_with_zero(mt, nt, ks):
    """For every tile and slice count: the map reaches every element of the legacy matrix [9 Cmain + Cskip][N] exactly once, every other packed
    position is padding (defined as zero) and is exactly the chunks at or past a wave's last, and the kernel's own offset arithmetic lands on the
    element its operand register expects.  The shapes include chunk counts that are no multiple of 8 (Cmain 48: 27 chunks; 32 + 32 skip: 20) and
    skip parts whose slice has fewer chunks than the main part (Cmain 128, Cskip 32)."""
    lib = _lib.load()
    ran = 0
    for cmain in (32, 48, 128):
        for cskip in (0, 32, 96):
            for n in (32, 64):
                if n % (16 * nt):
                    continue                       # (no whole column tile: conv_win_eligible refuses the conv)
                if not _sliceable(ks, cmain, cskip):
                    assert lib.mtv_selftest_win_pack(mt, nt, ks, cmain, cskip, n) < 0       # refused, not packed wrongly
                    continue
                assert lib.mtv_selftest_win_pack(mt, nt, ks, cmain, cskip, n) == 0, (mt, nt, ks, cmain, cskip, n)
                ran += 1
    assert ran >= {1: 9, 2: 6, 4: 1}[ks]           # (sliceable shapes of the lists above, at one N at least)


def test_packed_map_refuses_what_the_kernel_cannot_run():
    lib = _lib.load()
    assert lib.mtv_selftest_win_pack(4, 4, 1, 32, 0, 64) < 0          # no such tile
    assert lib.mtv_selftest_win_pack(1, 2, 3, 48, 0, 32) < 0          # three K slices
    assert lib.mtv_selftest_win_pack(1, 4, 1, 40, 0, 64) < 0          # not whole 16-channel chunks
    assert lib.mtv_selftest_win_pack(1, 4, 1, 32, 0, 32) < 0          # half a column tile
    assert lib.mtv_selftest_win_pack(1, 2, 1, 32, 0, 0) < 0
