"""tests/arena.py on a CPU tensor: alignment and exact lengths, bands intact after legitimate writes, a one-byte write just
behind a buffer, just in front of one and at the far edge of a band reported with the buffer's name and the offset, a changed
input reported. The same one-byte case on the device, through a plain torch fill, is in tests/test_gpu_buffer_contracts.py."""
import numpy as np
import pytest
import torch

import arena as ar
from arena import Arena


def _three(a):
    x = a.put(np.arange(37, dtype=np.uint8), name="x")
    y = a.take(1001, fill=0xA5, name="y")
    z = a.take(17, align=4, fill=0x00, name="z")
    return x, y, z


def test_alignment_and_exact_lengths():
    a = Arena(torch, capacity=1 << 18)
    last_end = a.base - ar.BAND                                        # (nothing lies in front of the first buffer's band)
    for nbytes, align in [(1, 256), (15, 256), (17, 4), (4099, 8), (0, 256), (33, 1), (256, 256), (5, 4096)]:
        v = a.take(nbytes, align, fill=0x00)
        assert v.dtype == torch.uint8 and v.numel() == nbytes
        start = a.base + a.bufs[-1][1]
        assert a.bufs[-1][2] == nbytes and start % align == 0 and (nbytes == 0 or v.data_ptr() == start)
        assert start - last_end >= 2 * ar.BAND                        # a band of its own on either side of every buffer
        assert start + nbytes + ar.BAND <= a.base + a.buf.numel()
        last_end = start + nbytes
    assert a.take(3, 4, fill=0xA5).tolist() == [0xA5] * 3 and a.take(2, fill=None).tolist() == [ar.CANARY] * 2
    pre = np.arange(12, dtype=np.int32)
    assert np.array_equal(a.read(a.take(48, fill=pre), np.int32, (3, 4)), pre.reshape(3, 4))
    a.check()
    with pytest.raises(AssertionError, match="too small"):
        a.take(1 << 18)
    with pytest.raises(AssertionError, match="differ from the canary"):
        a.take(4, fill=ar.CANARY)
    assert ar.CANARY not in ar.POISONS and ar.CANARY != 0xAB
    assert ar.ptr(None) is None and ar.ptr(a.take(0)) is None and ar.ptr(v) == v.data_ptr()


def test_bands_are_intact_after_legitimate_writes():
    a = Arena(torch, capacity=1 << 16)
    x, y, z = _three(a)
    y.fill_(ar.CANARY)                                                # any byte is a legitimate content, the canary's included
    y[0], y[-1], z[0], z[-1] = 1, 2, 3, 4
    z[:16].view(torch.int32)[:] = -1
    a.check()
    a.unchanged()
    assert a.read(x).tolist() == list(range(37))


@pytest.mark.parametrize("who,offset,side,where", [
    ("y", 1001, "behind", r"\+0 "), ("y", -1, "in front", "-1 "), ("y", 1001 + ar.BAND - 1, "behind", r"\+%d " % (ar.BAND - 1)),
    ("y", -ar.BAND, "in front", "-%d " % ar.BAND), ("z", 17, "behind", r"\+0 "), ("x", -1, "in front", "-1 ")])
def test_a_one_byte_write_into_a_band_is_reported(who, offset, side, where):
    a = Arena(torch, capacity=1 << 16)
    views = dict(zip("xyz", _three(a)))
    start = views[who].data_ptr() - a.base
    a.check()
    a.buf[start + offset] = 0x00
    phrase = {"in front": "the band in front of it", "behind": "the band behind it"}[side]
    with pytest.raises(AssertionError, match=r"^%s \(\d+ bytes\): %s was written, first at %s\(1 bytes" % (who, phrase, where)):
        a.check()
    a.unchanged()                                                     # the inputs themselves hold
    a.buf[start + offset] = ar.CANARY
    a.check()


def test_a_changed_input_is_reported():
    a = Arena(torch, capacity=1 << 16)
    x, y, z = _three(a)
    w = a.put(np.array([[1, 2], [3, 4]], np.int64), name="w")
    a.unchanged()
    w.view(torch.int64)[3] = 5
    with pytest.raises(AssertionError, match=r"^w \(32 bytes\): an input was written, first at offset 24 \(1 bytes"):
        a.unchanged()
    w.view(torch.int64)[3] = 4
    x[36] = 0
    with pytest.raises(AssertionError, match=r"^x \(37 bytes\): an input was written, first at offset 36 "):
        a.unchanged()
    a.check()                                                         # a changed input is no damaged band
