"""One allocation, cut into exact-size buffers with a canary band in front of and behind every one of them: the harness of the
buffer-contract tests (tests/test_gpu_buffer_contracts.py). Test helper only; it calls nothing of the library, and the same code
runs on a CPU tensor (tests/test_arena.py).

Everything a stray store could hit lies inside the arena's own allocation: a kernel that writes past a buffer damages a canary
byte, which ``check`` reports, and faults nothing.

    arena = Arena(torch, "cuda")
    src = arena.put(array)                       # an input: uploaded, remembered
    out = arena.take(nbytes, fill=0xA5)          # an output / workspace of EXACTLY nbytes, poisoned
    lib.gcs_...(src.data_ptr(), ..., out.data_ptr(), stream)
    arena.check(); arena.unchanged()
    got = arena.read(out, np.int32, (b, h, w))
"""
import numpy as np

BAND = 4096      # a 256-thread workgroup's worth of 16-byte stores, the widest store any kernel issues: no tail store jumps it
CANARY = 0xC7    # differs from every poison byte used for contents (POISONS, 0xAB of the older files)
POISONS = (0x00, 0xA5)


class Arena:
    def __init__(self, torch, device="cpu", capacity=8 << 20, pinned=False):
        self.torch = torch
        kw = dict(dtype=torch.uint8)
        if pinned:
            self.buf = torch.empty(int(capacity), pin_memory=True, **kw)
            self.buf.fill_(CANARY)
        else:
            self.buf = torch.full((int(capacity),), CANARY, device=device, **kw)
        self.base = self.buf.data_ptr()
        self.cursor = 0
        self.bufs = []         # (name, start, nbytes)
        self.inputs = []       # (name, start, bytes as a NumPy array)

    # ---- making buffers
    def take(self, nbytes, align=256, fill=0x00, name=None):
        """A uint8 view of exactly ``nbytes`` whose first byte is ``align``-aligned, a band of BAND canary bytes on either side.
        ``fill``: the poison byte, a NumPy array of ``nbytes`` bytes (contents the header prescribes), or None (left as canary)."""
        nbytes, align = int(nbytes), int(align)
        assert nbytes >= 0 and align >= 1 and align & (align - 1) == 0
        start = -(-(self.base + self.cursor + BAND) // align) * align - self.base
        assert start + nbytes + BAND <= self.buf.numel(), "the arena is too small: %d bytes asked for %s" % (nbytes, name)
        view = self.buf[start:start + nbytes]
        if isinstance(fill, np.ndarray):
            raw = np.ascontiguousarray(fill).reshape(-1).view(np.uint8)
            assert raw.size == nbytes
            if nbytes:
                view.copy_(self.torch.from_numpy(raw.copy()))
        elif fill is not None:
            assert 0 <= int(fill) < 256 and int(fill) != CANARY, "a poison byte must differ from the canary"
            view.fill_(int(fill))
        self.bufs.append((name or "buffer %d" % len(self.bufs), start, nbytes))
        self.cursor = start + nbytes + BAND          # bands are not shared: damage is reported for the buffer it lies next to
        return view

    def put(self, array, align=256, name=None):
        """Upload an input (any NumPy array, taken as bytes) into a buffer of its exact size and remember it for ``unchanged``."""
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8).copy()
        name = name or "input %d" % len(self.inputs)
        view = self.take(raw.size, align, raw, name)
        self.inputs.append((name, self.bufs[-1][1], raw))
        return view

    # ---- reading and checking
    def read(self, view, dtype=np.uint8, shape=(-1,)):
        """The bytes of a view (or of any tensor) as a NumPy array of ``dtype`` and ``shape`` on the host."""
        return view.cpu().numpy().copy().view(dtype).reshape(shape)

    def check(self):
        """Every band of every buffer is intact; else AssertionError naming the buffer, the side and the first damaged offset
        (``behind +i``: byte i past the buffer's end; ``in front -i``: byte i before its first byte)."""
        for name, start, nbytes in self.bufs:
            end = start + nbytes
            bad = np.flatnonzero(self.buf[end:end + BAND].cpu().numpy() != CANARY)       # (only the bands travel)
            assert bad.size == 0, "%s (%d bytes): the band behind it was written, first at +%d (%d bytes damaged)" % (
                name, nbytes, int(bad[0]), bad.size)
            bad = np.flatnonzero(self.buf[start - BAND:start].cpu().numpy() != CANARY)
            assert bad.size == 0, "%s (%d bytes): the band in front of it was written, first at -%d (%d bytes damaged)" % (
                name, nbytes, BAND - int(bad[-1]), bad.size)

    def unchanged(self):
        """Every input ``put`` still holds its bytes; else AssertionError naming it and the first changed offset."""
        for name, start, raw in self.inputs:
            bad = np.flatnonzero(self.buf[start:start + raw.size].cpu().numpy() != raw)
            assert bad.size == 0, "%s (%d bytes): an input was written, first at offset %d (%d bytes changed)" % (
                name, raw.size, int(bad[0]), bad.size)


def ptr(view):
    """The pointer a C entry point takes: None (NULL) for None and for a buffer of no bytes."""
    return None if view is None or view.numel() == 0 else view.data_ptr()
