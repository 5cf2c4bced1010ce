"""A NumPy codec of the feature slab, written from the prose at the head of csrc/common.h and SPEC.md §3, for the tests only: where
every value of every pyramid level sits, which bytes hold no pixel, how a slab is packed from per-level arrays and read back.

It is built the other way round from the library: the library asks "where does pixel (y, x) sit" (gcs_locate); here every BLOCK
enumerates its slots and says which level pixel each one holds, if any, and the pixel -> slot tables are the inverse of that list.

Terms. A block has side 8 >> L slots on level L; four consecutive blocks are a tile. Main blocks lie in raster order; behind them
the virtual blocks of a packed right edge (W mod 8 in {1, 2}), then those of a packed bottom edge (H mod 8 in {1, 2}) - only for banks
of at most two levels and shapes of at least 8 x 8. A virtual block holds 16 consecutive level-1 parents of its strip, parent q
in parent slot (q >> 2, q & 3), and under it the parent's up to four pixels.

Logical feature d = c F + f, f = 2 L n_orient + fl: the planes of level L, in ascending d, are (channel, filter in level) - the
physical order inside a level as well. ``levels[L]`` is (B, D_L, H_L, W_L) uint16 in that order."""
import functools

import numpy as np


def _level_planes(ns, no):
    """Per level: the logical features d of its planes, ascending."""
    f_n = ns * no
    out = []
    for lev in range((ns + 1) // 2):
        fl_n = min(2, ns - 2 * lev) * no
        out.append(np.array([c * f_n + 2 * lev * no + fl for c in range(3) for fl in range(fl_n)]))
    return out


class Geometry:
    """h, w, ns, no; n_levels, planes[L] (logical d of level L's planes), hl[L], wl[L]; split; nblk, ntiles, tile_bytes, value_bytes
    (= ntiles * tile_bytes: the bytes that hold values), img_bytes, pass_bytes (what a Lloyd pass streams when no tile is flagged:
    LO and MID, 3/4 of a split slab's value_bytes; all of a wide slab), mid_off / top_off / flag_off (split).

    Per level L: ``tile[L]`` (H_L, W_L) the tile of a level pixel, ``base[L]`` (H_L, W_L) and ``stride[L]``: plane i of the level
    sits at ``base + i * stride`` - a BYTE offset in the image's slab (wide), a SLOT index (split: the LO byte; nibble_of gives MID /
    TOP)."""

    def __init__(self, h, w, ns, no):
        assert h >= 1 and w >= 1 and 1 <= ns <= 8 and no >= 1
        self.h, self.w, self.ns, self.no = h, w, ns, no
        self.planes = _level_planes(ns, no)
        self.n_levels = len(self.planes)
        self.d = 3 * ns * no
        self.split = self.n_levels <= 2 and self.d < 80
        self.hl, self.wl = [h], [w]
        for _ in range(1, self.n_levels):
            self.hl.append((self.hl[-1] + 1) // 2)
            self.wl.append((self.wl[-1] + 1) // 2)
        may_pack = self.n_levels <= 2 and h >= 8 and w >= 8
        self.pack_r = may_pack and w % 8 in (1, 2)
        self.pack_b = may_pack and h % 8 in (1, 2)
        self.bx_n = w // 8 if self.pack_r else -(-w // 8)
        self.by_n = h // 8 if self.pack_b else -(-h // 8)
        self.nmain = self.bx_n * self.by_n
        wm, hm = 8 * self.bx_n, 8 * self.by_n                  # first column / row of a packed strip
        wb = wm if self.pack_r else w                            # the bottom strip's columns: the corner is the right strip's
        self.n_r = -(-((h + 1) // 2) // 16) if self.pack_r else 0
        self.n_b = -(-((wb + 1) // 2) // 16) if self.pack_b else 0
        self.nblk = self.nmain + self.n_r + self.n_b
        self.ntiles = -(-self.nblk // 4)
        npl = [256 >> (2 * lev) for lev in range(self.n_levels)]  # values of one plane in a tile
        dl = [len(p) for p in self.planes]
        if self.split:
            runs = [-(-dl[lev] * npl[lev] // 32) * 32 for lev in range(self.n_levels)]         # slots
            self.s = sum(runs)
            self.tile_bytes = 2 * self.s
            self.value_bytes = self.ntiles * self.tile_bytes
            self.mid_off, self.top_off, self.flag_off = self.ntiles * self.s, self.ntiles * self.s * 3 // 2, self.value_bytes
            self.img_bytes = self.value_bytes + -(-4 * self.ntiles // 256) * 256
            self.pass_bytes = self.value_bytes * 3 // 4
            unit, tile_stride = 1, self.s
        else:
            runs = [-(-dl[lev] * npl[lev] * 2 // 16) * 16 for lev in range(self.n_levels)]     # bytes
            self.tile_bytes = sum(runs)
            self.value_bytes = self.img_bytes = self.pass_bytes = self.ntiles * self.tile_bytes
            unit, tile_stride = 2, self.tile_bytes
        start = np.concatenate([[0], np.cumsum(runs)[:-1]])
        self.tile, self.base, self.stride = [], [], []
        for lev in range(self.n_levels):
            side = 8 >> lev
            blk, sy, sx, yy, xx = self._slots_of_blocks(lev, side, wm, hm, wb)
            keep = (yy < self.hl[lev]) & (xx < self.wl[lev])
            blk, sy, sx, yy, xx = (a[keep] for a in (blk, sy, sx, yy, xx))
            if self.split:      # a plane's slots in (slot row, block in tile, slot column) order
                inside = sy * 4 * side + (blk & 3) * side + sx
            else:               # (block in tile, slot row, slot column)
                inside = (blk & 3) * side * side + sy * side + sx
            base = np.full((self.hl[lev], self.wl[lev]), -1, np.int64)
            tile = np.full((self.hl[lev], self.wl[lev]), -1, np.int64)
            base[yy, xx] = (blk >> 2) * tile_stride + start[lev] + inside * unit
            tile[yy, xx] = blk >> 2
            before = np.zeros(base.shape, np.int32)
            np.add.at(before, (yy, xx), 1)
            assert (before == 1).all(), "every level pixel sits in exactly one slot"
            self.base.append(base)
            self.tile.append(tile)
            self.stride.append(npl[lev] * unit)

    def _slots_of_blocks(self, lev, side, wm, hm, wb):
        """Every slot of every block on level ``lev`` -> (block, slot row, slot column, level-pixel row, column); a slot whose pixel
        lies outside the level image holds none (the caller drops it)."""
        sy, sx = (a.reshape(-1) for a in np.mgrid[0:side, 0:side])
        out = []
        by, bx = (a.reshape(-1) for a in np.mgrid[0:self.by_n, 0:self.bx_n])
        blk = by * self.bx_n + bx
        # main blocks: slot (sy, sx) of block (by, bx) = level pixel (side by + sy, side bx + sx); beside a packed strip the main
        # blocks end where the strip begins (bx_n, by_n count whole blocks there)
        yy = (side * by)[:, None] + sy[None]
        xx = (side * bx)[:, None] + sx[None]
        out.append((np.broadcast_to(blk[:, None], yy.shape), np.broadcast_to(sy[None], yy.shape), np.broadcast_to(sx[None], yy.shape),
                    yy, xx))
        for first, count, right in ((self.nmain, self.n_r, True), (self.nmain + self.n_r, self.n_b, False)):
            if not count:
                continue
            assert lev <= 1
            v = np.arange(count)[:, None]
            if lev == 1:        # parent q of block v sits in parent slot (q >> 2, q & 3): parent 16 v + q of the strip
                along = 16 * v + (4 * sy + sx)[None]
                across = np.zeros_like(along)
            else:               # under its parent, a pixel keeps its place inside the 2 x 2
                along = 2 * (16 * v + (4 * (sy >> 1) + (sx >> 1))[None]) + ((sy & 1) if right else (sx & 1))[None]
                across = np.broadcast_to(((sx & 1) if right else (sy & 1))[None], along.shape)
            if right:
                yy, xx = along, (wm >> lev) + across
            else:
                yy, xx = (hm >> lev) + across, np.where(along < -(-wb >> lev), along, 1 << 30)
            shape = yy.shape
            out.append((np.broadcast_to(first + v, shape), np.broadcast_to(sy[None], shape), np.broadcast_to(sx[None], shape), yy, xx))
        return tuple(np.concatenate([np.asarray(o[i]).reshape(-1) for o in out]) for i in range(5))

    def index(self, lev):
        """(D_L, H_L, W_L) int64: the slot of every (plane, y_L, x_L) - byte offset (wide) or slot index (split)."""
        return self.base[lev][None] + (np.arange(len(self.planes[lev])) * self.stride[lev])[:, None, None]

    @staticmethod
    def nibble_of(lev, slot):
        """Split slab: (byte inside the MID / TOP array, shift) of a slot's nibble. Groups of g = max(2, 8 >> L) consecutive slots;
        byte i < g / 2 of a group holds slot i in bits 0..3 and slot i + g / 2 in bits 4..7."""
        g = max(2, 8 >> lev)
        in_group = slot % g
        return (slot // g) * (g // 2) + in_group % (g // 2), 4 * (in_group >= g // 2)

    def pixel_bits(self):
        """(img_bytes,) uint8: the bits of every byte that belong to some pixel's value (0xFF, or one nibble of a MID / TOP byte)."""
        bits = np.zeros(self.img_bytes, np.uint8)
        for lev in range(self.n_levels):
            idx = self.index(lev).reshape(-1)
            if self.split:
                bits[idx] = 0xFF
                byte, shift = self.nibble_of(lev, idx)
                for off in (self.mid_off, self.top_off):
                    bits[off + byte[shift == 0]] |= 0x0F          # (the slots of one half never share a byte)
                    bits[off + byte[shift == 4]] |= 0xF0
            else:
                bits[idx] = 0xFF
                bits[idx + 1] = 0xFF
        return bits

    def no_pixel_bits(self):
        """(img_bytes,) uint8: the bits of the VALUE bytes that hold no pixel - ragged main blocks, unused slots of the virtual strip
        blocks, the blocks missing from a last tile, level padding. Zero on the flag words and their padding."""
        bits = ~self.pixel_bits()
        bits[self.value_bytes:] = 0
        return bits

    # ------------------------------------------------------------------------------------------ pack / unpack
    def pack(self, levels, filler=0):
        """levels[L] (B, D_L, H_L, W_L) uint16 -> (B, img_bytes) uint8. ``filler``: the byte written to every no-pixel slot; the
        flag words come from the pixels' TOP nibbles alone, their padding is zero."""
        b = levels[0].shape[0]
        raw = np.zeros((b, self.img_bytes), np.uint8)
        for lev in range(self.n_levels):
            x = np.asarray(levels[lev])
            assert x.dtype == np.uint16 and x.shape == (b, len(self.planes[lev]), self.hl[lev], self.wl[lev]), (lev, x.shape, x.dtype)
            idx = self.index(lev).reshape(-1)
            v = x.reshape(b, -1)
            if self.split:
                raw[:, idx] = (v & 0xFF).astype(np.uint8) ^ 0x80
                byte, shift = self.nibble_of(lev, idx)
                first = shift == 0                                # (two slots share a byte: one half at a time)
                for off, sh in ((self.mid_off, 8), (self.top_off, 12)):
                    nib = ((v >> sh) & 15).astype(np.uint8)
                    raw[:, off + byte[first]] |= nib[:, first]
                    raw[:, off + byte[~first]] |= nib[:, ~first] << 4
                flagged = np.zeros((b, self.ntiles), bool)
                t = np.broadcast_to(self.tile[lev][None], (len(self.planes[lev]),) + self.tile[lev].shape).reshape(-1)
                for i in range(b):
                    flagged[i, np.unique(t[v[i] >= 4096])] = True
                raw[:, self.flag_off + 4 * np.arange(self.ntiles) + lev] = flagged
            else:
                o = v ^ 0x8080
                raw[:, idx] = (o & 0xFF).astype(np.uint8)
                raw[:, idx + 1] = (o >> 8).astype(np.uint8)
        mask = self.no_pixel_bits()
        return (raw & ~mask) | (np.uint8(filler) & mask)

    def unpack_levels(self, raw):
        """(B, img_bytes) uint8 -> levels[L] (B, D_L, H_L, W_L) uint16; a split slab's TOP nibbles count only under a set flag, as a
        Lloyd pass reads them. (gcs_slab_value reads the nibble whatever the flag says; on a legal slab, whose flag is set wherever a
        TOP nibble of a pixel is non-zero, the two readings agree.)"""
        raw = np.asarray(raw, np.uint8).reshape(-1, self.img_bytes)
        b = raw.shape[0]
        out = []
        for lev in range(self.n_levels):
            idx = self.index(lev)
            shape = (b,) + idx.shape
            idx = idx.reshape(-1)
            if self.split:
                byte, shift = self.nibble_of(lev, idx)
                low = (raw[:, idx] ^ 0x80).astype(np.uint16)
                mid = ((raw[:, self.mid_off + byte] >> shift) & 15).astype(np.uint16)
                top = ((raw[:, self.top_off + byte] >> shift) & 15).astype(np.uint16)
                flag = raw[:, self.flag_off + 4 * np.arange(self.ntiles) + lev] != 0                   # (B, ntiles)
                t = np.broadcast_to(self.tile[lev][None], (len(self.planes[lev]),) + self.tile[lev].shape).reshape(-1)
                top = np.where(flag[:, t], top, 0).astype(np.uint16)
                v = low | (mid << 8) | (top << 12)
            else:
                v = (raw[:, idx].astype(np.uint16) | (raw[:, idx + 1].astype(np.uint16) << 8)) ^ 0x8080
            out.append(v.reshape(shape))
        return out

    def canonical(self, levels):
        """levels -> (B, D, H, W) uint16 in logical feature order, level L replicated over its 2^L x 2^L blocks."""
        b = levels[0].shape[0]
        out = np.empty((b, self.d, self.h, self.w), np.uint16)
        y, x = np.mgrid[0:self.h, 0:self.w]
        for lev in range(self.n_levels):
            out[:, self.planes[lev]] = levels[lev][:, :, y >> lev, x >> lev]
        return out

    def levels_of(self, canon):
        """A canonical (B, D, H, W) tensor -> its levels (every 2^L-th row and column of a level's planes)."""
        step = [1 << lev for lev in range(self.n_levels)]
        return [np.ascontiguousarray(np.asarray(canon)[:, self.planes[lev], ::step[lev], ::step[lev]]) for lev in range(self.n_levels)]

    def unpack(self, raw):
        return self.canonical(self.unpack_levels(raw))

    def flags(self, raw):
        """(B, ntiles, 4) uint8: the flag words of a split slab."""
        raw = np.asarray(raw, np.uint8).reshape(-1, self.img_bytes)
        return raw[:, self.flag_off:self.flag_off + 4 * self.ntiles].reshape(-1, self.ntiles, 4)

    def set_flags(self, raw, value=1):
        """Set every flag byte of a split slab's (B, img_bytes) bytes, in place (so that every TOP nibble counts)."""
        if self.split:
            raw.reshape(-1, self.img_bytes)[:, self.flag_off:self.flag_off + 4 * self.ntiles] = value
        return raw


@functools.lru_cache(maxsize=24)         # (the tables of a shape are built once per run of tests; 481 x 321 holds 1.2 MB a level)
def geometry(h, w, n_scales, n_orient):
    return Geometry(h, w, n_scales, n_orient)


def pack(geo, levels, filler=0):
    return geo.pack(levels, filler)


def unpack(geo, raw):
    return geo.unpack(raw)
