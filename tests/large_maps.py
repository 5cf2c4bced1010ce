"""What tests/test_gpu_large_maps.py and its CPU companion (tests/test_large_map_geometry.py) share: the batches of label maps,
images, annotator maps and canonical tensors that cross element index and byte offset 2^31 / 2^32, built by replication of sixteen
distinct base arrays through the index sequence of tests/large_offsets.py, and the host assertions about them. No GPU here.

The shape, 161 x 241: 161 = 8 * 20 + 1 and 241 = 8 * 30 + 1, no side a multiple of 8, 16, 32 or 64, so every kernel's last tile in
either direction is ragged (the 8 x 32 tiles of the half-disc gradients, 16 x 64 of the sweep, the 64-bit plane words, the 4096-pixel
runs of the contour and paint kernels, four labels per thread in gcs_labels_widen: P = 38 801 is odd). P >= 32 769, so B <= 65535
reaches 2^31 pixels; one image is 38 801 pixels against the 2^21 = 2 097 152 (54 images) a batch reaches past its line."""
import numpy as np

from large_offsets import N_BASE, batch_order, multiplicity  # noqa: F401  (the sequence and its counts are the slab file's)

LINE31, LINE32, LINE33 = 1 << 31, 1 << 32, 1 << 33
MARGIN = 1 << 21                     # pixels a batch ends behind its line: 54 images
H, W = 161, 241
P = H * W
K_LABELS = 48                        # labels of the base maps: below the 64 bins of the half-disc gradients
D_CANON = 72                         # the default bank's feature count


def count_for(line, per_image=P):
    """The smallest B with B * per_image >= line + MARGIN."""
    return -(-(line + MARGIN) // per_image)


N31, N30, N29 = count_for(LINE31), count_for(1 << 30), count_for(1 << 29)
B_GUARD = (LINE31 - 1) // P          # the largest B with B * H * W < 2^31 (gcs_region_adjacency, gcs_cut_shapes)
N_CANON = count_for(LINE32, D_CANON * P)                       # images of the canonical batch: B D H W >= 2^32 + 2^21 elements
N_COLOUR = -(-(LINE32 + MARGIN) // (3 * P))                    # images of gcs_colour_opponent: 3 n_pixels >= 2^32 + 2^21 bytes


# ---- the sixteen base arrays (host, deterministic)
def base_labels(k=K_LABELS, seed=161):
    """int32 [16][H][W] in 0 .. k-1: blocks of 7 x 11 pixels whose numbering turns with the map's number, a twentieth of the pixels
    redrawn; pixel (0, 0) is 0 and the last pixel k - 1 in every map."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    blocks = (yy // 7) * (-(-W // 11)) + xx // 11
    maps = np.stack([(blocks * (2 * j + 1) + 5 * j) % k for j in range(N_BASE)]).astype(np.int32)
    noise = rng.random(maps.shape) < 0.05
    maps[noise] = rng.integers(0, k, int(noise.sum()))
    maps[:, 0, 0], maps[:, H - 1, W - 1] = 0, k - 1
    return np.ascontiguousarray(maps)


def base_images(seed=241):
    """uint8 [16][H][W][3]: a block picture per map (blocks of 5 x 9) with noise of +-24 on top; all 256 values occur."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, (N_BASE, -(-H // 5), -(-W // 9), 3))
    img = coarse.repeat(5, axis=1).repeat(9, axis=2)[:, :H, :W] + rng.integers(-24, 25, (N_BASE, H, W, 3))
    return np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8))


def base_truth(seed=38801):
    """uint16 [16][H][W] annotator maps with values 1 .. 9 (below 256: they narrow to uint8): blocks of 12 x 12, a tenth of the
    pixels redrawn so that no two maps agree over a window."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(1, 10, (N_BASE, -(-H // 12), -(-W // 12)))
    t = coarse.repeat(12, axis=1).repeat(12, axis=2)[:, :H, :W].copy()
    noise = rng.random(t.shape) < 0.1
    t[noise] = rng.integers(1, 10, int(noise.sum()))
    return np.ascontiguousarray(t.astype(np.uint16))


def base_canonical(d=D_CANON, seed=72):
    """uint16 [16][d][H][W] over SPEC.md §3's whole value range (0 .. 46 339): per feature a block picture (blocks of 10 x 14, so
    that superpixels and regions have something to find) with noise of +-2000 on top."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 46340, (N_BASE, d, -(-H // 10), -(-W // 14)))
    x = coarse.repeat(10, axis=2).repeat(14, axis=3)[:, :, :H, :W] + rng.integers(-2000, 2001, (N_BASE, d, H, W))
    return np.ascontiguousarray(np.clip(x, 0, 46339).astype(np.uint16))


# ---- the lines an array crosses, and what stands on either side of them
def lines_of(elem_bytes, per_image, b):
    """[(what, element offset of the line)] for an array of b images of per_image elements of elem_bytes bytes: element index 2^31
    and 2^32, byte offset 2^31, 2^32 and 2^33, each where it falls strictly inside the array (for one-byte elements an element
    line and a byte line are the same line: named once)."""
    n = b * per_image
    out = [("element 2^%d" % s, 1 << s) for s in (31, 32) if (1 << s) < n]
    if elem_bytes > 1:
        out += [("byte 2^%d" % s, (1 << s) // elem_bytes) for s in (31, 32, 33) if (1 << s) // elem_bytes < n]
    return out


def content(base_flat, idx, a):
    """The elements at the element addresses ``a`` (int64 array) of the batch base_flat[idx] laid out image after image."""
    n = base_flat.shape[1]
    return base_flat[idx[a // n], a % n]


def check_array(base, idx, elem_bytes, want):
    """base [16][...] of one element size: the batch base[idx] crosses exactly the lines ``want`` names; for each of them an image
    straddles the line, the base arrays below, across and above it are three different ones, and at the straddler and at a sample
    above it (three images on, or the batch's last image where the batch ends sooner: an image of the canonical batch is larger than
    the margin) the content found at "its address minus the line" differs from its own in more than half the elements (an address
    truncated by the line reads visibly wrong data). -> {line name: straddler}."""
    flat = base.reshape(N_BASE, -1)
    n, b = flat.shape[1], len(idx)
    assert flat.dtype.itemsize == elem_bytes, (flat.dtype, elem_bytes)
    assert len({r.tobytes() for r in flat}) == N_BASE                                       # sixteen DIFFERENT base arrays
    lines = lines_of(elem_bytes, n, b)
    assert [name for name, _ in lines] == list(want), ([name for name, _ in lines], want)
    out = {}
    for name, at in lines:
        i = at // n
        assert 1 <= i < b - 1 and i * n < at < (i + 1) * n, (name, i)                       # image i straddles the line
        assert len({int(idx[i - 1]), int(idx[i]), int(idx[i + 1])}) == 3, (name, i)       # below, across, above: distinct
        for j in (i, min(i + 3, b - 1)):
            a = np.arange(max(j * n, at), (j + 1) * n, dtype=np.int64)
            own, aliased = content(flat, idx, a), content(flat, idx, a - at)
            assert len(a) and 2 * int((own != aliased).sum()) > len(a), (name, j, float((own != aliased).mean()))
        out[name] = int(i)
    return out


# ---- chunked device work (``torch`` is the caller's): no single torch operation spans 2^31 elements, so that what is tested is the
# library's addressing and not torch's
TORCH_SPAN = 1 << 26                 # elements one torch operation may touch here (a gathered chunk is at most 512 MiB)


def chunk_of(per_image):
    """Images (rows of the first axis) one torch operation takes."""
    return max(1, TORCH_SPAN // max(1, per_image))


def per_image_of(t):
    n = 1
    for s in t.shape[1:]:
        n *= int(s)
    return n


def filled(torch, shape, dtype, value):
    """A device tensor of ``shape`` holding ``value`` everywhere, written chunk by chunk along its first axis."""
    out = torch.empty(shape, dtype=dtype, device="cuda")
    step = chunk_of(per_image_of(out))
    for i in range(0, shape[0], step):
        out[i:i + step].fill_(value)
    return out


def replicate(torch, small, idx_dev):
    """small[idx] on the device, (len(idx), ...) in chunks of images."""
    out = torch.empty((idx_dev.shape[0],) + tuple(small.shape[1:]), dtype=small.dtype, device="cuda")
    step = chunk_of(per_image_of(small))
    for i in range(0, idx_dev.shape[0], step):
        out[i:i + step] = small[idx_dev[i:i + step]]
    return out


def first_difference(torch, big, small, idx_dev):
    """big (B, ...) == small[idx] in every element, a chunk of images at a time on the device; -> None or (the first image that
    differs, the images that differ in its chunk)."""
    assert big.shape[0] == idx_dev.shape[0] and tuple(big.shape[1:]) == tuple(small.shape[1:]) and big.dtype == small.dtype
    step = chunk_of(per_image_of(small))
    for i in range(0, big.shape[0], step):
        want, got = small[idx_dev[i:i + step]], big[i:i + step]
        if not torch.equal(got, want):
            ne = (got != want).reshape(want.shape[0], -1).any(1)
            return i + int(ne.nonzero()[0]), int(ne.sum())
    return None


def batch(b):
    """idx of a batch of b images; every base array occurs, none rarely."""
    idx = batch_order(b)
    assert idx.min() == 0 and idx.max() == N_BASE - 1 and np.bincount(idx).min() > b // (2 * N_BASE)
    return idx
