"""gcs_superpixel_segment (csrc/superpixel.hip) called directly (tests/superpixel_raw.py: garbage in every buffer, guard bytes) on
hand-made features, grids and edges that Gabor features never produce, against the restatement on the caller's grid
(``superpixel_ref.superpixels_on_grid``): labels, centres and positions with ``==``, never against the GPU's own output. Every
group first shows on the restatement alone (its trace, or NumPy in the test) that its inputs reach what it is about: ties between
distinct centres in the last assign, a centre without a pixel at an update, a spatial term past 2^32, a tile at and a tile above
the 32 centres the pass holds in LDS, 4096 centres."""
import numpy as np
import pytest

import superpixel_raw as raw
import superpixel_ref as sr

pytestmark = pytest.mark.gpu
TOP = 46340                                                # the largest canonical feature value (include/gcs.h)


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _noise(seed, b, d, h, w, top=TOP):
    """(B, D, H, W) uint16, uniform in 0 .. top."""
    return np.random.default_rng(seed).integers(0, top + 1, (b, d, h, w)).astype(np.uint16)


def _reference(x, ny, nx, lam, n_iter):
    """[(labels, centres, trace)] of the restatement, image by image."""
    out = []
    for xi in x:
        trace = []
        lab, cen = sr.superpixels_on_grid(xi, ny, nx, lam, n_iter, return_centres=True, trace=trace)
        assert len(trace) == n_iter
        out.append((lab, cen, trace))
    return out


def _check(torch, x, ny, nx, lam, n_iter, ref=None):
    """Labels and centres of the raw call == the restatement's, image by image; returns the restatement's [(labels, centres, trace)]."""
    ref = _reference(x, ny, nx, lam, n_iter) if ref is None else ref
    lab, cen = raw.run(torch, x, ny, nx, lam, n_iter)
    for i, (want, wc, _) in enumerate(ref):
        assert cen[i].shape == wc.shape, (cen[i].shape, wc.shape)
        bad = np.flatnonzero((cen[i] != wc).any(axis=1))
        assert np.array_equal(lab[i], want), (i, x.shape, (ny, nx), lam, int((lab[i] != want).sum()), np.argwhere(lab[i] != want)[:4].tolist())
        assert bad.size == 0, (i, x.shape, (ny, nx), lam, bad[:8].tolist(), cen[i][bad[:2]].tolist(), wc[bad[:2]].tolist())
    return ref


# ---- a. D at its edges

@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 7, 8, 206, 207])
def test_quad_tail_and_largest_rows(torch_cuda, d):
    """D = 1 .. 8 (every remainder of the uint16 quads, in init, pass and update) and D = 206, 207 (52 quads: an even count whose last
    quad holds two or three planes, the largest LDS rows), full-range noise, two images, lambda = 1 and 576."""
    h, w = (24, 40) if d <= 8 else (16, 40)
    x = _noise(100 + d, 2, d, h, w)
    for lam in (1, 576):
        _check(torch_cuda, x, 3, 5, lam, 4)


def test_two_valued_planes_at_d_207_pass_2_38(torch_cuda):
    """207 planes that are 0 on the left half and 46 340 on the right half (mirrored in the second image): a pixel beside the edge
    is 207 * 46 340^2 = 4.4e11 away from a candidate of the other side."""
    left = np.zeros((16, 40), np.uint16)
    left[:, 20:] = TOP
    x = np.stack([np.broadcast_to(left, (207, 16, 40)), np.broadcast_to(TOP - left, (207, 16, 40))])
    for lam in (1, 576):
        ref = _reference(x, 3, 5, lam, 4)
        for _, _, trace in ref:
            assert max(t["dmax"] for t in trace) >= 207 * TOP ** 2 > 2 ** 38
        _check(torch_cuda, x, 3, 5, lam, 4, ref)


# ---- b. ties go to the lowest centre index

def _tied_in_the_last_assign(ref):
    return min(trace[-1]["tied"] for _, _, trace in ref)


def test_ties_of_few_valued_noise(torch_cuda):
    """Values 0 .. 2 in two planes, 5 x 5 cells, lambda = 1, one pass: dozens of pixels are equally far from two different centres."""
    x = _noise(1, 1, 2, 40, 100, top=2)
    ref = _reference(x, 8, 20, 1, 1)
    assert _tied_in_the_last_assign(ref) >= 20, ref[0][2]
    _check(torch_cuda, x, 8, 20, 1, 1, ref)


# (constant planes on 40 x 100 with the 8 x 20 grid and on 37 x 53 with the 1 x 2 grid have no tied pixel in the last of four assigns -
# odd cells, centres in their middle - so they are not here; 40 x 100 with 4 x 4 cells ties along every cell border instead)
@pytest.mark.parametrize("h,w,ny,nx", [(16, 24, 2, 3), (37, 53, 12, 1), (40, 100, 10, 25)])
@pytest.mark.parametrize("d", [1, 6])
def test_ties_of_constant_planes(torch_cuda, d, h, w, ny, nx):
    """Constant planes (another constant per plane): the feature term is 0, so whole rows and columns of pixels sit between two
    centres, and at cell corners between four; the order of the nine candidates decides every one of them, in all four assigns."""
    x = np.broadcast_to((np.arange(d) * 9001 + 7).astype(np.uint16)[None, :, None, None], (1, d, h, w))
    for lam in (1, 576, 65535):
        ref = _reference(x, ny, nx, lam, 4)
        assert _tied_in_the_last_assign(ref) >= 20, ref[0][2]
        _check(torch_cuda, x, ny, nx, lam, 4, ref)


# ---- c. an empty centre keeps its values

EMPTY_SEED, FULL_SEEDS = 0, (1, 2)                         # noise of these seeds: one centre empties / none does (asserted below)


def _empty_case(seed):
    return _noise(seed, 1, 2, 33, 70, top=TOP - 1)[0]


def test_empty_centre_keeps_features_and_position(torch_cuda):
    """iid noise, 2 x 2 cells, lambda = 1, six passes: a centre receives no pixel from the second assign on, so four updates in a row
    must leave its row alone."""
    x = _empty_case(EMPTY_SEED)[None]
    ref = _reference(x, 16, 35, 1, 6)
    lab, cen, trace = ref[0]
    empties = [t["empty_ids"] for t in trace]
    assert empties[0] == [] and all(len(e) == 1 and e == empties[1] for e in empties[1:]), empties
    q = empties[1][0]
    got_lab, got_cen = raw.run(torch_cuda, x, 16, 35, 1, 6)
    assert not (got_lab[0] == q).any()
    assert np.array_equal(got_cen[0][q], cen[q]), (q, got_cen[0][q].tolist(), cen[q].tolist())
    assert cen[q].any()                                    # (the kept values are not zeros)
    assert np.array_equal(got_lab[0], lab) and np.array_equal(got_cen[0], cen)


def test_empty_centre_in_the_middle_image_only(torch_cuda):
    x = np.stack([_empty_case(FULL_SEEDS[0]), _empty_case(EMPTY_SEED), _empty_case(FULL_SEEDS[1])])
    ref = _reference(x, 16, 35, 1, 6)
    assert [max(t["empty"] for t in trace[:-1]) for _, _, trace in ref] == [0, 1, 0]
    _check(torch_cuda, x, 16, 35, 1, 6, ref)


# ---- d. the spatial term is a 64-bit product

def _winners(x, cen, ny, nx, lam, wrap):
    """Labels of one assign with the centres ``cen`` (K, D + 2), restated apart from superpixel_ref.assign: the spatial term in 64
    bits, or (``wrap``) modulo 2^32 as a 32-bit product would leave it."""
    x = x.astype(np.int64)
    d, h, w = x.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    best, lab = None, None
    for q, ok in ((q, q >= 0) for q in sr.candidates(h, w, ny, nx)):
        qq = np.where(ok, q, 0)
        sp = lam * ((yy - cen[qq, d]) ** 2 + (xx - cen[qq, d + 1]) ** 2)
        dist = (sp % 2 ** 32 if wrap else sp) + ((x - cen[qq, :d].transpose(2, 0, 1)) ** 2).sum(axis=0)
        dist = np.where(ok, dist, np.iinfo(np.int64).max)
        if best is None:
            best, lab = dist, np.where(ok, q, 2 ** 40)
        else:
            better = (dist < best) | ((dist == best) & ok & (q < lab))
            best, lab = np.where(better, dist, best), np.where(better, q, lab)
    return lab


@pytest.mark.parametrize("h,w,ny,nx", [(8, 4096, 1, 2), (4096, 8, 2, 1), (1, 4096, 1, 1)])
def test_spatial_term_beyond_32_bits(torch_cuda, h, w, ny, nx):
    """lambda = 65 535 over cells 2048 pixels long: lambda (dy^2 + dx^2) reaches 2.7e11. One plane of values 0 .. 3, so the spatial
    term decides; on the two-cell grids hundreds of pixels would change their centre were the product taken modulo 2^32."""
    x = _noise(h, 1, 1, h, w, top=3)
    ref = _reference(x, ny, nx, 65535, 3)
    lab, cen, trace = ref[0]
    assert all(t["smax"] > 2 ** 32 for t in trace), [t["smax"] for t in trace]
    assert np.array_equal(_winners(x[0], cen, ny, nx, 65535, wrap=False), lab)
    if ny * nx > 1:
        assert int((_winners(x[0], cen, ny, nx, 65535, wrap=True) != lab).sum()) >= 100
    _check(torch_cuda, x, ny, nx, 65535, 3, ref)


# ---- e. the 32 centres a tile holds in LDS

def _tile_centres(h, w, ny, nx):
    """{(ty0, tx0): (centres the 8 x 32 tile sees, the set of them)}: the cell range of the tile's pixels, grown by one, clamped."""
    out = {}
    for ty0 in range(0, h, 8):
        for tx0 in range(0, w, 32):
            yl, xl = min(ty0 + 8, h) - 1, min(tx0 + 32, w) - 1
            gi = range(max(ty0 * ny // h - 1, 0), min(yl * ny // h + 1, ny - 1) + 1)
            gj = range(max(tx0 * nx // w - 1, 0), min(xl * nx // w + 1, nx - 1) + 1)
            out[(ty0, tx0)] = (len(gi) * len(gj), {i * nx + j for i in gi for j in gj})
    return out


@pytest.mark.parametrize("h,w,ny,nx,counts", [(40, 100, 8, 20, {6, 8, 10, 24, 27, 32, 36, 40, 45}), (40, 64, 8, 13, {24, 32, 40}),
                                              (48, 96, 8, 16, {21, 24, 28, 32})])
def test_tiles_at_and_above_the_lds_cap(torch_cuda, h, w, ny, nx, counts):
    """Tiles that see exactly 32 centres (the LDS form at its cap) beside tiles that see more (the global-atomics form) in one
    launch, and centres whose sums both forms add into; 48 x 96 stays in the LDS form everywhere, with tiles at 32."""
    tiles = _tile_centres(h, w, ny, nx)
    assert {n for n, _ in tiles.values()} == counts and 32 in counts
    x = _noise(h + w, 2, 5, h, w)
    mixed = max(counts) > 32
    for lam in (1, 576):
        ref = _reference(x, ny, nx, lam, 4)
        if mixed:
            for xi in x:                                   # the first assign is an accumulating pass: who adds into which centre
                first = sr.superpixels_on_grid(xi, ny, nx, lam, 1)
                lds, glob = set(), set()
                for (ty0, tx0), (n, _) in tiles.items():
                    (lds if n <= 32 else glob).update(np.unique(first[ty0:ty0 + 8, tx0:tx0 + 32]).tolist())
                assert lds & glob, (h, w, lam)
        _check(torch_cuda, x, ny, nx, lam, 4, ref)


# ---- f. K at its ceiling, and grids gcs_superpixel_grid never returns

@pytest.mark.parametrize("h,w,ny,nx,d", [(64, 64, 64, 64, 3), (128, 128, 64, 64, 3), (40, 9, 40, 1, 4), (9, 40, 1, 40, 4)])
def test_4096_centres_and_one_pixel_wide_cells(torch_cuda, h, w, ny, nx, d):
    """K = 4096 as one-pixel and as 2 x 2 cells; ny = H with nx = 1 and ny = 1 with nx = W (rows and columns of one-pixel-thick cells)."""
    x = _noise(h * w + d, 2, d, h, w)
    for lam in (1, 576):
        _check(torch_cuda, x, ny, nx, lam, 3)


# ---- g. one pass, and the optional output

def test_one_pass_is_the_init_pixels_and_the_first_assign(torch_cuda):
    x = _noise(7, 2, 5, 24, 40)
    cy, cx = sr.init_positions(24, 40, 3, 5)
    lab, cen = raw.run(torch_cuda, x, 3, 5, 576, 1)
    for i, xi in enumerate(x):
        init = xi.astype(np.int64)[:, cy, cx].T
        assert np.array_equal(cen[i][:, :5], init) and np.array_equal(cen[i][:, 5], cy) and np.array_equal(cen[i][:, 6], cx)
        assert np.array_equal(lab[i], sr.assign(xi.astype(np.int64), init, cy, cx, 3, 5, 576))
    _check(torch_cuda, x, 3, 5, 576, 1)


@pytest.mark.parametrize("n_iter", [1, 4])
def test_without_centres_out_the_labels_are_the_same_and_nothing_else_is_written(torch_cuda, n_iter):
    """centres_out = NULL: the helper keeps the centres buffer and its guards, and finds 0xAB in all of them afterwards."""
    x = _noise(8, 2, 5, 24, 40)
    ref = _reference(x, 3, 5, 576, n_iter)
    lab, cen = raw.run(torch_cuda, x, 3, 5, 576, n_iter, centres=False)
    with_cen, _ = raw.run(torch_cuda, x, 3, 5, 576, n_iter)
    assert cen is None and np.array_equal(lab, with_cen)
    for i, (want, _, _) in enumerate(ref):
        assert np.array_equal(lab[i], want), i


# ---- h. partial tiles

@pytest.mark.parametrize("h,w,ny,nx", [(9, 33, 2, 3), (15, 63, 3, 5), (17, 39, 2, 4), (1, 7, 1, 2)])
def test_partial_tiles(torch_cuda, h, w, ny, nx):
    """W mod 32 in {1, 31, 7}, H mod 8 in {1, 7}: tiles with one valid column, one valid row, lanes of an eight-lane group outside."""
    x = _noise(h * w, 2, 3, h, w)
    for lam in (1, 576):
        _check(torch_cuda, x, ny, nx, lam, 4)
