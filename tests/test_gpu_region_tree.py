"""GPU region tree (SPEC.md §14): gcs_region_tree / gcs_region_tree_cut and Segmenter(n_superpixels=n, n_regions=R) against the
restatement (tests/region_tree_ref.py on tests/superpixel_ref.py and the features of tests/position_ref.py), bit for bit and never
against the GPU's own output: merges, costs, alive and cut labels on hand-made maps through the raw entry points, then every host
path, graph replay, n_regions = 0, and the scores of six val fixture images against the numbers tools/region_tree_quality.py
wrote (profiles/region_tree_quality.json)."""
import json
import os

import numpy as np
import pytest

import position_ref as pr
import region_tree_ref as rt
import superpixel_ref as sr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)          # the recommended bank of the quality table
COLOUR_REF = dict(w=0.125, g=4, n_orient=5)


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _synth(b, h, w, seed):
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    return synthetic_batch(b, h, w, seed=seed)


# ---- the raw entry points on hand-made maps

def _gpu_tree(torch, x, lab, k, with_costs=True):
    """x (B, D, H, W) values, lab (B, H, W) labels -> (merges, costs uint64, alive) host arrays and the device tensors a cut needs. The
    workspace and the outputs start out as garbage: the call zeroes and fills what it uses."""
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    b, d, h, w = x.shape
    xs = torch.from_numpy(np.ascontiguousarray(x).astype(np.uint16).view(np.int16)).cuda()
    ls = torch.from_numpy(np.ascontiguousarray(lab).astype(np.int32)).cuda()
    need = lib.gcs_region_tree_workspace_bytes(b, h, w, d, k)
    assert need > 0
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    merges = torch.full((b, k - 1, 2), 7, dtype=torch.int32, device="cuda")
    costs = torch.full((b, k - 1), 7, dtype=torch.int64, device="cuda")
    alive = torch.full((b,), -5, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.gcs_region_tree(xs.data_ptr(), ls.data_ptr(), b, h, w, d, k, ws.data_ptr(), merges.data_ptr() if k > 1 else None,
                             costs.data_ptr() if with_costs and k > 1 else None, alive.data_ptr(), st)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    return merges.cpu().numpy(), costs.cpu().numpy().view(np.uint64), alive.cpu().numpy(), (ls, merges, alive)


def _gpu_cut(torch, dev, k, r, in_place=False):
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    ls, merges, alive = dev
    b, h, w = ls.shape
    src = ls.clone() if in_place else ls
    out = src if in_place else torch.full_like(ls, -9)
    rc = lib.gcs_region_tree_cut(src.data_ptr(), merges.data_ptr() if k > 1 else None, alive.data_ptr(), b, h, w, k, r, out.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    return out.cpu().numpy()


def _check_tree(torch, x, lab, k, rs, want_rounds=None):
    """Tree and cuts of every image == the restatement's; returns the restatement's (merges, costs, alive) per image."""
    x, lab = np.asarray(x), np.asarray(lab)
    merges, costs, alive, dev = _gpu_tree(torch, x, lab, k)
    cuts = {r: _gpu_cut(torch, dev, k, r, in_place=(j % 2 == 1)) for j, r in enumerate(rs)}
    refs = []
    for i in range(x.shape[0]):
        info = {}
        m, c, a = rt.build_tree(x[i], lab[i], k, info)
        print("image", i, "K", k, "alive", a, "rounds", info["rounds"], "tied rows", int((c[1:max(a - 1, 1)] == c[:max(a - 2, 0)]).sum()))
        assert int(alive[i]) == a, (i, int(alive[i]), a)
        assert np.array_equal(merges[i], m), (i, int((merges[i] != m).any(axis=1).sum()), merges[i][:6].tolist(), m[:6].tolist())
        assert np.array_equal(costs[i], c), (i, int((costs[i] != c).sum()))
        for r in rs:
            want = rt.cut(lab[i], m, a, r)
            assert np.array_equal(cuts[r][i], want), (i, r, int((cuts[r][i] != want).sum()))
        if want_rounds is not None:
            assert info["rounds"] == want_rounds
        refs.append((m, c, a))
    return refs


def test_worked_example_padded_to_8x8(torch_cuda):
    """SPEC.md §14's example in the first row of an 8 x 8 map whose other pixels carry no label (-1: counted nowhere)."""
    lab = np.full((1, 8, 8), -1, np.int32)
    lab[0, 0, :4] = [0, 1, 2, 3]
    x = np.full((1, 1, 8, 8), 999, np.uint16)
    x[0, 0, 0, :4] = [0, 10, 11, 30]
    (m, c, a), = _check_tree(torch_cuda, x, lab, 4, (1, 2, 3, 4, 9), want_rounds=3)
    assert m.tolist() == [[1, 2], [0, 1], [0, 3]] and c.tolist() == [1, 121, 529] and a == 4


def test_one_pixel_labels_37x53(torch_cuda):
    """K = 1961 one-pixel labels, D = 12: a tile sees 256 labels (the statistics kernel's global form), an odd shape, 62-word rows."""
    rng = np.random.default_rng(7)
    x = rng.integers(0, 46340, (1, 12, 37, 53)).astype(np.uint16)
    lab = np.arange(37 * 53, dtype=np.int32).reshape(1, 37, 53)
    _check_tree(torch_cuda, x, lab, 37 * 53, (1, 8, 500, 1961))


def test_one_pixel_labels_64x64_with_tied_costs(torch_cuda):
    """K = 4096 (the means stay in the workspace), D = 4, values 0 .. 299: many equal costs, so the order inside a round and the
    rep tie-break decide the rows."""
    rng = np.random.default_rng(0)
    x = rng.integers(0, 300, (1, 4, 64, 64)).astype(np.uint16)
    lab = np.arange(4096, dtype=np.int32).reshape(1, 64, 64)
    (m, c, a), = _check_tree(torch_cuda, x, lab, 4096, (1, 8, 4096))
    assert a == 4096 and int((c[1:] == c[:-1]).sum()) > 10


def test_constant_24x24_takes_575_rounds(torch_cuda):
    x = np.full((1, 3, 24, 24), 5, np.uint16)
    lab = np.arange(576, dtype=np.int32).reshape(1, 24, 24)
    (m, c, a), = _check_tree(torch_cuda, x, lab, 576, (1, 2, 575), want_rounds=575)
    assert not c.any()


def _three_labels():
    lab = np.full((8, 12), 7, np.int32)
    lab[:, :2] = 3
    lab[:, 10:] = 3
    lab[3:5, 4:8] = 12
    x = np.zeros((2, 8, 12), np.uint16)
    for q, v in ((3, 100), (7, 90), (12, 10)):
        x[:, lab == q] = v
    return x, lab


def test_unused_labels_a_label_in_two_pieces_and_out_of_range_labels(torch_cuda):
    x, lab = _three_labels()
    (m, c, a), = _check_tree(torch_cuda, x[None], lab[None], 16, (1, 2, 3, 16))
    assert a == 3 and m[:2].tolist() == [[3, 7], [3, 12]]
    # labels outside 0 .. K-1 (negative, K, far beyond): counted nowhere, adjacent to nothing, -1 after the cut
    lab2 = lab.copy()
    lab2[0, :] = 16
    lab2[5, 3] = -1
    lab2[7, 7] = 2 ** 31 - 1
    lab2[6, 6] = -2 ** 31
    (m, c, a), = _check_tree(torch_cuda, x[None], lab2[None], 16, (1, 2, 16))
    assert a == 3
    # a column of out-of-range labels cuts the graph apart: the rounds stop when nothing is adjacent
    lab3 = np.arange(6, dtype=np.int32).reshape(2, 3).repeat(4, axis=0).repeat(4, axis=1)
    lab3[:, 4:8] = 99
    x3 = (lab3 * 7 % 50).astype(np.uint16)[None]
    (m, c, a), = _check_tree(torch_cuda, x3[None], lab3[None], 6, (1, 3, 6))
    assert a == 4 and (m[2:] == -1).all()


def test_batch_of_three_images_with_different_alive(torch_cuda):
    rng = np.random.default_rng(11)
    lab = np.stack([rng.integers(0, 50, (19, 45)), rng.integers(0, 7, (19, 45)), np.zeros((19, 45), np.int64)]).astype(np.int32)
    lab[0][lab[0] == 13] = 14
    x = rng.integers(0, 46340, (3, 5, 19, 45)).astype(np.uint16)
    refs = _check_tree(torch_cuda, x, lab, 50, (1, 4, 50))
    assert [r[2] for r in refs] == [49, 7, 1]


def test_costs_beyond_2_53_and_picks_between_costs_beyond_2_32(torch_cuda):
    """D = 207, 256 x 256: two labels of 32 769 and 32 767 pixels with values 0 and 46 339 - one merge of cost 207 * 46 339^2 * 32 767,
    odd and above 2^53; then a thin third label between them whose two costs, both near 2.8e13, differ only below bit 32."""
    lab = np.zeros((256, 256), np.int32)
    lab.ravel()[32769:] = 1
    plane = np.where(lab == 0, 0, 46339).astype(np.uint16)
    x = np.broadcast_to(plane, (1, 207, 256, 256))
    (m, c, a), = _check_tree(torch_cuda, x, lab[None], 2, (1, 2))
    assert int(c[0]) == 14564659686168249
    lab = np.zeros((256, 256), np.int32)
    lab[129:] = 1
    lab[128] = 2
    for v, first in ((23170, 1), (23169, 0)):            # the thin label is nearer to label `first` by one unit per plane
        plane = np.where(lab == 0, 0, np.where(lab == 1, 46339, v)).astype(np.uint16)
        (m, c, a), = _check_tree(torch_cuda, np.broadcast_to(plane, (1, 207, 256, 256)), lab[None], 3, (1, 2, 3))
        assert m[0].tolist() == [first, 2] and int(c[0]) == 207 * 23169 ** 2 * 256 > 2 ** 32
        assert 207 * 23170 ** 2 * 256 - int(c[0]) < 2 ** 32


def test_raw_entry_points_refuse_what_is_outside_the_domain(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    b, d, h, w, k = 1, 3, 16, 24, 6
    x = torch.zeros((b, d, h, w), dtype=torch.int16, device="cuda")
    lab = torch.zeros((b, h, w), dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.gcs_region_tree_workspace_bytes(b, h, w, d, k), dtype=torch.uint8, device="cuda")
    merges = torch.full((b, k - 1, 2), -7, dtype=torch.int32, device="cuda")
    alive = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((b, h, w), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    good = dict(x=x.data_ptr(), lab=lab.data_ptr(), B=b, H=h, W=w, D=d, K=k, ws=ws.data_ptr(), m=merges.data_ptr(), a=alive.data_ptr(),
                R=2, out=out.data_ptr())
    for bad in (dict(x=None), dict(lab=None), dict(ws=None), dict(m=None), dict(a=None), dict(B=0), dict(H=0), dict(W=4097), dict(D=0),
                dict(D=208), dict(K=0), dict(K=4097)):
        a = dict(good, **bad)
        assert lib.gcs_region_tree(a["x"], a["lab"], a["B"], a["H"], a["W"], a["D"], a["K"], a["ws"], a["m"], None, a["a"], st) == 1, bad
    for bad in (dict(lab=None), dict(m=None), dict(a=None), dict(out=None), dict(B=0), dict(H=4097), dict(K=0), dict(K=4097), dict(R=0),
                dict(R=-3)):
        a = dict(good, **bad)
        assert lib.gcs_region_tree_cut(a["lab"], a["m"], a["a"], a["B"], a["H"], a["W"], a["K"], a["R"], a["out"], st) == 1, bad
    torch.cuda.current_stream().synchronize()
    assert int((out != -7).sum()) == 0 and int((merges != -7).sum()) == 0 and int(alive[0]) == -7        # nothing was launched
    for args in ((0, h, w, d, k), (b, h, 4097, d, k), (b, h, w, 208, k), (b, h, w, d, 0), (b, h, w, d, 4097)):
        assert lib.gcs_region_tree_workspace_bytes(*args) == 0
    # K = 1: no rows, the merges pointer is not read
    assert lib.gcs_region_tree(good["x"], good["lab"], b, h, w, d, 1, good["ws"], None, None, good["a"], st) == 0
    assert lib.gcs_region_tree_cut(good["lab"], None, good["a"], b, h, w, 1, 3, good["out"], st) == 0
    torch.cuda.current_stream().synchronize()
    assert int(alive[0]) == 1 and int((out != 0).sum()) == 0


# ---- the pipeline

_REFS = {}


def _ref(tag, img, n, n_iter, lam=576, **ref_kw):
    """(superpixel labels, merges, alive, K) of the restatement for one image, computed once per ``tag``."""
    if tag not in _REFS:
        x = pr.features(np.asarray(img), **ref_kw)
        lab = sr.superpixels(x, n, lam, n_iter)
        _, ny, nx = sr.grid(img.shape[0], img.shape[1], n)
        merges, _, alive = rt.build_tree(x, lab, ny * nx)
        _REFS[tag] = (lab, merges, alive, ny * nx)
    return _REFS[tag]


def _ref_cut(tag, img, n, r, n_iter, **kw):
    lab, merges, alive, _ = _ref(tag, img, n, n_iter, **kw)
    return rt.cut(lab, merges, alive, r)


@pytest.mark.parametrize("n", [64, 1200])
def test_small_odd_shape_through_the_plan(torch_cuda, n):
    """37 x 53 with n = 64 and n = 1200 (1961 one-pixel cells), R = 1, 8 and 4096 (>= alive: only renumbers)."""
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(2, 37, 53, seed=n)
    dev = torch_cuda.from_numpy(imgs).cuda()
    for r in (1, 8, 4096):
        got = Segmenter(n_superpixels=n, n_regions=r, n_iter=3).segment_device(dev).cpu().numpy()
        for i, im in enumerate(imgs):
            want = _ref_cut(("odd", n, i), im, n, r, 3)
            assert np.array_equal(got[i], want), (n, r, i, int((got[i] != want).sum()))
            assert got[i].max() + 1 == min(r, _ref(("odd", n, i), im, n, 3)[2])


def test_one_row_grid(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    assert sr.grid(16, 200, 8)[1] == 1
    imgs = _synth(1, 16, 200, seed=16)
    got = Segmenter(n_superpixels=8, n_regions=3, n_iter=4, **COLOUR).segment_batch(imgs)
    assert np.array_equal(got[0], _ref_cut("row", imgs[0], 8, 3, 4, **COLOUR_REF))


@pytest.mark.parametrize("shape", [(481, 321), (321, 481)])
def test_bsd_shapes_on_fixture_images(torch_cuda, shape):
    """Two val fixture images of either orientation, colour bank, n = 300, R = 8: labels == the restatement on superpixel_ref labels."""
    from gabor_color_image_segmentation_amd import Segmenter
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"] if val["img_" + str(i)].shape[:2] == shape][:2]
    assert len(ids) == 2
    imgs = np.stack([val["img_" + i] for i in ids])
    got = Segmenter(n_superpixels=300, n_regions=8, n_iter=4, **COLOUR).segment_device(torch_cuda.from_numpy(imgs).cuda()).cpu().numpy()
    for i, im in enumerate(imgs):
        want = _ref_cut(("bsd", ids[i]), im, 300, 8, 4, **COLOUR_REF)
        assert np.array_equal(got[i], want), (ids[i], int((got[i] != want).sum()))
        assert sorted(np.unique(got[i]).tolist()) == list(range(8))


@pytest.mark.parametrize("bank,ref", [
    (dict(n_orient=4, color_weight=0.125, chroma_gain=4, position_weight=6), dict(w=0.125, g=4, mu=6, n_orient=4)),
    (dict(smoothing=1.0), dict(smoothing=1.0)),
])
def test_position_bank_and_smoothing(torch_cuda, bank, ref):
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(2, 72, 104, seed=31)
    got = Segmenter(n_superpixels=64, n_regions=5, n_iter=4, **bank).segment_batch(imgs)
    for i, im in enumerate(imgs):
        assert np.array_equal(got[i], _ref_cut(("bank", str(sorted(bank)), i), im, 64, 5, 4, **ref)), i


def test_hot_bank_uses_the_whole_cost_range(torch_cuda):
    """Features up to 46 339 (tests/hot_banks.py): squared mean differences near 2^31 per plane, costs far beyond 2^32."""
    import hot_banks as hb
    from oracle import c_oracle as co
    bank = hb.hot_bank(4, 6, 13, 7)
    seg = hb.hot_segmenter(bank, n_superpixels=64, n_regions=4, n_iter=3)
    imgs = hb.hot_images(8, 81, 121, seed=9)
    lab, merges, costs, alive = [t.cpu().numpy() for t in seg.region_tree_device(torch_cuda.from_numpy(imgs).cuda())]
    got = seg.segment_batch(imgs)
    _, ny, nx = sr.grid(81, 121, 64)
    top = 0
    for i, im in enumerate(imgs):
        x = co.gabor_features(im, bank.tapq, bank.shift, bank.n_orient)
        want_lab = sr.superpixels(x, 64, 576, 3)
        m, c, a = rt.build_tree(x, want_lab, ny * nx)
        top = max(top, int(c.max()))
        assert np.array_equal(lab[i], want_lab) and np.array_equal(merges[i], m) and int(alive[i]) == a, i
        assert np.array_equal(costs[i].view(np.uint64), c), i
        assert np.array_equal(got[i], rt.cut(want_lab, m, a, 4)), i
    assert top > 2 ** 40, top


def test_post_passes_on_top_of_the_cut(torch_cuda):
    """min_region_size == merge_ref.merge_small_regions of the reference cut; connectivity=True == §7 of it."""
    from merge_ref import merge_small_regions
    from oracle import spec_oracle as so
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(2, 96, 130, seed=21)
    s = sr.grid(96, 130, 300)[0]
    got = Segmenter(n_superpixels=300, n_regions=6, n_iter=4, min_region_size=s * s // 4, **COLOUR).segment_batch(imgs)
    conn = Segmenter(n_superpixels=300, n_regions=6, n_iter=4, connectivity=True, **COLOUR).segment_batch(imgs)
    for i, im in enumerate(imgs):
        ref = _ref_cut(("post", i), im, 300, 6, 4, **COLOUR_REF)
        assert np.array_equal(got[i], merge_small_regions(ref, s * s // 4)), i
        assert np.array_equal(conn[i], so.connected_regions(ref)), i


def test_every_host_path_and_graph_replay(torch_cuda):
    """segment (graph replay, called twice) == the segment_batch row == segment_device; segment_images with mixed shapes,
    segment_stream, uint8 output with K > 256."""
    import gabor_color_image_segmentation_amd as pkg
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.segmenter import DebugSwitches
    kw = dict(n_superpixels=64, spatial_weight=144, n_iter=4, n_regions=5)
    a, b = _synth(3, 72, 104, seed=1), _synth(2, 104, 72, seed=2)
    ref_a = np.stack([_ref_cut(("host", "a", i), im, 64, 5, 4, lam=144) for i, im in enumerate(a)])
    ref_b = np.stack([_ref_cut(("host", "b", i), im, 64, 5, 4, lam=144) for i, im in enumerate(b)])
    seg = Segmenter(**kw)
    assert np.array_equal(seg(a[0]), ref_a[0]) and np.array_equal(seg(a[1]), ref_a[1]) and np.array_equal(seg(a[0]), ref_a[0])
    assert any(e["graph"] is not None and e["rt"] is not None for e in seg._graphs.values())      # the small call was captured
    assert np.array_equal(pkg.segment(a[1], **kw), ref_a[1]) and np.array_equal(pkg.segment(a[2], **kw), ref_a[2])
    first = seg.segment_batch(a)
    assert first.dtype == np.int32 and np.array_equal(first, ref_a)
    assert np.array_equal(seg.segment_batch(a[::-1].copy()), ref_a[::-1])         # the replay follows the new input
    assert np.array_equal(seg.segment_device(torch_cuda.from_numpy(a).cuda()).cpu().numpy(), ref_a)
    eager = Segmenter(**kw)
    eager.debug = DebugSwitches("no_graph")
    assert np.array_equal(eager.segment_batch(a), ref_a) and not eager._graphs
    mixed = [a[0], b[0], a[1], b[1], a[2]]
    for g, want in zip(seg.segment_images(mixed, batch=2), [ref_a[0], ref_b[0], ref_a[1], ref_b[1], ref_a[2]]):
        assert np.array_equal(g, want)
    got = list(pkg.segment_images(mixed, batch=3, **kw))
    assert np.array_equal(got[3], ref_b[1])
    outs = list(seg.segment_stream([a, a[::-1].copy()]))
    assert len(outs) == 2 and np.array_equal(outs[0], ref_a) and np.array_equal(outs[1], ref_a[::-1])
    assert np.array_equal(pkg.segment_batch(a, **kw), ref_a)
    # uint8 with K = 294 > 256 and R = 8 (captured, then replayed)
    many = Segmenter(n_superpixels=300, n_regions=8, n_iter=4)
    assert sr.grid(72, 104, 300)[1] * sr.grid(72, 104, 300)[2] > 256
    want = np.stack([_ref_cut(("host", "u8", i), im, 300, 8, 4) for i, im in enumerate(a)])
    for _ in range(2):
        u8 = many.segment_batch(a, out_dtype=np.uint8)
        assert u8.dtype == np.uint8 and np.array_equal(u8, want)
    with pytest.raises(ValueError):
        Segmenter(n_superpixels=300, n_regions=257).segment_batch(a, out_dtype=np.uint8)


def test_one_tree_many_cuts(torch_cuda):
    """region_tree_device + cut_regions_device at R = 2, 8, 32 == three plans Segmenter(n_regions=R)."""
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(3, 96, 130, seed=8)
    dev = torch_cuda.from_numpy(imgs).cuda()
    kw = dict(n_superpixels=120, n_iter=4, **COLOUR)
    tree = Segmenter(**kw)
    lab, merges, costs, alive = tree.region_tree_device(dev)
    keep = lab.clone()
    for i, im in enumerate(imgs):
        want = _ref(("cuts", i), im, 120, 4, **COLOUR_REF)
        assert np.array_equal(lab[i].cpu().numpy(), want[0]) and np.array_equal(merges[i].cpu().numpy(), want[1])
        assert int(alive[i]) == want[2]
    for r in (2, 8, 32):
        cut = tree.cut_regions_device(lab, merges, alive, r)
        assert torch_cuda.equal(cut, Segmenter(n_regions=r, **kw).segment_device(dev)), r
        for i, im in enumerate(imgs):
            assert np.array_equal(cut[i].cpu().numpy(), _ref_cut(("cuts", i), im, 120, r, 4, **COLOUR_REF)), (r, i)
    assert torch_cuda.equal(lab, keep)                    # a cut goes into a fresh tensor


def test_n_regions_zero_is_the_plan_without_the_argument(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    small, big = _synth(2, 72, 104, seed=3), _synth(8, 321, 481, seed=4)
    for kw in (dict(n_iter=4), dict(n_superpixels=64, n_iter=4)):
        off, plain = Segmenter(n_regions=0, **kw), Segmenter(**kw)
        for imgs in (small, big):
            assert np.array_equal(off.segment_batch(imgs), plain.segment_batch(imgs))
            dev = torch.from_numpy(imgs).cuda()
            assert torch.equal(off.segment_device(dev), plain.segment_device(dev))
        assert all(e.get("rt") is None for e in off._graphs.values())
    assert np.array_equal(off.segment_batch(small)[0], sr.segment(small[0], 64, n_iter=4))          # (the §13 map as it is)
    with pytest.raises(ValueError):
        Segmenter(n_regions=8)


def test_quality_of_six_val_images_through_the_gpu(torch_cuda):
    """The first six val images at the table's setting (colour bank, n = 300, lambda = 576, 10 passes, R = 8, raw and with
    min_region_size = S^2 / 4) through Segmenter and the batched GPU scorer against the per-image numbers of
    tools/region_tree_quality.py (CPU restatements, ``evaluate.metrics``): ``==`` where the GPU scorer and the host mirror run the
    same float operations (recall, precision, F, density, regions), 1e-12 for underseg, undersegNP, compactness, PRI, VoI and
    covering, whose sums the scorer takes in another order (as tests/test_gpu_superpixels.py holds its scores)."""
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    doc = json.load(open(os.path.join(HERE, "..", "profiles", "region_tree_quality.json")))
    sp = doc["superpixels"]
    assert (sp["n_superpixels"], sp["n_orient"], doc["per_image_n_regions"]) == (300, 5, 8)
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    ids = doc["ids"][:6]
    for state, post in (("raw", {}), ("merged", dict(min_region_size=sr.grid(321, 481, 300)[0] ** 2 // 4))):
        seg = Segmenter(n_superpixels=300, spatial_weight=sp["spatial_weight"], n_regions=8, **COLOUR, **post)
        labs = dict(zip(ids, seg.segment_images([val["img_" + i] for i in ids], batch=8)))
        rows = {}
        for shape in ((321, 481), (481, 321)):
            group = [i for i in ids if val["img_" + i].shape[:2] == shape]
            if group:
                scores = all_scores_batch_device(torch.from_numpy(np.stack([labs[i] for i in group])).cuda(), pt.to_device(group),
                                                 agreement=True)
                rows.update(zip(group, scores))
        for i in ids:
            want, got = doc["per_image"][state][i], rows[i]
            print(state, i, {k: got[k] for k in ("recall", "fmeasure", "PRI", "VoI", "covering", "regions")})
            for key in ("recall", "precision", "fmeasure", "density", "regions"):
                assert got[key] == want[key], (state, i, key, got[key], want[key])
            for key in ("underseg", "undersegNP", "compactness", "PRI", "VoI", "covering"):
                assert abs(got[key] - want[key]) <= 1e-12, (state, i, key, got[key], want[key])


# ---- the statistics kernel's 32-slot table at its threshold

def _bucket(l):
    """The slot a label's probe starts at in rt_stats_kernel's table (restated as a witness: the expected values do not use it)."""
    return ((int(l) * 2654435761) % 2 ** 32) >> 27


def _columns(labels):
    """An 8 x len(labels) block: every label an 8 x 1 column."""
    return np.broadcast_to(np.asarray(labels, np.int32), (8, len(labels))).copy()


def _threshold_map(bucket, k=4096):
    """16 x 64, four 8 x 32 tiles, all their labels from ONE bucket of the table's hash (so every probe walks a chain through the
    whole table): top left exactly 32 labels (the LDS form with every slot taken), top right the same 32 and a 33rd label in one
    pixel (the global form: both forms add into the same 32 rows of sums), bottom left another 32 labels and pixels outside
    0 .. K-1 (-1 and K, among them a whole eight-lane group), bottom right 32 labels of which 16 are the top row's."""
    own = [l for l in range(k) if _bucket(l) == bucket]
    assert 127 <= len(own) <= 130
    lab = np.empty((16, 64), np.int32)
    lab[:8, :32] = _columns(own[:32])
    lab[:8, 32:] = _columns(own[:32][::-1])
    lab[5, 45] = own[32]
    lab[8:, :32] = _columns(own[33:65])
    lab[9, 5], lab[12, 17], lab[15, 31] = -1, k, k
    lab[10, 8:16] = -1
    lab[8:, 32:] = _columns(own[16:32] + own[65:81])
    return lab


@pytest.mark.parametrize("buckets", [(0, 31), (13,)])
def test_stats_table_at_32_labels_and_one_more(torch_cuda, buckets):
    """K = 4096, D = 3: tiles with exactly 32 labels, with 33, and with 32 plus out-of-range pixels (see ``_threshold_map``), one
    image per bucket. The sums stay in the workspace; merges, costs, alive and cuts are functions of them and are compared."""
    k = 4096
    lab = np.stack([_threshold_map(b) for b in buckets])
    for m, b in zip(lab, buckets):
        seen = [np.unique(t[(t >= 0) & (t < k)]) for t in (m[:8, :32], m[:8, 32:], m[8:, :32], m[8:, 32:])]
        assert [len(s) for s in seen] == [32, 33, 32, 32]
        assert all(_bucket(l) == b for s in seen for l in s)
        assert set(seen[0]) <= set(seen[1]) and len(set(seen[0]) & set(seen[3])) == 16
        assert (m[8:, :32] == -1).sum() == 9 and (m[8:, :32] == k).sum() == 2
    x = np.random.default_rng(32).integers(0, 46341, (len(buckets), 3, 16, 64)).astype(np.uint16)
    refs = _check_tree(torch_cuda, x, lab, k, (1, 8, 4096))
    assert all(a == 81 for _, _, a in refs)


# ---- the tile accumulator (csrc/label_tile.h) at its slot boundary, inside one launch

def _stripes(h, w, extra=None):
    """Column stripes x % 32 (32 labels in every full tile row: every slot taken, none missing), ``extra``: one pixel of label 32."""
    lab = np.broadcast_to(np.arange(w, dtype=np.int32) % 32, (h, w)).copy()
    if extra is not None:
        lab[extra] = 32
    return lab


@pytest.mark.parametrize("h,w", [(8, 32), (9, 33)])
def test_stats_tile_with_32_labels_beside_one_with_33(torch_cuda, h, w):
    """B = 2, D = 2: image 0's first tile holds exactly 32 labels (the LDS rows), image 1's the same and a 33rd label in one pixel (the
    global rows), both in one launch; at 9 x 33 the second tiles are ragged in both directions."""
    lab = np.stack([_stripes(h, w), _stripes(h, w, (5, 13))])
    x = np.random.default_rng(h * w).integers(0, 46340, (2, 2, h, w)).astype(np.uint16)
    refs = _check_tree(torch_cuda, x, lab, 33, (1, 33))
    assert [a for _, _, a in refs] == [32, 33]


def test_stats_tile_of_one_label_at_full_range(torch_cuda):
    """8 x 64, D = 2: the left tile is label 0 with every feature at 46339, so every eight-lane sum is 8 * 46339 and both LDS cells reach
    256 * 46339; the right tile is label 1 at 0. The one merge costs 2 * 46339^2 * 256 exactly when label 0's mean is 46339."""
    lab = np.zeros((1, 8, 64), np.int32)
    lab[0, :, 32:] = 1
    x = np.where(lab == 0, 46339, 0).astype(np.uint16)[:, None].repeat(2, axis=1)
    (m, c, a), = _check_tree(torch_cuda, x, lab, 2, (1, 2))
    assert a == 2 and m.tolist() == [[0, 1]] and int(c[0]) == 2 * 46339 ** 2 * 256


# ---- the cut on lists outside the form gcs_region_tree writes: SPEC.md §16's row rule

def test_cut_of_a_list_with_rows_that_do_not_count(torch_cuda):
    """B = 2, 15 x 18, K = 24, alive 24 and 21: the balanced list with a = b, b >= K, an absorbed b, a dead a, (-1, -1) in the middle and
    a label (6) that is the b of two well-formed rows with different a. The cut of the raw list == the restatement's cut of the list
    with those rows cleared, every pixel, out-of-range labels (-1) included, out of place and in place."""
    import contour_map_ref as cm
    import region_props_ref as rp
    torch, k = torch_cuda, 24
    bad = cm.balanced(k).copy()
    bad[1], bad[3], bad[5], bad[7], bad[9] = (4, 4), (2, k), bad[0], (bad[0][1], 23), (-1, -1)
    assert bad[13].tolist() == [4, 6]
    bad[14] = (0, 6)
    clean = rp.counted(bad, k)
    assert (clean[[1, 3, 5, 7, 9, 14]] == -1).all() and (clean >= 0).all(1).sum() == k - 1 - 6
    lab = np.random.default_rng(24).integers(0, k, (2, 15, 18)).astype(np.int32)
    for q in (3, 11, 19):
        lab[1][lab[1] == q] = q + 1
    lab[0, 0, 0], lab[0, 7, 9], lab[1, 14, 17], lab[1, 3, 3] = -1, k, 2 ** 30, -2 ** 31
    alive = [24, 21]
    assert [len(np.unique(l[(l >= 0) & (l < k)])) for l in lab] == alive
    dev = (torch.from_numpy(lab).cuda(), torch.from_numpy(np.stack([bad, bad])).cuda(), torch.tensor(alive, dtype=torch.int32, device="cuda"))
    for r in (24, 12, 6, 3, 1):
        for in_place in (False, True):
            got = _gpu_cut(torch, dev, k, r, in_place=in_place)
            for i in range(2):
                want = rt.cut(lab[i], clean, alive[i], r)
                assert (want[(lab[i] < 0) | (lab[i] >= k)] == -1).all()
                assert np.array_equal(got[i], want), (r, in_place, i, int((got[i] != want).sum()))
    # K = 1: no list (a NULL pointer); label 0 stays 0, everything else is -1
    lab1 = np.zeros((2, 5, 7), np.int32)
    lab1[1, 0, 0], lab1[1, 4, 6] = 3, -1
    dev1 = (torch.from_numpy(lab1).cuda(), None, torch.tensor([1, 1], dtype=torch.int32, device="cuda"))
    for r, in_place in ((1, False), (5, True)):
        got = _gpu_cut(torch, dev1, 1, r, in_place=in_place)
        for i in range(2):
            assert np.array_equal(got[i], rt.cut(lab1[i], np.zeros((0, 2), np.int32), 1, r))
