"""gcs_feature_gradient (SPEC.md §22) on the GPU: every value of the map compared with ``==`` against the NumPy restatement
(tests/feature_gradient_ref.py) applied to the canonical features of the SAME slab (``features_device`` of the same plan, which
other tests hold to the C oracle; for shapes below the Gabor stage's 8 x 8 a slab of random bytes read back through
gcs_features_unpack). Shapes: 1 x 1, 1 x 9, 5 x 9 (nothing packed), 8 x 8, 9 x 10 and 17 x 18 (both strips packed, the corner, the
main block <-> strip neighbours), 13 x 11 (odd: level sizes round up), 33 x 41 (several tiles, a last tile that is not full), three
distinct images at once. Banks: one per slab format and pyramid depth, D = 207 among them; a hot bank for values of 4096 and more
(TOP runs, flagged beside unflagged tiles, the root of a large E); one plan per option; the argument rules; the threshold sweep
against ``evaluate.edge_scores`` on two fixture images; ``segment_regions(gradient=True)``."""
import os

import numpy as np
import pytest

import feature_gradient_ref as fg
import slab_layout

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name -> (n_scales, n_orient): D = 3 n_scales n_orient
BANKS = {"default": (4, 6),        # D = 72: split slab, two levels
         "one_level": (2, 6),      # D = 36: split slab, one level
         "wide2": (4, 7),          # D = 84: wide slab with packed strips
         "three": (6, 4),          # D = 72: three levels, wide, no strips
         "four": (8, 8),           # D = 192: four levels
         "d207": (3, 23)}          # D = 207: the most features the entry point takes
PLAN_SHAPES = [(8, 8), (9, 10), (17, 18), (13, 11), (33, 41)]
RAW_SHAPES = [(1, 1), (1, 9), (5, 9)]


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_PLANS = {}


def _plan(bank, **kw):
    key = (bank, tuple(sorted(kw.items())))
    if key not in _PLANS:
        from gabor_color_image_segmentation_amd import Segmenter
        _PLANS[key] = Segmenter(n_scales=BANKS[bank][0], n_orient=BANKS[bank][1], **kw)
    return _PLANS[key]


def _restated(canon, seg):
    """(B, D, H, W) int16 device tensor of ``features_device`` -> the maps of the restatement, (B, H, W) int32."""
    x = canon.cpu().numpy().view(np.uint16)
    return np.stack([fg.gradient(x[i], seg.bank.n_scales, seg.bank.n_orient) for i in range(x.shape[0])])


def _check_plan(torch, seg, imgs):
    dev = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    want = _restated(seg.features_device(dev), seg)
    got = seg.edges_device(dev)
    assert got.dtype == torch.int32 and tuple(got.shape) == imgs.shape[:3]
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (imgs.shape, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return want


@pytest.mark.parametrize("shape", PLAN_SHAPES)
@pytest.mark.parametrize("bank", list(BANKS))
def test_every_bank_and_shape(torch_cuda, bank, shape):
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    h, w = shape
    want = _check_plan(torch_cuda, _plan(bank), synthetic_batch(1, h, w, seed=h * w))
    assert want.max() > 0


@pytest.mark.parametrize("bank", ["default", "wide2", "four"])
def test_three_distinct_images(torch_cuda, bank):
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = synthetic_batch(3, 17, 18, seed=7)
    imgs[1] = imgs[1, ::-1, ::-1]
    want = _check_plan(torch_cuda, _plan(bank), imgs)
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[0], want[2])


@pytest.mark.parametrize("shape", RAW_SHAPES + [(9, 10)])
@pytest.mark.parametrize("bank", list(BANKS))
def test_slabs_of_random_bytes(torch_cuda, bank, shape):
    """Below 8 x 8 the Gabor stage takes no image, the entry point does: two slabs of random bytes (every 16-bit value; the flag
    bytes of a split slab set, so that its TOP nibbles count, as gcs_features_unpack counts them), their canonical tensors through
    gcs_features_unpack. 9 x 10: the same with packed strips."""
    torch = torch_cuda
    seg = _plan(bank)
    ops, lib = seg.ops, seg.ops.lib
    ns, no = BANKS[bank]
    b, (h, w) = 2, shape
    per = lib.gcs_feature_slab_bytes(1, h, w, ns, no)
    ntiles, tile_bytes, split = slab_layout.tile_geometry(lib, h, w, ns, no)
    raw = np.random.default_rng(h * 100 + w).integers(0, 256, size=(b, per), dtype=np.uint8)
    if split:
        raw[:, ntiles * tile_bytes:ntiles * tile_bytes + 4 * ntiles] = 1
    slab = torch.from_numpy(raw.reshape(-1)).cuda()
    canon = ops.features_unpack(slab, b, h, w)
    assert int(canon.cpu().numpy().view(np.uint16).max()) > 46340         # beyond what the Gabor stage writes: any 16 bits are taken
    out = torch.full((b, h, w), -7, dtype=torch.int32, device="cuda")
    ops.feature_gradient(slab, b, h, w, out)
    want = _restated(canon, seg)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (bank, shape, np.argwhere(got != want)[:4].tolist())
    if shape == (1, 1):
        assert not got.any()


def test_hot_bank_values_above_4096(torch_cuda):
    """Eight hot images on a hot 4 x 6 bank: values up to 46339, ``black_region`` with flagged and unflagged tiles side by side."""
    import hot_banks as hb
    torch = torch_cuda
    seg = hb.hot_segmenter(hb.hot_bank(4, 6, 13, 8))
    imgs = hb.hot_images(8, 24, 40, 5)
    dev = torch.from_numpy(imgs).cuda()
    canon = seg.features_device(dev).cpu().numpy().view(np.uint16)
    assert canon.max() > 32768
    b, h, w = 8, 24, 40
    feats = seg.ops.feature_slab(b, h, w)
    seg.ops.gabor_features(dev, feats)
    flags, _ = slab_layout.flag_bytes(seg, feats, b, h, w)
    black = flags[hb.BLACK_REGION][:, :2]
    assert black.any() and not black.all()                   # tiles with and without TOP nibbles in one image
    want = _check_plan(torch, seg, imgs)
    assert int(want.max()) ** 2 > 2 ** 32                    # E past 32 bits: the 64-bit sums and the corrected root


@pytest.mark.parametrize("kw", [dict(smoothing=1.0), dict(color_weight=0.125, chroma_gain=4), dict(position_weight=6)],
                         ids=["smoothing", "colour", "position"])
def test_options_shape_the_map(torch_cuda, kw):
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = synthetic_batch(2, 33, 41, seed=3)
    seg = Segmenter(n_orient=5 if "color_weight" in kw or "position_weight" in kw else 6, **kw)
    assert seg.bank.n_features == 72
    want = _check_plan(torch_cuda, seg, imgs)
    plain = _check_plan(torch_cuda, _plan("default"), imgs)
    assert not np.array_equal(want, plain)
    if "position_weight" in kw:                              # the coordinate slot adds a constant: mu^2 per step, both axes, two scales a level
        x0 = seg.features_device(torch_cuda.from_numpy(imgs).cuda()).cpu().numpy().view(np.uint16).astype(np.int64)
        f_n = 4 * seg.bank.n_orient
        slot = [c * f_n + s * seg.bank.n_orient + seg.bank.n_orient - 1 for c in range(3) for s in range(4)]
        x1 = x0.copy()
        x1[:, slot] = 0
        diff = fg.energy(x0[0], 4, seg.bank.n_orient) - fg.energy(x1[0], 4, seg.bank.n_orient)
        assert len(np.unique(diff[4:-5, 4:-5])) == 1 and diff[8, 8] == 2 * 2 * (2 * 6) ** 2 + 2 * 2 * ((4 * 6) ** 2 >> 2)


def test_bad_arguments_launch_nothing(torch_cuda):
    torch = torch_cuda
    seg = _plan("default")
    lib = seg.ops.lib
    b, h, w = 1, 16, 24
    feats = seg.ops.feature_slab(b, h, w)
    feats.zero_()
    out = torch.full((b, h, w), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    good = [feats.data_ptr(), b, h, w, 4, 6, out.data_ptr(), st]
    for pos, val in ((0, None), (6, None), (1, 0), (1, 65536), (2, 0), (2, 4097), (3, 0), (3, 4097), (4, 0), (4, 9), (5, 0),
                     (5, 18)):                               # (4 scales x 18 slots = 216 features > 207)
        args = list(good)
        args[pos] = val
        assert lib.gcs_feature_gradient(*args) == 1, (pos, val)
        assert b"gcs_feature_gradient" in lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    assert bool((out == -7).all())                           # nothing was launched
    assert lib.gcs_feature_gradient(*good) == 0
    torch.cuda.current_stream().synchronize()
    assert not bool(out.any())                               # a slab of zero bytes: every value is 0x8080 ^ 0x8080 ... constant
    with pytest.raises(ValueError):
        seg.ops.feature_gradient(feats, b, h, w, out.to(torch.int64))
    with pytest.raises(ValueError, match="row strips"):
        seg.edges_device(torch.zeros((1, 16, 24, 3), dtype=torch.uint8, device="cuda"), y0=8)


@pytest.mark.parametrize("shape", [(321, 481), (481, 321)])
def test_sweep_equals_edge_scores_at_every_level(torch_cuda, shape):
    """A val fixture image of either orientation with its real annotator maps: recall, precision and F of every level, ``==``."""
    from gabor_color_image_segmentation_amd.evaluate import edge_scores
    from gabor_color_image_segmentation_amd.evaluate_gpu import edge_sweep_resident
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    torch = torch_cuda
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    i = [str(i) for i in val["ids"] if val["img_" + str(i)].shape[:2] == shape][0]
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    dt = truth.to_device([i])
    g = _plan("default").edges_device(torch.from_numpy(val["img_" + i][None]).cuda())
    levels = 256
    rec, prec, f, step = edge_sweep_resident(g, dt, levels=levels)
    gh = g[0].cpu().numpy()
    assert step == -(-(int(gh.max()) + 1) // levels) and rec.shape == (1, levels)
    want = edge_scores(gh, truth[i], [step * (tau + 1) - 1 for tau in range(levels)])
    assert rec[0].tolist() == want["recall"].tolist() and prec[0].tolist() == want["precision"].tolist()
    assert f[0].tolist() == want["fmeasure"].tolist() and 0.2 < f.max() < 1.0
    # a step of the caller's: the levels above the map's largest value hold the zero rule
    rec2, prec2, f2, step2 = edge_sweep_resident(g, dt, levels=16, step=int(gh.max()) // 8 + 1)
    want2 = edge_scores(gh, truth[i], [step2 * (tau + 1) - 1 for tau in range(16)])
    assert f2[0].tolist() == want2["fmeasure"].tolist() and rec2[0].tolist() == want2["recall"].tolist()
    assert not f2[0, 8:].any() and f2[0, 0] > 0


def test_segment_regions_with_the_gradient_as_strength(torch_cuda):
    import gabor_color_image_segmentation_amd as pkg
    import region_adjacency_ref as ra
    from gabor_color_image_segmentation_amd.segmenter import _plan as pkg_plan
    torch = torch_cuda
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    img = val["img_" + str(val["ids"][0])]
    kw = dict(n_iter=4, k=6)
    labels0, table0 = pkg.segment_regions(img, adjacency=True, **kw)
    labels, table = pkg.segment_regions(img, adjacency=True, gradient=True, **kw)
    assert np.array_equal(labels, labels0)
    seg = pkg_plan(dict(kw))
    dev = torch.from_numpy(img[None]).cuda()
    plane = _restated(seg.features_device(dev), seg)[0]
    k = int(labels.max()) + 1
    we, wv = ra.leaf_graph(labels, k, img, plane)
    adj = table["adjacency"]
    assert np.array_equal(adj["pairs"], we) and np.array_equal(adj["length"], wv[:, 0].astype(np.int64))
    assert np.array_equal(adj["mean_strength"], wv[:, 2].astype(np.float64) / (2.0 * wv[:, 0].astype(np.float64)))
    assert adj["mean_strength"].min() > 0 and not table0["adjacency"]["mean_strength"].any()
    for key in table0:                                        # gradient=False is what it was
        if key != "adjacency":
            assert table[key].tobytes() == table0[key].tobytes(), key
    for key in ("pairs", "length", "mean_contrast", "degree"):
        assert np.array_equal(adj[key], table0["adjacency"][key]), key
    e = pkg.segment_edges(img, **kw)
    assert e.dtype == np.float32 and np.array_equal(e, fg.normalised(plane)) and e.max() == 1.0
