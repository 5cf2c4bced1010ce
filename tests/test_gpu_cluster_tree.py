"""Segmenter(tree_nodes="clusters") (SPEC.md §21) on the GPU against tests/cluster_tree_ref.py, bit for bit and never against the
GPU's own output: every host path on 37 x 53 and 72 x 104 (default bank) and on one val fixture image per orientation (colour bank,
k = 16) at R in {1, 2, 8, 300}, the trimmed tree of region_tree_device against the tree at K_cap from the unpacked tensor, cuts,
contour map and the sweep of every cut against what the plan delivers, the default plan's labels, and the argument rules."""
import json
import os

import numpy as np
import pytest
from scipy import ndimage

import cluster_tree_ref as cl
import position_ref as pr
import region_tree_ref as rt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
COLOUR_REF = dict(w=0.125, g=4, n_orient=5)
RS = (1, 2, 8, 300)
# case -> (plan options, restatement options)
CASES = {"odd": (dict(k=16, n_iter=3), dict(k=16, n_iter=3)),
         "synth": (dict(k=16, n_iter=3), dict(k=16, n_iter=3)),
         "bsd_landscape": (dict(k=16, n_iter=10, **COLOUR), dict(k=16, n_iter=10, **COLOUR_REF)),
         "bsd_portrait": (dict(k=16, n_iter=10, **COLOUR), dict(k=16, n_iter=10, **COLOUR_REF))}


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_IMGS, _REFS = {}, {}


def _images(case):
    """"odd": two synthetic 37 x 53 images; "synth": two of 72 x 104; "bsd_*": the val fixture image of that orientation with the
    fewest nodes in profiles/cluster_tree_quality.json (the plain-Python tree takes a second per thousand nodes and round)."""
    if case not in _IMGS:
        from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
        if case == "odd":
            _IMGS[case] = synthetic_batch(2, 37, 53, seed=21)
        elif case == "synth":
            _IMGS[case] = synthetic_batch(2, 72, 104, seed=3)
        else:
            val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
            trees = json.load(open(os.path.join(HERE, "..", "profiles", "cluster_tree_quality.json")))["tree"]["colour_k16"]
            shape = (321, 481) if case == "bsd_landscape" else (481, 321)
            i = min((i for i in trees if val["img_" + i].shape[:2] == shape), key=lambda i: trees[i]["nodes"])
            _IMGS[case] = val["img_" + i][None].copy()
    return _IMGS[case]


def _ref(case, i, m=0):
    """(features, k-means map, node map, merges, costs, alive, info) of the restatement for image ``i`` of a case, computed once."""
    key = (case, i, m)
    if key not in _REFS:
        kw = dict(CASES[case][1])
        k, n_iter = kw.pop("k"), kw.pop("n_iter")
        x = pr.features(_images(case)[i], **kw)
        lab = cl.kmeans_maps(x[None], k, n_iter)[0]
        info = {}
        _REFS[key] = (x, lab) + cl.tree(x, lab, m, info=info) + (info,)
    return _REFS[key]


def _want(case, r, m=0):
    out = []
    for i in range(len(_images(case))):
        _, _, n_map, merges, _, alive, _ = _ref(case, i, m)
        out.append(rt.cut(n_map, merges, alive, r) if r else n_map)
    return np.stack(out)


def _plan(case, **kw):
    from gabor_color_image_segmentation_amd import Segmenter
    return Segmenter(tree_nodes="clusters", **CASES[case][0], **kw)


@pytest.mark.parametrize("case", list(CASES))
def test_every_host_path_equals_the_restatement(torch_cuda, case):
    import gabor_color_image_segmentation_amd as pkg
    imgs = _images(case)
    dev = torch_cuda.from_numpy(imgs).cuda()
    for r in RS:
        want = _want(case, r)
        for i in range(len(imgs)):                       # exactly min(nodes, R) labels, each 4-connected
            nodes = _ref(case, i)[6]["nodes"]
            assert len(np.unique(want[i])) == min(nodes, r) == want[i].max() + 1
            assert all(ndimage.label(want[i] == v)[1] == 1 for v in range(min(nodes, r)))
        seg = _plan(case, n_regions=r)
        first = seg(imgs[0])                             # segment: the small call is captured, then replayed
        assert first.dtype == np.int32 and np.array_equal(first, want[0]), (r, int((first != want[0]).sum()))
        assert np.array_equal(seg(imgs[0]), want[0])
        assert any(e["graph"] is not None and e["rt"] is not None and "nd" in e["ws"] and "sp" not in e["ws"]
                   for e in seg._graphs.values())
        assert np.array_equal(seg.segment_batch(imgs), want) and np.array_equal(seg.segment_batch(imgs[::-1].copy()), want[::-1])
        for got, w in zip(seg.segment_images(list(imgs), batch=2), want):
            assert np.array_equal(got, w)
        outs = list(seg.segment_stream([imgs, imgs[::-1].copy()]))
        assert len(outs) == 2 and np.array_equal(outs[0], want) and np.array_equal(outs[1], want[::-1])
        assert np.array_equal(seg.segment_device(dev).cpu().numpy(), want)
    kw = dict(tree_nodes="clusters", n_regions=8, **CASES[case][0])
    want = _want(case, 8)
    for _ in range(2):                                   # uint8 (captured, then replayed), and through the stream's uint8 buffers
        u8 = pkg.segment_batch(imgs, out_dtype=np.uint8, **kw)
        assert u8.dtype == np.uint8 and np.array_equal(u8, want)
    u8 = list(_plan(case, n_regions=8).segment_stream([imgs], out_dtype=np.uint8))[0]
    assert u8.dtype == np.uint8 and np.array_equal(u8, want)
    assert np.array_equal(pkg.segment(imgs[0], **kw), want[0])
    assert np.array_equal(np.stack(list(pkg.segment_images(list(imgs), batch=3, **kw))), want)


def test_large_batches_take_the_chunked_and_the_pipelined_path(torch_cuda):
    """More than 2^20 pixels (144 images of 72 x 104): segment_batch uploads in chunks, segment_stream runs the three-stream
    pipeline; int32, and uint8 narrowed from the int32 map the workspace keeps."""
    imgs = np.concatenate([_images("synth")] * 72)
    assert imgs.shape[0] * 72 * 104 > 1 << 20
    want = np.concatenate([_want("synth", 8)] * 72)
    seg = _plan("synth", n_regions=8)
    assert seg._host_path(len(imgs), 72, 104, "per_image") == "chunked"
    assert np.array_equal(seg.segment_batch(imgs), want)
    u8 = seg.segment_batch(imgs, out_dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, want)
    outs = list(seg.segment_stream([imgs, imgs], out_dtype=np.uint8))
    assert len(outs) == 2 and all(o.dtype == np.uint8 and np.array_equal(o, want) for o in outs)
    outs = list(seg.segment_stream([imgs, imgs]))
    assert len(outs) == 2 and all(o.dtype == np.int32 and np.array_equal(o, want) for o in outs)


def test_min_region_size_global_mode_and_the_node_map(torch_cuda):
    """m = 5 joins the node map; connectivity=True changes nothing; n_regions = 0 delivers the node map; one rank's global codebook."""
    imgs = _images("odd")
    dev = torch_cuda.from_numpy(imgs).cuda()
    assert any(_ref("odd", i, 5)[6]["nodes"] < _ref("odd", i)[6]["nodes"] for i in range(2))
    for r in (2, 8):
        want = _want("odd", r, 5)
        assert np.array_equal(_plan("odd", n_regions=r, min_region_size=5).segment_device(dev).cpu().numpy(), want)
        assert np.array_equal(_plan("odd", n_regions=r, min_region_size=5, connectivity=True).segment_batch(imgs), want)
        assert np.array_equal(_plan("odd", n_regions=r, min_region_size=5).segment_batch(imgs, out_dtype=np.uint8), want)
    for m in (0, 5):
        nodes = _want("odd", 0, m)
        assert np.array_equal(_plan("odd", min_region_size=m).segment_device(dev).cpu().numpy(), nodes)
        assert np.array_equal(_plan("odd", min_region_size=m).segment_batch(imgs), nodes)
    want = cl.segment_batch(imgs, 4, mode="global", **CASES["odd"][1])
    assert np.array_equal(_plan("odd", n_regions=4).segment_batch(imgs, mode="global"), want)
    assert np.array_equal(_plan("odd", n_regions=4).segment_device(dev, mode="global").cpu().numpy(), want)


def test_the_default_plan_is_unchanged(torch_cuda):
    """Without the option: the k-means map of SPEC.md §4, as the oracle gives it, on every case's bank."""
    from gabor_color_image_segmentation_amd import Segmenter
    for case in ("odd", "bsd_landscape"):
        imgs = _images(case)
        want = np.stack([_ref(case, i)[1] for i in range(len(imgs))])
        seg = Segmenter(**CASES[case][0])
        assert np.array_equal(seg.segment_batch(imgs), want)
        assert np.array_equal(seg.segment_device(torch_cuda.from_numpy(imgs).cuda()).cpu().numpy(), want)
        assert np.array_equal(Segmenter(tree_nodes="superpixels", **CASES[case][0]).segment_batch(imgs), want)


@pytest.mark.parametrize("case", ["odd", "bsd_portrait"])
def test_trimmed_tree_cuts_and_contours(torch_cuda, case):
    torch = torch_cuda
    imgs = _images(case)
    dev = torch.from_numpy(imgs).cuda()
    seg = _plan(case)
    n_map, merges, costs, alive = seg.region_tree_device(dev)
    b, h, w = n_map.shape
    counts = [_ref(case, i)[6]["nodes"] for i in range(b)]
    K = merges.shape[1] + 1
    assert K == min(4096, -(-max(counts) // 64) * 64) and alive.tolist() == counts and tuple(costs.shape) == (b, K - 1)
    for i in range(b):                                   # the restatement, at capacity = node count
        _, _, want_map, want_merges, want_costs, want_alive, _ = _ref(case, i)
        assert np.array_equal(n_map[i].cpu().numpy(), want_map)
        got_m, got_c = merges[i].cpu().numpy(), costs[i].cpu().numpy().view(np.uint64)
        assert np.array_equal(got_m[:want_alive - 1], want_merges) and (got_m[want_alive - 1:] == -1).all()
        assert np.array_equal(got_c[:want_alive - 1], want_costs) and not got_c[want_alive - 1:].any()
    # the tree at K_cap from the UNPACKED tensor of the same features, on the same nodes: its first rows
    ops = seg.ops
    canon = seg.features_device(dev)
    ws, big_m, big_c, big_a = ops.region_tree_buffers(b, h, w, 4096)
    ops.region_tree(canon, n_map, b, h, w, 4096, ws, big_m, big_c, big_a)
    assert torch.equal(big_a, alive) and torch.equal(big_m[:, :K - 1], merges) and torch.equal(big_c[:, :K - 1], costs)
    assert bool((big_m[:, K - 1:] == -1).all()) and not bool(big_c[:, K - 1:].any())
    contours = seg.contour_map_device(n_map, merges, alive)
    both, al = seg.contours_device(dev)
    assert torch.equal(both, contours) and torch.equal(al, alive)
    for r in RS:
        delivered = _plan(case, n_regions=r).segment_device(dev)
        assert torch.equal(seg.cut_regions_device(n_map, merges, alive, r), delivered), r
        d = delivered
        bd = torch.zeros_like(d, dtype=torch.bool)       # find_boundaries (thick) of the delivered map
        e = d[:, :, 1:] != d[:, :, :-1]
        bd[:, :, 1:] |= e
        bd[:, :, :-1] |= e
        e = d[:, 1:, :] != d[:, :-1, :]
        bd[:, 1:, :] |= e
        bd[:, :-1, :] |= e
        assert torch.equal(contours > (alive - r).clamp(min=0)[:, None, None], bd), r


def _truth(counts, shape, seed):
    """Ragged synthetic annotator maps (as tests/test_gpu_contour_map.py makes them) -> DeviceTruth."""
    from gabor_color_image_segmentation_amd.evaluate_gpu import DeviceTruth
    rng = np.random.default_rng(seed)
    flat = []
    for n in counts:
        for _ in range(n):
            t = np.zeros(shape, np.uint16)
            t[rng.integers(2, shape[0] - 2):, :] += 1
            t[:, rng.integers(2, shape[1] - 2):] += 2
            t[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = 9
            flat.append(t)
    flat = np.stack(flat)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    img_of = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    return DeviceTruth(flat, first, img_of, [int(t.max()) + 1 for t in flat])


@pytest.mark.parametrize("case", ["odd", "bsd_landscape"])
def test_the_sweep_scores_the_delivered_maps(torch_cuda, case):
    """metrics_sweep_resident on the tree of the nodes == the per-cut scorer on what Segmenter(n_regions=R) delivers: the same keys,
    ``==`` where both run the same float operations, and the bounds tests/test_gpu_cut_metrics.py holds for compactness (1e-15
    relative), VoI and covering (1e-12), whose sums the two take in another order."""
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_resident, metrics_sweep_resident
    imgs = _images(case)
    dev = torch_cuda.from_numpy(imgs).cuda()
    seg = _plan(case)
    n_map, merges, _, alive = seg.region_tree_device(dev)
    contours = seg.contour_map_device(n_map, merges, alive)
    dt = _truth([3, 2][:len(imgs)], imgs.shape[1:3], seed=4)
    regions = [2, 8, 32]
    got = metrics_sweep_resident(n_map, merges, alive, contours, dt, regions, agreement=True)
    for j, r in enumerate(regions):
        ref = all_scores_batch_resident(_plan(case, n_regions=r).segment_device(dev), dt, agreement=True)
        for i in range(len(imgs)):
            assert sorted(got[i][j]) == sorted(ref[i])
            for key in ("regions", "underseg", "undersegNP", "density", "recall", "precision", "fmeasure", "PRI"):
                assert got[i][j][key] == ref[i][key], (i, r, key, got[i][j][key], ref[i][key])
            assert abs(got[i][j]["compactness"] - ref[i]["compactness"]) <= 1e-15 * max(1.0, abs(ref[i]["compactness"])), (i, r)
            for key in ("VoI", "covering"):
                assert abs(got[i][j][key] - ref[i][key]) <= 1e-12, (i, r, key, got[i][j][key], ref[i][key])
            assert ref[i]["regions"] == min(r, int(alive[i]))


def test_argument_rules_and_the_module_level_calls(torch_cuda):
    import gabor_color_image_segmentation_amd as pkg
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _images("odd")
    for bad in (dict(tree_nodes="clusters", n_superpixels=64), dict(tree_nodes="clusters", n_superpixels=64, n_regions=4),
                dict(n_regions=4), dict(tree_nodes="components"), dict(tree_nodes="nodes"), dict(tree_nodes=None)):
        with pytest.raises(ValueError):
            Segmenter(**bad)
        with pytest.raises(ValueError):
            pkg.segment(imgs[0], **bad)
    for kw in (dict(), dict(n_regions=257), dict(min_region_size=5)):               # uint8: only with 1 <= R <= 256
        seg = _plan("odd", **kw)
        with pytest.raises(ValueError):
            seg.segment_batch(imgs, out_dtype=np.uint8)
        with pytest.raises(ValueError):
            list(seg.segment_stream([imgs], out_dtype=np.uint8))
        assert not seg._graphs and not seg._ws                                      # nothing was built, nothing launched
    seg = _plan("odd", n_regions=4)
    for call in (lambda: seg.segment_device(torch_cuda.from_numpy(imgs).cuda(), dist_group=object()),
                 lambda: seg.segment_rows_sharded_device(torch_cuda.from_numpy(imgs).cuda(), 0, 37, 0, 37),
                 lambda: seg.segment_batch(np.zeros((1, 4100, 16, 3), np.uint8))):
        with pytest.raises(ValueError):
            call()
    assert not seg._graphs and not seg._ws
    kw = dict(tree_nodes="clusters", **CASES["odd"][0])
    c = pkg.segment_contours(imgs[0], **kw)
    assert c.shape == (37, 53) and c.dtype == np.float32 and 0.0 < c.max() <= 1.0
    labels, table = pkg.segment_regions(imgs[0], n_regions=8, **kw)
    assert np.array_equal(labels, _want("odd", 8)[0]) and len(table["area"]) == 8
    assert [int(a) for a in table["area"]] == np.bincount(labels.ravel()).tolist()
