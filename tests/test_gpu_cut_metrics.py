"""GPU region and shape metrics of every cut of the region tree (SPEC.md §17): gcs_region_sweep_under and gcs_cut_shapes against the
restatement (tests/cut_metrics_ref.py), every integer ``==``; the agreement outputs of gcs_region_sweep_under against gcs_region_sweep,
bit for bit; the library's own trees on the BSD fixtures against the per-cut scorer under the tolerances of tests/test_gpu_scoring.py
(regions, underseg, undersegNP and density ``==``, compactness within 1e-15 max(1, |ref|)); the existing paths before and after.
Workspace and outputs start out as 0xAB bytes."""
import os

import numpy as np
import pytest

import contour_map_ref as cm
import cut_metrics_ref as cr
import region_sweep_ref as rs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _ab(torch, nbytes):
    return torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")


def _leaf_tables(torch, lib, ls, groups, k):
    """-> (hist on the device, img_of on the device, T, stride): gcs_region_counts_batch_u8 when every annotator label fits a byte."""
    b, h, w = ls.shape
    flat = np.stack([g for group in groups for g in group]).astype(np.uint16)
    counts = [len(group) for group in groups]
    first = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
    img_of = torch.from_numpy(np.repeat(np.arange(b), counts).astype(np.int32)).cuda()
    t, stride = len(flat), int(flat.max()) + 1
    u8 = stride <= 256
    maps = torch.from_numpy(flat.astype(np.uint8) if u8 else flat.view(np.int16)).cuda()
    hist = torch.full((t * k * stride,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")         # the counts call zeroes it itself
    side = torch.empty(2 * b * k, dtype=torch.int32, device="cuda")
    fn = lib.gcs_region_counts_batch_u8 if u8 else lib.gcs_region_counts_batch
    rc = fn(ls.data_ptr(), maps.data_ptr(), first.data_ptr(), b, t, max(counts), h, w, k, stride, hist.data_ptr(), side.data_ptr(),
            side.data_ptr() + 4 * b * k, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    return hist, img_of, t, stride


def _gpu_calls(torch, lab, us, merges, alive, groups, regions, k, agreement=False):
    """The raw calls on a batch: lab, us (B, H, W); merges (B, k - 1, 2) or None (k = 1: a NULL pointer); alive (B,); groups: per image
    its annotator maps; regions strictly decreasing -> dict(under [n][T][3], area / perim [n][B][k], boundary [n][B], stride, and with
    ``agreement`` sums / terms [n][T][4])."""
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    ls, cs, al, rg = dev(lab), dev(us), dev(np.asarray(alive).reshape(-1)), dev(regions)
    b, h, w = ls.shape
    ms = None if merges is None else dev(np.asarray(merges).reshape(b, k - 1, 2))
    mp = None if ms is None else ms.data_ptr()
    n = len(regions)
    stream = torch.cuda.current_stream().cuda_stream
    hist, img_of, t, stride = _leaf_tables(torch, lib, ls, groups, k)
    need = lib.gcs_region_sweep_under_workspace_bytes(t, k, stride, n)
    assert need > 0
    ws, out = _ab(torch, need), _ab(torch, n * t * 88)
    agr = out.data_ptr() + n * t * 24
    rc = lib.gcs_region_sweep_under(hist.data_ptr(), mp, al.data_ptr(), img_of.data_ptr(), rg.data_ptr(), b, t, k, stride, n,
                                    ws.data_ptr(), out.data_ptr(), agr if agreement else None, agr + n * t * 32 if agreement else None,
                                    stream)
    assert rc == 0, lib.gcs_last_error()
    need = lib.gcs_cut_shapes_workspace_bytes(b, k, n)
    assert need > 0
    ws2, out2 = _ab(torch, need), _ab(torch, 4 * n * b * (2 * k + 1))
    rc = lib.gcs_cut_shapes(ls.data_ptr(), cs.data_ptr(), mp, al.data_ptr(), rg.data_ptr(), b, h, w, k, n, ws2.data_ptr(),
                            out2.data_ptr(), out2.data_ptr() + 4 * n * b * k, out2.data_ptr() + 8 * n * b * k, stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    raw, raw2 = out.cpu().numpy(), out2.cpu().numpy().view(np.uint32)
    got = dict(under=raw[:n * t * 24].view(np.uint64).reshape(n, t, 3), area=raw2[:n * b * k].reshape(n, b, k),
               perim=raw2[n * b * k:2 * n * b * k].reshape(n, b, k), boundary=raw2[2 * n * b * k:].reshape(n, b), stride=stride)
    if agreement:
        got["sums"] = raw[n * t * 24:n * t * 56].view(np.uint64).reshape(n, t, 4)
        got["terms"] = raw[n * t * 56:].view(np.float64).reshape(n, t, 4)
    else:
        assert (raw[n * t * 24:] == 0xAB).all()
    # the inputs are read only
    assert np.array_equal(ls.cpu().numpy(), lab) and np.array_equal(cs.cpu().numpy(), us)
    assert ms is None or np.array_equal(ms.cpu().numpy(), np.asarray(merges).reshape(b, k - 1, 2))
    return got


def _check(torch, labs, merges, alives, groups, regions, k):
    """The raw calls on a batch against the restatement, every output ``==``. -> (got, want)."""
    labs = np.asarray(labs)
    rows = [np.zeros((0, 2), np.int32)] * len(labs) if merges is None else list(np.asarray(merges).reshape(len(labs), k - 1, 2))
    stride = int(max(int(np.max(g)) for group in groups for g in group)) + 1
    want = cr.batch(labs, rows, list(alives), groups, regions, k=k, stride=stride)
    got = _gpu_calls(torch, labs, want[4], merges, alives, groups, regions, k)
    for name, ref in zip(("under", "area", "perim", "boundary"), want):
        assert got[name].shape == ref.shape, name
        assert np.array_equal(got[name], ref), (name, np.argwhere(got[name] != ref)[:4].tolist())
    return got, want


def _k40_batch(top):
    """Two 19 x 23 images at K = 40 with 2 and 3 annotator maps; the second image leaves three labels unused (alive = 37)."""
    lab0, truths0 = rs.noise_case(seed=40, n_maps=2, top=top)
    lab1, truths1 = rs.noise_case(seed=41, n_maps=3, top=top)
    lab1[lab1 == 17] = 3
    lab1[lab1 == 30] = 31
    lab1[lab1 == 5] = 6
    return np.stack([lab0, lab1]), [truths0, truths1], np.array([40, 37], np.int32)


def _k40_lists(lab, tree0, tree1):
    """The list of image 0 over all 40 labels; that of image 1 over the 37 labels that own a pixel, 36 written rows and (-1, -1)
    behind them, as gcs_region_tree writes a tree of alive = 37."""
    used = np.unique(lab[1])
    assert len(used) == 37
    rows = np.full((39, 2), -1, np.int32)
    rows[:36] = used[tree1(37)]                              # (the labels in increasing order: a < b stays)
    return np.stack([tree0(40), rows])


@pytest.mark.parametrize("top", [207, 300])
@pytest.mark.parametrize("tree", sorted(cr.TREES))
def test_k_40_batch_of_two(torch_cuda, tree, top):
    """R = 42 .. 1 in one call; annotator labels up to 207: uint8 maps, rows kept in registers; a label of 300: uint16 maps."""
    lab, groups, alive = _k40_batch(top)
    got, _ = _check(torch_cuda, lab, _k40_lists(lab, cr.TREES[tree], cr.TREES[tree]), alive, groups, list(range(42, 0, -1)), 40)
    assert got["stride"] == top + 1 and (got["under"][:, :, 0] == 19 * 23).all()


@pytest.mark.parametrize("name", sorted(cr.one_pixel_cases()))
def test_k_4096_one_pixel_labels(torch_cuda, name):
    """The deepest chain, the widest group, and counters that do not fit LDS: the global-atomics paths."""
    lab, merges, alive, truths, regions = cr.one_pixel_cases()[name]
    got, _ = _check(torch_cuda, lab[None], merges[None], [alive], [truths], regions, 4096)
    assert got["area"][-1, 0, 0] == 4096 and got["perim"][-1, 0, 0] == 252 and got["boundary"][-1, 0] == 0


def test_smallest_k_and_the_ends_of_n_cuts(torch_cuda):
    small = cr.small_cases()
    lab, _, _, t0, _ = small["k1"]                           # K = 1: no rows, a NULL merges pointer; every cut is the leaf table
    got, _ = _check(torch_cuda, np.stack([lab, lab]), None, [1, 1], [t0[:2], t0[2:]], [9, 2, 1], 1)
    assert np.array_equal(got["under"][0], got["under"][2]) and (got["area"] == 35).all() and (got["perim"] == 20).all()
    for name in ("k2_joined", "k2_never_joined"):
        lab, merges, alive, truths, _ = small[name]
        got, _ = _check(torch_cuda, lab[None], merges[None], [alive], [truths], [4, 3, 2, 1], 2)
        assert (got["area"][3, 0, 1] == 0) == (name == "k2_joined")
    lab, merges, alive, truths, _ = small["k40_balanced"]
    _check(torch_cuda, lab[None], merges[None], [alive], [truths], [7], 40)                       # one cut
    _check(torch_cuda, lab[None], cm.chain(40)[None], [alive], [truths], list(range(64, 0, -1)), 40)   # 64 cuts


@pytest.mark.parametrize("name", ["shape_1x7", "shape_7x1", "shape_2x2", "unused_labels", "two_pieces"])
def test_small_images_and_sparse_label_sets(torch_cuda, name):
    """Images whose every pixel lies on the border; labels that own no pixel; a label in two pieces."""
    lab, merges, alive, truths, regions = cr.small_cases()[name]
    k = merges.shape[0] + 1
    got, _ = _check(torch_cuda, lab[None], merges[None], [alive], [truths], regions[::-1], k)
    if name.startswith("shape"):
        assert np.array_equal(got["area"], got["perim"])


@pytest.mark.parametrize("name", sorted(cr.odd_cases()))
def test_holes_malformed_rows_and_the_wall(torch_cuda, name):
    lab, merges, alive, truths, regions = cr.odd_cases()[name]
    k = merges.shape[0] + 1
    got, _ = _check(torch_cuda, lab[None], merges[None], [alive], [truths], regions, k)
    if name == "wall":                                       # the pixels outside 0 .. K-1 are in no table and no area
        inside = int(((lab >= 0) & (lab < k)).sum())
        assert (got["under"][:, :, 0] == inside).all() and (got["area"].sum(axis=2) == inside).all()
        assert (got["boundary"][:, 0] >= 2 * 9).all()        # the wall and one side of it, at every cut


def test_the_agreement_outputs_are_those_of_gcs_region_sweep(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    for top in (207, 300):
        lab, groups, alive = _k40_batch(top)
        merges = _k40_lists(lab, cm.balanced, cm.chain)
        regions = [41, 40, 33, 12, 5, 2, 1]
        us = np.stack([cr.contour_map(lab[i], merges[i], alive[i]) for i in range(2)])
        plain = _gpu_calls(torch, lab, us, merges, alive, groups, regions, 40)
        both = _gpu_calls(torch, lab, us, merges, alive, groups, regions, 40, agreement=True)
        assert np.array_equal(plain["under"], both["under"])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
        ls, ms, al, rg = dev(lab), dev(merges), dev(alive), dev(regions)
        hist, img_of, t, stride = _leaf_tables(torch, lib, ls, groups, 40)                       # a fresh copy of the leaf tables
        n = len(regions)
        ws, out = _ab(torch, lib.gcs_region_sweep_workspace_bytes(t, 40, stride, n)), _ab(torch, n * t * 64)
        rc = lib.gcs_region_sweep(hist.data_ptr(), ms.data_ptr(), al.data_ptr(), img_of.data_ptr(), rg.data_ptr(), 2, t, 40, stride, n,
                                  ws.data_ptr(), out.data_ptr(), out.data_ptr() + n * t * 32, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.gcs_last_error()
        raw = out.cpu().numpy()
        assert np.array_equal(both["sums"].ravel(), raw[:n * t * 32].view(np.uint64))
        assert np.array_equal(both["terms"].view(np.uint64).ravel(), raw[n * t * 32:].view(np.uint64))


_BSD = {}


def _bsd(torch, shape):
    """One val fixture image of ``shape`` through the plan, with its real ground truth on the device, once."""
    if shape not in _BSD:
        from gabor_color_image_segmentation_amd import Segmenter
        from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
        val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
        i = [str(i) for i in val["ids"] if val["img_" + str(i)].shape[:2] == shape][0]
        seg = Segmenter(n_superpixels=300, n_iter=4, **COLOUR)
        lab, merges, _, alive = seg.region_tree_device(torch.from_numpy(val["img_" + i][None]).cuda())
        contours = seg.contour_map_device(lab, merges, alive)
        _BSD[shape] = (i, seg, lab, merges, alive, contours, PackedTruth(os.path.join(GOLD, "bsd500_truth.npz")).to_device([i]))
    return _BSD[shape]


@pytest.mark.parametrize("shape", [(481, 321), (321, 481)])
def test_bsd_fixture_against_the_per_cut_scorer(torch_cuda, shape):
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_resident, metrics_sweep_resident
    i, seg, lab, merges, alive, contours, dt = _bsd(torch_cuda, shape)
    regions = [4, 6, 8, 12, 16, 32]
    got = metrics_sweep_resident(lab, merges, alive, contours, dt, regions, agreement=True)[0]
    assert dt._uncollected() is None                          # buffers of its own
    plain = metrics_sweep_resident(lab, merges, alive, contours, dt, regions)[0]
    for j, r in enumerate(regions):
        ref = all_scores_batch_resident(seg.cut_regions_device(lab, merges, alive, r), dt, agreement=True)[0]
        assert sorted(got[j]) == sorted(ref) and sorted(plain[j]) == sorted(set(ref) - {"PRI", "VoI", "covering"})
        for key in ("regions", "underseg", "undersegNP", "density", "recall", "precision", "fmeasure", "PRI"):
            assert got[j][key] == ref[key], (i, r, key, got[j][key], ref[key])
        assert abs(got[j]["compactness"] - ref["compactness"]) <= 1e-15 * max(1.0, abs(ref["compactness"])), (i, r)
        for key in ("VoI", "covering"):                       # (the bound of tests/test_gpu_region_sweep.py)
            assert abs(got[j][key] - ref[key]) <= 1e-12, (i, r, key, got[j][key], ref[key])
        assert all(plain[j][key] == got[j][key] for key in plain[j])


def test_same_bits_order_of_regions_and_the_other_paths(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import (DeviceTruth, all_scores_batch_resident, boundary_sweep_resident,
                                                                  cut_shapes_device, metrics_sweep_resident, region_sweep_resident,
                                                                  submit_scores_batch_resident, sweep_reference_scores,
                                                                  under_sweep_resident)
    lab, groups, alive = _k40_batch(207)
    merges = _k40_lists(lab, cm.balanced, cm.chain)
    flat = np.stack([g for group in groups for g in group])
    dt = DeviceTruth(flat, [0, 2, 5], [0, 0, 1, 1, 1], [int(g.max()) + 1 for g in flat])
    ls, ms, al = (torch.from_numpy(np.ascontiguousarray(v, np.int32)).cuda() for v in (lab, merges, alive))
    seg = Segmenter(n_superpixels=64, n_iter=3)
    contours = seg.contour_map_device(ls, ms, al)
    us = contours.cpu().numpy()
    assert np.array_equal(us, np.stack([cr.contour_map(lab[i], merges[i], alive[i]) for i in range(2)]))
    cut = seg.cut_regions_device(ls, ms, al, 5)
    regions = [8, 40, 3, 12]
    before = (boundary_sweep_resident(contours, al, dt), all_scores_batch_resident(cut, dt, agreement=True),
              region_sweep_resident(ls, ms, al, dt, regions))
    # two calls: the same bits; the caller's order is kept; the restatement
    call = lambda rr: (under_sweep_resident(ls, ms, al, dt, rr),) + cut_shapes_device(ls, contours, ms, al, rr)
    first, second, ordered = call(regions), call(regions), call(sorted(regions, reverse=True))
    back = [sorted(regions, reverse=True).index(r) for r in regions]
    want = cr.batch(lab, merges, alive, groups, regions, k=40, stride=dt.stride, us=us)
    for a, b, c, ref in zip(first, second, ordered, want):
        assert a.dtype == ref.dtype and np.array_equal(a, ref) and np.array_equal(a, b) and np.array_equal(a, c[back])
    counts, sums, terms = under_sweep_resident(ls, ms, al, dt, regions, agreement=True)
    assert np.array_equal(counts, first[0]) and np.array_equal(sums, before[2][0])
    assert np.array_equal(terms.view(np.uint64), before[2][1].view(np.uint64))
    # the cut at R = 5 of the per-cut scorer, through the sweep; R = 1 has no boundary pixel
    five = metrics_sweep_resident(ls, ms, al, contours, dt, [5], agreement=True)
    for i in range(2):
        assert sorted(five[i][0]) == sorted(before[1][i])
        for key in ("regions", "underseg", "undersegNP", "density", "recall", "precision", "fmeasure", "PRI"):
            assert five[i][0][key] == before[1][i][key], (i, key)
        assert abs(five[i][0]["compactness"] - before[1][i]["compactness"]) <= 1e-15 * max(1.0, abs(before[1][i]["compactness"]))
    with pytest.raises(ZeroDivisionError):
        metrics_sweep_resident(ls, ms, al, contours, dt, [5, 1])
    one = sweep_reference_scores(*call([1]), alive, dt.first, 19, 23, [1])
    assert [row[0]["regions"] for row in one] == [1, 1] and [row[0]["density"] for row in one] == [0.0, 0.0]
    assert all(row[0]["underseg"] > 0.0 for row in one)
    # a submission that is still uncollected keeps its numbers through the new calls
    pending = submit_scores_batch_resident(cut, dt, agreement=True)
    metrics_sweep_resident(ls, ms, al, contours, dt, regions, agreement=True)
    assert dt._uncollected() is pending
    assert pending.result() == before[1]
    after = (boundary_sweep_resident(contours, al, dt), all_scores_batch_resident(cut, dt, agreement=True),
             region_sweep_resident(ls, ms, al, dt, regions))
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and before[1] == after[1]
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1].view(np.uint64), after[2][1].view(np.uint64))
    # the inputs are not modified
    assert np.array_equal(ls.cpu().numpy(), lab) and np.array_equal(ms.cpu().numpy(), merges) and np.array_equal(contours.cpu().numpy(), us)
    for bad in (lambda: under_sweep_resident(ls, ms, al, dt, [4, 4]), lambda: cut_shapes_device(ls, contours, ms, al, [4, 4]),
                lambda: under_sweep_resident(ls[:1], ms, al, dt, [4]), lambda: cut_shapes_device(ls[:1], contours[:1], ms, al, [4]),
                lambda: cut_shapes_device(ls, contours[:, :, :22], ms, al, [4]),
                lambda: metrics_sweep_resident(ls, ms, al, contours[:1], dt, [4])):
        with pytest.raises(ValueError):
            bad()
