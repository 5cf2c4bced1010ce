"""GPU region metrics of every cut of the region tree (SPEC.md §16): gcs_region_sweep on leaf tables of gcs_region_counts_batch[_u8]
against the restatement (tests/region_sweep_ref.py) - every integer sum ``==``, every finished score by the rule of the CPU tests
(PRI ``==``, VoI and covering within 1e-12 of ``evaluate.region_agreement`` on the relabelled cut) -, the edge cases of K and of the
number of cuts, the library's own trees on the BSD fixtures against the per-cut scorer, and the existing paths before and after.
Workspace and outputs start out as 0xAB bytes."""
import os

import numpy as np
import pytest

import contour_map_ref as cm
import region_sweep_ref as rs
import region_tree_ref as rt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
TREES = {"chain": cm.chain, "star": cm.star, "balanced": cm.balanced}
TOL = 1e-12


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _gpu_sweep(torch, lab, merges, alive, groups, regions, k):
    """lab (B, H, W); merges (B, k - 1, 2) or None (k = 1: a NULL pointer); alive (B,); groups: per image its list of annotator maps;
    regions strictly decreasing -> (sums uint64 [n][T][4], terms float64 [n][T][4], stride): the raw calls, the leaf tables by
    gcs_region_counts_batch_u8 when every annotator label fits a byte and by gcs_region_counts_batch otherwise."""
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    lab = np.ascontiguousarray(lab, np.int32)
    b, h, w = lab.shape
    flat = np.stack([g for group in groups for g in group]).astype(np.uint16)
    counts = [len(group) for group in groups]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    img_of = np.repeat(np.arange(b), counts).astype(np.int32)
    t, stride, n = len(flat), int(flat.max()) + 1, len(regions)
    u8 = stride <= 256
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ls, fs, io, al = dev(lab), dev(first), dev(img_of), dev(np.asarray(alive, np.int32).reshape(b))
    maps = dev(flat.astype(np.uint8)) if u8 else dev(flat.view(np.int16))
    ms = None if merges is None else dev(np.asarray(merges, np.int32).reshape(b, k - 1, 2))
    rg = dev(np.asarray(regions, np.int32))
    hist = torch.full((t * k * stride,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")         # the counts call zeroes it itself
    side = torch.empty(2 * b * k, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fn = lib.gcs_region_counts_batch_u8 if u8 else lib.gcs_region_counts_batch
    rc = fn(ls.data_ptr(), maps.data_ptr(), fs.data_ptr(), b, t, max(counts), h, w, k, stride, hist.data_ptr(), side.data_ptr(),
            side.data_ptr() + 4 * b * k, stream)
    assert rc == 0, lib.gcs_last_error()
    need = lib.gcs_region_sweep_workspace_bytes(t, k, stride, n)
    assert need > 0
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    out = torch.full((2 * n * t * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    rc = lib.gcs_region_sweep(hist.data_ptr(), None if ms is None else ms.data_ptr(), al.data_ptr(), io.data_ptr(), rg.data_ptr(), b, t,
                              k, stride, n, ws.data_ptr(), out.data_ptr(), out.data_ptr() + n * t * 32, stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    raw = out.cpu().numpy()
    return raw[:n * t * 32].view(np.uint64).reshape(n, t, 4), raw[n * t * 32:].view(np.float64).reshape(n, t, 4), stride


def _check(torch, lab, merges, alive, groups, regions, k):
    """The raw call against the restatement (sums ``==``) and against region_agreement of the relabelled cut (the finished scores)."""
    from gabor_color_image_segmentation_amd import evaluate as ev
    lab = np.asarray(lab)
    sums, terms, stride = _gpu_sweep(torch, lab, merges, alive, groups, regions, k)
    t0, worst = 0, 0.0
    for i, group in enumerate(groups):
        m = np.zeros((0, 2), np.int32) if merges is None else np.asarray(merges).reshape(lab.shape[0], k - 1, 2)[i]
        a = int(np.asarray(alive).reshape(-1)[i])
        want_s, want_t = rs.sweep(lab[i], m, a, group, regions, k=k, stride=stride)
        got_s, got_t = sums[:, t0:t0 + len(group)], terms[:, t0:t0 + len(group)]
        assert np.array_equal(got_s, want_s), (i, np.argwhere(got_s != want_s)[:4].tolist())
        assert np.isfinite(got_t).all()
        for j, r in enumerate(regions):
            got = ev.agreement_from_sums(got_s[j], got_t[j], [0, len(group)], lab[i].size)[0]
            mid = ev.agreement_from_sums(want_s[j], want_t[j], [0, len(group)], lab[i].size)[0]
            want = ev.region_agreement(rt.cut(lab[i], m, a, r), group)
            assert got["PRI"] == want["PRI"] == mid["PRI"], (i, r, got, want)
            for key in ("VoI", "covering"):
                worst = max(worst, abs(got[key] - want[key]))
                assert abs(got[key] - want[key]) <= TOL and abs(got[key] - mid[key]) <= TOL, (i, r, key, got[key], want[key], mid[key])
        t0 += len(group)
    print("largest difference of a finished score", worst)
    return sums, terms


def _k40_batch(top):
    """Two 19 x 23 images at K = 40 with 2 and 3 annotator maps; the second image leaves three labels unused (alive = 37)."""
    lab0, truths0 = rs.noise_case(seed=40, n_maps=2, top=top)
    lab1, truths1 = rs.noise_case(seed=41, n_maps=3, top=top)
    lab1[lab1 == 17] = 3
    lab1[lab1 == 30] = 31
    lab1[lab1 == 5] = 6
    return np.stack([lab0, lab1]), [truths0, truths1], np.array([40, 37], np.int32)


@pytest.mark.parametrize("top", [207, 300])
@pytest.mark.parametrize("tree", sorted(TREES))
def test_k_40_batch_of_two(torch_cuda, tree, top):
    """R = 42 .. 1 in one call; annotator labels up to 207: uint8 maps, stride 208; a label of 300: uint16 maps, stride 301."""
    lab, groups, alive = _k40_batch(top)
    assert len(np.unique(lab[1])) == 37
    merges = np.stack([TREES[tree](40)] * 2)
    _check(torch_cuda, lab, merges, alive, groups, list(range(42, 0, -1)), 40)


@pytest.mark.parametrize("tree", sorted(TREES))
def test_k_4096_one_pixel_labels(torch_cuda, tree):
    """The deepest chain, the widest group, and tables that do not fit LDS."""
    lab, truths = rs.one_pixel_case()
    sums, _ = _check(torch_cuda, lab[None], TREES[tree](4096)[None], [4096], [truths], [5000, 4096, 4095, 1000, 64, 8, 3, 2, 1], 4096)
    assert (sums[:, :, 0] == 4096).all() and sums[8, 0, 1] == 4096 ** 2 and sums[0, 0, 1] == 4096


def test_smallest_k_and_the_ends_of_n_cuts(torch_cuda):
    torch = torch_cuda
    # K = 1: no rows, a NULL merges pointer; every cut is the leaf table
    lab = np.zeros((2, 5, 7), np.int32)
    _, t0 = rs.noise_case(seed=2, shape=(5, 7), n_maps=2)
    _, t1 = rs.noise_case(seed=3, shape=(5, 7), n_maps=1)
    sums, terms = _check(torch, lab, None, [1, 1], [t0, t1], [9, 2, 1], 1)
    assert np.array_equal(sums[0], sums[2]) and np.array_equal(terms[0].view(np.uint64), terms[2].view(np.uint64))
    # K = 2: joined, and never joined
    lab = np.random.default_rng(2).integers(0, 2, (1, 9, 13)).astype(np.int32)
    _, tr = rs.noise_case(seed=4, shape=(9, 13))
    joined, _ = _check(torch, lab, np.array([[[0, 1]]]), [2], [tr], [3, 2, 1], 2)
    apart, _ = _check(torch, lab, np.array([[[-1, -1]]]), [2], [tr], [3, 2, 1], 2)
    assert np.array_equal(joined[:2], apart[:2]) and np.array_equal(apart[1], apart[2]) and not np.array_equal(joined[1], joined[2])
    # one cut; 64 cuts
    lab, truths = rs.noise_case()
    _check(torch, lab[None], cm.balanced(40)[None], [40], [truths], [7], 40)
    _check(torch, lab[None], cm.chain(40)[None], [40], [truths], list(range(64, 0, -1)), 40)


def test_rows_that_do_not_count_are_skipped(torch_cuda):
    """The lists of the CPU test: (-1, -1) rows among the written ones; rows that are not (a < b, both reps at that step)."""
    lab, truths = rs.noise_case(seed=8, k=6, shape=(9, 11))
    holes = np.array([[1, 2], [-1, -1], [0, 1], [-1, -1], [3, 4]], np.int32)
    _check(torch_cuda, lab[None], holes[None], [6], [truths], [7, 6, 5, 4, 3, 2, 1], 6)
    # not comparable with the relabelled cut (it applies every row): the restatement alone, and the bits of the list without them
    #                 ok      b is dead  a is dead  a > b    a == b   b >= K   ok
    bad = np.array([[1, 2], [0, 2], [2, 3], [4, 3], [3, 3], [0, 9], [0, 1]], np.int32)
    clean = np.array([[1, 2], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [0, 1]], np.int32)
    later = np.array([[0, 1], [1, 2], [0, 2], [-1, -1], [-1, -1], [-1, -1], [-1, -1]], np.int32)    # row 1 is skipped: 2 joins at row 2
    from gabor_color_image_segmentation_amd import evaluate as ev
    lab8, truths8 = rs.noise_case(seed=9, k=8, shape=(9, 11))
    regions, got = [8, 7, 6, 2, 1], {}
    for name, m in (("bad", bad), ("clean", clean), ("later", later)):
        got[name] = _gpu_sweep(torch_cuda, lab8[None], m[None], [8], [truths8], regions, 8)
        want = rs.sweep(lab8, m, 8, truths8, regions, k=8, stride=got[name][2])
        assert np.array_equal(got[name][0], want[0]), name
        for j in range(len(regions)):
            a = ev.agreement_from_sums(got[name][0][j], got[name][1][j], [0, 3], lab8.size)[0]
            b = ev.agreement_from_sums(want[0][j], want[1][j], [0, 3], lab8.size)[0]
            assert a["PRI"] == b["PRI"] and abs(a["VoI"] - b["VoI"]) <= TOL and abs(a["covering"] - b["covering"]) <= TOL, (name, j)
    assert np.array_equal(got["bad"][0], got["clean"][0])
    assert np.array_equal(got["bad"][1].view(np.uint64), got["clean"][1].view(np.uint64))
    assert np.array_equal(got["later"][0][1], got["later"][0][2])           # row 1 of `later` changed nothing


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
        _BSD[shape] = (i, seg, lab, merges, alive, PackedTruth(os.path.join(GOLD, "bsd500_truth.npz")).to_device([i]))
    return _BSD[shape]


@pytest.mark.parametrize("shape", [(481, 321), (321, 481)])
def test_bsd_fixture_against_the_per_cut_scorer(torch_cuda, shape):
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_resident, region_sweep_resident, sweep_agreement
    i, seg, lab, merges, alive, dt = _bsd(torch_cuda, shape)
    regions = [4, 6, 8, 12, 16, 32]
    sums, terms = region_sweep_resident(lab, merges, alive, dt, regions)
    assert sums.shape == (6, dt.t, 4) and sums.dtype == np.uint64 and terms.shape == (6, dt.t, 4) and terms.dtype == np.float64
    got = sweep_agreement(sums, terms, dt.first, shape[0] * shape[1], regions)[0]
    assert dt._uncollected() is None                          # buffers of its own
    for j, r in enumerate(regions):
        ref = all_scores_batch_resident(seg.cut_regions_device(lab, merges, alive, r), dt, agreement=True)[0]
        print(i, r, got[j], {key: ref[key] for key in ("PRI", "VoI", "covering")})
        assert got[j]["PRI"] == ref["PRI"], (i, r, got[j]["PRI"], ref["PRI"])
        for key in ("VoI", "covering"):
            assert abs(got[j][key] - ref[key]) <= TOL, (i, r, key, got[j][key], ref[key])


def test_same_bits_order_of_regions_and_the_other_paths(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import (DeviceTruth, all_scores_batch_resident, boundary_sweep_resident,
                                                                  region_sweep_resident, submit_scores_batch_resident, sweep_agreement)
    lab, groups, alive = _k40_batch(207)
    merges = np.stack([cm.balanced(40), cm.chain(40)])
    flat = np.stack([g for group in groups for g in group])
    dt = DeviceTruth(flat, [0, 2, 5], [0, 0, 1, 1, 1], [int(g.max()) + 1 for g in flat])
    ls, ms, al = (torch.from_numpy(np.ascontiguousarray(v, np.int32)).cuda() for v in (lab, merges, alive))
    seg = Segmenter(n_superpixels=64, n_iter=3)
    contours = seg.contour_map_device(ls, ms, al)
    cut = seg.cut_regions_device(ls, ms, al, 5)
    before = boundary_sweep_resident(contours, al, dt), all_scores_batch_resident(cut, dt, agreement=True)
    # two calls: the same bits; the caller's order is kept
    regions = [8, 40, 3, 12]
    first, second = region_sweep_resident(ls, ms, al, dt, regions), region_sweep_resident(ls, ms, al, dt, regions)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1].view(np.uint64), second[1].view(np.uint64))
    ordered = region_sweep_resident(ls, ms, al, dt, sorted(regions, reverse=True))
    back = [sorted(regions, reverse=True).index(r) for r in regions]
    assert np.array_equal(first[0], ordered[0][back]) and np.array_equal(first[1].view(np.uint64), ordered[1][back].view(np.uint64))
    for i in range(2):
        want = rs.sweep(lab[i], merges[i], alive[i], groups[i], regions, k=40, stride=dt.stride)
        assert np.array_equal(first[0][:, dt.first[i]:dt.first[i + 1]], want[0]), i
    scores = sweep_agreement(first[0], first[1], dt.first, 19 * 23, regions)
    assert len(scores) == 2 and len(scores[0]) == 4
    # the cut at R = 5 of the per-cut scorer, through the sweep
    five = sweep_agreement(*region_sweep_resident(ls, ms, al, dt, [5]), dt.first, 19 * 23, [5])
    for i in range(2):
        assert five[i][0]["PRI"] == before[1][i]["PRI"]
        assert abs(five[i][0]["VoI"] - before[1][i]["VoI"]) <= TOL and abs(five[i][0]["covering"] - before[1][i]["covering"]) <= TOL
    # a submission that is still uncollected keeps its numbers through a sweep call
    pending = submit_scores_batch_resident(cut, dt, agreement=True)
    region_sweep_resident(ls, ms, al, dt, regions)
    assert dt._uncollected() is pending
    assert pending.result() == before[1]
    after = boundary_sweep_resident(contours, al, dt), all_scores_batch_resident(cut, dt, agreement=True)
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and before[1] == after[1]
    # the inputs are not consumed: only the call's own leaf tables are
    assert np.array_equal(ls.cpu().numpy(), lab) and np.array_equal(ms.cpu().numpy(), merges)
    with pytest.raises(ValueError):
        region_sweep_resident(ls, ms, al, dt, [4, 4])
    with pytest.raises(ValueError):
        region_sweep_resident(ls[:1], ms, al, dt, [4])
