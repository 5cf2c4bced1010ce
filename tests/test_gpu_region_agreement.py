"""Region agreement on the GPU (SPEC.md §8): gcs_region_agreement through the single-map, batched and resident scorers,
against the third-party golden (tests/golden/region_agreement_golden.json) and the host definition."""
import json
import os

import numpy as np
import pytest

from test_region_agreement import connected, golden_maps

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
KEYS = ("PRI", "VoI", "covering")


def _gold():
    return json.load(open(os.path.join(GOLD, "region_agreement_golden.json")))


def _close(got, ref, what, pri_exact=True):
    """PRI comes from exact integer sums through the shared finishing step: the same float; the float terms within 1e-12."""
    if pri_exact:
        assert got["PRI"] == ref["PRI"], what
    for k in KEYS:
        assert abs(got[k] - ref[k]) <= 1e-12, (what, k, got[k], ref[k])


def _val_groups():
    """The 24 packed val maps by image shape: (ids, stored labels [B,H,W], connected labels [B,H,W])."""
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"]]
    out = []
    for shape in sorted({val["labels_" + i].shape for i in ids}):
        group = [i for i in ids if val["labels_" + i].shape == shape]
        stored = np.stack([val["labels_" + i].astype(np.int32) for i in group])
        out.append((group, stored, np.stack([connected(m).astype(np.int32) for m in stored])))
    return out


def test_single_map_equals_golden_and_host(built):
    import torch
    from gabor_color_image_segmentation_amd.evaluate import region_agreement
    from gabor_color_image_segmentation_amd.evaluate_gpu import region_agreement_device
    gold = _gold()
    for key, lab, segs in golden_maps()[:12]:
        got = region_agreement_device(torch.from_numpy(np.ascontiguousarray(lab)).cuda(), segs)
        _close(got, region_agreement(lab, segs), key)
        g = gold[key]
        _close(got, {"PRI": g["PRI"], "VoI": g["VoI"], "covering": g["covering_mean"]}, key, pri_exact=False)


def test_batched_and_resident_on_the_val_maps(built):
    """Stored and connected maps through the batched path (uint16 truth uploaded per call) and the resident path (uint8 maps,
    tables at a capacity of 8 192 segments for the connected maps, rows bounded by seg_max): the golden values, the other keys
    unchanged by agreement=True, resident == batched float for float, two calls the same bits."""
    import torch
    from gabor_color_image_segmentation_amd.evaluate import region_agreement
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    gold = _gold()
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    n = 0
    caps = set()
    for group, stored, conn in _val_groups():
        stack = pt.stack(group)
        dt = pt.to_device(group)
        assert dt.u8
        for kind, labs in (("stored", stored), ("connected", conn)):
            dev = torch.from_numpy(labs).cuda()
            got = all_scores_batch_device(dev, *stack, agreement=True)
            plain = all_scores_batch_device(dev, *stack)
            res = all_scores_batch_device(dev, dt, agreement=True)
            if kind == "connected":
                caps.add(dt._out[0])                                 # capacity of the resident tables
            assert res == got, kind
            assert all_scores_batch_device(dev, dt, agreement=True) == res, kind    # same bits again
            assert all_scores_batch_device(dev, dt) == plain, kind                  # agreement=False: as before
            for i, b, p, lab in zip(group, got, plain, labs):
                assert {k: v for k, v in b.items() if k not in KEYS} == p, (i, kind)
                g = gold["val/%s/%s" % (i, kind)]
                _close(b, {"PRI": g["PRI"], "VoI": g["VoI"], "covering": g["covering_mean"]}, (i, kind), pri_exact=False)
                if kind == "connected":
                    _close(b, region_agreement(lab, pt[i]), (i, kind))
                n += 1
    assert n == 48 and 8192 in caps


def _synthetic(n_labels, shape=(40, 56), counts=(3, 1, 4), seed=0):
    """Ragged synthetic truth with labels up to n_labels - 1 (uint16 maps) and label maps of a few segments."""
    rng = np.random.default_rng(seed)
    h, w = shape
    maps, first, img_of = [], [0], []
    for b, a in enumerate(counts):
        for _ in range(a):
            m = rng.integers(0, n_labels, (h, w)).astype(np.uint16)
            m[0, 0] = n_labels - 1
            maps.append(m)
            img_of.append(b)
        first.append(first[-1] + a)
    truth = np.stack(maps)
    labels = np.stack([(rng.integers(0, 6, (h, w)) + (np.arange(w)[None, :] * 3) // w).astype(np.int32) for _ in counts])
    return truth, np.array(first, np.int32), np.array(img_of, np.int32), [int(m.max()) + 1 for m in maps], labels


@pytest.mark.parametrize("n_labels", [300, 2500])
def test_uint16_truth_and_wide_tables(built, n_labels):
    """More than 256 annotator labels (uint16 resident maps); 2 500 columns run the kernel's column-chunk loop (1 024 per
    chunk). Ragged annotator counts 3 / 1 / 4."""
    import torch
    from gabor_color_image_segmentation_amd.evaluate import region_agreement
    from gabor_color_image_segmentation_amd.evaluate_gpu import DeviceTruth, all_scores_batch_device, region_agreement_device
    truth, first, img_of, n_truth, labels = _synthetic(n_labels)
    dev = torch.from_numpy(labels).cuda()
    got = all_scores_batch_device(dev, truth, first, img_of, n_truth, agreement=True)
    dt = DeviceTruth(truth, first, img_of, n_truth)
    assert not dt.u8 and dt.stride == n_labels
    assert all_scores_batch_device(dev, dt, agreement=True) == got
    for b in range(len(first) - 1):
        segs = list(truth[first[b]:first[b + 1]])
        _close(got[b], region_agreement(labels[b], segs), b)
        _close(region_agreement_device(dev[b], segs), got[b], b)


def test_labels_beyond_n_segments_raise(built):
    import torch
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    group, stored, _ = _val_groups()[0]
    dev = torch.from_numpy(stored).cuda()
    n_seg = int(stored.max())                                       # one too few
    with pytest.raises(ValueError):
        all_scores_batch_device(dev, *pt.stack(group), n_segments=n_seg, agreement=True)
    with pytest.raises(ValueError):
        all_scores_batch_device(dev, pt.to_device(group), n_segments=n_seg, agreement=True)
