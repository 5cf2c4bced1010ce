"""Region agreement (SPEC.md §8): PRI, VoI and segmentation covering on the host, against a brute-force restatement, the
third-party golden (scikit-learn / scikit-image, tests/golden/make_region_golden.py) and their invariances; host-only argument
checks of gcs_region_agreement (nothing is launched)."""
import ctypes as C
import itertools
import json
import math
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

from gabor_color_image_segmentation_amd import _lib
from gabor_color_image_segmentation_amd.evaluate import region_agreement

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _brute(s, segs):
    """O(N^2) pairs for RI, probabilities for VoI, region sets for covering."""
    s = np.asarray(s).ravel()
    n = s.size
    ri, voi, cov = [], [], []
    for g in segs:
        g = np.asarray(g).ravel()
        agree = sum((s[p] == s[q]) == (g[p] == g[q]) for p, q in itertools.combinations(range(n), 2))
        ri.append(agree / (n * (n - 1) / 2))
        v = 0.0                                                     # H(S|G) + H(G|S) = -sum p_xy log2(p_xy^2 / (p_x p_y))
        for x in set(s.tolist()):
            for y in set(g.tolist()):
                pxy = np.sum((s == x) & (g == y)) / n
                if pxy > 0:
                    v -= pxy * math.log2(pxy * pxy / ((np.sum(s == x) / n) * (np.sum(g == y) / n)))
        voi.append(v)
        c = 0.0
        for y in set(g.tolist()):
            r = g == y
            c += r.sum() * max(np.sum(r & (s == x)) / np.sum(r | (s == x)) for x in set(s[r].tolist()))
        cov.append(c / n)
    return np.mean(ri), np.mean(voi), np.mean(cov)


def test_equals_brute_force_on_small_random_maps():
    rng = np.random.default_rng(7)
    for _ in range(12):
        k = int(rng.integers(1, 7))
        s = rng.integers(0, k, (7, 9))
        segs = [rng.integers(0, int(rng.integers(1, 5)), (7, 9)) for _ in range(int(rng.integers(1, 5)))]
        got = region_agreement(s, segs)
        pri, voi, cov = _brute(s, segs)
        assert abs(got["PRI"] - pri) <= 1e-12 and abs(got["VoI"] - voi) <= 1e-12 and abs(got["covering"] - cov) <= 1e-12


def connected(lab):
    """4-connected components of equal labels (any numbering: the metrics ignore it)."""
    out = np.zeros(lab.shape, np.int64)
    nxt = 0
    for v in np.unique(lab):
        comp, n = ndi.label(lab == v)
        out[comp > 0] = comp[comp > 0] - 1 + nxt
        nxt += n
    return out


def golden_maps():
    """(key, label map, annotator maps) for the 12 scoring maps and the 24 val maps, stored and connected."""
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    inp = np.load(os.path.join(GOLD, "bsd_inputs.npz"))
    path = np.load(os.path.join(GOLD, "path_golden.npz"))
    maps = np.load(os.path.join(GOLD, "scoring_maps.npz"))
    out = []
    for i in inp["ids"]:
        i = str(i)
        segs = [inp["seg_%s_%d" % (i, a)] for a in range(int(inp["nseg_" + i]))]
        h, w = inp["img_" + i].shape[:2]
        cand = {"oracle": path["labels_" + i].astype(np.int32),
                "halves": (np.arange(w)[None, :] >= w // 2).astype(np.int32) * np.ones((h, 1), np.int32),
                "blocks": ((np.arange(h)[:, None] // 16) * ((w + 15) // 16) + np.arange(w)[None, :] // 16).astype(np.int32),
                "slic": maps["slic_" + i].astype(np.int32)}
        out += [("scoring/%s/%s" % (i, k), v, segs) for k, v in cand.items()]
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    for i in val["ids"]:
        i = str(i)
        lab = val["labels_" + i].astype(np.int32)
        out.append(("val/%s/stored" % i, lab, pt[i]))
        out.append(("val/%s/connected" % i, connected(lab).astype(np.int32), pt[i]))
    return out


def test_equals_the_third_party_golden():
    gold = json.load(open(os.path.join(GOLD, "region_agreement_golden.json")))
    keys = set()
    for key, lab, segs in golden_maps():
        g = gold[key]
        got = region_agreement(lab, segs)
        assert abs(got["PRI"] - g["PRI"]) <= 1e-12, key
        assert abs(got["VoI"] - g["VoI"]) <= 1e-12, key
        assert abs(got["covering"] - g["covering_mean"]) <= 1e-12, key
        if "regions" in g:
            assert int(lab.max()) + 1 == g["regions"], key
        keys.add(key)
    assert len(keys) == 12 + 48 == len(gold)


def test_invariances():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 5, (20, 30))
    segs = [rng.integers(0, 4, (20, 30)), rng.integers(0, 7, (20, 30))]
    ref = region_agreement(s, segs)
    perm = rng.permutation(50)                                      # relabel S injectively (and sparsely)
    assert region_agreement(perm[s], segs) == pytest.approx(ref, abs=1e-12)
    assert region_agreement(segs[0], [segs[0]]) == {"PRI": 1.0, "VoI": 0.0, "covering": 1.0}
    g = segs[1]
    b = np.bincount(g.ravel()).astype(np.float64)
    assert region_agreement(np.zeros_like(g), [g])["covering"] == pytest.approx(np.sum(b * b) / g.size ** 2, abs=1e-15)
    with pytest.raises(ValueError):
        region_agreement(np.zeros((1, 1), np.int32), [np.zeros((1, 1), np.int32)])
    with pytest.raises(ZeroDivisionError):
        region_agreement(s, [])


@pytest.fixture(scope="module")
def lib(built):
    return _lib.load()


def test_abi_rejects_bad_arguments(lib):
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    fn = lib.gcs_region_agreement
    cases = [(None, None, None, 1, 8, 8, p, p, p), (p, None, None, 1, 8, 8, None, p, p), (p, None, None, 1, 8, 8, p, None, p),
             (p, None, None, 1, 8, 8, p, p, None),
             (p, None, p, 1, 8, 8, p, p, p),                            # seg_max without img_of
             (p, p, p, 0, 8, 8, p, p, p), (p, p, p, 1, 0, 8, p, p, p), (p, p, p, 1, 8, -1, p, p, p),
             (p, p, p, 1 << 20, 1 << 10, 1 << 10, p, p, p)]              # table of more than 2^30 counters
    for args in cases:
        assert fn(*args, None) == 1, args                               # GCS_EINVAL
        assert b"gcs_region_agreement" in lib.gcs_last_error()
    assert lib.gcs_region_agreement_scratch_bytes(3, 8, 114) == 3 * (8 + 114) * 4
    assert lib.gcs_region_agreement_scratch_bytes(0, 8, 114) == 0
