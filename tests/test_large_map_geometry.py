"""The geometry of the batches of tests/test_gpu_large_maps.py, asserted on the host, and the completeness of that file's coverage
table. Nothing is launched."""
import inspect
import os
import re

import numpy as np

import large_maps as lm
from large_maps import H, LINE31, LINE32, MARGIN, N_BASE, P, W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

INT32 = ["element 2^31", "byte 2^31", "byte 2^32", "byte 2^33"]          # (element 2^31 of an int32 array IS its byte 2^33)


def test_the_shape_and_the_counts():
    """161 x 241: no side a multiple of 8 (so of 16, 32, 64), P >= 32 769 so that B <= 65535 reaches 2^31 pixels, one image far
    below the margin; every count is the smallest that passes its line by the margin, and inside B <= 65535."""
    assert (H, W, P) == (161, 241, 38801) and H % 8 and W % 8 and P >= 32769 and 50 * P < MARGIN
    assert (lm.N31, lm.N30, lm.N29, lm.B_GUARD, lm.N_CANON, lm.N_COLOUR) == (55401, 27728, 13891, 55346, 1539, 36916)
    for n, line in ((lm.N31, LINE31), (lm.N30, 1 << 30), (lm.N29, 1 << 29)):
        assert (n - 1) * P < line + MARGIN <= n * P and n <= 65535
    assert lm.B_GUARD * P < LINE31 <= (lm.B_GUARD + 1) * P and lm.B_GUARD < lm.N31
    per = lm.D_CANON * P
    assert (lm.N_CANON - 1) * per < LINE32 + MARGIN <= lm.N_CANON * per
    assert 3 * (lm.N_COLOUR - 1) * P < LINE32 + MARGIN <= 3 * lm.N_COLOUR * P
    assert lm.N31 + 10000 <= 65535                                      # gcs_boundary_counts_batch takes B + T <= 65535


def test_every_array_straddles_its_lines_with_three_different_images():
    """tests/large_maps.py: check_array's assertions for every kind of array the GPU file builds, with the lines each must cross -
    as element index and as byte offset for its element size (1, 2, 4, 8 bytes, and the 3-byte pixels of an interleaved image)."""
    lab, img, truth = lm.base_labels(), lm.base_images(), lm.base_truth()
    idx31, idx30, idx29 = lm.batch(lm.N31), lm.batch(lm.N30), lm.batch(lm.N29)
    got = lm.check_array(lab, idx31, 4, INT32)
    assert got["element 2^31"] == got["byte 2^33"] == lm.B_GUARD                     # the image the guards of B H W < 2^31 stop at
    lm.check_array(lab.astype(np.uint8), idx31, 1, ["element 2^31"])                 # uint8 maps: gcs_labels_widen, dir_out
    lm.check_array(truth, idx31, 2, ["element 2^31", "byte 2^31", "byte 2^32"])      # (element 2^31 IS byte 2^32)
    lm.check_array(truth.astype(np.uint8), idx31, 1, ["element 2^31"])
    lm.check_array(img, idx31, 1, ["element 2^31", "element 2^32"])                  # 3-byte pixels: byte lines
    lm.check_array(img, lm.batch(lm.N_COLOUR), 1, ["element 2^31", "element 2^32"])
    lm.check_array(lab, idx30, 4, ["byte 2^31", "byte 2^32"])                        # gcs_connected_regions: no element line
    lm.check_array(lab, idx29, 4, ["byte 2^31"])                                     # the merge kernels' int32 arrays
    lm.check_array(lab.astype(np.int64), idx29, 8, ["byte 2^31", "byte 2^32"])       # ... and a 64-bit array per pixel (`best`)
    for base in (lab, lm.base_labels(12, seed=12)):                                  # at the guard: byte lines only
        lm.check_array(base, lm.batch(lm.B_GUARD), 4, ["byte 2^31", "byte 2^32"])


def test_the_canonical_batch_holds_both_element_lines():
    """uint16 [B][72][H][W] at B = 1 539: element 2^31 (= byte 2^32) and element 2^32 (= byte 2^33) inside, byte 2^31 too."""
    x = lm.base_canonical()
    assert x.shape == (N_BASE, 72, H, W) and x.max() >= 32768 and x.max() <= 46339
    got = lm.check_array(x, lm.batch(lm.N_CANON), 2, ["element 2^31", "element 2^32", "byte 2^31", "byte 2^32", "byte 2^33"])
    assert got["element 2^32"] == got["byte 2^33"] == lm.N_CANON - 2


def _prototypes():
    text = "".join(open(os.path.join(ROOT, "include", name)).read() for name in ("gcs.h", "gcs_cues.h"))
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict(re.findall(r"\b(gcs_\w+)\s*\(([^;(){}]*)\);", code))


def test_the_coverage_table_is_complete():
    """COVERAGE of tests/test_gpu_large_maps.py holds exactly the entry points of SIGNATURES and EXTENSIONS that take a device
    pointer (not HOST_ONLY of tests/test_gpu_buffer_contracts.py) and no feature slab (no ``feats_dev`` / ``feats_slab_dev``
    parameter in the headers); each maps to a gpu test of the file whose source makes the call, or to "not covered: " and a reason."""
    import test_gpu_buffer_contracts as bc
    import test_gpu_large_maps as big
    from gabor_color_image_segmentation_amd import _lib
    protos = _prototypes()
    both = set(_lib.SIGNATURES) | set(_lib.EXTENSIONS)
    assert both <= set(protos), sorted(both - set(protos))
    slab = {s for s in both if re.search(r"\bfeats_(slab_)?dev\b", protos[s])}
    assert {"gcs_gabor_features", "gcs_kmeans_pass_fused", "gcs_region_tree_slab", "gcs_feature_gradient"} <= slab and len(slab) == 11
    want = both - bc.HOST_ONLY - slab
    assert "gcs_cue_gradient" in want and "gcs_region_tree" in want
    missing, extra = want - set(big.COVERAGE), set(big.COVERAGE) - want
    assert not missing and not extra, (sorted(missing), sorted(extra))
    covered = 0
    for sym, home in big.COVERAGE.items():
        if home.startswith(big.NOT_YET):
            assert len(home) > len(big.NOT_YET) + 10, sym
            continue
        fn = getattr(big, home, None)
        assert home.startswith("test_") and callable(fn), (sym, home)
        assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), (sym, home, "not marked gpu")
        text = inspect.getsource(fn)
        for helper in sorted(set(re.findall(r"\b(_[a-z]\w*)\(", text))):
            if inspect.isfunction(getattr(big, helper, None)):
                text += inspect.getsource(getattr(big, helper))
        assert '"%s"' % sym in text, (sym, home, "the case does not make this call")
        covered += 1
    assert covered >= 24
    doc = big.__doc__
    for sym, home in big.COVERAGE.items():                               # the docstring's "not covered" list is the table's
        if home.startswith(big.NOT_YET):
            assert sym in doc, (sym, "missing from the docstring's list of what is not covered")


def test_one_step_past_each_table_guard_is_refused(built):
    """Part 3 of the GPU file runs the last accepted side of three guards; the first refused side, here, on fake pointers (a refused
    call returns before its first launch): a table stack of 2^30 + 2^16 counters, a leaf table of T + 1 maps, a leaf table of K + 1."""
    import ctypes as C

    import test_gpu_large_maps as big
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)
    t, n = 1 << 14, 256
    assert t * n * n == 1 << 30
    assert lib.gcs_region_counts_batch(p, p, p, t + 1, t + 1, 1, big.H3, big.W3, n, n, p, p, p, None) == big.GCS_EINVAL
    assert lib.gcs_region_counts_batch_u8(p, p, p, t + 1, t + 1, 1, big.H3, big.W3, n, n, p, p, p, None) == big.GCS_EINVAL
    assert lib.gcs_region_agreement(p, p, None, t + 1, n, n, p, p, p, None) == big.GCS_EINVAL
    k, s, ts = big.K_SWEEP, big.TRUTH_SWEEP, big.T_SWEEP
    assert ts * k * s < 1 << 31 <= (ts + 1) * k * s
    assert lib.gcs_region_sweep(p, p, p, p, p, 16, ts + 1, k, s, 2, p, p, p, None) == big.GCS_EINVAL
    assert lib.gcs_region_sweep_under(p, p, p, p, p, 16, ts + 1, k, s, 2, p, p, p, p, None) == big.GCS_EINVAL
    b, kc, c = big.B_CUTS, big.K_CUTS, big.C_CUTS
    assert b * kc * c < 1 << 31 <= b * (kc + 1) * c
    assert lib.gcs_region_props_cuts(p, p, p, p, p, b, big.H3, big.W3, kc + 1, c, 1, 3, p, p, p, None) == big.GCS_EINVAL
    assert lib.gcs_region_paint(p, None, p, b, big.H3, big.W3, kc + 1, kc + 1, c, kc + 1, p, None) == big.GCS_EINVAL
    assert lib.gcs_region_props(p, p, p, b, big.H3, big.W3, c - 6, kc + 1, p, p, None) == big.GCS_EINVAL
