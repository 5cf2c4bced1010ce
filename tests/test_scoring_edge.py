"""The scoring mirror against the reference's own metrics class at the edge shapes of tests/golden/scoring_edge_golden.json
(1x70 ... 65x129: single rows and columns, tile and plane-word multiples and their neighbours), raising cases included; and the
GPU scorer's host arithmetic (evaluate_gpu) on the integer counts and tables NumPy / scipy give for the same cases."""
import numpy as np
import pytest

from gabor_color_image_segmentation_amd.evaluate import metrics

import scoring_edge

CASES = scoring_edge.load()


def test_the_fixture_covers_the_shapes_and_both_outcomes():
    shapes = {k.split("/")[0] for k, _, _, _ in CASES}
    assert shapes >= {"1x70", "70x1", "2x2", "3x5", "5x130", "16x64", "17x65", "15x63", "63x127", "64x128", "65x129", "33x193",
                      "48x192"}
    raising = [k for k, _, _, g in CASES if "raises" in g]
    assert len(CASES) == 195 and len(raising) == 54
    for shape in shapes:                                  # per shape: 1, 3 and 9 annotators, labels above 255, the three raising kinds
        keys = [k for k in raising if k.startswith(shape + "/")]
        assert any(k.endswith("/a0") for k in keys) and any(k.endswith("/a3const") for k in keys)
        assert any("/constant/" in k for k in keys)
    for k, lab, truth, g in CASES:
        if "raises" not in g:                             # a score exists only where every annotator map has a boundary
            assert len(truth) in (1, 3, 9) and all(t.min() >= 1 and t.min() != t.max() for t in truth), k
    assert max(int(t.max()) for _, _, t, _ in CASES if len(t)) > 255


@pytest.mark.parametrize("key,lab,truth,ref", CASES, ids=[c[0] for c in CASES])
def test_mirror_equals_the_reference_at_edge_shapes(key, lab, truth, ref):
    m = metrics(None, lab, list(truth))
    if "raises" in ref:
        with pytest.raises(scoring_edge.ERRORS[ref["raises"]]):
            m.set_metrics()
        return
    m.set_metrics()
    got = m.get_metrics()
    assert set(ref) == {"regions", *scoring_edge.EXACT, *scoring_edge.CLOSE}
    assert got["regions"] == ref["regions"]
    for k in scoring_edge.EXACT:
        assert got[k] == ref[k], k                     # same integer counts, same float divisions
    for k in scoring_edge.CLOSE:
        assert got[k] == pytest.approx(ref[k], rel=1e-12), k


@pytest.mark.parametrize("key,lab,truth,ref", CASES, ids=[c[0] for c in CASES])
def test_scorer_host_arithmetic_equals_the_reference_at_edge_shapes(key, lab, truth, ref):
    """The integer counts and tables of the restatements (what the kernels are held to, bit for bit, in test_gpu_scoring_edge.py)
    through the single-image arithmetic (scores_from_counts, region_scores_from_counts) and, as a one-image batch, through the
    batch arithmetic of the batched and resident scorers: the fixture's floats (its own EXACT / CLOSE split), the two forms equal
    to each other; a zero denominator (a constant label map, an annotator map without a boundary, no annotators) raises what the
    reference raised."""
    from gabor_color_image_segmentation_amd import evaluate_gpu as eg
    labs, stack, first, img_of = scoring_edge._assemble([(lab, truth)])
    counts = scoring_edge._np_counts(labs, stack, img_of).astype(np.uint64)
    seg_max, (h, w) = [int(lab.max())], lab.shape
    if "raises" in ref:
        with pytest.raises(scoring_edge.ERRORS[ref["raises"]]):
            eg.scores_from_counts(counts)
        with pytest.raises(scoring_edge.ERRORS[ref["raises"]]):
            eg._batch_scores(counts, seg_max, [{}], first, h * w)
        return
    n_seg, n_truth = seg_max[0] + 1, [int(t.max()) + 1 for t in truth]
    hist, area, perim = scoring_edge._np_tables(lab, truth, n_seg, max(n_truth))
    single = {"regions": n_seg, **eg.scores_from_counts(counts), **eg.region_scores_from_counts(hist, area, perim, n_truth, h, w),
              "density": float(counts[0]) / float(h * w)}
    hist_b, area_b, perim_b = scoring_edge._np_tables_batch(labs, stack, first, n_seg, max(n_truth))
    under, under_np = scoring_edge._np_reduce(hist_b, area_b, img_of)
    reg = eg._region_scores_batch(under.astype(np.uint64), under_np.astype(np.uint64), area_b, perim_b, first, h, w)
    (batch,) = eg._batch_scores(counts, seg_max, reg, first, h * w)
    for got in (single, batch):
        assert got["regions"] == ref["regions"]
        for k in scoring_edge.EXACT:
            assert got[k] == ref[k], k
        for k in scoring_edge.CLOSE:
            assert got[k] == pytest.approx(ref[k], rel=1e-12), k
    for k in scoring_edge.CLOSE:
        assert single[k] == batch[k], k
    assert single["fmeasure"] == batch["fmeasure"]
