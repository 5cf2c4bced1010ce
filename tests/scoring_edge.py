"""The edge-shape scoring fixture (tests/golden/make_scoring_edge_golden.py), for the host and the GPU tests: label maps and
annotator stacks at shapes around the scorer's 16 x 64 tiles and 64-bit plane words, with the reference class's own numbers."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EXACT = ("recall", "precision", "density")                       # tests/test_evaluate.py: same integer counts, same divisions
CLOSE = ("underseg", "undersegNP", "compactness")                # rel 1e-12 there
ERRORS = {"ZeroDivisionError": ZeroDivisionError, "ValueError": ValueError}


def load():
    """[(key, label map int32 (H,W), annotator maps uint16 [A][H][W] (A may be 0), golden dict)] in key order."""
    maps = np.load(os.path.join(GOLD, "scoring_edge_maps.npz"))
    gold = json.load(open(os.path.join(GOLD, "scoring_edge_golden.json")))
    out = []
    for key in sorted(gold):
        shape, kind, stack = key.split("/")
        lab = maps["lab_%s_%s" % (shape, kind)].astype(np.int32)
        truth = np.zeros((0,) + lab.shape, np.uint16) if stack == "a0" else maps["truth_%s_%s" % (shape, stack)]
        out.append((key, lab, truth, gold[key]))
    return out
