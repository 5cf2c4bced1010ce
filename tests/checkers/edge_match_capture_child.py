#!/usr/bin/env python3
"""Child process of tests/test_gpu_edge_match.py::test_capture_and_replay_on_other_inputs.

gcs_edge_match and gcs_truth_thin (include/gcs_match.h calls them capturable): the case of tests/test_gpu_edge_match.py
(``stream_cases``) is called once eagerly, captured on a side stream, its inputs are changed to the second valid set and its
outputs poisoned, and one replay must give the bytes of the quiet run on that second set.

A capture that fails leaves the capturing thread unable to launch on this runtime, so it runs here, where it fails one test and
not the session. Prints ``OK <symbol>`` or ``FAIL <symbol>: <why>`` per entry point; exit status 1 if any failed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]


def main():
    import torch
    import test_gpu_edge_match as tm
    from gabor_color_image_segmentation_amd import _lib
    from stream_order import Runner, same

    lib = _lib.load()
    run = Runner(torch, lib)
    failed = 0
    for case in tm.stream_cases(lib):
        sym = case.symbols[0]
        try:
            case.quiet["decoy"], _ = run.quiet_run(case, "decoy")
            got = run.capture_run(case)
            for name in case.outputs():
                same(got[name], case.quiet["decoy"][name], (case.name, name, "replay against the quiet run on the second set"))
            run.release(case)
            print("OK %s (%s)" % (sym, case.name), flush=True)
        except Exception as e:                                   # one line per symbol, whatever went wrong
            failed += 1
            print("FAIL %s: %s: %s" % (sym, type(e).__name__, " ".join(str(e).split())[:600]), flush=True)
    torch.cuda.synchronize()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
