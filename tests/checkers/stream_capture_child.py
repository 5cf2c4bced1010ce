#!/usr/bin/env python3
"""Child process of tests/test_gpu_stream_contract.py::test_capturable_entry_points_replay_on_new_inputs.

For every entry point include/gcs.h calls "(capturable)": the case of the stream-contract table (tests/test_gpu_stream_contract.py)
is called once eagerly, captured on a side stream (``torch.cuda.graph(..., capture_error_mode="thread_local")``), its inputs are
changed to the second valid set and its outputs poisoned, and one replay must give the bytes of the quiet run on that second set.
Then gcs_gabor_features at a size whose eager plan forks onto the library's side stream: the captured plan runs on one stream and
must write the slab the eager forked plan writes, byte for byte.

A capture that fails leaves the capturing thread unable to launch on this runtime, so all of it runs here, where it fails one
test and not the session. Prints ``OK <symbol>`` or ``FAIL <symbol>: <why>`` per entry point; exit status 1 if any failed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]


def main():
    import torch
    import test_gpu_stream_contract as sc
    from stream_order import same

    world = sc.World(torch).build([(sc._slab_cases, ("split",)), (sc._map_cases, ())])
    failed = 0

    def hold(sym, case):
        nonlocal failed
        try:
            if case is None:
                raise AssertionError("its case was not built: %r" % (world.builder_errors,))
            if case.error is not None:
                raise case.error
            got = world.run.capture_run(case)
            for name in case.outputs():
                same(got[name], case.quiet["decoy"][name], (case.name, name, "replay against the quiet run on the second set"))
            world.run.release(case)
            print("OK %s (%s)" % (sym, case.name), flush=True)
        except Exception as e:                                   # one line per symbol, whatever went wrong
            failed += 1
            print("FAIL %s: %s: %s" % (sym, type(e).__name__, " ".join(str(e).split())[:600]), flush=True)

    for sym in sc.CAPTURABLE:
        hold(sym, world.cases.get(sc.TABLE[sym][0]))
    case, _ = sc._fork_case(world.lib)
    case.quiet["decoy"], _ = world.run.quiet_run(case, "decoy")   # the eager plan of this size: forked
    hold("gcs_gabor_features", case)
    torch.cuda.synchronize()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
