#!/usr/bin/env python3
"""Writes tests/golden/pass_kernel_table.json: which Lloyd-pass kernel every (bank, k) takes and what every refused call answers,
RECORDED AT A GIVEN COMMIT (the one before the choice moved into csrc/lloyd_pass.h), never from the code under test.

    python tests/golden/make_pass_kernel_table.py <commit>

The commit is exported into a temporary directory (`git archive`; the working tree is not touched), PATCH below is inserted
behind the includes of its csrc/kmeans.hip - a launch then records the stringified kernel instead of launching -, the library
is built there and driven through ctypes with pointers that are never dereferenced. Needs hipcc; needs no GPU.

  choice   {display name: [[n_scales, n_orient, mask of k (bit k - 1)], ...]} over n_scales 1..8 x n_orient 1..70 x k 1..16, equal
           (asserted here) for the shapes 8 x 8, 321 x 481 and 2048 x 2048; "refused": the call fails and launches nothing.
  fused    [[n_scales, n_orient, mask of k]] where gcs_kmeans_fused_workspace_bytes != 0 (equal for n_sets = 1 and B, asserted)
  errors   [{fn, args, rc, message}]: bad-argument calls ("P" = a non-NULL pointer, null = NULL) of the three pass entry points
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

PATCH = r'''
#undef hipLaunchKernelGGL
extern "C" { const char *gcs_recorded_launch = nullptr; }
#define hipLaunchKernelGGL(kernel, ...) (void)(gcs_recorded_launch = #kernel)
#define hipFuncSetAttribute(...) hipSuccess
#define hipGetLastError() hipSuccess
'''
ANCHOR = '#include <type_traits>\n'
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(8, 8), (321, 481), (2048, 2048)]
P = "P"


def display_name(rec):
    """'(kmeans_pass_mfma_kernel<1, 3, KP_DSTEPS_NARROW, 4, true , 2>)' -> 'split<1,3,2>' (the names tests/test_gpu_value_range.py uses)"""
    if rec is None:
        return "refused"
    m = re.fullmatch(r"\(?(\w+)<(.*)>\)?", rec.replace(" ", ""))
    kern, a = m.group(1), m.group(2).split(",")
    if kern == "kmeans_assign_kernel":
        return "generic"
    if kern == "kmeans_pass_native_kernel":
        return "native<%s>" % ",".join(a)
    assert kern == "kmeans_pass_mfma_kernel" and a[2] in ("KP_DSTEPS_NARROW", "KP_DSTEPS_WIDE"), rec
    if len(a) > 4:
        assert a[2:5] == ["KP_DSTEPS_NARROW", "4", "true"] and len(a) <= 6, rec
        return "split<%s>" % ",".join(a[:2] + a[5:])
    if a[2] == "KP_DSTEPS_NARROW":
        assert a[3] == "4", rec
        return "narrow<%s,%s>" % (a[0], a[1])
    return ("wide8w<%s,%s>" if a[3] == "8" else "wide<%s,%s>") % (a[0], a[1])


def error_cases():
    """(fn, args): every rule of lloyd_pass and of gcs_kmeans_pass_fused; all return before any launch."""
    def acc(feats=P, cent=P, B=2, H=40, W=56, ns=4, no=6, k=8, n_sets=1, row_lo=0, row_hi=None, labels=P, partials=P):
        return ("gcs_kmeans_assign_accumulate",
                [feats, cent, B, H, W, ns, no, k, n_sets, row_lo, H if row_hi is None else row_hi, 0, labels, partials, None])

    def ras(feats=P, cent=P, B=2, H=40, W=56, ns=4, no=6, k=8, n_sets=1, out=P, out_u8=0, scratch=None):
        return ("gcs_kmeans_assign_raster", [feats, cent, B, H, W, ns, no, k, n_sets, 0, out, out_u8, scratch, None])

    def fus(feats=P, B=2, H=40, W=56, ns=4, no=6, k=8, n_sets=1, pas=0, last=0, ws=P, cent=P, out=None):
        return ("gcs_kmeans_pass_fused", [feats, B, H, W, ns, no, k, n_sets, 0, pas, last, ws, cent, out, 0, None])

    cases = [acc(feats=None), acc(cent=None), acc(labels=None, partials=None),
             acc(B=0), acc(B=-1), acc(H=0), acc(W=0), acc(ns=0), acc(ns=9), acc(no=0), acc(no=30000),
             acc(H=30000, W=30000),                                  # a split slab of more than 4 GB per image
             acc(row_lo=-1), acc(row_hi=41), acc(row_lo=5, row_hi=5), acc(row_lo=6, row_hi=5),
             acc(B=65536, H=8, W=8), acc(B=65535, H=2048, W=2048), acc(B=65535, H=2048, W=2048, ns=8, no=8),
             acc(k=0), acc(k=17), acc(k=-3), acc(B=3, n_sets=2), acc(B=3, n_sets=0),
             acc(ns=8, no=70, k=16), acc(ns=8, no=70, k=13),   # generic pass: k * D and the LDS
             ras(out=None), ras(feats=None), ras(cent=None), ras(B=0), ras(k=0), ras(k=17), ras(B=3, n_sets=2),
             ras(B=65536, H=8, W=8), ras(B=65535, H=2048, W=2048),
             ras(ns=7, no=10), ras(ns=7, no=10, k=16),                # D >= 208, an int32 map and no scratch label map
             fus(feats=None), fus(ws=None), fus(cent=None), fus(last=1, out=None), fus(B=0), fus(H=0), fus(ns=9), fus(no=0),
             fus(pas=-1), fus(ns=8, no=8), fus(k=9), fus(k=16), fus(k=0), fus(k=17), fus(B=3, n_sets=2), fus(ns=5, no=5),
             fus(ns=2, no=13), fus(ns=7, no=10), fus(B=65536, H=8, W=8), fus(B=65535, H=2048, W=2048)]
    return cases


def main():
    commit = sys.argv[1]
    root = os.path.dirname(os.path.dirname(HERE))
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", root, "archive", commit], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        csrc = os.path.join(tmp, "gabor_color_image_segmentation_amd", "csrc")
        src = open(os.path.join(csrc, "kmeans.hip")).read()
        assert src.count(ANCHOR) == 1
        open(os.path.join(csrc, "kmeans.hip"), "w").write(src.replace(ANCHOR, ANCHOR + PATCH))
        subprocess.run(["make", "-s", "-j4", "all"], cwd=csrc, check=True)
        lib = C.CDLL(os.path.join(csrc, "libgcs.so"))
        out = record(lib)
    out["commit"] = subprocess.run(["git", "-C", root, "rev-parse", commit], check=True, stdout=subprocess.PIPE,
                                   text=True).stdout.strip()
    with open(os.path.join(HERE, "pass_kernel_table.json"), "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(out[k], separators=(",", ":"))) for k in
                                   ("commit", "choice", "fused", "errors")) + "\n}\n")


def record(lib):
    rec = C.c_char_p.in_dll(lib, "gcs_recorded_launch")
    fake = C.c_void_p(4096)
    lib.gcs_last_error.restype = C.c_char_p
    lib.gcs_kmeans_fused_workspace_bytes.restype = C.c_size_t

    def call(fn, args):
        rec.value = None
        rc = getattr(lib, fn)(*[fake if a == P else C.c_void_p(None) if a is None else C.c_int(a) for a in args])
        return rc, rec.value.decode() if rec.value else None

    choice, fused = {}, []
    for ns in range(1, 9):
        for no in range(1, 71):
            names, fmask = {}, 0
            for k in range(1, 17):
                got = set()
                for h, w in SHAPES:
                    rc, r = call("gcs_kmeans_assign_accumulate", [P, P, 1, h, w, ns, no, k, 1, 0, h, 0, P, P, None])
                    assert (rc == 0) == (r is not None), (ns, no, k, rc, r)
                    got.add(display_name(r))
                    ws = {lib.gcs_kmeans_fused_workspace_bytes(b, h, w, ns, no, k, n) != 0 for b, n in ((1, 1), (3, 1), (3, 3))}
                    got.add(("fused", ws.pop()))
                    assert not ws
                assert len(got) == 2, (ns, no, k, got)                # the same for every shape
                for g in got:
                    if isinstance(g, tuple):
                        fmask |= int(g[1]) << (k - 1)
                    else:
                        names[g] = names.get(g, 0) | 1 << (k - 1)
            for name, mask in names.items():
                choice.setdefault(name, []).append([ns, no, mask])
            if fmask:
                fused.append([ns, no, fmask])
    errors = []
    for fn, args in error_cases():
        rc, r = call(fn, args)
        assert rc != 0 and r is None, (fn, args, rc, r)
        errors.append({"fn": fn, "args": args, "rc": rc, "message": lib.gcs_last_error().decode()})
    return {"choice": choice, "fused": fused, "errors": errors}


if __name__ == "__main__":
    main()
