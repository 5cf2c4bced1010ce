#!/usr/bin/env python3
"""Writes tests/golden/gabor_plan_table.json: which gabor_mfma_kernel instantiations every Gabor call launches, RECORDED AT A GIVEN
COMMIT (the one before the launch plan moved into csrc/gabor_plan.h), never from the code under test.

    python tests/golden/make_gabor_plan_table.py <commit> [--dump FILE]

The commit is exported into a temporary directory (`git archive`; the working tree is not touched), PATCH below is inserted into its
csrc/gabor.hip in front of the launch sequence - a launch then records the stringified kernel, the template arguments of the
gabor_launch<...> it sits in, its grid, its stream and the level / filter / tile fields of its arguments instead of launching; the
compute-unit count and the side stream are stand-ins the script sets -, the library is built there and gcs_gabor_features is driven
through ctypes with pointers that are never dereferenced. Needs hipcc; needs no GPU.

  plans    {plan: [[n_scales, n_orient, mask], ...]} over n_scales 1..8 x n_orient with n_scales * n_orient <= 70. A plan is the
           ordered bank-kernel launches of one call, "; "-joined, each "<MT,GQ,KS,LVL,FAST,SPLIT> L0:L1 +f0 xG": the instantiation,
           the levels [L0, L1) of its tile list, its first filter and its grid.y. Bit 4 * (ksize == 15) + 2 * (shift != 8) + small
           of the mask is set where the call (ksize <= 13 | 15, shift == 8 | 7, not small | small against 256 compute units) takes
           the plan. Asserted here: every odd ksize of a class, shift 7 and 5, and the shapes 8 x 8, 321 x 481 and 2048 x 2048
           (at batch sizes on the wanted side of the small-call bound; 2048 x 2048 is never small) give the same plan, with and
           without a side stream.
  --dump   also writes every recorded launch of every call (all kernels, grids, tile counts, streams, joins), one call per line, in
           the text format of gcs_selftest_gabor_plan: for comparing two commits by hand.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

PATCH = r'''
#include <tuple>
#include <type_traits>
extern "C" {
char gcs_rec[1 << 16];
int gcs_rec_n = 0, gcs_fake_cu = 256, gcs_fake_side = 0;
}
static void gcs_note_wait(hipStream_t s) {
    if (s != (hipStream_t)16) gcs_rec_n += snprintf(gcs_rec + gcs_rec_n, sizeof gcs_rec - gcs_rec_n, "join\n");
}
template <class... A>
static void gcs_record(const char *kernel, const char *fn, dim3 grid, hipStream_t st, A... a) {
    auto t = std::forward_as_tuple(a...);
    using First = std::decay_t<std::tuple_element_t<0, std::tuple<A...>>>;
    int n = gcs_rec_n;
    n += snprintf(gcs_rec + n, sizeof gcs_rec - n, "%s|%s|%u|%u|%d", kernel, fn, grid.x, grid.y, st == (hipStream_t)16 ? 1 : 0);
    if constexpr (std::is_same<First, GaborLevels>::value) {
        const GaborLevels &G = std::get<0>(t);
        int nl = 0;
        while (nl < GCS_LEVELS_MAX && G.lv[nl].tile_end != 0x7fffffff) ++nl;
        n += snprintf(gcs_rec + n, sizeof gcs_rec - n, "|%d|%d|%d|%d", G.lv[0].L, G.lv[0].L + nl, (int)std::get<2>(t), (int)std::get<5>(t));
    } else if constexpr (std::is_same<First, StripArgs>::value) {
        const StripArgs &S = std::get<0>(t);
        n += snprintf(gcs_rec + n, sizeof gcs_rec - n, "|%d|%d|0|%d", S.lv[0].L, S.lv[0].L + S.n_levels, (int)std::get<4>(t));
    }
    n += snprintf(gcs_rec + n, sizeof gcs_rec - n, "\n");
    gcs_rec_n = n;
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, st, ...) gcs_record(#kernel, __PRETTY_FUNCTION__, grid, st, __VA_ARGS__)
#define gcs_cu_count() gcs_fake_cu
#define hipGetLastError() hipSuccess
#define hipStreamIsCapturing(s, p) (*(p) = hipStreamCaptureStatusNone, hipSuccess)
#define hipGetDevice(p) (gcs_fake_side ? (*(p) = 0, hipSuccess) : hipErrorNoDevice)
#define hipStreamCreateWithFlags(p, f) (*(p) = (hipStream_t)16, hipSuccess)
#define hipEventCreateWithFlags(p, f) (*(p) = (hipEvent_t)16, hipSuccess)
#define hipEventRecord(e, s) hipSuccess
#define hipStreamWaitEvent(s, e, f) (gcs_note_wait(s), hipSuccess)
'''
ANCHOR = '// ------------------------------------------------------------------------------ workspace\n'
HERE = os.path.dirname(os.path.abspath(__file__))
CU = 256
KSIZES = {0: (1, 3, 5, 7, 9, 11, 13), 1: (15,)}
SHIFTS = {0: (8,), 1: (7, 5)}
# (H, W): (a batch that is not small for any bank of the domain, one that is small for every bank; None: no such batch)
SHAPES = {(8, 8): (300, 1), (321, 481): (16, 1), (2048, 2048): (1, None)}


def banks():
    return [(ns, no) for ns in range(1, 9) for no in range(1, 71) if ns * no <= 70]


def launches(text):
    """The recorded launches of one call -> the text lines of gcs_selftest_gabor_plan."""
    out, join, deep = [], 0, 1
    for line in text.splitlines():
        if line == "join":
            join = 1
            continue
        f = line.split("|")
        kern = f[0].strip("()").replace(" ", "")
        gx, gy, side = int(f[2]), int(f[3]), int(f[4])
        if kern.startswith("gabor_mfma_kernel"):
            m = re.search(r"MT = (\d+), GQ = (\d+), KS = (\d+), LV = (-?\d+), FA = (true|false)", f[1])
            split = re.fullmatch(r"gabor_mfma_kernel<MT,GQ,KS,LV,FA,(true|false)>", kern).group(1)
            kern = "gabor_mfma_kernel<%s,%s,%s,%s,%s,%s>" % (m.group(1), m.group(2), m.group(3), m.group(4), m.group(5), split)
            l0, l1, f0, tiles = map(int, f[5:9])
        elif kern.startswith("gabor_strip_kernel"):
            l0, l1, f0, tiles = map(int, f[5:9])
        else:
            f0 = tiles = 0
            if kern == "gabor_plane_kernel<0>":
                l0, l1 = 0, 1
            elif kern == "gabor_pre01_kernel":
                l0, l1 = 0, 2
            elif kern == "gabor_down_kernel<true>":
                l0, l1 = 1, 2
            else:
                assert kern == "gabor_down_kernel<false>", kern
                deep += 1
                l0, l1 = deep, deep + 1
        out.append("%s levels=%d:%d f0=%d grid=%dx%d tiles=%d stream=%s join=%d" %
                   (kern, l0, l1, f0, gx, gy, tiles, "side" if side else "main", join))
        join = 0
    return out


def plan_key(lines):
    """The shape-independent part of the bank-kernel launches of a call (see `plans` above)."""
    out = []
    for line in lines:
        m = re.match(r"gabor_mfma_kernel(<[^>]*>) levels=(\d+:\d+) f0=(\d+) grid=\d+x(\d+) ", line)
        if m:
            out.append("%s %s +%s x%s" % m.groups())
    return "; ".join(out)


def record(lib, dump=None):
    rec = (C.c_char * (1 << 16)).in_dll(lib, "gcs_rec")
    rec_n, side, cu = (C.c_int.in_dll(lib, n) for n in ("gcs_rec_n", "gcs_fake_side", "gcs_fake_cu"))
    cu.value = CU
    fake = C.c_void_p(4096)

    def call(b, h, w, ns, no, ks, shift, forked):
        rec_n.value, side.value = 0, forked
        rc = lib.gcs_gabor_features(fake, b, h, w, fake, fake, ns, no, ks, shift, fake, fake, None)
        assert rc == 0, (b, h, w, ns, no, ks, shift, rc)
        lines = launches(rec.raw[:rec_n.value].decode())
        if dump:
            dump.write("%s %s\n" % ((b, h, w, ns, no, ks, shift, CU, forked), " | ".join(lines)))
        return lines

    plans = {}
    for ns, no in banks():
        for ksc in (0, 1):
            for sh in (0, 1):
                for small in (0, 1):
                    got = set()
                    for (h, w), batch in SHAPES.items():
                        if batch[small] is None:
                            continue
                        for ks in KSIZES[ksc]:
                            for shift in SHIFTS[sh]:
                                for forked in (0, 1):
                                    lines = call(batch[small], h, w, ns, no, ks, shift, forked)
                                    assert any(" stream=side " in l for l in lines) == bool(
                                        forked and 3 <= ns <= 4 and batch[small] * h * w >= 1 << 21), (lines, ns, no, h, w)
                                    got.add(plan_key(lines))
                    assert len(got) == 1, (ns, no, ksc, sh, small, got)
                    rows = plans.setdefault(got.pop(), {})
                    rows[ns, no] = rows.get((ns, no), 0) | 1 << (4 * ksc + 2 * sh + small)
    return {k: [[ns, no, m] for (ns, no), m in sorted(v.items())] for k, v in sorted(plans.items())}


def main():
    commit = sys.argv[1]
    dump = open(sys.argv[sys.argv.index("--dump") + 1], "w") if "--dump" in sys.argv else None
    root = os.path.dirname(os.path.dirname(HERE))
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", root, "archive", commit], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        csrc = os.path.join(tmp, "gabor_color_image_segmentation_amd", "csrc")
        src = open(os.path.join(csrc, "gabor.hip")).read()
        assert src.count(ANCHOR) == 1
        open(os.path.join(csrc, "gabor.hip"), "w").write(src.replace(ANCHOR, ANCHOR + PATCH))
        subprocess.run(["make", "-s", "-j4", "all"], cwd=csrc, check=True)
        plans = record(C.CDLL(os.path.join(csrc, "libgcs.so")), dump)
    out = {"commit": subprocess.run(["git", "-C", root, "rev-parse", commit], check=True, stdout=subprocess.PIPE,
                                    text=True).stdout.strip(), "cu_count": CU, "plans": plans}
    with open(os.path.join(HERE, "gabor_plan_table.json"), "w") as f:
        f.write('{\n"commit": %s,\n"cu_count": %d,\n"plans": {\n' % (json.dumps(out["commit"]), CU))
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in plans.items()))
        f.write("\n}\n}\n")


if __name__ == "__main__":
    main()
