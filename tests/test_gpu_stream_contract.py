"""The stream contract of include/gcs.h ("Streams"), entry point by entry point, on the raw C calls: work is ordered on the caller's
stream alone, and no call waits on the host. The harness is tests/stream_order.py; this file holds the table.

Every case runs three ways. QUIET: on the default stream, synchronised on either side, on the true inputs - held to the entry
point's existing reference (the C oracle, tests/lloyd_ref.py, tests/smooth_ref.py, tests/position_ref.py, the region, scoring and
gradient restatements) - and on the decoys, whose outputs must differ from the true ones in every output buffer (else the case
proves nothing). LATE: on a fresh side stream behind a gate; the inputs hold their decoys until a copy enqueued behind the gate
puts the true bytes in place, and hold them again behind the clones of the outputs; the call must return while the gate still
runs, and the clones must equal the quiet run in every byte. CAPTURED (the entry points the header calls "(capturable)", in one
child process, tests/checkers/stream_capture_child.py): one eager call, the call captured on a side stream, the inputs changed to
the decoys, the outputs poisoned, one replay == the quiet run on the decoys. Opaque outputs (a slab, partial sums, bit planes) are
held to a reference through the case that consumes them: its true input IS that output.

Decoys are legal inputs of the same shape (other images, another hot bank, label maps in range, valid trees, decreasing cut
lists): a mis-ordered run computes on valid memory and can only give wrong bytes.

Measured on an MI355X (the whole file: 113 tests in 13.7 s). Gate G: 50.0 ms asked for (the 50 ms floor: 20 times the longest
enqueue is 3.5 ms), 56.9 - 57.7 ms measured per run. Host-side enqueue of the quiet runs: longest 0.148 - 0.176 ms (region_nodes,
merge_small_regions: their rounds are many launches), median 0.005 ms, gcs_gabor_features at the forked size 0.09 - 0.10 ms. Host time of
a late run from the gate's enqueue to the call's return, input copies included: 0.06 - 0.14 ms, longest 0.53 ms (download). Seconds
per part: building the table with its quiet runs and references 2.2 - 2.9 (once, in the first test's setup); a late case 0.06 - 0.07
each (95 of them); the forked Gabor case on six streams 1.1; a Python-layer method below 0.07, the resident scorer 0.13; the capture
child 2.9 - 3.3. Findings: none - no entry point waited, ran out of order or refused capture.

What the harness had to learn from its mutants: the runtime spreads streams over a few hardware queues, and a launch that strays
onto the null stream is in order by accident when that stream shares the gated stream's queue (``Runner.side_stream`` picks a
stream that does not; the forked Gabor case runs on six consecutive streams because the library's side stream shares a queue with
some); and a zeroing that strays runs EARLY, harmlessly, unless the outputs' entry contents are written once more behind the gate."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import stream_order as so_
from stream_order import Case, inplace, late, out, same, scratch, view

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

B = 3
SLAB_SHAPE = (33, 41)        # packed strips on the two-level banks, more than one tile, no multiple of 8
MAP_SHAPE = (37, 53)         # the largest map of tests/test_gpu_buffer_contracts.py
SCORE_SHAPE = (13, 65)       # its scoring shape with a word boundary inside a row
K_TREE = 33
BANKS = {"split": (4, 6, 13, 8), "wide": (4, 7, 13, 7), "deep": (8, 8, 13, 8), "generic": (7, 10, 13, 7)}
LLOYD_K = {"split": (3, 9), "wide": (3, 9), "deep": (3, 9), "generic": (3,)}    # one k per form gcs_selftest_pass_kernel names
FORK_STREAMS = 6
FORK_BATCH, FORK_SHAPE = 128, (130, 129)                                         # 2.15 M pixels >= GCS_GABOR_FORK_MIN_PIXELS

# ---- the table: symbol -> the cases (names of NAMES) whose call makes it
SLAB_SYMBOLS = ("gcs_gabor_features", "gcs_features_unpack", "gcs_features_gather", "gcs_smooth_features", "gcs_position_features",
                "gcs_kmeans_init")
LLOYD_SYMBOLS = ("gcs_kmeans_assign_accumulate", "gcs_kmeans_assign_raster", "gcs_kmeans_reduce", "gcs_kmeans_finalize",
                 "gcs_kmeans_reduce_finalize")
MAP_SYMBOLS = ("gcs_connected_regions", "gcs_merge_small_regions", "gcs_region_nodes", "gcs_region_tree", "gcs_region_tree_cut",
               "gcs_region_tree_contours", "gcs_truth_prepare", "gcs_boundary_sweep_resident", "gcs_texton_gradient",
               "gcs_cue_gradient", "gcs_colour_opponent", "gcs_superpixel_segment", "gcs_region_sweep", "gcs_region_sweep_under",
               "gcs_cut_shapes", "gcs_region_props", "gcs_region_props_cuts", "gcs_region_paint", "gcs_region_adjacency",
               "gcs_region_adjacency_cuts", "gcs_region_tree_edges", "gcs_label_used", "gcs_selftest_isqrt", "gcs_download")
SCORE_SYMBOLS = ("gcs_boundary_counts", "gcs_region_counts", "gcs_boundary_counts_batch", "gcs_boundary_counts_resident",
                 "gcs_region_counts_batch", "gcs_region_counts_batch_u8", "gcs_region_reduce", "gcs_score_batch_resident",
                 "gcs_region_agreement")


def _short(sym):
    return sym[len("gcs_"):]


def _table():
    t = {}
    for sym in SLAB_SYMBOLS:
        t[sym] = ["%s:%s" % (bank, _short(sym)) for bank in BANKS]
    for sym in ("gcs_feature_gradient", "gcs_region_tree_slab"):                 # D <= 207
        t[sym] = ["%s:%s" % (bank, _short(sym)) for bank in BANKS if bank != "generic"]
    for sym in LLOYD_SYMBOLS:
        t[sym] = ["%s:%s k=%d" % (bank, _short(sym), k) for bank in BANKS for k in LLOYD_K[bank]]
    t["gcs_labels_widen"] = ["split:labels_widen"]
    t["gcs_kmeans_pass_fused"] = ["split:kmeans_pass_fused"]
    for sym in MAP_SYMBOLS + SCORE_SYMBOLS:
        t[sym] = [_short(sym)]
    t["gcs_region_tree_cut"] = ["region_tree_cut", "region_tree_cut in place"]
    return t


TABLE = _table()
NAMES = sorted({name for names in TABLE.values() for name in names})
# the entry points whose header text says "(capturable)"
CAPTURABLE = ("gcs_region_nodes", "gcs_smooth_features", "gcs_colour_opponent", "gcs_position_features", "gcs_superpixel_segment",
              "gcs_region_tree", "gcs_region_tree_slab", "gcs_region_tree_contours", "gcs_boundary_sweep_resident", "gcs_region_sweep",
              "gcs_region_sweep_under", "gcs_cut_shapes", "gcs_region_props", "gcs_region_props_cuts", "gcs_region_paint",
              "gcs_region_adjacency", "gcs_region_adjacency_cuts", "gcs_feature_gradient", "gcs_region_tree_edges", "gcs_label_used",
              "gcs_texton_gradient", "gcs_cue_gradient")


def _headers():
    return "".join(open(os.path.join(ROOT, "include", name)).read() for name in ("gcs.h", "gcs_cues.h"))


def _stream_takers():
    """The functions of the two headers whose prototype takes a gcs_stream_t."""
    return _takers_of(re.sub(r"/\*.*?\*/", "", _headers(), flags=re.S))


def _takers_of(code):
    """(comments taken out) -> the functions whose prototype ends in a gcs_stream_t."""
    return set(re.findall(r"\b(gcs_\w+)\s*\([^;(){}]*gcs_stream_t stream\);", code))


def test_the_table_names_every_entry_point_that_takes_a_stream():
    """CPU: the table's symbols are exactly the functions of include/*.h that take a gcs_stream_t, which are CONTRACT + ELSEWHERE of
    tests/test_gpu_buffer_contracts.py (gcs_cue_gradient of ``_lib.EXTENSIONS`` among them) and the symbols of ``_lib.SIGNATURES`` and
    ``_lib.EXTENSIONS`` whose last argument is a pointer and that are not host only; every case
    named exists in NAMES; the builder of every case makes the call. A new entry point fails here until it has a case."""
    import test_gpu_buffer_contracts as bc
    from gabor_color_image_segmentation_amd import _lib
    takers = _stream_takers()
    assert takers == set(bc.CONTRACT) | set(bc.ELSEWHERE) and "gcs_cue_gradient" in takers
    both = dict(_lib.SIGNATURES, **_lib.EXTENSIONS)
    assert takers <= set(both) and all(both[s][1][-1] is ctypes.c_void_p for s in takers)
    assert takers == set(both) - bc.HOST_ONLY                                    # every device entry point of either table
    missing, extra = takers - set(TABLE), set(TABLE) - takers
    assert not missing and not extra, (sorted(missing), sorted(extra))
    text = open(os.path.abspath(__file__)).read()
    for sym, names in TABLE.items():
        assert names and set(names) <= set(NAMES), (sym, names)
        assert re.search(r"lib\.%s\(" % sym, text), (sym, "no builder of this file makes the call")
    without = dict(TABLE)                                                        # the check has teeth: a symbol taken out is missed
    without.pop("gcs_label_used")
    assert takers - set(without) == {"gcs_label_used"}


def test_capturable_is_what_the_headers_say():
    """CPU: every comment of the headers that says "(capturable)" belongs to entry points of CAPTURABLE, and every entry point of
    CAPTURABLE lies in or behind such a comment (the comment in front of its prototype, or of its group's)."""
    text = _headers()
    assert set(CAPTURABLE) <= _stream_takers()
    pieces = re.split(r"(/\*.*?\*/)", text, flags=re.S)          # comments at odd indices, the code behind each at even ones
    said = set()
    for i in range(1, len(pieces), 2):
        if "(capturable)" in pieces[i]:
            said |= _takers_of(pieces[i + 1])
    assert said, "no comment says (capturable)"
    # a group comment names which of its functions are capturable: gcs_region_tree_cut shares gcs_region_tree's comment without the
    # word on its own line, and the size functions take no stream
    assert set(CAPTURABLE) <= said, sorted(set(CAPTURABLE) - said)
    assert said - set(CAPTURABLE) <= {"gcs_region_tree_cut"}, sorted(said - set(CAPTURABLE))


def test_lloyd_cases_cover_every_pass_kernel_form():
    """CPU: at the slab shape, the k of LLOYD_K reach every form gcs_selftest_pass_kernel names for the four banks."""
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    h, w = SLAB_SHAPE
    seen = set()
    for bank, (ns, no, _, _) in BANKS.items():
        forms = {lib.gcs_selftest_pass_kernel(h, w, ns, no, k) for k in range(2, 17)}
        mine = {lib.gcs_selftest_pass_kernel(h, w, ns, no, k) for k in LLOYD_K[bank]}
        assert None not in forms and forms == mine, (bank, forms, mine)
        seen |= {f.decode().split("<")[0] for f in forms}
    assert seen == {"split", "native", "wide", "generic"}, seen
    assert lib.gcs_kmeans_fused_workspace_bytes(B, h, w, 4, 6, 3, B) > 0


# ------------------------------------------------------------------------------------------------------------ plumbing
def _ok(lib, rc, what):
    assert rc == 0, (what, lib.gcs_last_error())


class World:
    """Every case of the table, built once per module: the quiet runs (decoys first: they also warm every kernel up, so that the
    timed enqueue of the true run is an enqueue and not a code-object load), the references, the gate."""

    def __init__(self, torch):
        from gabor_color_image_segmentation_amd import _lib
        self.torch, self.lib = torch, _lib.load()
        self.run = so_.Runner(torch, self.lib)
        self.cases, self.builder_errors = {}, {}

    def add(self, case):
        assert case.name in NAMES and case.name not in self.cases, case.name
        for sym in case.symbols:
            assert case.name in TABLE[sym], (case.name, sym)
        self.cases[case.name] = case
        case.quiet["decoy"], _ = self.run.quiet_run(case, "decoy")
        case.quiet["true"], case.enqueue_s = self.run.quiet_run(case, "true")
        self.run.release(case)
        try:
            case.check(case.quiet["true"])
            for name in case.outputs():
                if name not in case.free_outputs:
                    assert not np.array_equal(case.quiet["true"][name], case.quiet["decoy"][name]), (
                        case.name, name, "the decoys give the same output: the case proves nothing")
        except AssertionError as e:
            case.error = e
        return case

    def build(self, builders):
        for fn, args in builders:
            try:
                fn(self, *args)
            except Exception as e:                                   # a builder that stops leaves its later cases unbuilt
                self.builder_errors[(fn.__name__,) + tuple(args)] = e
        self.run.calibrate()
        self.run.settle([c.enqueue_s for c in self.cases.values()])
        return self

    def canonical(self, cfg, slab_bytes, b, h, w):
        """gcs_features_unpack of slab bytes, quietly -> (B, D, H, W) uint16."""
        t, lib = self.torch, self.lib
        ns, no = cfg[:2]
        slab = t.from_numpy(np.ascontiguousarray(slab_bytes)).cuda()
        canon = t.empty(b * 3 * ns * no * h * w * 2, dtype=t.uint8, device="cuda")
        _ok(lib, lib.gcs_features_unpack(slab.data_ptr(), b, h, w, ns, no, canon.data_ptr(), t.cuda.current_stream().cuda_stream), "unpack")
        t.cuda.synchronize()
        return canon.cpu().numpy().view(np.uint16).reshape(b, 3 * ns * no, h, w)


def _pack(lib, tapq, ns, no, ks):
    tapq = np.ascontiguousarray(tapq, np.int16)
    packed = np.zeros(lib.gcs_bank_packed_bytes(ns, no), np.int8)
    bias = np.zeros(lib.gcs_bank_bias_count(ns, no), np.int32)
    _ok(lib, lib.gcs_bank_pack(tapq.ctypes.data, ns, no, ks, packed.ctypes.data, bias.ctypes.data), "gcs_bank_pack")
    return packed, bias


def _maybe_late(true, decoy):
    """``late``, for an input whose two legal contents may coincide (the bias words of two hot banks)."""
    if np.array_equal(so_.raw(true), so_.raw(decoy)):
        buf = so_.Buf("in", so_.raw(true).size, so_.raw(true), so_.raw(decoy))
        return buf
    return late(true, decoy)


def _gabor_case(lib, name, cfg, imgs_t, imgs_d):
    import hot_banks as hb
    ns, no, ks, shift = cfg
    b, h, w = imgs_t.shape[:3]
    pk_t, bi_t = _pack(lib, hb.hot_bank(*cfg).tapq, ns, no, ks)
    pk_d, bi_d = _pack(lib, hb.hot_bank(*cfg, odd="turned").tapq, ns, no, ks)
    bufs = dict(img=late(imgs_t, imgs_d), packed=late(pk_t, pk_d), bias=_maybe_late(bi_t, bi_d),
                ws=scratch(lib.gcs_gabor_workspace_bytes(b, h, w, ns)), slab=out(lib.gcs_feature_slab_bytes(b, h, w, ns, no)))

    def call(lib, p, st):
        _ok(lib, lib.gcs_gabor_features(p["img"], b, h, w, p["packed"], p["bias"], ns, no, ks, shift, p["ws"], p["slab"], st), name)
    return Case(name, ["gcs_gabor_features"], bufs, call, lambda o: None)        # the slab is held to the oracle by the unpack case


# ------------------------------------------------------------------------------------------------------------ slab stages
def _slab_cases(w, bank):
    import feature_gradient_ref as fg
    import hot_banks as hb
    import position_ref as pr
    import region_tree_ref as rt
    import smooth_ref as sr
    import test_gpu_buffer_contracts as bc
    from fused_stages import ref_features
    from lloyd_ref import _pass_reference, updated
    from oracle import spec_oracle as so
    lib = w.lib
    cfg = BANKS[bank]
    ns, no, ks, shift = cfg
    d = 3 * ns * no
    b, (h, wd) = B, SLAB_SHAPE
    p_ = h * wd
    imgs_t = hb.hot_images(b, h, wd, seed=h * wd)
    imgs_d = np.ascontiguousarray(hb.hot_images(8, h, wd, seed=5)[[4, 6, 7]])                  # stripes at 90 and 135 degrees, noise
    ref = ref_features(cfg, imgs_t)                                                            # (B, D, H, W) uint16, the C oracle
    x = ref.reshape(b, d, -1).transpose(0, 2, 1).astype(np.int64)                              # (B, P, D)
    nm = lambda sym, k=None: "%s:%s" % (bank, _short(sym)) + ("" if k is None else " k=%d" % k)

    g = w.add(_gabor_case(lib, nm("gcs_gabor_features"), cfg, imgs_t, imgs_d))
    slab_t, slab_d = g.quiet["true"]["slab"], g.quiet["decoy"]["slab"]
    slab = lambda: late(slab_t, slab_d)

    def call(lib, p, st):
        _ok(lib, lib.gcs_features_unpack(p["slab"], b, h, wd, ns, no, p["canon"], st), "gcs_features_unpack")
    w.add(Case(nm("gcs_features_unpack"), ["gcs_features_unpack"], dict(slab=slab(), canon=out(ref.nbytes)), call,
               lambda o: same(view(o["canon"], np.uint16, ref.shape), ref, (bank, "gcs_gabor_features -> gcs_features_unpack"))))

    n = 37
    byx = {}
    for key, seed in (("t", 1), ("d", 2)):
        rng = np.random.default_rng(seed)
        byx[key] = np.stack([rng.integers(-1, b, n), rng.integers(0, h, n), rng.integers(0, wd, n)], 1).astype(np.int32)
    want_rows = np.where(byx["t"][:, :1] >= 0, ref[np.maximum(byx["t"][:, 0], 0), :, byx["t"][:, 1], byx["t"][:, 2]], 0)

    def call(lib, p, st):
        _ok(lib, lib.gcs_features_gather(p["slab"], b, h, wd, ns, no, n, p["byx"], p["rows"], st), "gcs_features_gather")
    w.add(Case(nm("gcs_features_gather"), ["gcs_features_gather"], dict(slab=slab(), byx=late(byx["t"], byx["d"]), rows=out(n * d * 2)),
               call, lambda o: same(view(o["rows"], np.uint16, (n, d)), want_rows, (bank, "gcs_features_gather"))))

    if d <= 207:
        want_grad = np.stack([fg.gradient(ref[i], ns, no) for i in range(b)])

        def call(lib, p, st):
            _ok(lib, lib.gcs_feature_gradient(p["slab"], b, h, wd, ns, no, p["grad"], st), "gcs_feature_gradient")
        w.add(Case(nm("gcs_feature_gradient"), ["gcs_feature_gradient"], dict(slab=slab(), grad=out(b * p_ * 4)), call,
                   lambda o: same(view(o["grad"], np.int32, (b, h, wd)), want_grad, (bank, "gcs_feature_gradient"))))

        K = K_TREE
        lab_t, lab_d = bc._label_maps(SLAB_SHAPE, K, seed=h + wd), bc._label_maps(SLAB_SHAPE, 20, seed=9)
        trees = [rt.build_tree(ref[i], lab_t[i], K) for i in range(b)]

        def call(lib, p, st):
            _ok(lib, lib.gcs_region_tree_slab(p["slab"], p["labels"], b, h, wd, ns, no, K, p["ws"], p["merges"], p["costs"], p["alive"],
                                              st), "gcs_region_tree_slab")

        def check(o):
            same(view(o["alive"], np.int32), [tr[2] for tr in trees], (bank, "alive"))
            same(view(o["merges"], np.int32, (b, K - 1, 2)), np.stack([tr[0] for tr in trees]), (bank, "merges"))
            same(view(o["costs"], np.uint64, (b, K - 1)), np.stack([tr[1] for tr in trees]), (bank, "costs"))
        w.add(Case(nm("gcs_region_tree_slab"), ["gcs_region_tree_slab"],
                   dict(slab=slab(), labels=late(lab_t, lab_d), ws=scratch(lib.gcs_region_tree_workspace_bytes(b, h, wd, d, K)),
                        merges=out(b * (K - 1) * 8), costs=out(b * (K - 1) * 8), alive=out(b * 4)), call, check))

    # the in-place stages: the slab itself is the late input
    taps_t, rad_t = sr.taps_array(1.0, ns)
    taps_d, rad_d = sr.taps_array(2.0, ns)
    want_smooth = np.stack([sr.smooth_features(ref[i], 1.0, ns, no) for i in range(b)])

    def call(lib, p, st):
        _ok(lib, lib.gcs_smooth_features(p["slab"], b, h, wd, ns, no, p["taps"], p["radius"], p["ws"], st), "gcs_smooth_features")
    w.add(Case(nm("gcs_smooth_features"), ["gcs_smooth_features"],
               dict(slab=inplace(slab_t, slab_d), taps=late(taps_t, taps_d), radius=late(rad_t, rad_d),
                    ws=scratch(lib.gcs_smooth_workspace_bytes(b, h, wd, ns, no))), call,
               lambda o: same(w.canonical(cfg, o["slab"], b, h, wd), want_smooth, (bank, "gcs_smooth_features"))))

    mu = 5
    want_pos = ref.copy()
    for s in range(ns):
        rows, cols = pr.slot_planes(h, wd, s, mu)
        want_pos[:, 0 * ns * no + s * no + no - 1] = rows
        want_pos[:, 1 * ns * no + s * no + no - 1] = cols

    def call(lib, p, st):
        _ok(lib, lib.gcs_position_features(p["slab"], b, h, wd, ns, no, mu, 0, st), "gcs_position_features")
    w.add(Case(nm("gcs_position_features"), ["gcs_position_features"], dict(slab=inplace(slab_t, slab_d)), call,
               lambda o: same(w.canonical(cfg, o["slab"], b, h, wd), want_pos, (bank, "gcs_position_features"))))

    # the Lloyd entries, one codebook per image
    n_sets = b
    whole = np.ones((b, p_), bool)
    cents = {}
    for k in LLOYD_K[bank]:
        want_init = np.stack([so.kmeans_init(x[i], k) for i in range(n_sets)]).astype(np.int64)
        if k == LLOYD_K[bank][0]:
            def call(lib, p, st, k=k):
                _ok(lib, lib.gcs_kmeans_init(p["slab"], b, h, wd, ns, no, k, n_sets, p["cent"], st), "gcs_kmeans_init")
            c = w.add(Case(nm("gcs_kmeans_init"), ["gcs_kmeans_init"], dict(slab=slab(), cent=out(n_sets * k * d * 2)), call,
                           lambda o, k=k, want_init=want_init: same(view(o["cent"], np.uint16, (n_sets, k, d)), want_init, (bank, "init"))))
            cent_d = view(c.quiet["decoy"]["cent"], np.uint16, (n_sets, k, d))
        else:                                                         # another k: the decoy codebook is the decoy slab's init pixels
            t = w.torch
            sl = t.from_numpy(slab_d).cuda()
            cd = t.empty(n_sets * k * d * 2, dtype=t.uint8, device="cuda")
            _ok(lib, lib.gcs_kmeans_init(sl.data_ptr(), b, h, wd, ns, no, k, n_sets, cd.data_ptr(), t.cuda.current_stream().cuda_stream), "init")
            t.cuda.synchronize()
            cent_d = cd.cpu().numpy().view(np.uint16).reshape(n_sets, k, d)
        book = want_init.astype(np.uint16)
        want_lab, want_sums, want_cnt = _pass_reference(x, want_init, whole)
        want_table = np.concatenate([want_sums, want_cnt[..., None]], axis=2)
        want_new = updated(want_sums, want_cnt, want_init)
        pbytes = lib.gcs_kmeans_partial_bytes(b, h, wd, d, k)
        tag = (bank, k)

        def call(lib, p, st, k=k):
            _ok(lib, lib.gcs_kmeans_assign_accumulate(p["slab"], p["cent"], b, h, wd, ns, no, k, n_sets, 0, h, 0, p["labels"],
                                                      p["partials"], st), "gcs_kmeans_assign_accumulate")
        a = w.add(Case(nm("gcs_kmeans_assign_accumulate", k), ["gcs_kmeans_assign_accumulate"],
                       dict(slab=slab(), cent=late(book, cent_d), labels=out(b * p_), partials=out(pbytes)), call,
                       lambda o, want_lab=want_lab, tag=tag: same(view(o["labels"], np.uint8, (b, p_)), want_lab, (tag, "labels"))))
        part = late(a.quiet["true"]["partials"], a.quiet["decoy"]["partials"])
        tbytes = n_sets * k * (d + 1) * 8

        def call(lib, p, st, k=k):
            _ok(lib, lib.gcs_kmeans_reduce(p["partials"], b, h, wd, d, k, n_sets, p["sums"], st), "gcs_kmeans_reduce")
        r = w.add(Case(nm("gcs_kmeans_reduce", k), ["gcs_kmeans_reduce"], dict(partials=part, sums=out(tbytes)), call,
                       lambda o, want_table=want_table, tag=tag: same(view(o["sums"], np.int64, want_table.shape), want_table, (tag, "sums"))))

        def call(lib, p, st, k=k):
            _ok(lib, lib.gcs_kmeans_finalize(p["sums"], n_sets, k, d, p["cent"], st), "gcs_kmeans_finalize")
        w.add(Case(nm("gcs_kmeans_finalize", k), ["gcs_kmeans_finalize"],
                   dict(sums=late(r.quiet["true"]["sums"], r.quiet["decoy"]["sums"]), cent=inplace(book, cent_d)), call,
                   lambda o, want_new=want_new, tag=tag: same(view(o["cent"], np.uint16, want_new.shape), want_new, (tag, "finalize"))))

        def call(lib, p, st, k=k):
            _ok(lib, lib.gcs_kmeans_reduce_finalize(p["partials"], b, h, wd, d, k, n_sets, p["sums"], p["cent"], st), "reduce_finalize")

        def check(o, want_new=want_new, want_table=want_table, tag=tag):
            same(view(o["sums"], np.int64, want_table.shape), want_table, (tag, "sums of reduce_finalize"))
            same(view(o["cent"], np.uint16, want_new.shape), want_new, (tag, "centroids of reduce_finalize"))
        w.add(Case(nm("gcs_kmeans_reduce_finalize", k), ["gcs_kmeans_reduce_finalize"],
                   dict(partials=late(part.true, part.decoy), sums=out(tbytes), cent=inplace(book, cent_d)), call, check))

        def call(lib, p, st, k=k):
            _ok(lib, lib.gcs_kmeans_assign_raster(p["slab"], p["cent"], b, h, wd, ns, no, k, n_sets, 1, p["map"], 0, p["scratch"], st),
                "gcs_kmeans_assign_raster")
        w.add(Case(nm("gcs_kmeans_assign_raster", k), ["gcs_kmeans_assign_raster"],
                   dict(slab=slab(), cent=late(book, cent_d), map=out(b * p_ * 4), scratch=scratch(lib.gcs_label_slab_bytes(b, h, wd))), call,
                   lambda o, want_lab=want_lab, tag=tag: same(view(o["map"], np.int32, (b, p_)), want_lab, (tag, "raster map"))))
        cents[k] = (a, want_lab)

    if bank == "split":
        import fused_workspace as fw
        k = LLOYD_K[bank][0]
        a, want_lab = cents[k]

        def call(lib, p, st):
            _ok(lib, lib.gcs_labels_widen(p["narrow"], b, h, wd, p["wide"], st), "gcs_labels_widen")
        w.add(Case(nm("gcs_labels_widen"), ["gcs_labels_widen"],
                   dict(narrow=late(a.quiet["true"]["labels"], a.quiet["decoy"]["labels"]), wide=out(b * p_ * 4)), call,
                   lambda o: same(view(o["wide"], np.int32, (b, p_)), want_lab, (bank, "gcs_labels_widen"))))

        # a loop of three self-updating passes: the workspace the caller zeroed is the late buffer of pass 0. Its decoy: sums and
        # counts in the buffer pass 0 adds into, as a pass on other pixels would have left them
        fbytes = lib.gcs_kmeans_fused_workspace_bytes(b, h, wd, ns, no, k, n_sets)
        parts = int(lib.gcs_kmeans_parts_per_image(b, h, wd))
        lay = (n_sets, fw.fold_rows(b, parts, n_sets, fw.env_fold_rows()), k, d)
        assert fbytes > 0 and fw.workspace_bytes(*lay) == fbytes
        ws_d = np.zeros(fbytes, np.uint8)
        v = fw.views(ws_d, *lay)
        v.sums[0][..., :d] = 3 * 12345
        v.sums[0][..., d] = 3
        loop_cent, loop_lab, c = [], [], np.stack([so.kmeans_init(x[i], k) for i in range(n_sets)]).astype(np.int64)
        for t in range(3):
            loop_cent.append(c)
            lab_t, sm, cn = _pass_reference(x, c, whole)
            loop_lab.append(lab_t)
            c = updated(sm, cn, c)
        cb = n_sets * k * d * 2

        def call(lib, p, st):
            for t in range(3):
                _ok(lib, lib.gcs_kmeans_pass_fused(p["slab"], b, h, wd, ns, no, k, n_sets, t & 1, t, 1 if t == 2 else 0, p["ws"],
                                                   p["cent%d" % t], p["map"] if t == 2 else None, 0, st), "gcs_kmeans_pass_fused")

        def check(o):
            for t in range(3):
                same(view(o["cent%d" % t], np.uint16, (n_sets, k, d)), loop_cent[t], (bank, "centroids of fused pass", t))
            same(view(o["map"], np.int32, (b, p_)), loop_lab[2], (bank, "labels of the fused loop"))
            want_ws = np.zeros(fbytes, np.uint8)
            vv = fw.views(want_ws, *lay)
            for t in (1, 2):
                vv.cents[t & 1][...] = loop_cent[t].astype(np.uint16)
            same(o["ws"], want_ws, (bank, "the fused workspace after a complete loop"))
        w.add(Case(nm("gcs_kmeans_pass_fused"), ["gcs_kmeans_pass_fused"],
                   dict(slab=slab(), ws=inplace(np.zeros(fbytes, np.uint8), ws_d), cent0=out(cb), cent1=out(cb), cent2=out(cb),
                        map=out(b * p_ * 4)), call, check))


# ------------------------------------------------------------------------------------------------------------ maps, trees, cuts
def _blocks(shape, step, cols):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return np.broadcast_to(((y // step) * cols + x // step).astype(np.int32), (B,) + tuple(shape)).copy()


def _map_cases(w):
    import boundary_tree_ref as bt
    import colour_ref
    import component_tree_ref as ct
    import contour_map_ref as cm
    import cue_gradient_ref as cg
    import cut_metrics_ref as cx
    import merge_ref
    import region_adjacency_ref as ra
    import region_props_ref as rp
    import region_sweep_ref as rs
    import region_tree_ref as rt
    import superpixel_raw
    import superpixel_ref as sp
    import test_gpu_buffer_contracts as bc
    import texton_gradient_ref as tg
    from oracle import spec_oracle as so
    from scoring_edge import _np_counts, _np_planes
    lib = w.lib
    shape = MAP_SHAPE
    h, wd = shape
    n_px = B * h * wd
    K = K_TREE
    rng = np.random.default_rng(11)

    # ---- label maps of few labels: connected regions, small-region merging, node map
    lab7_t, lab7_d = bc._label_maps(shape, 7, seed=h * wd), bc._label_maps(shape, 7, seed=3)
    want_cc = np.stack([so.connected_regions(m) for m in lab7_t])
    want_m = np.stack([merge_ref.merge_small_regions(m, 3) for m in lab7_t])

    def call(lib, p, st):
        _ok(lib, lib.gcs_connected_regions(p["labels"], B, h, wd, p["ws"], p["cc"], st), "gcs_connected_regions")
    w.add(Case("connected_regions", ["gcs_connected_regions"],
               dict(labels=late(lab7_t, lab7_d), ws=scratch(lib.gcs_connected_scratch_bytes(B, h, wd)), cc=out(n_px * 4)), call,
               lambda o: same(view(o["cc"], np.int32, lab7_t.shape), want_cc, "gcs_connected_regions")))

    def call(lib, p, st):
        _ok(lib, lib.gcs_merge_small_regions(p["labels"], B, h, wd, 3, p["ws"], p["merged"], st), "gcs_merge_small_regions")
    w.add(Case("merge_small_regions", ["gcs_merge_small_regions"],
               dict(labels=late(lab7_t, lab7_d), ws=scratch(lib.gcs_merge_scratch_bytes(B, h, wd, 3)), merged=out(n_px * 4)), call,
               lambda o: same(view(o["merged"], np.int32, lab7_t.shape), want_m, "gcs_merge_small_regions")))

    # node map at k_cap = 64: the noisy maps have more components (the guard size applies), the decoy's 24 blocks have not
    k_cap = 64
    blocks = _blocks(shape, 10, 6)
    infos = [dict() for _ in range(B)]
    want_nodes = np.stack([ct.nodes(lab7_t[i], 3, k_cap, infos[i]) for i in range(B)])
    assert all(i["components"] > k_cap and i["min_size"] > 3 for i in infos)

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_nodes(p["labels"], B, h, wd, 3, k_cap, p["ws"], p["nodes"], p["n_nodes"], p["min_used"], st), "gcs_region_nodes")

    def check(o):
        same(view(o["nodes"], np.int32, lab7_t.shape), want_nodes, "gcs_region_nodes")
        same(view(o["n_nodes"], np.int32), [i["nodes"] for i in infos], "n_nodes")
        same(view(o["min_used"], np.int32), [i["min_size"] for i in infos], "min_size_used")
    w.add(Case("region_nodes", ["gcs_region_nodes"],
               dict(labels=late(lab7_t, blocks), ws=scratch(lib.gcs_region_nodes_scratch_bytes(B, h, wd)), nodes=out(n_px * 4),
                    n_nodes=out(B * 4), min_used=out(B * 4)), call, check))

    # ---- the region tree on canonical features, its cut, its contour map, the sweep histograms
    d = 5
    x_t = rng.integers(0, 46340, (B, d, h, wd)).astype(np.uint16)
    x_d = rng.integers(0, 46340, (B, d, h, wd)).astype(np.uint16)
    lab_t, lab_d = bc._label_maps(shape, K, seed=h * wd + K), bc._label_maps(shape, 20, seed=5)
    trees = [rt.build_tree(x_t[i], lab_t[i], K) for i in range(B)]
    want_merges, want_costs = np.stack([tr[0] for tr in trees]), np.stack([tr[1] for tr in trees])
    want_alive = np.array([tr[2] for tr in trees], np.int32)

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_tree(p["feats"], p["labels"], B, h, wd, d, K, p["ws"], p["merges"], p["costs"], p["alive"], st), "gcs_region_tree")

    def check(o):
        same(view(o["alive"], np.int32), want_alive, "alive")
        same(view(o["merges"], np.int32, want_merges.shape), want_merges, "merges")
        same(view(o["costs"], np.uint64, want_costs.shape), want_costs, "costs")
    tree = w.add(Case("region_tree", ["gcs_region_tree"],
                      dict(feats=late(x_t, x_d), labels=late(lab_t, lab_d), ws=scratch(lib.gcs_region_tree_workspace_bytes(B, h, wd, d, K)),
                           merges=out(B * (K - 1) * 8), costs=out(B * (K - 1) * 8), alive=out(B * 4)), call, check))
    mer_d = view(tree.quiet["decoy"]["merges"], np.int32, want_merges.shape)
    ali_d = view(tree.quiet["decoy"]["alive"], np.int32)
    labels, merges, alive = (lambda: late(lab_t, lab_d)), (lambda: late(want_merges, mer_d)), (lambda: late(want_alive, ali_d))

    R = 5
    want_cut = np.stack([rt.cut(lab_t[i], trees[i][0], trees[i][2], R) for i in range(B)])

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_tree_cut(p["labels"], p["merges"], p["alive"], B, h, wd, K, R, p["cut"], st), "gcs_region_tree_cut")
    w.add(Case("region_tree_cut", ["gcs_region_tree_cut"], dict(labels=labels(), merges=merges(), alive=alive(), cut=out(n_px * 4)), call,
               lambda o: same(view(o["cut"], np.int32, lab_t.shape), want_cut, "gcs_region_tree_cut")))

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_tree_cut(p["labels"], p["merges"], p["alive"], B, h, wd, K, R, p["labels"], st), "gcs_region_tree_cut in place")
    w.add(Case("region_tree_cut in place", ["gcs_region_tree_cut"], dict(labels=inplace(lab_t, lab_d), merges=merges(), alive=alive()), call,
               lambda o: same(view(o["labels"], np.int32, lab_t.shape), want_cut, "gcs_region_tree_cut in place")))

    want_u = np.stack([cm.contour_map(lab_t[i], trees[i][0], trees[i][2]) for i in range(B)])

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_tree_contours(p["labels"], p["merges"], p["alive"], B, h, wd, K, p["ws"], p["u"], st), "gcs_region_tree_contours")
    con = w.add(Case("region_tree_contours", ["gcs_region_tree_contours"],
                     dict(labels=labels(), merges=merges(), alive=alive(), ws=scratch(lib.gcs_region_tree_contours_workspace_bytes(B, K)),
                          u=out(n_px * 4)), call, lambda o: same(view(o["u"], np.int32, lab_t.shape), want_u, "gcs_region_tree_contours")))
    u_d = view(con.quiet["decoy"]["u"], np.int32, lab_t.shape)

    truth_t, first_t, iof_t = bc._truths(shape, seed=K + h)
    truth_d = bc._truths(shape, seed=1)[0]
    T = len(truth_t)
    iof_d = np.repeat(np.arange(B), (2, 2, 2)).astype(np.int32)
    planes_t = _np_planes(truth_t)
    wp = (wd + 63) // 64

    def call(lib, p, st):
        _ok(lib, lib.gcs_truth_prepare(p["truth"], T, h, wd, p["planes"], p["bd"], p["t8"], st), "gcs_truth_prepare")

    def check(o):
        bits = np.unpackbits(view(o["planes"], np.uint8), bitorder="little").reshape(2, T, h, wp * 64).astype(bool)
        assert not bits[..., wd:].any()
        same(bits[..., :wd], planes_t, "bit planes of gcs_truth_prepare")
        same(view(o["bd"], np.int64), _np_counts(lab_t, truth_t, iof_t)[B + 1::3], "bd_counts")
        same(view(o["t8"], np.uint8, truth_t.shape), truth_t.astype(np.uint8), "truth8")
    prep = w.add(Case("truth_prepare", ["gcs_truth_prepare"],
                      dict(truth=late(truth_t, truth_d), planes=out(lib.gcs_bit_planes_bytes(T, h, wd)), bd=out(T * 8), t8=out(T * h * wd)),
                      call, check))

    want_h = np.zeros((B + 2 * T, K + 1), np.uint32)
    for i in range(B):
        hm, rec, prec = cm.histograms(want_u[i], truth_t[first_t[i]:first_t[i + 1]], K)
        want_h[i] = hm
        want_h[B + 2 * first_t[i]:B + 2 * first_t[i + 1]:2], want_h[B + 2 * first_t[i] + 1:B + 2 * first_t[i + 1]:2] = rec, prec

    def call(lib, p, st):
        _ok(lib, lib.gcs_boundary_sweep_resident(p["u"], p["planes"], p["iof"], B, T, h, wd, K, p["hist"], st), "gcs_boundary_sweep_resident")
    w.add(Case("boundary_sweep_resident", ["gcs_boundary_sweep_resident"],
               dict(u=late(want_u, u_d), planes=late(prep.quiet["true"]["planes"], prep.quiet["decoy"]["planes"]), iof=late(iof_t, iof_d),
                    hist=out(want_h.nbytes)), call, lambda o: same(view(o["hist"], np.uint32, want_h.shape), want_h, "sweep histograms")))

    # ---- texton and cue gradients
    Kt, r, n = 64, 1, 16
    labt_t, labt_d = bc._label_maps(shape, Kt, seed=h * wd + Kt + r), bc._label_maps(shape, Kt, seed=8)
    masks_t = tg.masks(r, n)
    masks_d = np.ascontiguousarray(masks_t[::-1])                       # the directions in reverse order: the kernel takes any table
    g_t = rng.integers(0, 1 << 20, labt_t.shape).astype(np.int32)
    g_d = rng.integers(0, 1 << 20, labt_t.shape).astype(np.int32)
    want = [tg.texton_gradient(m, Kt, r, n) for m in labt_t]
    want_dir = np.stack([dd for _, dd in want])
    want_joined = np.stack([tg.joined(want[i][0], g_t[i]) for i in range(B)])

    def call(lib, p, st):
        _ok(lib, lib.gcs_texton_gradient(p["labels"], B, h, wd, Kt, r, n, p["masks"], p["grad"], p["map"], p["dir"], st), "gcs_texton_gradient")

    def check(o):
        same(view(o["map"], np.int32, labt_t.shape), want_joined, "gcs_texton_gradient")
        same(view(o["dir"], np.uint8, labt_t.shape), want_dir, "direction map")
    w.add(Case("texton_gradient", ["gcs_texton_gradient"],
               dict(labels=late(labt_t, labt_d), masks=late(masks_t, masks_d), grad=late(g_t, g_d), map=out(n_px * 4), dir=out(n_px)),
               call, check))

    img_t = rng.integers(0, 256, (B, h, wd, 3)).astype(np.uint8)
    img_d = rng.integers(0, 256, (B, h, wd, 3)).astype(np.uint8)
    rc_, nc_, bins, weights = 2, 4, 16, (1, 2, 3, 4)
    cmask_t = cg.masks(rc_, nc_)
    cmask_d = np.ascontiguousarray(cmask_t[::-1])
    want_pb = [cg.cue_gradient(lab_t[i], img_t[i], K, bins, weights, rc_, nc_) for i in range(B)]
    want_e = np.stack([cg.joined(want_pb[i][0], np.maximum(g_t[i], 0)) for i in range(B)])
    want_cdir = np.stack([dd for _, dd in want_pb])

    def call(lib, p, st):
        _ok(lib, lib.gcs_cue_gradient(p["labels"], p["img"], B, h, wd, K, cg.shift_of(bins), *weights, rc_, nc_, p["masks"], p["grad"],
                                      p["map"], p["dir"], st), "gcs_cue_gradient")

    def check(o):
        same(view(o["map"], np.int32, lab_t.shape), want_e, "gcs_cue_gradient")
        same(view(o["dir"], np.uint8, lab_t.shape), want_cdir, "direction map of gcs_cue_gradient")
    w.add(Case("cue_gradient", ["gcs_cue_gradient"],
               dict(labels=labels(), img=late(img_t, img_d), masks=late(cmask_t, cmask_d), grad=late(g_t, g_d), map=out(n_px * 4),
                    dir=out(n_px)), call, check))

    # ---- opponent colours, superpixels
    gain = 3

    def call(lib, p, st):
        _ok(lib, lib.gcs_colour_opponent(p["img"], n_px, gain, p["ycc"], st), "gcs_colour_opponent")
    w.add(Case("colour_opponent", ["gcs_colour_opponent"], dict(img=late(img_t, img_d), ycc=out(n_px * 3)), call,
               lambda o: same(view(o["ycc"], np.uint8, img_t.shape), colour_ref.opponent(img_t, gain), "gcs_colour_opponent")))

    ny, nx, lam, n_iter = 4, 5, 576, 3
    ks = ny * nx
    want_sp = [sp.superpixels_on_grid(x_t[i], ny, nx, lam, n_iter, return_centres=True) for i in range(B)]

    def call(lib, p, st):
        _ok(lib, lib.gcs_superpixel_segment(p["feats"], B, h, wd, d, ny, nx, lam, n_iter, p["ws"], p["labels"], p["centres"], st),
            "gcs_superpixel_segment")

    def check(o):
        same(view(o["labels"], np.int32, (B, h, wd)), np.stack([a for a, _ in want_sp]), "gcs_superpixel_segment")
        same(view(o["centres"], np.int32, (B, ks, d + 2)), np.stack([c for _, c in want_sp]), "centres of gcs_superpixel_segment")
    w.add(Case("superpixel_segment", ["gcs_superpixel_segment"],
               dict(feats=late(x_t, x_d), ws=scratch(lib.gcs_superpixel_workspace_bytes(B, h, wd, d, superpixel_raw.workspace_n(h, wd, ks))),
                    labels=out(n_px * 4), centres=out(B * ks * (d + 2) * 4)), call, check))

    # ---- the sweeps over every cut: leaf tables of the tree's label map against the annotator maps
    stride = 10
    truth_t = (truth_t % stride).astype(np.uint16)
    truth_d = (truth_d % stride).astype(np.uint16)
    leaf_t = np.stack([rs.leaf_table(lab_t[iof_t[t]], truth_t[t], K, stride) for t in range(T)]).astype(np.uint32)
    leaf_d = np.stack([rs.leaf_table(lab_d[iof_d[t]], truth_d[t], K, stride) for t in range(T)]).astype(np.uint32)
    reg_t, reg_d = np.array([40, 20, 10, 3, 1], np.int32), np.array([35, 16, 8, 2, 1], np.int32)
    nc = len(reg_t)
    per_image = [rs.sweep(lab_t[i], trees[i][0], trees[i][2], truth_t[first_t[i]:first_t[i + 1]], reg_t, K, stride) for i in range(B)]
    want_ss = np.concatenate([s for s, _ in per_image], axis=1)
    want_st = np.concatenate([t for _, t in per_image], axis=1)
    want_last = np.stack([rs.cut_table(leaf_t[t], trees[iof_t[t]][0], max(0, trees[iof_t[t]][2] - 1)) for t in range(T)])
    want_under = np.concatenate([cx.under_counts(lab_t[i], trees[i][0], trees[i][2], truth_t[first_t[i]:first_t[i + 1]], reg_t, K, stride)
                                 for i in range(B)], axis=1)

    def terms_close(got, what):
        err = np.abs(got - want_st)                       # sums of at most K * stride non-negative float64 terms, each within an ulp or
        assert (err <= 1e-11 * np.maximum(np.abs(want_st), 1.0)).all(), (what, float(err.max()))   # two: the bound of the agreement case

    def sweep_bufs(extra):
        bufs = dict(leaf=inplace(leaf_t, leaf_d), merges=merges(), alive=alive(), iof=late(iof_t, iof_d), regions=late(reg_t, reg_d),
                    ws=scratch(lib.gcs_region_sweep_workspace_bytes(T, K, stride, nc)))
        bufs.update(extra)
        bufs.update(sums=out(nc * T * 32), terms=out(nc * T * 32))
        return bufs

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_sweep(p["leaf"], p["merges"], p["alive"], p["iof"], p["regions"], B, T, K, stride, nc, p["ws"], p["sums"],
                                      p["terms"], st), "gcs_region_sweep")

    def check(o):
        same(view(o["sums"], np.uint64, want_ss.shape), want_ss, "sums of gcs_region_sweep")
        terms_close(view(o["terms"], np.float64, want_st.shape), "terms of gcs_region_sweep")
        same(view(o["leaf"], np.uint32, leaf_t.shape), want_last, "the consumed leaf tables: the table of the last cut")
    w.add(Case("region_sweep", ["gcs_region_sweep"], sweep_bufs({}), call, check))

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_sweep_under(p["leaf"], p["merges"], p["alive"], p["iof"], p["regions"], B, T, K, stride, nc, p["ws"],
                                            p["under"], p["sums"], p["terms"], st), "gcs_region_sweep_under")

    def check(o):
        same(view(o["under"], np.uint64, want_under.shape), want_under, "under counts")
        same(view(o["sums"], np.uint64, want_ss.shape), want_ss, "sums of gcs_region_sweep_under")
        terms_close(view(o["terms"], np.float64, want_st.shape), "terms of gcs_region_sweep_under")
    w.add(Case("region_sweep_under", ["gcs_region_sweep_under"], sweep_bufs(dict(under=out(nc * T * 24))), call, check))

    shapes_ = [cx.shapes(lab_t[i], want_u[i], trees[i][0], trees[i][2], reg_t, K) for i in range(B)]

    def call(lib, p, st):
        _ok(lib, lib.gcs_cut_shapes(p["labels"], p["u"], p["merges"], p["alive"], p["regions"], B, h, wd, K, nc, p["ws"], p["area"], p["perim"],
                                    p["boundary"], st), "gcs_cut_shapes")

    def check(o):
        same(view(o["area"], np.uint32, (nc, B, K)), np.stack([s[0] for s in shapes_], axis=1), "area of gcs_cut_shapes")
        same(view(o["perim"], np.uint32, (nc, B, K)), np.stack([s[1] for s in shapes_], axis=1), "perimeter of gcs_cut_shapes")
        same(view(o["boundary"], np.uint32, (nc, B)), np.stack([s[2] for s in shapes_], axis=1), "boundary of gcs_cut_shapes")
    w.add(Case("cut_shapes", ["gcs_cut_shapes"],
               dict(labels=labels(), u=late(want_u, u_d), merges=merges(), alive=alive(), regions=late(reg_t, reg_d),
                    ws=scratch(lib.gcs_cut_shapes_workspace_bytes(B, K, nc)), area=out(nc * B * K * 4), perim=out(nc * B * K * 4),
                    boundary=out(nc * B * 4)), call, check))

    # ---- region descriptors, their cuts, the mean-colour picture
    C = rp.FIXED + d
    leaves = [rp.leaf_table(lab_t[i], K, img_t[i], x_t[i]) for i in range(B)]
    want_sums, want_bbox = np.stack([s for s, _ in leaves]), np.stack([bx for _, bx in leaves])

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_props(p["labels"], p["img"], p["feats"], B, h, wd, d, K, p["sums"], p["bbox"], st), "gcs_region_props")

    def check(o):
        same(view(o["sums"], np.uint64, want_sums.shape), want_sums, "sums of gcs_region_props")
        same(view(o["bbox"], np.int32, want_bbox.shape), want_bbox, "boxes of gcs_region_props")
    props = w.add(Case("region_props", ["gcs_region_props"],
                       dict(labels=labels(), img=late(img_t, img_d), feats=late(x_t, x_d), sums=out(want_sums.nbytes), bbox=out(want_bbox.nbytes)),
                       call, check))
    sums_io = lambda: late(want_sums, props.quiet["decoy"]["sums"])
    rsum = int(sum(min(K, int(r_)) for r_ in reg_t))
    cuts = [rp.cut_tables_by_rows(want_sums[i], want_bbox[i], trees[i][0], trees[i][2], reg_t, shape) for i in range(B)]
    want_group = np.stack([c[0] for c in cuts], axis=1)                                         # [n_cuts][B][K]

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_props_cuts(p["sums"], p["bbox"], p["merges"], p["alive"], p["regions"], B, h, wd, K, C, nc, rsum, p["group"],
                                           p["sums_out"], p["bbox_out"], st), "gcs_region_props_cuts")

    def check(o):
        same(view(o["group"], np.int32, want_group.shape), want_group, "groups of gcs_region_props_cuts")
        same(view(o["sums_out"], np.uint64, (B, rsum, C)), np.stack([c[1] for c in cuts]), "sums of gcs_region_props_cuts")
        same(view(o["bbox_out"], np.int32, (B, rsum, 4)), np.stack([c[2] for c in cuts]), "boxes of gcs_region_props_cuts")
    pc = w.add(Case("region_props_cuts", ["gcs_region_props_cuts"],
                    dict(sums=sums_io(), bbox=late(want_bbox, props.quiet["decoy"]["bbox"]), merges=merges(), alive=alive(),
                         regions=late(reg_t, reg_d), group=out(want_group.nbytes), sums_out=out(B * rsum * C * 8), bbox_out=out(B * rsum * 16)),
                    call, check))
    group_d = view(pc.quiet["decoy"]["group"], np.int32, want_group.shape)
    cut_i = 2                                                                                   # the picture of the cut at R = 10
    want_rgb = np.stack([rp.paint(lab_t[i], want_sums[i], want_group[cut_i, i], K) for i in range(B)])

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_paint(p["labels"], p["group"], p["sums"], B, h, wd, K, K, C, K, p["rgb"], st), "gcs_region_paint")
    w.add(Case("region_paint", ["gcs_region_paint"],
               dict(labels=labels(), group=late(want_group[cut_i], group_d[cut_i]), sums=sums_io(), rgb=out(n_px * 3)), call,
               lambda o: same(view(o["rgb"], np.uint8, img_t.shape), want_rgb, "gcs_region_paint")))

    # ---- adjacency graph, its cuts, the tree merged by boundary strength
    cap = 1024
    graphs = [ra.table(*ra.leaf_graph(lab_t[i], K, img_t[i], g_t[i]), cap) for i in range(B)]
    want_e, want_v = np.stack([g_[0] for g_ in graphs]), np.stack([g_[1] for g_ in graphs])
    want_n = np.array([g_[2] for g_ in graphs], np.int32)
    assert (want_n > 0).all()

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_adjacency(p["labels"], p["img"], p["strength"], B, h, wd, K, cap, p["ws"], p["edges"], p["vals"], p["count"],
                                          st), "gcs_region_adjacency")

    def check(o):
        same(view(o["count"], np.int32), want_n, "edge counts")
        same(view(o["edges"], np.int32, want_e.shape), want_e, "edges")
        same(view(o["vals"], np.uint64, want_v.shape), want_v, "edge columns")
    adj = w.add(Case("region_adjacency", ["gcs_region_adjacency"],
                     dict(labels=labels(), img=late(img_t, img_d), strength=late(g_t, g_d), ws=scratch(lib.gcs_region_adjacency_workspace_bytes(B, cap)),
                          edges=out(want_e.nbytes), vals=out(want_v.nbytes), count=out(B * 4)), call, check))
    table = lambda: dict(edges=late(want_e, adj.quiet["decoy"]["edges"]), vals=late(want_v, adj.quiet["decoy"]["vals"]),
                         count=late(want_n, adj.quiet["decoy"]["count"]))
    cap_out, G = 1024, K
    cut_graphs = [[ra.table(*ra.cut_graph(want_e[i][:want_n[i]], want_v[i][:want_n[i]], want_group[c, i], G), cap_out) for i in range(B)]
                  for c in range(nc)]

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_adjacency_cuts(p["edges"], p["vals"], p["count"], p["group"], B, K, G, cap, nc, cap_out, p["ws"], p["edges_out"],
                                               p["vals_out"], p["count_out"], st), "gcs_region_adjacency_cuts")

    def check(o):
        same(view(o["count_out"], np.int32, (nc, B)), [[g_[2] for g_ in row] for row in cut_graphs], "edge counts of the cuts")
        same(view(o["edges_out"], np.int32, (nc, B, cap_out, 2)), [[g_[0] for g_ in row] for row in cut_graphs], "edges of the cuts")
        same(view(o["vals_out"], np.uint64, (nc, B, cap_out, 3)), [[g_[1] for g_ in row] for row in cut_graphs], "edge columns of the cuts")
    bufs = table()
    bufs.update(group=late(want_group, group_d), ws=scratch(lib.gcs_region_adjacency_workspace_bytes(nc * B, cap_out)),
                edges_out=out(nc * B * cap_out * 8), vals_out=out(nc * B * cap_out * 24), count_out=out(nc * B * 4))
    w.add(Case("region_adjacency_cuts", ["gcs_region_adjacency_cuts"], bufs, call, check))

    want_used = np.stack([bt.used_labels(m, K) for m in lab_t])

    def call(lib, p, st):
        _ok(lib, lib.gcs_label_used(p["labels"], B, h, wd, K, p["used"], st), "gcs_label_used")
    used = w.add(Case("label_used", ["gcs_label_used"], dict(labels=labels(), used=out(B * K * 4)), call,
                      lambda o: same(view(o["used"], np.int32, (B, K)), want_used, "gcs_label_used")))
    btrees = [bt.tree_of_table(want_e[i], want_v[i], want_n[i], want_used[i], K) for i in range(B)]

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_tree_edges(p["edges"], p["vals"], p["count"], p["used"], B, K, cap, p["ws"], p["merges"], p["costs"], p["alive"],
                                           st), "gcs_region_tree_edges")

    def check(o):
        same(view(o["alive"], np.int32), [tr[2] for tr in btrees], "alive of gcs_region_tree_edges")
        same(view(o["merges"], np.int32, (B, K - 1, 2)), np.stack([tr[0] for tr in btrees]), "merges of gcs_region_tree_edges")
        same(view(o["costs"], np.uint64, (B, K - 1)), np.stack([tr[1] for tr in btrees]), "costs of gcs_region_tree_edges")
    bufs = table()
    bufs.update(used=late(want_used, used.quiet["decoy"]["used"]), ws=scratch(lib.gcs_region_tree_edges_workspace_bytes(B, K, cap)),
                merges=out(B * (K - 1) * 8), costs=out(B * (K - 1) * 8), alive=out(B * 4))
    w.add(Case("region_tree_edges", ["gcs_region_tree_edges"], bufs, call, check))

    # ---- the two entry points without a device input of their own kind
    # gcs_selftest_isqrt reads no buffer: what arrives late is the entry content of the counter it zeroes. A launch (or the
    # zeroing) that ran before the gate is overwritten by the late bytes, and the clone shows them.
    def call(lib, p, st):
        _ok(lib, lib.gcs_selftest_isqrt(1 << 20, p["bad"], st), "gcs_selftest_isqrt")
    w.add(Case("selftest_isqrt", ["gcs_selftest_isqrt"], dict(bad=inplace(np.full(4, 0xA5, np.uint8), np.full(4, 0x5A, np.uint8))), call,
               lambda o: same(view(o["bad"], np.uint32), [0], "gcs_selftest_isqrt"), free_outputs=("bad",)))

    nbytes = 3 * 65536 + 4099                                          # whole 64 KiB rows and a rest: both copies of the call
    src_t, src_d = rng.integers(1, 256, nbytes, dtype=np.uint8), rng.integers(1, 256, nbytes, dtype=np.uint8)

    def call(lib, p, st):
        _ok(lib, lib.gcs_download(p["src"], p["dst"], nbytes, st), "gcs_download")
    w.add(Case("download", ["gcs_download"], dict(src=late(src_t, src_d), dst=out(nbytes, pinned=True)), call,
               lambda o: same(o["dst"], src_t, "gcs_download")))


# ------------------------------------------------------------------------------------------------------------ scoring
def _score_cases(w):
    import test_gpu_buffer_contracts as bc
    from scoring_edge import _np_counts, _np_reduce, _np_tables, _np_tables_batch
    lib = w.lib
    shape = SCORE_SHAPE
    h, wd = shape
    n_seg, STRIDE, A_MAX = bc.SEG_AT + 1, bc.STRIDE, bc.A_MAX          # just past the private-table limit
    rng = np.random.default_rng(h * 100 + wd + n_seg)
    labs_t = rng.integers(0, n_seg, (B, h, wd)).astype(np.int32)
    labs_t[:, h - 1, wd - 1] = n_seg - 1
    labs_d = rng.integers(0, n_seg - 7, (B, h, wd)).astype(np.int32)
    labs_d[:, 0, 0] = np.arange(n_seg - 10, n_seg - 10 + B)           # another largest label per image
    truths = {}
    for key, seed in (("t", n_seg + wd), ("d", 4)):
        tr, first, iof = bc._truths(shape, seed=seed)
        tr = (tr + rng.integers(0, STRIDE - 4, tr.shape)).astype(np.uint16)
        tr[:, 0, 0] = STRIDE - 1
        truths[key] = tr
    truth_t, truth_d = truths["t"], truths["d"]
    T = len(truth_t)
    first_d, iof_d = np.array([0, 2, 4, 6], np.int32), np.repeat(np.arange(B), (2, 2, 2)).astype(np.int32)
    one, a1 = 1, 3
    truth1_t, truth1_d = truth_t[first[one]:first[one + 1]], truth_d[first[one]:first[one + 1]]
    want_c1 = _np_counts(labs_t[one][None], truth1_t, np.zeros(a1, np.int32))
    want_c = _np_counts(labs_t, truth_t, iof)
    want_t1 = _np_tables(labs_t[one], truth1_t, n_seg, STRIDE)
    want_t = _np_tables_batch(labs_t, truth_t, first, n_seg, STRIDE)
    want_under = _np_reduce(want_t[0], want_t[1], iof)
    want_sums, want_terms = bc._agreement(want_t[0])
    smax = labs_t.reshape(B, -1).max(axis=1).astype(np.int32)
    hb_, ab_ = T * n_seg * STRIDE * 4, B * n_seg * 4

    def call(lib, p, st):
        _ok(lib, lib.gcs_boundary_counts(p["lab"], p["truth"], a1, h, wd, p["ws"], p["counts"], st), "gcs_boundary_counts")
    w.add(Case("boundary_counts", ["gcs_boundary_counts"],
               dict(lab=late(labs_t[one], labs_d[one]), truth=late(truth1_t, truth1_d), ws=scratch(lib.gcs_boundary_scratch_bytes(a1, h, wd)),
                    counts=out((1 + 3 * a1) * 8)), call, lambda o: same(view(o["counts"], np.int64), want_c1, "gcs_boundary_counts")))

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_counts(p["lab"], p["truth"], a1, h, wd, n_seg, STRIDE, p["hist"], p["area"], p["perim"], st), "gcs_region_counts")

    def check(o):
        for key, dt_, wv in zip(("hist", "area", "perim"), (np.uint32,) * 3, want_t1):
            same(view(o[key], dt_, np.asarray(wv).shape), wv, ("gcs_region_counts", key))
    w.add(Case("region_counts", ["gcs_region_counts"],
               dict(lab=late(labs_t[one], labs_d[one]), truth=late(truth1_t, truth1_d), hist=out(a1 * n_seg * STRIDE * 4), area=out(n_seg * 4),
                    perim=out(n_seg * 4)), call, check))

    def call(lib, p, st):
        _ok(lib, lib.gcs_boundary_counts_batch(p["labs"], p["truth"], p["iof"], B, T, h, wd, p["ws"], p["counts"], st), "gcs_boundary_counts_batch")
    w.add(Case("boundary_counts_batch", ["gcs_boundary_counts_batch"],
               dict(labs=late(labs_t, labs_d), truth=late(truth_t, truth_d), iof=late(iof, iof_d),
                    ws=scratch(lib.gcs_boundary_batch_scratch_bytes(B, T, h, wd)), counts=out((B + 3 * T) * 8)), call,
               lambda o: same(view(o["counts"], np.int64), want_c, "gcs_boundary_counts_batch")))

    # the resident truth of both sets, made quietly by gcs_truth_prepare (its own case: tests of the map shape)
    res = {}
    t = w.torch
    for key, tr in (("t", truth_t), ("d", truth_d)):
        src = t.from_numpy(tr.view(np.int16)).cuda()
        planes = t.empty(lib.gcs_bit_planes_bytes(T, h, wd), dtype=t.uint8, device="cuda")
        bd, t8 = t.empty(T * 8, dtype=t.uint8, device="cuda"), t.empty(T * h * wd, dtype=t.uint8, device="cuda")
        _ok(lib, lib.gcs_truth_prepare(src.data_ptr(), T, h, wd, planes.data_ptr(), bd.data_ptr(), t8.data_ptr(),
                                       t.cuda.current_stream().cuda_stream), "gcs_truth_prepare")
        t.cuda.synchronize()
        res[key] = tuple(v.cpu().numpy() for v in (planes, bd, t8))
    same(view(res["t"][1], np.int64), want_c[B + 1::3], "bd_counts of gcs_truth_prepare")
    same(view(res["t"][2], np.uint8, truth_t.shape), truth_t.astype(np.uint8), "truth8 of gcs_truth_prepare")
    planes, bd, t8 = (lambda: late(res["t"][0], res["d"][0])), (lambda: late(res["t"][1], res["d"][1])), (lambda: late(res["t"][2], res["d"][2]))

    def call(lib, p, st):
        _ok(lib, lib.gcs_boundary_counts_resident(p["labs"], p["planes"], p["bd"], p["iof"], B, T, h, wd, p["ws"], p["counts"], p["seg_max"], st),
            "gcs_boundary_counts_resident")

    def check(o):
        same(view(o["counts"], np.int64), want_c, "gcs_boundary_counts_resident")
        same(view(o["seg_max"], np.int32), smax, "seg_max")
    w.add(Case("boundary_counts_resident", ["gcs_boundary_counts_resident"],
               dict(labs=late(labs_t, labs_d), planes=planes(), bd=bd(), iof=late(iof, iof_d), ws=scratch(lib.gcs_bit_planes_bytes(B, h, wd)),
                    counts=out((B + 3 * T) * 8), seg_max=out(B * 4)), call, check))

    def tables_check(what):
        def check(o):
            for key, wv in zip(("hist", "area", "perim"), want_t):
                same(view(o[key], np.uint32, np.asarray(wv).shape), wv, (what, key))
        return check

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_counts_batch(p["labs"], p["truth"], p["first"], B, T, A_MAX, h, wd, n_seg, STRIDE, p["hist"], p["area"],
                                             p["perim"], st), "gcs_region_counts_batch")
    tab = w.add(Case("region_counts_batch", ["gcs_region_counts_batch"],
                     dict(labs=late(labs_t, labs_d), truth=late(truth_t, truth_d), first=late(first, first_d), hist=out(hb_), area=out(ab_),
                          perim=out(ab_)), call, tables_check("gcs_region_counts_batch")))

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_counts_batch_u8(p["labs"], p["t8"], p["first"], B, T, A_MAX, h, wd, n_seg, STRIDE, p["hist"], p["area"],
                                                p["perim"], st), "gcs_region_counts_batch_u8")
    w.add(Case("region_counts_batch_u8", ["gcs_region_counts_batch_u8"],
               dict(labs=late(labs_t, labs_d), t8=t8(), first=late(first, first_d), hist=out(hb_), area=out(ab_), perim=out(ab_)), call,
               tables_check("gcs_region_counts_batch_u8")))
    hist = lambda: late(tab.quiet["true"]["hist"], tab.quiet["decoy"]["hist"])

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_reduce(p["hist"], p["area"], p["iof"], T, n_seg, STRIDE, p["under"], p["under_np"], st), "gcs_region_reduce")

    def check(o):
        same(view(o["under"], np.int64), want_under[0], "under")
        same(view(o["under_np"], np.int64), want_under[1], "under_np")
    w.add(Case("region_reduce", ["gcs_region_reduce"],
               dict(hist=hist(), area=late(tab.quiet["true"]["area"], tab.quiet["decoy"]["area"]), iof=late(iof, iof_d), under=out(T * 8),
                    under_np=out(T * 8)), call, check))

    def call(lib, p, st):
        _ok(lib, lib.gcs_score_batch_resident(p["labs"], p["planes"], p["bd"], p["t8"], 1, p["first"], p["iof"], B, T, A_MAX, h, wd, n_seg,
                                              STRIDE, p["ws"], p["hist"], p["counts"], p["seg_max"], p["area"], p["perim"], p["under"],
                                              p["under_np"], st), "gcs_score_batch_resident")

    def check(o):
        for key, dt_, wv in (("hist", np.uint32, want_t[0]), ("counts", np.int64, want_c), ("seg_max", np.int32, smax),
                             ("area", np.uint32, want_t[1]), ("perim", np.uint32, want_t[2]), ("under", np.int64, want_under[0]),
                             ("under_np", np.int64, want_under[1])):
            same(view(o[key], dt_, np.asarray(wv).shape), wv, ("gcs_score_batch_resident", key))
    w.add(Case("score_batch_resident", ["gcs_score_batch_resident"],
               dict(labs=late(labs_t, labs_d), planes=planes(), bd=bd(), t8=t8(), first=late(first, first_d), iof=late(iof, iof_d),
                    ws=scratch(lib.gcs_bit_planes_bytes(B, h, wd)), hist=out(hb_), counts=out((B + 3 * T) * 8), seg_max=out(B * 4), area=out(ab_),
                    perim=out(ab_), under=out(T * 8), under_np=out(T * 8)), call, check))

    smax_d = labs_d.reshape(B, -1).max(axis=1).astype(np.int32)

    def call(lib, p, st):
        _ok(lib, lib.gcs_region_agreement(p["hist"], p["iof"], p["seg_max"], T, n_seg, STRIDE, p["ws"], p["sums"], p["terms"], st),
            "gcs_region_agreement")

    def check(o):
        same(view(o["sums"], np.uint64, (T, 4)), want_sums, "agreement sums")
        err = np.abs(view(o["terms"], np.float64, (T, 4)) - want_terms)           # the bound of tests/test_gpu_buffer_contracts.py
        assert (err <= 1e-11 * np.maximum(np.abs(want_terms), 1.0)).all(), ("agreement terms", float(err.max()))
    w.add(Case("region_agreement", ["gcs_region_agreement"],
               dict(hist=hist(), iof=late(iof, iof_d), seg_max=late(smax, smax_d), ws=scratch(lib.gcs_region_agreement_scratch_bytes(T, n_seg, STRIDE)),
                    sums=out(T * 32), terms=out(T * 32)), call, check))


BUILDERS = [(_slab_cases, (bank,)) for bank in BANKS] + [(_map_cases, ()), (_score_cases, ())]


def build_world(torch):
    return World(torch).build(BUILDERS)


# ------------------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def world(torch_cuda):
    return build_world(torch_cuda)


@gpu
def test_every_case_was_built(world):
    """Every name of the table has its quiet runs; the gate is at least 50 ms and 20 times the longest enqueue."""
    assert not world.builder_errors, world.builder_errors
    assert sorted(world.cases) == NAMES
    longest = max(c.enqueue_s for c in world.cases.values())
    assert world.run.gate_s >= max(so_.GATE_MIN_S, so_.GATE_FACTOR * longest)
    times = sorted(c.enqueue_s for c in world.cases.values())
    print("\nstream contract: gate %.1f ms; quiet enqueue longest %.3f ms (%s), median %.3f ms; %.0f sleep cycles per ms" % (
        world.run.gate_s * 1e3, longest * 1e3, max(world.cases.values(), key=lambda c: c.enqueue_s).name, times[len(times) // 2] * 1e3,
        world.run.cycles_per_s * 1e-3))


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_late_inputs_and_no_host_wait(world, name):
    """The quiet run == the reference and the decoys change every output; then the late run: back on the host while the gate still
    runs, and every output byte that of the quiet run."""
    case = world.cases.get(name)
    assert case is not None, (name, "not built", world.builder_errors)
    if case.error is not None:
        raise case.error
    world.run.hold_late(case)
    world.run.release(case)
    print("\n%s: quiet enqueue %.3f ms, late host %.3f ms, gate %.1f ms" % ((name, case.enqueue_s * 1e3) + tuple(v * 1e3 for v in world.run.log[-1][1:])))


def _fork_case(lib):
    import hot_banks as hb
    h, w = FORK_SHAPE
    imgs_t = hb.hot_images(FORK_BATCH, h, w, seed=1)
    imgs_d = np.ascontiguousarray(imgs_t[::-1])
    return _gabor_case(lib, "fork", BANKS["split"], imgs_t, imgs_d), imgs_t


@gpu
def test_gabor_fork_behind_pending_work(torch_cuda, world):
    """gcs_gabor_features at a size whose plan is forked (level 1 on the library's side stream): the late run's slab == the quiet
    run's in every byte, flag words and padding included, both from 0xA5; four images of the quiet slab == the C oracle."""
    from fused_stages import ref_features
    torch, lib = torch_cuda, world.lib
    cfg = BANKS["split"]
    ns, no, ks, shift = cfg
    h, w = FORK_SHAPE
    buf = ctypes.create_string_buffer(1 << 14)
    assert lib.gcs_selftest_gabor_plan(FORK_BATCH, h, w, ns, no, ks, shift, 0, 1, buf, len(buf)) > 0
    plan = buf.value.decode()
    assert "stream=side" in plan, plan
    assert lib.gcs_selftest_gabor_plan(FORK_BATCH, h, w, ns, no, ks, shift, 0, 0, buf, len(buf)) > 0
    assert "stream=side" not in buf.value.decode()
    case, imgs = _fork_case(lib)
    run = world.run
    case.quiet["decoy"], _ = run.quiet_run(case, "decoy")
    case.quiet["true"], case.enqueue_s = run.quiet_run(case, "true")
    assert so_.GATE_FACTOR * case.enqueue_s <= run.gate_s, (case.enqueue_s, run.gate_s)
    slab = case.quiet["true"]["slab"]
    assert not np.array_equal(slab, case.quiet["decoy"]["slab"])
    per = lib.gcs_feature_slab_bytes(1, h, w, ns, no)
    pick = [0, 1, 64, FORK_BATCH - 1]
    got = world.canonical(cfg, np.concatenate([slab[i * per:(i + 1) * per] for i in pick]), len(pick), h, w)
    same(got, ref_features(cfg, imgs[pick]), "the forked plan against the C oracle")
    # the library's side stream shares its hardware queue with some of torch's streams, and behind a gate on one of those its
    # launches are in order whatever the events say: several consecutive streams of the pool, so that most do not
    for _ in range(FORK_STREAMS):
        run.hold_late(case, torch.cuda.Stream())
    run.release(case)
    print("\nfork: quiet enqueue %.3f ms, late host %.3f ms, gate %.1f ms" % ((case.enqueue_s * 1e3,) + tuple(v * 1e3 for v in run.log[-1][1:])))


# ---- the Python layer
PY_SHAPE = (72, 104)         # tests/test_gpu_contour_map.py


def _late_tensor(torch, true, decoy, side, cycles):
    """A device tensor that holds ``decoy`` now and ``true`` only behind a gate on ``side``."""
    t = torch.from_numpy(np.ascontiguousarray(decoy)).cuda()
    src = torch.from_numpy(np.ascontiguousarray(true)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        t.copy_(src, non_blocking=True)
    return t


def _host(v):
    if isinstance(v, (tuple, list)):
        return [_host(x) for x in v]
    if isinstance(v, dict):
        return {k: _host(x) for k, x in v.items()}
    return v.cpu().numpy().copy() if hasattr(v, "cpu") else v


def _same_tree(a, b, what):
    if isinstance(a, list):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same_tree(x, y, (what, i))
    elif isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same_tree(a[k], b[k], (what, k))
    elif isinstance(a, np.ndarray):
        same(a, b, what)
    else:
        assert a == b, (what, a, b)


PY_METHODS = {
    "segment_device": (dict(), "segment_device", ()),
    "segment_device n_superpixels": (dict(n_superpixels=60), "segment_device", ()),
    "segment_device n_regions": (dict(n_superpixels=60, n_regions=6), "segment_device", ()),
    "region_tree_device": (dict(n_superpixels=60, n_regions=6), "region_tree_device", ()),
    "contours_device": (dict(n_superpixels=60, n_regions=6), "contours_device", ()),
    "edges_device": (dict(), "edges_device", ()),
    "texton_edges_device": (dict(), "texton_edges_device", ()),
    "cue_edges_device": (dict(), "cue_edges_device", ()),
}


@gpu
@pytest.mark.parametrize("method", list(PY_METHODS))
def test_python_layer_takes_a_late_device_input(torch_cuda, world, method):
    """Each device method of a fresh Segmenter, called on a side stream whose image tensor is still being written behind a gate,
    gives what it gives quietly on the default stream (no gate-still-running assertion: these paths may allocate)."""
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    torch = torch_cuda
    kw, attr, args = PY_METHODS[method]
    h, w = PY_SHAPE
    imgs_t, imgs_d = synthetic_batch(2, h, w, seed=3), synthetic_batch(2, h, w, seed=4)
    quiet = _host(getattr(Segmenter(n_iter=4, device="cuda:0", **kw), attr)(torch.from_numpy(imgs_t).cuda(), *args))
    torch.cuda.synchronize()
    quiet_d = _host(getattr(Segmenter(n_iter=4, device="cuda:0", **kw), attr)(torch.from_numpy(imgs_d).cuda(), *args))
    first = quiet[0] if isinstance(quiet, list) else quiet
    first_d = quiet_d[0] if isinstance(quiet_d, list) else quiet_d
    assert not np.array_equal(first, first_d), "the decoy images give the same result"
    seg = Segmenter(n_iter=4, device="cuda:0", **kw)
    side = world.run.side_stream()
    x = _late_tensor(torch, imgs_t, imgs_d, side, int(world.run.gate_s * world.run.cycles_per_s))
    with torch.cuda.stream(side):
        got = getattr(seg, attr)(x, *args)
        got = got.clone() if hasattr(got, "clone") else [g.clone() if hasattr(g, "clone") else g for g in got]
        x.copy_(torch.from_numpy(imgs_d).cuda(), non_blocking=True)
    side.synchronize()
    _same_tree(_host(got), quiet, method)


@gpu
def test_device_truth_scores_late_labels(torch_cuda, world):
    """DeviceTruth: labels written behind a gate on a side stream, submitted on that stream, collected: evaluate.py's numbers."""
    from gabor_color_image_segmentation_amd import evaluate as ev
    from gabor_color_image_segmentation_amd.evaluate_gpu import DeviceTruth, submit_scores_batch_resident
    torch = torch_cuda
    h, w = PY_SHAPE
    rng = np.random.default_rng(6)
    blocks = lambda step, k: np.kron(rng.integers(0, k, (-(-h // step), -(-w // step))), np.ones((step, step), np.int64))[:h, :w]
    truths = [[blocks(12, 5).astype(np.uint16) for _ in range(a)] for a in (2, 3)]
    labs_t = np.stack([blocks(8, 9) for _ in range(2)]).astype(np.int32)
    labs_d = np.stack([blocks(6, 7) for _ in range(2)]).astype(np.int32)
    first = np.array([0, 2, 5], np.int32)
    stack = np.stack(truths[0] + truths[1])
    dt = DeviceTruth(stack, first, np.repeat(np.arange(2), (2, 3)).astype(np.int32), [int(m.max()) + 1 for m in stack], device="cuda:0")
    side = world.run.side_stream()
    x = _late_tensor(torch, labs_t, labs_d, side, int(world.run.gate_s * world.run.cycles_per_s))
    with torch.cuda.stream(side):
        pending = submit_scores_batch_resident(x, dt, n_segments=9)
        x.copy_(torch.from_numpy(labs_d).cuda(), non_blocking=True)
    got = pending.result()
    side.synchronize()
    for i in range(2):
        m = ev.metrics(np.zeros((h, w, 3), np.uint8), labs_t[i], truths[i])
        m.set_metrics()
        want = m.get_metrics()
        assert got[i]["regions"] == want["regions"]
        for key in ("recall", "precision", "fmeasure", "density"):
            assert got[i][key] == want[key], (i, key)
        for key in ("underseg", "undersegNP", "compactness"):                    # the bound of tests/test_gpu_scoring.py
            assert abs(got[i][key] - want[key]) <= 1e-12, (i, key)


@gpu
def test_capturable_entry_points_replay_on_new_inputs(built):
    """One child process (a failed capture leaves its thread unable to launch: it must not take this process with it): every
    entry point the header calls "(capturable)", and gcs_gabor_features at the forked size, captured on a side stream and replayed
    on the second input set. The child prints one line per entry point; every line is asserted, so that a refusal names its symbol."""
    child = os.path.join(HERE, "checkers", "stream_capture_child.py")
    r = subprocess.run([sys.executable, child], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    lines = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(OK|FAIL) (gcs_\w+)(.*)", line)
        if m:
            lines[m.group(2)] = (m.group(1), m.group(3))
    for sym in CAPTURABLE + ("gcs_gabor_features",):
        assert sym in lines, (sym, "the child printed no line for it", r.returncode, r.stdout[-2000:])
        assert lines[sym][0] == "OK", (sym, lines[sym][1])
    assert r.returncode == 0, r.stdout[-2000:]
