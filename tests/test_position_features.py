"""Position features (SPEC.md §12) on the CPU: the bank of ``make_bank(position_weight=mu)`` against the restatement
(tests/position_ref.py), parameter validation, the restatement against a direct per-pixel loop, the Segmenter plumbing through a
CPU stand-in (tests/position_ops.py: call order on every host path a stand-in reaches, global row coordinates on a strip), the
restatement's quality on the val fixture, and the host-only argument checks of gcs_position_features (nothing is launched).

How the pinned scores were produced: ``QUALITY_6`` holds what ``position_ref.segment`` (C oracle, k = 8, 10 passes, raw cluster
labels) scores with ``evaluate.boundary_scores`` / ``region_agreement`` on each of the first six val fixture images at
n_orient = 4, color_weight = 1/8, chroma_gain = 4, position_weight = 6, printed with ``repr`` by the loop of
``test_quality_pin_on_six_val_fixture_images`` itself; they come from the restatement, never from the GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import colour_ref as cr
import position_ref as pr
from fake_ops import OracleOps
from position_ops import PositionOps
from gabor_color_image_segmentation_amd import Segmenter, _lib, make_bank, segment, segment_batch, segment_images
from gabor_color_image_segmentation_amd.evaluate import boundary_scores, region_agreement
from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
from oracle import spec_oracle as so

GOLD = os.path.join(os.path.dirname(__file__), "golden")


# ---- the bank

@pytest.mark.parametrize("ns,no,w,mu", [(4, 4, 0.125, 6), (4, 5, 0.0, 6), (4, 5, 0.125, 6), (4, 6, 0.0, 1), (2, 6, 0.25, 255),
                                        (8, 7, 1.0, 3), (3, 4, 0.3, 8), (1, 1, 0.0, 2), (5, 2, 0.5, 4)])
def test_position_bank_shape_and_the_other_filters(ns, no, w, mu):
    b = make_bank(ns, no, color_weight=w, position_weight=mu)
    tapq, shift, slots = pr.bank(ns, no, w, mu)
    assert slots == no + (w > 0) + 1 == pr.n_slots(no, w, mu)
    assert b.tapq.dtype == np.int16 and b.tapq.shape == (ns * slots, 2, 13, 13)
    assert np.array_equal(b.tapq, tapq) and b.shift == shift
    assert (b.n_orient, b.n_gabor_orient, b.color_weight, b.position_weight) == (slots, no, w, mu)
    assert b.n_filters == ns * slots and b.n_features == 3 * ns * slots
    without = make_bank(ns, no, color_weight=w)
    t = b.tapq.reshape(ns, slots, 2, 13, 13)
    assert not t[:, slots - 1].any()                                                 # the slot: all taps zero
    assert np.array_equal(t[:, :slots - 1].reshape(without.tapq.shape), without.tapq)   # every other filter bit for bit
    assert (b.exponent, b.shift) == (without.exponent, without.shift) and without.position_weight == 0
    assert (without.n_orient, without.n_gabor_orient) == (slots - 1, no)


def test_default_bank_is_unchanged():
    b, t = make_bank(), so.bank()
    assert np.array_equal(b.tapq, t[0]) and b.n_orient == 6 and b.n_features == 72 and b.position_weight == 0
    assert np.array_equal(make_bank(position_weight=0).tapq, b.tapq) and make_bank(position_weight=0).n_orient == 6
    assert make_bank(4, 4, color_weight=0.125, position_weight=6).n_features == 72   # the recommended plan: the default's shape


def test_bank_pack_accepts_the_zero_slot(built):
    lib = _lib.load()
    for ns, no, w, mu in ((4, 4, 0.125, 6), (4, 5, 0.125, 6), (4, 5, 0.0, 255), (8, 7, 1.0, 1), (1, 1, 0.0, 9), (2, 3, 0.0, 6)):
        b = make_bank(ns, no, color_weight=w, position_weight=mu)
        packed = np.zeros(lib.gcs_bank_packed_bytes(ns, b.n_orient), np.int8)
        bias = np.zeros(lib.gcs_bank_bias_count(ns, b.n_orient), np.int32)
        tapq = np.ascontiguousarray(b.tapq)
        assert lib.gcs_bank_pack(tapq.ctypes.data, ns, b.n_orient, 13, packed.ctypes.data, bias.ctypes.data) == 0
    assert lib.gcs_feature_slab_bytes(64, 321, 481, 4, make_bank(4, 4, color_weight=0.125, position_weight=6).n_orient) == \
        lib.gcs_feature_slab_bytes(64, 321, 481, 4, 6)


# ---- parameters

@pytest.mark.parametrize("bad", [True, False, 6.0, 0.5, 256, -1, 1 << 20, float("nan"), "6", None])
def test_position_weight_argument_errors(bad):
    with pytest.raises(ValueError):
        make_bank(position_weight=bad)
    with pytest.raises(ValueError):
        Segmenter(ops=OracleOps(make_bank()), position_weight=bad)
    with pytest.raises(ValueError):
        segment(np.zeros((8, 8, 3), np.uint8), position_weight=bad)


def test_numpy_integers_are_integers():
    assert make_bank(position_weight=np.int64(6)).position_weight == 6
    assert make_bank(position_weight=np.uint8(255)).position_weight == 255


def _seg(mu=6, w=0.125, g=4, no=4, smoothing=0.0, **kw):
    return Segmenter(n_orient=no, ops=PositionOps(make_bank(4, no, color_weight=w, position_weight=mu), g, smoothing), n_iter=3,
                     color_weight=w, chroma_gain=g, smoothing=smoothing, position_weight=mu, **kw)


def test_range_rule_raises_at_the_call():
    """mu (max(height, W) - 1) <= 46 340: 255 reaches 182 pixels and no further; on a strip the FULL image's rows count."""
    assert pr.in_domain(255, 182, 100) and not pr.in_domain(255, 183, 100) and not pr.in_domain(255, 100, 183)
    ok, tall, wide = (np.zeros((2, h, w, 3), np.uint8) for h, w in ((182, 24), (183, 24), (24, 183)))
    seg = _seg(255)
    seg.segment_batch(ok[:1])
    n_calls = len(seg.ops.calls)
    for bad in (tall, wide):
        with pytest.raises(ValueError, match="position_weight"):
            seg.segment_batch(bad)
        with pytest.raises(ValueError, match="position_weight"):
            seg.segment_device(torch.from_numpy(bad))
        with pytest.raises(ValueError, match="position_weight"):
            seg.features_device(torch.from_numpy(bad))
        with pytest.raises(ValueError, match="position_weight"):
            list(seg.segment_stream([bad]))
        with pytest.raises(ValueError, match="position_weight"):
            list(seg.segment_images(list(bad)))
        with pytest.raises(ValueError, match="position_weight"):
            seg(bad[0])
    assert len(seg.ops.calls) == n_calls                                   # refused before any stage ran
    strip = torch.zeros((1, 64, 24, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="position_weight"):
        seg.segment_rows_sharded_device(strip, 0, 52, 0, 183)              # the first 64 rows of a 183-row image
    seg.segment_rows_sharded_device(strip, 0, 64, 0, 64)
    assert _seg(8).segment_batch(np.zeros((1, 481, 8, 3), np.uint8)).shape == (1, 481, 8)      # mu <= 8: below 4096 on BSD sides


def test_ops_must_carry_the_same_position_bank():
    with pytest.raises(ValueError, match="same position bank"):
        Segmenter(ops=OracleOps(make_bank()), position_weight=6)
    with pytest.raises(ValueError, match="same position bank"):
        Segmenter(ops=PositionOps(make_bank(position_weight=4)), position_weight=6)
    with pytest.raises(ValueError, match="same position bank"):
        Segmenter(ops=PositionOps(make_bank(position_weight=6)))
    with pytest.raises(ValueError, match="same position bank"):
        Segmenter(n_orient=5, ops=PositionOps(make_bank(4, 6, position_weight=6)), position_weight=6)
    with pytest.raises(ValueError, match="same position bank"):
        Segmenter(ops=OracleOps(make_bank(position_weight=6)), position_weight=6)      # ops without the entry point
    Segmenter(n_orient=5, ops=PositionOps(make_bank(4, 5, position_weight=6)), position_weight=6)


# ---- the restatement against a direct per-pixel loop

@pytest.mark.parametrize("h,w,ns,no,cw,mu,y0", [(9, 13, 4, 2, 0.0, 6, 0), (17, 8, 4, 1, 0.125, 255, 0), (11, 15, 8, 2, 0.0, 7, 8),
                                                (8, 8, 1, 3, 0.0, 1, 0), (13, 21, 5, 1, 0.5, 100, 4), (10, 9, 2, 2, 0.0, 33, 3)])
def test_restatement_equals_a_per_pixel_loop(h, w, ns, no, cw, mu, y0):
    img = synthetic_batch(1, h, w, seed=h * w)[0]
    got = pr.features(img, cw, 0, mu, ns, no, y0=y0)
    slots = no + (cw > 0) + 1
    f_n = ns * slots
    base = cr.features(img, cw, 0, ns, no)                                 # the bank without the slot
    assert got.shape == (3 * f_n, h, w) and got.dtype == np.uint16
    for c in range(3):
        for s in range(ns):
            lv = s // 2
            for o in range(slots):
                plane = got[c * f_n + s * slots + o]
                if o < slots - 1:
                    assert np.array_equal(plane, base[c * ns * (slots - 1) + s * (slots - 1) + o]), (c, s, o)
                    continue
                for y in range(h):
                    for x in range(w):
                        want = (mu * (y0 + ((y >> lv) << lv)), mu * ((x >> lv) << lv), 0)[c]
                        assert plane[y, x] == want, (c, s, y, x)


def test_weight_in_the_squared_distance():
    """Each coordinate appears once per scale: two pixels one level-0 row apart differ by n_scales mu^2 in the slot's planes (on
    the scales of level 0; coarser levels quantise to 2^L pixels)."""
    f = pr.fill_slot(np.zeros((3 * 4 * 2, 16, 16), np.uint16), 4, 2, 6).astype(np.int64)
    d = ((f[:, 8, 5] - f[:, 0, 5]) ** 2).sum()
    assert d == 4 * 36 * 64                                                # 8 rows apart: exact on both levels
    assert ((f[:, 1, 5] - f[:, 0, 5]) ** 2).sum() == 2 * 36               # one row apart: the two level-0 scales only


# ---- Segmenter plumbing (CPU stand-in)

def _order(calls):
    """Names of the recorded calls up to and including the first Lloyd pass."""
    names = [c[0] for c in calls]
    return names[:names.index("assign") + 1]


def test_defaults_launch_nothing_new():
    imgs = synthetic_batch(2, 24, 40, seed=9)
    seg = Segmenter(ops=PositionOps(make_bank()), n_iter=3, position_weight=0)
    got = seg.segment_device(torch.from_numpy(imgs)).numpy()
    assert seg.position_weight == 0 and not any(c[0] == "position" for c in seg.ops.calls)
    for b in range(2):
        assert np.array_equal(got[b], so.segment(imgs[b], n_iter=3))
    assert seg.bank.n_orient == 6 and np.array_equal(seg.bank.tapq, make_bank().tapq)


def test_position_runs_behind_gabor_and_smoothing_on_every_host_path():
    imgs = synthetic_batch(3, 24, 40, seed=4)
    kw = dict(n_iter=3, n_orient=4)
    want = pr.segment_batch(imgs, 0.125, 4, 6, **kw)
    keep = imgs.copy()

    seg = _seg()
    assert np.array_equal(seg.segment_device(torch.from_numpy(imgs)).numpy(), want)
    assert _order(seg.ops.calls) == ["colour", "gabor", "position", "assign"]

    seg = _seg()
    assert np.array_equal(seg.segment_batch(imgs), want)
    assert _order(seg.ops.calls) == ["colour", "gabor", "position", "assign"]
    assert np.array_equal(seg(imgs[1]), want[1])
    assert np.array_equal(seg.segment_batch(imgs, out_dtype=np.uint8), want.astype(np.uint8))

    seg = _seg()
    ims = [imgs[0], imgs[1][:16], imgs[2]]
    for im, lab in zip(ims, seg.segment_images(ims, batch=2)):
        assert np.array_equal(lab, pr.segment(im, 0.125, 4, 6, **kw))
    names = [c[0] for c in seg.ops.calls]
    assert names.count("position") == names.count("gabor") == 2
    assert all(names[i + 1] == "position" for i, n in enumerate(names) if n == "gabor")

    seg = _seg()
    assert np.array_equal(np.concatenate(list(seg.segment_stream([imgs[:2], imgs[2:]]))), want)

    seg = _seg()
    f = seg.features_device(torch.from_numpy(imgs[:2])).numpy().view(np.uint16)
    for b in range(2):
        assert np.array_equal(f[b], pr.features(imgs[b], 0.125, 4, 6, n_orient=4))
    assert [c[0] for c in seg.ops.calls] == ["colour", "gabor", "position"]

    seg = _seg()
    assert np.array_equal(seg.segment_batch(imgs, mode="global"), pr.segment_batch(imgs, 0.125, 4, 6, mode="global", **kw))

    seg = _seg(smoothing=1.0)
    got = seg.segment_batch(imgs)
    assert np.array_equal(got, pr.segment_batch(imgs, 0.125, 4, 6, smoothing=1.0, **kw))
    assert _order(seg.ops.calls) == ["colour", "gabor", "smooth", "position", "assign"]
    f = seg.features_device(torch.from_numpy(imgs[:1])).numpy().view(np.uint16)[0]
    assert np.array_equal(f, pr.features(imgs[0], 0.125, 4, 6, n_orient=4, smoothing=1.0))      # the slot is never smoothed
    assert np.array_equal(f[5], pr.slot_planes(24, 40, 0, 6)[0]) and np.array_equal(f[24 + 23], pr.slot_planes(24, 40, 3, 6)[1])

    assert np.array_equal(imgs, keep)
    assert not np.array_equal(want, cr.segment_batch(imgs, 0.125, 4, **kw))                    # the slot changes labels
    assert not np.array_equal(want, pr.segment_batch(imgs, 0.125, 4, 4, **kw))                 # and so does mu

    # the module-level calls take the option through **kw (no GPU here: the plan is built before the ops are)
    for call in (lambda **k: segment(imgs[0], **k), lambda **k: segment_batch(imgs, **k), lambda **k: list(segment_images(imgs, **k))):
        with pytest.raises(ValueError, match="position_weight"):
            call(position_weight=256)


def test_plain_bank_with_the_slot_and_min_region_size():
    from merge_ref import merge_small_regions
    imgs = synthetic_batch(2, 24, 40, seed=3)
    seg = _seg(4, 0.0, 0, 5)
    assert np.array_equal(seg.segment_batch(imgs), pr.segment_batch(imgs, 0.0, 0, 4, n_iter=3, n_orient=5))
    assert _order(seg.ops.calls) == ["gabor", "position", "assign"]
    seg = _seg(min_region_size=20)
    got = seg.segment_batch(imgs)
    for b in range(2):
        assert np.array_equal(got[b], merge_small_regions(pr.segment(imgs[b], 0.125, 4, 6, n_iter=3, n_orient=4), 20))
    with pytest.raises(ValueError, match="int32"):
        seg.segment_batch(imgs, out_dtype=np.uint8)


def test_row_strips_carry_global_rows():
    """A strip of rows [s0, s1) is told y0 = s0, and its features equal those rows of the whole image's coordinate planes."""
    imgs = synthetic_batch(1, 64, 24, seed=2)
    seg = _seg()
    whole = seg.segment_rows_sharded_device(torch.from_numpy(imgs), 0, 64, 0, 64).numpy()
    assert np.array_equal(whole, pr.segment_batch(imgs, 0.125, 4, 6, n_iter=3, n_orient=4, mode="global"))
    assert _order(seg.ops.calls) == ["colour", "gabor", "position", "assign"]
    assert [c for c in seg.ops.calls if c[0] == "position"] == [("position", 1, 0)]
    seg = _seg()
    r0, r1, s0, s1 = seg.shard_rows(64, 2, 1)
    assert s0 > 0 and s0 % 2 == 0
    seg.segment_rows_sharded_device(torch.from_numpy(np.ascontiguousarray(imgs[:, s0:s1])), r0, r1, s0, 64)
    assert [c for c in seg.ops.calls if c[0] == "position"] == [("position", 1, s0)]
    full = pr.features(imgs[0], 0.125, 4, 6, n_orient=4)
    part = pr.features(np.ascontiguousarray(imgs[0, s0:s1]), 0.125, 4, 6, n_orient=4, y0=s0)
    slot = [c * 24 + s * 6 + 5 for c in range(3) for s in range(4)]
    assert np.array_equal(part[slot], full[slot][:, s0:s1])


def test_owned_rows_entry_passes_the_strip_offset():
    import tempfile
    import torch.distributed as td
    imgs = synthetic_batch(1, 32, 24, seed=2)
    with tempfile.TemporaryDirectory() as tmp:
        td.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "rdv"), rank=0, world_size=1)
        try:
            seg = _seg()
            got = seg.segment_owned_rows_device(torch.from_numpy(imgs), 32).numpy()
        finally:
            td.destroy_process_group()
    assert np.array_equal(got, pr.segment_batch(imgs, 0.125, 4, 6, n_iter=3, n_orient=4, mode="global"))
    assert _order(seg.ops.calls) == ["colour", "gabor", "position", "assign"]


# ---- quality of the restatement on the val fixture (DESIGN.md §7 has the table; tools/position_quality.py writes it)

BOLD = dict(w=0.125, g=4, mu=6, n_orient=4)          # the recommended setting: D = 72, the default's shape


def _scores(lab, truth):
    bs, ra = boundary_scores(lab, truth), region_agreement(lab, truth)
    return [bs["fmeasure"], ra["PRI"], ra["VoI"], ra["covering"]]


def _val():
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    return val, PackedTruth(os.path.join(GOLD, "bsd500_truth.npz")), [str(i) for i in val["ids"]]


def test_quality_bounds_on_the_val_fixture(built):
    """The recommended row against its own mu = 0 plan (n_orient = 4, w = 1/8, g = 4) on all 24 images: mean boundary F higher and
    mean VoI lower. Measured when the option was proposed: F 0.4056 > 0.3794, VoI 2.6453 < 3.2296."""
    val, pt, ids = _val()
    rows = {mu: np.mean([_scores(pr.segment(val["img_" + i], BOLD["w"], BOLD["g"], mu, n_orient=BOLD["n_orient"]), pt[i])
                         for i in ids], axis=0) for mu in (0, BOLD["mu"])}
    print("mu = 0:", rows[0].tolist(), "mu = 6:", rows[6].tolist())
    assert rows[6][0] > rows[0][0], (rows[6][0], rows[0][0])
    assert rows[6][2] < rows[0][2], (rows[6][2], rows[0][2])


# boundary F, PRI, VoI, covering of each of the FIRST SIX val fixture images (ids[:6]) at the recommended setting (see the docstring)
QUALITY_6 = [
    [0.6239306523523623, 0.8361769125465074, 3.467752805229061, 0.29923687854055847],
    [0.6319851252188252, 0.8584288452956071, 2.3557005947265095, 0.41080565303853234],
    [0.3275425570942075, 0.7831947547387961, 2.192954911278089, 0.40299521755040757],
    [0.4123492288951382, 0.774312851006171, 3.0301856184492095, 0.3252045893387044],
    [0.37545369002182527, 0.8504694345479901, 2.028496564788735, 0.5612831669193237],
    [0.34819119254001424, 0.6795814842604344, 2.64723787360655, 0.33932432806131524],
]


def test_quality_pin_on_six_val_fixture_images(built):
    val, pt, ids = _val()
    got = [_scores(pr.segment(val["img_" + i], BOLD["w"], BOLD["g"], BOLD["mu"], n_orient=BOLD["n_orient"]), pt[i]) for i in ids[:6]]
    print("QUALITY_6 = [\n" + "".join(f"    {row!r},\n" for row in got) + "]")
    assert len(QUALITY_6) == 6
    assert np.all(np.abs(np.array(got) - np.array(QUALITY_6)) <= 1e-12), got


# ---- C ABI: host-only checks

def test_position_entry_validates_before_launching(built):
    lib = _lib.load()
    a = C.c_void_p(1 << 20)                                              # a non-NULL dummy, never dereferenced
    fn = lib.gcs_position_features
    assert fn(None, 1, 64, 64, 4, 6, 6, 0, None) == 1
    assert b"NULL" in lib.gcs_last_error()
    for shape in ((0, 64, 64, 4, 6), (1, 7, 64, 4, 6), (1, 64, 7, 4, 6), (1, 64, 64, 0, 6), (1, 64, 64, 9, 6), (1, 64, 64, 4, 0),
                  (65536, 64, 64, 4, 6)):
        assert fn(a, *shape, 6, 0, None) == 1, shape
        assert b"shape" in lib.gcs_last_error()
    for weight in (0, -1, 256, 1 << 20):
        assert fn(a, 1, 64, 64, 4, 6, weight, 0, None) == 1
        assert b"weight" in lib.gcs_last_error()
    # the range rule: weight (max(y0 + H, W) - 1) <= 46 340
    for h, w, mu, y0 in ((183, 64, 255, 0), (64, 183, 255, 0), (64, 64, 255, 120), (481, 321, 97, 0), (321, 481, 97, 0)):
        assert fn(a, 1, h, w, 4, 6, mu, y0, None) == 1, (h, w, mu, y0)
        assert b"46340" in lib.gcs_last_error()
    # y0: negative, or not a multiple of 2^(levels - 1)
    for ns, y0 in ((4, -2), (4, 1), (4, 7), (6, 2), (8, 4), (8, 12), (2, -1)):
        assert fn(a, 1, 64, 64, ns, 6, 6, y0, None) == 1, (ns, y0)
        assert b"y0" in lib.gcs_last_error()
