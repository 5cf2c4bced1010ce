"""GPU position features (SPEC.md §12): gcs_position_features and Segmenter(position_weight=mu) against the NumPy restatement
(tests/position_ref.py), bit for bit and never against the GPU's own output - the coordinate planes on split and wide slabs, on
packed edge strips and on one to four pyramid levels, the flag words of the split slab, guard bytes and the planes of every other
filter, labels on every call path, a two-rank row-sharded run (global rows), the compositions with smoothing, colour and
min_region_size, and the scores of the 24 val fixture images."""
import os
import sys

import numpy as np
import pytest

import position_ref as pr
from slab_layout import flag_bytes as _flags, tile_of_pixels as _tile_of_pixels

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _synth(b, h, w, seed):
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    return synthetic_batch(b, h, w, seed=seed)


# ---- the kernel: features_unpack after the Gabor stage + gcs_position_features

# n_scales, Gabor orientations, colour weight -> (levels, slab): the recommended plan (2, split D = 72), D = 84 (2, wide, packed
# strips on a wide slab), one level (split), one scale, an odd scale count (2, split), three levels (wide), four levels (wide)
BANKS = [(4, 4, 0.125), (4, 5, 0.125), (2, 6, 0.0), (1, 3, 0.0), (3, 5, 0.0), (6, 3, 0.0), (8, 2, 0.125)]
# 8x8; one- and two-pixel strips on either side; a 3-row edge (not packed) beside a one-pixel strip; whole blocks
SMALL = [(8, 8), (17, 26), (18, 17), (19, 33), (64, 64), (43, 90)]


@pytest.mark.parametrize("ns,no,w", BANKS)
@pytest.mark.parametrize("mu", [6, 255])
def test_features_small_shapes(torch_cuda, ns, no, w, mu):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    seg = Segmenter(n_scales=ns, n_orient=no, color_weight=w, position_weight=mu)
    assert seg.bank.n_features == 3 * ns * pr.n_slots(no, w, mu)
    for h, wd in SMALL:
        imgs = _synth(3, h, wd, seed=h * wd)
        got = seg.features_device(torch.from_numpy(imgs).cuda()).cpu().numpy().view(np.uint16)
        for i in range(3):
            want = pr.features(imgs[i], w, 0, mu, ns, no)
            assert np.array_equal(got[i], want), (ns, no, w, mu, h, wd, i, int((got[i] != want).sum()))


@pytest.mark.parametrize("h,wd", [(321, 481), (481, 321)])
@pytest.mark.parametrize("ns,no,w", BANKS)
def test_features_bsd_shapes(torch_cuda, h, wd, ns, no, w):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    g = 4 if w else 0
    for mu in (6, 96):                                                     # 96 * 480 = 46 080: the top of the value range
        seg = Segmenter(n_scales=ns, n_orient=no, color_weight=w, chroma_gain=g, position_weight=mu)
        imgs = _synth(2, h, wd, seed=7)
        got = seg.features_device(torch.from_numpy(imgs).cuda()).cpu().numpy().view(np.uint16)
        for i in range(2):
            want = pr.features(imgs[i], w, g, mu, ns, no)
            assert np.array_equal(got[i], want), (ns, no, mu, i, int((got[i] != want).sum()))


@pytest.mark.parametrize("ns,no,w", [(4, 4, 0.125), (4, 5, 0.125), (8, 2, 0.0)])
@pytest.mark.parametrize("h,wd,y0", [(17, 26, 0), (81, 121, 0), (64, 40, 56), (321, 481, 0)])
def test_guard_bytes_and_the_other_planes(torch_cuda, ns, no, w, h, wd, y0):
    """The raw entry point on a slab inside a larger buffer: the bytes in front of and behind the slab come back as they were, the
    planes of every other filter are unchanged, channel 2 of the slot stays zero, the slot's planes carry y0."""
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    mu, b, guard = 5, 2, 4096
    seg = Segmenter(n_scales=ns, n_orient=no, color_weight=w, position_weight=mu)
    lib, slots = _lib.load(), seg.bank.n_orient
    n = lib.gcs_feature_slab_bytes(b, h, wd, ns, slots)
    rng = np.random.default_rng(h * wd)
    fill = rng.integers(0, 256, n + 2 * guard).astype(np.uint8)
    buf = torch.from_numpy(fill).cuda()
    slab = buf[guard:guard + n]
    imgs = _synth(b, h, wd, seed=3)
    seg.ops.gabor_features(torch.from_numpy(imgs).cuda(), slab)
    before = seg.ops.features_unpack(slab, b, h, wd).cpu().numpy().view(np.uint16)
    raw_before = buf.cpu().numpy()
    rc = lib.gcs_position_features(slab.data_ptr(), b, h, wd, ns, slots, mu, y0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    after = seg.ops.features_unpack(slab, b, h, wd).cpu().numpy().view(np.uint16)
    raw_after = buf.cpu().numpy()
    assert np.array_equal(raw_after[:guard], fill[:guard]) and np.array_equal(raw_after[guard + n:], fill[guard + n:])
    assert np.array_equal(raw_before[:guard], fill[:guard])
    f_n = ns * slots
    slot = np.zeros(3 * f_n, bool)
    slot.reshape(3, ns, slots)[:2, :, slots - 1] = True
    for i in range(b):
        assert np.array_equal(after[i][~slot], before[i][~slot]), i
        assert not before[i][slot | np.roll(slot, f_n)].any()                             # zero taps: the Gabor stage left zeros
        want = pr.fill_slot(before[i].copy(), ns, slots, mu, y0)
        assert np.array_equal(after[i], want), (i, int((after[i] != want).sum()))
        assert not after[i].reshape(3, ns, slots, h, wd)[2, :, slots - 1].any()
    assert (raw_after != raw_before).sum() > 0


@pytest.mark.parametrize("h,wd,mu", [(64, 96, 64), (81, 121, 255), (130, 182, 255), (321, 481, 96)])
def test_flag_words_of_the_split_slab(torch_cuda, h, wd, mu):
    """Coordinate planes of 4096 and more: the tile's flag byte of the level is set where the restated features say, whichever
    stage raised it; flags the Gabor stage set (bright colour planes at w = 1/4) are never cleared; a flag set by nothing stays 0."""
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    base = _synth(3, h, wd, seed=77)
    bright = (base[0] // 4 + 192).astype(np.uint8)
    dark = (base[1] // 4).astype(np.uint8)
    half = base[2].copy()
    half[:, : wd // 2] = 250                                               # bright LEFT half: where the column planes are small
    imgs = np.stack([bright, dark, half])
    seg = Segmenter(n_orient=4, color_weight=0.25, position_weight=mu)
    feats = seg.ops.feature_slab(3, h, wd)
    seg.ops.gabor_features(torch.from_numpy(imgs).cuda(), feats)
    flags0, ntiles = _flags(seg, feats, 3, h, wd)
    flags0 = flags0.copy()
    seg.ops.position_features(feats, 3, h, wd)
    got = seg.ops.features_unpack(feats, 3, h, wd).cpu().numpy().view(np.uint16)
    flags, _ = _flags(seg, feats, 3, h, wd)
    tile = _tile_of_pixels(h, wd)
    assert tile.max() + 1 == ntiles
    slot = np.zeros((3, 4, 6), bool)
    slot[:2, :, 5] = True
    for i in range(3):
        want = pr.features(imgs[i], 0.25, 0, mu, 4, 4)
        assert np.array_equal(got[i], want), i
        for L in (0, 1):
            rows = [c * 24 + f for c in range(3) for f in range(12 * L, 12 * L + 12)]
            wl = np.zeros(ntiles, bool)
            wl[np.unique(tile[(want[rows] >= 4096).any(axis=0)])] = True
            assert np.array_equal(flags[i, :, L] != 0, wl), (i, L)
            pos_rows = [r for r in rows if slot.ravel()[r]]
            by_slot = np.zeros(ntiles, bool)
            by_slot[np.unique(tile[(want[pos_rows] >= 4096).any(axis=0)])] = True
            assert np.array_equal(flags[i, :, L] != 0, (flags0[i, :, L] != 0) | by_slot), (i, L)      # set, never cleared
            assert by_slot.any() and not by_slot.all() or mu == 255
        assert not flags[i, :, 2:].any()
    # the bright image: Gabor-stage flags everywhere, also on tiles the slot does not raise; the dark one: the slot's tiles only
    assert (flags0[0, :, :2] != 0).all() and (flags[0, :, :2] != 0).all()
    assert flags[1, :, :2].any()


def test_entry_point_argument_errors_launch_nothing(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    lib = _lib.load()
    seg = Segmenter(n_orient=5, position_weight=6)
    feats = seg.ops.feature_slab(1, 64, 64)
    feats.fill_(7)
    stream = torch.cuda.current_stream().cuda_stream
    p = feats.data_ptr()
    assert lib.gcs_position_features(None, 1, 64, 64, 4, 6, 6, 0, stream) == 1
    for args in ((0, 64, 64, 4, 6, 6, 0), (1, 7, 64, 4, 6, 6, 0), (1, 64, 64, 4, 6, 0, 0), (1, 64, 64, 4, 6, 256, 0),
                 (1, 64, 64, 4, 6, 255, 128), (1, 64, 64, 4, 6, 6, 1), (1, 64, 64, 4, 6, 6, -2)):
        assert lib.gcs_position_features(p, *args, stream) == 1, args
    torch.cuda.current_stream().synchronize()
    assert (feats.cpu().numpy() == 7).all()
    with pytest.raises(ValueError):
        Segmenter().ops.position_features(feats, 1, 64, 64)


# ---- labels and call paths

REC = dict(n_orient=4, color_weight=0.125, chroma_gain=4, position_weight=6)      # the recommended setting


def _want(imgs, **kw):
    return pr.segment_batch(imgs, 0.125, 4, 6, n_orient=4, **kw)


@pytest.mark.parametrize("mode", ["per_image", "global"])
@pytest.mark.parametrize("k,b", [(8, 1), (8, 3), (16, 3), (1, 2)])
def test_labels_both_codebook_modes(torch_cuda, mode, k, b):
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(b, 97, 131, seed=k + b)
    got = Segmenter(k=k, **REC).segment_batch(imgs, mode)
    assert np.array_equal(got, _want(imgs, k=k, mode=mode))


def test_labels_plain_bank_wide_slab_and_deep_bank(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(2, 321, 481, seed=12)
    got = Segmenter(n_orient=5, position_weight=6).segment_batch(imgs)                       # no colour: split, D = 72
    assert np.array_equal(got, pr.segment_batch(imgs, 0.0, 0, 6, n_orient=5))
    got = Segmenter(n_orient=5, color_weight=0.125, chroma_gain=4, position_weight=6).segment_batch(imgs)      # D = 84: wide
    assert np.array_equal(got, pr.segment_batch(imgs, 0.125, 4, 6, n_orient=5))
    got = Segmenter(n_scales=8, n_orient=3, position_weight=3).segment_batch(imgs[:1])       # four levels
    assert np.array_equal(got, pr.segment_batch(imgs[:1], 0.0, 0, 3, n_scales=8, n_orient=3))


def test_every_call_path_agrees(torch_cuda):
    """segment == the row of segment_batch (graph path and the chunked fast path) == segment_stream == segment_images ==
    segment_device; graph replay == eager; uint8 labels; features_device == the restatement."""
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, segment, segment_batch, segment_images
    imgs = _synth(8, 481, 321, seed=21)                       # 8 x 481x321 > 2^20 pixels: segment_batch's chunked fast path
    want = _want(imgs)
    seg = Segmenter(**REC)
    assert np.array_equal(seg.segment_batch(imgs), want)
    assert np.array_equal(segment_batch(imgs[:2], **REC), want[:2])                    # graph path, a batch
    assert np.array_equal(segment(imgs[3], **REC), want[3])
    assert np.array_equal(seg.segment_batch(imgs, out_dtype=np.uint8), want.astype(np.uint8))
    dev = torch.from_numpy(imgs).cuda()
    assert np.array_equal(seg.segment_device(dev).cpu().numpy(), want)
    outs = list(seg.segment_stream([imgs[:4], imgs[4:]]))
    assert np.array_equal(np.concatenate(outs), want)                                  # segment_stream == segment_batch
    mixed = [imgs[0], np.ascontiguousarray(imgs[1].transpose(1, 0, 2)), imgs[2]]
    got = list(segment_images(mixed, batch=2, **REC))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], pr.segment(mixed[1], 0.125, 4, 6, n_orient=4))
    big = list(seg.segment_images(list(imgs), batch=4))                                # full batches: the three-stream pipeline
    assert np.array_equal(np.stack(big), want)
    for i in range(8):
        assert np.array_equal(seg(imgs[i]), want[i])                                   # replayed graph
    eager = Segmenter(**REC)
    eager.debug.no_graph = True
    assert np.array_equal(eager.segment_batch(imgs[:1]), want[:1])                     # graph replay == eager
    f = seg.features_device(dev[:2]).cpu().numpy().view(np.uint16)
    for i in range(2):
        assert np.array_equal(f[i], pr.features(imgs[i], 0.125, 4, 6, 4, 4))


def test_default_is_off_and_unchanged(torch_cuda):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, segment
    from oracle import c_oracle as co
    from oracle import spec_oracle as so
    imgs = _synth(2, 321, 481, seed=5)
    plain = Segmenter().segment_batch(imgs)
    zero = Segmenter(position_weight=0)
    assert np.array_equal(zero.segment_batch(imgs), plain)
    assert np.array_equal(segment(imgs[0], position_weight=0), plain[0])
    tapq, shift = so.bank()
    assert np.array_equal(plain, co.segment_batch(imgs, tapq, shift, 6))
    dev = torch.from_numpy(imgs).cuda()
    assert np.array_equal(zero.features_device(dev).cpu().numpy(), Segmenter().features_device(dev).cpu().numpy())
    assert not np.array_equal(Segmenter(n_orient=5, position_weight=6).segment_batch(imgs), plain)


def test_ops_built_for_another_bank_are_refused_and_the_range_rule_holds(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    a = Segmenter(**REC)
    with pytest.raises(ValueError, match="same position bank"):
        Segmenter(n_orient=4, color_weight=0.125, chroma_gain=4, position_weight=4, ops=a.ops)
    with pytest.raises(ValueError, match="same position bank"):
        Segmenter(n_orient=5, color_weight=0.125, chroma_gain=4, ops=a.ops)
    Segmenter(ops=a.ops, **REC)
    tall = Segmenter(n_orient=5, position_weight=97)
    for bad in (np.zeros((1, 481, 321, 3), np.uint8), np.zeros((7, 321, 481, 3), np.uint8)):      # graph path and chunked path
        with pytest.raises(ValueError, match="position_weight"):
            tall.segment_batch(bad)
        with pytest.raises(ValueError, match="position_weight"):
            list(tall.segment_stream([bad]))
    assert tall.segment_batch(np.zeros((1, 400, 321, 3), np.uint8)).shape == (1, 400, 321)


@pytest.mark.parametrize("kw,ref", [
    (dict(REC, smoothing=1.0), dict(smoothing=1.0)),
    (dict(n_orient=5, position_weight=4, smoothing=1.0), dict(w=0.0, g=0, mu=4, n_orient=5, smoothing=1.0)),
    (dict(n_orient=4, color_weight=0.125, position_weight=8), dict(g=0, mu=8)),
    (dict(n_orient=5, chroma_gain=4, position_weight=6), dict(w=0.0, n_orient=5)),
])
def test_with_smoothing_and_the_colour_options(torch_cuda, kw, ref):
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(2, 321, 481, seed=31)
    r = dict(dict(w=0.125, g=4, mu=6, n_orient=4), **ref)
    got = Segmenter(**kw).segment_batch(imgs)
    assert np.array_equal(got, pr.segment_batch(imgs, r.pop("w"), r.pop("g"), r.pop("mu"), **r))


def test_with_min_region_size(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    from merge_ref import merge_small_regions
    imgs = _synth(2, 321, 481, seed=32)
    seg = Segmenter(min_region_size=64, **REC)
    got = seg.segment_batch(imgs)
    want = _want(imgs)
    for i in range(2):
        assert np.array_equal(got[i], merge_small_regions(want[i], 64)), i
    got = Segmenter(min_region_size=64, smoothing=1.0, **REC).segment_batch(imgs[:1])
    assert np.array_equal(got[0], merge_small_regions(_want(imgs[:1], smoothing=1.0)[0], 64))


# ---- two ranks, row-sharded: the strips carry global rows

def _strip_worker(rank, world, port, height, width, tmp, owned):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = synthetic_batch(1, height, width, seed=13)
    seg = Segmenter(n_iter=5, device="cuda:0", **REC)
    r0, r1, s0, s1 = seg.shard_rows(height, world, rank)
    if owned:
        out = seg.segment_owned_rows_device(torch.from_numpy(np.ascontiguousarray(imgs[:, r0:r1])).cuda(), height)
    else:
        out = seg.segment_rows_sharded_device(torch.from_numpy(np.ascontiguousarray(imgs[:, s0:s1])).cuda(), r0, r1, s0, height)
    np.save(os.path.join(tmp, f"strip_{rank}.npy"), out.cpu().numpy())
    dist.destroy_process_group()


@pytest.mark.parametrize("owned", [False, True])
def test_row_sharded_two_ranks(tmp_path, built, owned):
    """Two processes share cuda:0, gloo carries the tiny collectives: the second strip's rows count from s0, not from 0, so the
    joined strips equal the unsharded labels."""
    import torch.multiprocessing as mp
    height, width = 202, 137
    port = 36500 + (os.getpid() % 2000) + int(owned)
    mp.spawn(_strip_worker, args=(2, port, height, width, str(tmp_path), owned), nprocs=2, join=True)
    got = np.concatenate([np.load(tmp_path / f"strip_{r}.npy") for r in range(2)], axis=1)
    want = _want(_synth(1, height, width, seed=13), n_iter=5, mode="global")
    assert np.array_equal(got, want)


# ---- quality through the GPU

# means over the 24 val fixture images of boundary F, PRI, VoI, covering at the recommended setting, from the
# restatement on the CPU (tools/position_quality.py); k = 8, raw cluster labels
QUALITY_24 = (0.4056486018932675, 0.749364136294176, 2.645327944107509, 0.38665203187715386)


def test_quality_on_the_val_fixture_through_the_gpu(torch_cuda):
    """The 24 val images through the recommended plan and the batched GPU scorer: the restatement's labels, and its means."""
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    ids = [str(i) for i in val["ids"]]
    seg = Segmenter(**REC)
    rows = {}
    for shape in ((321, 481), (481, 321)):
        group = [i for i in ids if val["img_" + i].shape[:2] == shape]
        labs = seg.segment_batch(np.stack([val["img_" + i] for i in group]))
        scores = all_scores_batch_device(torch.from_numpy(labs).cuda(), pt.to_device(group), agreement=True)
        for i, lab, sc in zip(group, labs, scores):
            assert np.array_equal(lab, pr.segment(val["img_" + i], 0.125, 4, 6, n_orient=4)), i
            rows[i] = [sc["fmeasure"], sc["PRI"], sc["VoI"], sc["covering"]]
    got = np.mean([rows[i] for i in ids], axis=0)
    assert np.all(np.abs(got - np.array(QUALITY_24)) <= 1e-12), got.tolist()
