"""GPU colour features (SPEC.md §11): gcs_colour_opponent and Segmenter(color_weight=w, chroma_gain=g) against the NumPy
restatement (tests/colour_ref.py), bit for bit and never against the GPU's own output - the transform on all 2^24 RGB triples and
at every byte alignment inside guarded buffers, the features of colour banks on split and wide slabs, the flag words of the split
slab, labels on every call path, a two-rank row-sharded run, the compositions with smoothing and min_region_size, and the scores of
the 24 val fixture images."""
import os
import sys

import numpy as np
import pytest

import colour_ref as cr
from oracle import c_oracle as co
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


def _transform(torch, src, n_pixels, gain, dst):
    """gcs_colour_opponent on raw device pointers (uint8 tensors, already offset by the caller) -> return code."""
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load().gcs_colour_opponent(src.data_ptr(), n_pixels, gain, dst.data_ptr(), torch.cuda.current_stream().cuda_stream)


# ---- the transform kernel

@pytest.mark.parametrize("gain", [1, 2, 4, 16])
def test_transform_on_all_rgb_triples(torch_cuda, gain):
    """One 4096 x 4096 image that holds every (R, G, B) once."""
    torch = torch_cuda
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([v >> 16, v >> 8 & 255, v & 255], -1).astype(np.uint8)
    src = torch.from_numpy(rgb).cuda()
    dst = torch.zeros_like(src)
    assert _transform(torch, src, 1 << 24, gain, dst) == 0
    got = dst.cpu().numpy()
    want = cr.opponent(rgb, gain)
    assert np.array_equal(got, want), int((got != want).any(axis=1).sum())
    assert np.array_equal(src.cpu().numpy(), rgb)                          # the input is not changed


@pytest.mark.parametrize("n", [1, 2, 5, 15, 16, 17, 63, 481 * 321])
def test_transform_at_every_byte_alignment_inside_guards(torch_cuda, n):
    """Source and destination offsets 0..15 bytes inside larger buffers: the 3 n bytes equal the restatement, every other byte of
    both buffers comes back as it was."""
    torch = torch_cuda
    rng = np.random.default_rng(n)
    guard = 256
    size = 3 * n + 2 * guard + 16
    src_np = rng.integers(0, 256, size).astype(np.uint8)
    dst_np = rng.integers(0, 256, size).astype(np.uint8)
    src = torch.from_numpy(src_np).cuda()
    assert src.data_ptr() % 16 == 0
    # (all 256 offset pairs for the short lengths; for the BSD image every destination offset with two source offsets each)
    pairs = [(so_, do) for so_ in range(16) for do in range(16)] if n < 1000 else \
        [((5 * do + 3) % 16, do) for do in range(16)] + [(do, do) for do in range(16)]
    for gain, (s_off, d_off) in zip(np.resize([1, 2, 4, 16, 3, 7], len(pairs)).tolist(), pairs):
        dst = torch.from_numpy(dst_np).cuda()
        assert dst.data_ptr() % 16 == 0
        a, b = guard + s_off, guard + d_off
        assert _transform(torch, src[a:], n, gain, dst[b:]) == 0
        got = dst.cpu().numpy()
        want = dst_np.copy()
        want[b:b + 3 * n] = cr.opponent(src_np[a:a + 3 * n].reshape(n, 3), gain).ravel()
        assert np.array_equal(got[b:b + 3 * n], want[b:b + 3 * n]), (n, gain, s_off, d_off)
        assert np.array_equal(got, want), (n, gain, s_off, d_off, "guard bytes written")
    assert np.array_equal(src.cpu().numpy(), src_np)


def test_transform_argument_errors_launch_nothing(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    src = torch.arange(96, dtype=torch.uint8, device="cuda")
    dst = torch.full((96,), 7, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.gcs_colour_opponent(None, 16, 4, dst.data_ptr(), stream) == 1
    assert lib.gcs_colour_opponent(src.data_ptr(), 16, 4, None, stream) == 1
    for gain in (0, -1, 17):
        assert lib.gcs_colour_opponent(src.data_ptr(), 16, gain, dst.data_ptr(), stream) == 1
    assert lib.gcs_colour_opponent(src.data_ptr(), 0, 4, dst.data_ptr(), stream) == 1
    assert lib.gcs_colour_opponent(src.data_ptr(), 16, 4, src.data_ptr(), stream) == 1             # in place
    assert lib.gcs_colour_opponent(src.data_ptr(), 16, 4, src.data_ptr() + 47, stream) == 1        # one byte of overlap
    assert lib.gcs_colour_opponent(src.data_ptr() + 47, 16, 4, src.data_ptr(), stream) == 1
    torch.cuda.current_stream().synchronize()
    assert (dst.cpu().numpy() == 7).all() and np.array_equal(src.cpu().numpy(), np.arange(96, dtype=np.uint8))
    assert lib.gcs_colour_opponent(src.data_ptr(), 16, 4, src.data_ptr() + 48, stream) == 0        # adjacent ranges are fine
    got = src.cpu().numpy()
    assert np.array_equal(got[48:], cr.opponent(got[:48].reshape(16, 3), 4).ravel())


def test_hipops_colour_opponent_checks_its_tensors(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    seg = Segmenter(chroma_gain=2)
    imgs = torch.from_numpy(_synth(2, 9, 13, seed=1)).cuda()
    out = seg.ops.colour_scratch(2, 9, 13)
    seg.ops.colour_opponent(imgs, out)
    assert np.array_equal(out.cpu().numpy(), cr.opponent(imgs.cpu().numpy(), 2))
    seg.ops.colour_opponent(imgs[1:], out[:1])                             # a slice: an odd byte offset (9 * 13 * 3 = 351)
    assert np.array_equal(out[0].cpu().numpy(), cr.opponent(imgs[1].cpu().numpy(), 2))
    with pytest.raises(ValueError):
        seg.ops.colour_opponent(imgs, out[:1])
    with pytest.raises(ValueError):
        seg.ops.colour_opponent(imgs.to(torch.int8), out)
    with pytest.raises(ValueError):
        Segmenter().ops.colour_opponent(imgs, out)


# ---- features

_FEATS = {}


def _ref_features(img, ns, no, w, g):
    key = (img.tobytes(), img.shape, ns, no, w, g)
    if key not in _FEATS:
        _FEATS[key] = cr.features(img, w, g, ns, no)
    return _FEATS[key]


# n_scales, Gabor orientations (+ 1 slot): split slab of the default shape, wide D = 84, one level, four levels
BANKS = [(4, 5), (4, 6), (2, 6), (8, 7)]


@pytest.mark.parametrize("ns,no", BANKS)
@pytest.mark.parametrize("g", [0, 4])
@pytest.mark.parametrize("w", [0.125, 1.0])
def test_features_small_shapes(torch_cuda, ns, no, g, w):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    seg = Segmenter(n_scales=ns, n_orient=no, color_weight=w, chroma_gain=g)
    assert seg.bank.n_features == 3 * ns * (no + 1)
    for h, wd in ((8, 8), (9, 13), (17, 8), (64, 64)):
        imgs = _synth(3, h, wd, seed=h * wd)
        got = seg.features_device(torch.from_numpy(imgs).cuda()).cpu().numpy().view(np.uint16)
        for i in range(3):
            want = _ref_features(imgs[i], ns, no, w, g)
            assert np.array_equal(got[i], want), (ns, no, w, g, h, wd, i, int((got[i] != want).sum()))


@pytest.mark.parametrize("h,wd", [(321, 481), (481, 321)])
@pytest.mark.parametrize("ns,no", BANKS)
@pytest.mark.parametrize("g", [0, 4])
def test_features_bsd_shapes(torch_cuda, h, wd, ns, no, g):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    seg = Segmenter(n_scales=ns, n_orient=no, color_weight=0.125, chroma_gain=g)
    imgs = _synth(2, h, wd, seed=7)
    got = seg.features_device(torch.from_numpy(imgs).cuda()).cpu().numpy().view(np.uint16)
    for i in range(2):
        want = _ref_features(imgs[i], ns, no, 0.125, g)
        assert np.array_equal(got[i], want), (ns, no, g, i, int((got[i] != want).sum()))


def test_features_on_val_images_and_a_saturating_gain(torch_cuda):
    """Real photographs (both BSD orientations) at g = 16, where T_g clamps on many pixels."""
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    seg = Segmenter(n_orient=5, color_weight=0.125, chroma_gain=16)
    seen = set()
    for i in val["ids"]:
        img = val["img_" + str(i)]
        if img.shape in seen:
            continue
        seen.add(img.shape)
        t = cr.opponent(img, 16)
        assert ((t[..., 1:] == 0) | (t[..., 1:] == 255)).mean() > 0.01
        got = seg.features_device(torch.from_numpy(img[None]).cuda()).cpu().numpy().view(np.uint16)[0]
        assert np.array_equal(got, _ref_features(img, 4, 5, 0.125, 16))
    assert len(seen) == 2


@pytest.mark.parametrize("h,wd", [(64, 96), (81, 121), (321, 481)])
@pytest.mark.parametrize("g", [0, 2])
def test_flag_words_of_the_split_slab(torch_cuda, h, wd, g):
    """w = 1/4 on bright images: colour planes reach 4096 and more (up to 8156), so TOP flags are set by the slot - exactly on the
    tiles, and in the level bytes, where the restated features say; a dark image sets none through the slot."""
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    base = _synth(3, h, wd, seed=77)
    bright = (base[0] // 4 + 192).astype(np.uint8)                        # 192..255
    dark = (base[1] // 4).astype(np.uint8)                                # 0..63
    half = base[2].copy()
    half[:, : wd // 2] = 250                                               # bright left half
    imgs = np.stack([bright, dark, half])
    seg = Segmenter(n_orient=5, color_weight=0.25, chroma_gain=g)
    feats = seg.ops.feature_slab(3, h, wd)
    dev = torch.from_numpy(imgs).cuda()
    seg.ops.gabor_features(seg._opponent(dev, seg.ops.colour_scratch(3, h, wd)) if g else dev, feats)
    got = seg.ops.features_unpack(feats, 3, h, wd).cpu().numpy().view(np.uint16)
    flags, ntiles = _flags(seg, feats, 3, h, wd)
    tile = _tile_of_pixels(h, wd)
    assert tile.max() + 1 == ntiles
    slot_rows = [c * 24 + s * 6 + 5 for c in range(3) for s in range(4)]
    for i in range(3):
        want = _ref_features(imgs[i], 4, 5, 0.25, g)
        assert np.array_equal(got[i], want), i
        for L in (0, 1):
            rows = [c * 24 + f for c in range(3) for f in range(12 * L, 12 * L + 12)]
            wl = np.zeros(ntiles, bool)
            wl[np.unique(tile[(want[rows] >= 4096).any(axis=0)])] = True
            assert np.array_equal(flags[i, :, L] != 0, wl), (i, L)
        assert not flags[i, :, 2:].any()
    assert (_ref_features(imgs[0], 4, 5, 0.25, g)[slot_rows[:4]] >= 4096).all()      # the Y / R plane of the bright image: everywhere
    assert (flags[0, :, :2] != 0).all()
    assert (_ref_features(imgs[1], 4, 5, 0.25, g)[slot_rows[:4]] < 4096).all()


# ---- labels and call paths

SETTINGS = [(0.125, 0), (0.125, 4)]          # (w, g) at n_orient = 5: the two recommended settings


@pytest.mark.parametrize("mode", ["per_image", "global"])
@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("w,g", SETTINGS)
def test_labels_both_codebook_modes(torch_cuda, mode, k, w, g):
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(3, 97, 131, seed=k)
    got = Segmenter(n_orient=5, k=k, color_weight=w, chroma_gain=g).segment_batch(imgs, mode)
    assert np.array_equal(got, cr.segment_batch(imgs, w, g, k=k, mode=mode, n_orient=5))


def test_labels_wide_slab_d84_and_deep_bank(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(2, 321, 481, seed=12)
    got = Segmenter(n_orient=6, color_weight=0.125, chroma_gain=4).segment_batch(imgs)
    assert np.array_equal(got, cr.segment_batch(imgs, 0.125, 4, n_orient=6))
    got = Segmenter(n_scales=8, n_orient=7, color_weight=0.5, chroma_gain=2).segment_batch(imgs[:1])
    assert np.array_equal(got, cr.segment_batch(imgs[:1], 0.5, 2, n_scales=8, n_orient=7))


def test_batch_64_global_codebook_every_label(torch_cuda):
    """The timed configuration's shape with colour (global codebook, 64 x 481x321, w = 1/8, g = 4): every label."""
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(64, 321, 481, seed=0)
    keep = imgs.copy()
    got = Segmenter(n_orient=5, color_weight=0.125, chroma_gain=4).segment_batch(imgs, "global")
    x = np.stack([cr.features(im, 0.125, 4, 4, 5) for im in imgs]).reshape(64, 72, -1)
    want = co.kmeans(x, 8, 10)[0].reshape(64, 321, 481)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(imgs, keep)


@pytest.mark.parametrize("w,g", SETTINGS)
def test_every_call_path_agrees(torch_cuda, w, g):
    """segment == the row of segment_batch (graph path and the chunked fast path) == segment_stream == segment_images ==
    segment_device; graph replay == eager; features_device == the restatement."""
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, segment, segment_batch, segment_images
    kw = dict(n_orient=5, color_weight=w, chroma_gain=g)
    imgs = _synth(8, 481, 321, seed=21)                       # 8 x 481x321 > 2^20 pixels: segment_batch's chunked fast path,
    want = cr.segment_batch(imgs, w, g, n_orient=5)           # whose chunks of two 463 203-byte images are not 16-byte aligned
    seg = Segmenter(**kw)
    assert np.array_equal(seg.segment_batch(imgs), want)
    assert np.array_equal(segment_batch(imgs[:2], **kw), want[:2])                     # graph path
    assert np.array_equal(segment(imgs[3], **kw), want[3])
    dev = torch.from_numpy(imgs).cuda()
    assert np.array_equal(seg.segment_device(dev).cpu().numpy(), want)
    assert np.array_equal(dev.cpu().numpy(), imgs)                                     # the caller's tensor is not mutated
    outs = list(seg.segment_stream([imgs[:4], imgs[4:]]))
    assert np.array_equal(np.concatenate(outs), want)
    mixed = [imgs[0], np.ascontiguousarray(imgs[1].transpose(1, 0, 2)), imgs[2]]
    got = list(segment_images(mixed, batch=2, **kw))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], cr.segment(mixed[1], w, g, n_orient=5))
    big = list(seg.segment_images(list(imgs), batch=4))                                # full batches: the three-stream pipeline
    assert np.array_equal(np.stack(big), want)
    for i in range(8):
        assert np.array_equal(seg(imgs[i]), want[i])                                   # replayed graph
    eager = Segmenter(**kw)
    eager.debug.no_graph = True
    assert np.array_equal(eager.segment_batch(imgs[:1]), want[:1])
    f = seg.features_device(dev[:2]).cpu().numpy().view(np.uint16)
    for i in range(2):
        assert np.array_equal(f[i], cr.features(imgs[i], w, g, 4, 5))


def test_defaults_equal_the_explicit_zeros_and_differ_from_colour(torch_cuda):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, segment
    from oracle import spec_oracle as so
    imgs = _synth(2, 321, 481, seed=5)
    plain = Segmenter().segment_batch(imgs)
    zero = Segmenter(color_weight=0, chroma_gain=0)
    assert np.array_equal(zero.segment_batch(imgs), plain)
    assert np.array_equal(segment(imgs[0], color_weight=0.0, chroma_gain=0), plain[0])
    assert zero.ops.chroma_gain == 0 and not any("colour" in ws for ws in zero._ws.values())
    tapq, shift = so.bank()
    assert np.array_equal(plain, co.segment_batch(imgs, tapq, shift, 6))
    dev = torch.from_numpy(imgs).cuda()
    f0 = Segmenter().features_device(dev).cpu().numpy()
    assert np.array_equal(zero.features_device(dev).cpu().numpy(), f0)
    for kw in (dict(n_orient=5, color_weight=0.125), dict(chroma_gain=4), dict(n_orient=5, color_weight=0.125, chroma_gain=4)):
        assert not np.array_equal(Segmenter(**kw).segment_batch(imgs), plain), kw
    # the transform alone (no slot): the plain bank on T_g(img)
    got = Segmenter(chroma_gain=4).segment_batch(imgs)
    assert np.array_equal(got, cr.segment_batch(imgs, 0.0, 4))


def test_ops_built_for_another_gain_or_bank_are_refused(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    colour = Segmenter(n_orient=5, color_weight=0.125, chroma_gain=4)
    with pytest.raises(ValueError, match="same chroma_gain"):
        Segmenter(n_orient=5, color_weight=0.125, chroma_gain=2, ops=colour.ops)
    with pytest.raises(ValueError, match="same chroma_gain"):
        Segmenter(n_orient=5, color_weight=0.125, ops=colour.ops)
    with pytest.raises(ValueError, match="same colour bank"):
        Segmenter(chroma_gain=4, ops=colour.ops)
    with pytest.raises(ValueError, match="same colour bank"):
        Segmenter(n_orient=5, color_weight=0.25, chroma_gain=4, ops=colour.ops)
    Segmenter(n_orient=5, color_weight=0.125, chroma_gain=4, ops=colour.ops)


@pytest.mark.parametrize("w,g", SETTINGS)
def test_colour_with_smoothing(torch_cuda, w, g):
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(2, 321, 481, seed=31)
    got = Segmenter(n_orient=5, color_weight=w, chroma_gain=g, smoothing=1.0).segment_batch(imgs)
    assert np.array_equal(got, cr.segment_batch(imgs, w, g, n_orient=5, smoothing=1.0))


@pytest.mark.parametrize("w,g", SETTINGS)
def test_colour_with_min_region_size(torch_cuda, w, g):
    from gabor_color_image_segmentation_amd import Segmenter
    from merge_ref import merge_small_regions
    imgs = _synth(2, 321, 481, seed=32)
    got = Segmenter(n_orient=5, color_weight=w, chroma_gain=g, min_region_size=64).segment_batch(imgs)
    for i in range(2):
        assert np.array_equal(got[i], merge_small_regions(cr.segment(imgs[i], w, g, n_orient=5), 64)), i


# ---- two ranks, row-sharded

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
    seg = Segmenter(n_orient=5, color_weight=0.125, chroma_gain=4, n_iter=5, device="cuda:0")
    r0, r1, s0, s1 = seg.shard_rows(height, world, rank)
    if owned:
        out = seg.segment_owned_rows_device(torch.from_numpy(np.ascontiguousarray(imgs[:, r0:r1])).cuda(), height)
    else:
        out = seg.segment_rows_sharded_device(torch.from_numpy(np.ascontiguousarray(imgs[:, s0:s1])).cuda(), r0, r1, s0, height)
    np.save(os.path.join(tmp, f"strip_{rank}.npy"), out.cpu().numpy())
    dist.destroy_process_group()


@pytest.mark.parametrize("owned", [False, True])
def test_row_sharded_two_ranks(tmp_path, built, owned):
    """Two processes share cuda:0, gloo carries the tiny collectives: every strip (halo included) is transformed on its own."""
    import torch.multiprocessing as mp
    height, width = 202, 137
    port = 35500 + (os.getpid() % 2000) + int(owned)
    mp.spawn(_strip_worker, args=(2, port, height, width, str(tmp_path), owned), nprocs=2, join=True)
    got = np.concatenate([np.load(tmp_path / f"strip_{r}.npy") for r in range(2)], axis=1)
    want = cr.segment_batch(_synth(1, height, width, seed=13), 0.125, 4, n_iter=5, n_orient=5, mode="global")
    assert np.array_equal(got, want)


# ---- quality through the GPU

# means over the 24 val fixture images of boundary F, PRI, VoI, covering, from the restatement on the CPU
# (tools/colour_quality.py); n_orient = 5, k = 8, raw cluster labels
QUALITY_24 = {
    (0.125, 0): (0.3553491718478852, 0.7145419534972733, 3.4576024441916924, 0.3265615546522393),
    (0.125, 4): (0.38056635496882746, 0.7301444206785535, 3.2096736063412057, 0.3601042504352936),
}


@pytest.mark.parametrize("w,g", SETTINGS)
def test_quality_on_the_val_fixture_through_the_gpu(torch_cuda, w, g):
    """The 24 val images through the colour plan and the batched GPU scorer: the restatement's labels, and its means."""
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    ids = [str(i) for i in val["ids"]]
    seg = Segmenter(n_orient=5, color_weight=w, chroma_gain=g)
    rows = {}
    for shape in ((321, 481), (481, 321)):
        group = [i for i in ids if val["img_" + i].shape[:2] == shape]
        labs = seg.segment_batch(np.stack([val["img_" + i] for i in group]))
        scores = all_scores_batch_device(torch.from_numpy(labs).cuda(), pt.to_device(group), agreement=True)
        for i, lab, sc in zip(group, labs, scores):
            assert np.array_equal(lab, cr.segment(val["img_" + i], w, g, n_orient=5)), i
            rows[i] = [sc["fmeasure"], sc["PRI"], sc["VoI"], sc["covering"]]
    got = np.mean([rows[i] for i in ids], axis=0)
    assert np.all(np.abs(got - np.array(QUALITY_24[(w, g)])) <= 1e-12), got.tolist()
