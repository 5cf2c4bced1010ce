"""The regulariser of SPEC.md §30 on the GPU, every comparison ``==``:

1. gcs_label_relax against its NumPy restatement (tests/label_relax_ref.py) on crafted volumes - the shapes where the launch
   geometry can go wrong (a workgroup of a sub-pass covers 8 rows x 128 columns of the image, one of the energy launch 4 x 64), every
   k bucket and its neighbours, both neighbourhoods, 0 / 1 / 2 / 5 sweeps, one image and three with their own beta (0, 2^58 - 1 and
   a small one), costs in 0..3 (ties and long chains of changes everywhere) and near 2^62, start maps with labels out of range,
   every buffer between canary bands (tests/arena.py), optional outputs NULL, and the call replayed from a captured graph;
2. gcs_kmeans_costs against the distances of tests/kmeans_model_ref.py: the C oracle's features of the hot banks (both slab formats,
   one to four levels, packed strips, ragged shapes) and crafted slabs over the full 16-bit range (tests/slab_codec.py through the
   contents of tests/test_gpu_crafted_slabs.py), one codebook and one per image, argmin and min == gcs_kmeans_evaluate's outputs;
3. the chain on two BSD fixture images at a reduced shape: segment_device(regularize=0.25) == the restatement on the C oracle's
   features - per-image and global codebooks, codebook= / refine=, connectivity and min_region_size behind it, the cluster tree,
   the host paths;
4. regularize = 0 == a plan built without the option;
5. gcs_kmeans_evaluate, all four outputs, == its restatement as before (it shares its device code with the costs launch)."""
import os

import numpy as np
import pytest

import hot_banks as hb
import kmeans_model_ref as km
import label_relax_ref as lr

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

PASS_TILE = (8, 128)                   # image rows x columns under one workgroup of a sub-pass (4 x 64 pixels of a class)
RELAX_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (33, 65), (70, 41),
                PASS_TILE, (PASS_TILE[0] + 1, PASS_TILE[1] + 1), (2 * PASS_TILE[0] - 1, 2 * PASS_TILE[1] - 1)]
RELAX_KS = (1, 2, 3, 8, 9, 16)
SWEEPS = (0, 1, 2, 5)
TOP = (1 << 62) - 1
BETAS = {1: [1], 3: [0, lr.BETA_MAX, 2]}


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def lib(torch_cuda):
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------- 1. gcs_label_relax

def _volume(rng, b, k, h, w, content):
    c = rng.integers(0, 4, size=(b, k, h, w), dtype=np.int64)
    return c if content == "small" else TOP - c


def _start(rng, b, k, h, w, stray):
    return rng.integers(-2 if stray else 0, k + (2 if stray else 0), size=(b, h, w)).astype(np.int32)


def _states(costs, start, beta, nb):
    """The restatement after 0, 1, .., max(SWEEPS) sweeps, one sweep at a time: [(labels, changed so far (B, s), energy (B, 2))]."""
    b = costs.shape[0]
    lab, seen, out = start, np.zeros((b, 0), np.int32), []
    for s in range(max(SWEEPS) + 1):
        out.append((lab, seen, np.array([lr.energy(c, m, nb) for c, m in zip(costs, lab)], np.int64)))
        lab, ch, _ = lr.relax_batch(costs, lab, beta, 1, nb)
        seen = np.concatenate([seen, ch], axis=1)
    return out


def _relax(torch, lib, arena, dev, b, h, w, k, nb, sweeps, fill, null=()):
    """One call with every output a fresh arena buffer of exactly the documented size -> (labels, changed or None, energy or None)."""
    n = b * h * w
    out = arena.take(4 * n, fill=fill, name="labels_out")
    work = None if "workspace" in null else arena.take(4 * n, fill=fill, name="workspace")
    changed = None if "changed" in null else arena.take(4 * b * sweeps, fill=fill, name="changed")
    energy = None if "energy" in null else arena.take(16 * b, fill=fill, name="energy")
    from arena import ptr
    rc = lib.gcs_label_relax(dev["costs"].data_ptr(), dev["beta"].data_ptr(), b, h, w, k, nb, sweeps, dev["start"].data_ptr(),
                             out.data_ptr(), ptr(work), ptr(changed), ptr(energy), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.synchronize()
    return (arena.read(out, np.int32, (b, h, w)), None if changed is None else arena.read(changed, np.int32, (b, sweeps)),
            None if energy is None else arena.read(energy, np.int64, (b, 2)))


@gpu
@pytest.mark.parametrize("shape", RELAX_SHAPES, ids=lambda s: "%dx%d" % s)
def test_relax_against_the_restatement(torch_cuda, lib, shape):
    from arena import POISONS, Arena
    torch = torch_cuda
    h, w = shape
    rng = np.random.default_rng([30, h, w])
    moved = chains = strays = 0
    for k in RELAX_KS:
        for nb in (4, 8):
            for b in (1, 3):
                case = (RELAX_KS.index(k) + nb // 4 + b) % 4
                content, stray = ("small", "large")[case & 1], case >= 2
                costs, start = _volume(rng, b, k, h, w, content), _start(rng, b, k, h, w, stray)
                beta = np.array(BETAS[b], np.int64)
                want = _states(costs, start, beta, nb)
                arena = Arena(torch, "cuda")
                dev = dict(costs=arena.put(costs, name="costs"), beta=arena.put(beta, name="beta"), start=arena.put(start, name="start"))
                for sweeps in SWEEPS:
                    # the optional outputs take turns at being NULL; the workspace may be NULL below two sweeps
                    null = {0: ("workspace", "changed"), 1: ("workspace", "energy"), 2: (), 5: ("changed",) if k == 3 else ()}[sweeps]
                    lab, changed, energy = _relax(torch, lib, arena, dev, b, h, w, k, nb, sweeps, POISONS[(k + sweeps) & 1], null)
                    tag = (shape, k, nb, b, content, stray, sweeps)
                    bad = np.argwhere(lab != want[sweeps][0])
                    assert bad.size == 0, (tag, len(bad), bad[:4].tolist())
                    if changed is not None:
                        assert np.array_equal(changed, want[sweeps][1]), (tag, changed.tolist(), want[sweeps][1].tolist())
                    if energy is not None:
                        assert np.array_equal(energy, want[sweeps][2]), (tag, energy.tolist(), want[sweeps][2].tolist())
                arena.check()
                arena.unchanged()
                ch = want[-1][1]
                moved += int(ch[:, 0].sum())
                chains += int((ch[:, 1:] > 0).sum())
                strays += int(stray and bool(((want[1][0] < 0) | (want[1][0] >= k)).any()))
    if h * w > 1:
        assert moved > 0, "no sweep changes a label: the cases prove nothing"
    if h * w >= 9 * 9:
        assert chains > 0 and strays > 0      # changes that later sweeps build on; "no label" pixels that outlive a sweep


@gpu
def test_relax_replayed_from_a_captured_graph(torch_cuda, lib):
    """Captured once, replayed three times on garbage in every output: the counters' zeroing is part of the graph, so ``changed`` and
    the energy are the same on every replay."""
    torch = torch_cuda
    b, k, h, w, nb, sweeps = 3, 5, 37, 150, 8, 3
    rng = np.random.default_rng(301)
    costs, start = _volume(rng, b, k, h, w, "small"), _start(rng, b, k, h, w, True)
    beta = np.array([1, 3, 0], np.int64)
    lab, ch, en = lr.relax_batch(costs, start, beta, sweeps, nb)
    assert ch[:, 0].min() > 0 and ch[0].min() > 0
    dev = {n: torch.from_numpy(a).cuda() for n, a in dict(costs=costs, start=start, beta=beta).items()}
    out = torch.empty((b, h, w), dtype=torch.int32, device="cuda")
    work = torch.empty((b, h, w), dtype=torch.int32, device="cuda")
    changed = torch.empty((b, sweeps), dtype=torch.int32, device="cuda")
    energy = torch.empty((b, 2), dtype=torch.int64, device="cuda")

    def call():
        rc = lib.gcs_label_relax(dev["costs"].data_ptr(), dev["beta"].data_ptr(), b, h, w, k, nb, sweeps, dev["start"].data_ptr(),
                                 out.data_ptr(), work.data_ptr(), changed.data_ptr(), energy.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.gcs_last_error()
    call()                                                    # eager once: the kernels are loaded outside the capture
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        call()
    for garbage in (0x5A, 0xFF, 0x00):
        for t in (out, changed, energy):
            t.view(torch.uint8).fill_(garbage)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(changed.cpu().numpy(), ch) and np.array_equal(energy.cpu().numpy(), en), garbage
        assert np.array_equal(out.cpu().numpy(), lab), garbage
    assert np.array_equal(dev["start"].cpu().numpy(), start)


@gpu
def test_relax_labels_device_on_any_volume(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    torch = torch_cuda
    rng = np.random.default_rng(302)
    costs, start = _volume(rng, 2, 7, 19, 140, "small") * 5, _start(rng, 2, 7, 19, 140, False)
    seg = Segmenter(device="cuda:0")
    for beta, sweeps, nb in ((3, 4, 8), (np.array([0, 9], np.int64), 2, 4), (1, 0, 8)):
        bt = np.broadcast_to(np.asarray(beta, np.int64), (2,))
        out, changed, energy = seg.relax_labels_device(torch.from_numpy(costs).cuda(), torch.from_numpy(start).cuda(),
                                                       beta if isinstance(beta, int) else torch.from_numpy(beta).cuda(), sweeps, nb)
        lab, ch, en = lr.relax_batch(costs, start, bt, sweeps, nb)
        assert np.array_equal(out.cpu().numpy(), lab) and np.array_equal(changed.cpu().numpy(), ch)
        assert np.array_equal(energy.cpu().numpy(), en)


# ---------------------------------------------------------------------------------------------------------- 2. gcs_kmeans_costs

# id -> (n_scales, n_orient, ksize, shift)
BANKS = {"split_4x6": (4, 6, 13, 7),            # split slab, two levels
         "split_2x3": (2, 3, 9, 8),             # split slab, one level
         "wide_3x9": (3, 9, 15, 7),             # wide slab, two levels (D = 81), packed strips
         "three_5x6": (5, 6, 13, 7),            # three levels
         "deep_7x1": (7, 1, 13, 7)}             # four levels, one filter on the last
COST_SHAPES = [(8, 8), (9, 9), (25, 10), (16, 33), (40, 50)]   # one block; one-pixel strips; ragged; two workgroups a row; several
B = 3


def _cent_dev(torch, cent):
    return torch.from_numpy(cent.astype(np.uint16).view(np.int16)).cuda()


def _costs_and_evaluate(torch, ops, slab, x, cent, h, w, tag):
    """One costs launch on a poisoned volume == the restatement's distances; its argmin and min == the evaluate launch's outputs."""
    n_sets, k = cent.shape[:2]
    cdev = _cent_dev(torch, cent)
    costs = torch.full((B, k, h, w), -77, dtype=torch.int64, device="cuda")
    ops.kmeans_costs(slab, cdev, B, h, w, k, n_sets, costs)
    got = costs.cpu().numpy()
    want = lr.cost_volume(x, cent, h, w)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, len(bad), bad[:4].tolist())
    labels = torch.full((B, h, w), -77, dtype=torch.int32, device="cuda")
    best = torch.full((B, h, w), -77, dtype=torch.int64, device="cuda")
    ops.kmeans_evaluate(slab, cdev, B, h, w, k, n_sets, labels=labels, best=best)
    assert np.array_equal(got.argmin(axis=1), labels.cpu().numpy()), tag
    assert np.array_equal(got.min(axis=1), best.cpu().numpy()), tag


@gpu
@pytest.mark.parametrize("bank", list(BANKS))
def test_costs_against_the_distances_on_the_hot_banks(torch_cuda, bank):
    from fused_stages import stage
    from test_gpu_kmeans_model import _crafted
    torch = torch_cuda
    for h, w in COST_SHAPES:
        st = stage(torch, BANKS[bank], hb.hot_images(B, h, w, seed=h * w))
        rng = np.random.default_rng(h + w)
        for k in (1, 2, 3, 8, 16):
            for n_sets in (1, B):
                _costs_and_evaluate(torch, st.ops, st.feats, st.x, _crafted(st.x, k, n_sets, rng), h, w, (bank, (h, w), k, n_sets))


@gpu
@pytest.mark.parametrize("bank", ["split_4x6", "wide_3x9", "deep_8x8"])
def test_costs_on_crafted_slabs_over_the_full_16_bit_range(torch_cuda, bank):
    import test_gpu_crafted_slabs as cs
    torch = torch_cuda
    cfg = cs.EVALUATE_BANKS[bank]
    ops = cs._ops(cfg)
    for h, w in ((1, 1), (9, 10), (17, 16), (33, 41)):
        for content in cs.CONTENTS:
            cr = cs.crafted((h, w), cfg[0], cfg[1], content)
            for filler in cs.FILLERS:
                slab = torch.from_numpy(np.ascontiguousarray(cr.raw[filler].reshape(-1))).cuda()
                for k, n_sets in ((1, 1), (3, B), (8, 1), (16, B)):
                    cent = cs.codebook(cr, k, n_sets, seed=h + w)
                    _costs_and_evaluate(torch, ops, slab, cr.x, cent, h, w, (bank, (h, w), content, filler, k, n_sets))
    top = lr.cost_volume(cr.x, np.zeros((1, 1, cr.d), np.int64), h, w)
    assert top.max() == cr.d * 65535 ** 2                      # (the ceiling content against an all-zero centroid: the largest cost)
    _costs_and_evaluate(torch, ops, slab, cr.x, np.zeros((1, 1, cr.d), np.int64), h, w, (bank, "largest cost"))


@gpu
def test_costs_buffer_contract(torch_cuda, lib):
    from arena import POISONS, Arena
    from fused_stages import stage
    from test_gpu_kmeans_model import _crafted
    torch = torch_cuda
    cfg, (h, w), k = BANKS["split_4x6"], (25, 42), 8
    st = stage(torch, cfg, hb.hot_images(B, h, w, seed=3))
    cent = _crafted(st.x, k, B, np.random.default_rng(1))
    for fill in POISONS:
        arena = Arena(torch, "cuda")
        slab, cdev = arena.put(st.feats.cpu().numpy(), name="slab"), arena.put(cent.astype(np.uint16), name="centroids")
        out = arena.take(8 * B * k * h * w, fill=fill, name="costs")
        rc = lib.gcs_kmeans_costs(slab.data_ptr(), cdev.data_ptr(), B, h, w, cfg[0], cfg[1], k, B, out.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.gcs_last_error()
        torch.cuda.synchronize()
        arena.check()
        arena.unchanged()
        assert np.array_equal(arena.read(out, np.int64, (B, k, h, w)), lr.cost_volume(st.x, cent, h, w))


# ---------------------------------------------------------------------------------------------------------- 3. the chain

K, N_ITER, LAM = 6, 5, 0.25


@pytest.fixture(scope="module")
def chain(torch_cuda):
    """Two BSD fixture images cut to 57 x 74, their C-oracle features, and the restatement's maps - made once, never changed."""
    from gabor_color_image_segmentation_amd import make_bank
    from oracle import c_oracle as co
    from oracle import spec_oracle as so
    z = np.load(os.path.join(GOLD, "bsd_inputs.npz"))
    imgs = np.ascontiguousarray(np.stack([z["img_100075"], z["img_100098"]])[:, 100:157, 60:134])
    bank = make_bank()
    canon = np.stack([co.gabor_features(im, bank.tapq, bank.shift, bank.n_orient) for im in imgs])
    b, (h, w) = 2, imgs.shape[1:3]
    canon = canon.reshape(b, -1, h, w).astype(np.int64)
    x = canon.reshape(b, canon.shape[1], -1).transpose(0, 2, 1).astype(np.int64)

    def want(mode, c0=None, n_iter=N_ITER, lam=LAM, sweeps=4, nb=8):
        if c0 is None:
            c0 = np.stack([so.kmeans_init(x[i], K) for i in range(b)]) if mode == "per_image" else so.kmeans_init(x[0], K)
        labels, cent = km.schedule(x, c0, n_iter, mode)
        beta = lr.beta_of(km.evaluate_batch(x, cent)[3], lr.q_of(lam))
        beta = beta if mode == "per_image" else np.repeat(beta, b)
        out, changed, _ = lr.relax_batch(lr.cost_volume(x, cent, h, w), labels.reshape(b, h, w), beta, sweeps, nb)
        assert changed[:, 0].min() > 0
        return out
    return dict(imgs=imgs, dev=torch_cuda.from_numpy(imgs).cuda(), canon=canon, x=x, want=want,
                maps={mode: want(mode) for mode in ("per_image", "global")})


def _seg(**kw):
    from gabor_color_image_segmentation_amd import Segmenter
    return Segmenter(k=K, n_iter=N_ITER, device="cuda:0", **kw)


@gpu
@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_regularised_step_is_the_restatement_on_the_oracles_features(torch_cuda, chain, mode):
    seg = _seg(regularize=LAM)
    got = seg.segment_device(chain["dev"], mode)
    assert got.dtype == torch_cuda.int32 and np.array_equal(got.cpu().numpy(), chain["maps"][mode])
    plain = _seg().segment_device(chain["dev"], mode).cpu().numpy()
    assert not np.array_equal(plain, chain["maps"][mode])
    if mode == "per_image":
        assert np.array_equal(seg.segment_device(chain["dev"], mode, group=1).cpu().numpy(), chain["maps"][mode])
    alt = _seg(regularize=1.0, regularize_sweeps=2, regularize_neighbours=4).segment_device(chain["dev"], mode).cpu().numpy()
    assert np.array_equal(alt, chain["want"](mode, lam=1.0, sweeps=2, nb=4))
    # behind a codebook: frozen, and refined twice
    model = _seg().fit_device(chain["dev"], mode)
    c0 = model.cpu().centroids.numpy().view(np.uint16).astype(np.int64)
    for m in (0, 2):
        got = seg.predict_device(chain["dev"], model, refine=m, mode=mode).cpu().numpy()
        assert np.array_equal(got, chain["want"](mode, c0=c0 if mode == "per_image" else c0[0], n_iter=m + 1)), m
    # the model's entry points ignore the option
    assert np.array_equal(seg.evaluate_device(chain["dev"], mode=mode)["labels"].cpu().numpy(), plain)
    assert torch_cuda.equal(seg.fit_device(chain["dev"], mode).centroids, model.centroids)
    costs, labels, stats = seg.kmeans_costs_device(chain["dev"], mode=mode)
    assert np.array_equal(labels.cpu().numpy(), plain) and np.array_equal(costs.cpu().numpy().argmin(axis=1), plain)
    assert np.array_equal(stats.cpu().numpy(), km.evaluate_batch(chain["x"], c0)[3])


@gpu
def test_every_later_stage_sees_the_relaxed_map(torch_cuda, chain):
    import cluster_tree_ref as cl
    import merge_ref as mr
    from oracle import spec_oracle as so
    dev, relaxed = chain["dev"], chain["maps"]["per_image"]
    got = _seg(regularize=LAM, connectivity=True).segment_device(dev).cpu().numpy()
    assert np.array_equal(got, np.stack([so.connected_regions(m) for m in relaxed]))
    got = _seg(regularize=LAM, min_region_size=12).segment_device(dev).cpu().numpy()
    assert np.array_equal(got, np.stack([mr.merge_small_regions(m, 12) for m in relaxed]))
    for m in (0, 12):
        seg = _seg(regularize=LAM, tree_nodes="clusters", n_regions=8, min_region_size=m)
        want = np.stack([cl.regions(x, lab, 8, m) for x, lab in zip(chain["canon"], relaxed)])
        assert np.array_equal(seg.segment_device(dev).cpu().numpy(), want), m
        assert np.array_equal(seg.segment_batch(chain["imgs"], out_dtype=np.uint8), want.astype(np.uint8))
    nodes = _seg(regularize=LAM, tree_nodes="clusters").segment_device(dev).cpu().numpy()
    raw = _seg(tree_nodes="clusters").segment_device(dev).cpu().numpy()
    assert np.array_equal(nodes, np.stack([cl.regions(x, lab, 0) for x, lab in zip(chain["canon"], relaxed)]))
    assert (nodes.reshape(2, -1).max(axis=1) < raw.reshape(2, -1).max(axis=1)).all()       # fewer nodes: what the option is for


@gpu
def test_host_paths_take_the_plain_path(torch_cuda, chain):
    import gabor_color_image_segmentation_amd as pkg
    imgs, want = chain["imgs"], chain["maps"]["per_image"]
    kw = dict(k=K, n_iter=N_ITER, regularize=LAM)
    seg = _seg(regularize=LAM)
    assert seg._host_path(2, *imgs.shape[1:3], "per_image") == "plain" and not seg._may_pipeline("per_image")
    assert np.array_equal(pkg.segment(imgs[1], **kw), want[1])
    assert np.array_equal(pkg.segment_batch(imgs, **kw), want)
    assert np.array_equal(pkg.segment_batch(imgs, mode="global", **kw), chain["maps"]["global"])
    assert np.array_equal(np.stack(list(pkg.segment_images(list(imgs), **kw))), want)
    assert np.array_equal(seg(imgs[0]), want[0])
    assert np.array_equal(seg.segment_batch(imgs, out_dtype=np.uint8), want.astype(np.uint8))
    assert np.array_equal(np.concatenate(list(seg.segment_stream([imgs[:1], imgs[1:]]))), want)
    for refuse in (seg.texton_edges_device, seg.cue_edges_device):
        with pytest.raises(ValueError, match="plain k-means map"):
            refuse(chain["dev"])


# ---------------------------------------------------------------------------------------------------------- 4. the option off

@gpu
def test_regularize_zero_is_a_plan_without_the_option(torch_cuda, chain):
    torch = torch_cuda
    for kw in (dict(), dict(tree_nodes="clusters", n_regions=8), dict(connectivity=True)):
        off, plain = _seg(regularize=0.0, regularize_sweeps=9, regularize_neighbours=4, **kw), _seg(**kw)
        assert off._opt == plain._opt and off._opt.relax is None
        for mode in ("per_image", "global"):
            assert torch.equal(off.segment_device(chain["dev"], mode), plain.segment_device(chain["dev"], mode)), (kw, mode)
        assert np.array_equal(off.segment_batch(chain["imgs"]), plain.segment_batch(chain["imgs"]))
        assert off._host_path(2, 57, 74, "per_image") == plain._host_path(2, 57, 74, "per_image")
        assert all("rx" not in ws for ws in off._ws.values())


# ---------------------------------------------------------------------------------------------------------- 5. the shared code

@gpu
@pytest.mark.parametrize("bank", list(BANKS))
def test_evaluate_still_equals_its_restatement(torch_cuda, bank):
    from fused_stages import stage
    from test_gpu_kmeans_model import _crafted, _hold, _run
    torch = torch_cuda
    for h, w in COST_SHAPES:
        st = stage(torch, BANKS[bank], hb.hot_images(B, h, w, seed=h * w))
        rng = np.random.default_rng(h * w + 5)
        for k in (1, 2, 3, 8, 16):
            for n_sets in (1, B):
                cent = _crafted(st.x, k, n_sets, rng)
                _hold(_run(torch, st, cent, ("labels", "best", "second", "stats")), km.evaluate_batch(st.x, cent), st,
                      (bank, (h, w), k, n_sets))
