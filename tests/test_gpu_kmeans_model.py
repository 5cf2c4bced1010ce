"""The k-means model (SPEC.md §28) on the GPU: gcs_kmeans_evaluate against its NumPy restatement (tests/kmeans_model_ref.py) on
the C oracle's features of the hot banks (tests/hot_banks.py: values above 4096, flagged tiles) - every output alone and all
together, both slab formats, packed edge strips, one to four levels, a bank of 216 planes, every k bucket, one codebook and one per
image, crafted centroids -; the kernel against the Lloyd passes on a BSD image; the table where many workgroups meet on the same
counters; fit / predict / warm start / confidence against the C oracle; the buffer, stream and graph contracts of the entry point
with the helpers of the contract tests (tests/arena.py, tests/stream_order.py); and one batch whose int64 map passes byte offsets
2^31 and 2^32 (the method of tests/test_gpu_large_maps.py)."""
import os

import numpy as np
import pytest

import hot_banks as hb
import kmeans_model_ref as km
import large_maps as lm

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

# id -> (n_scales, n_orient, ksize, shift)
BANKS = {"split_4x6": (4, 6, 13, 7),            # split slab, two levels
         "split_2x3": (2, 3, 9, 8),             # split slab, one level
         "wide_3x9": (3, 9, 15, 7),             # wide slab, two levels (D = 81), packed strips
         "deep_7x1": (7, 1, 13, 7),             # four levels, one filter on the last
         "deep_8x8": (8, 8, 15, 7),             # four levels, D = 192
         "generic_6x12": (6, 12, 13, 7)}        # D = 216: the Lloyd loop's generic pass, three levels
SHAPES = [(8, 8), (9, 9), (25, 10), (16, 33), (40, 50)]   # one block; one-pixel strips; ragged; two workgroups a row; several
KS = (1, 2, 3, 8, 16)
B = 3


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _crafted(x, k, n_sets, rng):
    """(n_sets, k, D) int64 centroids: pixel vectors of the set's own image (so a pixel sits ON a centroid), then, as k allows, a
    duplicate of centroid 0 (a tie: the lowest index wins, the margin is 0), an all-zero and an all-65535 centroid."""
    p = x.shape[1]
    cent = np.stack([x[s][rng.choice(p, k, replace=p < k)] for s in range(n_sets)]).astype(np.int64)
    if k >= 2:
        cent[:, 1] = cent[:, 0]
    if k >= 8:
        cent[:, 4] = 0
        cent[:, 6] = 65535
    return cent


def _to_dev(torch, cent):
    return torch.from_numpy(cent.astype(np.uint16).view(np.int16)).cuda()


def _run(torch, st, cent, names):
    """One evaluate call with exactly the outputs ``names`` -> {name: host array}; every given output starts as garbage."""
    n_sets, k = cent.shape[:2]
    shape = {"labels": ((st.b, st.h, st.w), torch.int32), "best": ((st.b, st.h, st.w), torch.int64),
             "second": ((st.b, st.h, st.w), torch.int64), "stats": ((n_sets, k, 2), torch.int64)}
    outs = {n: torch.full(shape[n][0], -77, dtype=shape[n][1], device="cuda") for n in names}
    st.ops.kmeans_evaluate(st.feats, _to_dev(torch, cent), st.b, st.h, st.w, k, n_sets, **outs)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in outs.items()}


def _hold(got, want, st, tag):
    lab, best, second, stats = want
    ref = dict(labels=lab.reshape(st.b, st.h, st.w), best=best.reshape(st.b, st.h, st.w),
               second=second.reshape(st.b, st.h, st.w), stats=stats)
    for name, g in got.items():
        bad = np.argwhere(g != ref[name])
        assert bad.size == 0, (tag, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], ref[name][tuple(bad[0])])


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("bank", list(BANKS))
def test_kernel_against_the_restatement(torch_cuda, bank, shape):
    from fused_stages import stage
    torch = torch_cuda
    h, w = shape
    st = stage(torch, BANKS[bank], hb.hot_images(B, h, w, seed=h * w))
    assert st.x.max() >= 4096
    rng = np.random.default_rng(h + w)
    alone = KS[(h + w + len(bank)) % len(KS)]                 # every k takes its turn at the runs with one output
    for k in KS:
        for n_sets in (1, B):
            cent = _crafted(st.x, k, n_sets, rng)
            want = km.evaluate_batch(st.x, cent)
            assert (want[1] == 0).any() and (k == 1 or (want[2] == want[1]).any())      # a pixel on a centroid; a tie
            tag = (bank, shape, k, n_sets)
            _hold(_run(torch, st, cent, ("labels", "best", "second", "stats")), want, st, tag)
            if k == alone:
                for name in ("labels", "best", "second", "stats"):
                    _hold(_run(torch, st, cent, (name,)), want, st, tag + ("alone",))


@gpu
def test_stats_where_many_workgroups_meet(torch_cuda):
    """B = 4 of 64 x 96, one codebook: 96 workgroups add into the same 2 k counters."""
    from fused_stages import stage
    torch = torch_cuda
    st = stage(torch, BANKS["split_4x6"], hb.hot_images(4, 64, 96, seed=64))
    for k in (8, 16):
        cent = _crafted(st.x, k, 1, np.random.default_rng(k))
        want = km.evaluate_batch(st.x, cent)
        assert (want[3][0, :, 0] > 0).sum() >= 3 and want[3][0, :, 0].sum() == 4 * 64 * 96
        _hold(_run(torch, st, cent, ("stats",)), want, st, ("meet", k))
        _hold(_run(torch, st, cent, ("labels", "best", "second", "stats")), want, st, ("meet", k, "all"))


@gpu
@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_evaluate_labels_are_the_lloyd_passes_labels_on_a_bsd_image(torch_cuda, mode):
    """Two kernels against each other: the label map of the plan's last pass and evaluate's under the centroids that pass used."""
    from gabor_color_image_segmentation_amd import Segmenter
    torch = torch_cuda
    z = np.load(os.path.join(GOLD, "bsd_inputs.npz"))
    imgs = torch.from_numpy(np.stack([z["img_100075"], z["img_100098"]])).cuda()
    seg = Segmenter(device="cuda:0")
    want = seg.segment_device(imgs, mode)
    res = seg.evaluate_device(imgs, mode=mode, best=True, second=True)
    assert torch.equal(res["labels"], want)
    stats = res["stats"].cpu().numpy()
    p = imgs.shape[1] * imgs.shape[2]
    assert stats.shape == ((2, 8, 2) if mode == "per_image" else (1, 8, 2))
    assert stats[:, :, 0].sum(axis=1).tolist() == ([p, p] if mode == "per_image" else [2 * p])
    lab = want.cpu().numpy().reshape(2, -1)
    counts = np.stack([np.bincount(l, minlength=8) for l in lab])
    assert np.array_equal(stats[:, :, 0], counts if mode == "per_image" else counts.sum(axis=0, keepdims=True))
    assert int(stats[:, :, 1].sum()) == int(res["best"].sum()) and bool((res["second"] >= res["best"]).all())


# ---- fit, predict, warm start, confidence: the device API against the C oracle and the restatement

K, N_ITER = 5, 4


@pytest.fixture(scope="module")
def small(torch_cuda):
    """Three small images, their C-oracle features (B, P, D) int64, and the model of the first two - fitted once, never changed."""
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    from oracle import c_oracle as co
    imgs = synthetic_batch(3, 41, 58, seed=7)
    seg = Segmenter(k=K, n_iter=N_ITER, device="cuda:0")
    feats = np.stack([co.gabor_features(im, seg.bank.tapq, seg.bank.shift, seg.bank.n_orient) for im in imgs])
    x = feats.reshape(3, feats.shape[1], -1).transpose(0, 2, 1).astype(np.int64)
    dev = torch_cuda.from_numpy(imgs).cuda()
    return dict(imgs=imgs, dev=dev, feats=feats.reshape(3, feats.shape[1], -1), x=x, seg=seg, model=seg.fit_device(dev[:2], "global"))


def _cent(model):
    return model.cpu().centroids.numpy().astype(np.int64)


@gpu
def test_fit_device_against_the_c_oracle(torch_cuda, small):
    from oracle import c_oracle as co
    seg, x, model = small["seg"], small["x"], small["model"]
    lab, cent = co.kmeans(small["feats"][:2], K, N_ITER)
    assert model.n_sets == 1 and np.array_equal(_cent(model)[0], cent.astype(np.int64))
    stats = km.evaluate_batch(x[:2], _cent(model))[3]
    assert np.array_equal(model.counts.cpu().numpy(), stats[:, :, 0]) and np.array_equal(model.inertia.cpu().numpy(), stats[:, :, 1])
    assert np.array_equal(np.bincount(lab.ravel(), minlength=K), stats[0, :, 0])
    assert np.array_equal(model.mse, km.mse(stats, x.shape[2])) and model.device.type == "cuda"
    per = seg.fit_device(small["dev"][:2], "per_image")
    for i in range(2):
        assert np.array_equal(_cent(per)[i], co.kmeans(small["feats"][i:i + 1], K, N_ITER)[1].astype(np.int64))
    assert np.array_equal(per.counts.cpu().numpy(), km.evaluate_batch(x[:2], _cent(per))[3][:, :, 0])


@gpu
def test_predict_refine_and_confidence_against_the_restatement(torch_cuda, small):
    from oracle import spec_oracle as so
    seg, x, model, dev = small["seg"], small["x"], small["model"], small["dev"]
    c = _cent(model)
    got = seg.predict_device(dev[2:], model).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got.reshape(-1), so.kmeans_assign(x[2], c[0]))
    for mode in ("per_image", "global"):
        got = seg.predict_device(dev, model, refine=2, mode=mode).cpu().numpy().reshape(3, -1)
        want, _ = km.schedule(x, c[0], 3, mode)
        assert np.array_equal(got, want), mode
    assert np.array_equal(_cent(model), c)                    # the warm start refined copies
    lab, best, second, stats = km.evaluate_batch(x, c)
    labels, conf = seg.confidence_device(dev, model)
    assert conf.dtype == torch_cuda.float32 and np.array_equal(labels.cpu().numpy().reshape(3, -1), lab)
    assert np.array_equal(conf.cpu().numpy().reshape(3, -1), km.confidence(best, second))
    res = seg.evaluate_device(dev, model, best=True, second=True)
    assert np.array_equal(res["stats"].cpu().numpy(), stats) and np.array_equal(res["best"].cpu().numpy().reshape(3, -1), best)


@gpu
@pytest.mark.parametrize("kw", [dict(), dict(tree_nodes="clusters", n_regions=6, min_region_size=20)], ids=["plain", "clusters"])
def test_a_model_of_the_init_pixels_is_the_plans_own_loop(torch_cuda, small, kw):
    """SPEC.md §28's warm start from c^0 = the init pixels of SPEC.md §4, refine = m, is the plan's loop at n_iter = m + 1: the
    codebook path (init kernel replaced, separate reduce launches) against the plan's own (self-updating passes), through every
    stage behind the Lloyd loop - the node map, the tree and its cut with tree_nodes = "clusters"."""
    from gabor_color_image_segmentation_amd import KMeansModel, Segmenter
    from oracle import spec_oracle as so
    torch = torch_cuda
    x, dev = small["x"], small["dev"]
    init = np.stack([so.kmeans_init(x[i], K) for i in range(3)]).astype(np.uint16)
    zeros = torch.zeros((3, K), dtype=torch.int64)
    for m in (0, 2):
        seg = Segmenter(k=K, n_iter=m + 1, device="cuda:0", **kw)
        model = KMeansModel(torch.from_numpy(init), zeros, zeros, seg.model_signature)
        assert torch.equal(seg.predict_device(dev, model, refine=m), seg.segment_device(dev)), (kw, m)
        one = KMeansModel(torch.from_numpy(init[:1]), zeros[:1], zeros[:1], seg.model_signature)
        assert torch.equal(seg.predict_device(dev, one, refine=m, mode="global"), seg.segment_device(dev, "global")), (kw, m)


@gpu
def test_host_calls_take_a_codebook(torch_cuda, small):
    import gabor_color_image_segmentation_amd as pkg
    seg, model, imgs = small["seg"], small["model"], small["imgs"]
    want = seg.predict_device(small["dev"], model, refine=1).cpu().numpy()
    kw = dict(k=K, n_iter=N_ITER)
    host = model.cpu()
    assert np.array_equal(pkg.segment(imgs[2], codebook=host, refine=1, **kw), want[2])
    assert np.array_equal(pkg.segment_batch(imgs, codebook=host, refine=1, **kw), want)
    assert np.array_equal(seg.segment_batch(imgs, codebook=model, refine=1, out_dtype=np.uint8), want.astype(np.uint8))
    assert np.array_equal(np.stack(list(seg.segment_images(list(imgs), batch=2, codebook=model, refine=1))), want)
    fit = pkg.fit_codebook(imgs[:2], **kw)
    assert fit.device.type == "cpu" and np.array_equal(_cent(fit), _cent(model))
    labels, conf = pkg.segment_confidence(imgs[2], codebook=fit, **kw)
    lab, best, second, _ = km.evaluate(small["x"][2], _cent(model)[0])
    assert np.array_equal(labels.reshape(-1), lab) and np.array_equal(conf.reshape(-1), km.confidence(best, second))


# ---- the entry point's contracts

def _contract_inputs(torch):
    """The slabs of two image sets (true, decoy) of one bank and shape, two codebooks, the true set's reference."""
    from fused_stages import stage
    cfg, (h, w), k = BANKS["split_4x6"], (25, 42), 8
    st_t = stage(torch, cfg, hb.hot_images(B, h, w, seed=3))
    st_d = stage(torch, cfg, np.ascontiguousarray(hb.hot_images(8, h, w, seed=5)[[4, 6, 7]]))
    cent_t = _crafted(st_t.x, k, B, np.random.default_rng(1))
    cent_d = _crafted(st_d.x, k, B, np.random.default_rng(2))
    raw = lambda c: c.astype(np.uint16)
    return st_t, st_d, raw(cent_t), raw(cent_d), km.evaluate_batch(st_t.x, cent_t), k


def _sizes(st, k, n_sets):
    p = st.b * st.h * st.w
    return dict(labels=4 * p, best=8 * p, second=8 * p, stats=16 * n_sets * k)


@gpu
def test_buffer_contract(torch_cuda):
    """Canary bands around every output, buffers of exactly the documented size holding either poison byte on entry (garbage in
    ``stats`` is harmless: the call zeroes it), inputs unchanged; a NULL output is never touched (the others' bands hold)."""
    from arena import POISONS, Arena
    from gabor_color_image_segmentation_amd import _lib
    torch = torch_cuda
    lib = _lib.load()
    st, _, cent, _, want, k = _contract_inputs(torch)
    ns, no = BANKS["split_4x6"][:2]
    for fill in POISONS:
        for names in (("labels", "best", "second", "stats"), ("stats",), ("second",), ("labels", "stats")):
            arena = Arena(torch, "cuda")
            slab = arena.put(st.feats.cpu().numpy(), name="slab")
            cdev = arena.put(cent, name="centroids")
            outs = {n: arena.take(_sizes(st, k, B)[n], fill=fill, name=n) for n in names}
            ptr = lambda n: outs[n].data_ptr() if n in outs else None
            rc = lib.gcs_kmeans_evaluate(slab.data_ptr(), cdev.data_ptr(), st.b, st.h, st.w, ns, no, k, B, ptr("labels"), ptr("best"),
                                         ptr("second"), ptr("stats"), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.gcs_last_error()
            torch.cuda.synchronize()
            arena.check()
            arena.unchanged()
            dt = dict(labels=np.int32, best=np.int64, second=np.int64, stats=np.int64)
            _hold({n: arena.read(outs[n], dt[n], (B, k, 2) if n == "stats" else (st.b, st.h, st.w)) for n in names}, want, st,
                  ("arena", fill, names))


@gpu
def test_late_inputs_no_host_wait_and_graph_replay(torch_cuda):
    """The stream contract (tests/stream_order.py): inputs that arrive late on another stream, a call that returns while the gate
    still runs; then the call captured in a graph and replayed twice on garbage in ``stats``: the same table both times."""
    import stream_order as so_
    from gabor_color_image_segmentation_amd import _lib
    torch = torch_cuda
    lib = _lib.load()
    st_t, st_d, cent_t, cent_d, want, k = _contract_inputs(torch)
    ns, no = BANKS["split_4x6"][:2]
    size = _sizes(st_t, k, B)
    bufs = dict(slab=so_.late(st_t.feats.cpu().numpy(), st_d.feats.cpu().numpy()), cent=so_.late(cent_t, cent_d),
                **{n: so_.out(size[n]) for n in size})

    def call(lib, p, stream):
        rc = lib.gcs_kmeans_evaluate(p["slab"], p["cent"], st_t.b, st_t.h, st_t.w, ns, no, k, B, p["labels"], p["best"], p["second"],
                                     p["stats"], stream)
        assert rc == 0, lib.gcs_last_error()

    def check(o):
        _hold(dict(labels=so_.view(o["labels"], np.int32, (B, st_t.h, st_t.w)), best=so_.view(o["best"], np.int64, (B, st_t.h, st_t.w)),
                   second=so_.view(o["second"], np.int64, (B, st_t.h, st_t.w)), stats=so_.view(o["stats"], np.int64, (B, k, 2))),
              want, st_t, "quiet run")
    case = so_.Case("kmeans_evaluate", ["gcs_kmeans_evaluate"], bufs, call, check)
    run = so_.Runner(torch, lib)
    case.quiet["decoy"], _ = run.quiet_run(case, "decoy")
    case.quiet["true"], case.enqueue_s = run.quiet_run(case, "true")
    check(case.quiet["true"])
    for name in case.outputs():
        assert not np.array_equal(case.quiet["true"][name], case.quiet["decoy"][name]), name
    run.calibrate()
    run.settle([case.enqueue_s])
    run.hold_late(case)
    # captured once, replayed twice: the zeroing of the table is part of the graph
    replayed = run.capture_run(case)                          # (one replay, on the decoys)
    for name in case.outputs():
        so_.same(replayed[name], case.quiet["decoy"][name], (name, "replay on the decoys"))
    work = run._entry(case, "true")
    p = run._ptrs(work)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        call(lib, p, torch.cuda.current_stream().cuda_stream)
    tables = []
    for garbage in (0x5A, 0xFF):
        work["stats"].fill_(garbage)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        tables.append(work["stats"].cpu().numpy().view(np.int64).reshape(B, k, 2))
    assert np.array_equal(tables[0], want[3]) and np.array_equal(tables[1], want[3])


# ---- one batch whose int64 map passes byte offsets 2^31 and 2^32

@gpu
def test_best_map_past_byte_offsets_two_to_the_31_and_32(torch_cuda):
    """The smallest bank (1 x 1: three planes) and ``best`` alone on N29 = 13 891 images of 161 x 241 (tests/large_maps.py): the
    int64 map is 4.3 GB and crosses byte 2^31 and byte 2^32, the slab 2^31. The sixteen base images are held to the restatement;
    the large run must equal them through the index sequence in every element - the images around both lines and the last pixel
    named on their own."""
    from fused_stages import stage
    torch = torch_cuda
    cfg = (1, 1, 15, 7)
    base = lm.base_images()
    st = stage(torch, cfg, base)
    k = 3
    cent = _crafted(st.x, k, 1, np.random.default_rng(29))
    want = km.evaluate_batch(st.x, cent)
    small = _run(torch, st, cent, ("best",))["best"]
    _hold(dict(best=small), want, st, "the sixteen base images")
    b = lm.N29
    idx = lm.batch(b)
    lines = dict(lm.lines_of(8, lm.P, b))
    assert sorted(lines) == ["byte 2^31", "byte 2^32"] and b * lm.P * 3 < 1 << 31           # (inside the entry point's bound)
    idx_dev = torch.from_numpy(idx).cuda()
    per_image = st.feats.numel() // lm.N_BASE
    assert per_image * lm.N_BASE == st.feats.numel() == st.ops.lib.gcs_feature_slab_bytes(lm.N_BASE, lm.H, lm.W, 1, 1)
    assert st.ops.lib.gcs_feature_slab_bytes(b, lm.H, lm.W, 1, 1) == b * per_image > 1 << 31
    slab = lm.replicate(torch, st.feats.view(lm.N_BASE, per_image), idx_dev)
    best = lm.filled(torch, (b, lm.H, lm.W), torch.int64, -77)
    st.ops.kmeans_evaluate(slab.view(-1), _to_dev(torch, cent), b, lm.H, lm.W, k, 1, best=best)
    torch.cuda.synchronize()
    small_dev = torch.from_numpy(small).cuda()
    for name, at in lines.items():
        i = at // lm.P
        for j in (i - 1, i, i + 1):
            assert torch.equal(best[j], small_dev[int(idx[j])]), (name, "image", j)
    assert int(best[b - 1, lm.H - 1, lm.W - 1]) == int(small[idx[b - 1], lm.H - 1, lm.W - 1])
    assert lm.first_difference(torch, best, small_dev, idx_dev) is None
