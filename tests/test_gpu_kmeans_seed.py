"""k-means++ seeding (SPEC.md §29) on the GPU: gcs_kmeans_seed against its restatement (tests/kmeans_seed_ref.py) on the C oracle's
features of the hot banks (tests/hot_banks.py: values above 4096, flagged tiles) - centroids, picks and potential, each optional
output present and absent, both slab formats, packed edge strips, one to four levels, a bank of 216 planes, every k and trial
bucket, the rule's stride and strides 1 and 2, one set and one per image -; sets of exactly 4096 candidates; slabs the tests wrote
(tests/slab_codec.py): a constant image, values up to 65535 whose potentials pass 2^32, trials that draw the same candidate, clamped
last rows and columns; the buffer, stream and graph contracts of the entry point (tests/arena.py, tests/stream_order.py); and the
plan's ``init="kmeans++"`` end to end against C-oracle features -> the restatement's seeds -> SPEC.md §4's schedule."""
import numpy as np
import pytest

import hot_banks as hb
import kmeans_model_ref as km
import kmeans_seed_ref as ks
import slab_codec as sc

gpu = pytest.mark.gpu

# id -> (n_scales, n_orient, ksize, shift): the banks of tests/test_gpu_kmeans_model.py
BANKS = {"split_4x6": (4, 6, 13, 7),            # split slab, two levels
         "split_2x3": (2, 3, 9, 8),             # split slab, one level
         "wide_3x9": (3, 9, 15, 7),             # wide slab, two levels (D = 81), packed strips
         "deep_7x1": (7, 1, 13, 7),             # four levels, one filter on the last
         "deep_8x8": (8, 8, 15, 7),             # four levels, D = 192
         "generic_6x12": (6, 12, 13, 7)}        # D = 216, three levels
SHAPES = [(8, 8), (9, 9), (25, 10), (16, 33), (40, 50)]   # one block; one-pixel strips; ragged; two blocks a row; 2000 candidates
KS = (1, 2, 3, 8, 16)
TRIALS = (1, 4, 8)
SEEDS = (0, 1, (1 << 63) + 5)
STRIDES = (8, 1, 2)                                       # the rule's for every shape here, then every pixel, every second
B = 3


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _run(torch, ops, feats, b, h, w, k, n_sets, stride, trials, seed, names=("picks", "potential")):
    """One seed call with the optional outputs ``names`` -> {name: host array}; every given output starts as garbage."""
    d = ops.bank.n_features
    outs = dict(cent=torch.full((n_sets, k, d), -77, dtype=torch.int16, device="cuda"))
    if "picks" in names:
        outs["picks"] = torch.full((n_sets, k), -77, dtype=torch.int32, device="cuda")
    if "potential" in names:
        outs["potential"] = torch.full((n_sets,), -77, dtype=torch.int64, device="cuda")
    ops.kmeans_seed(feats, b, h, w, k, n_sets, outs["cent"], stride, trials, seed,
                    picks=outs.get("picks"), potential=outs.get("potential"))
    torch.cuda.synchronize()
    got = {n: t.cpu().numpy() for n, t in outs.items()}
    got["cent"] = got["cent"].view(np.uint16).astype(np.int64)
    return got


def _hold(got, want, tag):
    ref = dict(cent=want[0], picks=want[1], potential=want[2])
    for name, g in got.items():
        bad = np.argwhere(g != ref[name])
        assert g.shape == ref[name].shape and bad.size == 0, (tag, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])],
                                                              ref[name][tuple(bad[0])])


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("bank", list(BANKS))
def test_kernel_against_the_restatement(torch_cuda, bank, shape):
    from fused_stages import stage
    torch = torch_cuda
    h, w = shape
    st = stage(torch, BANKS[bank], hb.hot_images(B, h, w, seed=h * w))
    assert st.x.max() >= 4096
    turn = h + w + len(bank)                                  # trials and seeds take turns; every (k, sets, stride) runs
    alone = KS[turn % len(KS)]
    for k in KS:
        for n_sets in (1, B):
            for stride in STRIDES:
                if (B if n_sets == 1 else 1) * len(ks.candidates(h, w, stride)) > ks.N_MAX:
                    continue                                  # (40 x 50 at stride 1 over three images: refused, see below)
                turn += 1
                trials, seed = TRIALS[turn % 3], SEEDS[(turn // 3) % 3]
                want = ks.seed_batch(st.x, h, w, k, n_sets, stride, seed, trials)
                tag = (bank, shape, k, n_sets, stride, trials, seed)
                _hold(_run(torch, st.ops, st.feats, B, h, w, k, n_sets, stride, trials, seed), want, tag)
                if k == alone:
                    for names in ((), ("picks",), ("potential",)):
                        _hold(_run(torch, st.ops, st.feats, B, h, w, k, n_sets, stride, trials, seed, names), want, tag + (names,))


@gpu
def test_every_trial_bucket_and_seed_on_one_slab(torch_cuda):
    """The full product the turns above thin out, on one bank and shape: trials 1 .. 8, the three seeds, k = 8 and 16."""
    from fused_stages import stage
    torch = torch_cuda
    h, w = 25, 10
    st = stage(torch, BANKS["split_4x6"], hb.hot_images(B, h, w, seed=h * w))
    for trials in range(1, 9):
        for seed in SEEDS:
            for k, n_sets in ((8, B), (16, 1)):
                want = ks.seed_batch(st.x, h, w, k, n_sets, 1, seed, trials)
                _hold(_run(torch, st.ops, st.feats, B, h, w, k, n_sets, 1, trials, seed), want, (trials, seed, k, n_sets))


@gpu
def test_sets_of_exactly_4096_candidates_and_one_more_row(torch_cuda):
    from fused_stages import stage
    from gabor_color_image_segmentation_amd import _lib
    torch = torch_cuda
    st = stage(torch, BANKS["split_4x6"], hb.hot_images(2, 64, 64, seed=64))
    assert len(ks.candidates(64, 64, 1)) == 4096
    for k, trials, seed in ((8, 4, 0), (16, 8, 1)):
        want = ks.seed_batch(st.x, 64, 64, k, 2, 1, seed, trials)            # two sets of 4096: every thread holds four candidates
        assert want[1].max() >= 3 * 1024                                      # a pick among a thread's last candidates
        _hold(_run(torch, st.ops, st.feats, 2, 64, 64, k, 2, 1, trials, seed), want, ("4096", k))
    want = ks.seed_batch(st.x, 64, 64, 8, 1, 2, 2, 4)                        # one set of 2 x 1024 over both images
    assert (want[1] >= 1024).any() and (want[1] < 1024).any()
    _hold(_run(torch, st.ops, st.feats, 2, 64, 64, 8, 1, 2, 4, 2), want, "two images, one set")
    tall = stage(torch, BANKS["split_4x6"], hb.hot_images(1, 65, 64, seed=65))
    cent = torch.full((1, 8, 72), -77, dtype=torch.int16, device="cuda")
    for st_, n_sets in ((tall, 1), (st, 1)):                                 # 65 x 64 = 4160; two images of 4096 in one set
        with pytest.raises(_lib.GcsError, match="more than 4096 candidates"):
            st_.ops.kmeans_seed(st_.feats, st_.b, st_.h, st_.w, 8, n_sets, cent, 1)
    torch.cuda.synchronize()
    assert bool((cent == -77).all())                                          # refused with nothing launched
    want = ks.seed_batch(tall.x, 65, 64, 8, 1, 2, 0, 4)
    _hold(_run(torch, tall.ops, tall.feats, 1, 65, 64, 8, 1, 2, 4, 0), want, "65 x 64 at stride 2")


# ---- slabs the tests wrote

CRAFT_BANKS = {"split_4x6": (4, 6, 13, 7), "wide_3x9": (3, 9, 15, 7), "deep_8x8": (8, 8, 15, 7)}
_OPS = {}


def _ops(cfg):
    if cfg not in _OPS:
        from gabor_color_image_segmentation_amd.segmenter import HipOps
        _OPS[cfg] = HipOps(hb.hot_bank(*cfg), "cuda:0")
    return _OPS[cfg]


def _written(torch, cfg, h, w, make, filler=0xFF):
    """A slab of B images written by the codec from ``make(shape of a level) -> uint16 array`` -> (device bytes, x (B, P, D))."""
    geo = sc.geometry(h, w, cfg[0], cfg[1])
    levels = [make((B, len(geo.planes[lev]), geo.hl[lev], geo.wl[lev])).astype(np.uint16) for lev in range(geo.n_levels)]
    x = geo.canonical(levels).reshape(B, geo.d, -1).transpose(0, 2, 1).astype(np.int64)
    return torch.from_numpy(np.ascontiguousarray(geo.pack(levels, filler=filler).reshape(-1))).cuda(), x


@gpu
@pytest.mark.parametrize("bank", list(CRAFT_BANKS))
def test_constant_images_take_the_uniform_branch(torch_cuda, bank):
    torch = torch_cuda
    cfg = CRAFT_BANKS[bank]
    for (h, w), value in (((13, 21), 0xFFFF), ((9, 10), 0), ((33, 41), 0x1234)):
        slab, x = _written(torch, cfg, h, w, lambda s: np.full(s, value))
        for n_sets, stride in ((B, 1), (1, 2), (B, 8)):
            want = ks.seed_batch(x, h, w, 6, n_sets, stride, 3, 4)
            n = len(ks.candidates(h, w, stride)) * (B if n_sets == 1 else 1)
            assert not want[2].any() and (want[0] == value).all()
            assert want[1][0].tolist() == [ks.pick(ks.u(3, r, 0), n) for r in range(6)]       # duplicates among them when n is small
            _hold(_run(torch, _ops(cfg), slab, B, h, w, 6, n_sets, stride, 4, 3), want, (bank, h, w, n_sets, stride))


@gpu
@pytest.mark.parametrize("bank", list(CRAFT_BANKS))
def test_distant_values_whose_potentials_pass_two_to_the_32(torch_cuda, bank):
    """Every feature 0, 1, 65534 or 65535: a distance is up to D * 65535^2 > 2^38, T passes 2^32 in every round with mass, so
    pick(u, T) needs the high word of the 128-bit product; and any value up to 65535 on the same shapes."""
    torch = torch_cuda
    cfg = CRAFT_BANKS[bank]
    rng = np.random.default_rng(len(bank))
    ends = np.array([0, 1, 65534, 65535])
    for h, w in ((16, 17), (13, 21)):
        for make in (lambda s: ends[rng.integers(0, 4, s)], lambda s: rng.integers(0, 65536, s)):
            slab, x = _written(torch, cfg, h, w, make)
            for n_sets, stride, k, trials in ((B, 1, 8, 4), (1, 1, 16, 8), (B, 2, 3, 1)):
                for seed in SEEDS[:2]:
                    cand = x[:, ks.candidates(h, w, stride)]
                    rounds = ks.seed_trace(cand[0] if n_sets == B else cand.reshape(-1, x.shape[2]), k, seed, trials)[3]
                    assert all(total > 1 << 32 for total, _ in rounds[1:])
                    assert any(ks.pick(ks.u(seed, r, 0), total & 0xFFFFFFFF) != ks.pick(ks.u(seed, r, 0), total)
                               for r, (total, _) in enumerate(rounds) if r)        # the low word of T alone would draw elsewhere
                    want = ks.seed_batch(x, h, w, k, n_sets, stride, seed, trials)
                    _hold(_run(torch, _ops(cfg), slab, B, h, w, k, n_sets, stride, trials, seed), want,
                          (bank, h, w, n_sets, stride, k, seed))


@gpu
def test_trials_that_draw_the_same_candidate(torch_cuda):
    """All the mass on two pixels: the trials of a round draw the same candidate again and again, the potentials tie, trial 0 wins."""
    torch = torch_cuda
    cfg = CRAFT_BANKS["split_4x6"]
    h, w = 16, 17

    def make(s):
        a = np.full(s, 7)
        if s[2:] == (h, w):
            a[:, :, 5, 11] = 65535
            a[:, :, 12, 3] = 40000
        return a
    slab, x = _written(torch, cfg, h, w, make)
    for seed in range(4):
        rounds = ks.seed_trace(x[0], 4, seed, 8)[3]
        assert len({q for _, q, _ in rounds[1][1]}) < 8                       # fewer distinct draws than trials
        _hold(_run(torch, _ops(cfg), slab, B, h, w, 4, B, 1, 8, seed), ks.seed_batch(x, h, w, 4, B, 1, seed, 8), seed)


@gpu
@pytest.mark.parametrize("bank", list(CRAFT_BANKS))
def test_clamped_last_row_and_column_candidates(torch_cuda, bank):
    """Shapes whose last grid row and column are clamped into the image (SPEC.md §29: min(s i + s / 2, H - 1)), strips included:
    every pixel holds its own values, so a candidate read one pixel off gives other seeds."""
    torch = torch_cuda
    cfg = CRAFT_BANKS[bank]
    rng = np.random.default_rng(5)
    for h, w, stride in ((9, 10, 8), (17, 16, 8), (13, 21, 8), (33, 41, 16), (5, 9, 4), (1, 1, 8), (33, 41, 64)):
        ys, xs = ks.grid(h, w, stride)
        assert ys[-1] == h - 1 or xs[-1] == w - 1
        slab, x = _written(torch, cfg, h, w, lambda s: rng.integers(0, 65536, s))
        for n_sets in (1, B):
            k = 5
            want = ks.seed_batch(x, h, w, k, n_sets, stride, 1, 4)
            _hold(_run(torch, _ops(cfg), slab, B, h, w, k, n_sets, stride, 4, 1), want, (bank, h, w, stride, n_sets))


# ---- the entry point's contracts

def _contract_inputs(torch):
    """The slabs of two image sets (true, decoy) of one bank and shape, and the true set's reference."""
    from fused_stages import stage
    cfg, (h, w), k = BANKS["split_4x6"], (25, 42), 8
    st_t = stage(torch, cfg, hb.hot_images(B, h, w, seed=3))
    st_d = stage(torch, cfg, np.ascontiguousarray(hb.hot_images(8, h, w, seed=5)[[4, 6, 7]]))
    return st_t, st_d, ks.seed_batch(st_t.x, h, w, k, B, 2, 1, 4), k


def _sizes(st, k, n_sets):
    return dict(cent=2 * n_sets * k * st.d, picks=4 * n_sets * k, potential=8 * n_sets)


_DT = dict(cent=np.uint16, picks=np.int32, potential=np.int64)


def _shaped(st, k, n_sets):
    return dict(cent=(n_sets, k, st.d), picks=(n_sets, k), potential=(n_sets,))


@gpu
def test_buffer_contract(torch_cuda):
    """Canary bands around every output, buffers of exactly the documented size holding either poison byte on entry, the slab
    unchanged; a NULL output is never touched (the others' bands hold)."""
    from arena import POISONS, Arena
    from gabor_color_image_segmentation_amd import _lib
    torch = torch_cuda
    lib = _lib.load()
    st, _, want, k = _contract_inputs(torch)
    ns, no = BANKS["split_4x6"][:2]
    for fill in POISONS:
        for names in (("cent", "picks", "potential"), ("cent",), ("cent", "potential"), ("cent", "picks")):
            arena = Arena(torch, "cuda")
            slab = arena.put(st.feats.cpu().numpy(), name="slab")
            outs = {n: arena.take(_sizes(st, k, B)[n], fill=fill, name=n) for n in names}
            ptr = lambda n: outs[n].data_ptr() if n in outs else None
            rc = lib.gcs_kmeans_seed(slab.data_ptr(), st.b, st.h, st.w, ns, no, k, B, 2, 4, 1, ptr("cent"), ptr("picks"),
                                     ptr("potential"), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.gcs_last_error()
            torch.cuda.synchronize()
            arena.check()
            arena.unchanged()
            got = {n: arena.read(outs[n], _DT[n], _shaped(st, k, B)[n]).astype(np.int64 if n == "cent" else _DT[n]) for n in names}
            _hold(got, want, ("arena", fill, names))


@gpu
def test_late_inputs_no_host_wait_and_graph_replay(torch_cuda):
    """The stream contract (tests/stream_order.py): a slab that arrives late on another stream, a call that returns while the gate
    still runs; then the call captured in a graph and replayed twice on garbage in the outputs: the same bits both times."""
    import stream_order as so_
    from gabor_color_image_segmentation_amd import _lib
    torch = torch_cuda
    lib = _lib.load()
    st_t, st_d, want, k = _contract_inputs(torch)
    ns, no = BANKS["split_4x6"][:2]
    size = _sizes(st_t, k, B)
    bufs = dict(slab=so_.late(st_t.feats.cpu().numpy(), st_d.feats.cpu().numpy()), **{n: so_.out(size[n]) for n in size})

    def call(lib, p, stream):
        rc = lib.gcs_kmeans_seed(p["slab"], st_t.b, st_t.h, st_t.w, ns, no, k, B, 2, 4, 1, p["cent"], p["picks"], p["potential"], stream)
        assert rc == 0, lib.gcs_last_error()

    def views(o):
        return {n: so_.view(o[n], _DT[n], _shaped(st_t, k, B)[n]).astype(np.int64 if n == "cent" else _DT[n]) for n in size}

    def check(o):
        _hold(views(o), want, "quiet run")
    case = so_.Case("kmeans_seed", ["gcs_kmeans_seed"], bufs, call, check)
    run = so_.Runner(torch, lib)
    case.quiet["decoy"], _ = run.quiet_run(case, "decoy")
    case.quiet["true"], case.enqueue_s = run.quiet_run(case, "true")
    check(case.quiet["true"])
    for name in case.outputs():
        assert not np.array_equal(case.quiet["true"][name], case.quiet["decoy"][name]), name
    run.calibrate()
    run.settle([case.enqueue_s])
    run.hold_late(case)
    replayed = run.capture_run(case)                          # (captured on the true slab, one replay on the decoy)
    for name in case.outputs():
        so_.same(replayed[name], case.quiet["decoy"][name], (name, "replay on the decoys"))
    work = run._entry(case, "true")
    p = run._ptrs(work)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        call(lib, p, torch.cuda.current_stream().cuda_stream)
    for garbage in (0x5A, 0xFF):
        for name in size:
            work[name].fill_(garbage)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _hold(views({n: work[n].cpu().numpy() for n in size}), want, ("replay", garbage))


# ---- the plan's init="kmeans++" against C-oracle features -> the restatement's seeds -> SPEC.md §4's schedule

K, N_ITER = 5, 4


@pytest.fixture(scope="module")
def small(torch_cuda):
    """Three small images and their C-oracle features (B, P, D) int64, computed once and never changed."""
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    from oracle import c_oracle as co
    imgs = synthetic_batch(3, 40, 50, seed=7)
    seg = Segmenter(k=K, n_iter=N_ITER, device="cuda:0", init="kmeans++", seed=2)
    feats = np.stack([co.gabor_features(im, seg.bank.tapq, seg.bank.shift, seg.bank.n_orient) for im in imgs])
    x = feats.reshape(3, feats.shape[1], -1).transpose(0, 2, 1).astype(np.int64)
    return dict(imgs=imgs, dev=torch_cuda.from_numpy(imgs).cuda(), feats=feats.reshape(3, feats.shape[1], -1), x=x, seg=seg)


def _want(x, mode, seed, n_iter=N_ITER, trials=4):
    b = x.shape[0]
    n_sets = b if mode == "per_image" else 1
    c0 = ks.seed_batch(x, 40, 50, K, n_sets, ks.seed_stride(1 if mode == "per_image" else b, 40, 50), seed, trials)[0]
    return km.schedule(x, c0 if mode == "per_image" else c0[0], n_iter, mode)


def _cent(model):
    return model.cpu().centroids.numpy().astype(np.int64)


@gpu
@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_seeded_plan_against_the_restatement(torch_cuda, small, mode):
    seg, x, dev, imgs = small["seg"], small["x"], small["dev"], small["imgs"]
    want, cents = _want(x, mode, 2)
    got = seg.segment_device(dev, mode).cpu().numpy().reshape(3, -1)
    assert np.array_equal(got, want)
    assert np.array_equal(seg.segment_batch(imgs, mode).reshape(3, -1), want)           # the captured small call
    assert np.array_equal(seg.segment_batch(imgs, mode).reshape(3, -1), want)           # ... and its replay
    streamed = np.concatenate(list(seg.segment_stream([imgs[i:i + 1] for i in range(3)], mode))).reshape(3, -1)
    assert np.array_equal(streamed, np.concatenate([_want(x[i:i + 1], mode, 2)[0] for i in range(3)]))     # (a batch is a set)
    assert np.array_equal(_cent(seg.fit_device(dev, mode)), cents)
    seeds = seg.seed_device(dev, mode)
    n_sets = 3 if mode == "per_image" else 1
    c0 = ks.seed_batch(x, 40, 50, K, n_sets, 8, 2, 4)[0]
    assert np.array_equal(_cent(seeds), c0)
    stats = km.evaluate_batch(x, c0)[3]
    assert np.array_equal(seeds.counts.cpu().numpy(), stats[:, :, 0]) and np.array_equal(seeds.inertia.cpu().numpy(), stats[:, :, 1])


@gpu
def test_single_image_is_its_batch_row(torch_cuda, small):
    seg, imgs, dev = small["seg"], small["imgs"], small["dev"]
    whole = seg.segment_device(dev).cpu().numpy()
    for i in range(3):
        assert np.array_equal(seg(imgs[i]), whole[i])
    assert np.array_equal(seg.segment_device(dev, group=2).cpu().numpy(), whole)


@gpu
@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_restarts_against_the_restatements_choice(torch_cuda, small, mode):
    seg, x, dev = small["seg"], small["x"], small["dev"]
    model = seg.fit_device(dev, mode, n_init=3)
    runs = [_want(x, mode, 2 + i)[1] for i in range(3)]
    tables = [km.evaluate_batch(x, c)[3] for c in runs]
    keep = ks.best_restart([t[:, :, 1].sum(axis=1) for t in tables])
    for s, i in enumerate(keep):
        assert np.array_equal(_cent(model)[s], runs[i][s]), (mode, s, i)
        assert np.array_equal(model.inertia.cpu().numpy()[s], tables[i][s, :, 1])
        assert np.array_equal(model.counts.cpu().numpy()[s], tables[i][s, :, 0])
    labels = seg.predict_device(dev, model, mode=mode).cpu().numpy().reshape(3, -1)
    assert np.array_equal(labels, km.evaluate_batch(x, _cent(model))[0])                # that loop's labels


@gpu
def test_default_plan_is_unchanged_and_clusters_take_the_seeds(torch_cuda, small):
    from gabor_color_image_segmentation_amd import Segmenter
    from oracle import c_oracle as co
    torch = torch_cuda
    dev, feats = small["dev"], small["feats"]
    for plan in (Segmenter(k=K, n_iter=N_ITER, device="cuda:0"), Segmenter(k=K, n_iter=N_ITER, device="cuda:0", init="spec", seed=9)):
        got = plan.segment_device(dev).cpu().numpy().reshape(3, -1)
        for i in range(3):
            assert np.array_equal(got[i], co.kmeans(feats[i:i + 1], K, N_ITER)[0][0])
    # tree_nodes = "clusters": the node map of the seeded k-means map
    kw = dict(k=K, n_iter=N_ITER, device="cuda:0", tree_nodes="clusters", min_region_size=20)
    seeded = Segmenter(init="kmeans++", seed=2, **kw)
    model = Segmenter(k=K, n_iter=N_ITER, device="cuda:0", init="kmeans++", seed=2).seed_device(dev)
    assert torch.equal(seeded.segment_device(dev), Segmenter(**kw).predict_device(dev, model, refine=N_ITER - 1))
