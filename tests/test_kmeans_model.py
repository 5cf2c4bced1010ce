"""The k-means model (SPEC.md §28) on the CPU: the contract the frozen symbol tables cannot carry (include/gcs_model.h <->
``_lib.MODEL_EXTENSIONS`` <-> the built library's exports), the argument rules of gcs_kmeans_evaluate (refused before anything is
launched, so they run without a GPU), the restatement (tests/kmeans_model_ref.py) against the oracle of SPEC.md §4 and on crafted
centroids, and the host logic - fit, predict, warm start, refusals, save / load - through the stand-in ops
(tests/kmeans_model_ops.py). No GPU."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

import kmeans_model_ref as km
from gabor_color_image_segmentation_amd import KMeansModel, Segmenter, make_bank
from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
from kmeans_model_ops import KMeansModelOps
from oracle import spec_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the library: symbols and argument rules

@pytest.fixture(scope="module")
def lib(built):
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load()


def test_header_table_and_exports_agree(lib):
    from gabor_color_image_segmentation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gcs_model.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gcs_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.MODEL_EXTENSIONS) == {"gcs_kmeans_evaluate"}, declared ^ set(_lib.MODEL_EXTENSIONS)
    assert 'extern "C"' in hdr and "ABI 18" in hdr and '#include "gcs.h"' in hdr
    assert "torch" not in hdr.lower() and "at::" not in hdr
    for name, (res, args) in _lib.MODEL_EXTENSIONS.items():
        fn = getattr(lib, name)                               # exported by the built library
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):                        # pointers and the stream are void pointers, the rest ints
            assert (a is C.c_void_p) == ("*" in p or p.startswith("gcs_stream_t")), (name, p)
    others = set(_lib.SIGNATURES) | set(_lib.EXTENSIONS) | set(_lib.THIN_EXTENSIONS) | set(_lib.MATCH_EXTENSIONS)
    assert not set(_lib.MODEL_EXTENSIONS) & others
    assert lib.gcs_abi_version() == 18 and _lib.ABI_VERSION == 18
    for name in ("gcs.h", "gcs_cues.h", "gcs_thin.h", "gcs_match.h"):     # the frozen headers do not know the symbol
        assert "gcs_kmeans_evaluate" not in open(os.path.join(ROOT, "include", name)).read(), name


def test_a_library_without_the_symbol_still_loads_and_the_ops_refuse(built):
    from gabor_color_image_segmentation_amd import _lib
    from gabor_color_image_segmentation_amd.segmenter import HipOps
    saved, held = dict(_lib.MODEL_EXTENSIONS), _lib._lib
    try:
        _lib.MODEL_EXTENSIONS["gcs_not_in_this_library"] = (C.c_int, [])
        _lib._lib = None
        lib = _lib.load()
        assert not hasattr(lib, "gcs_not_in_this_library") and hasattr(lib, "gcs_kmeans_evaluate")
    finally:
        _lib.MODEL_EXTENSIONS.clear()
        _lib.MODEL_EXTENSIONS.update(saved)
        _lib._lib = held

    class Old:                                               # what the method asks of its library, without the symbol
        pass
    ops = HipOps.__new__(HipOps)
    ops.lib = Old()
    with pytest.raises(_lib.GcsError, match="does not export gcs_kmeans_evaluate"):
        HipOps.kmeans_evaluate.__wrapped__(ops, None, None, 1, 8, 8, 2, 1)


def test_evaluate_validates_before_launching(lib):
    """Argument errors are reported with code 1 and a message, without touching the GPU (so this runs on the CPU box)."""
    p = [C.c_void_p(q << 34) for q in range(1, 7)]           # non-NULL dummies far apart, never dereferenced
    good = dict(feats=p[0], cent=p[1], B=3, H=19, W=23, ns=4, no=6, k=8, n_sets=3, labels=p[2], best=p[3], second=p[4], stats=p[5])

    def call(**bad):
        a = dict(good, **bad)
        return lib.gcs_kmeans_evaluate(a["feats"], a["cent"], a["B"], a["H"], a["W"], a["ns"], a["no"], a["k"], a["n_sets"],
                                       a["labels"], a["best"], a["second"], a["stats"], None)
    for bad in (dict(feats=None), dict(cent=None), dict(labels=None, best=None, second=None, stats=None)):
        assert call(**bad) == 1 and b"NULL" in lib.gcs_last_error(), bad
    for bad in (dict(k=0), dict(k=-1), dict(k=17)):
        assert call(**bad) == 1 and b"k must be in 1..16" in lib.gcs_last_error(), bad
    for bad in (dict(n_sets=0), dict(n_sets=2), dict(n_sets=4), dict(n_sets=-1)):
        assert call(**bad) == 1 and b"n_sets" in lib.gcs_last_error(), bad
    for bad in (dict(B=0, n_sets=1), dict(B=-1, n_sets=1), dict(B=65536, n_sets=1), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097),
                dict(ns=0), dict(ns=9), dict(no=0), dict(ns=8, no=65)):       # (8 x 65 filters: 1560 features)
        assert call(**bad) == 1 and b"bad shape or bank" in lib.gcs_last_error(), bad
    # the bound P_set * D < 2^31: the largest shapes in use are inside it, a set of twice the pixels is not
    d = 72
    inside = (dict(B=64, H=481, W=321, n_sets=1), dict(B=1, H=2048, W=2048, n_sets=1), dict(B=65535, H=481, W=321, n_sets=65535))
    for shape in inside:
        pixels = shape["H"] * shape["W"] * (shape["B"] if shape["n_sets"] == 1 else 1)
        assert pixels * d < 1 << 31
    for bad in (dict(B=130, H=481, W=481, n_sets=1), dict(B=8, H=4096, W=4096, ns=8, no=6, n_sets=8),
                dict(B=2, H=4096, W=4096, ns=1, no=22, n_sets=1)):
        a = dict(good, **bad)
        pixels = a["H"] * a["W"] * (a["B"] if a["n_sets"] == 1 else 1)
        assert pixels * 3 * a["ns"] * a["no"] >= 1 << 31
        assert call(**bad) == 1 and b"2^31" in lib.gcs_last_error(), bad
    assert b"gcs_kmeans_evaluate" in lib.gcs_last_error()
    # (a call inside every rule would launch, so it is made on the GPU: tests/test_gpu_kmeans_model.py)


# ---- the restatement

def _features(b, h, w, seed, bank=None):
    bank = bank or make_bank()
    imgs = synthetic_batch(b, h, w, seed=seed)
    tapq = bank.tapq.astype(np.int64)
    x = np.stack([so.gabor_features(im, tapq, bank.shift, bank.n_orient).reshape(bank.n_features, -1).T for im in imgs])
    return imgs, x.astype(np.int64)                           # (B, P, D)


@pytest.fixture(scope="module")
def feats():
    return _features(3, 24, 40, seed=11)


@pytest.mark.parametrize("k", [1, 2, 3, 8, 16])
def test_restatement_against_the_oracle_and_its_own_sums(feats, k):
    _, x = feats
    rng = np.random.default_rng(k)
    for n_sets in (1, 3):
        cent = np.stack([so.kmeans_init(x[s], k) for s in range(n_sets)])
        cent[:, k // 2] = rng.integers(0, 65536, cent.shape[2])       # one centroid anywhere in the uint16 range
        lab, best, second, stats = km.evaluate_batch(x, cent)
        for i in range(3):
            assert np.array_equal(lab[i], so.kmeans_assign(x[i], cent[i if n_sets == 3 else 0]))
        assert lab.dtype == np.int32 and best.dtype == second.dtype == stats.dtype == np.int64
        assert stats[:, :, 0].sum() == x.shape[0] * x.shape[1] and stats[:, :, 1].sum() == best.sum()
        if n_sets == 3:
            assert (stats[:, :, 0].sum(axis=1) == x.shape[1]).all()
            assert np.array_equal(stats[:, :, 1].sum(axis=1), best.sum(axis=1))
        assert (second >= best).all() and (best >= 0).all()
        if k == 1:
            assert np.array_equal(second, best) and not km.confidence(best, second).any()
        conf = km.confidence(best, second)
        assert conf.dtype == np.float32 and (conf >= 0).all() and (conf <= 1).all()
        assert np.array_equal(km.mse(stats, x.shape[2]),
                              stats[:, :, 1].sum(axis=1) / (stats[:, :, 0].sum(axis=1) * x.shape[2]))


def test_worked_example():
    """SPEC.md §28: D = 1, k = 3, centroids [10, 10, 40], pixels [10, 20, 30, 100]."""
    lab, best, second, stats = km.evaluate(np.array([[10], [20], [30], [100]]), np.array([[10], [10], [40]]))
    assert lab.tolist() == [0, 0, 2, 2] and best.tolist() == [0, 100, 100, 3600] and second.tolist() == [0, 100, 400, 8100]
    assert stats.tolist() == [[2, 100], [0, 0], [2, 3700]] and km.mse(stats[None], 1).tolist() == [950.0]
    assert km.confidence(best, second).tolist() == [0.0, 0.0, 0.75, float(np.float32(5 / 9))]


def test_restatement_on_crafted_centroids(feats):
    _, x = feats
    x0 = x[0]
    p, d = x0.shape
    c = so.kmeans_init(x0, 4)
    dup = np.concatenate([c, c])                              # every centroid twice: the runner-up is the twin
    lab, best, second, _ = km.evaluate(x0, dup)
    assert np.array_equal(second, best) and (lab < 4).all() and np.array_equal(lab, so.kmeans_assign(x0, c))
    own = c.copy()
    own[2] = x0[p // 3]                                       # a centroid equal to a pixel's vector
    lab, best, second, _ = km.evaluate(x0, own)
    assert best[p // 3] == 0
    assert km.confidence(best, second)[p // 3] == (1.0 if second[p // 3] > 0 else 0.0)
    for value in (0, 65535):                                  # all centroids alike: label 0 everywhere, margin 0
        flat = np.full((3, d), value, np.int64)
        lab, best, second, stats = km.evaluate(x0, flat)
        assert not lab.any() and np.array_equal(second, best) and stats[0, 0] == p and not stats[1:].any()
        assert np.array_equal(best, ((x0 - value) ** 2).sum(axis=1))
    # the largest term: a feature of 0 against a centroid of 65535 in every dimension stays exact in int64
    lab, best, second, stats = km.evaluate(np.zeros((2, d), np.int64), np.full((1, d), 65535, np.int64))
    assert best.tolist() == [d * 65535 ** 2] * 2 and stats.tolist() == [[2, 2 * d * 65535 ** 2]]
    assert km.confidence(np.array([0, 0, 5]), np.array([0, 7, 5])).tolist() == [0.0, 1.0, 0.0]


# ---- the host logic through the stand-in ops

K, N_ITER = 5, 4


def _seg(**kw):
    kw.setdefault("k", K)
    kw.setdefault("n_iter", N_ITER)
    return Segmenter(ops=KMeansModelOps(make_bank()), **kw)


def _t(imgs):
    return torch.from_numpy(np.ascontiguousarray(imgs))


def _cent(model):
    return model.centroids.numpy().astype(np.int64)


@pytest.fixture(scope="module")
def fitted(feats):
    """Models of images 0 and 1 in both modes, fitted once and never changed."""
    imgs, x = feats
    seg = _seg()
    return seg, {mode: seg.fit_device(_t(imgs[:2]), mode) for mode in ("global", "per_image")}


def test_fit_device_is_the_oracles_loop_with_the_restatements_tables(feats, fitted):
    imgs, x = feats
    seg, models = fitted
    g, pi = models["global"], models["per_image"]
    lab_g, cent_g = so.kmeans(x[:2].reshape(-1, x.shape[2]), K, N_ITER, init_from=x[0])
    assert g.n_sets == 1 and g.k == K and g.centroids.dtype == torch.uint16 and np.array_equal(_cent(g)[0], cent_g)
    assert pi.n_sets == 2
    for i in range(2):
        assert np.array_equal(_cent(pi)[i], so.kmeans(x[i], K, N_ITER)[1])
    for model, sets in ((g, 1), (pi, 2)):
        _, _, _, stats = km.evaluate_batch(x[:2], _cent(model))
        assert model.counts.dtype == model.inertia.dtype == torch.int64
        assert np.array_equal(model.counts.numpy(), stats[:, :, 0]) and np.array_equal(model.inertia.numpy(), stats[:, :, 1])
        assert model.mse.dtype == np.float64 and np.array_equal(model.mse, km.mse(stats, x.shape[2]))
        assert model.signature == seg.model_signature and model.signature["k"] == K
    assert np.array_equal(np.bincount(lab_g, minlength=K), g.counts.numpy()[0])
    assert [c[0] for c in seg.ops.calls if c[0] == "evaluate"] == ["evaluate"] * 2      # one evaluate launch per fit


def test_predict_device_is_the_assignment_under_the_model(feats, fitted):
    imgs, x = feats
    seg, models = fitted
    got = seg.predict_device(_t(imgs[2:]), models["global"]).numpy()
    assert got.dtype == np.int32 and np.array_equal(got.reshape(1, -1)[0], so.kmeans_assign(x[2], _cent(models["global"])[0]))
    # a model of B codebooks: image i under codebook i; the model itself is not changed by any call
    before = _cent(models["per_image"]).copy()
    got = seg.predict_device(_t(imgs[1:]), models["per_image"], refine=3).numpy()
    want, _ = km.schedule(x[1:], before, 4, "per_image")
    assert np.array_equal(got.reshape(2, -1), want) and np.array_equal(_cent(models["per_image"]), before)
    assert np.array_equal(seg.segment_device(_t(imgs), codebook=models["global"]).numpy(),
                          seg.predict_device(_t(imgs), models["global"]).numpy())


@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_refine_is_the_schedule_from_the_model(feats, fitted, mode):
    imgs, x = feats
    seg, models = fitted
    model = models["global"]
    got = seg.predict_device(_t(imgs), model, refine=2, mode=mode).numpy().reshape(3, -1)
    want, cents = km.schedule(x, _cent(model)[0], 3, mode)
    assert np.array_equal(got, want)
    frozen, _ = km.schedule(x, _cent(model)[0], 1, mode)
    assert not np.array_equal(want, frozen), "the refinement changes no label: the case proves nothing"
    assert np.array_equal(seg.predict_device(_t(imgs), model, refine=0, mode=mode).numpy().reshape(3, -1), frozen)
    # a fit warm-started from the model: the plan's n_iter passes from c^0 = the model
    warm = seg.fit_device(_t(imgs), mode, init=model)
    assert np.array_equal(_cent(warm), km.schedule(x, _cent(model)[0], N_ITER, mode)[1])


def test_evaluate_and_confidence_device(feats, fitted):
    imgs, x = feats
    seg, models = fitted
    model = models["global"]
    lab, best, second, stats = km.evaluate_batch(x, _cent(model))
    res = seg.evaluate_device(_t(imgs), model, best=True, second=True)
    assert sorted(res) == ["best", "labels", "second", "stats"]
    for name, want in (("labels", lab), ("best", best), ("second", second)):
        assert np.array_equal(res[name].numpy().reshape(3, -1), want), name
    assert np.array_equal(res["stats"].numpy(), stats)
    assert sorted(seg.evaluate_device(_t(imgs), model, labels=False)) == ["stats"]
    labels, conf = seg.confidence_device(_t(imgs), model)
    assert conf.dtype == torch.float32 and np.array_equal(conf.numpy().reshape(3, -1), km.confidence(best, second))
    assert np.array_equal(labels.numpy().reshape(3, -1), lab)
    # without a model: the plan's own loop first, then its centroids
    for mode in ("per_image", "global"):
        own = seg.evaluate_device(_t(imgs), mode=mode)
        assert np.array_equal(own["labels"].numpy(), seg.segment_device(_t(imgs), mode).numpy())
        assert np.array_equal(own["stats"].numpy()[:, :, 0].sum(axis=1), [x.shape[1]] * 3 if mode == "per_image" else [3 * x.shape[1]])
    with pytest.raises(ValueError, match="at least one"):
        seg.evaluate_device(_t(imgs), model, labels=False, stats=False)


def test_refusals(feats, fitted):
    imgs, x = feats
    seg, models = fitted
    g, pi = models["global"], models["per_image"]
    t = _t(imgs)
    with pytest.raises(ValueError, match="codebook must be a KMeansModel"):
        seg.predict_device(t, _cent(g))
    with pytest.raises(ValueError, match="another feature space.*k differ"):
        _seg(k=K + 1).predict_device(t, g)
    with pytest.raises(ValueError, match="another feature space.*smoothing differ"):
        other = dict(g.signature, smoothing=1.0)
        seg.predict_device(t, KMeansModel(g.centroids, g.counts, g.inertia, other))
    with pytest.raises(ValueError, match="a model of 2 codebooks"):
        seg.predict_device(t, pi)                              # B' = 2 codebooks, 3 images
    with pytest.raises(ValueError, match="a model of 2 codebooks"):
        seg.predict_device(t[:2], pi, mode="global")
    for bad in (-1, 0.5, "2", None, True):
        with pytest.raises(ValueError, match="refine must be an integer >= 0"):
            seg.predict_device(t, g, refine=bad)
    with pytest.raises(ValueError, match="dist_group"):
        seg.segment_device(t, codebook=g, dist_group=object())
    strip = _t(np.zeros((1, 32, 32, 3), np.uint8))
    with pytest.raises(ValueError, match="row strips"):
        seg.segment_rows_sharded_device(strip, 0, 32, 0, 32, codebook=g)
    with pytest.raises(ValueError, match="row strips"):
        seg.segment_owned_rows_device(strip, 32, codebook=g)
    with pytest.raises(ValueError, match="k = "):
        KMeansModel(g.centroids, g.counts, g.inertia, dict(g.signature, k=K + 1))
    with pytest.raises(ValueError, match="one codebook"):
        list(seg.segment_images([imgs[0]], codebook=pi))
    plain = Segmenter(ops=__import__("fake_ops").OracleOps(make_bank()), k=K, n_iter=N_ITER)
    with pytest.raises(ValueError, match="ops that have kmeans_evaluate"):
        plain.fit_device(t)


def test_superpixel_plans_refuse_a_codebook(fitted):
    from gabor_color_image_segmentation_amd import segmenter as sg
    seg, models = fitted
    sp = Segmenter.__new__(Segmenter)                          # (the stand-in has no superpixel stage: the rule alone)
    sp.n_superpixels, sp.model_signature = 64, seg.model_signature
    with pytest.raises(ValueError, match="n_superpixels = 0"):
        sg.Segmenter._codebook_check(sp, models["global"], 1, "per_image")


def test_save_and_load_round_trip(fitted, tmp_path):
    seg, models = fitted
    for name, model in models.items():
        path = str(tmp_path / (name + ".npz"))
        model.save(path)
        back = KMeansModel.load(path)
        assert back.signature == model.signature == seg.model_signature
        for a, b in ((back.centroids, model.centroids), (back.counts, model.counts), (back.inertia, model.inertia)):
            assert a.dtype == b.dtype and np.array_equal(a.numpy(), b.numpy())
        assert np.array_equal(back.mse, model.mse) and back.cpu() is back and back.to("cpu") is back
        with np.load(path) as z:
            assert sorted(z.files) == ["centroids", "counts", "inertia", "signature"] and z["centroids"].dtype == np.uint16
    buf = io.BytesIO()
    np.savez(buf, centroids=np.zeros((1, 2, 3), np.float32), counts=np.zeros((1, 2), np.int64), inertia=np.zeros((1, 2), np.int64),
             signature=np.array("{}"))
    buf.seek(0)
    with pytest.raises(ValueError, match="not a k-means model file"):
        KMeansModel.load(buf)


def test_two_models_used_alternately_each_give_their_own_labels(feats, fitted):
    imgs, x = feats
    seg, models = fitted
    a = models["global"]
    b = seg.fit_device(_t(imgs[2:]), "global")
    assert not np.array_equal(_cent(a), _cent(b))
    want = {id(m): np.stack([so.kmeans_assign(x[i], _cent(m)[0]) for i in range(3)]) for m in (a, b)}
    assert not np.array_equal(want[id(a)], want[id(b)])
    for m in (a, b, a, b, b, a):
        assert np.array_equal(seg.predict_device(_t(imgs), m).numpy().reshape(3, -1), want[id(m)])


def test_host_paths_take_a_codebook(feats, fitted):
    import gabor_color_image_segmentation_amd.segmenter as sg
    imgs, x = feats
    seg, models = fitted
    model = models["global"]
    want = seg.predict_device(_t(imgs), model, refine=1).numpy()
    assert np.array_equal(seg.segment_batch(imgs, codebook=model, refine=1), want)
    assert np.array_equal(seg(imgs[1], codebook=model, refine=1), want[1])
    assert np.array_equal(np.stack(list(seg.segment_images(list(imgs), batch=2, codebook=model, refine=1))), want)
    assert np.array_equal(np.concatenate(list(seg.segment_stream([imgs[:2], imgs[2:]], codebook=model, refine=1))), want)
    assert seg.segment_batch(imgs, out_dtype=np.uint8, codebook=model).dtype == np.uint8
    # the one-shot calls pop codebook and refine before the plan is looked up by its keywords
    kw = dict(k=K, n_iter=N_ITER)
    saved = dict(sg._default)
    try:
        sg._default.clear()
        sg._default[tuple(sorted(kw.items()))] = seg
        assert np.array_equal(sg.segment(imgs[1], codebook=model, refine=1, **kw), want[1])
        assert np.array_equal(sg.segment_batch(imgs, codebook=model, refine=1, **kw), want)
        assert list(sg._default) == [tuple(sorted(kw.items()))]
        fit = sg.fit_codebook(imgs[:2], **kw)
        assert np.array_equal(_cent(fit), _cent(model)) and fit.device.type == "cpu"
        labels, conf = sg.segment_confidence(imgs[2], codebook=model, **kw)
        lab, best, second, _ = km.evaluate(x[2], _cent(model)[0])
        assert np.array_equal(labels.reshape(-1), lab) and np.array_equal(conf.reshape(-1), km.confidence(best, second))
        own, _ = sg.segment_confidence(imgs[2], **kw)
        assert np.array_equal(own, seg(imgs[2]))
    finally:
        sg._default.clear()
        sg._default.update(saved)
