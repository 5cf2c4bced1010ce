"""The stage checks of the self-updating Lloyd pass on the device, shared by tests/test_gpu_self_updating_stages.py and its child
process tests/checkers/fold_rows_child.py (GCS_KP_FOLD_ROWS is read once per process): one launch of gcs_kmeans_pass_fused from a
workspace the test has written, compared piece by piece with the model of tests/fused_workspace.py - the centroid array the pass
writes and the one it keeps, the buffer it reads, the one it clears, the one it adds into, the ticket, every padding byte. All of it
goes through ops.fused_workspace, ops.assign_accumulate(fused=(ws, t)) and ops.assign_raster(fused=(ws, t)); features are the C
oracle's on the images and banks of tests/hot_banks.py."""
import numpy as np

import fused_workspace as fw
import hot_banks as hb
from lloyd_ref import _update_cases
from oracle import c_oracle as co
from oracle import spec_oracle as so
from slab_layout import tile_of_pixels

_REF = {}
_STAGES = {}


def ref_features(cfg, imgs):
    """C-oracle features (B, D, H, W) uint16 of a hot bank, cached per (bank, images)."""
    key = (cfg, imgs.shape, imgs.tobytes())
    if key not in _REF:
        if len(_REF) > 8:
            _REF.pop(next(iter(_REF)))
        bank = hb.hot_bank(*cfg)
        _REF[key] = np.stack([co.gabor_features(im, bank.tapq, bank.shift, bank.n_orient) for im in imgs])
    return _REF[key]


class Stage:
    """One (bank, images) on the device: the feature slab gabor_features wrote, and the oracle's features beside it."""

    def __init__(self, torch, cfg, imgs):
        self.torch, self.cfg, self.imgs = torch, cfg, imgs
        self.seg = hb.hot_segmenter(hb.hot_bank(*cfg))
        self.ops = self.seg.ops
        self.b, self.h, self.w = imgs.shape[:3]
        self.ref = ref_features(cfg, imgs)
        self.d = self.ref.shape[1]
        self.x = self.ref.reshape(self.b, self.d, -1).transpose(0, 2, 1).astype(np.int64)      # (B, P, D)
        self.feats = self.ops.feature_slab(self.b, self.h, self.w)
        self.ops.gabor_features(torch.from_numpy(imgs).cuda(), self.feats)
        self.parts = int(self.ops.lib.gcs_kmeans_parts_per_image(self.b, self.h, self.w))

    def layout(self, mode, k):
        n_sets = self.b if mode == "per_image" else 1
        return n_sets, fw.fold_rows(self.b, self.parts, n_sets, fw.env_fold_rows()), k, self.d

    def mixed_tiles(self):
        """Does some image hold tiles with and tiles without a value >= 4096 (flagged beside unflagged tiles of the split slab)?"""
        tile = tile_of_pixels(self.h, self.w)
        for i in range(self.b):
            n = len(np.unique(tile[(self.ref[i] >= 4096).any(axis=0)]))
            if 0 < n < tile.max() + 1:
                return True
        return False

    def run(self, buf, mode, k, t, last, reverse, out_dtype=None, seed=0):
        """One launch on a workspace holding ``buf`` -> (bytes after, cent (n_sets, k, D) int64, label map (B, P) or None).
        ``cent`` and the label map start as garbage."""
        torch = self.torch
        n_sets = self.layout(mode, k)[0]
        ws = self.ops.fused_workspace(self.b, self.h, self.w, k, n_sets)
        assert ws is not None and ws.numel() == len(buf), (None if ws is None else ws.numel(), len(buf))
        ws.copy_(torch.from_numpy(buf))
        g = torch.Generator().manual_seed(seed + 1)
        cent = torch.randint(-32768, 32767, (n_sets, k, self.d), generator=g, dtype=torch.int16).cuda()
        out = None
        if last:
            out = torch.full((self.b, self.h, self.w), 99, dtype=out_dtype, device="cuda")
            self.ops.assign_raster(self.feats, cent, self.b, self.h, self.w, k, n_sets, out, reverse=bool(reverse), fused=(ws, t))
            out = out.cpu().numpy().reshape(self.b, -1).astype(np.int64)
        else:
            self.ops.assign_accumulate(self.feats, cent, self.b, self.h, self.w, k, n_sets, None, None, reverse=bool(reverse),
                                       fused=(ws, t))
        return ws.cpu().numpy(), cent.cpu().numpy().view(np.uint16).astype(np.int64), out


def stage(torch, cfg, imgs):
    key = (cfg, imgs.shape, imgs.tobytes())
    if key not in _STAGES:
        if len(_STAGES) > 6:
            _STAGES.pop(next(iter(_STAGES)))
        _STAGES[key] = Stage(torch, cfg, imgs)
    return _STAGES[key]


def garbage(rng, view):
    """Fill a view with bytes that are all non-zero."""
    raw = view.reshape(-1).view(np.uint8)
    raw[...] = rng.integers(1, 256, raw.shape, dtype=np.uint8)


def written_state(lay, t, seed):
    """The workspace 'as pass t - 1 left it' (t >= 1): buffer (t - 1) % 3 holds the sums of _update_cases - for set s its clusters
    rotated by s, cut into random shares over the rows -, array (t - 1) & 1 its ``old`` codebook, buffer t % 3 zero, buffer
    (t + 1) % 3 and the array the pass writes all non-zero garbage, ticket zero.
    -> (bytes, centroids (n_sets, k, D) the pass must make in Python integers, the written sums (n_sets, k, D + 1))."""
    n_sets, rows, k, d = lay
    rng = np.random.default_rng(seed)
    old, sums, want = _update_cases(d, k)
    buf = np.zeros(fw.workspace_bytes(*lay), np.uint8)
    v = fw.views(buf, *lay)
    wants, written = [], []
    for s in range(n_sets):
        o, sm, wt = (np.roll(np.array(a, np.int64), s, axis=0) for a in (old, sums, want))
        cuts = np.sort(rng.integers(0, sm + 1, (rows - 1,) + sm.shape), axis=0)          # random shares that add up exactly
        share = np.diff(np.concatenate([np.zeros((1,) + sm.shape, np.int64), cuts, sm[None]]), axis=0)
        v.sums[(t - 1) % 3][s] = share.astype(np.uint64)
        v.cents[(t - 1) & 1][s] = o.astype(np.uint16)
        wants.append(wt)
        written.append(sm)
    garbage(rng, v.sums[(t + 1) % 3])
    garbage(rng, v.cents[t & 1])
    return buf, np.stack(wants), np.stack(written)


def pass0_state(lay, last, seed):
    """What pass 0 may find: buffer 0 zero, the buffer behind the rotation (2), both centroid arrays and the ticket garbage - pass
    0 reads none of them. Buffer 1 is the one its prologue clears: garbage before a pass that is not the last. A pass 0 that IS
    the last (n_iter = 1) must write to no sum buffer: buffer 0 is garbage too then, and buffer 1 holds the zeros of a legal
    workspace, onto which the prologue's clear stores zeros."""
    rng = np.random.default_rng(seed)
    buf = np.zeros(fw.workspace_bytes(*lay), np.uint8)
    v = fw.views(buf, *lay)
    garbage(rng, v.sums[2])
    garbage(rng, v.sums[0] if last else v.sums[1])
    garbage(rng, v.cents[0])
    garbage(rng, v.cents[1])
    garbage(rng, v.ticket)
    return buf


def inputs_hold(written, want):
    """What the written sums are about (all true for k >= 6 and D >= 8)."""
    n = written[..., -1:]
    s = written[..., :-1]
    full = (n[0, :, 0] > 0).tolist()
    return dict(past_38_bits=bool((2 * s + n >= 1 << 38).any()), g_max=bool((want == hb.G_MAX).any()),
                bit_15=bool((want == 32768).any()), tie=bool(((n > 0) & ((2 * s + n) % np.maximum(2 * n, 1) == 0)).any()),
                empty_between_full=any(not f and any(full[:j]) and any(full[j + 1:]) for j, f in enumerate(full)))


def _diff(got, want):
    bad = np.argwhere(got != want)
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} of {got.size} differ, first at {i}: got {got[i]}, want {want[i]}"


def compare(got, want, lay, t, last, tag):
    """The workspace after pass t against the model's, piece by piece, so that a failure names the stage."""
    n_sets, rows, k, d = lay
    g, e = fw.views(got, *lay), fw.views(want, *lay)
    for i in range(2):
        role = "the array the pass writes" if i == (t & 1) else "the array of the pass before (kept)"
        assert np.array_equal(g.cents[i], e.cents[i]), (tag, f"centroid array {i}: {role}", _diff(g.cents[i], e.cents[i]))
    for i in range(3):
        if i == (t + 1) % 3:
            role = "the buffer the prologue clears"
        elif i == t % 3:
            role = "the buffer the pass adds into" if not last else "the buffer a last pass leaves alone"
        else:
            role = "the buffer the pass reads (kept)" if not last else "the buffer the last workgroup clears"
        if i == t % 3 and not last and rows > 1:
            gt, et = fw.totals(g.sums[i]), fw.totals(e.sums[i])
            assert np.array_equal(gt, et), (tag, f"sum buffer {i}: {role}, total of {rows} rows", _diff(gt, et))
            used = int(g.sums[i].reshape(n_sets, rows, -1).any(axis=2).sum())
            assert used > 1, (tag, f"sum buffer {i}: {role}: {used} of {rows} rows hold anything")
        else:
            assert np.array_equal(g.sums[i], e.sums[i]), (tag, f"sum buffer {i}: {role}", _diff(g.sums[i], e.sums[i]))
        assert np.array_equal(g.sum_pad[i], e.sum_pad[i]), (tag, f"padding of sum buffer {i}")
    assert np.array_equal(g.ticket, e.ticket), (tag, "ticket", g.ticket[:2].tolist(), e.ticket[:2].tolist())
    for i in range(2):
        assert np.array_equal(g.cent_pad[i], e.cent_pad[i]), (tag, f"padding of centroid array {i}")


def check_pass(st, buf, mode, k, t, last, tag, want_cent=None):
    """One pass from the state ``buf``, both sweep directions (and both label dtypes when it is the last), against the model.
    ``want_cent``: the centroids in Python integers, where the caller has them from another source than the model."""
    import torch
    lay = st.layout(mode, k)
    exp, cent, lab = fw.expected_pass(buf, st.x, t, last, mode, k, lay[1])
    if want_cent is not None:
        assert np.array_equal(cent, want_cent), (tag, "model")
    for reverse in (0, 1):
        for dt in (torch.int32, torch.uint8) if last else (None,):
            tg = (tag, mode, f"k={k}", f"t={t}", "last" if last else "not last", f"reverse={reverse}", str(dt))
            got, got_cent, got_lab = st.run(buf, mode, k, t, last, reverse, dt, seed=t)
            assert np.array_equal(got_cent, cent), (tg, "cent", _diff(got_cent, cent))
            compare(got, exp, lay, t, last, tg)
            if last:
                assert np.array_equal(got_lab, lab), (tg, "labels", _diff(got_lab, lab))
    return exp, cent, lab


def check_written_pass(st, mode, k, t, last, tag, need_inputs=None):
    """(a) and (b) of the stage tests: pass t >= 1 from a written workspace."""
    lay = st.layout(mode, k)
    buf, want, written = written_state(lay, t, seed=17 * t + lay[0])
    hold = inputs_hold(written, want)
    if need_inputs if need_inputs is not None else (k >= 6 and st.d >= 8):
        assert all(hold.values()), (tag, hold)
    exp, cent, lab = check_pass(st, buf, mode, k, t, last, tag, want_cent=want)
    return hold


def check_pass0(st, mode, k, last, tag):
    """(c): pass 0 makes the SPEC.md §4 init centroids of every set and the exact sums; as the only pass of a loop it writes to no
    sum buffer and does not touch the ticket."""
    lay = st.layout(mode, k)
    init = np.stack([so.kmeans_init(st.x[s], k) for s in range(lay[0])])
    check_pass(st, pass0_state(lay, last, seed=5 + lay[0]), mode, k, 0, last, tag, want_cent=init)


def check_loop(st, mode, k, n_iter, tag):
    """(e): a loop of direct calls on a zeroed workspace, read back after every pass: the whole state equals the model's, the
    centroids of pass t > 0 equal so.kmeans_update of the exact assignment of pass t - 1, and the loop ends on the C oracle's labels
    and a workspace as it was found."""
    import torch
    lay = st.layout(mode, k)
    n_sets = lay[0]
    buf = np.zeros(fw.workspace_bytes(*lay), np.uint8)
    model = buf
    prev_cent = prev_lab = None
    for t in range(n_iter):
        last = t == n_iter - 1
        tg = (tag, mode, f"k={k}", f"loop of {n_iter}", f"t={t}")
        model, cent, lab = fw.expected_pass(model, st.x, t, last, mode, k, lay[1])
        if t > 0:
            for s in range(n_sets):
                xs = st.x[s] if n_sets > 1 else st.x.reshape(-1, st.d)
                ls = prev_lab[s] if n_sets > 1 else prev_lab.reshape(-1)
                assert np.array_equal(cent[s], so.kmeans_update(xs, ls, prev_cent[s])[0]), (tg, "model")
        buf, got_cent, got_lab = st.run(buf, mode, k, t, last, not (t & 1), torch.int32, seed=t)
        assert np.array_equal(got_cent, cent), (tg, "cent", _diff(got_cent, cent))
        compare(buf, model, lay, t, last, tg)
        if lay[1] > 1:
            model = buf            # same totals, but the kernel's spread over the rows: the next pass is modelled from it
        prev_cent, prev_lab = cent, lab
    feats = st.ref.reshape(st.b, st.d, -1)
    if mode == "global":
        want = co.kmeans(feats, k, n_iter)[0]
    else:
        want = np.stack([co.kmeans(feats[i:i + 1], k, n_iter)[0][0] for i in range(st.b)])
    assert np.array_equal(got_lab, want), (tag, mode, "labels of the loop", _diff(got_lab, want))
    assert fw.is_as_found(buf, *lay), (tag, mode, "the workspace after the loop")
    return want
