"""Edge-shape scoring fixture (run under /opt/conda/bin/python3.9, cwd = /root/reference/BSD_metrics).

Imports the reference's own ``metrics`` class (BSD_metrics/metrics.py:18) and records every key of ``get_metrics()``
(metrics.py:246-255) - or the exception it raises - for small synthetic label maps and annotator stacks at the shapes where
the GPU scorer's tiles, bit-plane words and table regimes change (tile 16 x 64 with a 2-pixel halo, 64-bit plane words):

    scoring_edge_maps.npz     lab_<HxW>_<kind> and truth_<HxW>_<stack> (uint16), built here from a fixed seed
    scoring_edge_golden.json  {"<HxW>/<kind>/<stack>": {key: float} | {"raises": "<exception name>"}}

A case key names its inputs: label map ``lab_<HxW>_<kind>``, annotator maps ``truth_<HxW>_<stack>`` ([A][H][W]; stack "a0"
is the empty list). Only data is written. The archive is written member by member with a fixed timestamp, so the same
script gives the same bytes.
"""
import io
import json
import sys
import zipfile

import numpy as np

sys.path.insert(0, '.')
from metrics import metrics            # noqa: E402  (the reference class)

SHAPES = [(1, 70), (70, 1), (2, 2), (3, 5), (5, 130), (16, 64), (17, 65), (15, 63), (63, 127), (64, 128), (65, 129),
          (33, 193), (48, 192)]
KINDS = ['noise2', 'noise3', 'rows1', 'cols1', 'rows7', 'cols7', 'checker', 'blocks5', 'seam', 'corners', 'constant']
STACKS = ['a1', 'a3big', 'a9frame']     # 1 / 3 / 9 maps; a3big: labels above 255; a9frame: boundaries on all four borders


def label_map(kind, h, w, rng):
    y, x = np.mgrid[:h, :w]
    if kind == 'noise2':
        return rng.integers(0, 2, (h, w))
    if kind == 'noise3':
        return rng.integers(0, 3, (h, w))
    if kind == 'rows1':
        return y % 2
    if kind == 'cols1':
        return x % 2
    if kind == 'rows7':
        return y // 7
    if kind == 'cols7':
        return x // 7
    if kind == 'checker':
        return (y + x) % 2
    if kind == 'blocks5':
        return (y // 5) * ((w + 4) // 5) + x // 5
    if kind == 'seam':                  # the only boundaries lie on columns 63/64 and rows 15/16 (the scorer's tile seams)
        return (x >= 64) + 2 * (y >= 16)
    if kind == 'corners':
        m = np.zeros((h, w), np.int64)
        m[0, 0], m[0, w - 1], m[h - 1, 0], m[h - 1, w - 1] = 1, 2, 3, 4
        return m
    return np.zeros((h, w), np.int64)   # 'constant'


def voronoi(h, w, n, rng):
    """Annotator-like map: n Voronoi cells, labels from 1 as BSD's. Never constant: a map that came out constant (tiny
    shapes) is split in two along its longer side."""
    pts = rng.uniform(0, 1, (n, 2)) * [h, w]
    y, x = np.mgrid[:h, :w]
    m = np.argmin((y[..., None] - pts[:, 0]) ** 2 + (x[..., None] - pts[:, 1]) ** 2, axis=2) + 1
    if m.min() == m.max():
        m = 1 + ((x >= w // 2) if w >= h else (y >= h // 2))
    return m


def stack(name, h, w, rng):
    n = {'a1': 1, 'a3big': 3, 'a9frame': 9, 'a3const': 3}[name]
    maps = [voronoi(h, w, 2 + (3 * a) % 7, rng) for a in range(n)]
    if name == 'a3big':                 # labels above 255: the uint16 region tables
        maps[1] = np.where(maps[1] % 2 == 0, maps[1] + 300, maps[1])
        maps[2] = maps[2] + 254
    if name == 'a9frame':               # boundaries that touch all four borders, and one in the last column alone
        m = maps[4]
        top = int(m.max())
        if min(h, w) == 1:              # a single row or column: its two end pixels (a full frame would make it constant)
            m[0, 0], m[h - 1, w - 1] = top + 1, top + 2
        else:
            m[0, :], m[h - 1, :], m[1:h - 1, 0], m[1:h - 1, w - 1] = top + 1, top + 2, top + 3, top + 4
        maps[7][h - 1, w - 1] = int(maps[7].max()) + 1
    if name == 'a3const':               # one annotator without a boundary: metrics.py:72 divides by zero
        maps[1] = np.full((h, w), 3)
    return np.stack(maps).astype(np.uint16)


def run(lab, segs):
    try:
        m = metrics(None, lab, segs)
        m.set_metrics()
        return {k: float(v) for k, v in m.get_metrics().items()}
    except Exception as e:              # recorded, not hidden: the mirror and the GPU scorer must raise the same
        return {'raises': type(e).__name__}


def save_npz(path, arrays):
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), version=(1, 0))
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


golden_dir = sys.argv[1]
rng = np.random.default_rng(20261016)
arrays, res = {}, {}
for si, (h, w) in enumerate(SHAPES):
    tag = '%dx%d' % (h, w)
    for s in STACKS + ['a3const']:
        arrays['truth_%s_%s' % (tag, s)] = stack(s, h, w, rng)
    for ki, kind in enumerate(KINDS):
        lab = np.asarray(label_map(kind, h, w, rng)).astype(np.uint16)
        arrays['lab_%s_%s' % (tag, kind)] = lab
        s = STACKS[(si + ki) % 3]
        res['%s/%s/%s' % (tag, kind, s)] = run(lab, list(arrays['truth_%s_%s' % (tag, s)]))
    # every stack size under the noise map, a constant annotator map, and no annotators at all
    noise = arrays['lab_%s_noise3' % tag]
    for s in STACKS + ['a3const']:
        res.setdefault('%s/noise3/%s' % (tag, s), run(noise, list(arrays['truth_%s_%s' % (tag, s)])))
    res['%s/noise3/a0' % tag] = run(noise, [])
for k in sorted(res):
    print(k, res[k])
save_npz(golden_dir + '/scoring_edge_maps.npz', arrays)
json.dump(res, open(golden_dir + '/scoring_edge_golden.json', 'w'), indent=1, sort_keys=True)
print(len(res), 'cases,', sum('raises' in v for v in res.values()), 'raising')
