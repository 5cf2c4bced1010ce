"""SLIC rows of the superpixel quality table: what scikit-image 0.18.3 gives on the 24 val fixture images.

Run under the golden generator's interpreter (the one that has scikit-image 0.18.3; see make_golden.sh) from the repository root:

    <python3.9> -W ignore tests/golden/make_superpixel_slic.py tests/golden

For every image of bsd_val_images.npz and every n_segments of N_SEGMENTS: skimage.segmentation.slic(img, n_segments=n,
compactness=10.0) - the call the slot ships with - scored by the package's mirror of the reference's metrics class
(evaluate.metrics, evaluate.region_agreement) against bsd500_truth.npz. Writes superpixel_slic_scores.json: per n_segments the
mean of every score over the 24 images and the per-image boundary recall, underseg and regions. Only numbers are stored."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
N_SEGMENTS = (300, 360, 420)          # 300: the slot's setting; 360, 420: region counts around those of n_superpixels = 300
KEYS = ("recall", "precision", "fmeasure", "underseg", "undersegNP", "compactness", "density", "PRI", "VoI", "covering", "regions")


def main(out_dir):
    import skimage
    from skimage.segmentation import slic
    from gabor_color_image_segmentation_amd.evaluate import metrics, region_agreement
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    val = np.load(os.path.join(HERE, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(HERE, "bsd500_truth.npz"))
    ids = [str(i) for i in val["ids"]]
    doc = dict(skimage=skimage.__version__, compactness=10.0, ids=ids, rows=[])
    for n in N_SEGMENTS:
        per = []
        for i in ids:
            lab = slic(val["img_" + i], n_segments=n, compactness=10.0)
            m = metrics(None, lab, pt[i])
            m.set_metrics()
            got = m.get_metrics()
            got.update(region_agreement(lab, pt[i]))
            per.append([float(got[k]) for k in KEYS])
        per = np.array(per)
        row = dict(n_segments=n)
        row.update({k: float(v) for k, v in zip(KEYS, per.mean(axis=0))})
        row["per_image"] = {i: dict(recall=p[0], underseg=p[3], regions=p[10]) for i, p in zip(ids, per.tolist())}
        doc["rows"].append(row)
        print(json.dumps({k: row[k] for k in ("n_segments",) + KEYS}), flush=True)
    with open(os.path.join(out_dir, "superpixel_slic_scores.json"), "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
