#!/usr/bin/env python3
"""One codebook for a stream of images: cluster ids that mean the same thing from call to call (SPEC.md §28).

    python examples/codebook_stream.py [--fit 8] [--k 8] [--refine 0] [--init spec|kmeans++] [--n-init 1] [--seed 0] [--save model.npz]

Fits ONE k-means codebook on the first ``--fit`` portrait val fixture images (tests/golden/bsd_val_images.npz, colour bank), then
labels the remaining ones with it, one call per image as a camera loop would: the Gabor stage and a single assign pass instead of
the ten passes of a per-image codebook. Prints the model's per-cluster counts and its mean squared error, and per image the share
of every cluster under the shared codebook, the error of the shared codebook on that image against the error of the image's own
codebook, and the mean confidence of its pixels. ``--save`` keeps the model as an ``.npz`` that ``KMeansModel.load`` reads back.
``--init kmeans++`` seeds every Lloyd loop by k-means++ (SPEC.md §29) instead of evenly spaced raster pixels, and ``--n-init n``
then fits the codebook n times from the seeds ``--seed``, ``--seed + 1``, ... and keeps the fit with the least inertia.
Needs a GPU."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BANK = dict(n_orient=5, color_weight=0.125, chroma_gain=4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fit", type=int, default=8, help="images the codebook is fitted on")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--refine", type=int, default=0, help="update passes per image from the shared codebook (0: frozen)")
    ap.add_argument("--init", default="spec", choices=["spec", "kmeans++"], help="how every Lloyd loop starts (SPEC.md §4 / §29)")
    ap.add_argument("--n-init", type=int, default=1, help="restarts of the fit (with --init kmeans++): the least inertia is kept")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None)
    args = ap.parse_args()
    import torch
    from gabor_color_image_segmentation_amd import KMeansModel, Segmenter
    val = np.load(os.path.join(ROOT, "tests", "golden", "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"] if val["img_" + str(i)].shape[:2] == (481, 321)]
    seg = Segmenter(k=args.k, init=args.init, seed=args.seed, **BANK)
    dev = lambda names: torch.from_numpy(np.stack([val["img_" + i] for i in names])).to(seg.ops.device)
    model = seg.fit_device(dev(ids[:args.fit]), "global", n_init=args.n_init)
    if args.save:
        model.save(args.save)
        model = KMeansModel.load(args.save)
    counts = model.counts.cpu().numpy()[0]
    print("codebook of %d clusters on %d features, fitted on %d images" % (model.k, model.n_features, args.fit))
    print("  pixels per cluster:", counts.tolist())
    print("  mse per feature: %.1f" % model.mse[0])
    print("image     share of every cluster under the shared codebook             mse shared / own   mean confidence")
    for name in ids[args.fit:]:
        img = dev([name])
        labels = seg.predict_device(img, model, refine=args.refine)
        shared = seg.evaluate_device(img, model, labels=False)["stats"].cpu().numpy()[0]
        own = seg.evaluate_device(img, labels=False)["stats"].cpu().numpy()[0]
        _, conf = seg.confidence_device(img, model)
        share = np.bincount(labels.cpu().numpy().ravel(), minlength=model.k) / labels.numel()
        per_feature = lambda st: st[:, 1].sum() / (st[:, 0].sum() * model.n_features)
        print("%-8s  %s   %8.1f / %-8.1f   %.3f" % (name, " ".join("%5.1f%%" % (100 * s) for s in share), per_feature(shared),
                                                   per_feature(own), float(conf.mean())))


if __name__ == "__main__":
    main()
