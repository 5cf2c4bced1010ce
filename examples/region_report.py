#!/usr/bin/env python3
"""Region descriptors and mean-colour pictures of the cuts of one image's region tree (SPEC.md §19).

    python examples/region_report.py [--regions 4,8,16] [--image ID] [--superpixels 300] [--tree-nodes components] [--out DIR]

Takes one val fixture image (tests/golden/bsd_val_images.npz), builds the region tree once (colour bank, n superpixels), makes the
table of its leaves in one pass over the pixels, the table of every requested cut from that table alone, prints them and writes
``regions_<R>.npy`` - the (H,W,3) uint8 picture of each cut in its regions' mean colours - and ``leaves.npy`` into DIR. Needs a
GPU; needs no image library (``numpy.load`` reads the pictures back)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BANK = dict(n_orient=5, color_weight=0.125, chroma_gain=4)


def print_table(title, t):
    print(title)
    print("  region    area   centroid (y, x)     bbox (y0, x0, y1, x1)    mean RGB")
    for q in np.flatnonzero(t["used"]):
        cy, cx = t["centroid"][q]
        print("  %6d %7d   %7.1f %7.1f     %4d %4d %4d %4d      %3d %3d %3d" % ((q, t["area"][q], cy, cx) + tuple(t["bbox"][q])
                                                                                + tuple(t["mean_rgb"][q])))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--regions", default="4,8,16")
    ap.add_argument("--image", default=None, help="id of a val fixture image (default: the first)")
    ap.add_argument("--superpixels", type=int, default=300)
    ap.add_argument("--tree-nodes", default="components", choices=["components", "superpixels"])
    ap.add_argument("--out", default="region_report")
    args = ap.parse_args()
    regions = [int(r) for r in args.regions.split(",")]
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, region_table
    val = np.load(os.path.join(ROOT, "tests", "golden", "bsd_val_images.npz"))
    name = args.image or str(val["ids"][0])
    img = val["img_" + name]
    seg = Segmenter(n_superpixels=args.superpixels, tree_nodes=args.tree_nodes, **BANK)
    imgs = torch.from_numpy(img[None].copy()).to(seg.ops.device)
    labels, merges, _, alive = seg.region_tree_device(imgs)
    K = merges.shape[1] + 1
    sums, bbox = seg.region_props_device(imgs, labels, K=K)                     # one pass over the pixels
    group, cut_sums, cut_bbox, offsets = seg.cut_props_device(sums, bbox, merges, alive, regions, shape=img.shape[:2])
    os.makedirs(args.out, exist_ok=True)
    print("image %s, %d x %d, %d leaves of the tree (K = %d)" % ((name,) + img.shape[:2] + (int(alive[0]), K)))
    np.save(os.path.join(args.out, "leaves.npy"), seg.paint_device(labels, sums)[0].cpu().numpy())
    for j, r in enumerate(regions):
        rows = slice(offsets[j], offsets[j] + min(K, r))
        print_table("cut at R = %d" % r, region_table(cut_sums[0, rows].cpu().numpy(), cut_bbox[0, rows].cpu().numpy()))
        picture = seg.paint_device(labels, cut_sums[:, rows], group[j])[0].cpu().numpy()
        np.save(os.path.join(args.out, "regions_%d.npy" % r), picture)
    print("pictures: %s/leaves.npy, %s" % (args.out, ", ".join("regions_%d.npy" % r for r in regions)))


if __name__ == "__main__":
    main()
