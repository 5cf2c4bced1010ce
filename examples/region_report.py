#!/usr/bin/env python3
"""Region descriptors and mean-colour pictures of the cuts of one image's region tree (SPEC.md §19), and which regions touch (§20).

    python examples/region_report.py [--regions 4,8,16] [--image ID] [--superpixels 300] [--tree-nodes components] [--out DIR]
                                     [--adjacency]

Takes one val fixture image (tests/golden/bsd_val_images.npz), builds the region tree once (colour bank, n superpixels), makes the
table of its leaves in one pass over the pixels, the table of every requested cut from that table alone, prints them and writes
``regions_<R>.npy`` - the (H,W,3) uint8 picture of each cut in its regions' mean colours - and ``leaves.npy`` into DIR. Needs a
GPU; needs no image library (``numpy.load`` reads the pictures back). ``--adjacency``: the region adjacency graph of the leaves in
the same way (one more pass over the pixels, with the tree's contour map as the strength plane), the graph of every requested cut from
the leaf graph alone, and per cut its edges with boundary length, mean colour contrast and mean contour level."""
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


def print_edges(t):
    print("  edge (a, b)    length   mean contrast   mean contour level")
    for (a, b), n, c, u in zip(t["pairs"], t["length"], t["mean_contrast"], t["mean_strength"]):
        print("  %5d %5d  %8d   %13.1f   %18.2f" % (a, b, n, c, u))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--regions", default="4,8,16")
    ap.add_argument("--image", default=None, help="id of a val fixture image (default: the first)")
    ap.add_argument("--superpixels", type=int, default=300)
    ap.add_argument("--tree-nodes", default="components", choices=["components", "superpixels"])
    ap.add_argument("--out", default="region_report")
    ap.add_argument("--adjacency", action="store_true", help="print the edges of every cut (SPEC.md §20)")
    args = ap.parse_args()
    regions = [int(r) for r in args.regions.split(",")]
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, adjacency_table, region_table
    val = np.load(os.path.join(ROOT, "tests", "golden", "bsd_val_images.npz"))
    name = args.image or str(val["ids"][0])
    img = val["img_" + name]
    seg = Segmenter(n_superpixels=args.superpixels, tree_nodes=args.tree_nodes, **BANK)
    imgs = torch.from_numpy(img[None].copy()).to(seg.ops.device)
    labels, merges, _, alive = seg.region_tree_device(imgs)
    K = merges.shape[1] + 1
    sums, bbox = seg.region_props_device(imgs, labels, K=K)                     # one pass over the pixels
    group, cut_sums, cut_bbox, offsets = seg.cut_props_device(sums, bbox, merges, alive, regions, shape=img.shape[:2])
    if args.adjacency:
        contours = seg.contour_map_device(labels, merges, alive)
        leaf_graph = seg.region_adjacency_device(labels, K=K, imgs=imgs, strength=contours)     # one more pass over the pixels
        cut_edges, cut_vals, cut_count = seg.cut_adjacency_device(*leaf_graph, group)
    os.makedirs(args.out, exist_ok=True)
    print("image %s, %d x %d, %d leaves of the tree (K = %d)" % ((name,) + img.shape[:2] + (int(alive[0]), K)))
    np.save(os.path.join(args.out, "leaves.npy"), seg.paint_device(labels, sums)[0].cpu().numpy())
    for j, r in enumerate(regions):
        rows = slice(offsets[j], offsets[j] + min(K, r))
        print_table("cut at R = %d" % r, region_table(cut_sums[0, rows].cpu().numpy(), cut_bbox[0, rows].cpu().numpy()))
        if args.adjacency:
            print_edges(adjacency_table(cut_edges[j, 0].cpu().numpy(), cut_vals[j, 0].cpu().numpy(), int(cut_count[j, 0])))
        picture = seg.paint_device(labels, cut_sums[:, rows], group[j])[0].cpu().numpy()
        np.save(os.path.join(args.out, "regions_%d.npy" % r), picture)
    print("pictures: %s/leaves.npy, %s" % (args.out, ", ".join("regions_%d.npy" % r for r in regions)))


if __name__ == "__main__":
    main()
