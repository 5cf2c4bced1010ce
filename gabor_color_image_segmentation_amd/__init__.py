"""MI355X-native Gabor-bank colour segmentation: a drop-in for the segmenter slot at
/root/reference/BSD_metrics/script.py:30 (``labels = segment(img)``)."""
from .bank import GaborBank, make_bank, gabor_taps, smoothing_taps, split_digits  # noqa: F401
from .segmenter import Segmenter, segment, segment_batch, fit_codebook, segment_confidence, segment_images, segment_contours, segment_edges, segment_texton_edges, segment_cue_edges, segment_regions, render_regions, HipOps, lloyd, shard_rows, halo_rows, superpixel_grid, seed_stride  # noqa: F401
from .regions import region_table, adjacency_table  # noqa: F401
from .kmeans_model import KMeansModel  # noqa: F401
from ._lib import GcsError  # noqa: F401
