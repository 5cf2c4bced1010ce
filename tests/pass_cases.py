"""The (bank, k) pairs that select every Lloyd-pass instantiation of the default build, and the largest smoothing K, shared by the
stage tests on hot banks (tests/test_gpu_value_range.py) and on crafted slabs (tests/test_gpu_crafted_slabs.py)."""
K_MAX = 4.525483399593902          # the largest smoothing K a bank accepts: radius 24 on the odd scales

# (n_scales, n_orient, ksize, shift, k): every pair of test_segment_small_and_ragged_feature_counts, the 4x6 / 2x6 pairs, the
# D = 210 bank, and one pair for each remaining instantiation. id = the arm of lloyd_pass the pair selects (split<KT,NR[,2]>:
# kmeans_pass_mfma_kernel on the split slab; narrow / wide<KT,NST>: the same kernel on the wide slab with 5 / 13 K-steps; wide8w:
# its 8-wave form; native<NL,MINB,N0>: kmeans_pass_native_kernel; generic: kmeans_assign_kernel).
PASS_CASES = [
    ((1, 1, 15, 7, 3), "split<1,3>_D3"), ((1, 4, 9, 7, 5), "split<1,3>_D12"), ((2, 5, 11, 7, 8), "split<1,3>_D30"),
    ((3, 8, 15, 7, 16), "split<2,5>_D72_3x8"), ((2, 13, 7, 7, 4), "split<1,5>_D78"), ((3, 9, 15, 7, 4), "wide8w<1,5>_D81"),
    ((1, 43, 11, 7, 5), "wide<1,18>_D129"), ((8, 8, 15, 7, 8), "native<4,3,6>_D192"), ((8, 8, 15, 8, 13), "wide<2,10>_D192"),
    ((3, 23, 9, 7, 16), "wide<2,26>_D207"), ((3, 23, 9, 8, 7), "wide<1,26>_D207"), ((6, 8, 15, 7, 8), "native<3,3,6>_D144"),
    ((5, 8, 13, 7, 7), "native<3,3,6>_D120"), ((8, 6, 13, 7, 8), "native<4,2,0>_D144"), ((7, 6, 11, 7, 6), "native<4,2,0>_D126"),
    ((4, 6, 13, 7, 8), "split<1,3,2>_D72"), ((4, 6, 13, 7, 16), "split<2,5>_D72"), ((4, 6, 13, 8, 8), "split<1,3,2>_D72_shift8"),
    ((2, 6, 13, 7, 8), "split<1,3,2>_D36"), ((7, 10, 13, 7, 4), "generic_D210_k4"), ((7, 10, 13, 8, 16), "generic_D210_k16"),
    ((5, 1, 13, 7, 3), "narrow<1,3>_D15"), ((5, 5, 13, 7, 8), "narrow<1,6>_D75"), ((6, 4, 13, 7, 12), "narrow<2,6>_D72"),
    ((4, 7, 13, 7, 8), "native<2,3,0>_D84"), ((4, 8, 13, 7, 8), "native<2,3,6>_D96"), ((5, 6, 13, 7, 8), "native<3,3,0>_D90"),
    ((1, 43, 11, 7, 12), "wide<2,18>_D129"),
]
