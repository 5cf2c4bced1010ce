// regions.hip — label-map post-processing kernels of libgcs.so (gfx950): connected regions (SPEC.md §7) and the small-region merge
// (SPEC.md §9), the Segmenter's connectivity / min_region_size steps. Nothing here allocates, frees or synchronises; every entry
// point enqueues on the caller's stream.
#include "region_kernels.h"

extern "C" size_t gcs_connected_scratch_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)2 * B * H * W * sizeof(int32_t);
}

extern "C" int gcs_connected_regions(const int32_t *labels, int B, int H, int W, void *scratch, int32_t *out,
                                     gcs_stream_t stream) {
    if (!labels || !scratch || !out) return gcs_fail(GCS_EINVAL, "gcs_connected_regions: NULL pointer");
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL)
        return gcs_fail(GCS_EINVAL, "gcs_connected_regions: bad shape");
    const int P = H * W;
    int *parent = static_cast<int *>(scratch);
    int *rootid = parent + (size_t)B * P;
    const dim3 grid(min(1024, (P + 255) / 256), B), block(256);
    hipLaunchKernelGGL(cc_local_init_kernel, grid, block, 0, stream, H, W, parent);
    GCS_CHECK_LAUNCH("gcs_connected_regions(init)");
    hipLaunchKernelGGL(cc_union_kernel, grid, block, 0, stream, labels, H, W, parent);
    GCS_CHECK_LAUNCH("gcs_connected_regions(union)");
    hipLaunchKernelGGL(cc_rank_kernel, dim3(B), dim3(1024), 0, stream, H, W, parent, rootid);
    GCS_CHECK_LAUNCH("gcs_connected_regions(rank)");
    hipLaunchKernelGGL(cc_relabel_kernel, grid, block, 0, stream, H, W, parent, rootid, out);
    GCS_CHECK_LAUNCH("gcs_connected_regions");
    return GCS_OK;
}


extern "C" size_t gcs_merge_scratch_bytes(int B, int H, int W, int min_size) {
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || min_size < 0) return 0;
    // best (u64) | parent | rootid | size per pixel, then one flag per (round, image)
    return (size_t)B * H * W * (sizeof(unsigned long long) + 3 * sizeof(int32_t)) + (size_t)32 * B * sizeof(int32_t);
}

extern "C" int gcs_merge_small_regions(const int32_t *labels, int B, int H, int W, int min_size, void *scratch, int32_t *out,
                                       gcs_stream_t stream) {
    if (!labels || !scratch || !out) return gcs_fail(GCS_EINVAL, "gcs_merge_small_regions: NULL pointer");
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL)
        return gcs_fail(GCS_EINVAL, "gcs_merge_small_regions: bad shape");
    if (min_size < 0) return gcs_fail(GCS_EINVAL, "gcs_merge_small_regions: min_size < 0");
    if (static_cast<const void *>(labels) == static_cast<const void *>(out))
        return gcs_fail(GCS_EINVAL, "gcs_merge_small_regions: out may not alias labels");
    const int P = H * W;
    const size_t n = (size_t)B * P;
    unsigned long long *best = static_cast<unsigned long long *>(scratch);
    int *parent = reinterpret_cast<int *>(best + n);
    int *rootid = parent + n;
    unsigned *size = reinterpret_cast<unsigned *>(rootid + n);
    int *act = reinterpret_cast<int *>(size + n);
    // every round at least halves the absorbable regions (SPEC.md §9): floor(log2(P)) + 1 rounds suffice; none for m <= 1
    int n_rounds = 0;
    if (min_size > 1)
        for (unsigned v = (unsigned)P; v; v >>= 1) ++n_rounds;
    const dim3 grid(min(1024, (P + 255) / 256), B), block(256);
    hipLaunchKernelGGL(mr_init_kernel, grid, block, 0, stream, H, W, B, n_rounds, parent, size, best, act);
    GCS_CHECK_LAUNCH("gcs_merge_small_regions(init)");
    hipLaunchKernelGGL(cc_union_kernel, grid, block, 0, stream, labels, H, W, parent);
    GCS_CHECK_LAUNCH("gcs_merge_small_regions(union)");
    if (n_rounds > 0) {
        hipLaunchKernelGGL(mr_flatten_kernel, grid, block, 0, stream, H, W, B, -1, parent, act);
        GCS_CHECK_LAUNCH("gcs_merge_small_regions(flatten)");
    }
    for (int r = 0; r < n_rounds; ++r) {
        hipLaunchKernelGGL(mr_size_kernel, grid, block, 0, stream, H, W, B, r, parent, size, act);
        GCS_CHECK_LAUNCH("gcs_merge_small_regions(size)");
        hipLaunchKernelGGL(mr_best_kernel, grid, block, 0, stream, H, W, B, r, (unsigned)min_size, parent, size, best, act);
        GCS_CHECK_LAUNCH("gcs_merge_small_regions(best)");
        hipLaunchKernelGGL(mr_union_kernel, grid, block, 0, stream, H, W, B, r, parent, size, best, act);
        GCS_CHECK_LAUNCH("gcs_merge_small_regions(merge)");
        hipLaunchKernelGGL(mr_flatten_kernel, grid, block, 0, stream, H, W, B, r, parent, act);
        GCS_CHECK_LAUNCH("gcs_merge_small_regions(flatten)");
    }
    hipLaunchKernelGGL(cc_rank_kernel, dim3(B), dim3(1024), 0, stream, H, W, parent, rootid);
    GCS_CHECK_LAUNCH("gcs_merge_small_regions(rank)");
    hipLaunchKernelGGL(cc_relabel_kernel, grid, block, 0, stream, H, W, parent, rootid, out);
    GCS_CHECK_LAUNCH("gcs_merge_small_regions");
    return GCS_OK;
}
