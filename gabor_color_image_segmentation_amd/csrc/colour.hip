// colour.hip — SPEC.md §11: the opponent-colour transform T_g in front of the Gabor stage (gfx950 only).
//
// One launch of a pure streaming kernel: interleaved RGB bytes in, interleaved (Y, Co, Cg) bytes out, 3 B read and 3 B written
// per pixel. A lane owns a CHUNK of 16 whole pixels = 48 bytes = three 16-byte loads and three 16-byte stores. 3 is invertible
// modulo 16 (3 * 11 = 33), so for any destination address there is a head of p0 = (5 * (out & 15)) & 15 pixels after which
// out + 3 p0 is a multiple of 16: every chunk store is then an aligned global_store_dwordx4 (a 128-byte line is written by at most
// three lanes of one wave and never torn between two stores). The source keeps whatever alignment it has relative to that - image
// rows are 3 bytes wide and a 481x321 image is 463 203 bytes, so sub-batch pointers arrive at any byte - and is read with
// byte-aligned 16-byte loads (global_load_dwordx4 takes any address in the unaligned access mode HSA code objects run in). The
// p0 head pixels and the (n - p0) & 15 tail pixels are done one per lane with byte loads and stores by the lanes behind the last
// chunk, in the same launch. Nothing outside [0, 3 n) of either buffer is read or written.
#include "common.h"

namespace {

constexpr int CO_CHUNK_PX = 16;              // pixels per lane
constexpr int CO_THREADS = 256;

// T_g of one pixel -> Y | Co << 8 | Cg << 16.  128 + (x >> 1) == (x + 256) >> 1 and 128 + (x >> 2) == (x + 512) >> 2 (floor shifts,
// the added terms are multiples of the divisor); |g (2G - R - B)| <= 16 * 510: everything stays far inside 32 bits.
__device__ __forceinline__ unsigned co_pixel(int R, int G, int B, int gain) {
    const int y = (R + 2 * G + B + 2) >> 2;
    const int co = min(max((__mul24(gain, R - B) + 256) >> 1, 0), 255);
    const int cg = min(max((__mul24(gain, 2 * G - R - B) + 512) >> 2, 0), 255);
    return (unsigned)y | (unsigned)co << 8 | (unsigned)cg << 16;
}

__global__ __launch_bounds__(CO_THREADS) void colour_opponent_kernel(const unsigned char *__restrict__ src,
                                                                     unsigned char *__restrict__ dst, size_t n_pixels,
                                                                     unsigned head, size_t n_chunks, int gain) {
    const size_t t = (size_t)blockIdx.x * CO_THREADS + threadIdx.x;
    if (t < n_chunks) {
        const size_t byte0 = 3 * ((size_t)head + CO_CHUNK_PX * t);       // dst + byte0 is 16-byte aligned
        unsigned w[12];
        __builtin_memcpy(w, src + byte0, 48);                             // three 16-byte loads at the source's own alignment
        unsigned o[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) o[i] = 0u;
#pragma unroll
        for (int p = 0; p < CO_CHUNK_PX; ++p) {
            int c[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] = (int)(w[(3 * p + j) >> 2] >> (8 * ((3 * p + j) & 3)) & 255u);
            const unsigned v = co_pixel(c[0], c[1], c[2], gain);
#pragma unroll
            for (int j = 0; j < 3; ++j) o[(3 * p + j) >> 2] |= (v >> (8 * j) & 255u) << (8 * ((3 * p + j) & 3));
        }
        v4i *out = reinterpret_cast<v4i *>(dst + byte0);
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = v4i{(int)o[4 * i], (int)o[4 * i + 1], (int)o[4 * i + 2], (int)o[4 * i + 3]};
        return;
    }
    // head pixels [0, head) and tail pixels [head + 16 n_chunks, n_pixels): at most 15 + 15 lanes
    size_t p = t - n_chunks;
    if (p >= head) p += CO_CHUNK_PX * n_chunks;
    if (p >= n_pixels) return;
    const unsigned v = co_pixel(src[3 * p], src[3 * p + 1], src[3 * p + 2], gain);
    dst[3 * p] = (unsigned char)v;
    dst[3 * p + 1] = (unsigned char)(v >> 8);
    dst[3 * p + 2] = (unsigned char)(v >> 16);
}

}  // namespace

extern "C" int gcs_colour_opponent(const uint8_t *img, size_t n_pixels, int gain, uint8_t *out, gcs_stream_t stream) {
    if (!img || !out) return gcs_fail(GCS_EINVAL, "gcs_colour_opponent: NULL pointer");
    if (gain < 1 || gain > 16) return gcs_fail(GCS_EINVAL, "gcs_colour_opponent: gain must be in 1..16");
    if (n_pixels == 0 || n_pixels > ((size_t)1 << 40)) return gcs_fail(GCS_EINVAL, "gcs_colour_opponent: n_pixels must be in 1..2^40");
    const uintptr_t a = reinterpret_cast<uintptr_t>(img), b = reinterpret_cast<uintptr_t>(out), bytes = 3 * n_pixels;
    if (a < b + bytes && b < a + bytes) return gcs_fail(GCS_EINVAL, "gcs_colour_opponent: out overlaps img");
    size_t head = (5 * (b & 15)) & 15;                                    // b + 3 head = b + 15 (b & 15) = 0 (mod 16)
    if (head > n_pixels) head = n_pixels;
    const size_t n_chunks = (n_pixels - head) / CO_CHUNK_PX;
    const size_t items = n_chunks + head + (n_pixels - head - CO_CHUNK_PX * n_chunks);
    const size_t blocks = (items + CO_THREADS - 1) / CO_THREADS;
    if (blocks > 0x7fffffffULL) return gcs_fail(GCS_EINVAL, "gcs_colour_opponent: n_pixels too large for one launch");
    hipLaunchKernelGGL(colour_opponent_kernel, dim3((unsigned)blocks), dim3(CO_THREADS), 0, stream, img, out, n_pixels,
                       (unsigned)head, n_chunks, gain);
    GCS_CHECK_LAUNCH("gcs_colour_opponent");
    return GCS_OK;
}
