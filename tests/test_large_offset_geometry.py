"""The size limits of the feature slab, just below and just above each bound include/gcs.h states, and the geometry of the batches
of tests/test_gpu_large_offsets.py. Host functions only: nothing is launched, and no pointer is dereferenced (a refused call returns
before its first launch; what a call ACCEPTS is asked of the host-only hooks gcs_selftest_pass_nt_limit and gcs_selftest_gabor_plan,
which run the entry points' own checks)."""
import ctypes as C

import pytest

import large_offsets as lo
from gabor_color_image_segmentation_amd import _lib
from slab_layout import tile_geometry


@pytest.fixture(scope="module")
def lib(built):
    return _lib.load()


def test_batches_cross_both_lines_inside_every_limit(lib):
    """tests/large_offsets.py: batch_geometry's own assertions for every bank of the GPU file (the slab crosses 2^31 and 2^32, an
    image straddles each line, three different base images around it, B <= 65535, kp_batch_fits, Gabor's 2^47) and the counts."""
    counts = {bank_id: lo.batch_geometry(lib, ns, no)[1] for bank_id, (ns, no, _ks, _shift) in lo.BANKS.items()}
    assert counts == {"split_4x6": 4576, "wide_3x9": 3391, "deep_8x8": 2888, "generic_7x10": 2324}, counts
    for ns, no in ((4, 5 + 1), (8, 7 + 1)):                                        # the banks with a coordinate slot
        lo.batch_geometry(lib, ns, no)
    for bank_id, (ns, no, _ks, _shift) in lo.BANKS.items():
        for k in (4, 8, 13, 16):
            for n_sets in (1, counts[bank_id]):
                assert lib.gcs_selftest_pass_nt_limit(counts[bank_id], lo.H, lo.W, ns, no, k, n_sets) >= 0, (bank_id, k, n_sets)
        assert lib.gcs_selftest_gabor_plan(counts[bank_id], lo.H, lo.W, ns, no, 13, 7, 256, 1, None, 0) > 0, bank_id


def test_split_image_limit_of_the_size_functions(lib):
    """A split image above 2^32 - 1 bytes: both size functions return 0; eight rows below the first refused height at W = 1000:
    the exact product, within 1 MiB of 2^32. 4x6 takes 47 001 x 1002 (0.987 x 2^32); 30 001 x 1002 on 2x13 is 1.09 x 2^32."""
    f, g = lib.gcs_feature_slab_bytes, lib.gcs_feature_pass_bytes

    def restated(h, w, ns, no):
        """(img_bytes, what gcs_make_layout holds against 2^32 - 1) of a shape that packs no strip: ntiles * 2 S + the flag words,
        rounded up to 256 bytes / plus 256 (csrc/common.h)."""
        assert h % 8 not in (1, 2) and w % 8 not in (1, 2)
        ntiles = -(-(-(-h // 8) * -(-w // 8)) // 4)
        s = sum(-(-3 * min(2, ns - 2 * L) * no * (256 >> 2 * L) // 32) * 32 for L in range((ns + 1) // 2))
        return ntiles * 2 * s + -(-4 * ntiles // 256) * 256, ntiles * 2 * s + 4 * ntiles + 256

    for ns, no in ((2, 13), (4, 6), (2, 3)):
        h_hi = next(h for h in range(8, 1 << 22, 8) if restated(h, 1000, ns, no)[1] > 0xffffffff)
        below, held = restated(h_hi - 8, 1000, ns, no)
        assert 0xffffffff - (1 << 20) < below <= held <= 0xffffffff, (ns, no, h_hi)
        assert f(1, h_hi - 8, 1000, ns, no) == below and g(1, h_hi - 8, 1000, ns, no) * 4 < below * 3, (ns, no, h_hi)
        assert f(1, h_hi, 1000, ns, no) == 0 and g(1, h_hi, 1000, ns, no) == 0, (ns, no, h_hi)
        assert lib.gcs_selftest_pass_kernel(h_hi - 8, 1000, ns, no, 8) is not None
        assert lib.gcs_selftest_pass_kernel(h_hi, 1000, ns, no, 8) is None
    assert f(1, 30001, 1002, 2, 13) == 0 and g(1, 30001, 1002, 2, 13) == 0
    assert f(1, 47001, 1002, 4, 6) == 4239381760 < 1 << 32
    assert f(1, 47001 + 800, 1002, 4, 6) == 0
    # the wide slab has no such bound in the size functions, and batches multiply in 64 bits
    assert f(1, 30001, 1002, 8, 8) == 3856644480 and f(1, 34001, 1002, 8, 8) > 1 << 32
    assert f(3, 47001, 1002, 4, 6) == 3 * 4239381760
    assert f(65535, 2048, 2048, 8, 8) == 65535 * f(1, 2048, 2048, 8, 8) > 1 << 44
    # every slab entry point refuses the shape the size functions refuse (fake pointers: the calls return before any launch)
    p = C.c_void_p(4096)
    assert lib.gcs_kmeans_assign_accumulate(p, p, 1, 30001, 1002, 2, 13, 8, 1, 0, 30001, 0, p, p, None) != 0
    assert lib.gcs_gabor_features(p, 1, 30001, 1002, p, p, 2, 13, 13, 7, p, p, None) != 0
    assert lib.gcs_features_unpack(p, 1, 30001, 1002, 2, 13, p, None) != 0
    assert lib.gcs_selftest_pass_kernel(30001, 1002, 2, 13, 8) is None


def test_gabor_one_image_below_4_gib(lib):
    """gcs_gabor_features: a wide-slab image of more than 2^32 - 1 bytes is refused by name, the largest one below is planned."""
    p = C.c_void_p(4096)
    f = lib.gcs_feature_slab_bytes
    h_hi = next(h for h in range(30008, 40000, 8) if f(1, h, 1002, 8, 8) > 0xffffffff)
    h_lo = h_hi - 8
    assert 0xffffffff - (1 << 20) < f(1, h_lo, 1002, 8, 8) <= 0xffffffff
    assert lib.gcs_selftest_gabor_plan(1, h_lo, 1002, 8, 8, 13, 7, 256, 1, None, 0) > 0
    assert lib.gcs_selftest_gabor_plan(1, h_hi, 1002, 8, 8, 13, 7, 256, 1, None, 0) == -1
    assert lib.gcs_gabor_features(p, 1, h_hi, 1002, p, p, 8, 8, 13, 7, p, p, None) != 0
    assert lib.gcs_last_error().decode() == "gcs_gabor_features: one image's feature slab must stay below 4 GiB"
    # the split image of part 2 of the GPU file is inside: 47 001 x 1002 on 4x6
    assert lib.gcs_selftest_gabor_plan(1, 47001, 1002, 4, 6, 13, 7, 256, 1, None, 0) > 0
    # B * img_bytes: refused from 2^47 on, B from 65 536 on
    per = f(1, 30001, 1002, 8, 8)
    b_hi = -(-(1 << 47) // per)
    assert b_hi <= 65535 and (b_hi - 1) * per <= 0x7fffffffffff < b_hi * per
    assert lib.gcs_selftest_gabor_plan(b_hi - 1, 30001, 1002, 8, 8, 13, 7, 256, 1, None, 0) > 0
    assert lib.gcs_gabor_features(p, b_hi, 30001, 1002, p, p, 8, 8, 13, 7, p, p, None) != 0
    assert lib.gcs_last_error().decode() == "gcs_gabor_features: slab too large"
    assert lib.gcs_gabor_features(p, 65536, 8, 8, p, p, 4, 6, 13, 7, p, p, None) != 0
    assert lib.gcs_last_error().decode() == "gcs_gabor_features: B too large for one launch"


def test_pass_batch_limit_is_at_2_to_29_tiles(lib):
    """kp_batch_fits: B * ntiles <= 2^29 - 1. 2048 x 2048 has 16 384 tiles on every bank: 32 767 images fit, 32 768 do not (the
    messages: tests/test_pass_kernel_choice.py)."""
    for ns, no in ((4, 6), (8, 8), (7, 10)):
        assert tile_geometry(lib, 2048, 2048, ns, no)[0] == 16384
        for n_sets in (1, "B"):
            assert lib.gcs_selftest_pass_nt_limit(32767, 2048, 2048, ns, no, 8, 32767 if n_sets == "B" else 1) >= 0
            assert lib.gcs_selftest_pass_nt_limit(32768, 2048, 2048, ns, no, 8, 32768 if n_sets == "B" else 1) == -1
    assert 32767 * 16384 <= 0x1fffffff < 32768 * 16384
