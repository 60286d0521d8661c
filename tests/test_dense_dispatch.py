"""Which S1 kernel a shape gets, and the sizes that follow from it, pinned as a table (no GPU memory is touched and
nothing is launched: the selection entry points are host arithmetic on the image shape and the CU count, which
falls back to the MI355X's 256 when there is no device, so the answers are the same with and without one).

The table was recorded from the library before the S1 selection became one function (s1_select) and the timing
arms, the alternative K-loops and the row-segment weight gradient k_wgrad_s1 were removed."""
import pytest

from robustpointclouds_amd import _ffi

S1 = 0
RPC_ERR_ARG = 1
# (B, H, W, ci, cout) -> rpc_dense_conv_s1_kernel, rpc_dense_conv_part_rows, rpc_dense_conv_blocks,
# rpc_dense_wgrad_workspace_size; kernels: 0 = k_conv3x3, 1 = k_conv3x3w, 2 = k_conv3x3x, 3 = k_conv3x3y
TABLE = [
    # the metric's SECOND layers
    ((6, 200, 176, 128, 128), 3, 858, 858, 75497472),
    ((6, 200, 176, 128, 256), 3, 858, 858, 99090432),
    ((6, 100, 88, 256, 256), 2, 126, 252, 75497472),
    # CenterPoint's
    ((4, 128, 128, 64, 64), 0, 256, 256, 12533760),
    ((4, 128, 128, 128, 128), 1, 256, 256, 73138176),
    ((4, 64, 64, 64, 64), 0, 64, 64, 12533760),
    ((4, 64, 64, 128, 128), 0, 64, 64, 62521344),
    # the S1 shapes of tests/test_gpu_dense_bev.py (cout % 128 != 0: 64, 320, 192)
    ((2, 20, 18, 128, 128), 0, 8, 8, 50135040),
    ((2, 9, 14, 256, 128), 0, 2, 2, 49545216),
    ((2, 16, 10, 128, 256), 0, 2, 2, 49545216),
    ((2, 24, 20, 128, 128), 0, 8, 8, 50135040),
    ((2, 12, 10, 256, 128), 0, 2, 2, 49545216),
    ((1, 200, 176, 128, 128), 0, 143, 143, 74317824),
    ((2, 37, 45, 256, 128), 0, 18, 18, 61341696),
    ((1, 100, 88, 256, 256), 0, 42, 42, 70778880),
    ((2, 33, 17, 128, 256), 0, 12, 12, 49545216),
    ((1, 16, 16, 512, 128), 0, 1, 1, 49545216),
    ((2, 37, 45, 320, 64), 0, 18, 18, 12533760),
    ((1, 40, 24, 64, 320), 0, 6, 6, 12533760),
    ((2, 17, 33, 64, 192), 0, 12, 12, 12386304),
    ((1, 64, 64, 256, 256), 0, 16, 16, 66060288),
    ((2, 200, 176, 256, 128), 2, 156, 286, 75497472),
    ((2, 100, 88, 256, 256), 0, 84, 84, 75497472),
    ((1, 16, 32, 128, 128), 0, 2, 2, 50135040),
    ((3, 24, 40, 128, 128), 0, 18, 18, 50135040),
    ((1, 9, 130, 128, 256), 0, 9, 9, 64880640),
    ((1, 21, 70, 384, 128), 0, 10, 10, 63700992),
    ((1, 19, 33, 192, 128), 0, 6, 6, 37158912),
    ((6, 200, 176, 256, 128), 3, 858, 858, 99090432),
    ((2, 200, 176, 128, 128), 2, 156, 286, 74317824),
    ((3, 200, 176, 128, 256), 3, 429, 429, 75497472),
    ((4, 128, 144, 128, 128), 2, 160, 288, 73728000),
    ((2, 24, 40, 128, 128), 0, 12, 12, 61341696),
    ((2, 17, 70, 128, 128), 0, 20, 20, 67239936),
    ((1, 5, 130, 128, 256), 0, 9, 9, 49545216),
    ((1, 37, 45, 256, 128), 0, 9, 9, 49545216),
    ((2, 17, 70, 64, 128), 0, 20, 20, 33619968),
    ((1, 5, 130, 192, 256), 0, 9, 9, 61931520),
    ((3, 1, 33, 128, 128), 0, 9, 9, 50135040),
    # either side of the thresholds on 256 CUs — small grids (2 x the 16x32 blocks <= CUs: 128 above / 160 here)
    ((4, 128, 129, 128, 128), 2, 160, 288, 73728000),
    # ... whole rounds filled to >= 90 % (231 blocks of 256 / 230)
    ((3, 112, 176, 128, 128), 1, 231, 231, 74317824),
    ((2, 80, 368, 128, 128), 0, 230, 230, 74317824),
    # ... more than one round of the 2 x CUs slots of the 16x16 blocks (512 / 544)
    ((1, 256, 256, 128, 256), 2, 128, 256, 75497472),
    ((1, 256, 257, 128, 256), 3, 272, 272, 74317824),
]
# the knobs that enter the selection and the workspace size, and their defaults (the RPC_DENSE_* variables set them)
DEFAULTS = {0: 0, 1: 0, 5: 0, 6: 0}


@pytest.fixture()
def lib():
    lib = _ffi.load()
    old = {k: lib.rpc_dense_tune(k, v) for k, v in DEFAULTS.items()}
    yield lib
    for k, v in old.items():
        lib.rpc_dense_tune(k, v)


def test_every_kernel_is_in_the_table():
    assert {row[1] for row in TABLE} == {0, 1, 2, 3}


@pytest.mark.parametrize("shape,kernel,part_rows,blocks,wgrad_ws", TABLE)
def test_s1_dispatch_table(lib, shape, kernel, part_rows, blocks, wgrad_ws):
    B, H, W, ci, cout = shape
    img = _ffi.int_arr((B, H, W))
    assert lib.rpc_dense_conv_s1_kernel(S1, cout, img) == kernel
    assert lib.rpc_dense_conv_part_rows(S1, cout, img) == part_rows
    assert lib.rpc_dense_conv_blocks(S1, img) == blocks
    assert lib.rpc_dense_wgrad_workspace_size(S1, img, ci, cout) == wgrad_ws


def test_removed_knobs_are_unknown(lib):
    for knob in (4, 7):   # the timing arms of k_conv3x3x / y and of k_wgrad_s1c
        assert lib.rpc_dense_tune(knob, -1) == RPC_ERR_ARG


@pytest.mark.parametrize("before", [0, 1, 3])
def test_removed_wgrad_variants_leave_knob_1_unchanged(lib, before):
    lib.rpc_dense_tune(1, before)
    for removed in (4, 2):
        assert lib.rpc_dense_tune(1, removed) == before
        assert lib.rpc_dense_tune(1, -1) == before
