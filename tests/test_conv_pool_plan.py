"""The resident conv forward's tile plan and the pooled-epilogue predicate
(host arithmetic of ops/csrc/conv_f32.hip; no GPU needed).

conv_fwd_res_plan(C, H, W, OH, OW, R) -> (tile_rows, tiles, mi, lds_rows,
lds_bytes); tile_rows == 0 means a 128-pixel tile that is no whole number
of output rows (the plan every shape had before there was a plan)."""

import pytest

LDS_3_PER_CU = 163840 // 3   # bytes that keep three blocks on a CU
LDS_GUARD = 100 * 1024       # launch_conv_fwd's limit for the resident path
B_BUFFERS = 2 * 32 * 72 * 4  # two BK x (BN + 8) weight buffers


@pytest.fixture(scope='module')
def E():
    from rlr_amd.ops import ext
    return ext()


def _legacy(C, H, W, OH, OW, R):
    """The launcher's arithmetic before the plan existed."""
    tiles = (OH * OW + 127) // 128
    lds_rows = 127 // OW + 2 + R - 1
    xf = (lds_rows * W * (C + 1) + 3) & ~3
    return (0, tiles, 4, lds_rows, xf * 4 + B_BUFFERS)


def test_flagship_conv2_plan(E):
    # 24x24 output: 8 rows = 192 pixels, 3 tiles, 10 input rows
    assert E.conv_fwd_res_plan(32, 26, 26, 24, 24, 3) == \
        (8, 3, 6, 10, 52752)
    assert 10 * 26 * 33 * 4 + B_BUFFERS == 52752 <= LDS_3_PER_CU


def test_whole_row_128_pixel_plan(E):
    # 16x16 output: 192 / 16 = 12 rows does not divide 16, 128 / 16 = 8 does
    assert E.conv_fwd_res_plan(32, 18, 18, 16, 16, 3) == \
        (8, 2, 4, 10, 10 * 18 * 33 * 4 + B_BUFFERS)


@pytest.mark.parametrize('shape', [
    (64, 15, 15, 13, 13, 3),    # CNN_CIFAR conv2
    (128, 6, 6, 4, 4, 3),       # CNN_CIFAR conv3 (below the resident path)
    (32, 14, 14, 12, 12, 3),    # 144 pixels: no exact tile
    (64, 12, 20, 10, 18, 3),    # 180 pixels: no exact tile
    (64, 26, 26, 24, 24, 3),    # exact tile exists but not at 3 blocks / CU
])
def test_other_shapes_keep_the_128_pixel_plan(E, shape):
    assert E.conv_fwd_res_plan(*shape) == _legacy(*shape)


def test_pool_predicate(E):
    ok = E.conv_pool_fused_ok
    assert ok(32, 26, 26, 64, 3, 3, 1, 0)          # flagship conv2
    assert ok(32, 18, 18, 96, 3, 3, 1, 0)          # 128-pixel whole rows
    assert not ok(64, 15, 15, 128, 3, 3, 1, 0)     # CIFAR conv2: 13x13
    assert not ok(32, 15, 15, 64, 3, 3, 1, 0)      # 13x13
    assert not ok(32, 26, 26, 64, 3, 3, 1, 1)      # pad 1
    assert not ok(32, 26, 26, 64, 3, 3, 2, 0)      # stride 2
    assert not ok(32, 14, 14, 64, 3, 3, 1, 0)      # tile is no whole rows
    assert not ok(1, 28, 28, 32, 3, 3, 1, 0)       # the small-C kernel's


def test_plan_invariants(E):
    """Every tile fits the launch guard, covers the image, and an exact
    tile is exact; the predicate only holds on exact even-row tiles."""
    for C in (32, 64):
        for H in range(6, 41):
            for W in range(6, 41):
                OH, OW = H - 2, W - 2
                if OH * OW < 128:
                    continue
                rows, tiles, mi, lds_rows, lds = \
                    E.conv_fwd_res_plan(C, H, W, OH, OW, 3)
                key = (C, H, W)
                assert lds <= LDS_GUARD, key
                assert mi in (4, 6) and tiles * mi * 32 >= OH * OW, key
                assert lds == ((lds_rows * W * (C + 1) + 3) & ~3) * 4 \
                    + B_BUFFERS, key
                if rows:
                    assert rows * OW == mi * 32 <= 192, key
                    assert tiles * rows == OH and lds_rows == rows + 2, key
                    assert lds <= LDS_3_PER_CU, key
                else:
                    assert (rows, tiles, mi, lds_rows, lds) == \
                        _legacy(C, H, W, OH, OW, 3), key
                    # a tile may straddle 127 // OW + 2 output rows
                    assert lds_rows == 127 // OW + 4, key
                fused = E.conv_pool_fused_ok(C, H, W, 64, 3, 3, 1, 0)
                assert bool(fused) == (rows > 0 and rows % 2 == 0
                                       and OH % 2 == 0 and OW % 2 == 0), key
