"""Workspace sizes: the functions beside the launchers (exported from the
extension, host arithmetic only — no GPU needed) against

  (a) the literal formulas the op wrappers carried before the sizes moved
      beside their launchers, written out below as plain Python: the new
      size never exceeds the old one, and equals it everywhere except the
      small-Ncrs backward-weight path, deliberately tightened from 2049
      slabs to the 2048 chunk cap of its launcher;
  (b) the slabs each launcher can touch, written out from its layout.
"""

import itertools

import pytest


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


def cdiv(a, b):
    return -(-a // b)


def stage1(sk):
    return cdiv(sk, 16) if sk > 16 else 0


# ---- the old call-site formulas (floats) ----

def old_gemm_ws(m, n, sk):
    return (sk + stage1(sk)) * m * n if sk > 1 else 0


def old_conv_f32_ws(kout, ncrs, sk):
    mult = 2049 if (ncrs <= 32 and kout <= 64) else sk + 1 + stage1(sk)
    return mult * kout * ncrs


def old_conv_bf16_ws(kout, ncrs, sk):
    return (sk + 1 + stage1(sk)) * kout * ncrs


def old_conv_db_ws(kout):
    return kout * 4096


OLD_FLAT_SCRATCH = 1025


def depth(sk):
    return 'one' if sk == 1 else 'single_stage' if sk <= 16 else 'two_stage'


ALL_DEPTHS = {'one', 'single_stage', 'two_stage'}


def test_gemm_splitk_workspace(ext):
    seen = set()
    dims = (1, 10, 64, 128, 256, 9216)
    for m, n, k in itertools.product(dims, dims, (32, 128, 256, 9216)):
        sk = ext.gemm_f32_splitk(m, n, k)
        assert sk >= 1
        seen.add(depth(sk))
        new = ext.gemm_splitk_ws_floats(m, n, sk)
        assert new == old_gemm_ws(m, n, sk), (m, n, k, sk)
        # SK partial slabs + the stage-1 slabs of launch_splitk_reduce
        touched = (sk + stage1(sk)) * m * n if sk > 1 else 0
        assert new >= touched, (m, n, k, sk)
    assert seen == ALL_DEPTHS


CONV_KOUT = (32, 64, 128, 256, 512)
CONV_NCRS = (9, 27, 288, 576, 1152, 4608)
CONV_KDIM = (64, 200, 1152, 5408, 8192, 131072)
FORCED_SK = (1, 16, 17, 192)


def test_conv_bwd_weight_workspace_fp32(ext):
    seen, small_seen = set(), 0
    for kout, ncrs, kdim in itertools.product(CONV_KOUT, CONV_NCRS,
                                              CONV_KDIM):
        picked = ext.conv_bwd_weight_splitk(kout, ncrs, kdim)
        assert picked >= 1
        for sk in (picked,) + FORCED_SK:
            new = ext.conv_bwd_weight_ws_floats(kout, ncrs, sk)
            old = old_conv_f32_ws(kout, ncrs, sk)
            if ncrs <= 32 and kout <= 64:
                # small path: one slab per m-chunk, chunks as the launcher
                # computes them; tightened to the chunk cap
                small_seen += 1
                chunks = min(max(cdiv(kdim, 128), 64), 2048)
                assert new == 2048 * kout * ncrs < old, (kout, ncrs, sk)
                assert new >= chunks * kout * ncrs, (kout, ncrs, kdim)
            else:
                seen.add(depth(sk))
                assert new == old, (kout, ncrs, sk)
                # slabs + rsc-ordered temp + stage-1 slabs
                touched = (sk + 1 + stage1(sk)) * kout * ncrs
                assert new >= touched, (kout, ncrs, sk)
                assert new == ext.conv_dwperm_ws_floats(kout, ncrs, sk)
    assert seen == ALL_DEPTHS
    assert small_seen > 0


def test_conv_bwd_weight_workspace_bf16(ext):
    seen = set()
    for kout, ncrs, kdim in itertools.product(CONV_KOUT, CONV_NCRS,
                                              CONV_KDIM):
        picked = ext.conv_bwd_weight_bf16_splitk(kout, ncrs, kdim)
        assert picked >= 1
        for sk in (picked,) + FORCED_SK:
            seen.add(depth(sk))
            new = ext.conv_dwperm_ws_floats(kout, ncrs, sk)
            assert new == old_conv_bf16_ws(kout, ncrs, sk), (kout, ncrs, sk)
            touched = (sk + 1 + stage1(sk)) * kout * ncrs
            assert new >= touched, (kout, ncrs, sk)
    assert seen == ALL_DEPTHS


def test_pickers_reach_every_depth(ext):
    """Not only the forced SK values: the policies themselves return
    SK == 1, 1 < SK <= 16 and SK > 16 somewhere in the sweep."""
    for pick in (ext.conv_bwd_weight_splitk,
                 ext.conv_bwd_weight_bf16_splitk):
        got = {depth(pick(ko, n, kd)) for ko, n, kd in
               itertools.product(CONV_KOUT, CONV_NCRS, CONV_KDIM)}
        assert got == ALL_DEPTHS, pick.__name__


def test_conv_db_workspace(ext):
    for kout in range(1, 513):
        new = ext.conv_db_ws_floats(kout)
        assert new == old_conv_db_ws(kout), kout
        # stage 1 writes one Kout row per chunk
        for m in (1, 64, 4096, 5408, 262144, 1 << 24, 1 << 31):
            chunks = ext.conv_db_chunks(m, kout)
            assert 64 <= chunks <= 4096, (m, kout)
            assert new >= chunks * kout, (m, kout)
    # the cap is reached, so the size is not loose by construction
    assert ext.conv_db_chunks(1 << 24, 16) == 4096


def test_flat_norm_scratch(ext):
    # kNPart partial sums of squares + the scale the update kernel reads
    assert ext.flat_norm_scratch_floats() == OLD_FLAT_SCRATCH == 1024 + 1
