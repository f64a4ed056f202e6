"""The backward entry points that share one body in bindings.cpp agree
bitwise on identical inputs.

conv2d_bwd, conv2d_bwd_into and conv2d_bwd_wdx_into differ only in where
dw / db land (a fresh tensor or a caller-owned view) and in whether a
relu_y mask is passed; linear_bwd and linear_bwd_into likewise.  They
launch the same kernels in the same order, so with relu_y=None every
output must be equal bit for bit (torch.equal), not merely close.
batchnorm_bwd vs batchnorm_bwd_into is covered by
test_bf16_reference_gpu.py::test_bn_bwd_and_bwd_into.
"""

import pytest
import torch

gpu = pytest.mark.gpu

DEV = 'cuda:0'
BF = torch.bfloat16


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def conv_inputs(shape, dtype):
    nb, c, h, w, ko, r, st, pad = shape
    g = torch.Generator().manual_seed(1000 * nb + 10 * c + ko + st)
    oh = (h + 2 * pad - r) // st + 1
    ow = (w + 2 * pad - r) // st + 1
    x = cl(torch.randn(nb, c, h, w, generator=g).to(dtype).to(DEV))
    wt = (torch.randn(ko, c, r, r, generator=g) * 0.05).to(DEV)
    dy = cl(torch.randn(nb, ko, oh, ow, generator=g).to(dtype).to(DEV))
    return x, wt, dy


# (Nb, C, H, W, Kout, R, stride, pad) and the backward-weight path reached
FP32_CONV = [
    ((2, 1, 12, 12, 32, 3, 1, 0), 'small'),
    ((2, 32, 12, 12, 64, 3, 1, 0), 'splitk'),
    ((8, 32, 12, 12, 64, 3, 1, 1), 'splitk2'),
]

# bf16: the (backward-data, backward-weight) branches reached
BF16_CONV = [
    ((3, 32, 8, 8, 32, 3, 1, 1), ('tap', 'tap_s1')),
    ((5, 32, 4, 4, 64, 3, 1, 1), ('w4', 'generic')),
    ((2, 32, 12, 8, 32, 3, 1, 1), ('generic', 'tap_s1')),
    ((3, 32, 32, 32, 64, 3, 2, 1), ('tap_s2', 'tap_s2')),
    ((2, 3, 8, 8, 32, 3, 1, 1), ('fp32', 'fp32')),
]


def sid(row):
    return 'x'.join(str(v) for v in row[0])


def fp32_path(ext, shape):
    nb, c, h, w, ko, r, st, pad = shape
    oh = (h + 2 * pad - r) // st + 1
    ow = (w + 2 * pad - r) // st + 1
    ncrs = c * r * r
    if ncrs <= 32 and ko <= 64:
        return 'small'
    sk = ext.conv_bwd_weight_splitk(ko, ncrs, nb * oh * ow)
    return 'direct' if sk == 1 else 'splitk' if sk <= 16 else 'splitk2'


def bf16_branches(ext, shape):
    nb, c, h, w, ko, r, st, pad = shape
    if ko % 32 or c % 8:
        return 'fp32', 'fp32'
    if ext.conv_tap_fwd_w4_ok(ko, h, w, c, r, r, st, pad):
        dx = 'w4'
    elif ext.conv_tap_fwd_ok(ko, h, w, c, r, r, st, pad):
        dx = 'tap'
    elif ext.conv_tap_bwdd_s2_ok(c, h, w, ko, r, r, st, pad):
        dx = 'tap_s2'
    else:
        dx = 'generic'
    if ext.conv_bwdw_tap_ok(c, h, w, ko, r, r, st, pad):
        dw = 'tap_s1'
    elif ext.conv_bwdw_tap_s2_ok(c, h, w, ko, r, r, st, pad):
        dw = 'tap_s2'
    else:
        dw = 'generic'
    return dx, dw


def test_rows_reach_each_path(ext):
    """Host arithmetic only: every row takes the path it is there for."""
    for shape, want in FP32_CONV:
        assert fp32_path(ext, shape) == want, shape
    for shape, want in BF16_CONV:
        assert bf16_branches(ext, shape) == want, shape
    assert {w[0] for _, w in BF16_CONV} == \
        {'tap', 'w4', 'generic', 'tap_s2', 'fp32'}
    assert {w[1] for _, w in BF16_CONV} >= {'tap_s1', 'tap_s2', 'generic'}


@gpu
@pytest.mark.parametrize('row', FP32_CONV, ids=sid)
def test_conv_fp32_entry_points_bitwise(ext, row):
    shape = row[0]
    st, pad = shape[6], shape[7]
    x, w, dy = conv_inputs(shape, torch.float32)
    dx, dw, db = ext.conv2d_bwd(x, w, dy, st, pad, True, True)
    dw_i, db_i = torch.empty_like(w), torch.empty_like(db)
    dx_i = ext.conv2d_bwd_into(x, w, dy, st, pad, True, dw_i, db_i, None)
    dw_w = torch.empty_like(w)
    dx_w = ext.conv2d_bwd_wdx_into(x, w, dy, st, pad, True, dw_w, None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx).all() and torch.isfinite(dw).all())
    assert float(dw.abs().max()) > 0 and float(dx.abs().max()) > 0
    assert torch.equal(dx, dx_i) and torch.equal(dx, dx_w)
    assert torch.equal(dw, dw_i) and torch.equal(dw, dw_w)
    assert torch.equal(db, db_i)
    # need_dx=False: no dx, same dw
    dw_n = torch.empty_like(w)
    assert ext.conv2d_bwd_into(x, w, dy, st, pad, False, dw_n, None,
                               None) is None
    none_dx, dw_m, none_db = ext.conv2d_bwd(x, w, dy, st, pad, False, False)
    assert none_dx is None and none_db is None
    assert torch.equal(dw, dw_n) and torch.equal(dw, dw_m)


@gpu
@pytest.mark.parametrize('row', BF16_CONV, ids=sid)
def test_conv_bf16_entry_points_bitwise(ext, row):
    shape = row[0]
    st, pad = shape[6], shape[7]
    x, w, dy = conv_inputs(shape, BF)
    dx, dw, db = ext.conv2d_bwd(x, w, dy, st, pad, False, True)
    dw_w = torch.empty_like(w)
    dx_w = ext.conv2d_bwd_wdx_into(x, w, dy, st, pad, True, dw_w, None)
    torch.cuda.synchronize()
    assert db is None
    assert dx.dtype == BF and dx_w.dtype == BF and dw.dtype == torch.float32
    assert bool(torch.isfinite(dx.float()).all() and torch.isfinite(dw).all())
    assert float(dw.abs().max()) > 0 and float(dx.float().abs().max()) > 0
    assert torch.equal(dx, dx_w)
    assert torch.equal(dw, dw_w)


@gpu
@pytest.mark.parametrize('mio', [(256, 9216, 128), (8, 50, 10)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_linear_entry_points_bitwise(ext, mio):
    m, n_in, n_out = mio
    g = torch.Generator().manual_seed(m + n_in)
    x = torch.randn(m, n_in, generator=g).to(DEV)
    w = (torch.randn(n_out, n_in, generator=g) * 0.05).to(DEV)
    dy = torch.randn(m, n_out, generator=g).to(DEV)
    dx, dw, db = ext.linear_bwd(x, w, dy)
    dw_i, db_i = torch.empty_like(w), torch.empty_like(db)
    dx_i = ext.linear_bwd_into(x, w, dy, dw_i, db_i, True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx).all() and torch.isfinite(dw).all())
    assert float(dw.abs().max()) > 0 and float(dx.abs().max()) > 0
    assert torch.equal(dx, dx_i)
    assert torch.equal(dw, dw_i)
    assert torch.equal(db, db_i)
    dw_n = torch.empty_like(w)
    assert ext.linear_bwd_into(x, w, dy, dw_n, None, False) is None
    assert torch.equal(dw, dw_n)
