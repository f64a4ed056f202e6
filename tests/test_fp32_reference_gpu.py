"""Every fp32 GEMM and conv kernel against an fp64 reference, element by
element, inside a DERIVED error bound.

The other fp32 tests either compare with the device's own fp32 torch
result at atol 1e-3..1e-2 (test_kernels_gpu.py: seven conv shapes, five
GEMM shapes, all on the aligned fast paths) or assert "bitwise equal to
another path of ours", which a bug shared by both sides passes.  Here
every instantiation the four launchers can reach (launch_gemm_f32_main,
launch_conv_fwd, launch_conv_bwd_data_relu, launch_conv_bwd_weight_main),
every split-K combine form and every M / N / K / Kout / C*R*S tail is
held to the bound below at the smallest shape that reaches it.

Inputs: fp32 randn from a seeded CPU generator, weights scaled by 0.05.
Reference: the same operation in fp64 on the CPU, on the up-cast inputs.

Bound for every output element, none excluded, with n the number of
products summed into it (plus 1 where a bias is added) and `mag` the same
operation applied to |inputs| (plus |bias|) in fp64:

    |got - ref| <= 2^-23 |ref| + n 2^-23 mag

Derivation: fp32 products and adds round to nearest, so a sum of n terms
in ANY order (split-K folds included) errs by at most n 2^-24 mag to
first order; the bound keeps a factor 2 over that in case the MFMA unit
does not round to nearest internally.  relu is 1-Lipschitz, so relu(ref)
keeps the bound.  NaN or Inf counts as over the bound.

What the bound sees: it is a test for STRUCTURAL bugs (a dropped tap, a
tail row, a bias added twice), not for rounding quality.  Such bugs sit
far over the bound only while n is small: at K = 9216 "bias added twice"
stays inside it.  So every row that is in a table for a tail, a bias or
an Nb edge has n <= N_TAIL_MAX, and the self-tests plant each bug at each
such row and require the checker to reject it.

The checker self-tests and the dispatch / coverage tests run without a
GPU; everything that launches a kernel is marked `gpu`.
"""

import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

DEV = 'cuda:0'
E23 = 2.0 ** -23
D = torch.float64
N_TAIL_MAX = 2400
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..',
                    'rlr_amd', 'ops', 'csrc')


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


# ------------------------------------------------------------------ checker

def bound_of(ref, mag, n):
    return E23 * ref.to(D).abs() + n * E23 * mag.to(D)


def check(got, ref, mag, n, what):
    """Assert every element of the fp32 tensor `got` within the derived
    bound of `ref`; prints and returns the worst error/bound ratio."""
    assert tuple(got.shape) == tuple(ref.shape), \
        f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert got.dtype == torch.float32, f"{what}: dtype {got.dtype}"
    g = got.detach().to('cpu', D)
    ref = ref.to(D)
    bound = bound_of(ref, mag, n)
    err = (g - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).nan_to_num(nan=float('inf'))
    bad = ~(err <= bound)  # NaN compares false, so it counts as bad
    worst = float(ratio.max())
    print(f"f32ref {what}: worst err/bound = {worst:.4g} over "
          f"{ratio.numel()} elements")
    if bad.any():
        flat = int(ratio.flatten().argmax())
        idx = tuple(int(i) for i in
                    torch.unravel_index(torch.tensor(flat), ratio.shape))
        raise AssertionError(
            f"{what}: {float(bad.double().mean()):.3%} of elements over "
            f"the bound; worst at {idx}: got {float(g[idx])!r} ref "
            f"{float(ref[idx])!r} bound {float(bound[idx])!r}")
    return worst


def rejected(got, ref, mag, n, what):
    with pytest.raises(AssertionError, match='over the bound'):
        check(got, ref, mag, n, 'mutant: ' + what)


def sid(s):
    return 'x'.join(str(v) for v in s)


def seed_of(*ints):
    s = 23
    for v in ints:
        s = (s * 1000003 + v) % (2 ** 31 - 1)
    return s


def cdiv(a, b):
    return -(-a // b)


def tf(b):
    return 'true' if b else 'false'


# ------------------------------------------------- GEMM dispatch, mirrored
# launch_gemm_f32_main and splitk_reduce_roles (gemm_f32.hip).  The split
# depth itself comes from the exported gemm_f32_splitk.

BM, BN, BK = 128, 64, 32


def py_gemm_tiny(m, n, k):
    return m * n * k <= 8_000_000 and m * n <= 65536


def py_gemm_kernel(m, n, k, lda, ldb, layout):
    if py_gemm_tiny(m, n, k):
        return 'gemm_small_wave_k' if k >= 32 else 'gemm_small_k'
    vec = lda % 4 == 0 and ldb % 4 == 0
    return f'gemm_f32_k<{tf(vec)},{tf(layout == 1)},{tf(layout == 2)}>'


def py_gemm_combine(m, n, sk):
    n_out = m * n
    if sk == 1:
        return 'direct'
    if sk > 16 and n_out <= 262144:
        return 'two_level'
    if n_out <= 8192 and sk >= 16:
        return 'wave'
    return 'thread'


def gemm_plan(ext, m, n, k, lda, ldb, layout):
    """(kernel, SK, combine, empty split-K chunks) of one GEMM call; the
    tiny kernels ignore SK."""
    kern = py_gemm_kernel(m, n, k, lda, ldb, layout)
    if not kern.startswith('gemm_f32_k'):
        return kern, 1, 'direct', 0
    sk = ext.gemm_f32_splitk(m, n, k)
    kpc = k if sk == 1 else cdiv(cdiv(k, sk), BK) * BK
    return kern, sk, py_gemm_combine(m, n, sk), sk - cdiv(k, kpc)


NN_V = 'gemm_f32_k<true,false,false>'
NN_S = 'gemm_f32_k<false,false,false>'
AT_V = 'gemm_f32_k<true,true,false>'
AT_S = 'gemm_f32_k<false,true,false>'
BT_V = 'gemm_f32_k<true,false,true>'
BT_S = 'gemm_f32_k<false,false,true>'
WAVE, SMALL = 'gemm_small_wave_k', 'gemm_small_k'

# ((M, N, K), (kernel, SK, combine, empty chunks)) through ext.gemm:
# layout 0, lda = K, ldb = N.
GEMM_ROWS = [
    # SK = 1: bias + relu inside the tile kernel; tails M 44, N 44, K 8
    ((300, 300, 40), (NN_V, 1, 'direct', 0)),
    ((300, 301, 41), (NN_S, 1, 'direct', 0)),
    # two-level fold; tails M 2, N 4, K 8
    ((130, 68, 1000), (NN_V, 32, 'two_level', 0)),
    ((130, 67, 1001), (NN_S, 32, 'two_level', 0)),
    # fold chunks 16 + 16 + 3; one-element M and N tails
    ((129, 65, 1100), (NN_S, 35, 'two_level', 0)),
    ((256, 256, 1100), (NN_V, 32, 'two_level', 14)),
    ((256, 512, 600), (NN_V, 16, 'thread', 6)),
    ((256, 512, 200), (NN_V, 7, 'thread', 0)),
    # SK = 16 with M*N = 8192: the wave-form combine; K == N
    ((8, 1024, 1024), (NN_V, 16, 'wave', 0)),
    ((100, 30, 50), (WAVE, 1, 'direct', 0)),
    ((64, 70, 300), (WAVE, 1, 'direct', 0)),
    ((40, 50, 20), (SMALL, 1, 'direct', 0)),
    # M == K, for the "A used transposed" mutant
    ((48, 20, 48), (WAVE, 1, 'direct', 0)),
]

# ((B, in, out), plans of (fwd: layout 2, dx: layout 0, dw: layout 1),
#  tail_row).  tail_row False: in the table for the launch path only, n is
# too large for the structural mutants.
LINEAR_ROWS = [
    ((132, 1000, 68), ((BT_V, 32, 'two_level', 0),
                       (NN_V, 3, 'thread', 0),
                       (AT_V, 5, 'thread', 0)), True),
    ((130, 1001, 68), ((BT_S, 32, 'two_level', 0),
                       (NN_S, 3, 'thread', 0),
                       (AT_S, 5, 'thread', 0)), True),
    ((8, 50, 10), ((WAVE, 1, 'direct', 0), (SMALL, 1, 'direct', 0),
                   (SMALL, 1, 'direct', 0)), True),
    # the real fc1 at a ragged batch: M tail, 32 empty chunks, K = 37 in dw
    ((37, 9216, 128), ((BT_V, 128, 'two_level', 32),
                       (NN_V, 2, 'thread', 0),
                       (AT_V, 1, 'direct', 0)), False),
]


def linear_plans(ext, row):
    b, i, o = row
    return (gemm_plan(ext, b, o, i, i, i, 2),
            gemm_plan(ext, b, i, o, o, i, 0),
            gemm_plan(ext, o, i, b, o, i, 1))


# ------------------------------------------------- conv dispatch, mirrored
# launch_conv_fwd, launch_conv_bwd_data_relu, launch_conv_bwd_weight_main
# and splitk_reduce_dwperm_roles (conv_f32.hip).  The resident plan, the
# pool predicate and the split depth come from the exported host functions.
# Shapes are (Nb, C, H, W, Kout, R, stride, pad), R x R taps.

RES_LDS_MAX = 100 * 1024


def out_hw(shape):
    nb, c, h, w, ko, r, st, pad = shape
    return (h + 2 * pad - r) // st + 1, (w + 2 * pad - r) // st + 1


def py_conv_fwd_small(c, ko, r):
    return c * r * r <= 32 and ko in (32, 64)


def py_conv_fwd_resident(ext, shape):
    nb, c, h, w, ko, r, st, pad = shape
    oh, ow = out_hw(shape)
    return pad == 0 and st == 1 and c % 32 == 0 and oh * ow >= 128 and \
        ext.conv_fwd_res_plan(c, h, w, oh, ow, r)[4] <= RES_LDS_MAX


def py_conv_fwd_kernel(ext, shape):
    nb, c, h, w, ko, r, st, pad = shape
    if py_conv_fwd_small(c, ko, r):
        return f'conv_small_fwd_k<{ko}>'
    if py_conv_fwd_resident(ext, shape):
        mi = ext.conv_fwd_res_plan(c, h, w, *out_hw(shape), r)[2]
        return f'conv_fwd_res_k<{mi},false>'
    return f'conv_fwd_k<{tf(pad == 0)},{tf(c % 32 == 0)}>'


def py_conv_pool_kernel(ext, shape):
    """The pooled-epilogue instantiation conv2d_pool_fwd launches, or None
    where it runs the two unfused launches."""
    nb, c, h, w, ko, r, st, pad = shape
    if not ext.conv_pool_fused_ok(c, h, w, ko, r, r, st, pad):
        return None
    mi = ext.conv_fwd_res_plan(c, h, w, *out_hw(shape), r)[2]
    return f'conv_fwd_res_k<{mi},true>'


def py_conv_bwdd_kernel(shape):
    nb, c, h, w, ko, r, st, pad = shape
    v4 = ko % 32 == 0
    if st == 1:
        form = f'1,{tf(v4)}'
    elif st == 2 and v4:
        form = '2,true'
    elif c <= 32:
        form = '0,false'
    else:
        form = '2,false' if st == 2 else '0,false'
    return ('conv_bwd_data32_k<' if c <= 32 else 'conv_bwd_data_k<') + \
        form + '>'


def py_conv_bwdw_small(ko, ncrs):
    return ncrs <= 32 and ko <= 64 and ko % 4 == 0


def py_conv_bwdw_combine(sk):
    return 'direct' if sk == 1 else 'one_level' if sk <= 16 else 'two_level'


def conv_bwdw_plan(ext, shape):
    """(kernel, SK, combine, empty split-K chunks); the small kernel has
    its own chunking and no split-K."""
    nb, c, h, w, ko, r, st, pad = shape
    oh, ow = out_hw(shape)
    ncrs, kdim = c * r * r, nb * oh * ow
    if py_conv_bwdw_small(ko, ncrs):
        return 'conv_small_bwdw_k<128>', 0, 'chunks', 0
    sk = ext.conv_bwd_weight_splitk(ko, ncrs, kdim)
    kpc = kdim if sk == 1 else cdiv(cdiv(kdim, sk), BK) * BK
    kern = f'conv_bwd_weight_k<{tf(pad == 0)},{tf(c % 4 == 0)}>'
    return kern, sk, py_conv_bwdw_combine(sk), sk - cdiv(kdim, kpc)


SM_W = ('conv_small_bwdw_k<128>', 0, 'chunks', 0)

# (shape, forward kernel, backward-data kernel, backward-weight plan).
# Every row runs all three; the comment says what the row is there for.
CONV_ROWS = [
    # the thin first layers: direct kernels
    ((3, 1, 12, 12, 32, 3, 1, 0), 'conv_small_fwd_k<32>',
     'conv_bwd_data32_k<1,true>', SM_W),
    ((3, 3, 12, 12, 64, 3, 1, 1), 'conv_small_fwd_k<64>',
     'conv_bwd_data32_k<1,true>', SM_W),
    ((3, 3, 13, 13, 64, 3, 2, 1), 'conv_small_fwd_k<64>',
     'conv_bwd_data32_k<2,true>', SM_W),
    # Kout = 10: Kout tail everywhere; backward-weight must NOT take the
    # small kernel, whose float4 dy staging needs Kout % 4 == 0
    ((2, 1, 12, 12, 10, 3, 1, 0), 'conv_fwd_k<true,false>',
     'conv_bwd_data32_k<1,false>',
     ('conv_bwd_weight_k<true,false>', 7, 'one_level', 0)),
    # Kout = 62: the largest even Kout the small kernel mis-staged
    ((2, 1, 8, 8, 62, 3, 1, 0), 'conv_fwd_k<true,false>',
     'conv_bwd_data32_k<1,false>',
     ('conv_bwd_weight_k<true,false>', 3, 'one_level', 0)),
    ((2, 2, 9, 9, 16, 3, 1, 1), 'conv_fwd_k<false,false>',
     'conv_bwd_data32_k<1,false>', SM_W),
    # resident forward: MI = 6 (3 tiles), MI = 4 exact with a Kout tail,
    # tile_rows = 0 with two n-blocks and a Kout tail of 8
    ((3, 32, 26, 26, 64, 3, 1, 0), 'conv_fwd_res_k<6,false>',
     'conv_bwd_data32_k<1,true>',
     ('conv_bwd_weight_k<true,true>', 54, 'two_level', 0)),
    ((3, 32, 18, 18, 40, 3, 1, 0), 'conv_fwd_res_k<4,false>',
     'conv_bwd_data32_k<1,false>',
     ('conv_bwd_weight_k<true,true>', 24, 'two_level', 0)),
    ((3, 64, 15, 15, 72, 3, 1, 0), 'conv_fwd_res_k<4,false>',
     'conv_bwd_data_k<1,false>',
     ('conv_bwd_weight_k<true,true>', 16, 'one_level', 0)),
    # the implicit-GEMM forward and backward-weight, all four forms each
    ((3, 32, 9, 9, 40, 3, 1, 0), 'conv_fwd_k<true,true>',
     'conv_bwd_data32_k<1,false>',
     ('conv_bwd_weight_k<true,true>', 5, 'one_level', 0)),
    ((3, 64, 9, 9, 64, 3, 1, 1), 'conv_fwd_k<false,true>',
     'conv_bwd_data_k<1,true>',
     ('conv_bwd_weight_k<false,true>', 8, 'one_level', 0)),
    ((3, 6, 9, 9, 20, 3, 1, 0), 'conv_fwd_k<true,false>',
     'conv_bwd_data32_k<1,false>',
     ('conv_bwd_weight_k<true,false>', 5, 'one_level', 0)),
    ((3, 6, 9, 9, 20, 3, 2, 1), 'conv_fwd_k<false,false>',
     'conv_bwd_data32_k<0,false>',
     ('conv_bwd_weight_k<false,false>', 3, 'one_level', 0)),
    # backward-data at stride 2 and 3 with a C tail of 40
    ((3, 40, 9, 9, 64, 3, 2, 1), 'conv_fwd_k<false,false>',
     'conv_bwd_data_k<2,true>',
     ('conv_bwd_weight_k<false,true>', 3, 'one_level', 0)),
    ((3, 40, 9, 9, 36, 3, 2, 1), 'conv_fwd_k<false,false>',
     'conv_bwd_data_k<2,false>',
     ('conv_bwd_weight_k<false,true>', 3, 'one_level', 0)),
    # stride 3; backward-weight SK = 1 writes the rsc temp directly
    ((2, 40, 10, 10, 36, 3, 3, 1), 'conv_fwd_k<false,false>',
     'conv_bwd_data_k<0,false>',
     ('conv_bwd_weight_k<false,true>', 1, 'direct', 0)),
    # the 1x1 stride-2 shortcut conv; SK = 1 with Kdim = 50
    ((2, 64, 9, 9, 32, 1, 2, 0), 'conv_fwd_k<true,true>',
     'conv_bwd_data_k<2,true>',
     ('conv_bwd_weight_k<true,true>', 1, 'direct', 0)),
    # fold chunks 16 + 3
    ((5, 3, 11, 11, 128, 3, 1, 1), 'conv_fwd_k<false,false>',
     'conv_bwd_data32_k<1,true>',
     ('conv_bwd_weight_k<false,false>', 19, 'two_level', 0)),
    # empty split-K chunks: 5766 output pixels in 128 chunks of 64
    ((6, 64, 31, 31, 256, 3, 1, 1), 'conv_fwd_k<false,true>',
     'conv_bwd_data_k<1,true>',
     ('conv_bwd_weight_k<false,true>', 128, 'two_level', 37)),
]
CONV_SHAPES = [r[0] for r in CONV_ROWS]

# rows whose fused conv + pool epilogue is checked too
POOL_ROWS = [
    ((3, 32, 26, 26, 64, 3, 1, 0), 'conv_fwd_res_k<6,true>'),
    ((3, 32, 18, 18, 40, 3, 1, 0), 'conv_fwd_res_k<4,true>'),
]

# relu_y-masked backward-data through conv2d_bwd_into: the epilogue of
# both kernel families, vectorised and scalar gathers
MASK_SHAPES = [
    (3, 3, 12, 12, 64, 3, 1, 1),    # data32<1,true>
    (3, 6, 9, 9, 20, 3, 2, 1),      # data32<0,false>
    (3, 64, 9, 9, 64, 3, 1, 1),     # data<1,true>
    (3, 40, 9, 9, 36, 3, 2, 1),     # data<2,false>
]


# -------------------------------------------------------------- references

@functools.lru_cache(maxsize=None)
def gemm_case(m, n, k):
    """A (M,K), B (K,N) scaled like weights, bias (N) and their fp64
    references, computed once and shared read-only."""
    g = torch.Generator().manual_seed(seed_of(m, n, k))
    a = torch.randn(m, k, generator=g)
    b = torch.randn(k, n, generator=g) * 0.05
    bias = torch.randn(n, generator=g)
    c = a.to(D) @ b.to(D)
    mag = a.to(D).abs() @ b.to(D).abs()
    return dict(a=a, b=b, bias=bias, n=k, c=c, mag=mag,
                cb=torch.relu(c + bias.to(D)), cb_mag=mag + bias.to(D).abs())


@functools.lru_cache(maxsize=None)
def linear_case(b, i, o):
    g = torch.Generator().manual_seed(seed_of(b, i, o, 7))
    x = torch.randn(b, i, generator=g)
    w = torch.randn(o, i, generator=g) * 0.05
    bias = torch.randn(o, generator=g)
    dy = torch.randn(b, o, generator=g)
    x6, w6, b6, d6 = x.to(D), w.to(D), bias.to(D), dy.to(D)
    y = x6 @ w6.t()
    ym = x6.abs() @ w6.abs().t()
    return dict(
        x=x, w=w, bias=bias, dy=dy,
        y=y, y_mag=ym, yb=torch.relu(y + b6), yb_mag=ym + b6.abs(),
        dx=d6 @ w6, dx_mag=d6.abs() @ w6.abs(),
        dw=d6.t() @ x6, dw_mag=d6.abs().t() @ x6.abs(),
        db=d6.sum(0), db_mag=d6.abs().sum(0))


def conv_all(x, w, dy, st, pad):
    """(y, dx, dw, db) of one conv in the dtype of its arguments."""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    y = F.conv2d(x, w, None, stride=st, padding=pad)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    return y.detach(), dx, dw, dy.sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def conv_case(shape):
    """Inputs and fp64 references of one shape, computed once on the CPU
    and shared (read-only) by every test that needs them."""
    nb, c, h, w, ko, r, st, pad = shape
    oh, ow = out_hw(shape)
    g = torch.Generator().manual_seed(seed_of(*shape))
    x = torch.randn(nb, c, h, w, generator=g)
    wt = torch.randn(ko, c, r, r, generator=g) * 0.05
    b = torch.randn(ko, generator=g)
    dy = torch.randn(nb, ko, oh, ow, generator=g)
    relu_y = torch.relu(torch.randn(nb, c, h, w, generator=g))
    y, dx, dw, db = conv_all(x.to(D), wt.to(D), dy.to(D), st, pad)
    ym, dxm, dwm, dbm = conv_all(x.to(D).abs(), wt.to(D).abs(),
                                 dy.to(D).abs(), st, pad)
    bd = b.to(D).view(1, -1, 1, 1)
    return dict(
        shape=shape, x=x, w=wt, b=b, dy=dy, relu_y=relu_y,
        n_y=c * r * r, n_dx=ko * r * r, n_dw=nb * oh * ow,
        y=y, y_mag=ym, yb=torch.relu(y + bd), yb_mag=ym + bd.abs(),
        dx=dx, dx_mag=dxm, dx_masked=dx * (relu_y > 0),
        dw=dw, dw_mag=dwm, db=db, db_mag=dbm)


def torch_fp32_conv(k):
    """torch's own fp32 CPU conv + backward: the stand-in 'kernel' of the
    checker self-tests."""
    st, pad = k['shape'][6], k['shape'][7]
    y, dx, dw, db = conv_all(k['x'], k['w'], k['dy'], st, pad)
    yb = torch.relu(F.conv2d(k['x'], k['w'], k['b'], stride=st,
                             padding=pad))
    return y, yb, dx, dw, db


# ------------------------------------------------- pooled-epilogue checker

def pool_cells(t):
    """The four cells of every 2x2 window, stacked in the argmax coding of
    maxpool2x2_fwd (00, 01, 10, 11)."""
    return torch.stack([t[:, :, 0::2, 0::2], t[:, :, 0::2, 1::2],
                        t[:, :, 1::2, 0::2], t[:, :, 1::2, 1::2]])


def check_pool(pooled, idx, k, what):
    """Each pooled value within the largest of its window's four bounds of
    max_pool2d(relu(ref + b)); idx names a cell whose reference value is
    within twice that bound of the window maximum."""
    ref = k['yb']
    bound = bound_of(ref, k['yb_mag'], k['n_y'] + 1)
    pref = F.max_pool2d(ref, 2)
    pbound = F.max_pool2d(bound, 2)
    assert tuple(pooled.shape) == tuple(pref.shape), what
    assert pooled.dtype == torch.float32 and idx.dtype == torch.uint8, what
    got = pooled.detach().to('cpu', D)
    err = (got - pref).abs()
    worst = float((err / pbound.clamp_min(1e-300))
                  .nan_to_num(nan=float('inf')).max())
    print(f"f32ref {what} pooled: worst err/bound = {worst:.4g} over "
          f"{err.numel()} elements")
    bad = ~(err <= pbound)
    assert not bad.any(), \
        f"{what}: {float(bad.double().mean()):.3%} of pooled values over " \
        f"the bound"
    ix = idx.detach().cpu().long()
    assert int(ix.max()) <= 3, what
    named = pool_cells(ref).gather(0, ix.unsqueeze(0))[0]
    off = ~(named >= pref - 2 * pbound)
    assert not off.any(), \
        f"{what}: {int(off.sum())} argmax cells over the bound below " \
        f"their window's maximum"
    return worst


def first_max_2x2(x):
    """2x2/2 max-pool with the first maximum of each window as argmax."""
    v = pool_cells(x)
    m, a = v[0].clone(), torch.zeros_like(v[0], dtype=torch.uint8)
    for i in (1, 2, 3):
        gt = v[i] > m
        m = torch.where(gt, v[i], m)
        a = torch.where(gt, torch.full_like(a, i), a)
    return m, a


# ------------------------------------------ checker self-tests (CPU only)

def gemm_id(r):
    return sid(r[0])


@pytest.mark.parametrize('row', GEMM_ROWS, ids=gemm_id)
def test_checker_accepts_torch_fp32_gemm(row):
    """(a) torch's own fp32 result is inside the bound at every row: the
    reference alone stays inside it."""
    k = gemm_case(*row[0])
    c = k['a'] @ k['b']
    check(c, k['c'], k['mag'], k['n'], 'torch C')
    check(torch.relu(c + k['bias']), k['cb'], k['cb_mag'], k['n'] + 1,
          'torch relu(C+b)')


@pytest.mark.parametrize('row', LINEAR_ROWS, ids=gemm_id)
def test_checker_accepts_torch_fp32_linear(row):
    b, i, o = row[0]
    k = linear_case(b, i, o)
    x, w, dy = k['x'], k['w'], k['dy']
    check(x @ w.t(), k['y'], k['y_mag'], i, 'torch y')
    check(torch.relu(x @ w.t() + k['bias']), k['yb'], k['yb_mag'], i + 1,
          'torch relu(y+b)')
    check(dy @ w, k['dx'], k['dx_mag'], o, 'torch dx')
    check(dy.t() @ x, k['dw'], k['dw_mag'], b, 'torch dw')
    check(dy.sum(0), k['db'], k['db_mag'], b, 'torch db')


def gemm_mutants(a, b, bias, m, n, k):
    """The bugs a GEMM kernel can have, planted in torch's fp32 result:
    (name, C, with_bias_relu) each."""
    c = a @ b
    out = []
    out.append(('last k dropped', a[:, :-1] @ b[:-1], False))
    z = c.clone()
    z[-1] = 0
    out.append(('last row zero', z, False))
    z = c.clone()
    z[:, -1] = z[:, -2]
    out.append(('last column copied from its neighbour', z, False))
    lo = BK if k > 2 * BK else 0   # the second k-tile where there is one
    a2 = a.clone()
    a2[:, lo:lo + BK] = 0
    out.append(('one 32-wide k-tile skipped', a2 @ b, False))
    out.append(('bias added twice', torch.relu(c + 2 * bias), True))
    if m == k:
        out.append(('A used transposed', a.t() @ b, False))
    if k == n:
        out.append(('B used transposed', a @ b.t(), False))
    return out


@pytest.mark.parametrize('row', GEMM_ROWS, ids=gemm_id)
def test_checker_rejects_gemm_mutants(row):
    """(b) every planted bug puts at least one element over the bound, at
    every GEMM row."""
    m, n, kk = row[0]
    assert kk <= N_TAIL_MAX
    k = gemm_case(m, n, kk)
    for name, c, with_bias in gemm_mutants(k['a'], k['b'], k['bias'],
                                           m, n, kk):
        if with_bias:
            rejected(c, k['cb'], k['cb_mag'], kk + 1, name)
        else:
            rejected(c, k['c'], k['mag'], kk, name)


@pytest.mark.parametrize('row', [r for r in LINEAR_ROWS if r[2]],
                         ids=gemm_id)
def test_checker_rejects_linear_mutants(row):
    """The same bugs in each of the three GEMMs of a linear layer (A and B
    as the launcher sees them), plus a batch row missing from db."""
    b, i, o = row[0]
    assert max(b, i, o) <= N_TAIL_MAX
    k = linear_case(b, i, o)
    x, w, dy, bias = k['x'], k['w'], k['dy'], k['bias']
    zero = torch.zeros
    for name, c, with_bias in gemm_mutants(x, w.t(), bias, b, o, i):
        if with_bias:
            rejected(c, k['yb'], k['yb_mag'], i + 1, 'fwd ' + name)
        else:
            rejected(c, k['y'], k['y_mag'], i, 'fwd ' + name)
    for name, c, with_bias in gemm_mutants(dy, w, zero(i), b, i, o):
        if not with_bias:
            rejected(c, k['dx'], k['dx_mag'], o, 'dx ' + name)
    for name, c, with_bias in gemm_mutants(dy.t(), x, zero(i), o, i, b):
        if not with_bias:
            rejected(c, k['dw'], k['dw_mag'], b, 'dw ' + name)
    rejected(dy[:-1].sum(0), k['db'], k['db_mag'], b, 'db last row dropped')


def test_mutant_rows_cover_transposed_cases():
    assert any(r[0][0] == r[0][2] for r in GEMM_ROWS)   # M == K
    assert any(r[0][2] == r[0][1] for r in GEMM_ROWS)   # K == N
    assert any(s[1] == s[4] for s in CONV_SHAPES)       # C == Kout


@pytest.mark.parametrize('shape', CONV_SHAPES, ids=sid)
def test_checker_accepts_torch_fp32_conv(shape):
    k = conv_case(shape)
    y, yb, dx, dw, db = torch_fp32_conv(k)
    check(y, k['y'], k['y_mag'], k['n_y'], 'torch y')
    check(yb, k['yb'], k['yb_mag'], k['n_y'] + 1, 'torch relu(y+b)')
    check(dx, k['dx'], k['dx_mag'], k['n_dx'], 'torch dx')
    check(dx * (k['relu_y'] > 0), k['dx_masked'], k['dx_mag'], k['n_dx'],
          'torch masked dx')
    check(dw, k['dw'], k['dw_mag'], k['n_dw'], 'torch dw')
    check(db, k['db'], k['db_mag'], k['n_dw'], 'torch db')


def tap_only(k, r, s):
    """fp32 conv of the case's inputs with every tap but (r, s) zeroed."""
    w1 = torch.zeros_like(k['w'])
    w1[:, :, r, s] = k['w'][:, :, r, s]
    return F.conv2d(k['x'], w1, None, stride=k['shape'][6],
                    padding=k['shape'][7])


@pytest.mark.parametrize('shape', CONV_SHAPES, ids=sid)
def test_checker_rejects_conv_mutants(shape):
    """(b) the bugs these kernels can have, planted in torch's fp32
    output: each must put at least one element over the bound, at every
    row whose n is small enough for the row to count as a tail row."""
    k = conv_case(shape)
    nb, c, h, w, ko, r, st, pad = shape
    y, _, dx, dw, _ = torch_fp32_conv(k)
    assert k['n_y'] <= N_TAIL_MAX and k['n_dx'] <= N_TAIL_MAX
    ya = (k['y'], k['y_mag'], k['n_y'])

    # one tap dropped on the last column only.  The tap is one that reads
    # real data there (s = 0; the last tap may read the zero halo)
    m = y.clone()
    m[..., -1] -= tap_only(k, r // 2, 0)[..., -1]
    rejected(m, *ya, 'tap dropped on the last column')
    # one tap dropped on the last row only
    m = y.clone()
    m[:, :, -1, :] -= tap_only(k, 0, r // 2)[:, :, -1, :]
    rejected(m, *ya, 'tap dropped on the last row')
    # the last image left as zeros (an Nb-tail bug)
    m = y.clone()
    m[-1] = 0
    rejected(m, *ya, 'last image missing from y')
    # weights used with C and Kout swapped
    if c == ko:
        m = F.conv2d(k['x'], k['w'].transpose(0, 1).contiguous(), None,
                     stride=st, padding=pad)
        rejected(m, *ya, 'C and Kout swapped')
    # the relu_y mask ignored in backward-data
    rejected(dx, k['dx_masked'], k['dx_mag'], k['n_dx'], 'mask ignored')

    if k['n_dw'] > N_TAIL_MAX:
        # in the table for its launch path (empty split-K chunks) only
        assert conv_row(shape)[3][3] > 0
        return
    wa = (k['dw'], k['dw_mag'], k['n_dw'])
    m = conv_all(k['x'][:-1], k['w'], k['dy'][:-1], st, pad)[2]
    rejected(m, *wa, 'last image missing from dw')
    dy1 = k['dy'].clone()
    dy1[-1, :, -1, -1] = 0
    m = conv_all(k['x'], k['w'], dy1, st, pad)[2]
    rejected(m, *wa, 'last output pixel missing from dw')


def conv_row(shape):
    return next(r for r in CONV_ROWS if r[0] == shape)


@pytest.mark.parametrize('row', POOL_ROWS, ids=lambda r: sid(r[0]))
def test_pool_checker_self_test(row):
    """torch's fp32 conv + first-maximum pool passes check_pool; a pool
    that ignores one cell of every window, and an argmax that always
    names cell 0, do not."""
    k = conv_case(row[0])
    yb = torch_fp32_conv(k)[1]
    m, a = first_max_2x2(yb)
    check_pool(m, a, k, 'torch')
    cells = pool_cells(yb)
    with pytest.raises(AssertionError, match='pooled values over'):
        check_pool(cells[:3].max(0).values, a, k, 'cell 11 ignored')
    with pytest.raises(AssertionError, match='argmax cells over'):
        check_pool(m, torch.zeros_like(a), k, 'argmax always 0')


# ------------------------------------------- dispatch + coverage (no GPU)

@pytest.mark.parametrize('row', GEMM_ROWS, ids=gemm_id)
def test_gemm_dispatch_branch(ext, row):
    """Each row reaches the kernel, the split depth, the combine form and
    the empty chunks it is there for."""
    (m, n, k), want = row
    assert gemm_plan(ext, m, n, k, k, n, 0) == want


@pytest.mark.parametrize('row', LINEAR_ROWS, ids=gemm_id)
def test_linear_dispatch_branch(ext, row):
    assert linear_plans(ext, row[0]) == row[1]


@pytest.mark.parametrize('row', CONV_ROWS, ids=lambda r: sid(r[0]))
def test_conv_dispatch_branch(ext, row):
    shape, fwd, bwdd, bwdw = row
    assert py_conv_fwd_kernel(ext, shape) == fwd
    assert py_conv_bwdd_kernel(shape) == bwdd
    assert conv_bwdw_plan(ext, shape) == bwdw


def test_pool_and_mask_rows(ext):
    """The pooled rows are exactly the table rows conv_pool_fused_ok
    admits, and the masked rows span both backward-data families."""
    fused = [(s, py_conv_pool_kernel(ext, s)) for s in CONV_SHAPES]
    assert [f for f in fused if f[1] is not None] == POOL_ROWS
    kinds = {py_conv_bwdd_kernel(s).split('<')[0] for s in MASK_SHAPES}
    assert kinds == {'conv_bwd_data32_k', 'conv_bwd_data_k'}
    assert all(s in CONV_SHAPES for s in MASK_SHAPES)
    # both gather forms of each family
    assert {py_conv_bwdd_kernel(s).endswith('true>') for s in MASK_SHAPES
            if s[1] <= 32} == {True, False}
    assert {py_conv_bwdd_kernel(s).endswith('true>') for s in MASK_SHAPES
            if s[1] > 32} == {True, False}


def test_resident_plans_of_the_table(ext):
    """The three resident rows are there for three different tile plans:
    (tile_rows, tiles, mi) of conv_fwd_res_plan."""
    def plan(s):
        nb, c, h, w, ko, r, st, pad = s
        return ext.conv_fwd_res_plan(c, h, w, *out_hw(s), r)[:3]
    assert plan((3, 32, 26, 26, 64, 3, 1, 0)) == (8, 3, 6)
    assert plan((3, 32, 18, 18, 40, 3, 1, 0)) == (8, 2, 4)
    assert plan((3, 64, 15, 15, 72, 3, 1, 0)) == (0, 2, 4)


def test_small_bwdw_needs_kout_multiple_of_4(ext):
    """conv_small_bwdw_k stages dy as float4s, which must not straddle two
    pixels: only Kout % 4 == 0 may take it.  The exported workspace size
    shows which path the C predicate picks (the small path's is the 2048
    chunk slabs, whatever SK is)."""
    for ko in range(1, 70):
        for ncrs in (9, 18, 27, 32, 36):
            small = ext.conv_bwd_weight_ws_floats(ko, ncrs, 3) == \
                2048 * ko * ncrs
            assert small == py_conv_bwdw_small(ko, ncrs), (ko, ncrs)
            assert small == (ncrs <= 32 and ko <= 64 and ko % 4 == 0)
            if not small:
                assert ext.conv_bwd_weight_ws_floats(ko, ncrs, 3) == \
                    ext.conv_dwperm_ws_floats(ko, ncrs, 3)


def test_small_bwdw_staging_replayed():
    """The dy staging index arithmetic of conv_small_bwdw_k, replayed: the
    float4 at flat offset e = 4 i of the [m][ko] tile lands in rows
    ko .. ko + 3 of column m = e / KO.  It is the transpose only when
    KO % 4 == 0; at KO = 10 values of pixel m + 1 land in rows 10 and 11
    of pixel m, at KO = 62 rows 62 and 63, and at KO = 63 the rows run
    past the 64 of dy_lds."""
    def staged(ko_n, mc=128):
        lds, top = {}, 0
        for i in range(mc * ko_n // 4):
            e = 4 * i
            m = e // ko_n
            ko = e - m * ko_n
            for j in range(4):
                lds[(ko + j, m)] = e + j
                top = max(top, ko + j)
        right = all(lds.get((ko, m)) == m * ko_n + ko
                    for m in range(mc) for ko in range(ko_n))
        return right, top
    for ko_n in (4, 16, 32, 60, 64):
        assert staged(ko_n) == (True, ko_n - 1)
    assert staged(10) == (False, 11)
    assert staged(62) == (False, 63)
    assert staged(63) == (False, 65)


def launched(fname, func):
    """The kernel instantiations one launcher's body can launch, read from
    the source: `name<args><<<` and the RLR_RES(MI, POOL) macro calls."""
    with open(os.path.join(CSRC, fname)) as f:
        text = f.read()
    m = re.search(r'^[\w \*]*\b' + func + r'\(.*?^}', text, re.S | re.M)
    assert m, func
    body = m.group(0)
    out = set()
    for name, args in re.findall(r'(\w+_k)(<[^<>]*>)?<<<', body):
        if name == 'conv_fwd_res_k':
            continue  # the macro's own body; its calls are counted below
        out.add(name + re.sub(r'\s+', '', args))
    for mi, pool in re.findall(r'RLR_RES\((\d), (true|false)\)', body):
        out.add(f'conv_fwd_res_k<{mi},{pool}>')
    return out


def test_every_instantiation_is_reached(ext):
    """The branches the rows reach are exactly the instantiations the four
    launchers (and the resident forward's own) can launch: a predicate or
    a table change cannot empty a branch silently, and a new
    instantiation needs a row."""
    gemm = {gemm_plan(ext, m, n, k, k, n, 0)[0] for (m, n, k), _ in GEMM_ROWS}
    for row in LINEAR_ROWS:
        gemm |= {p[0] for p in linear_plans(ext, row[0])}
    want = launched('gemm_f32.hip', 'launch_gemm_f32_main')
    want = {'gemm_f32_k<true,false,false>' if k == 'gemm_f32_k<true>' else
            'gemm_f32_k<false,false,false>' if k == 'gemm_f32_k<false>'
            else k for k in want}
    assert len(want) == 8
    assert gemm == want

    fwd = {py_conv_fwd_kernel(ext, s) for s in CONV_SHAPES}
    fwd |= {py_conv_pool_kernel(ext, s) for s in CONV_SHAPES} - {None}
    want = launched('conv_f32.hip', 'launch_conv_fwd') | \
        launched('conv_f32.hip', 'launch_conv_fwd_res')
    assert len(want) == 10
    assert fwd == want

    bwdd = {py_conv_bwdd_kernel(s) for s in CONV_SHAPES}
    want = launched('conv_f32.hip', 'launch_conv_bwd_data_relu')
    assert len(want) == 9
    assert bwdd == want

    plans = [conv_bwdw_plan(ext, s) for s in CONV_SHAPES]
    want = launched('conv_f32.hip', 'launch_conv_bwd_weight_main')
    assert len(want) == 5
    assert {p[0] for p in plans} == want

    # the combine forms, and a split with empty chunks in each family
    gplans = [gemm_plan(ext, m, n, k, k, n, 0) for (m, n, k), _ in GEMM_ROWS]
    assert {p[2] for p in gplans} == {'direct', 'thread', 'wave',
                                      'two_level'}
    assert any(p[3] > 0 for p in gplans if p[2] == 'two_level')
    assert any(p[3] > 0 for p in gplans if p[2] == 'thread')
    assert {p[2] for p in plans} == {'chunks', 'direct', 'one_level',
                                     'two_level'}
    assert any(p[3] > 0 for p in plans)
    # a ragged last fold chunk (SK not a multiple of 16) in each family
    assert any(p[1] > 16 and p[1] % 16 for p in gplans)
    assert any(p[1] > 16 and p[1] % 16 for p in plans)


# ------------------------------------------------------------- on the GPU

def dev(t):
    t = t.to(DEV)
    if t.dim() == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    return t


@gpu
@pytest.mark.parametrize('row', GEMM_ROWS, ids=gemm_id)
def test_gemm(ext, row):
    (m, n, kk), plan = row
    k = gemm_case(m, n, kk)
    a, b = dev(k['a']), dev(k['b'])
    tag = f'gemm {sid(row[0])} [{plan[0]} {plan[2]}]'
    check(ext.gemm(a, b, None, False), k['c'], k['mag'], kk, tag + ' C')


@gpu
@pytest.mark.parametrize('row', GEMM_ROWS, ids=gemm_id)
def test_gemm_bias_relu(ext, row):
    (m, n, kk), plan = row
    k = gemm_case(m, n, kk)
    c = ext.gemm(dev(k['a']), dev(k['b']), dev(k['bias']), True)
    tag = f'gemm {sid(row[0])} [{plan[0]} {plan[2]}]'
    check(c, k['cb'], k['cb_mag'], kk + 1, tag + ' relu(C+b)')
    assert float(c.min()) >= 0.0


@gpu
@pytest.mark.parametrize('row', LINEAR_ROWS, ids=gemm_id)
def test_linear_fwd(ext, row):
    (b, i, o), plans, _ = row
    k = linear_case(b, i, o)
    x, w = dev(k['x']), dev(k['w'])
    tag = f'linear {sid(row[0])} [{plans[0][0]} {plans[0][2]}]'
    check(ext.linear_fwd(x, w, None, False), k['y'], k['y_mag'], i,
          tag + ' y')
    check(ext.linear_fwd(x, w, dev(k['bias']), True), k['yb'], k['yb_mag'],
          i + 1, tag + ' relu(y+b)')


@gpu
@pytest.mark.parametrize('row', LINEAR_ROWS, ids=gemm_id)
def test_linear_bwd(ext, row):
    (b, i, o), plans, _ = row
    k = linear_case(b, i, o)
    dx, dw, db = ext.linear_bwd(dev(k['x']), dev(k['w']), dev(k['dy']))
    s = f'linear {sid(row[0])}'
    check(dx, k['dx'], k['dx_mag'], o,
          f'{s} [{plans[1][0]} {plans[1][2]}] dx')
    check(dw, k['dw'], k['dw_mag'], b,
          f'{s} [{plans[2][0]} {plans[2][2]}] dw')
    check(db, k['db'], k['db_mag'], b, f'{s} [colsum] db')


@gpu
@pytest.mark.parametrize('row', CONV_ROWS, ids=lambda r: sid(r[0]))
def test_conv_fwd(ext, row):
    shape, kern = row[0], row[1]
    k = conv_case(shape)
    st, pad = shape[6], shape[7]
    y = ext.conv2d_fwd(dev(k['x']), dev(k['w']), None, st, pad, False)
    check(y, k['y'], k['y_mag'], k['n_y'], f'conv {sid(shape)} [{kern}] y')


@gpu
@pytest.mark.parametrize('row', CONV_ROWS, ids=lambda r: sid(r[0]))
def test_conv_fwd_bias_relu(ext, row):
    shape, kern = row[0], row[1]
    k = conv_case(shape)
    st, pad = shape[6], shape[7]
    y = ext.conv2d_fwd(dev(k['x']), dev(k['w']), dev(k['b']), st, pad, True)
    check(y, k['yb'], k['yb_mag'], k['n_y'] + 1,
          f'conv {sid(shape)} [{kern}] relu(y+b)')
    assert float(y.min()) >= 0.0


@gpu
@pytest.mark.parametrize('row', CONV_ROWS, ids=lambda r: sid(r[0]))
def test_conv_bwd(ext, row):
    shape, _, bwdd, bwdw = row
    k = conv_case(shape)
    st, pad = shape[6], shape[7]
    dx, dw, db = ext.conv2d_bwd(dev(k['x']), dev(k['w']), dev(k['dy']), st,
                                pad, True, True)
    s = f'conv {sid(shape)}'
    check(dx, k['dx'], k['dx_mag'], k['n_dx'], f'{s} [{bwdd}] dx')
    check(dw, k['dw'], k['dw_mag'], k['n_dw'],
          f'{s} [{bwdw[0]} {bwdw[2]}] dw')
    check(db, k['db'], k['db_mag'], k['n_dw'], f'{s} [conv_db] db')


@gpu
@pytest.mark.parametrize('shape', MASK_SHAPES, ids=sid)
def test_conv_bwd_into_relu_mask(ext, shape):
    """The relu_y mask epilogue of backward-data: relu_y = relu(randn) has
    many exact zeros, and those cells must come out exactly 0."""
    k = conv_case(shape)
    st, pad = shape[6], shape[7]
    assert float((k['relu_y'] == 0).float().mean()) > 0.25
    dw = torch.empty_like(k['w'], device=DEV)
    db = torch.empty_like(k['b'], device=DEV)
    dx = ext.conv2d_bwd_into(dev(k['x']), dev(k['w']), dev(k['dy']), st,
                             pad, True, dw, db, dev(k['relu_y']))
    torch.cuda.synchronize()
    s = f'conv {sid(shape)}'
    check(dx, k['dx_masked'], k['dx_mag'], k['n_dx'],
          f'{s} [{py_conv_bwdd_kernel(shape)} masked] dx')
    assert bool((dx.cpu()[k['relu_y'] == 0] == 0).all())
    check(dw, k['dw'], k['dw_mag'], k['n_dw'], f'{s} [into] dw')
    check(db, k['db'], k['db_mag'], k['n_dw'], f'{s} [into] db')


@gpu
@pytest.mark.parametrize('row', POOL_ROWS, ids=lambda r: sid(r[0]))
def test_conv_pool_fwd(ext, row):
    shape, kern = row
    k = conv_case(shape)
    pooled, idx = ext.conv2d_pool_fwd(dev(k['x']), dev(k['w']), dev(k['b']),
                                      1, 0)
    check_pool(pooled, idx, k, f'conv {sid(shape)} [{kern}]')
