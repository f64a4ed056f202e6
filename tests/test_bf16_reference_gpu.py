"""Every bf16 conv, batch-norm and element-wise kernel against an fp64
reference, element by element, inside a DERIVED error bound.

The other bf16 tests assert `mean|got - ref| / mean|ref| < 2e-2`, which a
kernel that drops one tap along one border column passes (about 1/32 of
the pixels move by about 1/9 of their size at W = 32).  Here every output
element is held to the bound below, none excluded, at the smallest shapes
that still reach every instantiation and tail of the tap family
(conv_bwdw_tap.hip) and every shape class of the batch-norm kernels.

Reference: inputs rounded the way the kernel sees them (x, dy bf16;
weights `w.to(bfloat16)`, round-to-nearest-even like the wperm_*_bf16
kernels; bias fp32), then fp64 torch.nn.functional on the CPU.

Bound, with n the number of products summed into one output and `mag`
the same convolution applied to |inputs| in fp64:

    bf16 outputs (y, dx):  |got - ref| <= 2^-8  |ref| + n 2^-23 mag
    fp32 outputs (dw, db): |got - ref| <= 2^-23 |ref| + n 2^-23 mag

Derivation: a product of two bf16 values is exact in fp32; fp32
accumulation of n terms in ANY order is within n 2^-24 mag, and the bound
keeps a factor 2 over that in case the MFMA unit does not round to
nearest internally (the slack also absorbs the second-order term of the
final rounding); the final bf16 store rounds to nearest even, within 2^-8
relative.  A fused relu is 1-Lipschitz, so relu(ref) holds the same
bound; an element whose reference lies within the bound of 0 may come out
on either side of the relu and still be inside.

The checker self-tests and the dispatch / workspace arithmetic tests run
without a GPU; everything that launches a kernel is marked `gpu`.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

DEV = 'cuda:0'
BF = torch.bfloat16
E8, E23 = 2.0 ** -8, 2.0 ** -23


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


# ------------------------------------------------------------------ checker

def worst_ratio(got, ref, mag, n, out_bf16):
    """max over ALL elements of |got - ref| / bound (inf for NaN/Inf)."""
    got = got.detach().to('cpu', torch.float64)
    ref = ref.to(torch.float64)
    rel = E8 if out_bf16 else E23
    bound = rel * ref.abs() + n * E23 * mag.to(torch.float64)
    err = (got - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).nan_to_num(nan=float('inf'))
    return ratio, err, bound


def check(got, ref, mag, n, out_bf16, what):
    """Assert every element of `got` within the derived bound of `ref`;
    returns the worst error/bound ratio."""
    assert tuple(got.shape) == tuple(ref.shape), \
        f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    want = BF if out_bf16 else torch.float32
    assert got.dtype == want, f"{what}: dtype {got.dtype}"
    ratio, err, bound = worst_ratio(got, ref, mag, n, out_bf16)
    bad = ~(err <= bound)  # NaN compares false, so it counts as bad
    worst = float(ratio.max())
    print(f"{what}: worst err/bound = {worst:.4g} over {ratio.numel()} "
          f"elements")
    if bad.any():
        flat = int(ratio.flatten().argmax())
        idx = tuple(int(i) for i in
                    torch.unravel_index(torch.tensor(flat), ratio.shape))
        g = got.detach().to('cpu', torch.float64)
        raise AssertionError(
            f"{what}: {float(bad.double().mean()):.3%} of elements over "
            f"the bound; worst at {idx}: got {float(g[idx])!r} ref "
            f"{float(ref[idx])!r} bound {float(bound[idx])!r}")
    return worst


# -------------------------------------------------------- conv shape table
# (Nb, C, H, W, Kout, stride); all 3x3 pad 1.  The three names are the
# dispatch branches the row must take (forward, backward-data,
# backward-weight); `plan` pins (S, G, chunks) of the tap backward-weight
# launch where the row is about the combine.

CONV_ROWS = [
    # tap s1 W=32 fwd / flipped bwd-data / bwd-weight, Cin != Cout
    ((3, 32, 32, 32, 64, 1), ('tap', 'tap', 'tap_s1'), None),
    # W=16, two 32-channel chunks
    ((3, 64, 16, 16, 32, 1), ('tap', 'tap', 'tap_s1'), None),
    # W=8, odd Nb on the two-image block
    ((3, 64, 8, 8, 32, 1), ('tap', 'tap', 'tap_s1'), None),
    ((1, 32, 8, 8, 32, 1), ('tap', 'tap', 'tap_s1'), None),
    # packed W=4 kernel, 4-images-per-block tail
    ((5, 32, 4, 4, 64, 1), ('w4', 'w4', 'generic'), None),
    ((2, 64, 4, 4, 32, 1), ('w4', 'w4', 'generic'), None),
    # tap bwd-weight with H != W; fwd / bwd-data fall to the generic form
    ((2, 32, 12, 8, 32, 1), ('generic', 'generic', 'tap_s1'), None),
    ((2, 32, 8, 16, 32, 1), ('generic', 'generic', 'tap_s1'), None),
    # stride 2: bwdd_s2 W=32 + bwdw_tap_s2 OW=16
    ((3, 32, 32, 32, 64, 2), ('generic', 'tap_s2', 'tap_s2'), None),
    # bwdd_s2 W=16, generic bwd-weight
    ((3, 64, 16, 16, 32, 2), ('generic', 'tap_s2', 'generic'), None),
    # bwdd_s2 W=8
    ((3, 32, 8, 8, 64, 2), ('generic', 'tap_s2', 'generic'), None),
    # two-stage combine with a ragged last chunk (17 = 16 + 1), s1 and s2
    ((17, 32, 8, 8, 32, 1), ('tap', 'tap', 'tap_s1'), (17, 1, 2)),
    ((17, 32, 32, 32, 32, 2), ('generic', 'tap_s2', 'tap_s2'), (17, 1, 2)),
    # slab cap: G = 2 image groups, the last one short (9 = 2*4 + 1)
    ((9, 512, 8, 8, 512, 1), ('tap', 'tap', 'tap_s1'), (5, 2, 0)),
    # chunks = 17: one more chunk slab than the old fixed 16 spare slabs
    ((257, 32, 4, 8, 32, 1), ('generic', 'generic', 'tap_s1'),
     (257, 1, 17)),
]
CONV_SHAPES = [r[0] for r in CONV_ROWS]


def sid(s):
    return 'x'.join(str(v) for v in s)


# The five dispatch predicates of conv_bwdw_tap.hip, mirrored.  They MUST
# track the C ones (test_predicates_track_c compares them on every row);
# all take the 3x3 pad-1 case of this table for granted.

def py_tap_fwd_w4_ok(cin, h, w, cout, stride):
    return stride == 1 and cin % 32 == 0 and cout % 32 == 0 and \
        w == 4 and h == 4


def py_tap_fwd_ok(cin, h, w, cout, stride):
    return stride == 1 and cin % 32 == 0 and cout % 32 == 0 and \
        w in (8, 16, 32) and h == w


def py_tap_bwdd_s2_ok(c, h, w, ko, stride):
    return stride == 2 and c % 32 == 0 and ko % 32 == 0 and \
        w in (8, 16, 32) and h == w


def py_bwdw_tap_ok(c, h, w, ko, stride):
    return stride == 1 and c % 32 == 0 and ko % 32 == 0 and \
        w in (8, 16, 32) and h % (32 // w) == 0


def py_bwdw_tap_s2_ok(c, h, w, ko, stride):
    return stride == 2 and c % 32 == 0 and ko % 32 == 0 and \
        w // 2 == 16 and h == w and (h // 2) % 2 == 0


def branches(shape):
    """(forward, backward-data, backward-weight) branch of a table shape,
    in the order conv2d_fwd / conv2d_bwd / bf16_dw test the predicates
    (bindings.cpp).  Backward-data runs the forward tap kernels with the
    channel roles swapped."""
    nb, c, h, w, ko, st = shape
    if py_tap_fwd_w4_ok(c, h, w, ko, st):
        fwd = 'w4'
    elif py_tap_fwd_ok(c, h, w, ko, st):
        fwd = 'tap'
    else:
        fwd = 'generic'
    if py_tap_fwd_w4_ok(ko, h, w, c, st):
        bwdd = 'w4'
    elif py_tap_fwd_ok(ko, h, w, c, st):
        bwdd = 'tap'
    elif py_tap_bwdd_s2_ok(c, h, w, ko, st):
        bwdd = 'tap_s2'
    else:
        bwdd = 'generic'
    if py_bwdw_tap_ok(c, h, w, ko, st):
        bwdw = 'tap_s1'
    elif py_bwdw_tap_s2_ok(c, h, w, ko, st):
        bwdw = 'tap_s2'
    else:
        bwdw = 'generic'
    return fwd, bwdd, bwdw


# ---------------------------------------------------------- conv reference

def seed_of(*ints):
    s = 17
    for v in ints:
        s = (s * 1000003 + v) % (2 ** 31 - 1)
    return s


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def conv_case(shape, R=3, pad=1):
    """Inputs and fp64 references of one shape, computed once on the CPU
    and shared (read-only) by every test that needs them."""
    nb, c, h, w, ko, st = shape
    g = torch.Generator().manual_seed(seed_of(*shape, R))
    oh = (h + 2 * pad - R) // st + 1
    ow = (w + 2 * pad - R) // st + 1
    x = torch.randn(nb, c, h, w, generator=g).to(BF)
    wt = torch.randn(ko, c, R, R, generator=g) * 0.05
    b = torch.randn(ko, generator=g)
    dy = torch.randn(nb, ko, oh, ow, generator=g).to(BF)
    relu_y = torch.relu(torch.randn(nb, c, h, w, generator=g)).to(BF)
    wb = wt.to(BF)  # what the wperm_*_bf16 kernels feed the MFMA

    def run(x_, w_, dy_):
        x_ = x_.clone().requires_grad_(True)
        w_ = w_.clone().requires_grad_(True)
        y_ = F.conv2d(x_, w_, None, stride=st, padding=pad)
        dx_, dw_ = torch.autograd.grad(y_, (x_, w_), dy_)
        return y_.detach(), dx_, dw_, dy_.sum((0, 2, 3))

    d = torch.float64
    y, dx, dw, db = run(x.to(d), wb.to(d), dy.to(d))
    ym, dxm, dwm, dbm = run(x.to(d).abs(), wb.to(d).abs(), dy.to(d).abs())
    bd = b.to(d).view(1, -1, 1, 1)
    return dict(
        shape=shape, R=R, pad=pad, x=x, w=wt, wb=wb, b=b, dy=dy,
        relu_y=relu_y,
        n_y=c * R * R + 1, n_dx=ko * R * R, n_dw=nb * oh * ow,
        y=y, y_mag=ym, yb=torch.relu(y + bd), yb_mag=ym + bd.abs(),
        dx=dx, dx_mag=dxm, dx_masked=dx * (relu_y > 0),
        dw=dw, dw_mag=dwm, db=db, db_mag=dbm)


def torch_fp32_conv(case):
    """torch's own fp32 CPU conv + backward on the same rounded inputs:
    the stand-in 'kernel' of the checker self-tests."""
    st, pad = case['shape'][5], case['pad']
    x = case['x'].float().requires_grad_(True)
    w = case['wb'].float().requires_grad_(True)
    b = case['b'].clone().requires_grad_(True)
    y = F.conv2d(x, w, None, stride=st, padding=pad)
    yb = torch.relu(F.conv2d(x, w, b, stride=st, padding=pad))
    dx, dw = torch.autograd.grad(y, (x, w), case['dy'].float())
    db = case['dy'].float().sum((0, 2, 3))
    return y.detach(), yb.detach(), dx, dw, db


# ------------------------------------------ checker self-tests (CPU only)

@pytest.mark.parametrize('shape', CONV_SHAPES, ids=sid)
def test_checker_accepts_torch_fp32(shape):
    """(a) torch's fp32 conv, rounded once to bf16, is inside the bound at
    every shape: the reference alone stays inside it.  (Its bf16 outputs
    reach 0.83-0.98 of the bound at C <= 64 and 0.36-0.42 at C = 512,
    where the n-term takes a larger share; the printed ratios show it.)"""
    k = conv_case(shape)
    y, yb, dx, dw, db = torch_fp32_conv(k)
    check(y.to(BF), k['y'], k['y_mag'], k['n_y'], True, 'y')
    check(yb.to(BF), k['yb'], k['yb_mag'], k['n_y'], True, 'y+b relu')
    check(dx.to(BF), k['dx'], k['dx_mag'], k['n_dx'], True, 'dx')
    check(dw, k['dw'], k['dw_mag'], k['n_dw'], False, 'dw')
    check(db, k['db'], k['db_mag'], k['n_dw'], False, 'db')


MUTANT_SHAPES = [(3, 32, 32, 32, 64, 1), (3, 64, 8, 8, 32, 1),
                 (2, 32, 12, 8, 32, 1), (5, 32, 4, 4, 64, 1),
                 (3, 32, 32, 32, 64, 2)]


def _tap_only(k, r, s):
    """fp32 conv of the case's inputs with every tap but (r, s) zeroed."""
    w1 = torch.zeros_like(k['wb'].float())
    w1[:, :, r, s] = k['wb'].float()[:, :, r, s]
    return F.conv2d(k['x'].float(), w1, None, stride=k['shape'][5],
                    padding=1)


def _rejected(got, ref, mag, n):
    with pytest.raises(AssertionError, match='over the bound'):
        check(got, ref, mag, n, True, 'mutant')


@pytest.mark.parametrize('shape', MUTANT_SHAPES, ids=sid)
def test_checker_rejects_mutants(shape):
    """(b) the bugs these kernels can have, planted in torch's fp32
    output: each must put at least one element over the bound."""
    k = conv_case(shape)
    nb, c, h, w, ko, st = shape
    y, _, dx, _, _ = torch_fp32_conv(k)
    args = (k['y'], k['y_mag'], k['n_y'])
    check(y.to(BF), *args, True, 'unmutated')

    # one tap dropped on the first column only (tap s=2 reads real data
    # there; s=0 would read the zero halo and change nothing)
    m = y.clone()
    m[..., 0] -= _tap_only(k, 1, 2)[..., 0]
    _rejected(m.to(BF), *args)
    # one tap dropped on the last row only
    m = y.clone()
    m[:, :, -1, :] -= _tap_only(k, 0, 1)[:, :, -1, :]
    _rejected(m.to(BF), *args)
    # the last image left as zeros (an Nb-tail bug)
    m = y.clone()
    m[-1] = 0
    _rejected(m.to(BF), *args)
    # one 32-channel chunk skipped
    m = F.conv2d(k['x'].float()[:, :c - 32], k['wb'].float()[:, :c - 32],
                 None, stride=st, padding=1) if c > 32 else \
        torch.zeros_like(y)
    _rejected(m.to(BF), *args)
    # weights used with C and Kout transposed
    if c == ko:
        m = F.conv2d(k['x'].float(), k['wb'].float().transpose(0, 1), None,
                     stride=st, padding=1)
        _rejected(m.to(BF), *args)
    # the relu_y mask ignored in backward-data
    check((dx * (k['relu_y'] > 0)).to(BF), k['dx_masked'], k['dx_mag'],
          k['n_dx'], True, 'masked dx')
    _rejected(dx.to(BF), k['dx_masked'], k['dx_mag'], k['n_dx'])


def test_mutant_shapes_cover_transposed_case():
    assert any(s[1] == s[4] for s in MUTANT_SHAPES)
    assert all(s in CONV_SHAPES for s in MUTANT_SHAPES)


# -------------------------------- dispatch + workspace arithmetic (no GPU)

@pytest.mark.parametrize('row', CONV_ROWS, ids=lambda r: sid(r[0]))
def test_dispatch_branch(ext, row):
    """Each table row reaches the kernels it is there for: a later change
    to a predicate must not silently empty a row."""
    shape, want, plan = row
    assert branches(shape) == want
    if plan is not None:
        nb, c, _, _, ko, _ = shape
        S, G, chunks, slabs = ext.conv_bwdw_tap_ws_slabs(nb, c, ko)
        assert (S, G, chunks) == plan
        assert slabs == S + chunks


# shapes on the predicates' edges, beyond the table's
EDGE_SHAPES = [(2, 32, 16, 8, 32, 1), (2, 32, 6, 8, 32, 1),
               (2, 32, 64, 64, 32, 2), (2, 32, 16, 16, 64, 2),
               (2, 32, 4, 4, 32, 2), (2, 48, 8, 8, 32, 1)]


@pytest.mark.parametrize('shape', CONV_SHAPES + EDGE_SHAPES, ids=sid)
def test_predicates_track_c(ext, shape):
    """The Python mirrors above equal the C predicates, both channel
    orders (backward-data calls the forward predicates swapped)."""
    nb, c, h, w, ko, st = shape
    for a, b in ((c, ko), (ko, c)):
        t = (a, h, w, b, 3, 3, st, 1)
        p = (a, h, w, b, st)
        assert ext.conv_tap_fwd_w4_ok(*t) == py_tap_fwd_w4_ok(*p)
        assert ext.conv_tap_fwd_ok(*t) == py_tap_fwd_ok(*p)
        assert ext.conv_tap_bwdd_s2_ok(*t) == py_tap_bwdd_s2_ok(*p)
        assert ext.conv_bwdw_tap_ok(*t) == py_bwdw_tap_ok(*p)
        assert ext.conv_bwdw_tap_s2_ok(*t) == py_bwdw_tap_s2_ok(*p)
    # not 3x3 / pad 1: no tap kernel
    assert not ext.conv_tap_fwd_ok(c, h, w, ko, 1, 1, st, 0)
    assert not ext.conv_bwdw_tap_ok(c, h, w, ko, 3, 3, st, 0)


def test_bwdw_tap_workspace_covers_every_slab(ext):
    """The tap backward-weight launchers write S image-group slabs plus,
    when S > 16, ceil(S/16) chunk sums past them.  The workspace bf16_dw
    allocates (the 4th value) must hold all of them, and the S groups of
    G images must cover the batch.  A fixed 16 spare slabs was too few
    for S > 256."""
    for c in (32, 64, 128, 256, 512):
        for ko in (32, 64, 128, 256, 512):
            for nb in range(1, 2049):
                S, G, chunks, slabs = ext.conv_bwdw_tap_ws_slabs(nb, c, ko)
                touched = S + (-(-S // 16) if S > 16 else 0)
                assert chunks == (touched - S), (nb, c, ko)
                assert touched <= slabs, (nb, c, ko, S, slabs)
                assert S >= 1 and G >= 1 and G * S >= nb, (nb, c, ko)
                assert (S - 1) * G < nb, (nb, c, ko)  # no empty group
                # the slab cap (64 MiB of fp32 partials) still holds
                assert S == 1 or S * ko * c * 36 <= 64 << 20, (nb, c, ko)


# --------------------------------------------------------- conv on the GPU

def dev(t):
    t = t.to(DEV)
    return cl(t) if t.dim() == 4 else t


@gpu
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=sid)
def test_conv_fwd(ext, shape):
    k = conv_case(shape)
    st = shape[5]
    y = ext.conv2d_fwd(dev(k['x']), dev(k['w']), None, st, 1, False)
    check(y, k['y'], k['y_mag'], k['n_y'], True, f'{sid(shape)} y')


@gpu
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=sid)
def test_conv_fwd_bias_relu(ext, shape):
    k = conv_case(shape)
    st = shape[5]
    y = ext.conv2d_fwd(dev(k['x']), dev(k['w']), dev(k['b']), st, 1, True)
    check(y, k['yb'], k['yb_mag'], k['n_y'], True,
          f'{sid(shape)} relu(y+b)')
    assert float(y.float().min()) >= 0.0


@gpu
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=sid)
def test_conv_bwd(ext, shape):
    k = conv_case(shape)
    st = shape[5]
    dx, dw, db = ext.conv2d_bwd(dev(k['x']), dev(k['w']), dev(k['dy']), st,
                                1, True, True)
    s = sid(shape)
    check(dx, k['dx'], k['dx_mag'], k['n_dx'], True, f'{s} dx')
    check(dw, k['dw'], k['dw_mag'], k['n_dw'], False, f'{s} dw')
    check(db, k['db'], k['db_mag'], k['n_dw'], False, f'{s} db')


# one shape per backward-data branch of conv2d_bwd_wdx_into:
# (shape, R, pad, branch)
WDX_ROWS = [
    ((5, 32, 4, 4, 64, 1), 3, 1, 'w4'),
    ((3, 32, 32, 32, 64, 1), 3, 1, 'tap'),
    ((3, 32, 32, 32, 64, 2), 3, 1, 'tap_s2'),
    ((3, 32, 8, 8, 64, 2), 1, 0, 'generic'),   # 1x1 s2 shortcut conv
]
SENTINEL = -12345.0


def test_wdx_rows_reach_each_branch():
    for shape, R, pad, want in WDX_ROWS:
        got = branches(shape)[1] if R == 3 else 'generic'
        assert got == want, shape
    assert {r[3] for r in WDX_ROWS} == {'w4', 'tap', 'tap_s2', 'generic'}


@gpu
@pytest.mark.parametrize('row', WDX_ROWS, ids=lambda r: r[3])
def test_conv_bwd_wdx_into_relu_mask(ext, row):
    """The relu_y mask epilogue of every backward-data branch (relu_y =
    relu(randn) has many exact zeros), and dw written into a slice of a
    larger flat buffer without touching its neighbours."""
    shape, R, pad, _ = row
    k = conv_case(shape, R, pad)
    st = shape[5]
    n_w = k['w'].numel()
    flat = torch.full((n_w + 128,), SENTINEL, device=DEV)
    dw_out = flat[64:64 + n_w]
    assert float((k['relu_y'] == 0).float().mean()) > 0.25
    dx = ext.conv2d_bwd_wdx_into(dev(k['x']), dev(k['w']), dev(k['dy']), st,
                                 pad, True, dw_out, dev(k['relu_y']))
    torch.cuda.synchronize()
    s = sid(shape)
    check(dx, k['dx_masked'], k['dx_mag'], k['n_dx'], True, f'{s} masked dx')
    assert bool((dx.float().cpu()[k['relu_y'] == 0] == 0).all())
    check(dw_out.view_as(k['w']), k['dw'], k['dw_mag'], k['n_dw'], False,
          f'{s} dw_out')
    assert bool((flat[:64] == SENTINEL).all())
    assert bool((flat[64 + n_w:] == SENTINEL).all())


# -------------------------------------------------------------- batch-norm
# fp32 outputs keep the tolerances of test_batchnorm_train_fwd_bwd
# (test_kernels_gpu.py); bf16 y and dx add the final rounding, 2^-8 |ref|.
# save_mean / save_rstd are not compared there.  Their tolerances follow
# from the running-stat ones: running_mean moves by momentum * mean, so
# its atol 1e-5 at momentum 0.1 is atol 1e-4 on the batch mean; rstd has
# half the relative error of the variance, which carries running_var's
# rtol 1e-4.

BN_SHAPES = [
    (8, 512, 4, 4),    # C > 256: two y-blocks, bn_grid rounding
    (4, 48, 6, 6),     # non-power-of-two C; M = 144, ragged chunks
    (9, 32, 64, 64),   # M = 36864, above the 2048-chunk cap
    (1, 64, 2, 2),     # M = 4, below the 64-chunk floor
]
MOM, EPS = 0.1, 1e-5


def close(got, ref, rtol, atol, what, bf16=False, scale=1.0):
    got = got.detach().to('cpu', torch.float64)
    ref = ref.to(torch.float64)
    assert got.shape == ref.shape, what
    tol = scale * (atol + rtol * ref.abs()) + (E8 * ref.abs() if bf16 else 0)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    print(f"{what}: worst err/tol = {float((err / tol).max()):.4g}")
    if bad.any():
        flat = int((err / tol).nan_to_num(float('inf')).flatten().argmax())
        idx = tuple(int(i) for i in
                    torch.unravel_index(torch.tensor(flat), err.shape))
        raise AssertionError(
            f"{what}: {float(bad.double().mean()):.3%} over tolerance; "
            f"worst at {idx}: got {float(got[idx])!r} ref "
            f"{float(ref[idx])!r} tol {float(tol[idx])!r}")


@functools.lru_cache(maxsize=None)
def bn_case(shape, dtype, mu=0.0):
    nb, c, h, w = shape
    g = torch.Generator().manual_seed(
        seed_of(*shape, int(dtype == BF), int(mu)))
    x = (mu + torch.randn(nb, c, h, w, generator=g)).to(dtype)
    dy = torch.randn(nb, c, h, w, generator=g).to(dtype)
    wt = torch.rand(c, generator=g) + 0.5
    b = torch.randn(c, generator=g)
    rm = torch.randn(c, generator=g)
    rv = torch.rand(c, generator=g) + 0.5
    d = torch.float64
    xg = x.to(d).requires_grad_(True)
    wg = wt.to(d).requires_grad_(True)
    bg = b.to(d).requires_grad_(True)
    rm_t, rv_t = rm.to(d), rv.to(d)
    y = F.batch_norm(xg, rm_t, rv_t, wg, bg, True, MOM, EPS)
    dx, dw, db = torch.autograd.grad(y, (xg, wg, bg), dy.to(d))
    mean = x.to(d).mean((0, 2, 3))
    var = x.to(d).var((0, 2, 3), unbiased=False)
    y_eval = F.batch_norm(x.to(d), rm.to(d), rv.to(d), wt.to(d), b.to(d),
                          False, MOM, EPS)
    return dict(x=x, dy=dy, w=wt, b=b, rm=rm, rv=rv, y=y.detach(),
                y_eval=y_eval, rm_t=rm_t, rv_t=rv_t, mean=mean,
                rstd=(var + EPS).rsqrt(), dx=dx, dw=dw, db=db)


def bn_id(v):
    if isinstance(v, tuple):
        return sid(v)
    return 'bf16' if v == BF else 'fp32' if v == torch.float32 else str(v)


def run_bn_train(ext, k, relu, scale=1.0, tag=''):
    bf = k['x'].dtype == BF
    rm, rv = dev(k['rm'].clone()), dev(k['rv'].clone())
    y, sm, sr = ext.batchnorm_fwd(dev(k['x']), dev(k['w']), dev(k['b']),
                                  rm, rv, MOM, EPS, True, relu)
    assert y.dtype == k['x'].dtype
    ref = torch.relu(k['y']) if relu else k['y']
    close(y, ref, 1e-4, 1e-4, tag + 'bn y', bf, scale)
    close(rm, k['rm_t'], 1e-5, 1e-5, tag + 'running mean', scale=scale)
    close(rv, k['rv_t'], 1e-4, 1e-5, tag + 'running var', scale=scale)
    close(sm, k['mean'], 1e-5, 1e-4, tag + 'save_mean', scale=scale)
    close(sr, k['rstd'], 1e-4, 1e-5, tag + 'save_rstd', scale=scale)
    return sm, sr


@gpu
@pytest.mark.parametrize('relu', [False, True], ids=['plain', 'relu'])
@pytest.mark.parametrize('dtype', [BF, torch.float32], ids=bn_id)
@pytest.mark.parametrize('shape', BN_SHAPES, ids=bn_id)
def test_bn_train_fwd(ext, shape, dtype, relu):
    run_bn_train(ext, bn_case(shape, dtype), relu)


@gpu
@pytest.mark.parametrize('relu', [False, True], ids=['plain', 'relu'])
@pytest.mark.parametrize('dtype', [BF, torch.float32], ids=bn_id)
@pytest.mark.parametrize('shape', BN_SHAPES, ids=bn_id)
def test_bn_eval_fwd(ext, shape, dtype, relu):
    k = bn_case(shape, dtype)
    rm, rv = dev(k['rm'].clone()), dev(k['rv'].clone())
    y, sm, sr = ext.batchnorm_fwd(dev(k['x']), dev(k['w']), dev(k['b']),
                                  rm, rv, MOM, EPS, False, relu)
    ref = torch.relu(k['y_eval']) if relu else k['y_eval']
    close(y, ref, 1e-4, 1e-4, 'bn eval y', dtype == BF)
    # eval leaves the running statistics alone and saves them as the stats
    assert torch.equal(rm.cpu(), k['rm']) and torch.equal(rv.cpu(), k['rv'])
    assert torch.equal(sm.cpu(), k['rm'])
    close(sr, (k['rv'].double() + EPS).rsqrt(), 1e-4, 1e-5, 'eval rstd')


def run_bn_bwd(ext, k, scale=1.0, tag=''):
    bf = k['x'].dtype == BF
    sm, sr = run_bn_train(ext, k, False, scale, tag)
    x, w, dy = dev(k['x']), dev(k['w']), dev(k['dy'])
    dx, dw, db = ext.batchnorm_bwd(x, w, sm, sr, dy)
    assert dx.dtype == k['x'].dtype and dw.dtype == torch.float32
    close(dx, k['dx'], 1e-3, 1e-4, tag + 'bn dx', bf, scale)
    close(dw, k['dw'], 1e-3, 1e-3, tag + 'bn dw', scale=scale)
    close(db, k['db'], 1e-3, 1e-3, tag + 'bn db', scale=scale)

    # the manual-tape form: dw/db land in slices of a flat buffer, the
    # neighbours stay untouched, the values are the same kernels' values
    c = k['w'].numel()
    flat = torch.full((2 * c + 192,), SENTINEL, device=DEV)
    dw_o, db_o = flat[64:64 + c], flat[128 + c:128 + 2 * c]
    dx2 = ext.batchnorm_bwd_into(x, w, sm, sr, dy, dw_o, db_o)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx)
    assert torch.equal(dw_o, dw) and torch.equal(db_o, db)
    for lo, hi in ((0, 64), (64 + c, 128 + c), (128 + 2 * c, 192 + 2 * c)):
        assert bool((flat[lo:hi] == SENTINEL).all()), (lo, hi)


@gpu
@pytest.mark.parametrize('dtype', [BF, torch.float32], ids=bn_id)
@pytest.mark.parametrize('shape', BN_SHAPES, ids=bn_id)
def test_bn_bwd_and_bwd_into(ext, shape, dtype):
    run_bn_bwd(ext, bn_case(shape, dtype))


@gpu
@pytest.mark.parametrize('dtype', [BF, torch.float32], ids=bn_id)
def test_bn_large_mean(ext, dtype):
    """Input mu + sigma * randn with mu/sigma = 4.  The kernel's variance
    is the single-pass E[x^2] - mean^2: E[x^2] is (1 + (mu/sigma)^2) times
    the variance it is there to find, so the rounding of the fp32 sums is
    amplified by that factor in the variance and in everything computed
    from it.  The tolerances are therefore multiplied by 1 + 4^2 = 17, and
    by no more."""
    run_bn_bwd(ext, bn_case((8, 64, 8, 8), dtype, 4.0), scale=17.0,
               tag='mu/sigma=4 ')


# ------------------------------------------------------- bf16 element-wise

EW_SHAPE = (3, 40, 6, 6)   # C = 40: not a power of two, 8 | C
EW_FLAT = 4099             # odd: exercises the 8-wide kernels' tail


def ew_inputs(n_tensors, shape, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_tensors):
        out.append(dev(torch.randn(shape, generator=g).to(BF)))
    return out


def same_bits(got, want_f32, what):
    """`got` (bf16) equals the fp32 result rounded ONCE to bf16, bit for
    bit (+0 and -0 both count as zero: relu of -x may carry either)."""
    assert got.dtype == BF, what
    want = want_f32.to(BF)
    assert got.shape == want.shape, what
    assert not bool(torch.isnan(got.float()).any()), what
    g16 = got.contiguous().view(torch.int16)
    w16 = want.contiguous().view(torch.int16)
    both_zero = (got.contiguous().float() == 0) & \
        (want.contiguous().float() == 0)
    ok = (g16 == w16) | both_zero
    assert bool(ok.all()), \
        f"{what}: {int((~ok).sum())} of {ok.numel()} elements differ"


EW_SHAPES = [EW_SHAPE, EW_FLAT]


@gpu
@pytest.mark.parametrize('shape', EW_SHAPES, ids=['nhwc', 'flat_odd'])
def test_ew_relu_add_family_bitwise(ext, shape):
    """One operation, one rounding: bitwise equal to the fp32 op on the
    up-cast inputs rounded once."""
    a, b, c = ew_inputs(3, shape, 7)
    y = ext.relu_fwd(a)
    same_bits(y, torch.relu(a.float()), 'relu_fwd')
    same_bits(ext.relu_bwd(y, b), b.float() * (y.float() > 0), 'relu_bwd')
    same_bits(ext.add_relu_fwd(a, b), torch.relu(a.float() + b.float()),
              'add_relu_fwd')
    a2 = a.clone()
    r = ext.add_(a2, b)
    same_bits(a2, a.float() + b.float(), 'add_')
    assert r.data_ptr() == a2.data_ptr()
    a3 = a.clone()
    ry = torch.relu(c)
    ext.add_relu_bwd_(a3, b, ry)
    same_bits(a3, (a.float() + b.float()) * (ry.float() > 0),
              'add_relu_bwd_')


def first_max_2x2(x):
    """2x2/2 max-pool of fp32 NCHW x with the FIRST maximum of each window
    in (00, 01, 10, 11) order as argmax — torch's tie rule too."""
    v = [x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2],
         x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]]
    m, a = v[0].clone(), torch.zeros_like(v[0], dtype=torch.uint8)
    for i in (1, 2, 3):
        gt = v[i] > m
        m = torch.where(gt, v[i], m)
        a = torch.where(gt, torch.full_like(a, i), a)
    return m, a


@gpu
def test_ew_maxpool_bitwise(ext):
    x, = ew_inputs(1, EW_SHAPE, 8)
    y, idx = ext.maxpool2x2_fwd(x)
    m, a = first_max_2x2(x.float())
    same_bits(y, m, 'maxpool fwd')
    assert torch.equal(y.float(), F.max_pool2d(x.float(), 2))
    assert torch.equal(idx, a), 'maxpool argmax'
    dy, = ew_inputs(1, tuple(y.shape), 9)
    dx = ext.maxpool2x2_bwd(dy, idx, list(x.shape))
    want = torch.zeros_like(x, dtype=torch.float32)
    for i, (r, s) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        want[:, :, r::2, s::2] = dy.float() * (a == i)
    same_bits(dx, want, 'maxpool bwd')


@gpu
def test_ew_gap_within_bound(ext):
    """Global average pool: HW-term fp32 sum, one division, one rounding:
    |got - ref| <= 2^-8 |ref| + HW 2^-23 mean|x|."""
    x, ry = ew_inputs(2, EW_SHAPE, 10)
    nb, c, h, w = EW_SHAPE
    hw = h * w
    x64 = x.double().cpu()
    y = ext.gap_fwd(x)
    assert tuple(y.shape) == (nb, c)
    check(y, x64.mean((2, 3)), x64.abs().mean((2, 3)), hw, True, 'gap_fwd')

    dy, = ew_inputs(1, (nb, c), 11)
    d64 = dy.double().cpu()
    ref = (d64 / hw).view(nb, c, 1, 1).expand(nb, c, h, w)
    mag = d64.abs().view(nb, c, 1, 1).expand(nb, c, h, w)
    dx = ext.gap_bwd(dy, list(EW_SHAPE))
    check(dx, ref, mag, hw, True, 'gap_bwd')
    ry = torch.relu(ry)
    mask = (ry.double().cpu() > 0)
    dxr = ext.gap_bwd_relu(dy, ry, list(EW_SHAPE))
    check(dxr, ref * mask, mag, hw, True, 'gap_bwd_relu')
    assert bool((dxr.float().cpu()[~mask] == 0).all())
