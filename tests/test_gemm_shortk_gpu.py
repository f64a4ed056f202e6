"""The short-K form of the fp32 tile GEMM (gemm_f32_shortk_k, gemm_f32.hip)
against the kernel it replaces, bit for bit.

An fp32 MFMA is a k-ordered fmaf chain per output; the short-K form keeps
gemm_f32_k's chunk boundaries, its ascending k order inside a chunk and the
split-K fold, so C must come out with the SAME BITS, signed zeros included.
Every GPU case runs the new form, then the old one in the same process under
RLR_AMD_NO_GEMM_SHORTK=1 (read by the launcher on every call), compares the
raw int32 views, and holds each result to the fp64 bound of
test_fp32_reference_gpu.py (2^-23 |ref| + n 2^-23 mag) as well: "equal to
another path of ours" alone would pass a bug both share.

The routing predicate gemm_f32_shortk_tiles is host arithmetic and is pinned
without a GPU, together with the branch every GPU row is in the table for.
"""

import functools

import pytest
import torch

from test_fp32_reference_gpu import cdiv, check, seed_of

gpu = pytest.mark.gpu

DEV = 'cuda:0'
D = torch.float64
BK = 32
SWITCH = 'RLR_AMD_NO_GEMM_SHORTK'


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


def gemm_dims(kind, dims):
    """(M, N, K, lda, ldb) of the launch behind one Python entry point."""
    if kind == 'gemm':          # C (m,n) = A (m,k) B (k,n): layout 0
        m, n, k = dims
        return m, n, k, k, n
    b, i, o = dims
    if kind == 'fwd':           # y = x w^T: layout 2, w (out,in) as B^T
        return b, o, i, i, i
    if kind == 'dx':            # dx = dy w: layout 0
        return b, i, o, o, i
    assert kind == 'dw'         # dw = dy^T x: layout 1, dy as A^T
    return o, i, b, o, i


def plan(ext, kind, dims):
    """(SK, tiles of the short-K form or 0, tiles in the last non-empty
    chunk, empty chunks) of one call."""
    m, n, k, lda, ldb = gemm_dims(kind, dims)
    sk = ext.gemm_f32_splitk(m, n, k)
    t = ext.gemm_f32_shortk_tiles(m, n, k, sk, lda, ldb)
    kpc = k if sk == 1 else cdiv(cdiv(k, sk), BK) * BK
    used = cdiv(k, kpc)
    return sk, t, cdiv(k - (used - 1) * kpc, BK), sk - used


# (entry point, dims, (SK, T, tiles in the last chunk, empty chunks)).
# dims: (M, N, K) for gemm, (B, in, out) for the linear entry points.
ROWS = [
    # NN, SK = 1, direct_out epilogue, 4 tiles; M tail 2, N tail 24
    ('gemm', (130, 6104, 128), (1, 4, 4, 0)),
    # NN, K = 100: the last of 4 tiles holds 4 k rows (K guard)
    ('gemm', (130, 6104, 100), (1, 4, 4, 0)),
    # NN split, 3-tile chunks, a 2-tile last chunk; M tail 2, N tail 4
    ('gemm', (130, 68, 6100), (64, 3, 2, 0)),
    # fc1 forward at batch 37: B transposed, 3-tile chunks, 32 empty chunks
    ('fwd', (37, 9216, 128), (128, 3, 3, 32)),
    # B transposed, 5-tile chunks (k_per_chunk = 160), a 3-tile last chunk
    # whose last tile holds 4 k columns, 25 empty chunks
    ('fwd', (37, 16388, 128), (128, 5, 3, 25)),
    # fc1's dW narrowed: A transposed, SK = 2, chunk 128, M tail 4; K = 250
    # leaves 26 k rows in the second chunk's last tile
    ('dw', (250, 4036, 132), (2, 4, 4, 0)),
    # the dx of the same layer: NN split, 3 tiles then 2 (K = 132)
    ('dx', (250, 4036, 132), (2, 3, 2, 0)),
]


def row_id(r):
    return f'{r[0]}-' + 'x'.join(str(v) for v in r[1])


# --------------------------------------------------------- CPU: the predicate

def test_predicate_is_zero_outside_its_range(ext):
    f = ext.gemm_f32_shortk_tiles
    # 1- and 2-tile chunks (SK = 1 and split)
    assert f(300, 300, 32, 1, 32, 300) == 0
    assert f(300, 300, 40, 1, 40, 300) == 0
    assert f(300, 300, 64, 1, 64, 300) == 0
    assert ext.gemm_f32_splitk(256, 512, 600) == 16   # chunk 64
    assert f(256, 512, 600, 16, 600, 512) == 0
    assert f(37, 9216, 128, 2, 128, 9216) == 0        # fc1 dx at batch 37
    # 6 tiles
    assert f(130, 6104, 192, 1, 192, 6104) == 0
    assert f(130, 6104, 161, 1, 164, 6104) == 0
    # a row stride that is no multiple of 4
    assert f(130, 6104, 128, 1, 130, 6104) == 0
    assert f(130, 6104, 128, 1, 128, 6106) == 0
    # the tiny-problem branch never reaches the tile kernels
    assert f(64, 70, 100, 1, 100, 72) == 0
    assert f(100, 32, 128, 1, 128, 32) == 0
    # 3, 4 and 5 tiles are in
    assert f(300, 300, 65, 1, 68, 300) == 3
    assert f(130, 6104, 160, 1, 160, 6104) == 5


def test_predicate_at_the_fc1_shapes(ext):
    assert plan(ext, 'fwd', (256, 9216, 128)) == (64, 5, 3, 6)
    assert plan(ext, 'dx', (256, 9216, 128))[:2] == (1, 4)
    assert plan(ext, 'dw', (256, 9216, 128))[:2] == (2, 4)
    # batch 112: SK = 128, chunk 96
    assert plan(ext, 'fwd', (112, 9216, 128))[:2] == (128, 3)


@pytest.mark.parametrize('row', ROWS, ids=row_id)
def test_row_takes_its_branch(ext, row):
    kind, dims, want = row
    assert plan(ext, kind, dims) == want


def test_rows_cover_every_case(ext):
    plans = {(r[0], r[2]) for r in ROWS}
    kinds = {r[0] for r in ROWS}
    assert kinds == {'gemm', 'fwd', 'dx', 'dw'}           # NN, BT, NN, AT
    assert {p[1] for _, p in plans} == {3, 4, 5}          # every depth
    assert any(p[0] == 1 for _, p in plans)               # direct_out
    assert any(p[2] < p[1] for _, p in plans)             # short last chunk
    assert any(p[3] > 0 for _, p in plans)                # empty chunks


# -------------------------------------------------------------- references

@functools.lru_cache(maxsize=None)
def case(kind, dims):
    """Inputs on the CPU and the fp64 reference / magnitude of the one
    product the row is about, computed once and shared read-only."""
    g = torch.Generator().manual_seed(seed_of(*dims, len(kind)))
    if kind == 'gemm':
        m, n, k = dims
        a = torch.randn(m, k, generator=g)
        b = torch.randn(k, n, generator=g) * 0.05
        bias = torch.randn(n, generator=g)
        ref = a.to(D) @ b.to(D)
        mag = a.to(D).abs() @ b.to(D).abs()
        return dict(a=a, b=b, bias=bias, n=k, ref=ref, mag=mag)
    b, i, o = dims
    x = torch.randn(b, i, generator=g)
    w = torch.randn(o, i, generator=g) * 0.05
    bias = torch.randn(o, generator=g)
    dy = torch.randn(b, o, generator=g)
    x6, w6, d6 = x.to(D), w.to(D), dy.to(D)
    if kind == 'fwd':
        ref, mag, n = x6 @ w6.t(), x6.abs() @ w6.abs().t(), i
    elif kind == 'dx':
        ref, mag, n = d6 @ w6, d6.abs() @ w6.abs(), o
    else:
        ref, mag, n = d6.t() @ x6, d6.abs().t() @ x6.abs(), b
    return dict(x=x, w=w, bias=bias, dy=dy, n=n, ref=ref, mag=mag)


def run(ext, kind, k, bias_relu):
    """One call through the row's entry point: the product the row checks."""
    if kind == 'gemm':
        return ext.gemm(k['a'].to(DEV), k['b'].to(DEV),
                        k['bias'].to(DEV) if bias_relu else None, bias_relu)
    x, w = k['x'].to(DEV), k['w'].to(DEV)
    if kind == 'fwd':
        return ext.linear_fwd(x, w, k['bias'].to(DEV) if bias_relu else None,
                              bias_relu)
    dw = torch.empty_like(w)
    dx = ext.linear_bwd_into(x, w, k['dy'].to(DEV), dw, None, kind == 'dx')
    return dx if kind == 'dx' else dw


def both(ext, monkeypatch, kind, k, bias_relu):
    monkeypatch.delenv(SWITCH, raising=False)
    new = run(ext, kind, k, bias_relu)
    monkeypatch.setenv(SWITCH, '1')
    old = run(ext, kind, k, bias_relu)
    monkeypatch.delenv(SWITCH)
    torch.cuda.synchronize()
    return new, old


def same_bits(new, old, what):
    assert new.dtype == torch.float32 and old.dtype == torch.float32
    ne = new.view(torch.int32) != old.view(torch.int32)
    print(f'shortk {what}: {int(ne.sum())} of {ne.numel()} words differ')
    assert torch.equal(new.view(torch.int32), old.view(torch.int32)), what


# ------------------------------------------------------------- on the GPU

@gpu
@pytest.mark.parametrize('row', ROWS, ids=row_id)
def test_bits_equal_old_kernel(ext, monkeypatch, row):
    kind, dims, _ = row
    k = case(kind, dims)
    new, old = both(ext, monkeypatch, kind, k, False)
    what = row_id(row)
    same_bits(new, old, what)
    check(new, k['ref'], k['mag'], k['n'], what + ' short-K')
    check(old, k['ref'], k['mag'], k['n'], what + ' gemm_f32_k')


@gpu
@pytest.mark.parametrize('row', [r for r in ROWS if r[0] in ('gemm', 'fwd')],
                         ids=row_id)
def test_bias_relu_bits_equal_old_kernel(ext, monkeypatch, row):
    """bias + relu in the direct_out epilogue (SK = 1) and through the
    split-K reduce (SK > 1)."""
    kind, dims, _ = row
    k = case(kind, dims)
    new, old = both(ext, monkeypatch, kind, k, True)
    what = row_id(row) + ' relu(.+b)'
    same_bits(new, old, what)
    ref = torch.relu(k['ref'] + k['bias'].to(D))
    mag = k['mag'] + k['bias'].to(D).abs()
    check(new, ref, mag, k['n'] + 1, what + ' short-K')
    check(old, ref, mag, k['n'] + 1, what + ' gemm_f32_k')
    assert float(new.min()) >= 0.0


@gpu
def test_signed_zeros_survive(ext, monkeypatch):
    """An all-zero product: +0 everywhere on both paths (the MFMA chain
    starts from +0 and the empty chunks' slabs are +0), and a column of A
    negated against a zero B keeps whatever sign the old kernel gives."""
    m, n, kk = 130, 6104, 128
    a = -torch.ones(m, kk, device=DEV)
    b = torch.zeros(kk, n, device=DEV)
    b[:, ::2] = -0.0
    k = dict(a=a, b=b, bias=None)
    new, old = both(ext, monkeypatch, 'gemm', k, False)
    same_bits(new, old, 'signed zeros')
    assert float(new.abs().max()) == 0.0
