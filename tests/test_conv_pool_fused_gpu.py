"""conv2's pooled epilogue and the seam forward from pooled input: raw bits
against the unfused kernels they replace (signed zeros included), and the
plain resident forward under its tile plan against a golden written by the
commit before the plan existed.

Shapes (Nb, C, H, W, Kout), 3x3 stride 1 pad 0, the smallest that reach
each path:
  (2, 32, 26, 26, 64)  three full 192-pixel tiles per image (MI = 6)
  (3, 32, 14, 14, 64)  144 pixels: a partial last 128-pixel tile, odd Nb
  (1, 64, 12, 20, 32)  two K-tiles per tap; Kout below BN; H != W
  (2, 32, 18, 18, 96)  128-pixel whole-row tiles, a half-filled N block
  (2, 32, 15, 15, 64)  13x13 output: the fallback through the same binding
Inputs are small integers, so exact ties inside a window and windows that
are negative everywhere are common: the select order and the relu's 0.f
both decide bits."""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [
    (2, 32, 26, 26, 64),
    (3, 32, 14, 14, 64),
    (1, 64, 12, 20, 32),
    (2, 32, 18, 18, 96),
    (2, 32, 15, 15, 64),
]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'conv_fwd_res_1x32x26x26_k64.npy')


def _bits(t):
    t = t.contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _int_case(shape, seed):
    """Integer-valued x, w, b: every partial sum is exact, ties abound and
    the strongly negative bias makes whole windows negative."""
    nb, c, h, w, kout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (nb, c, h, w), generator=g).float()
    wgt = torch.randint(-1, 2, (kout, c, 3, 3), generator=g).float()
    b = torch.randint(-12, 5, (kout,), generator=g).float()
    x = x.cuda().contiguous(memory_format=torch.channels_last)
    return x, wgt.cuda(), b.cuda()


@pytest.fixture(scope='module')
def E():
    from rlr_amd.ops import ext
    return ext()


@pytest.fixture(scope='module')
def cases(E):
    """Per shape: the inputs and the unfused reference, computed once."""
    out = {}
    for i, shape in enumerate(SHAPES):
        x, w, b = _int_case(shape, 11 + i)
        a2 = E.conv2d_fwd(x, w, b, 1, 0, True)
        pooled, idx = E.maxpool2x2_fwd(a2)
        out[shape] = (x, w, b, a2, pooled, idx)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_conv_pool_bitwise(E, cases, shape):
    x, w, b, a2, pooled, idx = cases[shape]
    p2, i2 = E.conv2d_pool_fwd(x, w, b, 1, 0)
    assert _same(p2, pooled)
    assert i2.dtype == torch.uint8 and _same(i2, idx)
    # the cases do what the docstring says: ties, and all-negative windows
    # (pooled == +0 after the relu) next to positive ones
    assert (pooled == 0).any() and (pooled > 0).any()
    nb, k, oh, ow = a2.shape
    if oh % 2 == 0 and ow % 2 == 0:
        win = a2.reshape(nb, k, oh // 2, 2, ow // 2, 2)
        ties = ((win == pooled[:, :, :, None, :, None]).sum((3, 5)) > 1)
        assert (ties & (pooled > 0)).any()


def test_conv_pool_without_bias_and_with_given_wt(E, cases):
    shape = SHAPES[0]
    x, w, b, _, _, _ = cases[shape]
    ref = E.maxpool2x2_fwd(E.conv2d_fwd(x, w, None, 1, 0, True))
    got = E.conv2d_pool_fwd(x, w, None, 1, 0)
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    wt = w.permute(2, 3, 1, 0).contiguous().reshape(-1, w.shape[0])
    got = E.conv2d_pool_fwd(x, w, None, 1, 0, wt)
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])


def test_predicate_matches_the_cases(E):
    fused = [bool(E.conv_pool_fused_ok(c, h, w, k, 3, 3, 1, 0))
             for (_, c, h, w, k) in SHAPES]
    assert fused == [True, False, False, True, False]


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_seam_from_pooled_bitwise(E, cases, shape):
    _, _, _, a2, pooled, _ = cases[shape]
    st = torch.tensor([1234, 40], dtype=torch.int64, device='cuda')
    pl, _, d_ref, m_ref = E.pool_flatten_dropout_fwd(a2, 0.5, st, 3)
    assert _same(pl, pooled)
    d, m = E.flatten_dropout_fwd(pooled, 0.5, st, 3)
    assert _same(d, d_ref) and _same(m, m_ref)
    assert 0 < int(m.sum()) < m.numel()


def _golden_inputs():
    rs = np.random.RandomState(20240)
    x = rs.standard_normal((1, 32, 26, 26)).astype(np.float32)
    w = (rs.standard_normal((64, 32, 3, 3)) * 0.1).astype(np.float32)
    b = rs.standard_normal((64,)).astype(np.float32)
    return x, w, b


def test_plain_forward_matches_parent_golden(E):
    """conv2d_fwd (no relu) at the flagship image size, MI = 6 tiles,
    against the NCHW-ordered output of the 128-pixel kernel."""
    x, w, b = _golden_inputs()
    y = E.conv2d_fwd(torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(),
                     torch.from_numpy(b).cuda(), 1, 0, False)
    got = y.contiguous().cpu().numpy()
    want = np.load(GOLDEN)
    assert got.shape == want.shape == (1, 64, 24, 24)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_manual_step_matches_autograd_batch3():
    """CNN_MNIST.manual_step (pooled conv2 epilogue, seam from pooled
    input) against the autograd path at batch 3: loss and every gradient
    bitwise."""
    from rlr_amd.flatmodel import FlatParamModel
    from rlr_amd.models import CNN_MNIST
    from rlr_amd.ops import functional as Fo

    g = torch.Generator().manual_seed(5)
    X = torch.randn(3, 1, 28, 28, generator=g).cuda()
    Y = torch.randint(0, 10, (3,), generator=g).cuda()
    res = []
    for manual in (False, True):
        torch.manual_seed(7)
        gm = FlatParamModel(CNN_MNIST(), 'cuda:0')
        gm.train()
        gm.set_dropout_seed(99)
        gm.ensure_grad_views()
        if manual:
            loss = gm.model.manual_step(X, Y, gm.dloss_ones())
        else:
            gm.zero_grad()
            loss = Fo.cross_entropy(gm(X), Y)
            loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().reshape(()).clone(),
                    gm.flat_grads.clone()))
    (l_auto, g_auto), (l_man, g_man) = res
    assert _same(l_auto, l_man)
    assert g_man.abs().max() > 0
    assert _same(g_auto, g_man), (g_auto - g_man).abs().max().item()
