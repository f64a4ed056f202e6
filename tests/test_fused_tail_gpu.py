"""Fused tail kernels (ops/csrc/fused_tail.hip) against the kernel sequences
they replace: every output bit for bit, signed zeros included.

Each case runs the fused entry point and the unfused sequence on the same
seeded inputs with the same dropout state and site.  The two CPU-runnable
tests pin the host-side dispatch predicates and the workspace size."""

import itertools

import pytest
import torch

P = 0.5
SEED, BASE = 1234567, 48     # dropout state: seed, base offset


@pytest.fixture(scope='module')
def E():
    from rlr_amd.ops import ext
    return ext()


def bits_equal(a, b):
    """torch.equal on the raw bits (so -0.0 != 0.0), same logical shape."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _state():
    return torch.tensor([SEED, BASE], dtype=torch.int64, device='cuda')


# ------------------------------------------------------------ host only

def _tiny(m, n, k):
    # launch_gemm_f32's tiny-problem branch
    return m * n * k <= 8_000_000 and m * n <= 65536


def test_head_predicate_and_workspace(E):
    Bs = (1, 5, 31, 32, 112, 256, 512, 513, 600, 65536, 65537)
    Hs = (1, 20, 31, 32, 70, 128, 256, 1024, 9216)
    Cs = (1, 7, 10, 31, 32, 40, 64, 65, 128)
    seen = set()
    for B, H, C in itertools.product(Bs, Hs, Cs):
        want = (C <= 64 and _tiny(B, C, H)       # forward  (M=B, N=C, K=H)
                and _tiny(B, H, C)               # dx       (M=B, N=H, K=C)
                and _tiny(C, H, B))              # dW       (M=C, N=H, K=B)
        assert bool(E.fc_head_fused_ok(B, H, C)) == want, (B, H, C)
        seen.add(want)
        # dropped activations + dlogits + row losses
        assert E.fc_head_ws_floats(B, H, C) == B * H + B * C + B, (B, H, C)
    assert seen == {True, False}
    # the edge of M*N <= 65536 in the dx GEMM
    assert E.fc_head_fused_ok(512, 128, 10)
    assert not E.fc_head_fused_ok(513, 128, 10)
    assert E.fc_head_ws_floats(256, 128, 10) == 35584


def test_seam_predicate(E):
    tile = 9600     # floats of the kernels' static LDS tile, rows of C + 1
    for C, H, W in itertools.product((1, 4, 6, 8, 64, 256, 512),
                                     (1, 2, 4, 7, 24, 26, 32),
                                     (1, 2, 6, 10, 24, 26)):
        ohw = (H // 2) * (W // 2)
        want = C % 4 == 0 and ohw > 0 and ohw * (C + 1) <= tile
        assert bool(E.pool_seam_fused_ok(C, H, W)) == want, (C, H, W)
    assert E.pool_seam_fused_ok(64, 24, 24)       # CNN_MNIST: 144 x 65
    assert E.pool_seam_fused_ok(256, 4, 4)        # CNN_CIFAR: 4 x 257
    assert not E.pool_seam_fused_ok(64, 26, 26)   # 169 x 65 > tile
    assert not E.pool_seam_fused_ok(6, 4, 4)


# ------------------------------------------------------------- the seam

SEAM_SHAPES = [
    (3, 64, 24, 24),   # MNIST tile, odd B
    (5, 256, 4, 4),    # CIFAR tile
    (2, 8, 7, 6),      # odd H; OHW = 9: philox groups cross channel rows
    (1, 4, 6, 6),      # small image, B = 1
    (1, 4, 6, 10),     # 60 pooled elements, tile not square
    (2, 6, 4, 4),      # C % 4 != 0: fallback
]


def _seam_inputs(shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(B * 1000003 + C * 1009 + H * 31 + W)
    # post-relu activations on a coarse grid: exact zeros and ties inside
    # the 2x2 windows (first maximum must win)
    a = torch.round(torch.randn(B, C, H, W, generator=g) * 4).clamp_(min=0) / 4
    a = a.cuda().contiguous(memory_format=torch.channels_last)
    gr = torch.randn(B, C * (H // 2) * (W // 2), generator=g).cuda()
    return a, gr


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SEAM_SHAPES, ids=str)
def test_seam_forward_backward(E, shape):
    B, C, H, W = shape
    OH, OW = H // 2, W // 2
    a, gr = _seam_inputs(shape)
    st, site = _state(), 3
    assert bool(E.pool_seam_fused_ok(C, H, W)) == (C % 4 == 0)

    pl0, idx0 = E.maxpool2x2_fwd(a)
    d0, m0 = E.dropout_fwd_dev(E.nhwc_flatten(pl0), P, st, site)
    pl1, idx1, d1, m1 = E.pool_flatten_dropout_fwd(a, P, st, site)
    assert bits_equal(pl1, pl0)
    assert bits_equal(idx1, idx0)
    assert bits_equal(d1, d0)
    assert bits_equal(m1, m0)
    assert pl1.is_contiguous(memory_format=torch.channels_last) or C == 1
    assert 0 < int(m0.sum()) < m0.numel()      # a real mask, not all-or-none

    gu = E.nhwc_unflatten(E.dropout_bwd(gr, m0, P), C, OH, OW)
    if C % 4 == 0:
        dx0 = E.maxpool2x2_bwd_relu(gu, idx0, pl0, list(a.shape))
    else:   # the relu-mask gather needs C % 4 == 0
        dx0 = E.maxpool2x2_bwd(E.relu_bwd(pl0, gu), idx0, list(a.shape))
    dx1 = E.dropout_unflatten_pool_bwd_relu(gr, m0, idx0, pl0, P,
                                            list(a.shape))
    assert bits_equal(dx1, dx0)
    if H % 2:   # odd tail row lies outside every window
        assert not dx1[:, :, H - 1, :].any()
    torch.cuda.synchronize()


# ------------------------------------------------------------- the head

HEAD_SHAPES = [
    (256, 128, 10),    # the workload's full batch
    (112, 128, 10),    # ... and its last batch
    (40, 256, 10),     # CIFAR head
    (5, 128, 10),      # B < 32: dW in the thread form
    (3, 70, 7),        # H no multiple of 64 or 4
    (8, 64, 40),       # C >= 32: dx in the wave form
    (4, 20, 5),        # H < 32: forward in the thread form
    (600, 128, 10),    # B*H > 65536: predicate false, unfused sequence
]


def _head_unfused(E, h1, w, b, labels, dloss, st, site):
    dw, db = torch.empty_like(w), torch.empty_like(b)
    d2, m2 = E.dropout_fwd_dev(h1, P, st, site)
    out = E.linear_fwd(d2, w, b, False)
    loss, softmax = E.cross_entropy_fwd(out, labels)
    g = E.cross_entropy_bwd(softmax, labels, dloss)
    g = E.linear_bwd_into(d2, w, g, dw, db, True)
    g = E.dropout_relu_bwd(g, m2, h1, P)
    return loss, g, dw, db


@pytest.mark.gpu
@pytest.mark.parametrize('shape', HEAD_SHAPES, ids=str)
def test_head_step(E, shape):
    B, H, C = shape
    g = torch.Generator().manual_seed(B * 7919 + H * 13 + C)
    h1 = torch.randn(B, H, generator=g).clamp_(min=0).cuda()   # post-relu
    w = (torch.randn(C, H, generator=g) / H ** 0.5).cuda()
    b = torch.randn(C, generator=g).cuda()
    labels = torch.randint(0, C, (B,), generator=g).cuda()
    dloss = torch.full((1,), 0.75, device='cuda')
    st, site = _state(), 1
    assert bool(E.fc_head_fused_ok(B, H, C)) == (shape != (600, 128, 10))

    loss0, g0, dw0, db0 = _head_unfused(E, h1, w, b, labels, dloss, st, site)
    # grads land in views of one flat buffer, as in the manual tape
    flat = torch.full((C * H + C + 8,), float('nan'), device='cuda')
    dw1 = flat[4:4 + C * H].view(C, H)
    db1 = flat[4 + C * H:4 + C * H + C]
    loss1, g1 = E.fc_head_step(h1, w, b, labels, dloss, P, st, site, dw1, db1)
    assert bits_equal(loss1, loss0)
    assert bits_equal(g1, g0)
    assert bits_equal(dw1, dw0)
    assert bits_equal(db1, db0)
    # nothing written outside the two views
    assert flat[:4].isnan().all() and flat[4 + C * H + C:].isnan().all()
    assert torch.isfinite(loss1).all() and g1.any()
    torch.cuda.synchronize()
