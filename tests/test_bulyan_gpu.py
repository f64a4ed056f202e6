"""Bulyan on the GPU: the fused select-and-trim kernel (bulyan_k in
ops/csrc/orderstat.hip) bitwise against the CPU rule, its vote and fused
apply, the device selection loop given D, the server on both backends, the
binding's argument checks and the driver.
Every test needs an MI355X: run with `pytest -m gpu`."""

import functools

import pytest
import torch

import server_helpers
from bulyan_helpers import (SHAPES, counts, gather_select, graded, ints,
                            selected_first)
from server_helpers import P as _P, randn

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N = server_helpers.N
SMALL_N = [1, 3, 33]
SMALL_N_SHAPES = [(3, 0), (10, 1), (21, 1), (338, 33)]


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


make_agg = functools.partial(server_helpers.make_agg, aggr='bulyan')


def window_mean(rows, beta):
    from rlr_amd.aggregation import bulyan_window_mean
    return bulyan_window_mean(rows, beta)


def data(kind, K, n=N):
    return ints(K, n) if kind == 'ints' else randn(K, n)


@functools.lru_cache(maxsize=None)
def scattered(K, f):
    """A RANDOM perm: theta rows scattered over U in no order first, the
    rest behind them, shuffled too."""
    g = torch.Generator().manual_seed(97 * K + f)
    theta, _ = counts(K, f)
    sel = torch.randperm(K, generator=g)[:theta]
    perm = selected_first(sel, K, generator=g)
    assert sorted(perm.tolist()) == list(range(K))
    return perm


@functools.lru_cache(maxsize=None)
def cpu_trim(kind, K, f, n=N):
    """The CPU stage 2 over the scattered rows; computed once."""
    theta, beta = counts(K, f)
    rows = data(kind, K, n)[scattered(K, f)[:theta].long()]
    return window_mean(rows, beta)


@functools.lru_cache(maxsize=None)
def cpu_graded(K, f):
    """The CPU server's answers on graded(K, f) and the independent
    selection with its smallest score gap, computed once:
    (selection, aggregate, independent picks, gap)."""
    U, _ = graded(K, f)
    agg = make_agg(N, 'cpu', bulyan_f=f)
    D = agg.pairwise_sqdist(U)
    sel = agg.bulyan_picks(D)
    return (sel, agg._bulyan_trim(U, sel)) + gather_select(D, f)


# ----------------------------------------------------- stage 2, the kernel

@pytest.mark.parametrize("kind", ['ints', 'randn'])
@pytest.mark.parametrize("K,f", SHAPES)
def test_trim_bitwise_against_cpu_rule(ext, K, f, kind):
    theta, beta = counts(K, f)
    U = data(kind, K).to(DEV)
    out, lr = ext.bulyan_trim(U, scattered(K, f).to(DEV), theta, beta, False,
                              0.0, 0.0)
    assert out.shape == (N,) and out.dtype == torch.float64
    assert lr.numel() == 0
    assert torch.equal(out.cpu(), cpu_trim(kind, K, f))


@pytest.mark.parametrize("kind", ['ints', 'randn'])
@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("K,f", SMALL_N_SHAPES)
def test_trim_bitwise_small_n(ext, K, f, n, kind):
    theta, beta = counts(K, f)
    U = data(kind, K, n).to(DEV)
    out = ext.bulyan_trim(U, scattered(K, f).to(DEV), theta, beta, False,
                          0.0, 0.0)[0]
    assert torch.equal(out.cpu(), cpu_trim(kind, K, f, n))


@pytest.mark.parametrize("K,f", [(10, 1), (40, 4)])
def test_trim_does_not_depend_on_the_order_inside_perm(ext, K, f):
    theta, beta = counts(K, f)
    U = randn(K).to(DEV)
    perm = scattered(K, f)
    tidy = torch.cat([perm[:theta].sort().values, perm[theta:].sort().values])
    a = ext.bulyan_trim(U, perm.to(DEV), theta, beta, False, 0.0, 0.0)[0]
    b = ext.bulyan_trim(U, tidy.to(DEV), theta, beta, False, 0.0, 0.0)[0]
    assert torch.equal(a, b)


# ------------------------------------------------------------------ the vote

@pytest.mark.parametrize("kind", ['ints', 'randn'])
@pytest.mark.parametrize("K,f", SHAPES)
def test_lr_is_rlr_vote_over_all_rows(ext, K, f, kind):
    theta, beta = counts(K, f)
    U = data(kind, K).to(DEV)
    thresh = float(max(1, K // 5))
    out, lr = ext.bulyan_trim(U, scattered(K, f).to(DEV), theta, beta, True,
                              thresh, 0.7)
    assert torch.equal(lr, ext.rlr_vote(U, thresh, 0.7))
    assert torch.equal(out.cpu(), cpu_trim(kind, K, f))
    assert set(lr.unique().tolist()) <= {0.7, -0.7}


@pytest.mark.parametrize("K,f", [(10, 1), (21, 1), (67, 16), (512, 127)])
def test_unselected_rows_decide_the_vote(ext, K, f):
    """The selected rows cancel (or nearly: theta odd leaves +-1), the
    K - theta unselected rows all agree: only a vote that counts them
    reaches the threshold."""
    theta, beta = counts(K, f)
    perm = scattered(K, f)
    U = torch.empty(K, 65, dtype=torch.float64)
    signs = torch.tensor([1.0, -1.0]).repeat(theta)[:theta]
    U[perm[:theta].long()] = signs.unsqueeze(1) * (1.0 + randn(theta, 65).abs())
    U[perm[theta:].long()] = -(1.0 + randn(K - theta, 65).abs())
    U = U.to(DEV)
    thresh = float(K - theta - 1)
    assert thresh > 1
    _, lr = ext.bulyan_trim(U, perm.to(DEV), theta, beta, True, thresh, 1.0)
    assert (lr == 1.0).all()
    assert torch.equal(lr, ext.rlr_vote(U, thresh, 1.0))
    # and the selected rows alone would not have carried it
    assert (ext.rlr_vote(U[perm[:theta].long().to(DEV)].contiguous(), thresh,
                         1.0) == -1.0).all()


# ----------------------------------------------------------- the fused apply

@pytest.mark.parametrize("rlr", [False, True])
@pytest.mark.parametrize("K,f", SHAPES)
def test_fused_apply_equals_the_composition(ext, K, f, rlr):
    theta, beta = counts(K, f)
    U = randn(K).to(DEV)
    perm = scattered(K, f).to(DEV)
    thresh = float(max(1, K // 5))
    g = torch.Generator().manual_seed(K)
    start = torch.randn(N, generator=g).to(DEV)
    fused = start.clone()
    lr = ext.bulyan_rlr_apply(U, perm, theta, beta, fused, rlr, thresh, 1.0,
                              True)
    composed = start.clone()
    vote = (ext.rlr_vote(U, thresh, 1.0) if rlr
            else torch.empty(0, device=DEV))
    agg = ext.bulyan_trim(U, perm, theta, beta, False, 0.0, 0.0)[0]
    ext.apply_update(composed, agg, vote, 1.0)
    assert torch.equal(fused, composed)
    assert not torch.equal(fused, start)
    if rlr:
        assert torch.equal(lr, vote)
    else:
        assert (lr == 1.0).all()
    none = ext.bulyan_rlr_apply(U, perm, theta, beta, start.clone(), rlr,
                                thresh, 1.0, False)
    assert none.numel() == 0


# ---------------------------------------------------- selection, given D

@pytest.mark.parametrize("kind", ['ints', 'graded'])
@pytest.mark.parametrize("K,f", SHAPES)
def test_selection_given_D(ext, K, f, kind):
    U = ints(K) if kind == 'ints' else graded(K, f)[0]
    D = ext.pairwise_sqdist(U.to(DEV))
    got = make_agg(N, DEV, bulyan_f=f).bulyan_picks(D)
    want = make_agg(N, 'cpu', bulyan_f=f).bulyan_picks(D.cpu())
    assert got.dtype == torch.long and got.is_cuda
    assert torch.equal(got.cpu(), want)
    if K <= 67:     # the larger K are compared in the CPU suite
        assert want.tolist() == gather_select(D.cpu(), f)[0]


# ------------------------------------------------------------- end to end

@pytest.mark.parametrize("K,f", SHAPES)
def test_server_gpu_matches_cpu_on_graded(K, f):
    from rlr_amd.flatmodel import FlatParamModel
    U, bad = graded(K, f)
    want, _, picks, gap = cpu_graded(K, f)
    # the test's own precondition, on the CPU reference: every pick is
    # decided by a margin above what the two backends' distances can differ
    # by: 2 scores x the Gram form's 4 n 2^-53 (|u_i|^2 + |u_j|^2)
    bound = 2 * 4.0 * N * 2.0 ** -53 * 2 * float((U * U).sum(1).max())
    print(f"K={K} f={f}: min score gap {gap:.3e}, bound {bound:.3e}")
    assert picks == want.tolist()
    assert gap > bound, "ambiguous input"
    assert not set(picks) & set(bad.tolist())

    ids = list(range(K))
    theta, _ = counts(K, f)
    vote = 0 if K % 2 else max(1, K // 5)
    out, sel = {}, {}
    for dev in ('cpu', DEV):
        gm = FlatParamModel(_P(N), dev)
        agg = make_agg(N, dev, bulyan_f=f, robustLR_threshold=vote)
        agg.aggregate_updates(gm, U.to(dev), cur_round=1, agent_ids=ids)
        out[dev] = gm.flat_params.detach().cpu()
        sel[dev] = agg.last_selected.cpu()
    assert torch.equal(sel[DEV], sel['cpu']) and torch.equal(sel[DEV], want)
    assert len(sel[DEV]) == theta
    assert not set(sel[DEV].tolist()) & set(bad.tolist())
    assert out[DEV].abs().sum() > 0
    assert torch.allclose(out[DEV], out['cpu'], rtol=1e-6, atol=1e-7), \
        f"max|d|={float((out[DEV] - out['cpu']).abs().max())}"


@pytest.mark.parametrize("K,f", SHAPES)
def test_agg_bulyan_bitwise_between_backends(K, f):
    U, _ = graded(K, f)
    want, ref, _, _ = cpu_graded(K, f)
    agg = make_agg(N, DEV, bulyan_f=f)
    out = agg.agg_bulyan(U.to(DEV))
    assert torch.equal(agg.last_selected.cpu(), want)
    assert torch.equal(out.cpu(), ref)


def test_one_fused_launch_is_the_composed_path(ext):
    """The server's fused route (no noise) and its composed route (what
    noise takes) leave the same parameters."""
    from rlr_amd.flatmodel import FlatParamModel
    K, f = 21, 1
    U, _ = graded(K, f)
    Ug = U.to(DEV)
    gm = FlatParamModel(_P(N), DEV)
    agg = make_agg(N, DEV, bulyan_f=f, robustLR_threshold=4)
    agg.aggregate_updates(gm, Ug, cur_round=1, agent_ids=list(range(K)))
    composed = torch.zeros(N, device=DEV)
    ext.apply_update(composed, agg.agg_bulyan(Ug), agg.compute_robustLR(Ug),
                     1.0)
    assert torch.equal(gm.flat_params.detach(), composed)
    # with noise the server still answers, and differently
    gm2 = FlatParamModel(_P(N), DEV)
    noisy = make_agg(N, DEV, bulyan_f=f, robustLR_threshold=4, noise=0.1,
                     clip=1.0)
    noisy.aggregate_updates(gm2, Ug, cur_round=1, agent_ids=list(range(K)))
    assert torch.isfinite(gm2.flat_params).all()
    assert not torch.equal(gm2.flat_params.detach(), composed)


def test_buffers_use_the_selection():
    from rlr_amd.flatmodel import FlatParamModel

    class BN(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(N))
            self.register_buffer('b', torch.zeros(3))

    K, f = 10, 1
    U, _ = graded(K, f)
    agg = make_agg(N, DEV, bulyan_f=f)
    gm = FlatParamModel(BN(), DEV)
    ids = list(range(K))
    agg.aggregate_updates(gm, U.to(DEV), cur_round=1, agent_ids=ids)
    sel = agg.last_selected.tolist()
    deltas = torch.full((K, 3), 1e6)
    deltas[sel] = 3.0
    agg.aggregate_buffers(gm, deltas.to(DEV), ids)
    assert gm.flat_buffers.tolist() == [3.0, 3.0, 3.0]


# --------------------------------------------------------- argument checks

def test_argument_checks(ext):
    assert ext.bulyan_max_k() == 512
    K, n, theta, beta = 7, 8, 3, 1
    U = randn(K, n).to(DEV)
    perm = torch.arange(K, dtype=torch.int32, device=DEV)
    params = torch.zeros(n, device=DEV)
    ext.bulyan_trim(U, perm, theta, beta, False, 0.0, 0.0)
    ext.bulyan_rlr_apply(U, perm, theta, beta, params, False, 0.0, 1.0, False)

    def both(U=U, perm=perm, theta=theta, beta=beta, params=params):
        with pytest.raises(RuntimeError):
            ext.bulyan_trim(U, perm, theta, beta, False, 0.0, 0.0)
        with pytest.raises(RuntimeError):
            ext.bulyan_rlr_apply(U, perm, theta, beta, params, False, 0.0,
                                 1.0, False)

    both(U=U.float())
    both(U=U.cpu())
    both(U=randn(n, K).to(DEV).T)                   # transposed view
    both(U=U[0])                                    # 1-d
    both(perm=perm[:-1])                            # bad length
    both(perm=torch.arange(K + 1, dtype=torch.int32, device=DEV))
    both(perm=perm.long())                          # bad dtype
    both(perm=perm.cpu())
    both(perm=torch.arange(2 * K, dtype=torch.int32, device=DEV)[::2])
    both(beta=theta + 1)
    both(beta=0)
    both(theta=K + 1, beta=1)
    with pytest.raises(RuntimeError):
        ext.bulyan_rlr_apply(U, perm, theta, beta, params.double(), False,
                             0.0, 1.0, False)
    with pytest.raises(RuntimeError):
        ext.bulyan_rlr_apply(U, perm, theta, beta, params[:-1], False, 0.0,
                             1.0, False)


def test_above_the_limit_the_binding_raises_and_the_server_answers(ext):
    K = ext.bulyan_max_k() + 1
    f, n = 127, 8
    theta, beta = counts(K, f)
    U = randn(K, n)
    perm = torch.arange(K, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        ext.bulyan_trim(U.to(DEV), perm, theta, beta, False, 0.0, 0.0)
    with pytest.raises(RuntimeError):
        ext.bulyan_rlr_apply(U.to(DEV), perm, theta, beta,
                             torch.zeros(n, device=DEV), False, 0.0, 1.0,
                             False)
    # the server takes the torch rule on the device; given the same
    # selection it is the CPU rule bit for bit
    from rlr_amd.flatmodel import FlatParamModel
    agg = make_agg(n, DEV, bulyan_f=f, table=K)
    gm = FlatParamModel(_P(n), DEV)
    agg.aggregate_updates(gm, U.to(DEV), cur_round=1, agent_ids=list(range(K)))
    sel = agg.last_selected.cpu()
    assert sel.numel() == theta
    assert torch.equal(gm.flat_params.detach().cpu(),
                       window_mean(U[sel], beta).float())


# ------------------------------------------------------------------ driver

def test_bulyan_aggregation_gpu_end_to_end(monkeypatch):
    import rlr_amd.data.datasets as D
    from rlr_amd.federated import run
    from rlr_amd.options import default_args
    monkeypatch.setitem(D.DEFAULT_SIZES, 'cifar10', (4000, 400))
    h = run(default_args(num_agents=7, rounds=1, snap=1, local_ep=1, bs=128,
                         synthetic=True, no_tb=True, device=DEV,
                         data='cifar10', aggr='bulyan', bulyan_f=1))
    assert torch.isfinite(h['final_params']).all()
