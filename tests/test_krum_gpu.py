"""fp64 MFMA pairwise-distance kernel (ops/csrc/pairdist.hip) and the Krum
server path on top of it: exact-integer layout checks, the structure of D,
accuracy against the CPU direct-difference rule, scores and selection
bitwise given D, selection end to end, the server on both backends, the
argument checks and the driver.
Every test needs an MI355X: run with `pytest -m gpu`."""

import functools

import pytest
import torch

import server_helpers
from server_helpers import P as _P, clustered, randn

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N = 4099   # prime and odd: every second row of U is only 8-byte aligned,
           # and every 32-column slab sequence ends in a tail
EXACT_K = [1, 2, 3, 15, 16, 17, 65, 338, 512]
ACC_K = [4, 10, 17, 65, 338, 512]
KF = [(4, 1), (10, 2), (65, 10), (338, 33), (512, 100)]


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


make_agg = functools.partial(server_helpers.make_agg, aggr='krum')


# ------------------------------------------------------------------ inputs
# CPU tensors, built once and never modified; tests move copies to the GPU

@functools.lru_cache(maxsize=None)
def ints(K, n=N):
    g = torch.Generator().manual_seed(7 * K + n)
    return torch.randint(-3, 4, (K, n), generator=g).double()


def gram_sqdist(U):
    """CPU fp64 Gram form, as the kernel computes it."""
    G = U @ U.T
    g = G.diagonal()
    D = (g.unsqueeze(1) + g.unsqueeze(0)) - 2.0 * G
    D = D.clamp(min=0.0)
    D.fill_diagonal_(0.0)
    return D


@functools.lru_cache(maxsize=None)
def direct_sqdist(K, f):
    """The CPU rule (direct differences) on the clustered input."""
    U, _ = clustered(K, f)
    return make_agg(N, 'cpu', krum_f=f).pairwise_sqdist(U)


def cpu_scores(D, c):
    """The CPU rule: sort, skip element 0, add 1..c ascending, scale."""
    srt = torch.sort(D, dim=0).values
    out = torch.zeros(D.shape[0], dtype=torch.float64)
    for r in range(1, c + 1):
        out += srt[r]
    return out * (1.0 / c)


def cpu_select(scores, m):
    order = torch.sort(scores, stable=True).indices
    return torch.sort(order[:m]).values


# ---------------------------------------------------------- exact integers
# every sum is an integer <= 9 * n * 4 and so exact in any order: a wrong
# lane map, a dropped tail or a missed chunk changes the value, rounding
# cannot

@pytest.mark.parametrize("K", EXACT_K)
def test_exact_integers(ext, K):
    U = ints(K)
    assert torch.equal(ext.pairwise_sqdist(U.to(DEV)).cpu(), gram_sqdist(U))


@pytest.mark.parametrize("K", [3, 17])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_exact_integers_tiny_n(ext, K, n):
    U = ints(K, n)
    assert torch.equal(ext.pairwise_sqdist(U.to(DEV)).cpu(), gram_sqdist(U))


@pytest.mark.parametrize("K", [17, 10])    # 64-row kernel, 16-row kernel
def test_exact_integers_multi_chunk(ext, K):
    n = 2 ** 20 + 3
    assert ext.pairdist_chunks(K, n) >= 3
    U = ints(K, n)
    assert torch.equal(ext.pairwise_sqdist(U.to(DEV)).cpu(), gram_sqdist(U))


def test_asymmetric_rows_land_in_their_own_cell(ext):
    """Row i is i + 1 in column i alone, so G is diagonal with distinct
    entries and D[i][j] = (i+1)^2 + (j+1)^2: a transposed or permuted
    accumulator write cannot pass."""
    K = 100
    U = torch.zeros(K, N, dtype=torch.float64)
    U[torch.arange(K), torch.arange(K) * 37] = \
        torch.arange(1, K + 1, dtype=torch.float64)
    sq = torch.arange(1, K + 1, dtype=torch.float64) ** 2
    expect = sq.unsqueeze(1) + sq.unsqueeze(0)
    expect.fill_diagonal_(0.0)
    assert torch.equal(ext.pairwise_sqdist(U.to(DEV)).cpu(), expect)


# --------------------------------------------------------------- structure

@pytest.mark.parametrize("K", [1, 2, 17, 65, 338, 512])
def test_structure_on_randn(ext, K):
    U = randn(K).to(DEV)
    D = ext.pairwise_sqdist(U)
    assert D.shape == (K, K) and D.dtype == torch.float64
    assert torch.equal(D, D.T)
    assert (D.diagonal() == 0).all()
    assert (D >= 0).all()
    assert torch.equal(ext.pairwise_sqdist(U), D)


def test_multi_chunk_is_reproducible(ext):
    K, n = 17, 2 ** 20 + 3
    U = randn(K, n).to(DEV)
    D = ext.pairwise_sqdist(U)
    assert torch.equal(D, D.T) and (D.diagonal() == 0).all()
    assert torch.equal(ext.pairwise_sqdist(U), D)


# ---------------------------------------------------------------- accuracy

@pytest.mark.parametrize("K,f", [(4, 1), (10, 2), (17, 3), (65, 10),
                                 (338, 33), (512, 100)])
def test_accuracy_against_direct_differences(ext, K, f):
    """|D_gpu - D_ref| <= 4 n 2^-53 (|u_i|^2 + |u_j|^2): the worst-case
    bound of the three dot products of the Gram form (n 2^-53 |u_i||u_j|
    each, to first order, and 2 |u_i||u_j| <= |u_i|^2 + |u_j|^2) with a
    factor 2 to spare for the reference's own rounding.  Derived, not
    measured."""
    assert K in ACC_K
    U, _ = clustered(K, f)
    D = ext.pairwise_sqdist(U.to(DEV)).cpu()
    ref = direct_sqdist(K, f)
    sq = (U * U).sum(1)
    bound = 4.0 * N * 2.0 ** -53 * (sq.unsqueeze(1) + sq.unsqueeze(0))
    err = (D - ref).abs()
    print(f"K={K}: max err/bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all()


# ------------------------------------------------- scores, selection given D

@pytest.mark.parametrize("kind", ['ints', 'real'])
@pytest.mark.parametrize("K,f", KF)
def test_scores_and_selection_given_D(ext, K, f, kind):
    U = ints(K) if kind == 'ints' else clustered(K, f)[0]
    Ug = U.to(DEV)
    c = K - f - 2
    D = ext.pairwise_sqdist(Ug)
    agg = make_agg(N, DEV, krum_f=f)
    scores = agg.krum_scores(D)
    ref = cpu_scores(D.cpu(), c)
    assert torch.equal(scores.cpu(), ref)
    for m in (1, K - f):
        agg = make_agg(N, DEV, krum_f=f, krum_m=m)
        sel = agg.krum_select(Ug)
        assert sel.dtype == torch.long
        assert torch.equal(sel.cpu(), cpu_select(ref, m))


# ------------------------------------------------- selection, GPU vs direct

@pytest.mark.parametrize("K,f", KF)
def test_selection_end_to_end(K, f):
    U, bad = clustered(K, f)
    m = K - f
    ref_scores = cpu_scores(direct_sqdist(K, f), K - f - 2)
    srt = torch.sort(ref_scores).values
    gap = float((srt[m] - srt[m - 1]) / srt[m - 1])
    print(f"K={K}: relative gap between score m and m+1 = {gap:.1f}")
    assert gap > 1, "ambiguous input: the test's own precondition fails"
    want = cpu_select(ref_scores, m)
    got = make_agg(N, DEV, krum_f=f).krum_select(U.to(DEV)).cpu()
    assert torch.equal(got, want)
    assert not set(got.tolist()) & set(bad.tolist())


# ------------------------------------------------------------ server level

@pytest.mark.parametrize("K,f,theta", [(10, 2, 4), (65, 10, 0)])
def test_server_gpu_matches_cpu(K, f, theta):
    from rlr_amd.flatmodel import FlatParamModel
    U, bad = clustered(K, f)
    ids = list(range(K))
    out, sel = {}, {}
    for dev in ('cpu', DEV):
        gm = FlatParamModel(_P(N), dev)
        before = gm.flat_params.clone()
        agg = make_agg(N, dev, krum_f=f, robustLR_threshold=theta)
        agg.aggregate_updates(gm, U.to(dev), cur_round=1, agent_ids=ids)
        agg.aggregate_buffers(gm, None, ids)
        assert gm.n_buffers == 0 and gm.flat_buffers.numel() == 0
        assert not torch.equal(gm.flat_params, before)
        out[dev] = gm.flat_params.detach().cpu()
        sel[dev] = agg.last_selected.cpu()
    assert torch.equal(sel[DEV], sel['cpu'])
    assert len(sel[DEV]) == K - f
    assert not set(sel[DEV].tolist()) & set(bad.tolist())
    assert torch.allclose(out[DEV], out['cpu'], rtol=1e-6, atol=1e-7), \
        f"max|d|={float((out[DEV] - out['cpu']).abs().max())}"


def test_krum_mean_bitwise_between_backends():
    """0/1 weights through agg_avg are the CPU loop bit for bit."""
    K, f = 10, 2
    U, _ = clustered(K, f)
    cpu = make_agg(N, 'cpu', krum_f=f).agg_krum(U)
    gpu = make_agg(N, DEV, krum_f=f).agg_krum(U.to(DEV))
    assert torch.equal(gpu.cpu(), cpu)


# --------------------------------------------------------- argument checks

def test_argument_checks(ext):
    U = randn(5, 8).to(DEV)
    ext.pairwise_sqdist(U)
    with pytest.raises(RuntimeError):
        ext.pairwise_sqdist(U.float())
    with pytest.raises(RuntimeError):
        ext.pairwise_sqdist(randn(8, 5).to(DEV).T)      # transposed view
    with pytest.raises(RuntimeError):
        ext.pairwise_sqdist(U.cpu())
    with pytest.raises(RuntimeError):
        ext.pairwise_sqdist(U[0])                       # 1-d
    big = ints(ext.pairdist_max_k() + 1, 8)
    with pytest.raises(RuntimeError):
        ext.pairwise_sqdist(big.to(DEV))
    # above the limit the server still answers, through the fallback
    D = make_agg(8, DEV).pairwise_sqdist(big.to(DEV))
    assert torch.equal(D.cpu(), gram_sqdist(big))
    assert torch.equal(D, D.T) and (D.diagonal() == 0).all()


# ------------------------------------------------------------------ driver

def test_krum_aggregation_gpu_end_to_end(monkeypatch):
    import rlr_amd.data.datasets as D
    from rlr_amd.federated import run
    from rlr_amd.options import default_args
    monkeypatch.setitem(D.DEFAULT_SIZES, 'cifar10', (2000, 400))
    h = run(default_args(num_agents=4, rounds=1, snap=1, local_ep=1, bs=128,
                         synthetic=True, no_tb=True, device=DEV,
                         data='cifar10', aggr='krum', krum_f=1))
    assert torch.isfinite(h['final_params']).all()
