"""FoolsGold on the GPU: the history add (ops/csrc/foolsgold.hip), the
indexed fp64 MFMA Gram kernel (ops/csrc/pairdist.hip), the weights kernels,
and the server path on top of them against the CPU rule.
Every test needs an MI355X: run with `pytest -m gpu`."""

import functools

import pytest
import torch

from foolsgold_helpers import (N, assert_graded_preconditions,
                               assert_sybils_decisive, cpu_gram, graded, ints,
                               make_agg, sybils, weights_from_cosines)
from rlr_amd.aggregation import _row_sum, foolsgold_weights
from server_helpers import P as _P, randn

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PAD = 7                                     # rows of H nobody samples
BIG_N = 2 ** 20 + 3
EXACT_K = [1, 2, 3, 15, 16, 17, 65, 338, 512]
GRADED_K = [10, 17, 65, 338, 512]
KF = [(10, 3), (65, 10), (338, 33)]


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


# ------------------------------------------------------------------ inputs
# CPU tensors, built once and never modified; tests move copies to the GPU

@functools.lru_cache(maxsize=None)
def shuffled(K, A=None):
    """K distinct rows of A = K + PAD, shuffled."""
    A = K + PAD if A is None else A
    g = torch.Generator().manual_seed(13 * K + A)
    return torch.randperm(A, generator=g)[:K].contiguous()


def scattered(rows, idx, A=None):
    """An (A, n) matrix holding rows[k] in row idx[k] and, in the rows nobody
    samples, 5.0: a kernel that reads one of them changes the result."""
    A = rows.shape[0] + PAD if A is None else A
    H = torch.full((A, rows.shape[1]), 5.0, dtype=torch.float64)
    H[idx] = rows
    return H


@functools.lru_cache(maxsize=None)
def cpu_reference(K):
    """(G, alpha at kappa 1, cs) of the CPU rule on graded(K)."""
    G = cpu_gram(graded(K))
    alpha, cs = foolsgold_weights(G, 1.0)
    return G, alpha, cs


# --------------------------------------------------------------- rows_add_

def check_rows_add(ext, K, n):
    A = K + PAD
    idx = shuffled(K)
    H0 = randn(A, n, seed=1)
    U = randn(K, n, seed=2)
    want = H0.clone().index_add_(0, idx, U)
    H = H0.to(DEV)
    assert ext.rows_add_(H, idx, U.to(DEV)) is None
    assert torch.equal(H.cpu(), want)
    rest = torch.ones(A, dtype=torch.bool)
    rest[idx] = False
    assert torch.equal(H.cpu()[rest], H0[rest])
    assert not torch.equal(H.cpu()[idx], H0[idx])


@pytest.mark.parametrize("K", [1, 3, 17, 65, 512])
@pytest.mark.parametrize("n", [1, 5, N])
def test_rows_add(ext, K, n):
    check_rows_add(ext, K, n)


def test_rows_add_many_tiles(ext):
    check_rows_add(ext, 10, BIG_N)


# ---------------------------------------------------------- exact integers
# every sum is an integer <= 9 n and so exact in any order: a wrong lane
# map, a dropped tail, a missed chunk or a wrong row changes the value,
# rounding cannot

def check_gram_exact(ext, K, n):
    rows, idx = ints(K, n), shuffled(K)
    G = ext.gram_rows(scattered(rows, idx).to(DEV), idx)
    assert G.shape == (K, K) and G.dtype == torch.float64
    assert torch.equal(G.cpu(), rows @ rows.T)


@pytest.mark.parametrize("K", EXACT_K)
def test_gram_exact_integers(ext, K):
    check_gram_exact(ext, K, N)


@pytest.mark.parametrize("K", [3, 17])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_gram_exact_integers_tiny_n(ext, K, n):
    check_gram_exact(ext, K, n)


@pytest.mark.parametrize("K", [17, 10])    # 64-row kernel, 16-row kernel
def test_gram_exact_integers_multi_chunk(ext, K):
    assert ext.pairdist_chunks(K, BIG_N) >= 3
    check_gram_exact(ext, K, BIG_N)


def test_gram_rows_land_in_their_own_cell(ext):
    """Sampled row i is i + 1 in column 37 i alone and sits in row
    K - 1 - i of H, so G is diagonal with distinct entries: a transposed or
    permuted accumulator write, or an ignored row map, cannot pass."""
    K = 100
    rows = torch.zeros(K, N, dtype=torch.float64)
    rows[torch.arange(K), torch.arange(K) * 37] = \
        torch.arange(1, K + 1, dtype=torch.float64)
    idx = torch.arange(K - 1, -1, -1)
    H = scattered(rows, idx, A=K)
    assert torch.equal(H, rows.flip(0))
    expect = torch.diag(torch.arange(1, K + 1, dtype=torch.float64) ** 2)
    assert torch.equal(ext.gram_rows(H.to(DEV), idx).cpu(), expect)


# --------------------------------------------------------------- structure

@pytest.mark.parametrize("K", [1, 2, 17, 65, 338, 512])
def test_gram_structure_on_randn(ext, K):
    idx = shuffled(K)
    H = scattered(randn(K), idx).to(DEV)
    G = ext.gram_rows(H, idx)
    assert torch.equal(G, G.T)
    assert (G.diagonal() > 0).all()
    assert torch.equal(ext.gram_rows(H, idx), G)


# ----------------------------------------------------------------- cosines

@pytest.mark.parametrize("K", GRADED_K)
def test_cosines_against_cpu_rule(ext, K):
    """|cs_gpu - cs_cpu| <= (4 n + 8) 2^-53: each backend's G_ij is within
    n u |h_i||h_j| of exact, sqrt(G_ii G_jj) within (n + 2) u relative, the
    quotient adds one rounding (u = 2^-53).  Derived, not measured."""
    _, _, ref = cpu_reference(K)
    assert_graded_preconditions(ref, 1.0)
    idx = shuffled(K)
    G = ext.gram_rows(scattered(graded(K), idx).to(DEV), idx)
    alpha, cs = ext.foolsgold_weights(G, 1.0)
    assert cs.shape == (K, K) and alpha.shape == (K,)
    assert torch.equal(cs, cs.T) and not cs.diagonal().any()
    bound = (4.0 * N + 8.0) * 2.0 ** -53
    err = float((cs.cpu() - ref).abs().max())
    print(f"K={K}: max err/bound = {err / bound:.3e}")
    assert err <= bound


# ------------------------------------------- weights given the same cosines

@pytest.mark.parametrize("kappa", [1.0, 0.5])
@pytest.mark.parametrize("K", GRADED_K)
def test_weights_given_the_kernels_cosines(ext, K, kappa):
    """|alpha_gpu - alpha_ref| <= kappa 2^-52 (8 / (wv (1 - wv)) + 4 |L| + 8)
    with wv, L from the CPU steps 3-7 on the kernel's own cs: at most four
    1-ulp operations from cs to wv and two for the quotient, alpha
    kappa / (wv (1 - wv))-Lipschitz in wv; log within 1 ulp on the host and
    3 ulp (OpenCL full profile, which ocml is built to) on the device.
    Where wv == 0 on the reference alpha is exactly 0."""
    assert kappa >= 0.25
    G = cpu_reference(K)[0].to(DEV)
    alpha, cs = ext.foolsgold_weights(G, kappa)
    cs = cs.cpu()
    assert_graded_preconditions(cs, kappa)
    ref, wv, L = weights_from_cosines(cs, kappa)
    alpha = alpha.cpu()
    dead = wv == 0
    assert (alpha[dead] == 0).all()
    live = ~dead
    bound = kappa * 2.0 ** -52 * (8.0 / (wv[live] * (1.0 - wv[live]))
                                  + 4.0 * L[live].abs() + 8.0)
    err = (alpha[live] - ref[live]).abs()
    print(f"K={K} kappa={kappa}: max err/bound = "
          f"{float((err / bound).max()):.3e}")
    assert (err <= bound).all()
    assert ((alpha >= 0) & (alpha <= 1)).all()


# ---------------------------------------------------- selection, end to end

@pytest.mark.parametrize("K,f", KF)
def test_selection_end_to_end(K, f):
    U, bad = sybils(K, f)
    _, cs = foolsgold_weights(cpu_gram(U), 1.0)
    assert_sybils_decisive(cs, 1.0, bad)
    want = torch.ones(K, dtype=torch.float64)
    want[bad] = 0.0
    ids = shuffled(K).tolist()
    out, alpha = {}, {}
    for dev in ('cpu', DEV):
        agg = make_agg(N, dev, num_agents=K + PAD)
        out[dev] = agg.agg_foolsgold(U.to(dev), ids).cpu()
        alpha[dev] = agg.last_weights.cpu()
    assert torch.equal(alpha['cpu'], want)
    assert torch.equal(alpha[DEV], want)
    assert torch.equal(out['cpu'], _row_sum(U, want) * (1.0 / K))
    assert torch.equal(out[DEV], out['cpu'])


# ------------------------------------------------------------ server level

SERVER_ROUNDS = [(10, 3), (10, 2), (17, 4)]   # sybils(K, f) per round


@pytest.mark.parametrize("theta", [0, 4])
def test_server_gpu_matches_cpu(theta):
    from rlr_amd.flatmodel import FlatParamModel
    A = 40
    out, hist = {}, {}
    for dev in ('cpu', DEV):
        gm = FlatParamModel(_P(N), dev)
        agg = make_agg(N, dev, num_agents=A, robustLR_threshold=theta)
        for rnd, (K, f) in enumerate(SERVER_ROUNDS):
            before = gm.flat_params.clone()
            g = torch.Generator().manual_seed(rnd)
            ids = torch.randperm(A, generator=g)[:K]
            agg.aggregate_updates(gm, sybils(K, f)[0].to(dev), rnd + 1,
                                  agent_ids=ids.tolist())
            assert not torch.equal(gm.flat_params, before)
        out[dev] = gm.flat_params.detach().cpu()
        hist[dev] = agg.foolsgold_history.cpu()
    assert torch.equal(hist[DEV], hist['cpu'])
    assert not hist['cpu'].all(1).all(), "some agent is never sampled"
    assert torch.allclose(out[DEV], out['cpu'], rtol=1e-6, atol=1e-7), \
        f"max|d|={float((out[DEV] - out['cpu']).abs().max())}"


def test_identical_rows_get_zero_on_the_device():
    """Four copies of one row: G is one value, sqrt(g g) = g, cs = 1 off the
    diagonal, wv = 0 = m, alpha is exactly 0 and the parameters keep their
    bits."""
    from rlr_amd.flatmodel import FlatParamModel
    U = randn(1)[0].repeat(4, 1).to(DEV)
    gm = FlatParamModel(_P(N), DEV)
    with torch.no_grad():
        gm.flat_params.copy_(randn(1, seed=5)[0].float())
    before = gm.flat_params.clone()
    agg = make_agg(N, DEV, num_agents=6, robustLR_threshold=2)
    agg.aggregate_updates(gm, U, 1, agent_ids=[5, 0, 3, 2])
    assert torch.equal(agg.last_weights.cpu(), torch.zeros(4).double())
    assert torch.equal(gm.flat_params, before)


def test_server_noise_is_finite_and_deterministic():
    from rlr_amd.flatmodel import FlatParamModel
    K, f = 10, 3
    U = sybils(K, f)[0].to(DEV)
    out = []
    for _ in range(2):
        gm = FlatParamModel(_P(N), DEV)
        agg = make_agg(N, DEV, num_agents=K, noise=0.01, clip=1.0,
                       robustLR_threshold=4)
        agg.aggregate_updates(gm, U, 1, agent_ids=list(range(K)))
        out.append(gm.flat_params.detach().cpu())
    assert torch.isfinite(out[0]).all() and out[0].any()
    assert torch.equal(out[0], out[1])


# --------------------------------------------------------- argument checks

def test_argument_checks(ext):
    H = randn(5, 8).to(DEV)
    idx = torch.tensor([4, 0, 2])
    U = randn(3, 8, seed=1).to(DEV)
    ext.gram_rows(H, idx)
    ext.rows_add_(H.clone(), idx, U)
    bad_H = [H.float(), randn(8, 5).to(DEV).T, H.cpu(), H[0]]
    bad_idx = [torch.tensor([0, 5, 1]), torch.tensor([0, -1, 1]),
               torch.tensor([0, 2, 2]), idx.int(), idx.to(DEV),
               torch.tensor([[4, 0, 2]])]
    for h in bad_H:
        with pytest.raises(RuntimeError):
            ext.gram_rows(h, idx)
        with pytest.raises(RuntimeError):
            ext.rows_add_(h, idx, U)
    for i in bad_idx:
        with pytest.raises(RuntimeError):
            ext.gram_rows(H, i)
        before = H.clone()
        with pytest.raises(RuntimeError):
            ext.rows_add_(H, i, U)
        assert torch.equal(H, before)
    for u in (U.float(), U.cpu(), U[:2], randn(3, 9).to(DEV), U[0]):
        with pytest.raises(RuntimeError):
            ext.rows_add_(H, idx, u)

    G = ext.gram_rows(H, idx)
    ext.foolsgold_weights(G, 1.0)
    for g in (G.float(), G.cpu(), G[0], G[:2]):
        with pytest.raises(RuntimeError):
            ext.foolsgold_weights(g, 1.0)
    with pytest.raises(RuntimeError):
        ext.foolsgold_weights(randn(4, 6).to(DEV)[:, :4], 1.0)   # a view
    with pytest.raises(RuntimeError):
        ext.foolsgold_weights(G, 0.0)

    over = ext.pairdist_max_k() + 1
    assert ext.foolsgold_max_k() == 512
    big = ints(over, 8)
    with pytest.raises(RuntimeError):
        ext.gram_rows(big.to(DEV), torch.arange(over))
    with pytest.raises(RuntimeError):
        ext.foolsgold_weights(torch.eye(over, dtype=torch.float64,
                                        device=DEV), 1.0)


def test_server_answers_above_the_kernel_limit(ext):
    """Through the fallback, and equal to the CPU rule on exact integers."""
    over = ext.pairdist_max_k() + 1
    big = ints(over, 8)
    ids = list(range(over))
    res = {}
    for dev in ('cpu', DEV):
        agg = make_agg(8, dev, num_agents=over)
        agg.foolsgold_accumulate(big.to(dev), ids)
        res[dev] = (agg.foolsgold_history.cpu(),
                    agg.foolsgold_gram(ids).cpu())
    assert torch.equal(res[DEV][0], big)
    assert torch.equal(res[DEV][1], big @ big.T)
    assert torch.equal(res['cpu'][1], big @ big.T)
    a_gpu = make_agg(8, DEV, num_agents=over)
    a_gpu.agg_foolsgold(big.to(DEV), ids)
    a_cpu = make_agg(8, 'cpu', num_agents=over)
    a_cpu.agg_foolsgold(big, ids)
    assert a_gpu.last_weights.is_cuda
    # the same G bit for bit; only the device's log and divide differ
    assert torch.allclose(a_gpu.last_weights.cpu(), a_cpu.last_weights,
                          rtol=0, atol=1e-12)


# ----------------------------------------------------------------- divisor

def test_divisor(ext):
    K = 10
    U = randn(K).to(DEV)
    w = (randn(1, K, seed=4)[0].abs() + 0.1).to(DEV)
    plain = ext.agg_avg(U, w)
    assert torch.equal(ext.agg_avg(U, w, 0.0), plain)
    assert torch.equal(ext.agg_avg(U, w, divisor=0.0), plain)
    got = ext.agg_avg(U, w, divisor=float(K))
    want = plain * (w.sum() / K)
    ulp = 2.0 ** -52 * want.abs()
    assert ((got - want).abs() <= 2 * ulp).all()
    assert not torch.equal(got, plain)

    w01 = torch.ones(K, dtype=torch.float64)
    w01[[1, 4, 5]] = 0.0
    got = ext.agg_avg(U, w01.to(DEV), float(K)).cpu()
    assert torch.equal(got, _row_sum(U.cpu(), w01) * (1.0 / K))

    # the fused entry: default bitwise as before, divisor K as agg_avg's
    def fused(*tail):
        p = torch.zeros(N, device=DEV)
        ext.fused_avg_rlr_apply(U, w, p, False, 0.0, 1.0, 0.0, 0, 0, False,
                                *tail)
        return p
    assert torch.equal(fused(), fused(0.0))
    assert torch.equal(fused(), plain.float())
    assert torch.equal(fused(float(K)),
                       ext.agg_avg(U, w, float(K)).float())
    with pytest.raises(RuntimeError):
        ext.agg_avg(U, w, -1.0)


# ------------------------------------------------------------------ driver

def test_foolsgold_aggregation_gpu_end_to_end(monkeypatch):
    import rlr_amd.data.datasets as D
    from rlr_amd.federated import run
    from rlr_amd.options import default_args
    monkeypatch.setitem(D.DEFAULT_SIZES, 'cifar10', (2000, 400))
    h = run(default_args(num_agents=4, rounds=2, snap=1, local_ep=1, bs=128,
                         synthetic=True, no_tb=True, device=DEV,
                         data='cifar10', aggr='foolsgold', num_corrupt=2,
                         poison_frac=0.5))
    assert torch.isfinite(h['final_params']).all()
