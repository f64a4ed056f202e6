"""Fused Weiszfeld kernels (ops/csrc/geomed.hip) and the geometric-median
server path on top of them: exact-integer layout checks, row placement, the
accuracy of one step against the CPU rule, the loop as the composition of its
steps, the rule's properties, both backends end to end, the argument checks
and the driver.
Every test needs an MI355X: run with `pytest -m gpu`."""

import functools

import pytest
import torch

import server_helpers
from server_helpers import P as _P, clustered, randn

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N = 4099   # prime and odd: every second row of U is only 8-byte aligned,
           # and every tile sequence ends in a tail
EXACT_K = [1, 2, 3, 10, 17, 65, 338, 512]
KF = [(4, 1), (10, 2), (65, 10), (338, 33), (512, 100)]
NU = 1e-6
# End to end, GPU against the CPU rule at R = 8 (see test_end_to_end): 100 x
# the largest measured relative difference, rounded up to a power of ten,
# and never looser than 1e-8.  Measured on an MI355X: aggregate 2.5e-16
# (K = 10) and 3.7e-16 (K = 65), weights 2.2e-16 and 5.7e-16; 100 x 5.7e-16
# rounds up to 1e-13.
E2E_BOUND = 1e-13


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


make_agg = functools.partial(server_helpers.make_agg, aggr='geomed')


# ------------------------------------------------------------------ inputs
# CPU tensors, built once and never modified; tests move copies to the GPU

@functools.lru_cache(maxsize=None)
def ints(K, n=N):
    g = torch.Generator().manual_seed(7 * K + n)
    return torch.randint(-3, 4, (K, n), generator=g).double()


def cpu_sqdist(U, a):
    """One step of the CPU rule: s and z sequential in k, d2 in fp64."""
    s = torch.zeros((), dtype=torch.float64)
    z = torch.zeros(U.shape[1], dtype=torch.float64)
    for k in range(U.shape[0]):
        s = s + a[k]
        z += a[k] * U[k]
    z = z * (1.0 / s)
    return ((U - z) ** 2).sum(1)


def zero_one(K, ones):
    """0/1 weights with `ones` ones spread over the rows, the last row
    among them."""
    a = torch.zeros(K, dtype=torch.float64)
    a[torch.linspace(0, K - 1, ones).round().long()] = 1.0
    assert int(a.sum()) == ones
    return a


@functools.lru_cache(maxsize=None)
def cpu_end_to_end(K, f, R=8):
    """(aggregate, normalised weights) of the CPU rule on clustered(K, f)."""
    agg = make_agg(N, 'cpu', geomed_iters=R)
    z = agg.agg_geomed(clustered(K, f)[0])
    return z, agg.last_weights


def rel(x, ref):
    """max |x - ref| / max |ref|."""
    return float((x - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------- exact integers
# U in {-3..3} and a 0/1 vector with 1, 2, 4 or 8 ones: z is a multiple of
# 1/8 and every term a multiple of 1/64, so every sum is exact in any order.
# A wrong lane map, a dropped tail or a missed chunk changes the value,
# rounding cannot.

def check_exact(ext, K, n):
    U = ints(K, n)
    Ug = U.to(DEV)
    for ones in (1, 2, 4, 8):
        if ones > K:
            break
        a = zero_one(K, ones)
        got = ext.geomed_sqdist(Ug, a.to(DEV)).cpu()
        assert torch.equal(got, cpu_sqdist(U, a)), (K, n, ones)


@pytest.mark.parametrize("K", EXACT_K)
def test_exact_integers(ext, K):
    check_exact(ext, K, N)


@pytest.mark.parametrize("K", [3, 17])
@pytest.mark.parametrize("n", [1, 3, 5, 31, 33])
def test_exact_integers_tiny_n(ext, K, n):
    check_exact(ext, K, n)


@pytest.mark.parametrize("K", [10, 17])
def test_exact_integers_multi_chunk(ext, K):
    n = 2 ** 20 + 3
    assert ext.geomed_chunks(K, n) >= 3
    check_exact(ext, K, n)


def test_rows_land_in_their_own_cell(ext):
    """Row i holds i + 1 in column 37 i alone and a is one-hot on row 0, so
    z = U_0 and d2[i] = (i + 1)^2 + 1 (0 for row 0): a permuted partial
    write cannot pass."""
    K = 100
    U = torch.zeros(K, N, dtype=torch.float64)
    U[torch.arange(K), torch.arange(K) * 37] = \
        torch.arange(1, K + 1, dtype=torch.float64)
    a = torch.zeros(K, dtype=torch.float64)
    a[0] = 1.0
    expect = torch.arange(1, K + 1, dtype=torch.float64) ** 2 + 1.0
    expect[0] = 0.0
    assert torch.equal(ext.geomed_sqdist(U.to(DEV), a.to(DEV)).cpu(), expect)


# ------------------------------------------------------- one-step accuracy

@pytest.mark.parametrize("K,f", KF)
def test_one_step_accuracy(ext, K, f):
    """|d2_gpu - d2_cpu| <= 2^-52 (2 (n + 2) d2 + 4 (K + 1) sqrt(d2 S)) per
    k, with S = sum_k ||U_k||^2.  Each side sums n non-negative terms that
    carry at most 3 roundings each (subtract, square, add): relative error
    (n + 2) 2^-53 of d2 per side.  The two z differ by at most
    2 (K + 1) 2^-53 max_k |U_kj| per column (a K-term dot product and the
    scaling on each side); through d/dz (u - z)^2 = 2 (u - z) and
    Cauchy-Schwarz that moves d2 by at most
    2 sqrt(d2) 2 (K + 1) 2^-53 sqrt(sum_j max_k U_kj^2)
    <= 4 (K + 1) 2^-53 sqrt(d2 S).  A factor 2 covers second order.
    Derived, not measured."""
    U, _ = clustered(K, f)
    g = torch.Generator().manual_seed(K)
    a = 1.0 + torch.rand(K, dtype=torch.float64, generator=g)
    got = ext.geomed_sqdist(U.to(DEV), a.to(DEV)).cpu()
    ref = cpu_sqdist(U, a)
    S = (U * U).sum()
    bound = 2.0 ** -52 * (2 * (N + 2) * ref + 4 * (K + 1) * (ref * S).sqrt())
    err = (got - ref).abs()
    print(f"K={K}: max err/bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all()


# --------------------------------------- the loop composes its own steps

@pytest.mark.parametrize("K,f", [(10, 2), (338, 33)])
def test_loop_is_the_composition_of_its_steps(ext, K, f):
    U = clustered(K, f)[0].to(DEV)
    a0, d0 = ext.geomed_weights(U, 0, NU)
    assert torch.equal(a0, torch.ones(K, dtype=torch.float64, device=DEV))
    assert torch.equal(d0, torch.zeros(K, dtype=torch.float64, device=DEV))
    for R in (1, 2, 8):
        a1, _ = ext.geomed_weights(U, R - 1, NU)
        aR, dR = ext.geomed_weights(U, R, NU)
        step = ext.geomed_sqdist(U, a1)
        assert torch.equal(dR, step), R
        assert torch.equal(aR, 1.0 / torch.sqrt(step).clamp(min=NU)), R
        again = ext.geomed_weights(U, R, NU)
        assert torch.equal(again[0], aR) and torch.equal(again[1], dR)
        assert torch.equal(ext.geomed_sqdist(U, a1), step)


def test_nu_caps_the_weight_on_the_gpu(ext):
    # the mean of these rows is row 1 itself: distance 0, weight 1 / nu
    U = torch.tensor([[-1, 0], [0, 0], [1, 0]], dtype=torch.float64)
    a, d2 = ext.geomed_weights(U.to(DEV), 1, 0.25)
    assert a.tolist() == [1.0, 4.0, 1.0] and d2.tolist() == [1.0, 0.0, 1.0]


# -------------------------------------------------------------- properties

@pytest.mark.parametrize("K,f", KF)
def test_corrupted_rows_weigh_less_than_every_honest_row(K, f):
    U, bad = clustered(K, f)
    agg = make_agg(N, DEV)
    agg.agg_geomed(U.to(DEV))
    w = agg.last_weights.cpu()
    good = torch.ones(K, dtype=torch.bool)
    good[bad] = False
    assert abs(float(w.sum()) - 1.0) < 1e-12
    assert float(w[bad].max()) < float(w[good].min())


def test_objective_is_non_increasing():
    U = clustered(10, 2)[0].to(DEV)
    objs = []
    for R in range(0, 9):
        z = make_agg(N, DEV, geomed_iters=R).agg_geomed(U)
        objs.append(float((U - z).norm(dim=1).sum()))
    for R in range(1, 9):
        assert objs[R] <= objs[R - 1] * (1 + 1e-12), (R, objs)
    assert objs[8] < objs[0] * 0.999


# ----------------------------------------------- end to end, both backends

@pytest.mark.parametrize("K,f", [(10, 2), (65, 10)])
def test_end_to_end_against_the_cpu_rule(K, f):
    """agg_geomed on both backends at R = 8: the fp64 aggregate and the
    normalised weights, each as max |gpu - cpu| / max |cpu|, against
    E2E_BOUND."""
    U, _ = clustered(K, f)
    z_ref, w_ref = cpu_end_to_end(K, f)
    agg = make_agg(N, DEV)
    z = agg.agg_geomed(U.to(DEV)).cpu()
    w = agg.last_weights.cpu()
    print(f"K={K}: rel diff aggregate = {rel(z, z_ref):.3e}, "
          f"weights = {rel(w, w_ref):.3e}")
    assert rel(z, z_ref) <= E2E_BOUND
    assert rel(w, w_ref) <= E2E_BOUND


@pytest.mark.parametrize("K,f,theta", [(10, 2, 4), (65, 10, 0)])
def test_server_gpu_matches_cpu(K, f, theta):
    from rlr_amd.flatmodel import FlatParamModel
    U, bad = clustered(K, f)
    ids = list(range(K))
    out, wts = {}, {}
    for dev in ('cpu', DEV):
        gm = FlatParamModel(_P(N), dev)
        before = gm.flat_params.clone()
        agg = make_agg(N, dev, robustLR_threshold=theta)
        agg.aggregate_updates(gm, U.to(dev), cur_round=1, agent_ids=ids)
        agg.aggregate_buffers(gm, None, ids)
        assert gm.n_buffers == 0 and gm.flat_buffers.numel() == 0
        assert not torch.equal(gm.flat_params, before)
        out[dev] = gm.flat_params.detach().cpu()
        wts[dev] = agg.last_weights.cpu()
    print(f"K={K}: rel diff weights = {rel(wts[DEV], wts['cpu']):.3e}")
    assert rel(wts[DEV], wts['cpu']) <= E2E_BOUND
    good = torch.ones(K, dtype=torch.bool)
    good[bad] = False
    assert float(wts[DEV][bad].max()) < float(wts[DEV][good].min())
    assert torch.allclose(out[DEV], out['cpu'], rtol=1e-6, atol=1e-7), \
        f"max|d|={float((out[DEV] - out['cpu']).abs().max())}"


# --------------------------------------------------------- argument checks

def test_argument_checks(ext):
    U = randn(5, 8).to(DEV)
    a = torch.ones(5, dtype=torch.float64, device=DEV)
    ext.geomed_sqdist(U, a)
    ext.geomed_weights(U, 2, NU)
    bad_U = [U.float(),                       # fp32
             randn(8, 5).to(DEV).T,           # transposed view
             U.cpu(),
             U[0]]                            # 1-d
    for X in bad_U:
        with pytest.raises(RuntimeError):
            ext.geomed_sqdist(X, a)
        with pytest.raises(RuntimeError):
            ext.geomed_weights(X, 2, NU)
    with pytest.raises(RuntimeError):
        ext.geomed_sqdist(U, torch.ones(4, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError):
        ext.geomed_sqdist(U, a.float())
    with pytest.raises(RuntimeError):
        ext.geomed_sqdist(U, a.cpu())
    with pytest.raises(RuntimeError):
        ext.geomed_weights(U, -1, NU)
    with pytest.raises(RuntimeError):
        ext.geomed_weights(U, 2, 0.0)
    Kbig = ext.geomed_max_k() + 1
    big = randn(Kbig, 8)
    with pytest.raises(RuntimeError):
        ext.geomed_sqdist(big.to(DEV),
                          torch.ones(Kbig, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError):
        ext.geomed_weights(big.to(DEV), 2, NU)
    # above the limit the server still answers, through the torch loop on
    # the device, and agrees with the CPU rule
    ref = make_agg(8, 'cpu')
    z_ref = ref.agg_geomed(big)
    agg = make_agg(8, DEV)
    z = agg.agg_geomed(big.to(DEV))
    assert z.is_cuda
    print(f"K={Kbig}: rel diff aggregate = {rel(z.cpu(), z_ref):.3e}, "
          f"weights = {rel(agg.last_weights.cpu(), ref.last_weights):.3e}")
    assert rel(z.cpu(), z_ref) <= E2E_BOUND
    assert rel(agg.last_weights.cpu(), ref.last_weights) <= E2E_BOUND


# ------------------------------------------------------------------ driver

def test_geomed_aggregation_gpu_end_to_end(monkeypatch):
    import rlr_amd.data.datasets as D
    from rlr_amd.federated import run
    from rlr_amd.options import default_args
    monkeypatch.setitem(D.DEFAULT_SIZES, 'cifar10', (2000, 400))
    h = run(default_args(num_agents=4, rounds=1, snap=1, local_ep=1, bs=128,
                         synthetic=True, no_tb=True, device=DEV,
                         data='cifar10', aggr='geomed'))
    assert torch.isfinite(h['final_params']).all()
