"""LDS sorting-network order-statistic kernels (ops/csrc/orderstat.hip):
median at any K, trimmed mean bitwise against the CPU rule, the vote taken
from the resident tile, the fused apply and the server routing.
Every test needs an MI355X: run with `pytest -m gpu`."""

import pytest
import torch

from server_helpers import make_agg, randn

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N = 4099   # prime: never a multiple of the column tile


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


def _randn(K, n=N, seed=0):
    return randn(K, n, seed).to(DEV)


def _ints(K, n=N):
    g = torch.Generator().manual_seed(K)
    return torch.randint(-3, 4, (K, n), generator=g).double().to(DEV)


def cpu_trmean(U, b):
    """The CPU rule: sort, drop b per side, sum ascending, scale."""
    U = U.cpu()
    K = U.shape[0]
    kept = torch.sort(U, dim=0).values[b:K - b]
    out = torch.zeros(U.shape[1], dtype=torch.float64)
    for r in range(K - 2 * b):
        out += kept[r]
    return out * (1.0 / (K - 2 * b))


def gpu_median(ext, U):
    m = (U.shape[0] - 1) // 2
    return ext.agg_orderstat(U, m, m + 1, False, 0.0, 0.0)[0]


# ------------------------------------------------------------------ median

@pytest.mark.parametrize("K", [1, 2, 3, 8, 40, 63, 64, 65, 100, 338, 512])
def test_median_matches_torch(ext, K):
    U = _randn(K)
    assert torch.equal(gpu_median(ext, U), torch.median(U, 0).values)


@pytest.mark.parametrize("K", [7, 65])
@pytest.mark.parametrize("n", [1, 5])
def test_median_tiny_n(ext, K, n):
    U = _randn(K, n)
    assert torch.equal(gpu_median(ext, U), torch.median(U, 0).values)


@pytest.mark.parametrize("K", [8, 65])
def test_ties_and_zeros(ext, K):
    U = _ints(K)
    assert torch.equal(gpu_median(ext, U), torch.median(U, 0).values)
    b = K // 8
    out = ext.agg_orderstat(U, b, K - b, False, 0.0, 0.0)[0]
    assert torch.equal(out.cpu(), cpu_trmean(U, b))


# ------------------------------------------------------------ trimmed mean

@pytest.mark.parametrize("K,b", [(7, 0), (10, 1), (10, 4), (40, 4), (65, 6),
                                 (338, 33), (512, 255)])
def test_trmean_bitwise_vs_cpu_rule(ext, K, b):
    U = _randn(K)
    out = ext.agg_orderstat(U, b, K - b, False, 0.0, 0.0)[0]
    assert torch.equal(out.cpu(), cpu_trmean(U, b))


# -------------------------------------------------------------------- vote

@pytest.mark.parametrize("K,theta", [(7, 4.0), (65, 30.0)])
def test_vote_output_matches_rlr_vote(ext, K, theta):
    U = _ints(K)     # zeros and both signs in a column ...
    U[:, ::7] = U[:, ::7].abs() + 1.0     # ... and some unanimous columns
    agg, lr = ext.agg_orderstat(U, 0, K, True, theta, 0.5)
    ref = ext.rlr_vote(U, theta, 0.5)
    assert torch.equal(lr, ref)
    assert (ref == 0.5).any() and (ref == -0.5).any()
    assert torch.equal(agg.cpu(), cpu_trmean(U, 0))


# ------------------------------------------------------------------- fused

@pytest.mark.parametrize("K", [5, 65])
@pytest.mark.parametrize("rlr", [True, False])
def test_fused_matches_pieces(ext, K, rlr):
    U = _randn(K)
    b = K // 5
    theta = 3.0 if K == 5 else 16.0    # both vote outcomes occur
    g = torch.Generator().manual_seed(K)
    p0 = torch.randn(N, generator=g).to(DEV)
    p, p_fused, p_again = p0.clone(), p0.clone(), p0.clone()
    lr_fused = ext.orderstat_rlr_apply(U, b, K - b, p_fused, rlr, theta, 1.0,
                                       True)
    agg = ext.agg_orderstat(U, b, K - b, False, 0.0, 0.0)[0]
    if rlr:
        lr = ext.rlr_vote(U, theta, 1.0)
        assert (lr == 1.0).any() and (lr == -1.0).any()
        ext.apply_update(p, agg, lr, 1.0)
    else:
        lr = torch.full((N,), 1.0, dtype=torch.float64, device=DEV)
        ext.apply_update(p, agg, torch.empty(0, device=DEV), 1.0)
    assert torch.equal(lr_fused, lr)
    assert torch.allclose(p_fused, p, rtol=1e-6, atol=1e-7), \
        f"max|d|={float((p_fused - p).abs().max())}"
    # want_lr=False returns an empty tensor and applies the same update
    none = ext.orderstat_rlr_apply(U, b, K - b, p_again, rlr, theta, 1.0,
                                   False)
    assert none.numel() == 0
    assert torch.equal(p_again, p_fused)


def test_deterministic(ext):
    U = _randn(100)
    a, la = ext.agg_orderstat(U, 10, 90, True, 20.0, 1.0)
    b, lb = ext.agg_orderstat(U, 10, 90, True, 20.0, 1.0)
    assert torch.equal(a, b) and torch.equal(la, lb)
    p1 = torch.ones(N, device=DEV)
    p2 = torch.ones(N, device=DEV)
    ext.orderstat_rlr_apply(U, 10, 90, p1, True, 20.0, 1.0, False)
    ext.orderstat_rlr_apply(U, 10, 90, p2, True, 20.0, 1.0, False)
    assert torch.equal(p1, p2)


# ------------------------------------------------------------------- limit

def test_argument_checks(ext):
    U = _randn(8, 33)
    for lo, hi in [(-1, 4), (4, 4), (5, 4), (0, 9)]:
        with pytest.raises(RuntimeError):
            ext.agg_orderstat(U, lo, hi, False, 0.0, 0.0)
    with pytest.raises(RuntimeError):
        ext.agg_orderstat(U.float(), 0, 8, False, 0.0, 0.0)
    with pytest.raises(RuntimeError):
        ext.agg_orderstat(U.t(), 0, 8, False, 0.0, 0.0)
    with pytest.raises(RuntimeError):
        ext.agg_orderstat(U.cpu(), 0, 8, False, 0.0, 0.0)
    with pytest.raises(RuntimeError):      # params length != n
        ext.orderstat_rlr_apply(U, 0, 8, torch.zeros(32, device=DEV), False,
                                0.0, 1.0, False)


def test_above_k_limit(ext):
    K = ext.orderstat_max_k() + 1
    assert K > 512
    n = 257
    U = _randn(K, n)
    with pytest.raises(RuntimeError):
        ext.agg_orderstat(U, 0, K, False, 0.0, 0.0)
    with pytest.raises(RuntimeError):
        ext.orderstat_rlr_apply(U, 0, K, torch.zeros(n, device=DEV), False,
                                0.0, 1.0, False)
    agg = make_agg(n, DEV, aggr='trmean', trim_frac=0.1)
    b = int(0.1 * K)
    # the device fallback sums the same sorted values in the same order
    assert torch.equal(agg.agg_trmean(U).cpu(), cpu_trmean(U, b))
    assert torch.equal(agg.agg_comed(U), torch.median(U, 0).values)


# ------------------------------------------------------------ server level

class _P(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.p = torch.nn.Parameter(torch.randn(n, generator=g))


@pytest.mark.parametrize("aggr,K,theta", [('trmean', 10, 4), ('trmean', 65, 0),
                                          ('comed', 65, 0)])
def test_server_gpu_matches_cpu(aggr, K, theta):
    from rlr_amd.flatmodel import FlatParamModel
    U = _randn(K)
    ids = list(range(K))
    out = {}
    for dev in ('cpu', DEV):
        gm = FlatParamModel(_P(N), dev)
        before = gm.flat_params.clone()
        agg = make_agg(N, dev, aggr=aggr, trim_frac=0.2,
                       robustLR_threshold=theta)
        agg.aggregate_updates(gm, U.to(dev), cur_round=1, agent_ids=ids)
        assert not torch.equal(gm.flat_params, before)
        out[dev] = gm.flat_params.detach().cpu()
    assert torch.allclose(out[DEV], out['cpu'], rtol=1e-6, atol=1e-7), \
        f"max|d|={float((out[DEV] - out['cpu']).abs().max())}"


def test_comed_above_64_routes_bitwise():
    U = _randn(65)
    agg = make_agg(N, DEV, aggr='comed')
    assert torch.equal(agg.agg_comed(U), torch.median(U, 0).values)


def test_trmean_aggregation_gpu_end_to_end(monkeypatch):
    import rlr_amd.data.datasets as D
    from rlr_amd.federated import run
    from rlr_amd.options import default_args
    monkeypatch.setitem(D.DEFAULT_SIZES, 'cifar10', (2000, 400))
    h = run(default_args(num_agents=2, rounds=1, snap=1, local_ep=1, bs=128,
                         synthetic=True, no_tb=True, device=DEV,
                         data='cifar10', aggr='trmean'))
    assert torch.isfinite(h['final_params']).all()
