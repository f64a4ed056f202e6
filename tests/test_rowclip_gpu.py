"""Row-norm and clip kernels (ops/csrc/rowclip.hip) and server-side clipping
on top of them: exact-integer layout checks, agreement with the CPU rule to
the derived bounds, the clipped set, the in-place scaling bit for bit,
determinism, the workspace, the argument checks, both backends end to end and
the driver under a boosted attack.
Every test needs an MI355X: run with `pytest -m gpu`."""

import functools

import pytest
import torch

import server_helpers
from server_helpers import P as _P

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MC = 'multi-chunk'      # an n the launcher splits into >= 3 chunks
# every K with two n, every n with two K
SHAPES = [(1, 1), (1, 4099), (2, 31), (2, 257), (3, 33), (3, 1),
          (10, 4099), (10, MC), (64, 31), (64, MC), (65, 33), (65, 257),
          (513, 257), (513, 33), (1500, 4099), (1500, 31)]
EPS = 2.0 ** -52
GAP = 1e-6              # no norm this close to tau (relative): see no_straddle


@pytest.fixture(scope='module')
def ext():
    from rlr_amd.ops import ext as _e
    return _e()


make_agg = functools.partial(server_helpers.make_agg, table=2048)


def resolve(ext, K, n):
    """MC -> the smallest 2^m + 3 above the other sizes that the launcher
    splits into at least three chunks for this K: odd, so the last chunk is
    ragged whatever the chunk width."""
    if n != MC:
        return n
    for m in range(13, 24):
        if ext.rownorm_chunks(K, 2 ** m + 3) >= 3:
            return 2 ** m + 3
    raise AssertionError(f"no multi-chunk n below 2^24 for K={K}")


# ------------------------------------------------------------------ inputs
# CPU tensors, built once and never modified; tests move copies to the GPU

@functools.lru_cache(maxsize=None)
def ints(K, n):
    g = torch.Generator().manual_seed(7 * K + n)
    return torch.randint(-8, 9, (K, n), generator=g).double()


@functools.lru_cache(maxsize=None)
def scaled(K, n):
    """Normal rows times 10^e, e spread over [-3, 3] and shuffled."""
    g = torch.Generator().manual_seed(1000 * K + n)
    U = torch.randn(K, n, dtype=torch.float64, generator=g)
    e = torch.linspace(-3, 3, K, dtype=torch.float64)
    e = e[torch.randperm(K, generator=g)]
    return U * (10.0 ** e).unsqueeze(1)


@functools.lru_cache(maxsize=None)
def cpu_norms(K, n):
    U = scaled(K, n)
    return torch.sqrt((U * U).sum(1))


@functools.lru_cache(maxsize=None)
def fixed_bound(K, n):
    """A bound in the widest gap between neighbouring norms around the
    middle, so some rows are clipped and some are not (K = 1: half the
    norm)."""
    srt = torch.sort(cpu_norms(K, n)).values
    if K == 1:
        return float(srt[0]) * 0.5
    lo = max(0, (K - 1) // 2 - 3)
    hi = min(K - 1, lo + 7)
    ratio = srt[lo + 1:hi + 1] / srt[lo:hi]
    i = lo + int(torch.argmax(ratio))
    return float(torch.sqrt(srt[i] * srt[i + 1]))


@functools.lru_cache(maxsize=None)
def cpu_clip(K, n, mode, value):
    """(s, tau, C) of the CPU rule on scaled(K, n)."""
    agg = make_agg(n, 'cpu', server_clip=value, server_clip_mode=mode)
    C = agg.server_clip_updates(scaled(K, n))
    return agg.last_clip_scale, agg.last_clip_bound, C


def no_straddle(K, n, mode, value):
    """A condition on the INPUTS, checked on the CPU reference alone: every
    norm is further than GAP (relative) from tau, so rounding cannot move a
    row across the bound.  The one exception is the median agent at
    multiplier 1.0, whose norm IS tau on each backend: unclipped on both."""
    norm = cpu_norms(K, n)
    tau = float(cpu_clip(K, n, mode, value)[1])
    near = ((norm - tau).abs() <= GAP * tau).nonzero().flatten().tolist()
    if mode == 'median' and value == 1.0:
        assert len(near) == 1 and float(norm[near[0]]) == tau, (K, n, near)
    else:
        assert near == [], (K, n, mode, value, near)


def cases(K, n):
    return [('fixed', fixed_bound(K, n)), ('median', 1.0), ('median', 2.5)]


# ---------------------------------------------------------- exact integers
# Values in [-8, 8]: every square, partial and total is an integer below
# 2^53, exact in any order.  A wrong lane map, a dropped tail or a missed
# chunk changes the value, rounding cannot.

def check_exact(ext, U):
    K, n = U.shape
    sq = (U * U).sum(1)
    assert float(sq.max()) < 2.0 ** 53
    Ug = U.to(DEV)
    part = ext.rownorm_partials(Ug)
    assert part.shape == (ext.rownorm_chunks(K, n), K)
    assert torch.equal(part.sum(0).cpu(), sq), (K, n)
    assert torch.equal(part.cpu(), part.cpu().round())
    # the sums of squares are exact, so the norms differ from sqrt(sq) by
    # the square root's own rounding alone: the device's is within 1 ulp,
    # not always correctly rounded (and sqrt(sq)^2 need not be sq again,
    # so the square of the norm is not what is compared)
    norm = ext.row_norms(Ug).cpu()
    ref = torch.sqrt(sq)
    assert ((norm - ref).abs() <= EPS * ref).all(), (K, n)
    perfect = ref == ref.round()                # a perfect square: exact
    assert torch.equal(norm[perfect], ref[perfect]), (K, n)
    assert torch.equal(Ug.cpu(), U)             # read only


@pytest.mark.parametrize("K,n", SHAPES)
def test_exact_integers(ext, K, n):
    check_exact(ext, ints(K, resolve(ext, K, n)))


@pytest.mark.parametrize("K,n", [(3, 33), (10, 4099), (65, 257), (10, MC)])
def test_exact_integers_shifted_alignment(ext, K, n):
    """Odd n leaves every second row 8-byte aligned only; dropping a column
    and starting one double into the storage shift the base as well."""
    n = resolve(ext, K, n)
    U = ints(K, n)
    check_exact(ext, U[:, 1:].contiguous())
    buf = torch.zeros(K * n + 1, dtype=torch.float64, device=DEV)
    shifted = buf[1:].view(K, n)
    shifted.copy_(U)
    assert shifted.storage_offset() == 1 and shifted.is_contiguous()
    sq = (U * U).sum(1)
    assert torch.equal(ext.rownorm_partials(shifted).sum(0).cpu(), sq)
    s, norm, tau = ext.rowclip_(shifted, 0.5, True)
    assert torch.equal(norm.cpu(), ext.row_norms(U.to(DEV)).cpu())
    assert torch.equal(shifted.cpu(), s.cpu().unsqueeze(1) * U)
    assert float(buf[0]) == 0.0


def test_rows_land_in_their_own_cell(ext):
    """Row i holds i + 1 in column 37 i alone: norm[i] = i + 1 exactly, and a
    permuted partial write cannot pass."""
    K, n = 100, 4099
    U = torch.zeros(K, n, dtype=torch.float64)
    U[torch.arange(K), torch.arange(K) * 37] = \
        torch.arange(1, K + 1, dtype=torch.float64)
    expect = torch.arange(1, K + 1, dtype=torch.float64)
    Ug = U.to(DEV)
    assert torch.equal(ext.row_norms(Ug).cpu(), expect)
    s, norm, tau = ext.rowclip_(Ug, 1.0, True)
    assert float(tau) == 50.0                   # the lower median of 1..100
    assert torch.equal(norm.cpu(), expect)
    # (a tensor over a tensor: a float over a tensor is reciprocal-times)
    fifty = torch.full((K,), 50.0, dtype=torch.float64)
    assert torch.equal(s.cpu(), torch.where(expect > 50.0, fifty / expect,
                                            torch.ones(K, dtype=torch.float64)))


def test_zero_rows_and_a_row_on_the_bound(ext):
    U = torch.tensor([[1, 2, 2, 4], [0, 0, 0, 0], [2, 4, 4, 8]],
                     dtype=torch.float64)
    for median, value in ((False, 5.0), (True, 1.0)):
        Ug = U.to(DEV)
        s, norm, tau = ext.rowclip_(Ug, value, median)
        assert norm.tolist() == [5.0, 0.0, 10.0] and float(tau) == 5.0
        assert s.tolist() == [1.0, 1.0, 0.5]
        assert torch.equal(Ug.cpu(), torch.tensor(
            [[1, 2, 2, 4], [0, 0, 0, 0], [1, 2, 2, 4]], dtype=torch.float64))
    Z = torch.zeros(3, 5, dtype=torch.float64, device=DEV)
    s, norm, tau = ext.rowclip_(Z, 1.0, True)
    assert s.tolist() == [1.0] * 3 and float(tau) == 0.0
    assert not torch.isnan(Z).any()


# ------------------------------------------------ against the CPU rule

@pytest.mark.parametrize("K,n", SHAPES)
def test_agrees_with_the_cpu_rule(ext, K, n):
    """sq is a sum of n non-negative terms, each rounded once, so two
    summation orders differ by at most 2 (n + 1) 2^-53 sq; through the square
    root and its rounding the norms agree to (n + 4) 2^-52 relative, and so
    does s = tau / norm in fixed mode.  In median mode tau carries the same
    error (an order statistic moves by no more than its inputs do), so s
    agrees to 2 (n + 4) 2^-52.  Derived, not measured.  Then: the same rows
    are clipped, the matrix is s * U with the kernel's own s bit for bit,
    unclipped rows keep their bits, and a second call gives the same bits."""
    n = resolve(ext, K, n)
    U = scaled(K, n)
    norm_ref = cpu_norms(K, n)
    tol = (n + 4) * EPS
    for mode, value in cases(K, n):
        no_straddle(K, n, mode, value)
        s_ref, tau_ref, _ = cpu_clip(K, n, mode, value)
        Ug = U.to(DEV)
        s, norm, tau = ext.rowclip_(Ug, value, mode == 'median')
        torch.cuda.synchronize()
        s_c, norm_c, tau_c = s.cpu(), norm.cpu(), float(tau)
        e_norm = float(((norm_c - norm_ref).abs() / norm_ref).max())
        e_tau = abs(tau_c - float(tau_ref)) / float(tau_ref)
        e_s = float(((s_c - s_ref).abs() / s_ref).max())
        print(f"K={K} n={n} {mode} {value:.4g}: norm {e_norm / tol:.3f} "
              f"tau {e_tau / tol:.3f} s {e_s / tol:.3f} of the bound; "
              f"{int((s_c < 1).sum())} of {K} rows clipped")
        assert e_norm <= tol
        assert torch.equal(norm_c, ext.row_norms(U.to(DEV)).cpu())
        if mode == 'fixed':
            assert tau_c == value
            assert e_s <= tol
        else:
            assert e_tau <= tol
            assert e_s <= 2 * tol
        assert torch.equal(s_c < 1.0, s_ref < 1.0)
        assert mode != 'median' or value != 1.0 or \
            int((norm_c == tau_c).sum()) == 1
        # composition, bit for bit, with the kernel's own s
        assert torch.equal(Ug, s.unsqueeze(1) * U.to(DEV))
        keep = s_c == 1.0
        assert torch.equal(Ug.cpu()[keep], U[keep])
        # determinism
        Ug2 = U.to(DEV).clone()
        s2, norm2, tau2 = ext.rowclip_(Ug2, value, mode == 'median')
        assert torch.equal(s2, s) and torch.equal(norm2, norm)
        assert torch.equal(tau2, tau) and torch.equal(Ug2, Ug)


# --------------------------------------------------------------- workspace

@pytest.mark.parametrize("K,n", SHAPES)
def test_workspace_is_large_enough_and_not_overrun(ext, K, n):
    multi = n == MC
    n = resolve(ext, K, n)
    need = ext.rownorm_ws_doubles(K, n)
    chunks = ext.rownorm_chunks(K, n)
    assert need >= chunks * K and 1 <= chunks <= n
    assert chunks >= 3 or not multi
    canary = -12345.0
    U = scaled(K, n)
    ws = torch.full((need + 64,), canary, dtype=torch.float64, device=DEV)
    Ug = U.to(DEV)
    s, norm, tau = ext.rowclip_(Ug, 1.0, True, ws)
    assert torch.equal(ws[need:].cpu(),
                       torch.full((64,), canary, dtype=torch.float64))
    assert not (ws[:chunks * K] == canary).any()
    # the caller's workspace and the binding's own give the same bits
    Ug2 = U.to(DEV)
    s2, norm2, tau2 = ext.rowclip_(Ug2, 1.0, True)
    assert torch.equal(s2, s) and torch.equal(norm2, norm)
    assert torch.equal(ext.row_norms(U.to(DEV), ws), norm)
    assert torch.equal(ws[need:].cpu(),
                       torch.full((64,), canary, dtype=torch.float64))


def test_chunking_occupies_the_chip_at_the_workload_sizes(ext):
    for K, n in [(10, 1199882), (40, 537610), (338, 1199882),
                 (3383, 1199882)]:
        chunks = ext.rownorm_chunks(K, n)
        assert ext.rownorm_ws_doubles(K, n) >= chunks * K
        assert chunks * K >= 1024, (K, n, chunks)
        assert chunks == ext.rownorm_chunks(K, n)


# --------------------------------------------------------- argument checks

def test_argument_checks(ext):
    U = scaled(5, 31).to(DEV)
    ext.row_norms(U.clone())
    ext.rowclip_(U.clone(), 1.0, False)
    bad_U = [U.float(),                         # fp32
             scaled(31, 5).to(DEV).T,           # transposed view
             U.cpu(),
             U[0],                              # 1-d
             U[:0],                             # K = 0
             U[:, :0]]                          # n = 0
    for X in bad_U:
        with pytest.raises(RuntimeError):
            ext.row_norms(X)
        with pytest.raises(RuntimeError):
            ext.rowclip_(X, 1.0, False)
        with pytest.raises(RuntimeError):
            ext.rownorm_partials(X)
    with pytest.raises(RuntimeError):
        ext.rowclip_(U.clone(), -1.0, False)
    with pytest.raises(RuntimeError):
        ext.rowclip_(U.clone(), float('nan'), True)
    need = ext.rownorm_ws_doubles(5, 31)
    for ws in (torch.zeros(need - 1, dtype=torch.float64, device=DEV),
               torch.zeros(need, dtype=torch.float32, device=DEV),
               torch.zeros(need, dtype=torch.float64)):
        with pytest.raises(RuntimeError):
            ext.rowclip_(U.clone(), 1.0, False, ws)
        with pytest.raises(RuntimeError):
            ext.row_norms(U, ws)


# ----------------------------------------------- end to end, both backends

E2E_K, E2E_N = 10, 4099


@functools.lru_cache(maxsize=None)
def attacked():
    """Honest rows base + 0.3 randn; rows 2 and 7 boosted 20 x."""
    g = torch.Generator().manual_seed(77)
    base = torch.randn(E2E_N, dtype=torch.float64, generator=g)
    U = base + 0.3 * torch.randn(E2E_K, E2E_N, dtype=torch.float64,
                                 generator=g)
    U[2] *= -20.0
    U[7] *= 20.0
    return U


def e2e_clip(mode):
    """(mode, value): a fixed bound between two honest norms, or the median
    norm itself; no norm within GAP of the bound except the median agent."""
    U = attacked()
    norm = torch.sqrt((U * U).sum(1))
    srt = torch.sort(norm).values
    value = float(torch.sqrt(srt[3] * srt[4])) if mode == 'fixed' else 1.0
    tau = value if mode == 'fixed' else float(srt[(E2E_K - 1) // 2])
    near = int(((norm - tau).abs() <= GAP * tau).sum())
    assert near == (0 if mode == 'fixed' else 1)
    return value


@pytest.mark.parametrize("mode", ['fixed', 'median'])
@pytest.mark.parametrize("aggr,theta", [('avg', 4), ('trmean', 0),
                                        ('geomed', 4)])
def test_server_gpu_matches_cpu(aggr, theta, mode):
    """aggregate_updates under --server_clip on both backends.  The fp32
    parameters agree to rtol 1e-6, atol 1e-7: the tolerance of
    test_geomed_gpu.py::test_server_gpu_matches_cpu for the same
    comparison."""
    from rlr_amd.flatmodel import FlatParamModel
    U = attacked()
    value = e2e_clip(mode)
    ids = list(range(E2E_K))
    out, st = {}, {}
    for dev in ('cpu', DEV):
        gm = FlatParamModel(_P(E2E_N), dev)
        agg = make_agg(E2E_N, dev, aggr=aggr, robustLR_threshold=theta,
                       server_clip=value, server_clip_mode=mode)
        Ud = U.to(dev).clone()
        agg.aggregate_updates(gm, Ud, cur_round=1, agent_ids=ids)
        out[dev] = gm.flat_params.detach().cpu()
        st[dev] = agg
        assert agg.last_clip_scale.device == Ud.device
        assert agg.last_clip_bound.device == Ud.device
        assert agg.last_norms.device == Ud.device
        # the GPU clips the matrix it was given, the CPU a copy
        assert torch.equal(Ud.cpu(), U) == (dev == 'cpu')
    s_cpu, s_gpu = st['cpu'].last_clip_scale, st[DEV].last_clip_scale.cpu()
    tol = (E2E_N + 4) * EPS * (1 if mode == 'fixed' else 2)
    assert float(((s_gpu - s_cpu).abs() / s_cpu).max()) <= tol
    assert torch.equal(s_gpu < 1, s_cpu < 1)
    assert s_gpu[2] < 0.1 and s_gpu[7] < 0.1 and int((s_gpu < 1).sum()) >= 2
    assert out['cpu'].abs().max() > 0
    assert torch.allclose(out[DEV], out['cpu'], rtol=1e-6, atol=1e-7), \
        f"max|d|={float((out[DEV] - out['cpu']).abs().max())}"


@pytest.mark.parametrize("mode", ['fixed', 'median'])
def test_krum_selects_the_same_agents_under_clipping(mode):
    from rlr_amd.flatmodel import FlatParamModel
    U = attacked()
    value = e2e_clip(mode)
    ids = list(range(E2E_K))
    sel = {}
    for dev in ('cpu', DEV):
        gm = FlatParamModel(_P(E2E_N), dev)
        agg = make_agg(E2E_N, dev, aggr='krum', krum_f=2, krum_m=0,
                       server_clip=value, server_clip_mode=mode)
        agg.aggregate_updates(gm, U.to(dev).clone(), cur_round=1,
                              agent_ids=ids)
        sel[dev] = agg.last_selected.cpu()
    assert torch.equal(sel[DEV], sel['cpu'])
    assert sel[DEV].numel() == E2E_K - 2


def test_buffers_are_scaled_on_the_gpu():
    from rlr_amd.flatmodel import FlatParamModel

    class BN(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(4))
            self.register_buffer('b', torch.zeros(3))

    U = torch.tensor([[1, 2, 2, 4], [0, 0, 0, 0], [2, 4, 4, 8]],
                     dtype=torch.float64)
    deltas = torch.tensor([[4.0, 0, 8], [0, 4, 8], [2, 2, 2]])
    ids = [2, 0, 1]
    got = {}
    for dev in ('cpu', DEV):
        agg = make_agg(4, dev, server_clip=5.0)
        gm = FlatParamModel(BN(), dev)
        agg.aggregate_updates(gm, U.to(dev).clone(), cur_round=1,
                              agent_ids=ids)
        agg.aggregate_buffers(gm, deltas.to(dev), ids)
        got[dev] = gm.flat_buffers.cpu()
    w = torch.tensor([30.0, 10.0, 20.0], dtype=torch.float64) / 60.0
    want = (deltas.double() * torch.tensor([1.0, 1.0, 0.5]).unsqueeze(1)
            * w.unsqueeze(1)).sum(0)
    assert torch.allclose(got[DEV].double(), want, rtol=1e-6)
    assert torch.allclose(got[DEV], got['cpu'], rtol=1e-6)


# ------------------------------------------------------------------ driver

def test_driver_clips_the_boosted_attacker(monkeypatch):
    import rlr_amd.data.datasets as D
    from rlr_amd.aggregation import Aggregation
    from rlr_amd.federated import run
    from rlr_amd.options import default_args
    monkeypatch.setitem(D.DEFAULT_SIZES, 'cifar10', (2000, 400))
    seen = []
    inner = Aggregation.aggregate_updates

    def spy(self, gm, updates, rnd, agent_ids=None):
        inner(self, gm, updates, rnd, agent_ids=agent_ids)
        seen.append((list(agent_ids), self.last_clip_scale.cpu(),
                     self.last_norms.cpu(), float(self.last_clip_bound)))

    monkeypatch.setattr(Aggregation, 'aggregate_updates', spy)
    h = run(default_args(num_agents=4, rounds=2, snap=2, local_ep=1, bs=128,
                         synthetic=True, no_tb=True, device=DEV,
                         data='cifar10', num_corrupt=1, poison_frac=0.5,
                         attack_boost=20.0, server_clip=1.0,
                         server_clip_mode='median'))
    assert torch.isfinite(h['final_params']).all()
    assert len(seen) == 2
    for ids, s, norm, tau in seen:
        p = ids.index(0)                        # the corrupt agent
        assert sorted(ids) == [0, 1, 2, 3]
        assert float(s[p]) < 1.0
        assert float(norm[p]) > tau > 0
        assert float(s.max()) == 1.0            # the median agent at least
