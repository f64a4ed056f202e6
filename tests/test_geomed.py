"""Geometric-median (RFA) aggregation (--aggr geomed): closed-form cases,
breakdown, the Weiszfeld objective, the weight ordering, CLI surface, the RLR
vote on top, logging, buffers, the driver and world-size invariance on the
CPU path, and the kernel's workspace arithmetic (host only)."""

import functools
import math
from time import ctime

import pytest
import torch

from rlr_amd.aggregation import Aggregation
from rlr_amd.options import args_parser, default_args
from rlr_amd.utils.logging import print_exp_details, run_name

import server_helpers
from server_helpers import N, P as _P, Writer, clustered, t64

NU = 1e-6
KF = [(4, 1), (10, 2), (65, 10), (338, 33), (512, 100)]


make_agg = functools.partial(server_helpers.make_agg, n=2, dev='cpu',
                             aggr='geomed')
_run_world = functools.partial(server_helpers.run_world, base_port=29591,
                               aggr='geomed', geomed_iters=3)


# ------------------------------------------------------------ closed form
# When the median is a data point p, the smoothed iteration settles where the
# capped weight 1/nu of p balances the pull of the others: within
# nu * sum_{k != p} a_k |x_k - p| <= nu * (K - 1) of p.  10 nu covers that.

def test_collinear_points_give_the_middle_point():
    agg = make_agg(geomed_iters=32, geomed_nu=NU)
    U = t64([[0, 0], [1, 0], [10, 0]])
    z = agg.agg_geomed(U)
    assert (z - t64([1, 0])).norm() <= 10 * NU, z
    # the weight sits on the middle point
    assert agg.last_weights.argmax() == 1
    assert abs(float(agg.last_weights.sum()) - 1.0) < 1e-15


def test_four_points_with_a_data_point_median():
    # unit vectors from (1,1) to the others sum to (-0.205, -0.129):
    # norm 0.24 < 1, so (1,1) is the geometric median
    agg = make_agg(geomed_iters=48, geomed_nu=NU)
    U = t64([[0, 0], [4, 0], [0, 3], [1, 1]])
    z = agg.agg_geomed(U)
    assert (z - t64([1, 1])).norm() <= 10 * NU, z


def test_equilateral_triangle_gives_the_centroid():
    agg = make_agg()
    U = t64([[0, 0], [1, 0], [0.5, math.sqrt(3) / 2]])
    z = agg.agg_geomed(U)
    assert torch.allclose(z, U.sum(0) / 3, rtol=0, atol=1e-14)
    assert torch.allclose(agg.last_weights, t64([1, 1, 1]) / 3, rtol=1e-14)


def test_zero_iterations_is_the_unweighted_mean_bitwise():
    U, _ = clustered(10, 2)
    agg = make_agg(n=N, geomed_iters=0)
    out = torch.zeros(N, dtype=torch.float64)
    for k in range(10):
        out += U[k]
    assert torch.equal(agg.agg_geomed(U), out * (1.0 / 10))
    assert torch.equal(agg.geomed_weights(U),
                       torch.ones(10, dtype=torch.float64))
    assert torch.equal(agg.last_weights,
                       torch.full((10,), 0.1, dtype=torch.float64))


def test_weights_are_the_rule_as_written():
    """One and two iterations by hand."""
    U = t64([[0, 0], [4, 0], [0, 3], [1, 1], [7, 7]])
    agg = make_agg(geomed_iters=1)
    z0 = U.sum(0) / 5
    a1 = 1.0 / (U - z0).norm(dim=1)
    assert torch.allclose(agg.geomed_weights(U), a1, rtol=1e-14)
    agg = make_agg(geomed_iters=2)
    z1 = (a1.unsqueeze(1) * U).sum(0) / a1.sum()
    a2 = 1.0 / (U - z1).norm(dim=1)
    assert torch.allclose(agg.geomed_weights(U), a2, rtol=1e-14)
    assert torch.allclose(agg.agg_geomed(U),
                          (a2.unsqueeze(1) * U).sum(0) / a2.sum(), rtol=1e-14)


def test_nu_caps_the_weight_of_a_row_at_the_mean():
    # the mean of these rows is row 1 itself: distance 0, weight 1 / nu
    agg = make_agg(geomed_iters=1, geomed_nu=0.25)
    a = agg.geomed_weights(t64([[-1, 0], [0, 0], [1, 0]]))
    assert a.tolist() == [1.0, 4.0, 1.0]


# --------------------------------------------------------------- breakdown

def test_breakdown_one_outlier_of_five():
    """Started at the mean, which follows the outlier, every iteration cuts
    the outlier's pull about f / (K - f) = 4-fold while z is still far out:
    R = 32 brings 1e6 down to nothing (the default R = 8 would leave
    1e6 * 0.2 / 4^8 ~ 3).  Both medians then lie by the honest square, so
    they are within its diameter of each other."""
    honest = t64([[0, 0], [1, 0], [0, 1], [1, 1]])
    agg = make_agg(geomed_iters=32)
    far = {}
    mean = {}
    for scale in (10.0, 1e6):
        U = torch.cat([honest, t64([[scale, scale]])])
        far[scale] = agg.agg_geomed(U)
        mean[scale] = U.mean(0)
    # the aggregate stays within the honest square's diameter of itself ...
    assert (far[1e6] - far[10.0]).norm() < math.sqrt(2)
    assert 0 <= far[1e6].min() and far[1e6].max() <= 1.5
    # ... while the mean follows the outlier
    assert (mean[1e6] - mean[10.0]).norm() > 1e5


# --------------------------------------------------------------- objective

def objective(U, z):
    return float((U - z).norm(dim=1).sum())


def test_objective_is_non_increasing():
    U, _ = clustered(10, 2)
    prev = None
    for R in range(0, 9):
        agg = make_agg(n=N, geomed_iters=R)
        obj = objective(U, agg.agg_geomed(U))
        if prev is not None:
            assert obj <= prev * (1 + 1e-12), (R, obj, prev)
        prev = obj
    agg = make_agg(n=N, geomed_iters=0)
    assert prev < objective(U, agg.agg_geomed(U)) * 0.999


# ----------------------------------------------------------------- weights

@pytest.mark.parametrize("K,f", KF)
def test_corrupted_rows_weigh_less_than_every_honest_row(K, f):
    U, bad = clustered(K, f)
    agg = make_agg(n=N)
    agg.agg_geomed(U)
    w = agg.last_weights
    good = torch.ones(K, dtype=torch.bool)
    good[bad] = False
    assert abs(float(w.sum()) - 1.0) < 1e-12
    assert float(w[bad].max()) < float(w[good].min())


# ---------------------------------------------------------- flags, naming

@pytest.mark.parametrize("flag", ['--geomed_iters=-1', '--geomed_nu=0',
                                  '--geomed_nu=-1e-6', '--geomed_nu=nan'])
def test_bad_flags_rejected_at_parse_time(flag):
    with pytest.raises(SystemExit):
        args_parser(['--aggr', 'geomed', flag])


def test_cli_parses_and_names_the_run():
    args = args_parser(['--aggr', 'geomed', '--geomed_iters', '3',
                        '--geomed_nu', '0.001', '--server_lr', '0.3',
                        '--device', 'cpu'])
    assert (args.aggr, args.geomed_iters, args.geomed_nu) == \
        ('geomed', 3, 0.001)
    assert args.server_lr == 1.0
    assert run_name(args).endswith('-gm_iters:3-gm_nu:0.001')
    d = default_args()
    assert (d.geomed_iters, d.geomed_nu) == (8, 1e-6)
    assert args_parser(['--aggr', 'geomed', '--geomed_iters', '0',
                        '--device', 'cpu']).geomed_iters == 0


@pytest.mark.parametrize("aggr", ['avg', 'comed', 'sign', 'trmean', 'krum'])
def test_run_name_of_other_rules_unchanged(aggr):
    args = default_args(clip=3.0, noise=0.1, aggr=aggr, num_corrupt=4,
                        robustLR_threshold=8, pattern_type='square',
                        trim_frac=0.2, krum_f=3, krum_m=2, geomed_iters=5,
                        geomed_nu=0.5)
    before = ctime()
    name = run_name(args)
    after = ctime()

    def expect(t):
        s = (f"time:{t}-clip_val:{args.clip}-noise_std:{args.noise}"
             f"-aggr:{args.aggr}-s_lr:{args.server_lr}"
             f"-num_cor:{args.num_corrupt}"
             f"thrs_robustLR:{args.robustLR_threshold}"
             f"-num_corrupt:{args.num_corrupt}-pttrn:{args.pattern_type}")
        return s + {'trmean': '-trim:0.2',
                    'krum': '-krum_f:3-krum_m:2'}.get(aggr, '')

    assert name in (expect(before), expect(after))
    assert 'gm_' not in name


def test_banner_line_only_for_geomed(capsys):
    print_exp_details(default_args(aggr='geomed', geomed_iters=5,
                                   geomed_nu=0.5))
    out = capsys.readouterr().out
    assert '    Geomed iters / nu: 5 / 0.5\n' in out
    assert 'Trim' not in out and 'Krum' not in out
    gm_lines = out.splitlines()
    for aggr in ('avg', 'comed', 'sign', 'trmean', 'krum'):
        print_exp_details(default_args(aggr=aggr, geomed_iters=5,
                                       geomed_nu=0.5))
        other = capsys.readouterr().out
        assert 'Geomed' not in other and 'geomed' not in other
        if aggr == 'avg':
            # the geomed banner is the avg banner plus its one line
            expect = [ln.replace('geomed', 'avg') for ln in gm_lines
                      if 'Geomed iters' not in ln]
            assert other.splitlines() == expect


# ------------------------------------------------------------ server level

# K = 5; agent 4 is the outlier.  coord 0: all five positive, |vote| = 5.
# coord 1: signs + + - - (+ from the outlier): |vote| = 1.
U_VOTE = t64([[1, 1], [1, 2], [1, -1], [1, -4], [100, 100]])


def test_rlr_with_geomed_sign_flip():
    """The vote counts all K and decides the direction; the geometric
    median decides the size: a coordinate whose majority is too thin moves
    AGAINST the aggregate."""
    from rlr_amd.flatmodel import FlatParamModel
    ids = [0, 1, 2, 3, 4]
    ref = make_agg()
    z = ref.agg_geomed(U_VOTE)
    assert z[0] > 0 and z[1] != 0
    for theta, sign in ((0, (1, 1)), (4, (1, -1)), (5, (1, -1))):
        agg = make_agg(robustLR_threshold=theta)
        gm = FlatParamModel(_P(2), 'cpu')
        agg.aggregate_updates(gm, U_VOTE, cur_round=1, agent_ids=ids)
        want = (t64(sign) * z).float()
        assert torch.equal(gm.flat_params.detach(), want), (theta, want)
        assert torch.equal(agg.last_weights, ref.last_weights)
    # the outlier pulls the mean to 20.8 but the median stays by the four
    assert abs(float(z[0]) - 1.0) < 0.5


def test_corrupt_weight_is_logged():
    from rlr_amd.flatmodel import FlatParamModel
    args = default_args(no_tb=True, aggr='geomed', device='cpu',
                        num_corrupt=2)
    w = Writer()
    agg = Aggregation({i: 1 for i in range(8)}, 2, None, args, writer=w)
    gm = FlatParamModel(_P(2), 'cpu')
    order = [4, 1, 3, 0, 2]
    agg.aggregate_updates(gm, U_VOTE[order], cur_round=7, agent_ids=order)
    rows = [r for r in w.rows if r[0] == 'Geomed/Corrupt_Weight']
    assert len(rows) == 1 and rows[0][2] == 7
    # ids 1 and 0 are below num_corrupt = 2: sampled positions 1 and 3
    want = float(agg.last_weights[1] + agg.last_weights[3])
    assert isinstance(rows[0][1], float)
    assert abs(rows[0][1] - want) < 1e-15 and 0.0 < want < 1.0


def test_buffers_are_averaged_with_last_weights():
    from rlr_amd.flatmodel import FlatParamModel

    class BN(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(2))
            self.register_buffer('b', torch.zeros(3))

    agg = make_agg()
    gm = FlatParamModel(BN(), 'cpu')
    ids = [0, 1, 2, 3, 4]
    agg.aggregate_updates(gm, U_VOTE, cur_round=1, agent_ids=ids)
    w = agg.last_weights
    assert w[4] < w[:4].min()
    deltas = torch.tensor([[4.0, 0, 0], [0, 4, 0], [0, 0, 4], [4, 4, 4],
                           [8, 8, 8]])
    agg.aggregate_buffers(gm, deltas, ids)
    want = (deltas.double() * w.unsqueeze(1)).sum(0)
    assert torch.allclose(gm.flat_buffers.double(), want, rtol=1e-6)
    # not the data-size-weighted mean FedAvg would take
    sizes = t64([10, 20, 30, 40, 50])
    fedavg = (deltas.double() * (sizes / sizes.sum()).unsqueeze(1)).sum(0)
    assert not torch.allclose(gm.flat_buffers.double(), fedavg, rtol=1e-3)


# ------------------------------------------------------------------ driver

def test_driver_runs_geomed(tiny_args, tiny_sizes):
    from rlr_amd.federated import build_world, run
    tiny_args.aggr = 'geomed'
    tiny_args.num_agents = 4
    tiny_args.device = 'cpu'
    initial = build_world(tiny_args)['global_model'].flat_params.detach() \
        .cpu().clone()
    h = run(tiny_args)
    assert torch.isfinite(h['final_params']).all()
    assert h['final_params'].shape == initial.shape
    assert not torch.equal(h['final_params'], initial)


@pytest.mark.timeout(900)
def test_world_size_invariance_geomed():
    p1 = _run_world(1)
    p2 = _run_world(2)
    p3 = _run_world(3)
    assert torch.equal(p1, p2), (p1 - p2).abs().max()
    assert torch.equal(p1, p3), (p1 - p3).abs().max()


# ---------------------------------------------------------- size functions

def test_geomed_workspace_sizes():
    from rlr_amd.ops import ext, have_ext
    if not have_ext():
        pytest.skip("the HIP extension is not built")
    e = ext()
    assert e.geomed_max_k() == e.orderstat_max_k() == 512
    cap = 512
    seen = set()
    sweep_n = [1, 2, 31, 32, 33, 255, 256, 257, 4099, 2 ** 16 + 1,
               1199882, 2 ** 20 + 3, 11173962, 2 ** 24]
    for K in range(1, 513):
        for n in sweep_n:
            chunks = e.geomed_chunks(K, n)
            assert 1 <= chunks <= cap, (K, n)
            # stage 1 writes one partial per (chunk, k)
            assert e.geomed_ws_doubles(K, n) >= chunks * K, (K, n)
            # a chunk holds at least one column
            assert chunks <= n, (K, n)
            seen.add(chunks)
    assert 1 in seen and max(seen) == cap
    # the matrix must split to occupy the chip at the workload sizes
    assert e.geomed_chunks(10, 2 ** 20 + 3) >= 3
    assert e.geomed_chunks(17, 2 ** 20 + 3) >= 3
    assert e.geomed_chunks(338, 1199882) >= 128
