"""Bulyan aggregation (--aggr bulyan) on the CPU path: the window rule on
hand-built columns, stage 2 against a brute-force selection, stage 1
against a plain-Python re-implementation, validity, CLI surface, the server
with the RLR vote and noise on top, buffers, the driver and world-size
invariance."""

import functools

import pytest
import torch

from rlr_amd.aggregation import Aggregation, _row_sum, bulyan_window_mean
from rlr_amd.options import args_parser, default_args
from rlr_amd.utils.logging import print_exp_details, run_name

import server_helpers
from bulyan_helpers import (SHAPES, brute_trim, counts, direct_sqdist,
                            gather_select, graded, ints, python_select)
from server_helpers import P as _P, Writer, randn, t64

make_agg = functools.partial(server_helpers.make_agg, dev='cpu',
                             aggr='bulyan', table=512)
# K = 4 sampled agents in the spawned world: f = 0 is the only valid f
_run_world = functools.partial(server_helpers.run_world, base_port=29621,
                               aggr='bulyan', bulyan_f=0)

N = server_helpers.N


def col(values):
    return t64(values).unsqueeze(1)


# ---------------------------------------------------------- the window rule

def test_window_tie_goes_left():
    c = col([0, 1, 2, 3, 4])                 # m = 2, med = 2
    # beta = 2: dl = dr = 1, the tie takes s[1]; going right would give 2.5
    assert bulyan_window_mean(c, 2).tolist() == [(1 + 2) * 0.5]
    # beta = 3: then dl = 2 > dr = 1
    assert bulyan_window_mean(c, 3).tolist() == [(1 + 2 + 3) * (1.0 / 3)]
    # beta = 4: dl = dr = 2, left again
    assert bulyan_window_mean(c, 4).tolist() == [(0 + 1 + 2 + 3) * 0.25]


def test_window_is_order_free_and_per_column():
    rows = t64([[4, 0], [0, 10], [3, 11], [1, 100], [2, 12]])
    # column 0 is 0..4 shuffled; column 1 sorted is [0, 10, 11, 12, 100]:
    # med = 11, dl = dr = 1 -> 10; then dl = 11 > dr = 1 -> 12
    out = bulyan_window_mean(rows, 3)
    assert out.tolist() == [(1 + 2 + 3) * (1.0 / 3), (10 + 11 + 12) * (1.0 / 3)]


def test_window_runs_into_the_left_edge():
    c = col([-2, -1, 0, 100])                # m = 1, med = -1
    # dl = dr = 1 -> left, l = 0; then dl = +inf -> right
    assert bulyan_window_mean(c, 3).tolist() == [(-2 + -1 + 0) * (1.0 / 3)]
    c = col([1, 5])                          # m = 0: the median IS the edge
    assert bulyan_window_mean(c, 2).tolist() == [(1 + 5) * 0.5]


def test_window_runs_into_the_right_edge():
    c = col([-100, 0, 1, 2])                 # m = 1, med = 0
    # dl = 100 > dr = 1 -> right; dl = 100 > dr = 2 -> right, r = theta - 1
    assert bulyan_window_mean(c, 3).tolist() == [(0 + 1 + 2) * (1.0 / 3)]
    # one more step has only the left side to go to
    assert bulyan_window_mean(c, 4).tolist() == [(-100 + 0 + 1 + 2) * 0.25]
    c = col([-50, -40, -35])                 # m = 1 next to the right edge
    assert bulyan_window_mean(c, 2).tolist() == [(-40 + -35) * 0.5]
    assert bulyan_window_mean(c, 3).tolist() == [(-50 + -40 + -35) * (1.0 / 3)]


def test_window_beta_one_and_beta_theta():
    U = randn(9, 33)
    srt = torch.sort(U, dim=0).values
    assert torch.equal(bulyan_window_mean(U, 1), srt[4] * 1.0)
    assert torch.equal(bulyan_window_mean(U, 9), _row_sum(srt) * (1.0 / 9))
    U = randn(8, 33)                         # even theta: the LOWER median
    assert torch.equal(bulyan_window_mean(U, 1),
                       torch.median(U, dim=0).values)
    with pytest.raises(ValueError):
        bulyan_window_mean(U, 0)
    with pytest.raises(ValueError):
        bulyan_window_mean(U, 9)


@pytest.mark.parametrize("kind", ['ints', 'randn'])
@pytest.mark.parametrize("K,f", SHAPES)
def test_stage2_against_brute_force(K, f, kind):
    theta, beta = counts(K, f)
    rows = (ints(K) if kind == 'ints' else randn(K))[:theta]
    assert torch.equal(bulyan_window_mean(rows, beta), brute_trim(rows, beta))


# ---------------------------------------------------------------- selection

def test_closed_form_smallest_case():
    # K = 3, f = 0: theta = 1, c = 1; D = [[0,1,25],[1,0,16],[25,16,0]],
    # scores [1, 1, 16]: the tie goes to position 0
    U = t64([[0.0], [1.0], [5.0]])
    agg = make_agg(n=1, bulyan_f=0)
    assert agg.bulyan_select(U).tolist() == [0]
    assert torch.equal(agg.agg_bulyan(U), U[0])
    assert agg.last_selected.tolist() == [0]


@pytest.mark.parametrize("K,f", [(3, 0), (7, 1), (10, 1), (21, 1), (40, 4)])
@pytest.mark.parametrize("kind", ['ints', 'randn'])
def test_selection_against_plain_python(K, f, kind):
    U = ints(K) if kind == 'ints' else randn(K)
    agg = make_agg(n=N, bulyan_f=f)
    D = agg.pairwise_sqdist(U)
    assert torch.equal(D, direct_sqdist(U))
    sel = agg.bulyan_picks(D)
    assert sel.dtype == torch.long
    assert sel.tolist() == python_select(D, f)
    assert sel.tolist() == gather_select(D, f)[0]
    assert torch.equal(agg.bulyan_select(U), sel)


@pytest.mark.parametrize("K,f", [(67, 16), (338, 33), (512, 127)])
def test_selection_against_gathered_distances(K, f):
    D = direct_sqdist(ints(K))
    agg = make_agg(n=N, bulyan_f=f)
    assert agg.bulyan_picks(D).tolist() == gather_select(D, f)[0]


@pytest.mark.parametrize("K,f", [s for s in SHAPES if s[1] > 0])
def test_graded_excludes_every_attacker(K, f):
    U, bad = graded(K, f)
    agg = make_agg(n=N, bulyan_f=f)
    sel = agg.bulyan_select(U)
    theta, _ = counts(K, f)
    assert sel.numel() == theta and sel.unique().numel() == theta
    assert torch.equal(sel, torch.sort(sel).values)
    assert not set(sel.tolist()) & set(bad.tolist())


@pytest.mark.parametrize("K", [7, 10])
def test_f0_averages_all_selected(K):
    U = randn(K)
    agg = make_agg(n=N, bulyan_f=0)
    out = agg.agg_bulyan(U)
    sel = agg.last_selected
    theta = K - 2
    assert sel.numel() == theta
    srt = torch.sort(U[sel], dim=0).values
    assert torch.equal(out, _row_sum(srt) * (1.0 / theta))
    if K == 10:     # theta = 8: the multiply by 1/8 IS the division by 8
        assert torch.equal(out, _row_sum(srt) / theta)


@pytest.mark.parametrize("K,f", [(10, 1), (21, 1), (40, 4)])
def test_row_permutation_invariance(K, f):
    U = randn(K)
    g = torch.Generator().manual_seed(K)
    p = torch.randperm(K, generator=g)
    a, b = make_agg(n=N, bulyan_f=f), make_agg(n=N, bulyan_f=f)
    out = a.agg_bulyan(U)
    assert torch.equal(b.agg_bulyan(U[p]), out)
    # the same agents, named by their new positions
    assert sorted(p[b.last_selected].tolist()) == a.last_selected.tolist()


# ----------------------------------------------------------------- validity

@pytest.mark.parametrize("K,f", [(2, 0), (6, 1), (10, 2), (5, -1)])
def test_validity_errors(K, f):
    agg = make_agg(n=2)
    agg.args.bulyan_f = f                    # past the parser on purpose
    U = torch.zeros(K, 2, dtype=torch.float64)
    for call in (agg.agg_bulyan, agg.bulyan_select):
        with pytest.raises(ValueError, match='bulyan_f') as e:
            call(U)
        assert f'K={K}' in str(e.value) and f'bulyan_f={f}' in str(e.value)
        assert f'4 f + 3 = {4 * f + 3}' in str(e.value)
    from rlr_amd.flatmodel import FlatParamModel
    with pytest.raises(ValueError, match='bulyan_f'):
        agg.aggregate_updates(FlatParamModel(_P(2), 'cpu'), U, cur_round=1,
                              agent_ids=list(range(K)))


def test_smallest_valid_K_per_f():
    for f in (0, 1, 2):
        K = 4 * f + 3
        agg = make_agg(n=33, bulyan_f=f)
        out = agg.agg_bulyan(randn(K, 33))
        assert agg.last_selected.numel() == 2 * f + 1
        assert torch.isfinite(out).all()


def test_negative_flag_rejected_at_parse_time():
    with pytest.raises(SystemExit):
        args_parser(['--aggr', 'bulyan', '--bulyan_f=-1'])
    with pytest.raises(ValueError, match='bulyan_f'):
        default_args(bulyan_f=-1)


# ---------------------------------------------------------------------- CLI

def test_cli_parses_and_names_the_run(capsys):
    args = args_parser(['--aggr', 'bulyan', '--bulyan_f', '3',
                        '--server_lr', '0.3', '--device', 'cpu'])
    assert (args.aggr, args.bulyan_f) == ('bulyan', 3)
    assert args.server_lr == 1.0
    assert run_name(args).endswith('-bulyan_f:3')
    assert default_args().bulyan_f == 1
    assert args_parser(['--bulyan_f', '0', '--device', 'cpu']).bulyan_f == 0
    print_exp_details(args)
    assert 'Bulyan f: 3' in capsys.readouterr().out
    for aggr in ('avg', 'krum', 'trmean'):
        other = default_args(aggr=aggr, bulyan_f=3)
        assert 'bulyan' not in run_name(other)
        print_exp_details(other)
        assert 'ulyan' not in capsys.readouterr().out


# ------------------------------------------------------------- server level

# six honest agents around (1, 1) and one far outlier; K = 7, f = 1:
# theta = 3, beta = 1
U7 = t64([[1, 1], [1, 2], [2, 1], [1, -1], [0.5, 1], [1, 0], [100, 100]])


def _server_round(U, **over):
    from rlr_amd.flatmodel import FlatParamModel
    n = U.shape[1]
    agg = make_agg(n=n, **over)
    gm = FlatParamModel(_P(n), 'cpu')
    agg.aggregate_updates(gm, U, cur_round=3,
                          agent_ids=list(range(U.shape[0])))
    return agg, gm.flat_params.detach().clone()


def test_server_without_rlr():
    agg, p = _server_round(U7, bulyan_f=1)
    D = direct_sqdist(U7)
    assert agg.last_selected.tolist() == python_select(D, 1)
    assert 6 not in agg.last_selected.tolist()
    expect = brute_trim(U7[agg.last_selected], 1)
    assert torch.equal(p, expect.float())
    U = randn(21)
    agg, p = _server_round(U, bulyan_f=2)
    expect = brute_trim(U[agg.last_selected], 21 - 4 * 2 - 2)
    assert torch.equal(p, expect.float())
    assert torch.equal(make_agg(n=N, bulyan_f=2).agg_bulyan(U), expect)


def test_rlr_votes_over_all_sampled_agents():
    """Bulyan decides what is averaged, the vote over all K the direction:
    coordinate 0 has all seven signs positive, coordinate 1 has
    + + + - + 0 + = 4."""
    agg, plain = _server_round(U7, bulyan_f=1)
    for theta, lr in ((4, [1.0, 1.0]), (5, [1.0, -1.0]), (7, [1.0, -1.0])):
        _, p = _server_round(U7, bulyan_f=1, robustLR_threshold=theta)
        assert torch.equal(p, plain * torch.tensor(lr))
    # the three selected agents alone could never reach a vote of 4
    assert agg.last_selected.numel() == 3


def test_server_with_noise_takes_the_composed_path():
    U = randn(10)
    quiet, p0 = _server_round(U, bulyan_f=1, robustLR_threshold=4)
    agg, p = _server_round(U, bulyan_f=1, robustLR_threshold=4, noise=0.5,
                           clip=2.0)
    assert torch.equal(agg.last_selected, quiet.last_selected)
    lr = agg.compute_robustLR(U)
    noisy = agg.agg_bulyan(U) + agg._noise(3, 'cpu', torch.float64)
    assert torch.equal(p, (lr * noisy).float())
    assert not torch.equal(p, p0)
    _, again = _server_round(U, bulyan_f=1, robustLR_threshold=4, noise=0.5,
                             clip=2.0)
    assert torch.equal(again, p)


def test_server_clip_runs_in_front():
    U = randn(10)
    agg, p = _server_round(U, bulyan_f=1, server_clip=30.0)
    C = agg.last_clip_scale.unsqueeze(1) * U
    assert (agg.last_clip_scale < 1).any()
    ref = make_agg(n=N, bulyan_f=1)
    assert torch.equal(p, ref.agg_bulyan(C).float())
    assert torch.equal(agg.last_selected, ref.last_selected)


def test_last_selected_and_corrupt_selected_scalar():
    from rlr_amd.flatmodel import FlatParamModel
    args = default_args(no_tb=True, aggr='bulyan', device='cpu', bulyan_f=1,
                        num_corrupt=2)
    w = Writer()
    agg = Aggregation({i: 1 for i in range(8)}, 2, None, args, writer=w)
    gm = FlatParamModel(_P(2), 'cpu')
    order = [6, 1, 3, 0, 2, 5, 4]        # the outlier (id 6) at position 0
    agg.aggregate_updates(gm, U7[order], cur_round=7, agent_ids=order)
    sel = agg.last_selected.tolist()
    assert sel == python_select(direct_sqdist(U7[order]), 1)
    assert sel == sorted(sel) and len(sel) == 3 and 0 not in sel
    n_bad = sum(1 for p in sel if order[p] < 2)
    assert ('Bulyan/Corrupt_Selected', n_bad, 7) in w.rows
    assert not any(name.startswith('Krum') for name, _, _ in w.rows)


def test_buffers_average_the_selection_unweighted():
    from rlr_amd.flatmodel import FlatParamModel

    class BN(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(2))
            self.register_buffer('b', torch.zeros(3))

    agg = make_agg(n=2, bulyan_f=1)
    gm = FlatParamModel(BN(), 'cpu')
    ids = list(range(7))
    agg.aggregate_updates(gm, U7, cur_round=1, agent_ids=ids)
    sel = agg.last_selected.tolist()
    assert len(sel) == 3
    deltas = torch.full((7, 3), 1e6)
    for i, p in enumerate(sel):
        deltas[p] = 0.0
        deltas[p, i] = 6.0
    agg.aggregate_buffers(gm, deltas, ids)
    assert gm.flat_buffers.tolist() == [2.0, 2.0, 2.0]


# ------------------------------------------------------------------- driver

def test_driver_runs_bulyan(tiny_args, tiny_sizes):
    from rlr_amd.federated import build_world, run
    tiny_args.aggr = 'bulyan'
    tiny_args.num_agents = 7
    tiny_args.bulyan_f = 1
    tiny_args.device = 'cpu'
    initial = build_world(tiny_args)['global_model'].flat_params.detach() \
        .cpu().clone()
    h = run(tiny_args)
    assert torch.isfinite(h['final_params']).all()
    assert h['final_params'].shape == initial.shape
    assert not torch.equal(h['final_params'], initial)


@pytest.mark.timeout(600)
def test_world_size_invariance_bulyan():
    p1 = _run_world(1)
    p2 = _run_world(2)
    assert torch.equal(p1, p2), (p1 - p2).abs().max()
