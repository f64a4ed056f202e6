"""Coordinate-wise trimmed-mean aggregation (--aggr trmean): closed-form
cases, invariances, CLI surface and the driver, all on the CPU path."""

import functools
from time import ctime

import pytest
import torch

from rlr_amd.options import args_parser, default_args
from rlr_amd.utils.logging import run_name

import server_helpers


make_agg = functools.partial(server_helpers.make_agg, n=3, aggr='trmean',
                             table=32)


# rows are agents, columns coordinates; every column is a permutation of a
# set whose trimmed sums are exact in fp64
U5 = torch.tensor([
    [5.0, -1.0, 0.5],
    [1.0, 100.0, 0.25],
    [3.0, 2.0, -8.0],
    [2.0, 0.0, 0.125],
    [4.0, 1.0, 4.0],
], dtype=torch.float64)


# ------------------------------------------------------------ closed form

def test_closed_form_k5_b1():
    agg = make_agg(trim_frac=0.2)          # b = floor(0.2 * 5) = 1
    out = agg.agg_trmean(U5)
    # sorted columns: [1,2,3,4,5], [-1,0,1,2,100], [-8,.125,.25,.5,4]
    expect = torch.tensor([(2.0 + 3.0 + 4.0) * (1.0 / 3),
                           (0.0 + 1.0 + 2.0) * (1.0 / 3),
                           (0.125 + 0.25 + 0.5) * (1.0 / 3)],
                          dtype=torch.float64)
    assert torch.equal(out, expect)


def test_closed_form_b0_is_sorted_mean():
    agg = make_agg(trim_frac=0.0)
    out = agg.agg_trmean(U5)
    expect = torch.tensor([15.0 * (1.0 / 5), 102.0 * (1.0 / 5),
                           ((((-8.0 + 0.125) + 0.25) + 0.5) + 4.0) * (1.0 / 5)],
                          dtype=torch.float64)
    assert torch.equal(out, expect)


@pytest.mark.parametrize("k", [1, 3, 5, 9])
def test_full_trim_equals_median(k):
    # odd K with b = (K-1)/2 keeps the middle value only
    torch.manual_seed(k)
    U = torch.randn(k, 101, dtype=torch.float64)
    b = (k - 1) // 2
    # (b + 0.25) / K floors to b and stays below 0.5 for every odd K
    agg = make_agg(n=101, trim_frac=(b + 0.25) / k)
    assert agg._trim_count(k) == b
    assert torch.equal(agg.agg_trmean(U), torch.median(U, dim=0).values)


# ------------------------------------------------------------ invariances

def test_permutation_invariance_bitwise():
    torch.manual_seed(1)
    U = torch.randn(11, 257, dtype=torch.float64) * 1e3
    agg = make_agg(n=257, trim_frac=0.2)
    ref = agg.agg_trmean(U)
    g = torch.Generator().manual_seed(7)
    for _ in range(4):
        perm = torch.randperm(11, generator=g)
        assert torch.equal(agg.agg_trmean(U[perm]), ref)


def test_robust_to_two_outliers_where_avg_is_not():
    torch.manual_seed(2)
    U = torch.randn(10, 64, dtype=torch.float64)
    U[3] = 1e6
    U[8] = -1e6
    U[8, :32] = 1e6        # half the coordinates see two outliers on one side
    honest = U[[0, 1, 2, 4, 5, 6, 7, 9]]
    lo, hi = honest.min(dim=0).values, honest.max(dim=0).values
    agg = make_agg(n=64, trim_frac=0.2)
    out = agg.agg_trmean(U)
    assert ((out >= lo) & (out <= hi)).all()
    avg = agg.agg_avg(U, list(range(10)))
    assert not ((avg >= lo) & (avg <= hi)).all()


# -------------------------------------------------------------- validation

@pytest.mark.parametrize("bad", ['0.5', '-0.1'])
def test_trim_frac_out_of_range_rejected_at_parse_time(bad):
    with pytest.raises(SystemExit):
        args_parser(['--aggr', 'trmean', f'--trim_frac={bad}'])


def test_k2_with_trim_049_keeps_both():
    agg = make_agg(n=2, trim_frac=0.49)
    U = torch.tensor([[1.0, -4.0], [3.0, 2.0]], dtype=torch.float64)
    assert agg._trim_count(2) == 0
    assert torch.equal(agg.agg_trmean(U),
                       torch.tensor([2.0, -1.0], dtype=torch.float64))


def test_trim_never_empties_a_column():
    for frac in (0.0, 0.1, 0.25, 1 / 3, 0.49, 0.4999999):
        agg = make_agg(trim_frac=frac)
        for k in range(1, 21):
            assert k - 2 * agg._trim_count(k) >= 1, (frac, k)


def test_trim_count_guard_message():
    agg = make_agg()
    agg.args.trim_frac = 0.5       # past the parser's range check on purpose
    with pytest.raises(ValueError, match='trim_frac'):
        agg.agg_trmean(torch.zeros(4, 3, dtype=torch.float64))


# --------------------------------------------------------------------- CLI

def test_cli_parses_and_names_the_run():
    args = args_parser(['--aggr', 'trmean', '--trim_frac', '0.2',
                        '--server_lr', '0.3', '--device', 'cpu'])
    assert args.aggr == 'trmean' and args.trim_frac == 0.2
    assert args.server_lr == 1.0
    assert '-trim:0.2' in run_name(args)
    assert default_args().trim_frac == 0.1


def test_run_name_of_other_rules_unchanged():
    args = default_args(clip=3.0, noise=0.1, aggr='comed', num_corrupt=4,
                        robustLR_threshold=8, pattern_type='square',
                        trim_frac=0.2)
    before = ctime()
    name = run_name(args)
    after = ctime()

    def expect(t):
        return (f"time:{t}-clip_val:{args.clip}-noise_std:{args.noise}"
                f"-aggr:{args.aggr}-s_lr:{args.server_lr}"
                f"-num_cor:{args.num_corrupt}"
                f"thrs_robustLR:{args.robustLR_threshold}"
                f"-num_corrupt:{args.num_corrupt}-pttrn:{args.pattern_type}")

    assert name in (expect(before), expect(after))
    assert 'trim' not in name


def test_banner_prints_trim_fraction_only_for_trmean(capsys):
    from rlr_amd.utils.logging import print_exp_details
    print_exp_details(default_args(aggr='trmean', trim_frac=0.2))
    assert 'Trim Fraction: 0.2' in capsys.readouterr().out
    print_exp_details(default_args(aggr='avg'))
    assert 'Trim' not in capsys.readouterr().out


# ------------------------------------------------------------ server level

def test_rlr_with_trmean_sign_flip():
    """Coordinates below the vote threshold move AGAINST the aggregate."""
    from rlr_amd.flatmodel import FlatParamModel
    agg = make_agg(n=2, robustLR_threshold=2)   # b = floor(0.1 * 2) = 0

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(2))

    gm = FlatParamModel(M(), 'cpu')
    # both agents agree on coord 0 (+), disagree on coord 1
    U = torch.tensor([[+1.0, +1.0], [+1.0, -2.0]], dtype=torch.float64)
    agg.aggregate_updates(gm, U, cur_round=1, agent_ids=[0, 1])
    # coord0: lr=+1, trmean=+1 -> +1; coord1: trmean=-0.5, lr=-1 -> +0.5
    assert gm.flat_params.tolist() == [1.0, 0.5]


def test_driver_runs_trmean(tiny_args, tiny_sizes):
    from rlr_amd.federated import build_world, run
    tiny_args.aggr = 'trmean'
    tiny_args.device = 'cpu'
    initial = build_world(tiny_args)['global_model'].flat_params.detach() \
        .cpu().clone()
    h = run(tiny_args)
    assert torch.isfinite(h['final_params']).all()
    assert h['final_params'].shape == initial.shape
    assert not torch.equal(h['final_params'], initial)
