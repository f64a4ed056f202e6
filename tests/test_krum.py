"""Krum / Multi-Krum aggregation (--aggr krum): closed-form cases, validity,
CLI surface, the RLR vote on top, the driver and world-size invariance on
the CPU path, and the kernel's workspace arithmetic (host only)."""

import functools
from time import ctime

import pytest
import torch

from rlr_amd.aggregation import Aggregation
from rlr_amd.options import args_parser, default_args
from rlr_amd.utils.logging import print_exp_details, run_name

import server_helpers
from server_helpers import P as _P, Writer, t64


make_agg = functools.partial(server_helpers.make_agg, n=2, dev='cpu',
                             aggr='krum', table=32)
_run_world = functools.partial(server_helpers.run_world, base_port=29561,
                               aggr='krum', krum_f=1)


# four honest agents near the origin and one far outlier; every distance is
# a small integer:
#         0    1    2    3    4
#   0 [   0,   1,   1,   4, 181]
#   1 [   1,   0,   2,   1, 162]
#   2 [   1,   2,   0,   5, 164]
#   3 [   4,   1,   5,   0, 145]
#   4 [ 181, 162, 164, 145,   0]
U5 = t64([[0, 0], [1, 0], [0, 1], [2, 0], [10, 9]])
D5 = t64([[0, 1, 1, 4, 181],
          [1, 0, 2, 1, 162],
          [1, 2, 0, 5, 164],
          [4, 1, 5, 0, 145],
          [181, 162, 164, 145, 0]])
# f = 1: c = K - f - 2 = 2 nearest neighbours, summed ascending, times 1/2
S5 = t64([(1 + 1) * 0.5, (1 + 1) * 0.5, (1 + 2) * 0.5, (1 + 4) * 0.5,
          (145 + 162) * 0.5])


# ------------------------------------------------------------ closed form

def test_closed_form_distances_and_scores():
    agg = make_agg(krum_f=1)
    D = agg.pairwise_sqdist(U5)
    assert torch.equal(D, D5)
    assert torch.equal(agg.krum_scores(D), S5)


def test_closed_form_classic_krum_m1():
    agg = make_agg(krum_f=1, krum_m=1)
    # agents 0 and 1 tie at score 1.0: the lower position wins
    assert agg.krum_select(U5).tolist() == [0]
    assert torch.equal(agg.agg_krum(U5), U5[0])
    assert agg.last_selected.tolist() == [0]


def test_closed_form_multi_krum_m0():
    agg = make_agg(krum_f=1, krum_m=0)         # m = K - f = 4
    sel = agg.krum_select(U5)
    assert sel.dtype == torch.long and sel.tolist() == [0, 1, 2, 3]
    expect = t64([(0 + 1 + 0 + 2) * 0.25, (0 + 0 + 1 + 0) * 0.25])
    assert torch.equal(agg.agg_krum(U5), expect)


def test_selection_is_returned_in_sampled_order():
    agg = make_agg(krum_f=1, krum_m=3)
    perm = [4, 3, 2, 1, 0]          # the outlier first, best agents last
    # scores by position: [153.5, 2.5, 1.5, 1.0, 1.0] -> keep {3, 4, 2}
    assert agg.krum_select(U5[perm]).tolist() == [2, 3, 4]


def test_tie_break_prefers_lower_position():
    # two far-apart pairs of mutual nearest neighbours; K = 4, f = 1 -> c = 1,
    # score = distance to the nearest neighbour = 1 for every agent
    U = t64([[0, 0], [1, 0], [10, 0], [11, 0]])
    agg = make_agg(krum_f=1, krum_m=1)
    assert torch.equal(agg.krum_scores(agg.pairwise_sqdist(U)),
                       t64([1, 1, 1, 1]))
    assert agg.krum_select(U).tolist() == [0]
    agg = make_agg(krum_f=1, krum_m=2)
    assert agg.krum_select(U).tolist() == [0, 1]
    agg = make_agg(krum_f=1, krum_m=0)
    assert agg.krum_select(U).tolist() == [0, 1, 2]


def test_duplicate_rows_skip_one_zero_only():
    # agents 0 and 1 are identical: each row of D holds two zeros, the sort
    # skips element 0 and the duplicate's zero is scored
    U = t64([[1, 1], [1, 1], [3, 1], [9, 9]])
    agg = make_agg(krum_f=1)
    D = agg.pairwise_sqdist(U)
    assert torch.equal(D, D.T) and D.diagonal().abs().sum() == 0
    assert torch.equal(agg.krum_scores(D), t64([0, 0, 4, 100]))


def test_distance_matrix_structure_on_real_values():
    torch.manual_seed(0)
    U = torch.randn(9, 4099, dtype=torch.float64)
    agg = make_agg()
    D = agg.pairwise_sqdist(U)
    assert torch.equal(D, D.T)
    assert (D.diagonal() == 0).all() and (D >= 0).all()
    assert torch.allclose(D, torch.cdist(U, U) ** 2, rtol=1e-12)


# ---------------------------------------------------------------- validity

@pytest.mark.parametrize("K,f,m,word", [
    (3, 1, 0, 'krum_f'),       # K - f - 2 = 0 neighbours
    (5, 3, 0, 'krum_f'),
    (5, -1, 0, 'krum_f'),      # past the parser on purpose
    (5, 1, 5, 'krum_m'),       # m > K - f
    (5, 1, -1, 'krum_m'),
])
def test_validity_errors(K, f, m, word):
    agg = make_agg()
    agg.args.krum_f, agg.args.krum_m = f, m
    with pytest.raises(ValueError, match=word):
        agg.agg_krum(torch.zeros(K, 2, dtype=torch.float64))


def test_smallest_valid_case():
    agg = make_agg(krum_f=0, krum_m=0)          # K = 3: c = 1, m = 3
    U = t64([[0, 0], [3, 0], [0, 6]])
    assert agg.krum_select(U).tolist() == [0, 1, 2]
    assert torch.equal(agg.agg_krum(U), t64([1, 2]))


@pytest.mark.parametrize("flag", ['--krum_f=-1', '--krum_m=-1'])
def test_negative_flags_rejected_at_parse_time(flag):
    with pytest.raises(SystemExit):
        args_parser(['--aggr', 'krum', flag])


# --------------------------------------------------------------------- CLI

def test_cli_parses_and_names_the_run():
    args = args_parser(['--aggr', 'krum', '--krum_f', '3', '--krum_m', '1',
                        '--server_lr', '0.3', '--device', 'cpu'])
    assert (args.aggr, args.krum_f, args.krum_m) == ('krum', 3, 1)
    assert args.server_lr == 1.0
    assert run_name(args).endswith('-krum_f:3-krum_m:1')
    d = default_args()
    assert (d.krum_f, d.krum_m) == (1, 0)


@pytest.mark.parametrize("aggr", ['avg', 'comed', 'trmean'])
def test_run_name_of_other_rules_unchanged(aggr):
    args = default_args(clip=3.0, noise=0.1, aggr=aggr, num_corrupt=4,
                        robustLR_threshold=8, pattern_type='square',
                        trim_frac=0.2, krum_f=3, krum_m=2)
    before = ctime()
    name = run_name(args)
    after = ctime()

    def expect(t):
        s = (f"time:{t}-clip_val:{args.clip}-noise_std:{args.noise}"
             f"-aggr:{args.aggr}-s_lr:{args.server_lr}"
             f"-num_cor:{args.num_corrupt}"
             f"thrs_robustLR:{args.robustLR_threshold}"
             f"-num_corrupt:{args.num_corrupt}-pttrn:{args.pattern_type}")
        return s + ('-trim:0.2' if aggr == 'trmean' else '')

    assert name in (expect(before), expect(after))
    assert 'krum' not in name


def test_banner_line_only_for_krum(capsys):
    print_exp_details(default_args(aggr='krum', krum_f=3, krum_m=2))
    out = capsys.readouterr().out
    assert 'Krum f / m: 3 / 2' in out
    assert 'Trim' not in out
    krum_lines = out.splitlines()
    for aggr in ('avg', 'comed', 'trmean'):
        print_exp_details(default_args(aggr=aggr, krum_f=3, krum_m=2))
        other = capsys.readouterr().out
        assert 'Krum' not in other and 'krum' not in other
        if aggr == 'avg':
            # the krum banner is the avg banner plus its one line
            expect = [ln.replace('krum', 'avg') for ln in krum_lines
                      if 'Krum f / m' not in ln]
            assert other.splitlines() == expect


# ------------------------------------------------------------ server level

def test_rlr_with_krum_sign_flip():
    """Krum drops the outlier from the mean, yet the vote counts all K:
    a coordinate whose honest majority is too thin moves AGAINST the
    aggregate."""
    from rlr_amd.flatmodel import FlatParamModel
    agg = make_agg(n=2, krum_f=1, krum_m=0, robustLR_threshold=4)
    gm = FlatParamModel(_P(2), 'cpu')
    # K = 5; agent 4 is the outlier.  coord 0: all five positive, |vote| = 5.
    # coord 1: signs + + - - (+ from the outlier): |vote| = 1 < 4 -> flipped.
    U = t64([[1, 1], [1, 2], [1, -1], [1, -4], [100, 100]])
    agg.aggregate_updates(gm, U, cur_round=1, agent_ids=[0, 1, 2, 3, 4])
    assert agg.last_selected.tolist() == [0, 1, 2, 3]
    # mean over the four kept: coord 0 = 1, coord 1 = -0.5; lr = (+1, -1)
    assert gm.flat_params.tolist() == [1.0, 0.5]
    # coord 1 would flip under a vote over the four KEPT agents too
    # (|+1+1-1-1| = 0), so show the all-K property on coord 0: at theta = 5
    # only the excluded outlier's vote carries it over the threshold
    agg = make_agg(n=2, krum_f=1, krum_m=0, robustLR_threshold=5)
    gm = FlatParamModel(_P(2), 'cpu')
    agg.aggregate_updates(gm, U, cur_round=1, agent_ids=[0, 1, 2, 3, 4])
    assert gm.flat_params.tolist() == [1.0, 0.5]


def test_corrupt_selected_is_logged():
    from rlr_amd.flatmodel import FlatParamModel
    args = default_args(no_tb=True, aggr='krum', device='cpu', krum_f=1,
                        num_corrupt=2)
    w = Writer()
    agg = Aggregation({i: 1 for i in range(8)}, 2, None, args, writer=w)
    gm = FlatParamModel(_P(2), 'cpu')
    # sampled order 4, 1, 3, 0, 2 ; the outlier sits at position 0 (id 4)
    agg.aggregate_updates(gm, U5[[4, 1, 3, 0, 2]], cur_round=7,
                          agent_ids=[4, 1, 3, 0, 2])
    assert agg.last_selected.tolist() == [1, 2, 3, 4]
    # kept ids 1, 3, 0, 2: ids 1 and 0 are below num_corrupt = 2
    assert ('Krum/Corrupt_Selected', 2, 7) in w.rows


def test_buffers_average_the_selection_unweighted():
    from rlr_amd.flatmodel import FlatParamModel

    class BN(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(2))
            self.register_buffer('b', torch.zeros(3))

    agg = make_agg(n=2, krum_f=1, krum_m=0)
    gm = FlatParamModel(BN(), 'cpu')
    ids = [0, 1, 2, 3, 4]
    agg.aggregate_updates(gm, U5, cur_round=1, agent_ids=ids)
    deltas = torch.tensor([[4.0, 0, 0], [0, 4, 0], [0, 0, 4], [4, 4, 4],
                           [1e6, 1e6, 1e6]])
    agg.aggregate_buffers(gm, deltas, ids)
    assert gm.flat_buffers.tolist() == [2.0, 2.0, 2.0]


# ------------------------------------------------------------------ driver

def test_driver_runs_krum(tiny_args, tiny_sizes):
    from rlr_amd.federated import build_world, run
    tiny_args.aggr = 'krum'
    tiny_args.num_agents = 4
    tiny_args.krum_f = 1
    tiny_args.device = 'cpu'
    initial = build_world(tiny_args)['global_model'].flat_params.detach() \
        .cpu().clone()
    h = run(tiny_args)
    assert torch.isfinite(h['final_params']).all()
    assert h['final_params'].shape == initial.shape
    assert not torch.equal(h['final_params'], initial)


@pytest.mark.timeout(600)
def test_world_size_invariance_krum():
    p1 = _run_world(1)
    p2 = _run_world(2)
    assert torch.equal(p1, p2), (p1 - p2).abs().max()


# ---------------------------------------------------------- size functions

SWEEP_K = (1, 16, 17, 338, 512)
SWEEP_N = (1, 4099, 2 ** 20 + 3, 11173962, 2 ** 27)


def test_pairdist_workspace_sizes():
    from rlr_amd.ops import ext
    e = ext()
    assert e.pairdist_max_k() == e.orderstat_max_k() == 512
    seen = set()
    for K in SWEEP_K:
        for n in SWEEP_N:
            chunks = e.pairdist_chunks(K, n)
            ws = e.pairdist_ws_doubles(K, n)
            assert chunks >= 1
            seen.add(chunks)
            # stage 1 writes, per chunk, one 64 x 64 slab of partial Gram
            # entries for every pair (ti <= tj) of 64-row tiles of U; up to
            # K = 16 the small kernel writes one 16 x 16 slab per chunk
            tiles = -(-K // 64)
            per_chunk = (16 * 16 if K <= 16
                         else tiles * (tiles + 1) // 2 * 64 * 64)
            assert ws >= chunks * per_chunk, (K, n)
            assert ws * 8 <= 64 * 2 ** 20, (K, n)
            # a chunk holds at least one column
            assert chunks <= n, (K, n)
    assert 1 in seen and max(seen) > 1
    # a single tile pair at this size must split to occupy the chip
    assert e.pairdist_chunks(17, 2 ** 20 + 3) >= 3
    # and the chunking is a function of (K, n) alone
    assert e.pairdist_chunks(17, 2 ** 20 + 3) == \
        e.pairdist_chunks(17, 2 ** 20 + 3)
