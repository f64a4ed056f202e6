"""FoolsGold on the CPU: the vectorised rule against brute-force loops,
hand-worked cases, the history across rounds, order invariance, the server
round, the argument checks, the checkpoint and the world size."""

import math
import os

import pytest
import torch

import server_helpers
from foolsgold_helpers import (N, assert_sybils_decisive, cpu_gram, make_agg,
                               steps_3_to_6, sybils)
from rlr_amd.aggregation import _row_sum, foolsgold_weights
from rlr_amd.flatmodel import FlatParamModel
from server_helpers import P, Writer, randn, t64


# ------------------------------------------------------------- brute force

def brute_force(cs, kappa):
    """Steps 3-5 in plain Python loops over lists of floats, from the cosine
    matrix of step 2; steps 6-7 in torch, so that log is the same
    routine."""
    K = cs.shape[0]
    cs = cs.tolist()
    v = [max(cs[i]) for i in range(K)]
    pard = [row[:] for row in cs]
    for i in range(K):
        for j in range(K):
            if i != j and v[i] < v[j]:
                pard[i][j] = (cs[i][j] * v[i]) / v[j]
    wv = t64([min(max(1.0 - max(pard[i]), 0.0), 1.0) for i in range(K)])
    m = wv.max()
    if m > 0:
        wv = wv / m
    wv[wv == 1.0] = 0.99
    return (kappa * (torch.log(wv / (1.0 - wv)) + 0.5)).clamp(0.0, 1.0)


@pytest.mark.parametrize("K", [1, 2, 3, 10, 65])
@pytest.mark.parametrize("kappa", [1.0, 0.5])
def test_rule_equals_brute_force(K, kappa):
    g = torch.Generator().manual_seed(11 * K)
    B = torch.randn(K, 7, dtype=torch.float64, generator=g)
    B[:, 0] += 2.0                      # a shared direction: cosines > 0
    G = cpu_gram(B)
    assert torch.equal(G, G.T)
    alpha, cs = foolsgold_weights(G, kappa)
    assert torch.equal(cs, cs.T) and not cs.diagonal().any()
    assert torch.equal(alpha, brute_force(cs, kappa))
    if K >= 10:
        assert ((alpha > 0) & (alpha < 1)).any()


# -------------------------------------------------------------- hand-worked

def test_pardoning_lowers_the_low_v_row():
    """h0 = (4, 0, 0), h1 = h2 = (4, 3, 0), h3 = (0, 0, 1).
    cs01 = cs02 = 16 / sqrt(16 * 25) = 0.8, cs12 = 25 / sqrt(25 * 25) = 1,
    row 3 is orthogonal to all: v = (0.8, 1, 1, 0).
    Pardoning: v0 < v1 = v2, so cs0j <- (0.8 * 0.8) / 1 = 0.64 for j = 1, 2;
    rows 1 and 2 keep their 1 against each other (v1 = v2) and their 0.8
    against agent 0 (v1 > v0).
    wv = (1 - 0.64, 0, 0, 1), not (1 - 0.8, 0, 0, 1); m = 1; wv3 -> 0.99.
    alpha0 = ln(0.36 / 0.64) + 0.5 = -0.075 -> 0; alpha3 -> 1."""
    H = t64([[4, 0, 0], [4, 3, 0], [4, 3, 0], [0, 0, 1]])
    alpha, cs = foolsgold_weights(cpu_gram(H), 1.0)
    assert torch.equal(cs, t64([[0, 0.8, 0.8, 0], [0.8, 0, 1, 0],
                                [0.8, 1, 0, 0], [0, 0, 0, 0]]))
    wv, m, _ = steps_3_to_6(cs)
    assert wv.tolist() == [1.0 - (0.8 * 0.8) / 1.0, 0.0, 0.0, 0.99]
    assert float(m) == 1.0
    assert torch.equal(alpha, t64([0, 0, 0, 1]))


def test_pardoning_changes_alpha():
    """h0 = (1, 0, 0), h1 = (3, 4, 0), h2 = (3, 4, 1), h3 = (0, 0, 1).
    cs01 = 3 / sqrt(1 * 25) = 0.6, cs02 = 3 / sqrt(26) = 0.58835,
    cs12 = 25 / sqrt(25 * 26) = 0.98058, cs23 = 1 / sqrt(26) = 0.19612,
    cs03 = cs13 = 0.  v = (0.6, 0.98058, 0.98058, 0.19612).
    Row 0 is pardoned against 1 and 2: 0.6 * 0.6 / 0.98058 = 0.36713 and
    0.58835 * 0.6 / 0.98058 = 0.36, so wv0 = 0.63287 (0.4 without).
    Row 3: 0.19612 * 0.19612 / 0.98058 = 0.03922, wv3 = 0.96078 = m.
    Rows 1, 2: wv = 1 - 0.98058 = 0.01942.
    wv / m = (0.65871, 0.02021, 0.02021, 1 -> 0.99).
    alpha0 = ln(0.65871 / 0.34129) + 0.5 = 1.158 -> 1; without the
    pardoning wv0 / m = 0.41633 and alpha0 = ln(0.41633 / 0.58367) + 0.5 =
    0.162.  alpha1 = alpha2 = ln(0.02021 / 0.97979) + 0.5 < 0 -> 0."""
    H = t64([[1, 0, 0], [3, 4, 0], [3, 4, 1], [0, 0, 1]])
    alpha, cs = foolsgold_weights(cpu_gram(H), 1.0)
    assert float(cs[0, 1]) == 0.6 and float(cs[0, 3]) == 0.0
    assert cs[0, 2].item() == pytest.approx(3 / math.sqrt(26), abs=1e-15)
    wv, m, scaled = steps_3_to_6(cs)
    assert scaled.tolist() == pytest.approx([0.65871, 0.02021, 0.02021, 1.0],
                                            abs=1e-5)
    assert float(m) == pytest.approx(0.96078, abs=1e-5)
    assert torch.equal(alpha, t64([1, 0, 0, 1]))
    unpardoned = (1.0 - 0.6) / float(m)
    assert 0 < math.log(unpardoned / (1 - unpardoned)) + 0.5 < 1


def test_zero_diagonal_takes_part():
    """h0 = (1, 0), h1 = (-1, 0), h2 = (0, -1): every cosine is <= 0, so
    v = 0 from the diagonal (not -1 or 0 off it), nothing is pardoned,
    wv = 1 -> 0.99 everywhere and alpha = 1."""
    H = t64([[1, 0], [-1, 0], [0, -1]])
    alpha, cs = foolsgold_weights(cpu_gram(H), 1.0)
    assert torch.equal(cs, t64([[0, -1, 0], [-1, 0, 0], [0, 0, 0]]))
    assert torch.equal(alpha, t64([1, 1, 1]))


def test_zero_history_row():
    """A zero row has den = 0 against everybody: cs = 0, not NaN, and its
    alpha is 1; the two identical rows beside it get 0."""
    H = t64([[0, 0], [1, 2], [1, 2]])
    alpha, cs = foolsgold_weights(cpu_gram(H), 1.0)
    assert torch.equal(cs, t64([[0, 0, 0], [0, 0, 1], [0, 1, 0]]))
    assert torch.equal(alpha, t64([1, 0, 0]))


def test_single_agent():
    alpha, cs = foolsgold_weights(t64([[5.0]]), 1.0)
    assert torch.equal(cs, t64([[0]]))
    # wv = 1 -> 0.99; ln(99) + 0.5 > 1
    assert torch.equal(alpha, t64([1]))


@pytest.mark.parametrize("rlr", [0, 2])
def test_all_sybils_move_nothing(rlr):
    """Four identical rows: cs = 1 exactly off the diagonal (sqrt(g g) = g
    on IEEE arithmetic), wv = 0, m = 0, alpha = 0 and the parameters keep
    their bits."""
    row = randn(1)[0]
    U = row.repeat(4, 1)
    agg = make_agg(N, 'cpu', num_agents=4, robustLR_threshold=rlr)
    gm = FlatParamModel(P(N), 'cpu')
    with torch.no_grad():
        gm.flat_params.copy_(randn(1, seed=5)[0].float())
    before = gm.flat_params.clone()
    agg.aggregate_updates(gm, U, 1, agent_ids=[0, 1, 2, 3])
    _, cs = foolsgold_weights(agg.foolsgold_gram([0, 1, 2, 3]), 1.0)
    assert torch.equal(cs, torch.ones(4, 4).double() - torch.eye(4).double())
    assert torch.equal(agg.last_weights, torch.zeros(4).double())
    assert torch.equal(gm.flat_params, before)


# ------------------------------------------------------------------ history

ROUNDS = [[0, 3, 5], [5, 1, 0, 4], [3, 6]]      # of A = 7; agent 2 never


def _round_updates(r, K):
    return randn(K, seed=100 + r)


@pytest.mark.parametrize("clip", [0.0, 30.0])
def test_history_is_the_hand_sum(clip):
    A = 7
    agg = make_agg(N, 'cpu', num_agents=A, server_clip=clip)
    gm = FlatParamModel(P(N), 'cpu')
    assert agg.foolsgold_history is None and agg.state_dict() == {}
    want = torch.zeros(A, N, dtype=torch.float64)
    clipper = make_agg(N, 'cpu', num_agents=A, server_clip=clip)
    clipped = 0
    for r, ids in enumerate(ROUNDS):
        U = _round_updates(r, len(ids))
        agg.aggregate_updates(gm, U, r + 1, agent_ids=ids)
        C = clipper.server_clip_updates(U) if clip > 0 else U
        clipped += int((C != U).any(1).sum())
        for k, i in enumerate(ids):
            want[i] += C[k]
    assert (clipped > 0) == (clip > 0), "the bound's own precondition"
    H = agg.foolsgold_history
    assert H.dtype == torch.float64 and H.shape == (A, N)
    assert torch.equal(H, want)
    assert not H[2].any()
    assert agg.state_dict()['foolsgold_history'] is H


def test_order_invariance():
    U, _ = sybils(10, 3)
    ids = [7, 2, 9, 0, 4, 1, 8, 3, 6, 5]
    perm = torch.tensor([3, 0, 9, 5, 1, 8, 2, 7, 4, 6])
    a = make_agg(N, 'cpu', num_agents=10)
    b = make_agg(N, 'cpu', num_agents=10)
    g = randn(10, seed=9) + 2.0         # in-between alphas too
    for rnd, M in enumerate((g, U)):
        a.agg_foolsgold(M, ids)
        b.agg_foolsgold(M[perm], [ids[p] for p in perm.tolist()])
    assert torch.equal(a.foolsgold_history, b.foolsgold_history)
    assert torch.equal(a.last_weights[perm], b.last_weights)
    assert ((a.last_weights > 0) & (a.last_weights < 1)).any()


# ------------------------------------------------------------- server round

@pytest.mark.parametrize("rlr", [0, 4])
def test_server_round_on_sybils(rlr):
    K, f = 10, 3
    U, bad = sybils(K, f)
    ids = list(range(K))
    assert bad.tolist() != list(range(f))   # not simply the corrupt ids
    _, cs = foolsgold_weights(cpu_gram(U), 1.0)
    assert_sybils_decisive(cs, 1.0, bad)
    want = torch.ones(K, dtype=torch.float64)
    want[bad] = 0.0

    w = Writer()
    agg = make_agg(N, 'cpu', num_agents=K, num_corrupt=f,
                   robustLR_threshold=rlr, writer=w)
    gm = FlatParamModel(P(N), 'cpu')
    agg.aggregate_updates(gm, U, 3, agent_ids=ids)
    assert torch.equal(agg.last_weights, want)

    mean = _row_sum(U, want) * (1.0 / K)
    if rlr:
        sm = torch.sign(U).sum(0).abs()
        mean = torch.where(sm >= rlr, mean, -mean)
    assert torch.equal(gm.flat_params.detach(), (0.0 + mean).float())

    bad_ids = [p for p in range(K) if ids[p] < f]
    good_ids = [p for p in range(K) if ids[p] >= f]
    assert w.last['FoolsGold/Corrupt_Alpha_Mean'] == (
        float(want[bad_ids].mean()), 3)
    assert w.last['FoolsGold/Honest_Alpha_Mean'] == (
        float(want[good_ids].mean()), 3)


class _BN(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.bn = torch.nn.BatchNorm1d(3)


def test_buffers_take_alpha_and_divisor_k():
    K, f = 10, 3
    U, bad = sybils(K, f)
    agg = make_agg(N, 'cpu', num_agents=K)
    agg.agg_foolsgold(U, list(range(K)))
    alpha = agg.last_weights
    gm = FlatParamModel(_BN(), 'cpu')
    assert gm.n_buffers > 0
    before = gm.flat_buffers.clone()
    deltas = randn(K, gm.n_buffers, seed=3).float()
    agg.aggregate_buffers(gm, deltas, list(range(K)))
    want = (deltas.double() * alpha.unsqueeze(1)).sum(0) * (1.0 / K)
    assert torch.equal(gm.flat_buffers, before + want.to(before.dtype))
    # K, not sum(alpha) = K - f
    assert float(alpha.sum()) == K - f


# ---------------------------------------------------------- argument checks

def test_bad_ids_raise():
    U = randn(3)
    agg = make_agg(N, 'cpu', num_agents=5)
    for ids in ([0, 1, 1], [0, 1, 5], [0, -1, 2], [0, 1]):
        with pytest.raises(ValueError):
            agg.agg_foolsgold(U, ids)
    assert agg.foolsgold_history is None or not agg.foolsgold_history.any()


@pytest.mark.parametrize("kappa", [0.0, -1.0, float('nan')])
def test_kappa_is_checked_everywhere(kappa):
    from rlr_amd.options import args_parser, default_args
    with pytest.raises(SystemExit):
        args_parser(['--aggr', 'foolsgold', '--foolsgold_kappa', str(kappa)])
    with pytest.raises(ValueError):
        default_args(aggr='foolsgold', foolsgold_kappa=kappa)
    agg = make_agg(N, 'cpu', num_agents=3)
    agg.args.foolsgold_kappa = kappa
    with pytest.raises(ValueError):
        agg.agg_foolsgold(randn(3), [0, 1, 2])


def test_parser_accepts_the_rule():
    from rlr_amd.options import args_parser
    a = args_parser(['--aggr', 'foolsgold', '--foolsgold_kappa', '0.5',
                     '--server_lr', '3'])
    assert a.aggr == 'foolsgold' and a.foolsgold_kappa == 0.5
    assert a.server_lr == 1.0


def test_run_name_and_banner(capsys):
    from rlr_amd.options import default_args
    from rlr_amd.utils.logging import print_exp_details, run_name
    fg = default_args(aggr='foolsgold', foolsgold_kappa=0.5, num_agents=10)
    assert '-fg_kappa:0.5' in run_name(fg)
    print_exp_details(fg)
    out = capsys.readouterr().out
    assert 'FoolsGold kappa: 0.5' in out
    assert '96 MB' in out               # 8 * 10 * 1199882 bytes
    for aggr in ('avg', 'comed', 'sign', 'trmean', 'krum', 'geomed',
                 'bulyan'):
        other = default_args(aggr=aggr, foolsgold_kappa=0.5)
        assert 'fg_kappa' not in run_name(other)
        print_exp_details(other)
        assert 'FoolsGold' not in capsys.readouterr().out


# --------------------------------------------------------------- checkpoint

def _args(tmp, **over):
    from rlr_amd.options import default_args
    base = dict(num_agents=2, rounds=4, snap=1, local_ep=1, bs=64,
                synthetic=True, no_tb=True, data='fmnist', num_corrupt=1,
                poison_frac=0.5, aggr='foolsgold', ckpt_dir=str(tmp))
    base.update(over)
    return default_args(**base)


def test_resume_bitwise_identical(tmp_path, tiny_sizes):
    from rlr_amd.federated import run
    h_full = run(_args(tmp_path / 'full'))
    run(_args(tmp_path / 'half', rounds=2))
    ck = os.path.join(str(tmp_path / 'half'), 'round_000002.pt')
    state = torch.load(ck, weights_only=False)
    assert state['version'] == 1
    H = state['server_state']['foolsgold_history']
    assert H.shape == (2, 1_199_882) and H.dtype == torch.float64
    assert H.any()
    h_res = run(_args(tmp_path / 'resumed', resume=ck))
    assert torch.equal(h_full['final_params'], h_res['final_params'])


def test_other_rules_write_no_server_state(tmp_path, tiny_sizes):
    from rlr_amd.federated import run
    run(_args(tmp_path, rounds=1, aggr='avg'))
    ck = os.path.join(str(tmp_path), 'round_000001.pt')
    state = torch.load(ck, weights_only=False)
    assert 'server_state' not in state
    assert set(state) == {'version', 'round', 'args', 'seed', 'params',
                          'cum_poison_acc_mean'}
    # and foolsgold refuses to resume from it
    with pytest.raises(ValueError, match='FoolsGold history'):
        run(_args(tmp_path / 'fg', rounds=2, resume=ck))


# --------------------------------------------------------------- world size

def test_world_size_invariance():
    one = server_helpers.run_world(1, 29840, aggr='foolsgold')
    two = server_helpers.run_world(2, 29840, aggr='foolsgold')
    assert torch.equal(one, two)
