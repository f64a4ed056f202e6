"""Server-side update-norm clipping (--server_clip, --server_clip_mode) and
the boosted attack (--attack_boost) on the CPU path: CLI surface, the rule on
hand-computed cases, the norm guarantees in exact arithmetic, the RLR vote,
the default-off identity, the boost, composition with krum and geomed,
buffers, noise, logging and the run name."""

import argparse
import functools
from fractions import Fraction
from time import ctime

import pytest
import torch

from rlr_amd.options import args_parser, default_args
from rlr_amd.utils.logging import print_exp_details, run_name

import server_helpers
from server_helpers import P as _P, Writer, t64

NEW_FLAGS = ('server_clip', 'server_clip_mode', 'attack_boost')
# the issue's slack on a clipped norm: tau * (1 + 4 * 2^-52)
SLACK = Fraction(4, 2 ** 52)


make_agg = functools.partial(server_helpers.make_agg, n=4, dev='cpu')


def exact_sq_norm(row):
    return sum(Fraction(float(v)) ** 2 for v in row.tolist())


def rows_of_many_scales(K, n, seed):
    g = torch.Generator().manual_seed(seed)
    U = torch.randn(K, n, dtype=torch.float64, generator=g)
    e = torch.linspace(-3, 3, K, dtype=torch.float64)
    return U * (10.0 ** e).unsqueeze(1)


# --------------------------------------------------------------------- CLI

@pytest.mark.parametrize("flags", [
    ['--server_clip=-1'], ['--server_clip=-1e-9'], ['--server_clip=nan'],
    ['--attack_boost=0'], ['--attack_boost=-2'], ['--attack_boost=nan'],
    ['--server_clip', '1', '--server_clip_mode', 'mean'],
    ['--server_clip_mode', 'Median']])
def test_cli_rejects_at_parse_time(flags):
    with pytest.raises(SystemExit):
        args_parser(['--device', 'cpu'] + flags)


def test_cli_accepts_and_defaults():
    d = default_args(device='cpu')
    assert (d.server_clip, d.server_clip_mode, d.attack_boost) == \
        (0, 'fixed', 1.0)
    a = args_parser(['--server_clip', '2.5', '--server_clip_mode', 'median',
                     '--attack_boost', '20', '--device', 'cpu'])
    assert (a.server_clip, a.server_clip_mode, a.attack_boost) == \
        (2.5, 'median', 20.0)
    with pytest.raises(ValueError):
        default_args(device='cpu', server_clip_mode='mean')
    with pytest.raises(ValueError):
        default_args(device='cpu', attack_boost=0.0)


def test_run_name_and_banner_only_when_switched_on(capsys):
    base = dict(clip=3.0, noise=0.1, aggr='comed', num_corrupt=4,
                robustLR_threshold=8, pattern_type='square', device='cpu')
    plain = default_args(**base)
    old = argparse.Namespace(**{k: v for k, v in vars(plain).items()
                                if k not in NEW_FLAGS})
    on = default_args(server_clip=2.5, server_clip_mode='median',
                      attack_boost=7.5, **base)
    before = ctime()
    names = run_name(plain), run_name(old), run_name(on)
    after = ctime()

    def expect(t, tail=''):
        return (f"time:{t}-clip_val:3.0-noise_std:0.1-aggr:comed-s_lr:1.0"
                f"-num_cor:4thrs_robustLR:8-num_corrupt:4-pttrn:square"
                + tail)

    assert names[0] in (expect(before), expect(after))
    assert names[1] in (expect(before), expect(after))
    tail = '-sclip:2.5-median-boost:7.5'
    assert names[2] in (expect(before, tail), expect(after, tail))
    assert 'boost' not in run_name(default_args(server_clip=1.0, **base))
    assert 'sclip' not in run_name(default_args(attack_boost=2.0, **base))

    print_exp_details(plain)
    off = capsys.readouterr().out
    print_exp_details(old)
    assert capsys.readouterr().out == off
    assert 'Server Clip' not in off and 'Boost' not in off
    print_exp_details(on)
    out = capsys.readouterr().out
    assert '    Server Clip: 2.5 (median)\n' in out
    assert [ln for ln in out.splitlines()
            if 'Server Clip' not in ln and 'Attack Boost' not in ln] \
        == off.splitlines()


# ------------------------------------------------------ the rule, by hand
# norms 5, 0, 10.  Row 0 sits exactly on tau = 5, row 1 is zero.
U_HAND = t64([[1, 2, 2, 4], [0, 0, 0, 0], [2, 4, 4, 8]])


@pytest.mark.parametrize("mode,value,tau,s", [
    ('fixed', 5.0, 5.0, [1.0, 1.0, 0.5]),
    ('median', 1.0, 5.0, [1.0, 1.0, 0.5]),      # the median agent: == tau
    ('median', 0.5, 2.5, [0.5, 1.0, 0.25]),
    ('fixed', 20.0, 20.0, [1.0, 1.0, 1.0]),
    ('fixed', 1.25, 1.25, [0.25, 1.0, 0.125])])
def test_rule_by_hand(mode, value, tau, s):
    agg = make_agg(server_clip=value, server_clip_mode=mode)
    U = U_HAND.clone()
    C = agg.server_clip_updates(U)
    assert torch.equal(U, U_HAND)               # the CPU path copies
    assert agg.last_norms.tolist() == [5.0, 0.0, 10.0]
    assert float(agg.last_clip_bound) == tau
    assert agg.last_clip_bound.dtype == torch.float64
    assert agg.last_clip_scale.tolist() == s
    assert torch.equal(C, t64(s).unsqueeze(1) * U_HAND)
    for k in range(3):
        if s[k] == 1.0:
            assert torch.equal(C[k], U_HAND[k])
    assert not torch.isnan(C).any()             # the zero row: no 0 / 0


def test_even_k_takes_the_lower_median():
    # norms 1, 2, 3, 4: the lower of the two middle values is 2
    U = t64([[4, 0], [0, 1], [3, 0], [0, 2]])
    agg = make_agg(n=2, server_clip=1.0, server_clip_mode='median')
    agg.server_clip_updates(U)
    assert float(agg.last_clip_bound) == 2.0
    assert agg.last_clip_scale.tolist() == [0.5, 1.0, 2.0 / 3.0, 1.0]


def test_mode_and_value_are_checked_by_the_server_too():
    agg = make_agg(server_clip=1.0)
    agg.args.server_clip_mode = 'mean'
    with pytest.raises(ValueError):
        agg.server_clip_updates(U_HAND)


# ------------------------------------------------------------- guarantees
# Checked in exact rational arithmetic, so the check adds no rounding of its
# own.  With n <= 8 the slack is provable: the computed norm is within
# (n / 2 + 1) 2^-53 of the true one, s = tau / norm and each product add one
# rounding each: (n / 2 + 3) 2^-53 <= 7 * 2^-53 < 4 * 2^-52.

@pytest.mark.parametrize("n", [5, 8])
@pytest.mark.parametrize("tau", [1.0, 0.3, 17.0])
def test_clipped_norms_are_bounded(n, tau):
    U = rows_of_many_scales(64, n, seed=n)
    agg = make_agg(n=n, server_clip=tau)
    C = agg.server_clip_updates(U)
    cap = (Fraction(tau) * (1 + SLACK)) ** 2
    clipped = 0
    for k in range(64):
        assert exact_sq_norm(C[k]) <= cap, k
        if agg.last_clip_scale[k] < 1.0:
            clipped += 1
            # and not shrunk further than rounding: the norm is tau
            assert exact_sq_norm(C[k]) >= (Fraction(tau) * (1 - SLACK)) ** 2
        else:
            assert torch.equal(C[k], U[k])
    assert 0 < clipped < 64


def test_avg_aggregate_norm_is_bounded():
    tau = 0.7
    cap = (Fraction(tau) * (1 + SLACK)) ** 2
    agg = make_agg(n=8, server_clip=tau)
    U = rows_of_many_scales(16, 8, seed=3)
    out = agg.agg_avg(agg.server_clip_updates(U), list(range(16)))
    assert exact_sq_norm(out) <= cap
    assert exact_sq_norm(out) < exact_sq_norm(
        agg.agg_avg(U, list(range(16))))
    # the triangle inequality's worst case: every row the same, far outside
    # the ball (equal weights, K = 2: the mean of C and C is C exactly)
    agg = make_agg(n=8, server_clip=tau)
    agg.agent_data_sizes = {0: 16, 1: 16}
    same = (1e3 * U[7]).repeat(2, 1)
    out = agg.agg_avg(agg.server_clip_updates(same), [0, 1])
    assert exact_sq_norm(out) <= cap
    assert exact_sq_norm(out) >= (Fraction(tau) * (1 - SLACK)) ** 2


def test_through_the_server_the_aggregate_is_bounded():
    tau = 0.05
    U = rows_of_many_scales(10, 8, seed=11)
    from rlr_amd.flatmodel import FlatParamModel
    gm = FlatParamModel(_P(8), 'cpu')
    agg = make_agg(n=8, server_clip=tau)
    agg.aggregate_updates(gm, U, cur_round=1, agent_ids=list(range(10)))
    # the parameters are fp32(0 + 1 * aggregate): 2^-24 relative each
    assert float(gm.flat_params.double().norm()) <= tau * (1 + 2.0 ** -23)
    assert torch.equal(agg.last_norms, torch.sqrt((U * U).sum(1)))


@pytest.mark.parametrize("mode", ['fixed', 'median'])
def test_vote_is_unchanged(mode):
    g = torch.Generator().manual_seed(5)
    U = rows_of_many_scales(9, 64, seed=5)
    U[torch.rand(9, 64, generator=g) < 0.2] = 0.0
    agg = make_agg(n=64, server_clip=0.5, server_clip_mode=mode,
                   robustLR_threshold=4)
    C = agg.server_clip_updates(U)
    assert (agg.last_clip_scale < 1.0).any()
    assert torch.equal(torch.sign(C), torch.sign(U))
    assert torch.equal(agg.compute_robustLR(C), agg.compute_robustLR(U))


# ---------------------------------------------------------- default is off

def _old_namespace(args):
    """The same run as a caller that predates the new flags would set it
    up: no server_clip, server_clip_mode or attack_boost attribute."""
    return argparse.Namespace(**{k: v for k, v in vars(args).items()
                                 if k not in NEW_FLAGS})


def test_default_is_off_bitwise(tiny_args, tiny_sizes):
    from rlr_amd.federated import run
    tiny_args.num_agents = 3
    tiny_args.num_corrupt = 1
    tiny_args.poison_frac = 0.5
    tiny_args.device = 'cpu'
    tiny_args.clip = 2.0
    assert (tiny_args.server_clip, tiny_args.attack_boost) == (0, 1.0)
    old = _old_namespace(tiny_args)
    assert not any(hasattr(old, f) for f in NEW_FLAGS)
    h_new = run(tiny_args)
    h_old = run(old)
    assert torch.isfinite(h_new['final_params']).all()
    assert torch.equal(h_new['final_params'], h_old['final_params'])


@pytest.mark.parametrize("aggr", ['avg', 'comed', 'krum', 'geomed'])
def test_default_leaves_the_server_alone(aggr):
    from rlr_amd.flatmodel import FlatParamModel
    U = rows_of_many_scales(7, 16, seed=2)
    ids = list(range(7))
    out = []
    for strip in (False, True):
        agg = make_agg(n=16, aggr=aggr, noise=0.01, clip=1.5,
                       robustLR_threshold=3)
        if strip:
            agg.args = _old_namespace(agg.args)
        gm = FlatParamModel(_P(16), 'cpu')
        keep = U.clone()
        agg.aggregate_updates(gm, keep, cur_round=3, agent_ids=ids)
        assert torch.equal(keep, U)
        assert agg.last_clip_scale is None and agg.last_norms is None
        out.append(gm.flat_params.detach().clone())
    assert torch.equal(out[0], out[1])


# ------------------------------------------------------------------- boost

def _updates(args, rnd=1):
    from rlr_amd.federated import build_world
    world = build_world(args)
    gm = world['global_model']
    before = gm.flat_params.detach().clone()
    ups = [a.local_train(gm, rnd=rnd).clone() for a in world['agents']]
    assert torch.equal(gm.flat_params.detach(), before)
    return ups


def test_boost_scales_the_corrupt_update_only(tiny_args, tiny_sizes):
    tiny_args.device = 'cpu'
    tiny_args.num_corrupt = 1
    tiny_args.poison_frac = 0.5
    tiny_args.clip = 0.5            # the client's own projection is on
    plain = _updates(tiny_args)
    tiny_args.attack_boost = 7.5
    boosted = _updates(tiny_args)
    assert plain[0].dtype == torch.float64 and plain[0].abs().max() > 0
    assert torch.equal(boosted[0], 7.5 * plain[0])      # agent 0 is corrupt
    assert torch.equal(boosted[1], plain[1])            # agent 1 is honest
    # the boost escapes the client's ball
    assert float(plain[0].float().norm()) <= 0.5 * (1 + 1e-5)
    assert float(boosted[0].norm()) > 0.5


def test_boost_scales_the_buffer_delta():
    from rlr_amd.agent import Agent
    from rlr_amd.flatmodel import FlatParamModel
    from rlr_amd.models.cnn import _OpsModel

    class BN(_OpsModel):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(6, 3)
            self.bn = torch.nn.BatchNorm1d(3)

        def forward(self, x):
            return self.bn(self.fc(x.flatten(1)))

    g = torch.Generator().manual_seed(0)
    X = torch.randn(32, 6, generator=g)
    Y = torch.randint(0, 3, (32,), generator=g)
    got = {}
    for boost in (1.0, 4.0):
        args = default_args(no_tb=True, device='cpu', bs=16, local_ep=1,
                            num_corrupt=1, attack_boost=boost)
        for aid in (0, 1):
            torch.manual_seed(1)
            gm = FlatParamModel(BN(), 'cpu')
            a = Agent.__new__(Agent)
            a.id, a.args, a.device = aid, args, torch.device('cpu')
            a._X, a._Y = X, Y
            up = a.local_train(gm, rnd=1)
            got[boost, aid] = (up.clone(), a.buffer_delta.clone())
    assert got[1.0, 0][1].abs().max() > 0
    assert torch.equal(got[4.0, 0][0], 4.0 * got[1.0, 0][0])
    assert torch.equal(got[4.0, 0][1], 4.0 * got[1.0, 0][1])
    assert torch.equal(got[4.0, 1][0], got[1.0, 1][0])
    assert torch.equal(got[4.0, 1][1], got[1.0, 1][1])


# ------------------------------------------------------------- composition

def _outlier_matrix():
    g = torch.Generator().manual_seed(9)
    base = torch.randn(32, dtype=torch.float64, generator=g)
    U = base + 0.3 * torch.randn(8, 32, dtype=torch.float64, generator=g)
    U[5] = 1e3 * U[5]
    return U


@pytest.mark.parametrize("mode,value", [('fixed', 4.0), ('median', 1.0)])
def test_krum_and_geomed_see_the_clipped_matrix(mode, value):
    from rlr_amd.flatmodel import FlatParamModel
    U = _outlier_matrix()
    ids = list(range(8))
    clip = make_agg(n=32, server_clip=value, server_clip_mode=mode)
    C = clip.server_clip_updates(U)
    s = clip.last_clip_scale
    assert s[5] < 1e-2 and torch.equal(C, s.unsqueeze(1) * U)

    for aggr in ('krum', 'geomed'):
        res = {}
        for on in (False, True):
            over = dict(server_clip=value, server_clip_mode=mode) if on else {}
            agg = make_agg(n=32, aggr=aggr, krum_f=1, krum_m=7, **over)
            gm = FlatParamModel(_P(32), 'cpu')
            agg.aggregate_updates(gm, U.clone(), cur_round=1, agent_ids=ids)
            res[on] = (agg, gm.flat_params.detach().clone())
        hand = make_agg(n=32, aggr=aggr, krum_f=1, krum_m=7)
        gm = FlatParamModel(_P(32), 'cpu')
        hand.aggregate_updates(gm, s.unsqueeze(1) * U, cur_round=1,
                               agent_ids=ids)
        assert torch.equal(res[True][1], gm.flat_params.detach())
        assert not torch.equal(res[True][1], res[False][1])
        if aggr == 'krum':
            assert torch.equal(res[True][0].last_selected, hand.last_selected)
            assert torch.equal(res[False][0].last_selected,
                               make_agg(n=32, aggr='krum', krum_f=1,
                                        krum_m=7).krum_select(U))
            assert 5 not in res[False][0].last_selected.tolist()
        else:
            assert torch.equal(res[True][0].last_weights, hand.last_weights)
            w_off, w_on = res[False][0].last_weights, res[True][0].last_weights
            assert not torch.equal(w_on, w_off)
            assert w_on[5] > 10 * w_off[5]      # no longer a far outlier


# ------------------------------------------------------------------ buffers

def test_buffers_are_scaled_by_the_clip_factors():
    from rlr_amd.flatmodel import FlatParamModel

    class BN(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(4))
            self.register_buffer('b', torch.zeros(3))

    ids = [2, 0, 1]
    deltas = torch.tensor([[4.0, 0, 8], [0, 4, 8], [2, 2, 2]])
    sizes = t64([30, 10, 20])               # make_agg: 10 * (id + 1)
    w = sizes / sizes.sum()

    agg = make_agg(server_clip=5.0)
    gm = FlatParamModel(BN(), 'cpu')
    agg.aggregate_updates(gm, U_HAND, cur_round=1, agent_ids=ids)
    assert agg.last_clip_scale.tolist() == [1.0, 1.0, 0.5]
    agg.aggregate_buffers(gm, deltas, ids)
    want = (deltas.double() * t64([1.0, 1.0, 0.5]).unsqueeze(1)
            * w.unsqueeze(1)).sum(0)
    assert torch.allclose(gm.flat_buffers.double(), want, rtol=1e-6)

    # a known s, set by hand; and with the flag off it is not used
    for value, s in ((5.0, [0.25, 1.0, 0.5]), (0.0, [1.0, 1.0, 1.0])):
        agg = make_agg(server_clip=value)
        agg.last_clip_scale = t64([0.25, 1.0, 0.5])
        gm = FlatParamModel(BN(), 'cpu')
        agg.aggregate_buffers(gm, [d for d in deltas], ids)
        want = (deltas.double() * t64(s).unsqueeze(1)
                * w.unsqueeze(1)).sum(0)
        assert torch.allclose(gm.flat_buffers.double(), want, rtol=1e-6)


# -------------------------------------------------------- noise and logging

def test_noise_std_follows_the_enforced_bound():
    assert make_agg(noise=0.5, clip=3.0)._noise_std() == 1.5
    assert make_agg(noise=0.5, clip=3.0, server_clip=0.2)._noise_std() == 0.1
    assert make_agg(noise=0.5, clip=3.0, server_clip=0.2,
                    server_clip_mode='median')._noise_std() == 1.5
    a = make_agg(noise=0.5, clip=3.0, server_clip=0.25)
    b = make_agg(noise=0.5, clip=0.25)
    assert torch.equal(a._noise(4, 'cpu', torch.float64),
                       b._noise(4, 'cpu', torch.float64))


def test_clip_scalars_are_logged():
    from rlr_amd.flatmodel import FlatParamModel
    w = Writer()
    agg = make_agg(writer=w, server_clip=5.0, num_corrupt=2)
    gm = FlatParamModel(_P(4), 'cpu')
    # ids 1 and 0 are corrupt: sampled positions 2 and 1, s = 0.5 and 1
    agg.aggregate_updates(gm, U_HAND, cur_round=6, agent_ids=[4, 0, 1])
    assert w.last['Clip/Bound'] == (5.0, 6)
    assert w.last['Clip/Frac_Clipped'][0] == pytest.approx(1 / 3)
    assert w.last['Clip/Corrupt_Scale_Mean'] == (0.75, 6)
    assert all(isinstance(v, float) for v, _ in w.last.values())


def test_dict_api_leaves_the_callers_tensors_alone():
    from rlr_amd.flatmodel import FlatParamModel
    agg = make_agg(server_clip=5.0)
    gm = FlatParamModel(_P(4), 'cpu')
    ups = {i: U_HAND[i].clone() for i in range(3)}
    agg.aggregate_updates(gm, ups, cur_round=1)
    for i in range(3):
        assert torch.equal(ups[i], U_HAND[i])
    assert agg.last_clip_scale.tolist() == [1.0, 1.0, 0.5]
