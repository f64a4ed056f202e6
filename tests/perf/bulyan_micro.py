"""Microbenchmark of Bulyan on the GPU (bulyan_k in ops/csrc/orderstat.hip
and the device selection loop of aggregation.py) against what it replaces,
at the workload shapes (K sampled agents, f assumed Byzantine, n
parameters): FMNIST K=10, CIFAR10 K=40, Fed-EMNIST --agent_frac 0.1 K=338.

Usage: python tests/perf/bulyan_micro.py [--rounds R] [--out FILE.md]

Per shape it times
  selection: the iterated-Krum loop given D | with pairwise_sqdist in front
  trim     : bulyan_trim | the torch rule (bulyan_window_mean) on the device
  server   : fused bulyan_rlr_apply | rlr_vote + bulyan_trim + apply_update
             | rlr_vote + torch rule + apply_update
  yardstick: the fused trimmed mean orderstat_rlr_apply at the same K and n
             (trim_frac 0.1): the nearest existing work, the same sort over
             the larger K-row tile
Method: as orderstat_micro.py — every variant is warmed up, one call is
timed to size a window of at least ~0.25 s of device work, then R rounds
visit the variants of a shape in ALTERNATING order, each window timed with
device events.  The table gives the median ms per call over the rounds and
the min..max spread; the outputs of kernel and torch rule are compared with
torch.equal at the timed size first."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..', '..'))
import torch  # noqa: E402

from rlr_amd.aggregation import Aggregation, bulyan_window_mean  # noqa: E402
from rlr_amd.ops import ext  # noqa: E402
from rlr_amd.options import default_args  # noqa: E402

DEV = 'cuda:0'
SHAPES = [(10, 1, 1199882), (40, 4, 537610), (338, 33, 1199882)]
TRIM_FRAC = 0.1
THETA_FRAC = 0.2


def window_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bulyan_micro needs a GPU")
    e = ext()
    none = torch.empty(0, device=DEV)
    lines = ['| K | f | theta | beta | n | what | variant | ms/call median '
             '| min..max | calls/window |',
             '|---|---|---|---|---|---|---|---|---|---|']
    for K, f, n in SHAPES:
        torch.manual_seed(K)
        U = torch.randn(K, n, dtype=torch.float64, device=DEV) * 1e-2
        params = torch.zeros(n, device=DEV)
        agg = Aggregation({}, n, None,
                          default_args(aggr='bulyan', bulyan_f=f, device=DEV,
                                       no_tb=True))
        theta, beta = agg._bulyan_counts(K)
        vote = float(max(1, int(THETA_FRAC * K)))
        b = int(TRIM_FRAC * K)
        D = agg.pairwise_sqdist(U)
        sel = agg.bulyan_picks(D)
        perm = agg._bulyan_perm(sel, K)

        def trim():
            return e.bulyan_trim(U, perm, theta, beta, False, 0.0, 0.0)[0]

        def torch_rule():
            return bulyan_window_mean(U[sel], beta)

        def composed(rule):
            lr = e.rlr_vote(U, vote, 1.0)
            e.apply_update(params, rule(), lr, 1.0)

        # kernel and torch rule must agree at the timed size before any
        # timing counts, and so must the fused launch and its composition
        assert torch.equal(trim(), torch_rule())
        p1, p2 = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        e.bulyan_rlr_apply(U, perm, theta, beta, p1, True, vote, 1.0, False)
        e.apply_update(p2, trim(), e.rlr_vote(U, vote, 1.0), 1.0)
        assert torch.equal(p1, p2)
        del p1, p2

        v = [
            ('selection', 'iterated-Krum loop given D',
             lambda: agg.bulyan_picks(D)),
            ('selection', 'pairwise_sqdist + loop',
             lambda: agg.bulyan_select(U)),
            ('trim', 'bulyan_trim', trim),
            ('trim', 'torch rule on the device', torch_rule),
            ('server', 'fused bulyan_rlr_apply',
             lambda: e.bulyan_rlr_apply(U, perm, theta, beta, params, True,
                                        vote, 1.0, False)),
            ('server', 'rlr_vote + bulyan_trim + apply_update',
             lambda: composed(trim)),
            ('server', 'rlr_vote + torch rule + apply_update',
             lambda: composed(torch_rule)),
            ('yardstick', f'fused trmean orderstat_rlr_apply, all {K} rows',
             lambda: e.orderstat_rlr_apply(U, b, K - b, params, True, vote,
                                           1.0, False)),
        ]
        iters = []
        for _, _, fn in v:
            fn()
            fn()
            torch.cuda.synchronize()
            t1 = window_ms(fn, 1)
            iters.append(max(1, min(200, int(250.0 / max(t1, 1e-3)))))
        times = [[] for _ in v]
        for r in range(a.rounds):
            order = range(len(v)) if r % 2 == 0 else reversed(range(len(v)))
            for i in order:
                times[i].append(window_ms(v[i][2], iters[i]))
        for (what, name, _), t, it in zip(v, times, iters):
            lines.append(f'| {K} | {f} | {theta} | {beta} | {n} | {what} | '
                         f'{name} | {statistics.median(t):.3f} | '
                         f'{min(t):.3f}..{max(t):.3f} | {it} |')
            print(lines[-1], flush=True)
        del U, params, v, D
        torch.cuda.empty_cache()
    table = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(table)
    print(table)


if __name__ == '__main__':
    main()
