"""Microbenchmark of the fp64 MFMA pairwise-distance kernel
(ops/csrc/pairdist.hip) and the Krum server step, at the workload shapes
(K sampled agents, n parameters): FMNIST K=10, CIFAR10 K=40, Fed-EMNIST
--agent_frac 0.1 K=338.

Usage: python tests/perf/krum_micro.py [--rounds R] [--out FILE.md]

Per shape it times
  distances: pairwise_sqdist | U @ U.T + elementwise composition in torch
  server   : the whole Krum step (distances, scores, selection, fused
             0/1-weighted average + RLR vote + apply) | the fused FedAvg
             step alone, for scale
Method (that of orderstat_micro.py): every variant is warmed up, one call
is timed to size a window of at least ~0.25 s of device work, then R rounds
visit the variants of a shape in ALTERNATING order, each window timed with
device events.  The table gives the median ms per call over the rounds and
the min..max spread; the outputs of kernel and composition are compared at
the timed size first.

Each distance row is read against two floors, computed from the shape:
  HBM floor  : K n 8 B (U read once) / 8.0 TB/s (spec peak)
  fp64 floor : K (K + 1) n flop (the upper triangle of G incl. diagonal,
               2 flop per product) / 78.6 Tflop/s (spec fp64 matrix peak)"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..', '..'))
import torch  # noqa: E402

from rlr_amd.aggregation import Aggregation  # noqa: E402
from rlr_amd.ops import ext  # noqa: E402
from rlr_amd.options import default_args  # noqa: E402

DEV = 'cuda:0'
SHAPES = [(10, 1199882), (40, 537610), (338, 1199882)]
F_FRAC = 0.1
THETA_FRAC = 0.2
HBM_BPS = 8.0e12
FP64_FLOPS = 78.6e12


def window_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def torch_sqdist(U):
    G = U @ U.T
    g = G.diagonal()
    D = (g.unsqueeze(1) + g.unsqueeze(0) - 2.0 * G).clamp_(min=0.0)
    D.fill_diagonal_(0.0)
    return D


class _Model:
    """What aggregate_updates needs of the global model."""

    def __init__(self, n):
        self.flat_params = torch.zeros(n, device=DEV)
        self.n_buffers = 0


def floors_ms(K, n):
    return (K * n * 8 / HBM_BPS * 1e3, K * (K + 1) * n / FP64_FLOPS * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("krum_micro needs a GPU")
    e = ext()
    lines = ['| K | n | what | variant | ms/call median | min..max | '
             'calls/window | HBM floor ms | fp64 floor ms |',
             '|---|---|---|---|---|---|---|---|---|']
    for K, n in SHAPES:
        torch.manual_seed(K)
        U = torch.randn(K, n, dtype=torch.float64, device=DEV) * 1e-2
        gm = _Model(n)
        ids = list(range(K))
        f = max(1, int(F_FRAC * K))
        theta = max(1, int(THETA_FRAC * K))
        sizes = {i: 10 * (i + 1) for i in ids}
        krum = Aggregation(sizes, n, None, default_args(
            no_tb=True, device=DEV, aggr='krum', krum_f=f,
            robustLR_threshold=theta))
        avg = Aggregation(sizes, n, None, default_args(
            no_tb=True, device=DEV, aggr='avg', robustLR_threshold=theta))

        # kernel and composition must agree at the timed size before any
        # timing counts: to the worst-case dot-product bound, and on what
        # Krum makes of them
        D = e.pairwise_sqdist(U)
        Dt = torch_sqdist(U)
        sq = (U * U).sum(1)
        bound = 4.0 * n * 2.0 ** -53 * (sq.unsqueeze(1) + sq.unsqueeze(0))
        assert ((D - Dt).abs() <= 2 * bound).all()
        assert torch.equal(D, D.T) and (D.diagonal() == 0).all()
        sel = torch.sort(torch.sort(krum.krum_scores(Dt), stable=True)
                         .indices[:K - f]).values
        assert torch.equal(krum.krum_select(U), sel)
        del D, Dt, sq, bound

        hbm, fp = floors_ms(K, n)
        v = [
            ('distances', 'pairwise_sqdist', lambda: e.pairwise_sqdist(U),
             True),
            ('distances', 'U @ U.T + elementwise (torch)',
             lambda: torch_sqdist(U), True),
            ('server', 'krum step',
             lambda: krum.aggregate_updates(gm, U, 1, ids), False),
            ('server', 'fused avg step (for scale)',
             lambda: avg.aggregate_updates(gm, U, 1, ids), False),
        ]
        iters = []
        for _, _, fn, _ in v:
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
        for (what, name, _, fl), t, it in zip(v, times, iters):
            lines.append(f'| {K} | {n} | {what} | {name} | '
                         f'{statistics.median(t):.3f} | '
                         f'{min(t):.3f}..{max(t):.3f} | {it} | '
                         + (f'{hbm:.3f} | {fp:.3f} |' if fl else '- | - |'))
            print(lines[-1], flush=True)
        del U, gm, v
        torch.cuda.empty_cache()
    table = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(table)
    print(table)


if __name__ == '__main__':
    main()
