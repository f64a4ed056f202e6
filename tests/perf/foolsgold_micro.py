"""Microbenchmark of the FoolsGold server kernels (ops/csrc/foolsgold.hip and
the indexed Gram path of ops/csrc/pairdist.hip) and the FoolsGold server
step, at the workload shapes (K sampled agents, n parameters): FMNIST K=10,
CIFAR10 K=40, Fed-EMNIST --agent_frac 0.1 K=338; the history has A = 2 K
rows and the sampled ids are shuffled.

Usage: python tests/perf/foolsgold_micro.py [--rounds R] [--out FILE.md]

Per shape it times
  history: rows_add_ | index_add_ in torch
  gram   : gram_rows | H[idx] @ H[idx].T in torch | pairwise_sqdist on a
           contiguous copy of the sampled rows, for scale
  server : the whole FoolsGold step (history, Gram, weights, fused
           alpha-weighted average + RLR vote + apply) | the fused FedAvg
           step alone, for scale
Method (that of krum_micro.py): every variant is warmed up, one call is
timed to size a window of at least ~0.25 s of device work, then R rounds
visit the variants of a shape in ALTERNATING order, each window timed with
device events.  The table gives the median ms per call over the rounds and
the min..max spread; the outputs of kernel and composition are compared at
the timed size first.

Each row is read against two floors, computed from the shape:
  HBM floor  : history 3 K n 8 B (U read, H read and written), gram
               K n 8 B (the sampled rows read once) / 8.0 TB/s (spec peak)
  fp64 floor : gram K (K + 1) n flop (the upper triangle of G incl.
               diagonal, 2 flop per product) / 78.6 Tflop/s (spec fp64
               matrix peak); none for the history add"""

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


class _Model:
    """What aggregate_updates needs of the global model."""

    def __init__(self, n):
        self.flat_params = torch.zeros(n, device=DEV)
        self.n_buffers = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("foolsgold_micro needs a GPU")
    e = ext()
    lines = ['| K | n | what | variant | ms/call median | min..max | '
             'calls/window | HBM floor ms | fp64 floor ms |',
             '|---|---|---|---|---|---|---|---|---|']
    for K, n in SHAPES:
        A = 2 * K
        torch.manual_seed(K)
        U = torch.randn(K, n, dtype=torch.float64, device=DEV) * 1e-2
        H = torch.randn(A, n, dtype=torch.float64, device=DEV) * 1e-2
        idx = torch.randperm(A)[:K].contiguous()
        idx_dev = idx.to(DEV)
        ids = idx.tolist()
        gm = _Model(n)
        theta = max(1, int(THETA_FRAC * K))
        sizes = {i: 10 * (i + 1) for i in range(A)}
        fg = Aggregation(sizes, n, None, default_args(
            no_tb=True, device=DEV, aggr='foolsgold', num_agents=A,
            robustLR_threshold=theta))
        avg = Aggregation(sizes, n, None, default_args(
            no_tb=True, device=DEV, aggr='avg', num_agents=A,
            robustLR_threshold=theta))

        # kernel and composition must agree at the timed size before any
        # timing counts: the history bit for bit, the Gram matrix to the
        # worst-case dot-product bound
        H1 = H.clone()
        e.rows_add_(H1, idx, U)
        assert torch.equal(H1, H.clone().index_add_(0, idx_dev, U))
        del H1
        G = e.gram_rows(H, idx)
        Hs = H[idx_dev]
        Gt = Hs @ Hs.T
        nrm = torch.sqrt((Hs * Hs).sum(1))
        bound = 2.0 * n * 2.0 ** -53 * nrm.unsqueeze(1) * nrm.unsqueeze(0)
        assert ((G - Gt).abs() <= bound).all()
        assert torch.equal(G, G.T)
        del G, Gt, nrm, bound

        v = [
            ('history', 'rows_add_', lambda: e.rows_add_(H, idx, U),
             (3 * K * n * 8 / HBM_BPS * 1e3, None)),
            ('history', 'index_add_ (torch)',
             lambda: H.index_add_(0, idx_dev, U),
             (3 * K * n * 8 / HBM_BPS * 1e3, None)),
            ('gram', 'gram_rows', lambda: e.gram_rows(H, idx),
             (K * n * 8 / HBM_BPS * 1e3, K * (K + 1) * n / FP64_FLOPS * 1e3)),
            ('gram', 'H[idx] @ H[idx].T (torch)',
             lambda: H[idx_dev] @ H[idx_dev].T,
             (K * n * 8 / HBM_BPS * 1e3, K * (K + 1) * n / FP64_FLOPS * 1e3)),
            ('gram', 'pairwise_sqdist on a contiguous copy (for scale)',
             lambda: e.pairwise_sqdist(Hs),
             (K * n * 8 / HBM_BPS * 1e3, K * (K + 1) * n / FP64_FLOPS * 1e3)),
            ('server', 'foolsgold step',
             lambda: fg.aggregate_updates(gm, U, 1, ids), None),
            ('server', 'fused avg step (for scale)',
             lambda: avg.aggregate_updates(gm, U, 1, ids), None),
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
            hbm = f'{fl[0]:.3f}' if fl else '-'
            fp = f'{fl[1]:.3f}' if fl and fl[1] is not None else '-'
            lines.append(f'| {K} | {n} | {what} | {name} | '
                         f'{statistics.median(t):.3f} | '
                         f'{min(t):.3f}..{max(t):.3f} | {it} | '
                         f'{hbm} | {fp} |')
            print(lines[-1], flush=True)
        del U, H, Hs, gm, v, fg, avg
        torch.cuda.empty_cache()
    table = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(table)
    print(table)


if __name__ == '__main__':
    main()
