"""Microbenchmark of the LDS order-statistic kernels (ops/csrc/orderstat.hip)
against what they replace, at the workload shapes (K sampled agents, n
parameters): FMNIST K=10, CIFAR10 K=40, Fed-EMNIST --agent_frac 0.1 K=338.

Usage: python tests/perf/orderstat_micro.py [--rounds R] [--out FILE.md]

Per shape it times
  median : agg_orderstat | agg_comed_k (K <= 64) | device torch.median
  trimmed: agg_orderstat | torch.sort + ascending row loop (trim_frac 0.1)
  server : fused orderstat_rlr_apply | rlr_vote + rule + apply_update
Method: every variant is warmed up, one call is timed to size a window of
at least ~0.25 s of device work, then R rounds visit the variants of a shape
in ALTERNATING order, each window timed with device events.  The table
gives the median ms per call over the rounds and the min..max spread, and
the outputs of old and new code are compared at the timed size first."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..', '..'))
import torch  # noqa: E402

from rlr_amd.ops import ext  # noqa: E402

DEV = 'cuda:0'
SHAPES = [(10, 1199882), (40, 537610), (338, 1199882)]
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


def torch_trmean(U, b):
    K = U.shape[0]
    kept = torch.sort(U, dim=0).values[b:K - b]
    out = torch.zeros(U.shape[1], dtype=torch.float64, device=U.device)
    for r in range(K - 2 * b):
        out += kept[r]
    return out * (1.0 / (K - 2 * b))


def variants(e, U, params):
    K = U.shape[0]
    m = (K - 1) // 2
    b = int(TRIM_FRAC * K)
    theta = float(max(1, int(THETA_FRAC * K)))
    none = torch.empty(0, device=DEV)

    def old_median(U):
        return e.agg_comed(U) if K <= 64 else torch.median(U, 0).values

    def seq(rule):
        lr = e.rlr_vote(U, theta, 1.0)
        e.apply_update(params, rule(U), lr, 1.0)

    v = [('median', 'agg_orderstat',
          lambda: e.agg_orderstat(U, m, m + 1, False, 0.0, 0.0)[0])]
    if K <= 64:
        v.append(('median', 'agg_comed_k', lambda: e.agg_comed(U)))
    v += [
        ('median', 'torch.median', lambda: torch.median(U, 0).values),
        ('trimmed', 'agg_orderstat',
         lambda: e.agg_orderstat(U, b, K - b, False, 0.0, 0.0)[0]),
        ('trimmed', 'torch.sort + row loop', lambda: torch_trmean(U, b)),
        ('server median', 'fused orderstat_rlr_apply',
         lambda: e.orderstat_rlr_apply(U, m, m + 1, params, True, theta, 1.0,
                                       False)),
        ('server median', 'rlr_vote + '
         + ('agg_comed_k' if K <= 64 else 'torch.median') + ' + apply_update',
         lambda: seq(old_median)),
        ('server trimmed', 'fused orderstat_rlr_apply',
         lambda: e.orderstat_rlr_apply(U, b, K - b, params, True, theta, 1.0,
                                       False)),
        ('server trimmed', 'rlr_vote + agg_orderstat + apply_update',
         lambda: seq(lambda U: e.agg_orderstat(U, b, K - b, False, 0.0,
                                               0.0)[0])),
    ]
    return v, m, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("orderstat_micro needs a GPU")
    e = ext()
    lines = ['| K | n | what | variant | ms/call median | min..max | calls/window |',
             '|---|---|---|---|---|---|---|']
    for K, n in SHAPES:
        torch.manual_seed(K)
        U = torch.randn(K, n, dtype=torch.float64, device=DEV) * 1e-2
        params = torch.zeros(n, device=DEV)
        v, m, b = variants(e, U, params)

        # old and new must agree at the timed size before any timing counts
        new_med = e.agg_orderstat(U, m, m + 1, False, 0.0, 0.0)[0]
        assert torch.equal(new_med, torch.median(U, 0).values)
        if K <= 64:
            assert torch.equal(new_med, e.agg_comed(U))
        assert torch.equal(e.agg_orderstat(U, b, K - b, False, 0.0, 0.0)[0],
                           torch_trmean(U, b))
        del new_med

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
            lines.append(f'| {K} | {n} | {what} | {name} | '
                         f'{statistics.median(t):.3f} | '
                         f'{min(t):.3f}..{max(t):.3f} | {it} |')
            print(lines[-1], flush=True)
        del U, params, v
        torch.cuda.empty_cache()
    table = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(table)
    print(table)


if __name__ == '__main__':
    main()
