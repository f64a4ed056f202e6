"""Microbenchmark of the fused Weiszfeld kernels (ops/csrc/geomed.hip) and
the geometric-median server step, at the workload shapes (K sampled agents,
n parameters): FMNIST K=10, CIFAR10 K=40, Fed-EMNIST --agent_frac 0.1 K=338.

Usage: python tests/perf/geomed_micro.py [--rounds R] [--out FILE.md]

Per shape it times
  step   : one geomed_sqdist (1 / s, stage 1, stage 2) | fused_avg_rlr_apply
           alone, which reads the same bytes once
  server : the whole geomed step at R = 8 (8 x (stage 1, stage 2), then the
           fused weighted average + RLR vote + apply) | the same loop
           composed in torch on the device, for scale
Method (that of krum_micro.py): every variant is warmed up, one call is
timed to size a window of at least ~0.25 s of device work, then R rounds
visit the variants of a shape in ALTERNATING order, each window timed with
device events.  The table gives the median ms per call over the rounds and
the min..max spread; kernel and composition are compared at the timed size
first.

Each row that streams U is read against the HBM floor of ONE pass,
K n 8 B / 8.0 TB/s (spec peak); the server step makes R + 1 = 9 passes."""

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
ITERS = 8
NU = 1e-6
HBM_BPS = 8.0e12


def window_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def torch_weights(U):
    """The Weiszfeld loop composed of torch ops on the device (matrix-vector
    products; not the sequential order of the rule)."""
    a = torch.ones(U.shape[0], dtype=torch.float64, device=U.device)
    for _ in range(ITERS):
        z = (a @ U) * (1.0 / a.sum())
        d2 = ((U - z) ** 2).sum(1)
        a = 1.0 / torch.sqrt(d2).clamp(min=NU)
    return a


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
        sys.exit("geomed_micro needs a GPU")
    e = ext()
    lines = ['| K | n | what | variant | ms/call median | min..max | '
             'calls/window | HBM floor ms (one pass) |',
             '|---|---|---|---|---|---|---|---|']
    for K, n in SHAPES:
        torch.manual_seed(K)
        U = torch.randn(K, n, dtype=torch.float64, device=DEV) * 1e-2
        gm = _Model(n)
        ids = list(range(K))
        theta = max(1, int(THETA_FRAC * K))
        sizes = {i: 10 * (i + 1) for i in ids}
        geomed = Aggregation(sizes, n, None, default_args(
            no_tb=True, device=DEV, aggr='geomed', geomed_iters=ITERS,
            geomed_nu=NU, robustLR_threshold=theta))
        w = 1.0 + torch.rand(K, dtype=torch.float64, device=DEV)

        # kernel and composition must agree at the timed size before any
        # timing counts
        a_k = e.geomed_weights(U, ITERS, NU)[0]
        a_t = torch_weights(U)
        assert torch.allclose(a_k, a_t, rtol=1e-9), \
            float(((a_k - a_t) / a_t).abs().max())
        z = (w @ U) * (1.0 / w.sum())
        d2 = ((U - z) ** 2).sum(1)
        assert torch.allclose(e.geomed_sqdist(U, w), d2, rtol=1e-10)
        del a_k, a_t, z, d2

        def torch_server():
            a_t = torch_weights(U)
            e.fused_avg_rlr_apply(U, a_t, gm.flat_params, True, float(theta),
                                  1.0, 0.0, 0, 0, False)

        hbm = K * n * 8 / HBM_BPS * 1e3
        v = [
            ('step', 'geomed_sqdist', lambda: e.geomed_sqdist(U, w)),
            ('step', 'fused_avg_rlr_apply alone',
             lambda: e.fused_avg_rlr_apply(U, w, gm.flat_params, True,
                                           float(theta), 1.0, 0.0, 0, 0,
                                           False)),
            ('server', f'geomed step, R = {ITERS}',
             lambda: geomed.aggregate_updates(gm, U, 1, ids)),
            ('server', f'torch loop + fused avg, R = {ITERS} (for scale)',
             torch_server),
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
            lines.append(f'| {K} | {n} | {what} | {name} | '
                         f'{statistics.median(t):.3f} | '
                         f'{min(t):.3f}..{max(t):.3f} | {it} | {hbm:.3f} |')
            print(lines[-1], flush=True)
        del U, gm, v, w
        torch.cuda.empty_cache()
    table = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(table)
    print(table)


if __name__ == '__main__':
    main()
