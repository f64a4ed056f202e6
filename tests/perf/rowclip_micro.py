"""Microbenchmark of the row-norm and clip kernels (ops/csrc/rowclip.hip) at
the workload shapes (K sampled agents, n parameters): FMNIST K=10, CIFAR10
K=40, Fed-EMNIST at full participation K=3383.

Usage: python tests/perf/rowclip_micro.py [--rounds R] [--out FILE.md]

Per shape it times
  stage 1        : rownorm_partials alone, one read of U
  geomed_sqdist  : one Weiszfeld distance pass (ops/csrc/geomed.hip, K <= 512
                   only), the comparison: it reads U once too and does more
                   work per byte
  clip, none     : the whole rowclip_ under a bound no row reaches: stage 1,
                   stage 2, and a stage 3 whose blocks all return at once,
                   one read of U
  clip, all      : the whole rowclip_ with every row clipped, read + read +
                   write = three passes.  Median mode at multiplier 0.99 on
                   rows of (after the first call) equal norm: every call
                   clips every row by 0.99, so the matrix never settles under
                   the bound and never underflows within the run; checked
                   after the timing.
Method (that of geomed_micro.py): every variant is warmed up, one call is
timed to size a window of at least ~0.25 s of device work, then R rounds
visit the variants of a shape in ALTERNATING order, each window timed with
device events.  The table gives the median ms per call over the rounds and
the min..max spread, the bytes the variant has to move, and the time those
bytes cost at the HBM rates of MI355X_MICROARCH.md, 8.0 TB/s (spec peak) and
6.3 TB/s (achievable), as a fraction of the measured time.  A matrix below
the 256 MiB Infinity Cache (K = 10, K = 40) is re-read on chip from the
second call on, so its fraction can exceed 1: only the K = 3383 rows are
HBM-bound measurements."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..', '..'))
import torch  # noqa: E402

from rlr_amd.ops import ext  # noqa: E402

DEV = 'cuda:0'
SHAPES = [(10, 1199882), (40, 537610), (3383, 1199882)]
HBM_PEAK_BPS = 8.0e12
HBM_ACHIEVABLE_BPS = 6.3e12
SHRINK = 0.99


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
        sys.exit("rowclip_micro needs a GPU")
    e = ext()
    lines = ['| K | n | chunks | variant | ms/call median | min..max | '
             'calls/window | MB moved | of 8.0 TB/s | of 6.3 TB/s |',
             '|---|---|---|---|---|---|---|---|---|---|']
    for K, n in SHAPES:
        torch.manual_seed(K)
        U = torch.empty(K, n, dtype=torch.float64, device=DEV)
        for lo in range(0, K, 256):             # in slabs: no 2x peak memory
            U[lo:lo + 256].normal_().mul_(1e-2)
        V = U.clone()                           # the matrix 'clip, all' eats
        w = 1.0 + torch.rand(K, dtype=torch.float64, device=DEV)

        # the kernels must be right at the timed size before any timing
        # counts: against torch, at the relative bound of PARITY.md
        ref = torch.stack([U[k].norm() for k in range(min(K, 16))])
        got = e.row_norms(U)
        assert torch.allclose(got[:16], ref, rtol=(n + 4) * 2.0 ** -52, atol=0)
        assert torch.allclose(e.rownorm_partials(U).sum(0).sqrt(), got,
                              rtol=2.0 ** -50, atol=0)
        s, _, _ = e.rowclip_(U, 1e30, False)
        assert bool((s == 1.0).all())
        del ref, got, s

        one = K * n * 8
        v = [('stage 1 (rownorm_partials)', one,
              lambda: e.rownorm_partials(U)),
             ('clip, no row clipped', one,
              lambda: e.rowclip_(U, 1e30, False)),
             ('clip, every row clipped', 3 * one,
              lambda: e.rowclip_(V, SHRINK, True))]
        if K <= e.geomed_max_k():
            v.insert(1, ('geomed_sqdist (comparison)', one,
                         lambda: e.geomed_sqdist(U, w)))
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
        # 'every row clipped' was that to the end, and V is still a matrix
        s, norm, _ = e.rowclip_(V, SHRINK, True)
        assert bool((s < 1.0).all()) and float(norm.min()) > 1e-30
        for (name, nbytes, _), t, it in zip(v, times, iters):
            med = statistics.median(t)
            lines.append(
                f'| {K} | {n} | {e.rownorm_chunks(K, n)} | {name} | '
                f'{med:.3f} | {min(t):.3f}..{max(t):.3f} | {it} | '
                f'{nbytes / 1e6:.0f} | '
                f'{nbytes / HBM_PEAK_BPS * 1e3 / med:.2f} | '
                f'{nbytes / HBM_ACHIEVABLE_BPS * 1e3 / med:.2f} |')
            print(lines[-1], flush=True)
        del U, V, v, w, s, norm
        torch.cuda.empty_cache()
    table = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(table)
    print(table)


if __name__ == '__main__':
    main()
