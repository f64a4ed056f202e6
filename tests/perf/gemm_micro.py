"""Microbenchmark of the short-K form of the fp32 tile GEMM
(gemm_f32_shortk_k, ops/csrc/gemm_f32.hip) against the kernel it replaces at
the three fc1 products of CNN_MNIST, Linear(9216, 128), at batch 256 (the
benchmark's) and batch 112 (3-tile chunks in the forward).

Usage: python tests/perf/gemm_micro.py [--rounds R] [--out FILE.md]

Per shape it times the whole call of the entry point the model uses
  fwd : linear_fwd(x, w)            layout B^T, split-K + two-level fold
  dx  : gemm(dy, w)                 layout NN, SK = 1 at batch 256
  dw  : linear_bwd_into(.., dw)     layout A^T, split-K + one-level fold
once with RLR_AMD_NO_GEMM_SHORTK=1 (gemm_f32_k, "old") and once without
("new").  The launcher reads the switch on every call, so both run in one
process on the same buffers.  The split-K fold and the output allocation are
in both timings and are the same code; the difference is the main kernel's.

Method (that of rowclip_micro.py): both variants are warmed up, one call is
timed to size a window of ~0.1 s of device work, then R rounds visit old and
new in ALTERNATING order, each window timed with device events.  The table
gives the median us per call over the rounds and the min..max spread, beside
two floors of the main kernel alone: the unique bytes it has to move (A, B
and the SK slabs or C) at 8.0 TB/s, and its 2 M N K flops at the 157 TF fp32
MFMA rate (MI355X_MICROARCH.md).  Before any timing the two variants' results
are compared bit for bit."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..', '..'))
import torch  # noqa: E402

from rlr_amd.ops import ext  # noqa: E402

DEV = 'cuda:0'
SWITCH = 'RLR_AMD_NO_GEMM_SHORTK'
IN, OUT = 9216, 128
BATCHES = [256, 112]
HBM_PEAK_BPS = 8.0e12
MFMA_F32_FLOPS = 157e12


def window_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def with_switch(on, fn):
    def f():
        if on:
            os.environ[SWITCH] = '1'
        else:
            os.environ.pop(SWITCH, None)
        return fn()
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gemm_micro needs a GPU")
    e = ext()
    lines = ['| batch | call | M, N, K | SK | tiles | old us median | min..max '
             '| new us median | min..max | new / old | HBM floor us | '
             'MFMA floor us |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for B in BATCHES:
        torch.manual_seed(B)
        x = torch.randn(B, IN, device=DEV)
        w = torch.randn(OUT, IN, device=DEV) * 0.05
        dy = torch.randn(B, OUT, device=DEV)
        dw = torch.empty_like(w)
        calls = [
            ('fwd', (B, OUT, IN, IN, IN), lambda: e.linear_fwd(x, w, None,
                                                               False)),
            ('dx', (B, IN, OUT, OUT, IN), lambda: e.gemm(dy, w, None, False)),
            ('dw', (OUT, IN, B, OUT, IN),
             lambda: (e.linear_bwd_into(x, w, dy, dw, None, False), dw)[1]),
        ]
        for name, (m, n, k, lda, ldb), fn in calls:
            sk = e.gemm_f32_splitk(m, n, k)
            tiles = e.gemm_f32_shortk_tiles(m, n, k, sk, lda, ldb)
            old, new = with_switch(True, fn), with_switch(False, fn)
            r_old = old().clone()
            r_new = new().clone()
            assert torch.equal(r_old.view(torch.int32),
                               r_new.view(torch.int32)), (B, name)
            v = [old, new]
            iters = []
            for f in v:
                f()
                f()
                torch.cuda.synchronize()
                t1 = window_ms(f, 20)
                iters.append(max(20, min(5000, int(100.0 / max(t1, 1e-3)))))
            times = [[], []]
            for r in range(a.rounds):
                for i in ((0, 1) if r % 2 == 0 else (1, 0)):
                    times[i].append(window_ms(v[i], iters[i]) * 1e3)
            os.environ.pop(SWITCH, None)
            mo, mn = (statistics.median(t) for t in times)
            nbytes = 4 * (m * k + k * n + sk * m * n)
            lines.append(
                f'| {B} | {name} | {m}, {n}, {k} | {sk} | {tiles} | '
                f'{mo:.2f} | {min(times[0]):.2f}..{max(times[0]):.2f} | '
                f'{mn:.2f} | {min(times[1]):.2f}..{max(times[1]):.2f} | '
                f'{mn / mo:.3f} | {nbytes / HBM_PEAK_BPS * 1e6:.2f} | '
                f'{2.0 * m * n * k / MFMA_F32_FLOPS * 1e6:.2f} |')
            print(lines[-1], flush=True)
    table = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(table)
    print(table)


if __name__ == '__main__':
    main()
