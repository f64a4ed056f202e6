"""Inputs and independent re-implementations shared by the Bulyan tests
(CPU and GPU).  A plain module like server_helpers; the seeds are part of
what those tests pin.  Nothing here calls the code under test."""

import functools

import torch

from server_helpers import N

# (K, f): theta = K - 2f - 2 selected, beta = K - 4f - 2 averaged.  Each
# crosses a boundary of the kernel (P = pow2 >= theta, L lanes per column):
SHAPES = [
    (3, 0),      # theta 1, beta 1: the smallest case
    (7, 1),      # theta 3, beta 1
    (10, 1),     # theta 6, beta 4: the headline K
    (18, 1),     # theta 14: just below P = 16
    (20, 1),     # theta 16: P = 16 exactly, the last L = 1 shape
    (21, 1),     # theta 17: the first P = 32 shape, L = 2
    (40, 4),     # theta 30, beta 22: the 40-agent configuration
    (67, 16),    # theta 33, beta 1
    (338, 33),   # theta 270, beta 204: P = 512
    (512, 127),  # theta 256, beta 2: P = 256 under the full K
]


def counts(K, f):
    return K - 2 * f - 2, K - 4 * f - 2


# CPU tensors, built once and never modified; tests move copies to the GPU

@functools.lru_cache(maxsize=None)
def ints(K, n=N):
    """Values in -3..3: almost every window step is a tie, so a wrong tie
    rule changes the value."""
    g = torch.Generator().manual_seed(11 * K + n)
    return torch.randint(-3, 4, (K, n), generator=g).double()


@functools.lru_cache(maxsize=None)
def graded(K, f, n=N):
    """Honest row k is base + sigma_k randn with sigma = 0.1 * 3^(k/K) in a
    random permutation; f random rows are -2 base + 0.3 randn.  The graded
    spreads make every Krum pick unambiguous.  Returns (U, sorted positions
    of the corrupted rows)."""
    g = torch.Generator().manual_seed(53 * K + f)
    base = torch.randn(n, dtype=torch.float64, generator=g)
    sigma = 0.1 * 3.0 ** (torch.arange(K, dtype=torch.float64) / K)
    sigma = sigma[torch.randperm(K, generator=g)]
    U = base + sigma.unsqueeze(1) * torch.randn(K, n, dtype=torch.float64,
                                                generator=g)
    bad = torch.randperm(K, generator=g)[:f].sort().values
    U[bad] = -2.0 * base + 0.3 * torch.randn(f, n, dtype=torch.float64,
                                             generator=g)
    return U, bad


def direct_sqdist(U):
    """D[i][j] = sum (U_i - U_j)^2, one triangle mirrored."""
    K = U.shape[0]
    D = torch.stack([((U - U[i]) ** 2).sum(1) for i in range(K)])
    D = torch.triu(D, diagonal=1)
    return D + D.T


def python_select(D, f):
    """Stage 1 written out in plain Python floats, agent by agent."""
    K = D.shape[0]
    d = D.tolist()
    alive = list(range(K))
    picks = []
    for t in range(K - 2 * f - 2):
        c = K - t - f - 2
        best, best_score = None, None
        for i in alive:
            near = sorted(d[i][j] for j in alive if j != i)
            acc = 0.0
            for x in near[:c]:
                acc += x
            score = acc * (1.0 / c)
            if best is None or score < best_score:   # ties: lowest position
                best, best_score = i, score
        picks.append(best)
        alive.remove(best)
    return sorted(picks)


def gather_select(D, f):
    """Stage 1 with the alive agents' mutual distances gathered explicitly
    (no +inf bookkeeping), vectorised over the agents so that K = 512 stays
    quick.  Returns (sorted picks, smallest gap between the lowest score
    and the next DISTINCT one over all iterations; mutual nearest
    neighbours tie exactly at c = 1, on any backend, because D is
    symmetric)."""
    K = D.shape[0]
    alive = torch.arange(K)
    picks, gap = [], float('inf')
    for t in range(K - 2 * f - 2):
        r = alive.numel()
        c = r - f - 2
        sub = D[alive][:, alive]
        off = sub[~torch.eye(r, dtype=torch.bool)].view(r, r - 1)
        near = torch.sort(off, dim=1).values.T.contiguous()
        acc = torch.zeros(r, dtype=torch.float64)
        for q in range(c):
            acc += near[q]
        scores = acc * (1.0 / c)
        order = torch.sort(scores, stable=True)
        above = order.values[order.values > order.values[0]]
        if above.numel():
            gap = min(gap, float(above[0] - order.values[0]))
        picks.append(int(alive[order.indices[0]]))
        alive = alive[alive != picks[-1]]
    return sorted(picks), gap


def brute_trim(rows, beta):
    """Stage 2 as a selection: per column the beta values of smallest
    |x - med|, a stable sort over the candidates taken outward from the
    median with the left side first; the chosen values are then added in
    ascending order and scaled."""
    theta, n = rows.shape
    s = torch.sort(rows, dim=0).values
    m = (theta - 1) // 2
    outward = torch.cat([torch.arange(m, -1, -1), torch.arange(m + 1, theta)])
    key = (s[outward] - s[m]).abs()
    first = torch.sort(key, dim=0, stable=True).indices[:beta]
    chosen = torch.sort(outward[first], dim=0).values      # (beta, n)
    vals = torch.gather(s, 0, chosen)
    out = torch.zeros(n, dtype=torch.float64)
    for i in range(beta):
        out += vals[i]
    return out * (1.0 / beta)


def selected_first(sel, K, generator=None):
    """int32 permutation of 0..K-1 with the rows sel first; with a
    generator both parts are shuffled."""
    mask = torch.ones(K, dtype=torch.bool)
    mask[sel] = False
    head, tail = sel.clone(), torch.arange(K)[mask]
    if generator is not None:
        head = head[torch.randperm(head.numel(), generator=generator)]
        tail = tail[torch.randperm(tail.numel(), generator=generator)]
    return torch.cat([head, tail]).to(torch.int32)
