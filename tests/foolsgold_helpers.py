"""Inputs shared by the FoolsGold tests (CPU and GPU) and the checks of their
own preconditions on the CPU rule.  A plain module, imported by its sibling
test files; the seeds are part of what those tests pin."""

import functools
import math

import torch

import server_helpers

N = server_helpers.N

make_agg = functools.partial(server_helpers.make_agg, aggr='foolsgold')


# CPU tensors, built once and never modified; tests move copies to the GPU

@functools.lru_cache(maxsize=None)
def sybils(K, f, n=N):
    """Independent randn rows; f random positions hold d + 0.1 randn for one
    shared d.  Returns (U, sorted positions of the sybils)."""
    g = torch.Generator().manual_seed(53 * K + f)
    U = torch.randn(K, n, dtype=torch.float64, generator=g)
    d = torch.randn(n, dtype=torch.float64, generator=g)
    bad = torch.randperm(K, generator=g)[:f].sort().values
    U[bad] = d + 0.1 * torch.randn(f, n, dtype=torch.float64, generator=g)
    return U, bad


@functools.lru_cache(maxsize=None)
def graded(K, n=N):
    """Row k is t_k d + (1 - t_k) r_k: t = 0 for half the rows and
    linspace(0.3, 0.8, K // 2) for the rest, shuffled — alphas at 0, at 1
    and strictly between."""
    g = torch.Generator().manual_seed(97 * K + 3)
    d = torch.randn(n, dtype=torch.float64, generator=g)
    r = torch.randn(K, n, dtype=torch.float64, generator=g)
    t = torch.zeros(K, dtype=torch.float64)
    t[K - K // 2:] = torch.linspace(0.3, 0.8, K // 2, dtype=torch.float64)
    t = t[torch.randperm(K, generator=g)].unsqueeze(1)
    return t * d + (1.0 - t) * r


@functools.lru_cache(maxsize=None)
def ints(K, n=N):
    """Integers in [-3, 3]: every sum of products is exact in any order."""
    g = torch.Generator().manual_seed(7 * K + n)
    return torch.randint(-3, 4, (K, n), generator=g).double()


def cpu_gram(Hs):
    """The CPU rule's Gram matrix: a row loop, the upper triangle mirrored."""
    K = Hs.shape[0]
    G = torch.empty(K, K, dtype=torch.float64)
    for i in range(K):
        G[i] = (Hs * Hs[i]).sum(1)
    up = torch.triu(G, diagonal=1)
    return up + up.T + torch.diag(G.diagonal())


def steps_3_to_6(cs):
    """(wv after step 6, m, wv / m before the == 1.0 replacement) from the
    cosine matrix of step 2, vectorised as the CPU rule does it."""
    v = cs.max(dim=1).values
    vi, vj = v.unsqueeze(1), v.unsqueeze(0)
    pard = torch.where(vi < vj, (cs * vi) / vj, cs)
    wv = (1.0 - pard.max(dim=1).values).clamp(0.0, 1.0)
    m = wv.max()
    scaled = wv / m if m > 0 else wv
    return torch.where(scaled == 1.0, torch.full_like(scaled, 0.99),
                       scaled), m, scaled


def weights_from_cosines(cs, kappa):
    """Steps 3-7 of the CPU rule on a given cs: (alpha, wv, L) with wv after
    step 6 and L = ln(wv / (1 - wv))."""
    wv, _, _ = steps_3_to_6(cs)
    L = torch.log(wv / (1.0 - wv))
    return (kappa * (L + 0.5)).clamp(0.0, 1.0), wv, L


def assert_graded_preconditions(cs, kappa):
    """graded()'s promise: alphas at 0, at 1 and strictly between, and no
    wv / m in (1 - 1e-9, 1), so the == 1.0 branch cannot differ between
    backends."""
    alpha, _, _ = weights_from_cosines(cs, kappa)
    _, _, scaled = steps_3_to_6(cs)
    assert not ((scaled > 1.0 - 1e-9) & (scaled < 1.0)).any()
    assert (alpha == 0).any() and (alpha == 1).any()
    assert ((alpha > 0) & (alpha < 1)).any()


def assert_sybils_decisive(cs, kappa, bad):
    """sybils()'s promise: every unclamped kappa (L + 0.5) lies at least 0.1
    outside (0, 1), the honest rows above and the sybils below."""
    _, _, L = weights_from_cosines(cs, kappa)
    raw = kappa * (L + 0.5)
    is_bad = torch.zeros(cs.shape[0], dtype=torch.bool)
    is_bad[bad] = True
    assert (raw[is_bad] <= -0.1).all()
    assert (raw[~is_bad] >= 1.1).all()
    assert math.isfinite(float(raw[~is_bad].max()))
