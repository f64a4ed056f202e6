"""Scaffolding shared by the aggregation-server tests (CPU and GPU): the
server under test, its hand-built and seeded inputs, a recording writer and
the spawn-a-world runner.  A plain module, imported by its sibling test
files; the seeds are part of what those tests pin."""

import functools
import os

import torch
import torch.multiprocessing as mp

N = 4099   # prime and odd: rows are only 8-byte aligned, every tile has a tail


def make_agg(n, dev=None, *, aggr=None, table=1024, writer=None, **over):
    """The server over n parameters, agent i holding 10 (i + 1) samples for
    i < table; its args are its .args.  dev and aggr are left to the
    parser's defaults when None."""
    from rlr_amd.aggregation import Aggregation
    from rlr_amd.options import default_args
    if dev is not None:
        over['device'] = dev
    if aggr is not None:
        over['aggr'] = aggr
    args = default_args(no_tb=True, **over)
    sizes = {i: 10 * (i + 1) for i in range(table)}
    return Aggregation(sizes, n, None, args, writer=writer)


def t64(rows):
    return torch.tensor(rows, dtype=torch.float64)


class P(torch.nn.Module):
    """A model of one zero parameter vector."""

    def __init__(self, n):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(n))


class Writer:
    """Records add_scalar calls: .rows in call order, .last by name."""

    def __init__(self):
        self.rows = []
        self.last = {}

    def add_scalar(self, name, v, step):
        self.rows.append((name, v, step))
        self.last[name] = (v, step)


# CPU tensors, built once and never modified; tests move copies to the GPU

@functools.lru_cache(maxsize=None)
def randn(K, n=N, seed=0):
    g = torch.Generator().manual_seed(1000 * K + n + seed)
    return torch.randn(K, n, dtype=torch.float64, generator=g)


@functools.lru_cache(maxsize=None)
def clustered(K, f, n=N):
    """Honest rows base + 0.3 randn; f random rows -2 base + 0.3 randn.
    Returns (U, sorted positions of the corrupted rows)."""
    g = torch.Generator().manual_seed(31 * K + f)
    base = torch.randn(n, dtype=torch.float64, generator=g)
    U = base + 0.3 * torch.randn(K, n, dtype=torch.float64, generator=g)
    bad = torch.randperm(K, generator=g)[:f].sort().values
    U[bad] = -2.0 * base + 0.3 * torch.randn(f, n, dtype=torch.float64,
                                             generator=g)
    return U, bad


def _world_worker(rank, world_size, port, out_q, over):
    os.environ['RANK'] = str(rank)
    os.environ['WORLD_SIZE'] = str(world_size)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import rlr_amd.data.datasets as D
    D.DEFAULT_SIZES['fmnist'] = (2000, 400)
    from rlr_amd.federated import run
    from rlr_amd.options import default_args
    from rlr_amd.parallel import dist as pdist
    args = default_args(num_agents=4, rounds=2, snap=2, local_ep=1, bs=64,
                        synthetic=True, no_tb=True, data='fmnist',
                        num_corrupt=1, poison_frac=0.5, robustLR_threshold=3,
                        device='cpu', **over)
    try:
        h = run(args)
        if rank == 0:
            out_q.put(h['final_params'].numpy().copy())
    finally:
        pdist.teardown()


def run_world(world_size, base_port, **over):
    """Final parameters of a two-round CPU run on world_size spawned ranks
    that rendezvous on base_port + world_size."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = base_port + world_size
    procs = [ctx.Process(target=_world_worker,
                         args=(r, world_size, port, q, over))
             for r in range(world_size)]
    for p in procs:
        p.start()
    params = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return torch.from_numpy(params)
