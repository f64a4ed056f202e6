"""Step batching (ops/csrc/step_batch.hip, step_roles.h): the small fold /
permute / copy kernels of a training step as roles of one launch.

  1. the launch plan (host arithmetic, no GPU);
  2. every role against the stand-alone launcher it shares its body with,
     batched behind other roles so that it never starts at block 0;
  3. the CNN tapes with the queue, the weight prep and the feed against
     the same tapes with RLR_AMD_NO_STEP_BATCH=1;
  4. the dropout offset after engine steps and after eager steps.

Every comparison is on raw bits (signed zeros included)."""

import pytest
import torch

DEV = 'cuda:0'
gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def E():
    from rlr_amd.ops import ext
    return ext()


def bits_equal(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype == torch.float32:
        a = a.reshape(-1).contiguous().view(torch.int32)
        b = b.reshape(-1).contiguous().view(torch.int32)
    return torch.equal(a, b)


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    # a few exact and signed zeros, so the bit comparison sees them
    x.view(-1)[::7] = 0.0
    x.view(-1)[3::11] = -0.0
    return x.to(DEV)


# ------------------------------------------------------------------ 1. plan

def _check_plan(E, counts):
    first, total = E.step_batch_plan(counts)
    assert total == sum(counts)
    # the ranges tile [0, total): each starts where the one before ended
    end = 0
    for f, c in zip(first, counts):
        assert f == end
        end += c
    assert end == total
    for r, (f, c) in enumerate(zip(first, counts)):
        if c == 0:
            continue
        assert E.step_batch_lookup(counts, f) == (r, 0)
        assert E.step_batch_lookup(counts, f + c - 1) == (r, c - 1)
    # a role with zero blocks owns no block at all
    owners = {E.step_batch_lookup(counts, b)[0] for b in range(total)}
    assert owners == {r for r, c in enumerate(counts) if c > 0}
    assert E.step_batch_lookup(counts, total)[0] == -1
    assert E.step_batch_lookup(counts, -1)[0] == -1


def test_plan_one_role(E):
    _check_plan(E, [1])
    _check_plan(E, [37])


def test_plan_max_roles(E):
    n = E.step_batch_max_roles()
    assert n >= 16
    _check_plan(E, [(3 * r) % 7 + 1 for r in range(n)])
    _check_plan(E, [2048] * n)


def test_plan_zero_block_roles(E):
    n = E.step_batch_max_roles()
    _check_plan(E, [0, 5, 0, 0, 1, 0])
    _check_plan(E, [4, 0, 9])
    _check_plan(E, [0] * n)
    _check_plan(E, [0] * (n - 1) + [3])


def test_prof_summary_names_every_role_kind():
    """scripts/prof_summary.py prints step_role_k<KIND> by the kind's name:
    its list follows StepRoleKind (launchers.h), entry for entry."""
    import importlib.util
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'rlr_amd', 'ops', 'csrc',
                           'launchers.h')) as f:
        body = re.search(r'enum StepRoleKind \{(.*?)\};', f.read(),
                         re.S).group(1)
    kinds = re.findall(r'kRole(\w+)', body)
    snake = [re.sub(r'(?<!^)(?=[A-Z])', '_', k).lower() for k in kinds]
    spec = importlib.util.spec_from_file_location(
        'prof_summary', os.path.join(root, 'scripts', 'prof_summary.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert len(snake) == 12 and mod.ROLE_KINDS == snake
    assert (mod.readable('void step_role_k<6>(StepRole)')
            == 'step_role_k<colsum>')
    assert mod.readable('step_batch_k(StepTable)') == 'step_batch_k(StepTable)'


# ----------------------------------------------------------------- 2. roles

def filled_queue(E):
    """A queue that already holds two roles on each level, so the role
    under test starts past block 0 of both launches."""
    q = E.StepQueue()
    sink = []
    for s in (101, 102):
        dy = rnd(2, 8, 3, 3, seed=s).contiguous(
            memory_format=torch.channels_last)
        db = torch.empty(8, device=DEV)
        q.conv_db(dy, db)
        sink.append((dy, db))
    assert q.pending() == (2, 2)
    return q, sink


def check_fillers(E, sink):
    for dy, db in sink:
        assert bits_equal(db, E.conv_db(dy))


@gpu
@pytest.mark.parametrize('Nb,OHW,Kout', [
    (2, 25, 32),     # 64 chunks, most of them empty
    (3, 49, 48),     # 256 % Kout != 0: K_blk = 256
    (2, 36, 300),    # two y-blocks
    (5, 100, 64),    # ragged last chunk
])
def test_role_conv_db(E, Nb, OHW, Kout):
    dy = rnd(Nb, Kout, OHW, 1, seed=Nb).contiguous(
        memory_format=torch.channels_last)
    ref = E.conv_db(dy)
    q, sink = filled_queue(E)
    db = torch.full((Kout,), float('nan'), device=DEV)
    q.conv_db(dy, db)
    assert q.pending() == (3, 3)
    q.flush()
    assert q.pending() == (0, 0)
    assert bits_equal(db, ref)
    check_fillers(E, sink)


@gpu
@pytest.mark.parametrize('SK,levels', [(17, 2), (48, 2), (5, 1)])
def test_role_splitk_reduce_dwperm(E, SK, levels):
    Kout, C, RS = 64, 32, 9
    ws = rnd(E.conv_dwperm_ws_floats(Kout, C * RS, SK), seed=SK)
    ref = E.splitk_reduce_dwperm(ws.clone(), Kout, C, RS, SK)
    q, sink = filled_queue(E)
    dw = torch.full((Kout * C * RS,), float('nan'), device=DEV)
    q.splitk_reduce_dwperm(ws, dw, Kout, C, RS, SK)
    # SK > 16: splitk_partial on level 1, splitk_reduce_dwperm on level 2
    assert q.pending() == (3, 2 + (levels == 2))
    q.flush()
    assert bits_equal(dw, ref)
    check_fillers(E, sink)


@gpu
@pytest.mark.parametrize('SK', [2, 7])
def test_role_splitk_reduce(E, SK):
    M, N = 37, 300          # > 8192 outputs: the thread form
    ws = rnd(E.gemm_splitk_ws_floats(M, N, SK), seed=SK)
    ref = E.splitk_reduce(ws, M, N, SK)
    q, sink = filled_queue(E)
    out = torch.full((M, N), float('nan'), device=DEV)
    assert q.splitk_reduce(ws, out, None, M, N, N, SK, False)
    assert q.pending() == (3, 2)
    q.flush()
    assert bits_equal(out, ref)
    check_fillers(E, sink)


@gpu
def test_role_splitk_reduce_wave_form_has_no_role(E):
    M, N, SK = 8, 36, 16    # <= 8192 outputs and SK >= 16: wave form
    ws = rnd(E.gemm_splitk_ws_floats(M, N, SK))
    q = E.StepQueue()
    out = torch.empty(M, N, device=DEV)
    assert not q.splitk_reduce(ws, out, None, M, N, N, SK, False)
    assert q.pending() == (0, 0)


@gpu
@pytest.mark.parametrize('Nb,OH,OW,chunks', [(8, 32, 32, 64),
                                             (10, 28, 32, 70)])
def test_role_conv_small_bwdw_reduce(E, Nb, OH, OW, chunks):
    C, Kout, R, S = 1, 32, 3, 3
    assert max(64, -(-(Nb * OH * OW) // 128)) == chunks
    ws = rnd(E.conv_bwd_weight_ws_floats(Kout, C * R * S, 1), seed=chunks)
    ref = E.conv_small_bwdw_reduce(ws, Nb, C, Kout, R, S, OH, OW)
    q, sink = filled_queue(E)
    dw = torch.full((Kout * C * R * S,), float('nan'), device=DEV)
    q.conv_small_bwdw_reduce(ws, dw, Nb, C, Kout, R, S, OH, OW)
    assert q.pending() == (3, 2)
    q.flush()
    assert bits_equal(dw, ref)
    check_fillers(E, sink)


@gpu
@pytest.mark.parametrize('M', [5, 130])
def test_role_colsum(E, M):
    dy = rnd(M, 37, seed=M)
    ref = E.colsum(dy)
    q, sink = filled_queue(E)
    db = torch.full((37,), float('nan'), device=DEV)
    q.colsum(dy, db)
    q.flush()
    assert bits_equal(db, ref)
    check_fillers(E, sink)


@gpu
@pytest.mark.parametrize('Kout,C', [(32, 1), (64, 32)])
def test_role_weight_permutes(E, Kout, C):
    w = rnd(Kout, C, 3, 3, seed=Kout)
    q, sink = filled_queue(E)
    wt = q.wperm(w, 0)
    wp = q.wperm(w, 1)
    assert q.pending() == (4, 2)
    q.flush()
    assert bits_equal(wt, E.wperm(w, 0))
    assert bits_equal(wp, E.wperm(w, 1))
    check_fillers(E, sink)
    # the one-launch helper the tapes call
    wt2, wp2 = E.prep_conv_weights([(w, 0), (w, 1)])
    assert bits_equal(wt2, wt) and bits_equal(wp2, wp)
    # and the permutes against their definition
    assert bits_equal(wt, w.permute(2, 3, 1, 0).reshape(9 * C, Kout))
    assert bits_equal(wp, w.permute(2, 3, 0, 1).reshape(9 * Kout, C))


@gpu
def test_role_gather(E):
    X = rnd(50, 1, 28, 28, seed=5)
    Y = torch.randint(-2 ** 40, 2 ** 40, (50,),
                      generator=torch.Generator().manual_seed(6)).to(DEV)
    g = torch.Generator().manual_seed(7)
    sel = torch.randint(0, 50, (37,), generator=g)
    sel[5] = sel[4]                     # repeated
    sel[0], sel[1] = 49, 0              # out of order, both ends
    sel = sel.to(DEV)
    q, sink = filled_queue(E)
    ox = torch.full((37, 1, 28, 28), float('nan'), device=DEV)
    oy = torch.zeros(37, dtype=torch.long, device=DEV)
    q.gather_rows(X, sel, ox)
    q.gather_rows(Y, sel, oy)
    assert q.pending() == (4, 2)
    q.flush()
    assert bits_equal(ox, X.index_select(0, sel))
    assert bits_equal(oy, Y.index_select(0, sel))
    check_fillers(E, sink)
    # rows that are no multiple of four words take the scalar form
    X3 = rnd(50, 3, 5, 5, seed=8)
    o3 = torch.empty(37, 3, 5, 5, device=DEV)
    ox.fill_(float('nan'))
    oy.zero_()
    E.feed_gather(X, Y, sel, ox, oy)
    q.gather_rows(X3, sel, o3)
    q.flush()
    assert bits_equal(ox, X.index_select(0, sel))
    assert bits_equal(oy, Y.index_select(0, sel))
    assert bits_equal(o3, X3.index_select(0, sel))


@gpu
@pytest.mark.parametrize('B,H,C', [(37, 128, 10),   # wave-form dW, B >= 32
                                   (5, 24, 10)])    # thread-form dW
def test_role_fc_head_reduce(E, B, H, C):
    """fc_head_step with the queue (stage B as a role behind two others)
    against fc_head_step without it (the same role, run alone)."""
    assert E.fc_head_fused_ok(B, H, C)
    h1 = rnd(B, H, seed=B).relu()
    w, b = rnd(C, H, seed=1), rnd(C, seed=2)
    labels = torch.randint(0, C, (B,),
                           generator=torch.Generator().manual_seed(3)).to(DEV)
    dloss = torch.ones(1, device=DEV)
    state = torch.tensor([11, 32], dtype=torch.int64, device=DEV)

    def run(q):
        dw = torch.full((C, H), float('nan'), device=DEV)
        db = torch.full((C,), float('nan'), device=DEV)
        loss, g = E.fc_head_step(h1, w, b, labels, dloss, 0.5, state, 1, dw,
                                 db, q)
        return loss, g, dw, db

    ref = run(None)
    q, sink = filled_queue(E)
    got = run(q)
    assert q.pending() == (3, 2)
    q.flush()
    for a, r in zip(got, ref):
        assert bits_equal(a, r)
    check_fillers(E, sink)


@gpu
def test_role_add_u64(E):
    state = torch.tensor([2 ** 40 + 5, 2 ** 33 - 3, 9], dtype=torch.int64,
                         device=DEV)
    q, sink = filled_queue(E)
    q.add_u64(state, 1, 16)          # level 2, behind the two fillers
    assert q.pending() == (2, 3)
    q.flush()
    assert state.tolist() == [2 ** 40 + 5, 2 ** 33 + 13, 9]
    check_fillers(E, sink)


@gpu
def test_gather_out_of_range_index_is_not_read(E):
    """The documented precondition of the feed: an index outside the rows
    of src is never dereferenced; its row comes out as all-one bits."""
    X = rnd(6, 1, 4, 4, seed=1)
    Y = torch.arange(6, device=DEV)
    sel = torch.tensor([5, 6, -1, 0], device=DEV)
    ox = torch.zeros(4, 1, 4, 4, device=DEV)
    oy = torch.zeros(4, dtype=torch.long, device=DEV)
    E.feed_gather(X, Y, sel, ox, oy)
    assert bits_equal(ox[0], X[5]) and bits_equal(ox[3], X[0])
    assert oy.tolist() == [5, -1, -1, 0]
    assert (ox[1:3].contiguous().view(torch.int32) == -1).all()


# ------------------------------------------------------------------ 3. tape

def _tape_run(model_cls, data_shape, bs, steps=3):
    from rlr_amd.flatmodel import FlatParamModel
    from rlr_amd.ops import flat as flat_ops

    torch.manual_seed(7)
    gm = FlatParamModel(model_cls(), DEV)
    gm.train()
    gm.set_dropout_seed(99)
    gm.ensure_grad_views()
    g = torch.Generator().manual_seed(3)
    X = torch.randn(steps, bs, *data_shape, generator=g).to(DEV)
    Y = torch.randint(0, 10, (steps, bs), generator=g).to(DEV)
    out = []
    for i in range(steps):
        loss = gm.model.manual_step(X[i], Y[i], gm.dloss_ones())
        grads = gm.flat_grads.clone()
        flat_ops.clipped_sgd_step_(gm.flat_params, gm.flat_grads,
                                   gm.momentum, 0.1, 0.9, 10.0)
        gm.model.rng.advance_step()
        out.append((loss.clone(), grads, gm.flat_params.clone()))
    torch.cuda.synchronize()
    return out, gm.model.rng.gpu_state(DEV).clone()


@gpu
@pytest.mark.parametrize('bs', [64, 37])
@pytest.mark.parametrize('which', ['mnist', 'cifar'])
def test_tape_with_queue_matches_tape_without(monkeypatch, which, bs):
    from rlr_amd.models import CNN_CIFAR, CNN_MNIST
    cls, shape = ((CNN_MNIST, (1, 28, 28)) if which == 'mnist'
                  else (CNN_CIFAR, (3, 32, 32)))
    monkeypatch.delenv('RLR_AMD_NO_STEP_BATCH', raising=False)
    batched, st_b = _tape_run(cls, shape, bs)
    monkeypatch.setenv('RLR_AMD_NO_STEP_BATCH', '1')
    plain, st_p = _tape_run(cls, shape, bs)
    for (lb, gb, pb), (lp, gp, pp) in zip(batched, plain):
        assert bits_equal(lb, lp)
        assert bits_equal(gb, gp)
        assert bits_equal(pb, pp)
    assert torch.equal(st_b, st_p)


# -------------------------------------------------------- 4. dropout offset

def _engine_run(n, bs=64, count=None):
    from rlr_amd.flatmodel import FlatParamModel
    from rlr_amd.models import CNN_MNIST
    from rlr_amd.options import default_args
    torch.manual_seed(0)
    gm = FlatParamModel(CNN_MNIST(), DEV)
    gm.train()
    gm.set_dropout_seed(7)
    args = default_args(num_agents=2, rounds=2, snap=2, local_ep=1, bs=bs,
                        synthetic=True, no_tb=True, data='fmnist', device=DEV)
    eng = gm.get_engine(args)
    g = torch.Generator().manual_seed(1)
    # NHWC storage, as the datasets hand it to the engine
    X = torch.empty(200, 1, 28, 28, device=DEV,
                    memory_format=torch.channels_last)
    X.copy_(torch.randn(200, 1, 28, 28, generator=g))
    Y = torch.randint(0, 10, (200,), generator=g).to(DEV)
    eng.begin_round(gm.flat_params.clone())
    if count is not None:
        import rlr_amd.engine as engine_mod
        real = engine_mod.ext()

        class Counting:
            def __getattr__(self, name):
                return getattr(real, name)

            def feed_gather(self, *a):
                count.append(1)
                return real.feed_gather(*a)
        engine_mod.ext = lambda: Counting()
    for i in range(n):
        sel = torch.randperm(200, generator=g)[:bs].to(DEV)
        eng.step(X, Y, sel)
        assert gm.model.rng.site == 0
    torch.cuda.synchronize()
    return gm.model.rng.gpu_state(DEV).clone(), gm.flat_params.clone()


@gpu
def test_dropout_offset_engine_and_eager(monkeypatch):
    n = 3
    monkeypatch.delenv('RLR_AMD_NO_STEP_BATCH', raising=False)
    feeds = []
    import rlr_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, 'ext', engine_mod.ext)  # restored after
    st, params = _engine_run(n, count=feeds)
    assert st.tolist() == [7, 16 * n]
    assert len(feeds) == n      # every step fed by the one batched launch
    # the engine without the feed launch and the in-graph bump: same state,
    # same parameters
    monkeypatch.setenv('RLR_AMD_NO_STEP_BATCH', '1')
    st_plain, params_plain = _engine_run(n)
    assert st_plain.tolist() == [7, 16 * n]
    assert bits_equal(params, params_plain)
    # eager manual_step + advance_step: exactly one advance per step, with
    # and without the queue
    from rlr_amd.models import CNN_MNIST
    for env in ('0', '1'):
        monkeypatch.setenv('RLR_AMD_NO_STEP_BATCH', env)
        _, st_eager = _tape_run(CNN_MNIST, (1, 28, 28), 64, steps=n)
        assert st_eager.tolist() == [99, 16 * n]
