"""hipGraph-captured training step.

One FL step of the tiny reference CNNs is ~35-40 short kernels; eagerly
launched that is host-launch-bound (~3.5 us per launch — MI355X_MICROARCH
'graph-replay-floor').  The TrainEngine captures the whole step — the
model's hand-rolled manual tape (fwd + fused backward with grads written
straight into the flat views; models/*.manual_step) or the autograd
fallback, then the fused clip+SGD and optional PGD projection — into one
hipGraph per batch size and replays it (~10-16 us host cost).  Per step
only one launch runs outside the graph: the feed, which gathers X[sel] and
Y[sel] into the static input buffers (ops/csrc/step_batch.hip).  The
dropout-state advance is the last role of the captured step (the philox
seed/offset pair lives in DEVICE memory precisely so replays draw fresh
masks — ops/functional.DropoutCtx).  The fp32 CNN_MNIST step is 19 launches:
18 in the graph (weight prep, 2 conv fwd, the second one pooling in its
epilogue, seam fwd from the pooled image, fc1 GEMM + partial +
reduce, head rows, 2 fc1 bwd GEMMs, seam bwd, bwd-data, 2 bwd-weight
partial kernels, the 2 batched fold levels, 2 optimizer kernels) and the
feed (1 + 2 + 1 + 3 + 1 + 2 + 1 + 1 + 2 + 2 + 2 = 18).  With
RLR_AMD_NO_STEP_BATCH=1, and for models whose tape does not batch (the
autograd fallback, bf16, ResNet), the static input stays contiguous, the
feed is two index_selects and the advance a host-issued add, as before.

The captured kernel stream is identical to the eager GPU path, so results
are bitwise equal with graphs on or off (asserted in test_e2e_gpu), and
the manual tape is bitwise-equal to autograd (test_manual_tape_gpu)."""

import torch

from .ops import ext, step_batching
from .ops import flat as flat_ops
from .ops import functional as Fo


def _rows_alike(src, dst):
    """Whether row i of src and row j of dst are the same dense run of
    storage elements (dims of size 1 carry no layout), so the feed launch
    can copy whole rows."""
    if src.shape[1:] != dst.shape[1:] or src.dtype != dst.dtype:
        return False
    row = src[0].numel() if src.shape[0] else 0
    for t in (src, dst):
        if t.shape[0] > 1 and t.stride(0) != row:
            return False
    return all(a == b for n, a, b in zip(src.shape[1:], src.stride()[1:],
                                         dst.stride()[1:]) if n > 1)


class TrainEngine:
    def __init__(self, gm, args):
        self.gm = gm
        self.args = args
        self.graphs = {}
        self.theta0_static = (torch.zeros_like(gm.flat_params)
                              if args.clip > 0 else None)
        self.pool = None

    # ------------------------------------------------------------ round

    def begin_round(self, theta0):
        if self.theta0_static is not None:
            self.theta0_static.copy_(theta0)

    # ------------------------------------------------------------- step

    def _batched(self):
        """Whether this engine's step is the batched fp32 manual tape: only
        then does it feed with one launch, keep an NHWC dataset's layout in
        the static input and leave the dropout-offset bump to the tape.
        Never with RLR_AMD_NO_STEP_BATCH=1, the autograd fallback or bf16."""
        model = self.gm.model
        return (step_batching()
                and getattr(model, 'manual_step', None) is not None
                and getattr(model, 'tape_bumps_offset', False)
                and model.compute_dtype is None)

    def _step_body(self, static_x, static_y):
        # Preferred path: the model's hand-rolled fwd+bwd (manual_step)
        # writes each weight/bias grad DIRECTLY into its flat_grads view —
        # no zero-grad fill and no autograd accumulate-add kernels, with a
        # bitwise-identical kernel stream otherwise (assignment ==
        # accumulate-into-zero).  The autograd fallback below remains for
        # models without a manual tape (bf16 ResNet).
        # Returns whether the body advanced the dropout offset itself.
        gm, args = self.gm, self.args
        model = gm.model
        bumped = False
        if (getattr(model, 'manual_step', None) is not None
                and (model.compute_dtype is None
                     or getattr(model, 'manual_bf16_ok', False))):
            if self._batched():
                model.manual_step(static_x, static_y, gm.dloss_ones(),
                                  bump_offset=True)
                bumped = True
            else:
                model.manual_step(static_x, static_y, gm.dloss_ones())
        else:
            gm.flat_grads.zero_()
            out = gm(static_x)
            loss = Fo.cross_entropy(out, static_y)
            loss.backward()
        flat_ops.clipped_sgd_step_(gm.flat_params, gm.flat_grads,
                                   gm.momentum, args.client_lr,
                                   args.client_moment, 10.0)
        if args.clip > 0:
            flat_ops.pgd_project_(gm.flat_params, self.theta0_static,
                                  args.clip)
        return bumped

    def _build(self, bs, X):
        gm = self.gm
        x_shape, device = X.shape[1:], X.device
        # graph capture must not race other streams' submissions (several
        # replicas train concurrently on their own streams): drain the
        # device first; capture itself is thread_local-error-mode
        torch.cuda.synchronize(device)
        static_x = torch.zeros((bs,) + tuple(x_shape), device=device)
        if (self._batched() and X.dim() == 4 and not X.is_contiguous()
                and X.is_contiguous(memory_format=torch.channels_last)):
            # keep the dataset's NHWC storage: the feed copies whole rows,
            # and the conv bindings want channels_last anyway
            static_x = static_x.contiguous(
                memory_format=torch.channels_last)
        static_y = torch.zeros(bs, dtype=torch.long, device=device)

        # warmup + capture corrupt params/momentum/dropout state; snapshot
        # and restore so graph building is invisible to training
        snap_p = gm.flat_params.clone()
        snap_m = gm.momentum.clone()
        snap_b = gm.flat_buffers.clone() if gm.n_buffers else None
        rng = gm.model.rng
        snap_state = rng.gpu_state(device).clone()
        snap_site = rng.site

        gm.ensure_grad_views()
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for _ in range(2):
                self._step_body(static_x, static_y)
                rng.site = snap_site
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)

        g = torch.cuda.CUDAGraph()
        # a GC cycle during capture frees pre-capture tensors -> hipFree
        # inside an active capture -> abort; collect first, then hold GC off
        import gc
        gc.collect()
        gc.disable()
        try:
            with torch.cuda.graph(g, pool=self.pool,
                                  capture_error_mode="thread_local"):
                bumped = self._step_body(static_x, static_y)
        finally:
            gc.enable()
        if self.pool is None:
            self.pool = g.pool()
        rng.site = snap_site

        gm.flat_params.copy_(snap_p)
        gm.momentum.copy_(snap_m)
        if snap_b is not None:
            gm.flat_buffers.copy_(snap_b)
        rng.gpu_state(device).copy_(snap_state)
        torch.cuda.synchronize(device)

        # one feed launch when the rows of X and static_x are laid out
        # alike (fp32 images, int64 labels); index_select otherwise
        feed = (X.stride() if self._batched() and X.is_cuda
                and X.dtype == torch.float32 and X.shape[0] > 1
                and _rows_alike(X, static_x) else None)
        entry = (g, static_x, static_y, bumped, feed)
        self.graphs[(bs,) + tuple(x_shape)] = entry
        return entry

    def step(self, X, Y, sel):
        bs = sel.numel()
        key = (bs,) + tuple(X.shape[1:])
        entry = self.graphs.get(key)
        if entry is None:
            entry = self._build(bs, X)
        g, static_x, static_y, bumped, feed = entry
        # feed: the strides of the X the entry was built for, when its rows
        # can be copied whole
        if (feed is not None and X.stride() == feed
                and X.dtype == torch.float32 and Y.dtype == torch.int64
                and Y.is_contiguous() and sel.dtype == torch.int64
                and sel.is_contiguous()):
            ext().feed_gather(X, Y, sel, static_x, static_y)
        else:
            torch.index_select(X, 0, sel, out=static_x)
            torch.index_select(Y, 0, sel, out=static_y)
        g.replay()
        rng = self.gm.model.rng
        if bumped:
            rng.site = 0   # the captured step advanced the device offset
        else:
            rng.advance_step()
