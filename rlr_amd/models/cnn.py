"""The reference model zoo (reference src/models.py:11-58), rebuilt on the
rlr_amd op layer.  Parameter shapes, registration order and default init are
identical to the reference (nn.Conv2d / nn.Linear containers), so the flat
parameter vector is layout-compatible: CNN_MNIST = 1,199,882 params,
CNN_CIFAR = 537,610 params (asserted in tests/test_models.py).

forward() composes the fused conv+relu / linear+relu HIP ops; dropout uses
the deterministic philox stream (ops.functional.DropoutCtx)."""

import torch.nn as nn

from ..ops import functional as Fo


class _OpsModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.rng = Fo.DropoutCtx()
        self.compute_dtype = None  # None = fp32; torch.bfloat16 for the
                                   # bf16 MFMA path (--dtype bf16, GPU only)

    def set_dropout_seed(self, seed: int):
        self.rng.reset(seed)

    def set_compute_dtype(self, dtype):
        self.compute_dtype = dtype

    # True where manual_step takes bump_offset=True and then advances the
    # device dropout offset itself, as the last thing of the step
    # (engine.TrainEngine asks for it)
    tape_bumps_offset = False

    def _tape_begin(self, convs):
        """Start of an fp32 manual tape: the queue its reductions wait on
        and the step's conv weight permutes, ((weight, kind), ...) with
        kind 0 = forward wt, 1 = bwd-data wp, in one launch.  Weights only
        change in the optimizer kernels after the tape, so one permute per
        step serves the forward and the backward.  (None, Nones) with
        RLR_AMD_NO_STEP_BATCH=1: every kernel then runs stand-alone."""
        from ..ops import ext, step_batching
        if not step_batching():
            return None, [None] * len(convs)
        E = ext()
        return E.StepQueue(), E.prep_conv_weights(list(convs))

    def _tape_end(self, q, st, bump_offset):
        """End of a manual tape: the queued folds in two launches; the
        dropout-offset bump rides in the second one when asked for."""
        if bump_offset:
            if q is not None:
                q.add_u64(st, 1, self.rng.SITE_STRIDE)
            else:
                st[1] += self.rng.SITE_STRIDE
        if q is not None:
            q.flush()

    def _cast_in(self, x):
        if self.compute_dtype is not None and x.dtype != self.compute_dtype:
            x = x.to(self.compute_dtype)
        return x


class CNN_MNIST(_OpsModel):
    """28x28x1: conv(1->32,3x3)+relu, conv(32->64,3x3)+relu, maxpool2,
    flatten 9216, dropout .5, fc 9216->128+relu, dropout, fc 128->10
    (reference models.py:11-31)."""

    tape_bumps_offset = True

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 32, kernel_size=(3, 3))
        self.conv2 = nn.Conv2d(32, 64, kernel_size=(3, 3))
        self.fc1 = nn.Linear(9216, 128)
        self.fc2 = nn.Linear(128, 10)
        self.p_drop = 0.5

    def forward(self, x):
        x = self._cast_in(x)
        x = Fo.conv2d(x, self.conv1.weight, self.conv1.bias, relu=True)
        x = Fo.conv2d(x, self.conv2.weight, self.conv2.bias, relu=True)
        x = Fo.max_pool2d_2x2(x)
        x = Fo.flatten2d(x)
        x = Fo.dropout(x, self.p_drop, self.training, self.rng)
        x = Fo.linear(x, self.fc1.weight, self.fc1.bias, relu=True)
        x = Fo.dropout(x, self.p_drop, self.training, self.rng)
        x = Fo.linear(x, self.fc2.weight, self.fc2.bias)
        return x

    def manual_step(self, x, labels, dloss, bump_offset=False):
        """Hand-rolled fwd+bwd (fp32 GPU): identical kernel sequence to
        the autograd path, but weight/bias grads are written DIRECTLY into
        the preset p.grad flat-views (assignment == accumulate-into-zero,
        bitwise) — no zero-grad fill, no autograd accumulate-adds.

        The folds of the backward (bias grads, split-K / chunk combines,
        the head's stage B) wait on a StepQueue and run as two batched
        launches at the end; every gradient is complete on return."""
        from ..ops import ext
        E = ext()
        p = self.p_drop
        st = self.rng.gpu_state(x.device)
        q, (wt1, wt2, wp2) = self._tape_begin((
            (self.conv1.weight, 0), (self.conv2.weight, 0),
            (self.conv2.weight, 1)))
        a1 = E.conv2d_fwd(x, self.conv1.weight, self.conv1.bias, 1, 0, True,
                          wt1)
        # conv2 pools in its own epilogue (ops/csrc/conv_f32.hip): its
        # full-size output a2 is never stored, only its shape is kept
        pl, idx = E.conv2d_pool_fwd(a1, self.conv2.weight, self.conv2.bias,
                                    1, 0, wt2)
        a2_shape = [a1.shape[0], self.conv2.weight.shape[0],
                    a1.shape[2] - 2, a1.shape[3] - 2]
        # flatten + dropout-1 in one kernel (ops/csrc/fused_tail.hip)
        d1, m1 = E.flatten_dropout_fwd(pl, p, st, 0)
        h1 = E.linear_fwd(d1, self.fc1.weight, self.fc1.bias, True)

        # Backward with the relu masks FUSED away (each bitwise-identical
        # to the separate relu_bwd: see maxpool2x2_bwd_gather4_k /
        # dropout_relu_bwd_k / conv_bwd_data relu_y notes in ops/csrc):
        #   * fc1's relu folds into the dropout-2 backward;
        #   * conv2's relu folds into the maxpool gather via the pooled
        #     values (window max == pooled value for post-relu inputs);
        #   * conv1's relu folds into conv2's bwd-data epilogue.
        # The classifier head (dropout-2, fc2, CE, and their backwards up
        # to fc1's relu mask) is two launches; the seam backward is one.
        loss, g = E.fc_head_step(h1, self.fc2.weight, self.fc2.bias, labels,
                                 dloss, p, st, 1, self.fc2.weight.grad,
                                 self.fc2.bias.grad, q)
        g = E.linear_bwd_into(d1, self.fc1.weight, g,
                              self.fc1.weight.grad, self.fc1.bias.grad, True,
                              q)
        g = E.dropout_unflatten_pool_bwd_relu(g, m1, idx, pl, p, a2_shape)
        g = E.conv2d_bwd_into(a1, self.conv2.weight, g, 1, 0, True,
                              self.conv2.weight.grad, self.conv2.bias.grad,
                              a1, wp2, q)
        E.conv2d_bwd_into(x, self.conv1.weight, g, 1, 0, False,
                          self.conv1.weight.grad, self.conv1.bias.grad,
                          None, None, q)
        self._tape_end(q, st, bump_offset)
        return loss


class CNN_CIFAR(_OpsModel):
    """32x32x3: 3 x [conv3x3 (3->64->128->256)+relu+maxpool2], flatten 1024,
    dropout-interleaved FCs 1024->128->256->10 (reference models.py:33-58;
    the reference's `64*4*4` flatten literal equals 256*2*2 = 1024)."""

    tape_bumps_offset = True

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 3)
        self.conv2 = nn.Conv2d(64, 128, 3)
        self.conv3 = nn.Conv2d(128, 256, 3)
        self.fc1 = nn.Linear(1024, 128)
        self.fc2 = nn.Linear(128, 256)
        self.fc3 = nn.Linear(256, 10)
        self.p_drop = 0.5

    def forward(self, x):
        x = self._cast_in(x)
        x = Fo.max_pool2d_2x2(Fo.conv2d(x, self.conv1.weight, self.conv1.bias, relu=True))
        x = Fo.max_pool2d_2x2(Fo.conv2d(x, self.conv2.weight, self.conv2.bias, relu=True))
        x = Fo.max_pool2d_2x2(Fo.conv2d(x, self.conv3.weight, self.conv3.bias, relu=True))
        x = Fo.flatten2d(x)
        x = Fo.dropout(x, self.p_drop, self.training, self.rng)
        x = Fo.linear(x, self.fc1.weight, self.fc1.bias, relu=True)
        x = Fo.dropout(x, self.p_drop, self.training, self.rng)
        x = Fo.linear(x, self.fc2.weight, self.fc2.bias, relu=True)
        x = Fo.dropout(x, self.p_drop, self.training, self.rng)
        x = Fo.linear(x, self.fc3.weight, self.fc3.bias)
        return x

    def manual_step(self, x, labels, dloss, bump_offset=False):
        """Hand-rolled fwd+bwd — see CNN_MNIST.manual_step."""
        from ..ops import ext
        E = ext()
        p = self.p_drop
        st = self.rng.gpu_state(x.device)
        q, (wt1, wt2, wt3, wp2, wp3) = self._tape_begin((
            (self.conv1.weight, 0), (self.conv2.weight, 0),
            (self.conv3.weight, 0), (self.conv2.weight, 1),
            (self.conv3.weight, 1)))
        a1 = E.conv2d_fwd(x, self.conv1.weight, self.conv1.bias, 1, 0, True,
                          wt1)
        p1, i1 = E.maxpool2x2_fwd(a1)
        a2 = E.conv2d_fwd(p1, self.conv2.weight, self.conv2.bias, 1, 0, True,
                          wt2)
        p2, i2 = E.maxpool2x2_fwd(a2)
        a3 = E.conv2d_fwd(p2, self.conv3.weight, self.conv3.bias, 1, 0, True,
                          wt3)
        p3, i3, d1, m1 = E.pool_flatten_dropout_fwd(a3, p, st, 0)
        h1 = E.linear_fwd(d1, self.fc1.weight, self.fc1.bias, True)
        d2, m2 = E.dropout_fwd_dev(h1, p, st, 1)
        h2 = E.linear_fwd(d2, self.fc2.weight, self.fc2.bias, True)

        # relu masks fused (see CNN_MNIST.manual_step): fc relus fold
        # into the dropout backwards; every conv relu folds into the
        # following maxpool gather via the pooled values.
        loss, g = E.fc_head_step(h2, self.fc3.weight, self.fc3.bias, labels,
                                 dloss, p, st, 2, self.fc3.weight.grad,
                                 self.fc3.bias.grad, q)
        g = E.linear_bwd_into(d2, self.fc2.weight, g,
                              self.fc2.weight.grad, self.fc2.bias.grad, True,
                              q)
        g = E.dropout_relu_bwd(g, m2, h1, p)
        g = E.linear_bwd_into(d1, self.fc1.weight, g,
                              self.fc1.weight.grad, self.fc1.bias.grad, True,
                              q)
        g = E.dropout_unflatten_pool_bwd_relu(g, m1, i3, p3, p,
                                              list(a3.shape))
        g = E.conv2d_bwd_into(p2, self.conv3.weight, g, 1, 0, True,
                              self.conv3.weight.grad, self.conv3.bias.grad,
                              None, wp3, q)
        g = E.maxpool2x2_bwd_relu(g, i2, p2, list(a2.shape))
        g = E.conv2d_bwd_into(p1, self.conv2.weight, g, 1, 0, True,
                              self.conv2.weight.grad, self.conv2.bias.grad,
                              None, wp2, q)
        g = E.maxpool2x2_bwd_relu(g, i1, p1, list(a1.shape))
        E.conv2d_bwd_into(x, self.conv1.weight, g, 1, 0, False,
                          self.conv1.weight.grad, self.conv1.bias.grad,
                          None, None, q)
        self._tape_end(q, st, bump_offset)
        return loss
