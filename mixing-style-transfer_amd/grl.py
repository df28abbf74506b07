"""Gradient reversal for the adversarial branch -- the names, signatures and values of the reference's src/grl.py:16-164, so
that `from grl import GradientReversalLayer, compute_grl_lambda, compute_adversarial_lambda` (src/train.py:19) resolves here.

The layer is a plain autograd Function on any device and dtype: the forward is a view of its input, the backward one scaled
negation of a (K, embed_dim) tensor.  It has no kernel of its own: the work is one elementwise pass
over a few hundred kilobytes between two hand-written kernels, and the discriminator's input gradient is already a GEMM
epilogue away from it."""
import numpy as np
import torch.nn as nn
from torch.autograd import Function


class GradientReversalFunction(Function):
    """y = x in the forward pass; d x = -lambda * d y in the backward pass (Ganin & Lempitsky, 2015)."""

    @staticmethod
    def forward(ctx, x, lambda_param):
        ctx.lambda_param = lambda_param
        return x.view_as(x)

    @staticmethod
    def backward(ctx, grad_output):
        return grad_output.neg() * ctx.lambda_param, None


class GradientReversalLayer(nn.Module):
    """Module form of GradientReversalFunction; `lambda_param` is a plain attribute (no parameter, no buffer: the layer adds
    nothing to a state_dict), changed through `set_lambda`."""

    def __init__(self, init_lambda=1.0):
        super().__init__()
        self.lambda_param = init_lambda

    def forward(self, x):
        return GradientReversalFunction.apply(x, self.lambda_param)

    def set_lambda(self, lambda_param):
        self.lambda_param = lambda_param


def _progress(current_step, total_steps, warmup_steps):
    return np.clip((current_step - warmup_steps) / (total_steps - warmup_steps), 0.0, 1.0)


def compute_grl_lambda(current_step, total_steps, warmup_steps=2000):
    """The DANN schedule (Ganin et al., 2016): 0.0 before `warmup_steps`, then 2 / (1 + exp(-10 p)) - 1 with p the fraction of
    the remaining steps done, clipped to [0, 1]."""
    if current_step < warmup_steps:
        return 0.0
    return 2.0 / (1.0 + np.exp(-10.0 * _progress(current_step, total_steps, warmup_steps))) - 1.0


def compute_adversarial_lambda(current_step, total_steps, warmup_steps, initial_lambda, final_lambda):
    """Weight of the adversarial loss: `initial_lambda` before `warmup_steps`, then linear in the same clipped progress up to
    `final_lambda`."""
    if current_step < warmup_steps:
        return initial_lambda
    return initial_lambda + (final_lambda - initial_lambda) * _progress(current_step, total_steps, warmup_steps)
