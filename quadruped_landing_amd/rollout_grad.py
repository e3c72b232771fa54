"""torch autograd for the closed-loop roll-out (HybridNLP.differentiable_rollout): the forward pass is
qln_tracking_rollout, the backward pass its reverse sweep qln_tracking_rollout_vjp (include/qln_evaluator.h)."""
from __future__ import annotations

import torch


class RolloutFunction(torch.autograd.Function):
    """Zout = rollout(Zref, K, x0).  Zref, K and x0 are float64 CUDA tensors (K and x0 may be None); the gradient of an
    input that is None or needs none is None.  Entries of Zref past n_nlp are never read, so their gradient is zero."""

    @staticmethod
    def forward(ctx, nlp, Zref, K, x0):
        Zref_c = Zref.detach().contiguous()
        K_c = None if K is None else K.detach().contiguous()
        x0_c = None if x0 is None else x0.detach().contiguous()
        Zout = nlp.tracking_rollout(Zref_c, K_c, x0_c)
        ctx.nlp = nlp
        ctx.K_shape = None if K is None else K.shape
        ctx.x0_shape = None if x0 is None else x0.shape
        ctx.save_for_backward(Zref_c, K_c, Zout)
        return Zout

    @staticmethod
    def backward(ctx, Zbar):
        Zref, K, Zout = ctx.saved_tensors
        _, need_zref, need_k, need_x0 = ctx.needs_input_grad
        want = [w for w, on in (("Zref", need_zref), ("K", need_k and K is not None), ("x0", need_x0)) if on]
        if not want:
            return None, None, None, None
        zb, kb, xb = ctx.nlp.tracking_rollout_vjp(Zref, Zout, Zbar.contiguous(), K, want=want)
        kb = None if kb is None else kb.reshape(ctx.K_shape)
        xb = None if xb is None or ctx.x0_shape is None else xb.reshape(ctx.x0_shape)
        return None, zb, kb, xb
