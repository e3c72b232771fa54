"""torch autograd for the closed-loop roll-out (HybridNLP.differentiable_rollout): the forward pass is
qln_tracking_rollout, the backward pass its reverse sweep qln_tracking_rollout_vjp and the forward-mode tangent its forward
sweep qln_tracking_rollout_jvp (include/qln_evaluator.h).  ModelRolloutFunction is the same over the _model_ forms, with the
per-problem plant model as a fourth differentiable input."""
from __future__ import annotations

import torch


def _plain(t):
    """t (or None) without its torch.func wrappers.  Inside torch.func.jvp the saved tensors and the tangents reach the jvp
    staticmethod wrapped, with no storage of their own; the launch needs the values."""
    F = torch._C._functorch
    while t is not None and F.is_functorch_wrapped_tensor(t):
        t = F.get_unwrapped(t)
    return t


class RolloutFunction(torch.autograd.Function):
    """Zout = rollout(Zref, K, x0).  Zref, K and x0 are float64 CUDA tensors (K and x0 may be None); the gradient of an
    input that is None or needs none is None.  Entries of Zref past n_nlp are never read, so their gradient is zero.
    forward takes no ctx and setup_context keeps the inputs and the output: the form torch.func's transforms need."""

    @staticmethod
    def forward(nlp, Zref, K, x0):
        Zref_c = Zref.detach().contiguous()
        K_c = None if K is None else K.detach().contiguous()
        x0_c = None if x0 is None else x0.detach().contiguous()
        return nlp.tracking_rollout(Zref_c, K_c, x0_c)

    @staticmethod
    def setup_context(ctx, inputs, output):
        nlp, Zref, K, x0 = inputs
        ctx.nlp = nlp
        ctx.K_shape = None if K is None else K.shape
        ctx.x0_shape = None if x0 is None else x0.shape
        ctx.save_for_backward(Zref, K, output)
        ctx.save_for_forward(Zref, K, output)

    @staticmethod
    def backward(ctx, Zbar):
        _, need_zref, need_k, need_x0 = ctx.needs_input_grad
        Zref, K, Zout, Zbar = (_plain(t) for t in (*ctx.saved_tensors, Zbar))
        want = [w for w, on in (("Zref", need_zref), ("K", need_k and K is not None), ("x0", need_x0)) if on]
        if not want:
            return None, None, None, None
        with torch._C._DisableFuncTorch():  # as in jvp: plain tensors for the launch
            Zref, K, Zout, Zbar = (None if t is None else t.detach().contiguous() for t in (Zref, K, Zout, Zbar))
            zb, kb, xb = ctx.nlp.tracking_rollout_vjp(Zref, Zout, Zbar, K, want=want)
            kb = None if kb is None else kb.reshape(ctx.K_shape)
            xb = None if xb is None or ctx.x0_shape is None else xb.reshape(ctx.x0_shape)
        return None, zb, kb, xb

    @staticmethod
    def jvp(ctx, _, Zref_dot, K_dot, x0_dot):
        Zref, K, Zout, *dots = (_plain(t) for t in (*ctx.saved_tensors, Zref_dot, K_dot, x0_dot))
        # the launch takes plain tensors: while a torch.func level is active every torch op would wrap its result again
        with torch._C._DisableFuncTorch():
            Zref, K, Zout, *dots = (None if t is None else t.detach().contiguous() for t in (Zref, K, Zout, *dots))
            if K is None:
                dots[1] = None
            if all(t is None for t in dots):
                return torch.zeros_like(Zout)
            return ctx.nlp.tracking_rollout_jvp(Zref, Zout, K, *dots)


class ModelRolloutFunction(torch.autograd.Function):
    """Zout = rollout(Zref, K, x0, model), model a (B, 4) float64 CUDA tensor of per-problem plant models (g, mb, mf, lb).
    As RolloutFunction, over qln_tracking_rollout_model and its two sweeps; the gradient of model is model_bar."""

    @staticmethod
    def forward(nlp, Zref, K, x0, model):
        Zref_c, K_c, x0_c, model_c = (None if t is None else t.detach().contiguous() for t in (Zref, K, x0, model))
        return nlp.tracking_rollout_model(Zref_c, K_c, x0_c, model_c)

    @staticmethod
    def setup_context(ctx, inputs, output):
        nlp, Zref, K, x0, model = inputs
        ctx.nlp = nlp
        ctx.K_shape = None if K is None else K.shape
        ctx.x0_shape = None if x0 is None else x0.shape
        ctx.model_shape = model.shape
        ctx.save_for_backward(Zref, K, model, output)
        ctx.save_for_forward(Zref, K, model, output)

    @staticmethod
    def backward(ctx, Zbar):
        _, need_zref, need_k, need_x0, need_model = ctx.needs_input_grad
        Zref, K, model, Zout, Zbar = (_plain(t) for t in (*ctx.saved_tensors, Zbar))
        want = [w for w, on in (("Zref", need_zref), ("K", need_k and K is not None), ("x0", need_x0), ("model", need_model))
                if on]
        if not want:
            return None, None, None, None, None
        with torch._C._DisableFuncTorch():  # as in jvp: plain tensors for the launch
            Zref, K, model, Zout, Zbar = (None if t is None else t.detach().contiguous() for t in (Zref, K, model, Zout, Zbar))
            zb, kb, xb, mb = ctx.nlp.tracking_rollout_model_vjp(Zref, Zout, Zbar, K, model, want=want)
            kb = None if kb is None else kb.reshape(ctx.K_shape)
            xb = None if xb is None or ctx.x0_shape is None else xb.reshape(ctx.x0_shape)
            mb = None if mb is None else mb.reshape(ctx.model_shape)
        return None, zb, kb, xb, mb

    @staticmethod
    def jvp(ctx, _, Zref_dot, K_dot, x0_dot, model_dot):
        Zref, K, model, Zout, *dots = (_plain(t) for t in (*ctx.saved_tensors, Zref_dot, K_dot, x0_dot, model_dot))
        with torch._C._DisableFuncTorch():
            Zref, K, model, Zout, *dots = (None if t is None else t.detach().contiguous()
                                           for t in (Zref, K, model, Zout, *dots))
            if K is None:
                dots[1] = None
            if all(t is None for t in dots):
                return torch.zeros_like(Zout)
            return ctx.nlp.tracking_rollout_model_jvp(Zref, Zout, K, model, *dots)
