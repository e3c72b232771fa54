"""torch autograd for the closed-loop roll-out (HybridNLP.differentiable_rollout): the forward pass is
qln_tracking_rollout, the backward pass its reverse sweep qln_tracking_rollout_vjp and the forward-mode tangent its forward
sweep qln_tracking_rollout_jvp (include/qln_evaluator.h).  ModelRolloutFunction is the same over the _model_ forms, with the
per-problem plant model as a fourth differentiable input.  GuardedRolloutFunction is the roll-out with guard-triggered
touchdown over qln_tracking_rollout_guarded and the two sweeps through the touchdown, which take its event record.
EstimatedRolloutFunction is the estimate-feedback roll-out over qln_tracking_rollout_estimated and its two sweeps."""
from __future__ import annotations

import torch


def _plain(t):
    """t (or None) without its torch.func wrappers.  Inside torch.func.jvp the saved tensors and the tangents reach the jvp
    staticmethod wrapped, with no storage of their own; the launch needs the values."""
    F = torch._C._functorch
    while t is not None and F.is_functorch_wrapped_tensor(t):
        t = F.get_unwrapped(t)
    return t


def _launchable(ts):
    """Each tensor of ts (or None) detached and contiguous: what a launch takes."""
    return [None if t is None else t.detach().contiguous() for t in ts]


class RolloutFunction(torch.autograd.Function):
    """Zout = rollout(Zref, K, x0).  Zref, K and x0 are float64 CUDA tensors (K and x0 may be None); the gradient of an
    input that is None or needs none is None.  Entries of Zref past n_nlp are never read, so their gradient is zero.
    forward takes no ctx and setup_context keeps the inputs and the output: the form torch.func's transforms need.

    The four methods are written over "the inputs after nlp", (Zref, K, x0) here and (Zref, K, x0, model) in
    ModelRolloutFunction, which inherits them: a fourth input sends the calls to the _model_ entry points."""

    @staticmethod
    def forward(nlp, Zref, K, x0, *model):
        return nlp._rollout(bool(model), *_launchable((Zref, K, x0)), *_launchable(model or (None,)), None)

    @staticmethod
    def setup_context(ctx, inputs, output):
        nlp, Zref, K, x0, *model = inputs
        ctx.nlp = nlp
        ctx.shapes = [None if t is None else t.shape for t in (K, x0, *model)]
        ctx.save_for_backward(Zref, K, *model, output)
        ctx.save_for_forward(Zref, K, *model, output)

    @staticmethod
    def backward(ctx, Zbar):
        need = ctx.needs_input_grad[1:]
        Zref, K, *model, Zout, Zbar = (_plain(t) for t in (*ctx.saved_tensors, Zbar))
        want = [w for w, on in zip(("Zref", "K", "x0", "model"), need) if on and not (w == "K" and K is None)]
        if not want:
            return (None,) * (1 + len(need))
        with torch._C._DisableFuncTorch():  # as in jvp: plain tensors for the launch
            Zref, K, Zout, Zbar = _launchable((Zref, K, Zout, Zbar))
            zb, *bars = ctx.nlp._rollout_vjp(bool(model), Zref, Zout, Zbar, K, *_launchable(model or (None,)), want)
            bars = [None if b is None or shape is None else b.reshape(shape) for b, shape in zip(bars, ctx.shapes)]
        return (None, zb, *bars)

    @staticmethod
    def jvp(ctx, _, *dots):
        Zref, K, *model, Zout = (_plain(t) for t in ctx.saved_tensors)
        # the launch takes plain tensors: while a torch.func level is active every torch op would wrap its result again
        with torch._C._DisableFuncTorch():
            Zref, K, Zout = _launchable((Zref, K, Zout))
            zd, kd, xd, *md = _launchable(_plain(t) for t in dots)
            if K is None:
                kd = None
            if all(t is None for t in (zd, kd, xd, *md)):
                return torch.zeros_like(Zout)
            return ctx.nlp._rollout_jvp(bool(model), Zref, Zout, K, *_launchable(model or (None,)), zd, kd, xd,
                                        *(md or (None,)), None)


class ModelRolloutFunction(RolloutFunction):
    """Zout = rollout(Zref, K, x0, model), model a (B, 4) float64 CUDA tensor of per-problem plant models (g, mb, mf, lb).
    As RolloutFunction, over qln_tracking_rollout_model and its two sweeps; the gradient of model is model_bar."""


class GuardedRolloutFunction(torch.autograd.Function):
    """(Zout, events) = guarded rollout(Zref, K, x0, model): qln_tracking_rollout_guarded.  K, x0 and model may be None
    (model None: the handle's).  Zout is differentiable in all four through qln_tracking_rollout_guarded_vjp / _jvp at the
    (Zout, events) the forward produced, that is at fixed touchdown knot; events is marked non-differentiable."""

    @staticmethod
    def forward(nlp, Zref, K, x0, model):
        return nlp.tracking_rollout_guarded(*_launchable((Zref, K, x0, model)))

    @staticmethod
    def setup_context(ctx, inputs, output):
        nlp, Zref, K, x0, model = inputs
        Zout, events = output
        ctx.nlp = nlp
        ctx.shapes = [None if t is None else t.shape for t in (K, x0, model)]
        ctx.mark_non_differentiable(events)
        ctx.save_for_backward(Zref, K, model, Zout, events)
        ctx.save_for_forward(Zref, K, model, Zout, events)

    @staticmethod
    def backward(ctx, Zbar, _events_bar):
        need = ctx.needs_input_grad[1:]
        Zref, K, model, Zout, events, Zbar = (_plain(t) for t in (*ctx.saved_tensors, Zbar))
        want = [w for w, on in zip(("Zref", "K", "x0", "model"), need) if on and not (w == "K" and K is None)]
        if not want:
            return (None,) * 5
        with torch._C._DisableFuncTorch():
            Zref, K, model, Zout, events, Zbar = _launchable((Zref, K, model, Zout, events, Zbar))
            zb, *bars = ctx.nlp.tracking_rollout_guarded_vjp(Zref, Zout, events, Zbar, K, model, want)
            bars = [None if b is None or shape is None else b.reshape(shape) for b, shape in zip(bars, ctx.shapes)]
        return (None, zb, *bars)

    @staticmethod
    def jvp(ctx, _, *dots):
        Zref, K, model, Zout, events = (_plain(t) for t in ctx.saved_tensors)
        with torch._C._DisableFuncTorch():
            Zref, K, model, Zout, events = _launchable((Zref, K, model, Zout, events))
            zd, kd, xd, md = _launchable(_plain(t) for t in dots)
            if K is None:
                kd = None
            if all(t is None for t in (zd, kd, xd, md)):
                return torch.zeros_like(Zout), None
            out, _ = ctx.nlp.tracking_rollout_guarded_jvp(Zref, Zout, events, K, model, zd, kd, xd, md, with_event_dot=False)
            return out, None  # events is not differentiable: event_dot is tracking_rollout_guarded_jvp's to ask for


class LimitedRolloutFunction(torch.autograd.Function):
    """(Zout, events, sat) = limited rollout(Zref, K, x0, model; limits, guarded): qln_tracking_rollout_limited, without events
    when not guarded.  limits (eight numbers) and guarded are not tensors.  Zout is differentiable in Zref, K, x0 and model
    through qln_tracking_rollout_limited_vjp / _jvp at the (Zout, events, sat) the forward produced, that is at fixed active
    set and fixed touchdown knot; events and sat are marked non-differentiable."""

    @staticmethod
    def forward(nlp, Zref, K, x0, model, limits, guarded):
        Zout, events, sat = nlp.tracking_rollout_limited(_launchable((Zref,))[0], limits, *_launchable((K, x0, model)),
                                                         guarded=guarded)
        return (Zout, events, sat) if guarded else (Zout, sat)

    @staticmethod
    def setup_context(ctx, inputs, output):
        nlp, Zref, K, x0, model, _, guarded = inputs
        Zout, *events, sat = output
        ctx.nlp, ctx.guarded = nlp, guarded
        ctx.shapes = [None if t is None else t.shape for t in (K, x0, model)]
        ctx.mark_non_differentiable(*events, sat)
        ctx.save_for_backward(Zref, K, model, Zout, sat, *events)
        ctx.save_for_forward(Zref, K, model, Zout, sat, *events)

    @staticmethod
    def backward(ctx, Zbar, *_):
        need = ctx.needs_input_grad[1:5]
        Zref, K, model, Zout, sat, *events = (_plain(t) for t in ctx.saved_tensors)
        Zbar = _plain(Zbar)
        want = [w for w, on in zip(("Zref", "K", "x0", "model"), need) if on and not (w == "K" and K is None)]
        if not want:
            return (None,) * 7
        with torch._C._DisableFuncTorch():
            Zref, K, model, Zout, sat, Zbar, *events = _launchable((Zref, K, model, Zout, sat, Zbar, *events))
            zb, *bars = ctx.nlp.tracking_rollout_limited_vjp(Zref, Zout, sat, Zbar, (events or (None,))[0], K, model, want)
            bars = [None if b is None or shape is None else b.reshape(shape) for b, shape in zip(bars, ctx.shapes)]
        return (None, zb, *bars, None, None)

    @staticmethod
    def jvp(ctx, _, *dots):
        Zref, K, model, Zout, sat, *events = (_plain(t) for t in ctx.saved_tensors)
        rest = (None,) * (2 if ctx.guarded else 1)
        with torch._C._DisableFuncTorch():
            Zref, K, model, Zout, sat, *events = _launchable((Zref, K, model, Zout, sat, *events))
            zd, kd, xd, md = _launchable(_plain(t) for t in dots[:4])
            if K is None:
                kd = None
            if all(t is None for t in (zd, kd, xd, md)):
                return (torch.zeros_like(Zout), *rest)
            out, _ = ctx.nlp.tracking_rollout_limited_jvp(Zref, Zout, sat, (events or (None,))[0], K, model, zd, kd, xd, md,
                                                          with_event_dot=False)
            return (out, *rest)


class EstimatedRolloutFunction(torch.autograd.Function):
    """(Zout, Xhat, innov[, events, events_hat]) = estimate-feedback rollout(Zref, K, Lgain, x0, xhat0, model; H, vnoise, wnoise,
    guarded): qln_tracking_rollout_estimated / _guarded.  K, x0, xhat0 and model may be None.  Zout, Xhat and innov are
    differentiable in Zref, K, Lgain, x0, xhat0 and model through qln_tracking_rollout_estimated_vjp / _jvp at the trajectory
    the forward produced, that is at fixed noise samples and (guarded) fixed touchdown knots; H, vnoise and wnoise take no
    gradient and the event records are marked non-differentiable.  xhat0 None is the forward call's: the estimate starts on
    Zref's first knot, and its gradient and tangent are Zref's there."""

    @staticmethod
    def forward(nlp, Zref, K, Lgain, x0, xhat0, model, H, vnoise, wnoise, guarded):
        Zref, K, Lgain, x0, xhat0, model, vnoise, wnoise = _launchable((Zref, K, Lgain, x0, xhat0, model, vnoise, wnoise))
        return nlp.tracking_rollout_estimated(Zref, K, Lgain, H, vnoise, wnoise, x0, xhat0, model, guarded=guarded,
                                              with_innovations=True)

    @staticmethod
    def setup_context(ctx, inputs, output):
        nlp, Zref, K, Lgain, x0, xhat0, model, H, _, _, guarded = inputs
        Zout, Xhat, innov, *events = output
        ctx.nlp, ctx.H, ctx.guarded, ctx.has_xhat0 = nlp, H, guarded, xhat0 is not None
        ctx.shapes = [None if t is None else t.shape for t in (K, Lgain, x0, xhat0, model)]
        ctx.mark_non_differentiable(*events)
        ctx.save_for_backward(Zref, K, Lgain, model, Zout, Xhat, innov, *events)
        ctx.save_for_forward(Zref, K, Lgain, model, Zout, Xhat, innov, *events)

    @staticmethod
    def backward(ctx, Zbar, Xhat_bar, innov_bar, *_):
        need = ctx.needs_input_grad[1:7]
        names = ("Zref", "K", "Lgain", "x0", "xhat0", "model")
        saved = (_plain(t) for t in (*ctx.saved_tensors, Zbar, Xhat_bar, innov_bar))
        Zref, K, Lgain, model, Zout, Xhat, innov, *rest = saved
        *events, Zbar, Xhat_bar, innov_bar = rest
        want = [w for w, on in zip(names, need) if on and not (w == "K" and K is None)]
        if not want:
            return (None,) * 11
        if ctx.has_xhat0 and "xhat0" not in want:
            want.append("xhat0")  # a given xhat0 keeps its cotangent out of Zref_bar whether or not it is asked for
        with torch._C._DisableFuncTorch():
            Zref, K, Lgain, model, Zout, Xhat, innov, Zbar, Xhat_bar, innov_bar, *events = _launchable(
                (Zref, K, Lgain, model, Zout, Xhat, innov, Zbar, Xhat_bar, innov_bar, *events))
            ev, eh = events or (None, None)
            zb, *bars = ctx.nlp.tracking_rollout_estimated_vjp(Zref, K, Lgain, ctx.H, Zout, Xhat, Zbar, innov, model, ctx.guarded,
                                                               ev, eh, Xhat_bar, innov_bar, want)
            bars = [None if b is None or shape is None or not on else b.reshape(shape)
                    for b, shape, on in zip(bars, ctx.shapes, need[1:])]
        return (None, zb if need[0] else None, *bars, None, None, None, None)

    @staticmethod
    def jvp(ctx, _, *dots):
        Zref, K, Lgain, model, Zout, Xhat, innov, *events = (_plain(t) for t in ctx.saved_tensors)
        none = (None,) * len(events)
        with torch._C._DisableFuncTorch():
            Zref, K, Lgain, model, Zout, Xhat, innov, *events = _launchable((Zref, K, Lgain, model, Zout, Xhat, innov, *events))
            zd, kd, ld, xd, hd, md = _launchable(_plain(t) for t in dots[:6])
            if K is None:
                kd = None
            if all(t is None for t in (zd, kd, ld, xd, hd, md)):
                return (torch.zeros_like(Zout), torch.zeros_like(Xhat), torch.zeros_like(innov), *none)
            if ctx.has_xhat0 and hd is None:
                hd = torch.zeros_like(Xhat[:, 0])  # a given xhat0 without a tangent does not follow Zref_dot
            ev, eh = events or (None, None)
            out = ctx.nlp.tracking_rollout_estimated_jvp(Zref, K, Lgain, ctx.H, Zout, Xhat, innov, model, ctx.guarded, ev, eh, zd,
                                                         kd, ld, xd, hd if ctx.has_xhat0 else None, md, with_event_dot=False)
            return (*out[:3], *none)


class EstimatedLimitedRolloutFunction(torch.autograd.Function):
    """(Zout, Xhat, innov[, events, events_hat], sat) = estimate-feedback rollout within force limits(Zref, K, Lgain, x0, xhat0,
    model; H, vnoise, wnoise, limits, guarded): qln_tracking_rollout_estimated_limited.  EstimatedRolloutFunction with the
    sweeps at the active set the forward produced, qln_tracking_rollout_estimated_limited_vjp / _jvp; limits (eight numbers)
    is not a tensor, and sat and the event records are marked non-differentiable."""

    @staticmethod
    def forward(nlp, Zref, K, Lgain, x0, xhat0, model, H, vnoise, wnoise, limits, guarded):
        Zref, K, Lgain, x0, xhat0, model, vnoise, wnoise = _launchable((Zref, K, Lgain, x0, xhat0, model, vnoise, wnoise))
        Zout, Xhat, innov, ev, eh, sat = nlp.tracking_rollout_estimated_limited(Zref, limits, K, Lgain, H, vnoise, wnoise, x0, xhat0,
                                                                                model, guarded=guarded, with_innovations=True)
        return (Zout, Xhat, innov, ev, eh, sat) if guarded else (Zout, Xhat, innov, sat)

    @staticmethod
    def setup_context(ctx, inputs, output):
        nlp, Zref, K, Lgain, x0, xhat0, model, H, _, _, _, guarded = inputs
        Zout, Xhat, innov, *events, sat = output
        ctx.nlp, ctx.H, ctx.guarded, ctx.has_xhat0 = nlp, H, guarded, xhat0 is not None
        ctx.shapes = [None if t is None else t.shape for t in (K, Lgain, x0, xhat0, model)]
        ctx.mark_non_differentiable(*events, sat)
        ctx.save_for_backward(Zref, K, Lgain, model, Zout, Xhat, innov, sat, *events)
        ctx.save_for_forward(Zref, K, Lgain, model, Zout, Xhat, innov, sat, *events)

    @staticmethod
    def backward(ctx, Zbar, Xhat_bar, innov_bar, *_):
        need = ctx.needs_input_grad[1:7]
        names = ("Zref", "K", "Lgain", "x0", "xhat0", "model")
        saved = (_plain(t) for t in (*ctx.saved_tensors, Zbar, Xhat_bar, innov_bar))
        Zref, K, Lgain, model, Zout, Xhat, innov, sat, *rest = saved
        *events, Zbar, Xhat_bar, innov_bar = rest
        want = [w for w, on in zip(names, need) if on and not (w == "K" and K is None)]
        if not want:
            return (None,) * 12
        if ctx.has_xhat0 and "xhat0" not in want:
            want.append("xhat0")  # a given xhat0 keeps its cotangent out of Zref_bar whether or not it is asked for
        with torch._C._DisableFuncTorch():
            Zref, K, Lgain, model, Zout, Xhat, innov, sat, Zbar, Xhat_bar, innov_bar, *events = _launchable(
                (Zref, K, Lgain, model, Zout, Xhat, innov, sat, Zbar, Xhat_bar, innov_bar, *events))
            ev, eh = events or (None, None)
            zb, *bars = ctx.nlp.tracking_rollout_estimated_limited_vjp(Zref, K, Lgain, ctx.H, Zout, Xhat, sat, Zbar, innov, model,
                                                                       ev, eh, Xhat_bar, innov_bar, want)
            bars = [None if b is None or shape is None or not on else b.reshape(shape)
                    for b, shape, on in zip(bars, ctx.shapes, need[1:])]
        return (None, zb if need[0] else None, *bars, None, None, None, None, None)

    @staticmethod
    def jvp(ctx, _, *dots):
        Zref, K, Lgain, model, Zout, Xhat, innov, sat, *events = (_plain(t) for t in ctx.saved_tensors)
        none = (None,) * (len(events) + 1)
        with torch._C._DisableFuncTorch():
            Zref, K, Lgain, model, Zout, Xhat, innov, sat, *events = _launchable(
                (Zref, K, Lgain, model, Zout, Xhat, innov, sat, *events))
            zd, kd, ld, xd, hd, md = _launchable(_plain(t) for t in dots[:6])
            if K is None:
                kd = None
            if all(t is None for t in (zd, kd, ld, xd, hd, md)):
                return (torch.zeros_like(Zout), torch.zeros_like(Xhat), torch.zeros_like(innov), *none)
            if ctx.has_xhat0 and hd is None:
                hd = torch.zeros_like(Xhat[:, 0])  # a given xhat0 without a tangent does not follow Zref_dot
            ev, eh = events or (None, None)
            out = ctx.nlp.tracking_rollout_estimated_limited_jvp(Zref, K, Lgain, ctx.H, Zout, Xhat, sat, innov, model, ev, eh, zd,
                                                                 kd, ld, xd, hd if ctx.has_xhat0 else None, md,
                                                                 with_event_dot=False)
            return (*out[:3], *none)


class LandingFilterFunction(torch.autograd.Function):
    """(Xhat, innov[, loglik][, events_hat]) = landing filter(Y, Zrec, xhat0, model, Lgain; Zref, H, V, guarded):
    qln_landing_filter_model / _guarded_model on a record.  xhat0 and model may be None.  Xhat, innov and loglik are
    differentiable in Y, Zrec (its control slots), xhat0 and model through qln_landing_filter_vjp / _jvp at the trajectory the
    forward produced: at fixed gains and (guarded) fixed touchdown knot.  Lgain is differentiable only without V, that is without
    the loglik output: log det S_k depends on the gains and its derivative is not offered.  Zref and H take no gradient, and the
    event record is marked non-differentiable."""

    @staticmethod
    def forward(nlp, Y, Zrec, xhat0, model, Lgain, Zref, H, V, guarded):
        Y, Zrec, xhat0, model, Lgain, Zref = _launchable((Y, Zrec, xhat0, model, Lgain, Zref))
        f = nlp.landing_filter_guarded if guarded else nlp.landing_filter
        Xhat, innov, _, loglik, *events = f(Zref, Zrec, Lgain, H, Y, V, xhat0, model=model)
        return (Xhat, innov, *(() if V is None else (loglik,)), *events)

    @staticmethod
    def setup_context(ctx, inputs, output):
        nlp, Y, Zrec, xhat0, model, Lgain, Zref, H, V, guarded = inputs
        ctx.nlp, ctx.H, ctx.V, ctx.guarded = nlp, H, V, guarded
        ctx.shapes = [None if t is None else t.shape for t in (Y, Zrec, xhat0, model, Lgain)]
        ctx.set_materialize_grads(False)  # an absent cotangent or tangent stays None: the sweeps tell absent from zero
        Xhat, innov, *rest = output
        events = rest[-1:] if guarded else []
        ctx.mark_non_differentiable(*events)
        ctx.save_for_backward(Zrec, model, Lgain, Zref, Xhat, innov, *events)
        ctx.save_for_forward(Zrec, model, Lgain, Zref, Xhat, innov, *events)

    @staticmethod
    def backward(ctx, Xhat_bar, innov_bar, *rest):
        need = ctx.needs_input_grad[1:6]
        score = ctx.V is not None
        if score and need[4]:
            raise RuntimeError("Lgain is differentiable only without V: the score is differentiated at fixed gains")
        loglik_bar = rest[0] if score else None
        names = ("Y", "Zrec", "xhat0", "model", "Lgain")
        want = [w for w, on, shape in zip(names, need, ctx.shapes) if on and shape is not None]
        if not want or all(t is None for t in (Xhat_bar, innov_bar, loglik_bar)):
            return (None,) * 10
        saved = [_plain(t) for t in (*ctx.saved_tensors, Xhat_bar, innov_bar, loglik_bar)]
        with torch._C._DisableFuncTorch():
            Zrec, model, Lgain, Zref, Xhat, innov, *tail = _launchable(saved)
            *events, Xhat_bar, innov_bar, loglik_bar = tail
            got = ctx.nlp.landing_filter_vjp(Zref, Zrec, Lgain, ctx.H, Xhat, innov, ctx.V, model, events[0] if events else None,
                                             ctx.guarded, Xhat_bar, innov_bar, None, loglik_bar, want)
            bars = [got[w].reshape(shape) if w in got else None for w, shape in zip(names, ctx.shapes)]
        return (None, *bars, None, None, None, None)

    @staticmethod
    def jvp(ctx, _, *dots):
        Zrec, model, Lgain, Zref, Xhat, innov, *events = (_plain(t) for t in ctx.saved_tensors)
        score = ctx.V is not None
        none = (None,) * len(events)
        with torch._C._DisableFuncTorch():
            Zrec, model, Lgain, Zref, Xhat, innov, *events = _launchable((Zrec, model, Lgain, Zref, Xhat, innov, *events))
            yd, zd, xd, md, ld = _launchable(_plain(t) for t in dots[:5])
            if score and ld is not None:
                raise RuntimeError("Lgain is differentiable only without V: the score is differentiated at fixed gains")
            zeros = (torch.zeros_like(Xhat), torch.zeros_like(innov), *((torch.zeros_like(Xhat[:, 0, 0]),) if score else ()))
            if all(t is None for t in (yd, zd, xd, md, ld)):
                return (*zeros, *none)
            want = ("Xhat", "innov") + (("loglik",) if score else ())
            got = ctx.nlp.landing_filter_jvp(Zref, Zrec, Lgain, ctx.H, Xhat, innov, ctx.V, model, events[0] if events else None,
                                             ctx.guarded, yd, zd, ld, xd, md, want)
            return (*(got[w] for w in want), *none)
