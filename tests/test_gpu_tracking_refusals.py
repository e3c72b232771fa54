"""The refusals of the qln_tracking_*, qln_landing_* and qln_kalman_design_* entry points that sit behind the handle: the
overlap rule of each of the fourteen operations (the forward and the reverse sweeps counted apart), in both memory forms, and
the value checks of the host forms with the precedence between two bad values.  Every call here is refused before the device
is bound: no kernel runs.

The pairs are the ones the overlap rule has always looked at -- every (output, input) and (output, output) of the lists
below, which are written out from the rule's lists at commit b1a6346 (the tracking operations) and from the argument tables
at commit 016f813 (the smoother, the filter, its sweeps and the Kalman design's sweep) -- and only those: a pair the rule
accepts would launch and write through the alias, past the end of the smaller buffer."""
import itertools

import numpy as np
import pytest

from quadruped_landing_amd import _lib
from tests import tracking_abi as TA
from tests import tracking_cases as TC

pytestmark = pytest.mark.gpu

B, N = 3, 5
INTS = {"ny": 2, "sigma0_batch": 1, "guarded": 1}
TRAJ = ["Zref", "K", "Lgain", "H", "model", "Zout", "Xhat", "innov", "event", "event_hat", "sat"]  # the estimated sweeps'
FILTER_TRAJ = ["Zref", "Zrec", "Lgain", "H", "model", "Xhat", "innov", "event_hat"]  # the filter sweeps'
# operation -> (the entry point with every argument, the outputs the rule looks at, the inputs it looks at)
RULE = {
    "lqr": ("qln_tracking_lqr_limited", ["K", "P"], ["Ztraj", "model", "event", "sat"]),
    "rollout": ("qln_tracking_rollout_limited", ["Zout", "event", "sat"], ["Zref"]),  # not K, x0 and model
    "rollout_vjp": ("qln_tracking_rollout_limited_vjp", ["Zref_bar", "K_bar", "x0_bar", "model_bar"],
                    ["Zref", "K", "Zout", "Zbar", "model", "event", "sat"]),
    "rollout_jvp": ("qln_tracking_rollout_limited_jvp", ["Zout_dot", "event_dot"],
                    ["Zref", "K", "Zout", "model", "event", "sat", "Zref_dot", "K_dot", "x0_dot", "model_dot"]),
    "covariance": ("qln_tracking_covariance_guarded", ["Sigma", "marg", "event_var"],
                   ["Zout", "K", "Sigma0", "model", "event"]),
    "kalman": ("qln_tracking_kalman_guarded", ["Lgain", "Pest", "Sigma", "marg", "event_var"],
               ["Zout", "K", "H", "Sigma0", "model", "event"]),
    "estimated": ("qln_tracking_rollout_estimated_limited", ["Zout", "Xhat", "innov", "event", "event_hat", "sat"],
                  ["Zref", "K", "Lgain", "H", "vnoise", "wnoise", "x0", "xhat0", "model"]),
    # innov is in the rule because Lgain_dot / Lgain_bar is given
    "estimated_jvp": ("qln_tracking_rollout_estimated_limited_jvp",
                      ["Zout_dot", "Xhat_dot", "innov_dot", "event_dot", "event_hat_dot"],
                      TRAJ + ["Zref_dot", "K_dot", "Lgain_dot", "x0_dot", "xhat0_dot", "model_dot"]),
    "estimated_vjp": ("qln_tracking_rollout_estimated_limited_vjp",
                      ["Zref_bar", "K_bar", "Lgain_bar", "x0_bar", "xhat0_bar", "model_bar"],
                      TRAJ + ["Zbar", "Xhat_bar", "innov_bar"]),
    "smoother": ("qln_landing_smoother_guarded", ["Xs", "Ps"],
                 ["Ztraj", "model", "event", "Lgain", "Pest", "H", "Xhat", "innov"]),
    "filter": ("qln_landing_filter_guarded_model", ["Xhat", "innov", "score", "loglik", "event_hat"],
               ["Zref", "Zrec", "Lgain", "H", "model", "Y", "xhat0"]),
    # innov is in the rule because nis_dot and loglik_dot / nis_bar and loglik_bar are given
    "filter_jvp": ("qln_landing_filter_guarded_jvp", ["Xhat_dot", "innov_dot", "nis_dot", "loglik_dot", "event_hat_dot"],
                   FILTER_TRAJ + ["Y_dot", "Zrec_dot", "xhat0_dot", "model_dot"]),
    "filter_vjp": ("qln_landing_filter_guarded_vjp", ["Y_bar", "Zrec_bar", "xhat0_bar", "model_bar"],
                   FILTER_TRAJ + ["Xhat_bar", "innov_bar", "nis_bar", "loglik_bar"]),
    "kalman_jvp": ("qln_kalman_design_guarded_jvp", ["Lgain_dot", "Pest_dot", "logdet_dot"],
                   ["Zout", "model", "event", "Lgain", "H", "Sigma0_dot"]),
}
# left NULL: the filter's sweeps differentiate the score at fixed gains, and refuse a call that asks for both
LEFT_OUT = {"filter_jvp": ["Lgain_dot"], "filter_vjp": ["Lgain_bar"]}
# host forms: (the parameter, the entry of its buffer, the value, what the refusal says)
VALUES = [
    ("model", 1, 0.0, "is not finite, or a mass or the body length is not positive"),  # mb = 0
    ("event", 0, float(N - 1), "is not a knot of the roll-out"),
    ("event", 1, -0.5, "(tau) is not finite or is negative"),
    ("event_hat", 0, float(N - 1), "is not a knot of the roll-out"),
    ("sat", 0, 3.0, "is not a saturation code"),
    ("H", 0, float("nan"), "H is not finite"),
]


@pytest.fixture(scope="module")
def handle():
    nlp = TC.nlp(TC.batch(B, N, 2, 1, seed=5))
    yield nlp
    del nlp


def _ones(name, nlp, device, left_out=()):
    """parameter -> its own buffer of ones of the right size (a host array where the parameter is one in both forms)"""
    import torch

    vals = {}
    for p in TA.PARAMS[name]:
        if p in left_out:
            vals[p] = None
        elif TA.is_int(name, p):
            vals[p] = INTS[p]
        elif device and p not in TA.HOST_ONLY:
            vals[p] = torch.ones(TA.size(p, B, N, nlp.dims.z_total), dtype=torch.float64, device="cuda")
        else:
            vals[p] = np.ones(TA.size(p, B, N, nlp.dims.z_total))
    return vals


def _inputs_of(name, op):
    """The event records and sat are outputs of the two roll-outs and inputs of everything else."""
    return [p for p in ("model", "event", "event_hat", "sat", "H") if p in TA.PARAMS[name] and p not in RULE[op][1]]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("op", sorted(RULE))
def test_every_pair_of_the_overlap_rule_is_refused(handle, op, host):
    name, outs, ins = RULE[op]
    name += "_host" if host else ""
    assert set(outs) | set(ins) <= set(TA.PARAMS[name])
    L, base = _lib.lib(), _ones(name, handle, device=not host, left_out=LEFT_OUT.get(op, ()))
    pairs = [(o, i, "an output overlaps an input") for o in outs for i in ins]
    pairs += [(o, q, "two outputs overlap") for o, q in itertools.combinations(outs, 2)]
    for first, second, text in pairs:
        vals = dict(base)
        vals[second] = vals[first]
        assert TA.call(handle._h, name, vals) == _lib.QLN_ERR_INVALID_ARGUMENT, (name, first, second)
        assert L.qln_last_error().decode() == f"{name}: {text}", (name, first, second)


@pytest.mark.parametrize("op", sorted(RULE))
def test_host_forms_refuse_bad_values_before_they_bind_the_device(handle, op):
    name = RULE[op][0] + "_host"
    L, checked = _lib.lib(), _inputs_of(name, op)
    for p, entry, value, text in VALUES:
        if p not in checked:
            continue
        vals = _ones(name, handle, device=False, left_out=LEFT_OUT.get(op, ()))
        vals[p][entry] = value
        outs = {q: vals[q].copy() for q in RULE[op][1]}
        assert TA.call(handle._h, name, vals) == _lib.QLN_ERR_INVALID_ARGUMENT, (name, p, value)
        assert text in L.qln_last_error().decode(), (name, p, L.qln_last_error())
        assert all(np.array_equal(vals[q], outs[q]) for q in outs)


# (operation, the two parameters whose first entry is broken in one call, which refusal wins): the order in which the host
# forms have always looked at H, the models, the event records and the saturation record -- the estimated sweeps look at the
# saturation record before the events, everything else after them
PRECEDENCE = [
    ("rollout_vjp", "event", "sat", "is not a knot of the roll-out"),
    ("lqr", "event", "sat", "is not a knot of the roll-out"),
    ("estimated_jvp", "event", "sat", "is not a saturation code"),
    ("estimated_vjp", "event", "sat", "is not a saturation code"),
    ("estimated_jvp", "model", "H", "H is not finite"),
    ("estimated_vjp", "model", "H", "H is not finite"),
]
BAD = {p: (entry, value) for p, entry, value, _ in reversed(VALUES)}  # the first bad value of each parameter above


@pytest.mark.parametrize("op,first,second,text", PRECEDENCE)
def test_two_bad_values_keep_their_precedence(handle, op, first, second, text):
    name = RULE[op][0] + "_host"
    vals = _ones(name, handle, device=False)
    for p in (first, second):
        vals[p][BAD[p][0]] = BAD[p][1]
    outs = {q: vals[q].copy() for q in RULE[op][1]}
    assert TA.call(handle._h, name, vals) == _lib.QLN_ERR_INVALID_ARGUMENT, (name, first, second)
    assert text in _lib.lib().qln_last_error().decode(), (name, first, second, _lib.lib().qln_last_error())
    assert all(np.array_equal(vals[q], outs[q]) for q in outs)
