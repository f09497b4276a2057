"""The order in which the three tape-path calls -- mdt_sample_ddim_steer, mdt_sample_steer, mdt_log_likelihood
(include/mdt_hip_train.h) -- refuse their arguments: two faults at once, and the call reports the one it meets first.  The head
checks (null pointers, batch, candidates), each entry's own checks and the tail checks (tokens2, the handle's state) are one
sequence per entry; tests/test_cpu_steer_abi.py, test_cpu_steer_plan_abi.py and test_cpu_loglik_abi.py pin each message one fault
at a time, and their fake handles and ``observe`` calls are the ones used here.  No device is needed."""
import pytest

from tests import test_cpu_loglik_abi as loglik
from tests import test_cpu_steer_abi as ddim
from tests import test_cpu_steer_plan_abi as plan

INVALID, STATE = 1, 5
NEGATIVE = (80.0, -2.0, 0.05, 0.0)  # a schedule with a negative level at [1]

# entry -> [(the two faults, the arguments that hold both, what the message must say, what it must not)]
PAIRS = {
    ddim: [
        ("null tokens + batch 0", dict(tokens=None, batch=0), ": null tokens", "batch"),
        ("batch 0 + n_steps 0", dict(batch=0, n_steps=0), ": batch is 0", "n_steps"),
        ("candidates 0 + beta nan", dict(candidates=0, beta=float("nan")), ": candidates is 0", "beta"),
        ("n_steps 0 + beta 0", dict(n_steps=0, beta=0.0), ": n_steps is 0", "beta"),
        ("beta 0 + a negative level", dict(beta=0.0, sigmas=NEGATIVE), ": beta is 0", "sigmas"),
        ("a negative level + lo without hi", dict(sigmas=NEGATIVE, lo=ddim.PTR), ": sigmas[1] is -2", "null hi"),
        ("lo without hi + MDT without tokens2", dict(lo=ddim.PTR, handle=ddim.HANDLE_MDT), ": null hi", "tokens2"),
        ("MDT without tokens2 + no training state", dict(handle=ddim.HANDLE_MDT), ": null tokens2", "mdt_train_prepare"),
    ],
    plan: [
        ("candidates 0 + beta 0", dict(candidates=0, beta=0.0), ": candidates is 0", "beta"),
        ("beta 0 + kind 11", dict(beta=0.0, kind=11), ": beta is 0", "kind"),
        ("kind 11 + a negative level", dict(kind=11, sigmas=NEGATIVE), ": kind is 11", "sigmas_host"),
        ("a negative level + lo without hi", dict(sigmas=NEGATIVE, lo=plan.PTR), ": sigmas_host[1] is -2", "null hi"),
        ("lo without hi + churn without noise", dict(lo=plan.PTR, params=dict(s_churn=1.0)), ": null hi", "noise"),
        ("churn without noise + MDT without tokens2", dict(params=dict(s_churn=1.0), handle=plan.HANDLE_MDT), ": null noise",
         "tokens2"),
    ],
    loglik: [
        ("candidates 0 + params.size", dict(candidates=0, p=loglik.params(size=loglik.SIZE - 8)), ": candidates is 0", "size"),
        ("probes 0 + sigma_min 0", dict(p=loglik.params(probes=0), sigma_min=0.0), ": params.probes is 0", "sigma_min"),
        ("sigma_max <= sigma_min + rtol 0", dict(sigma_max=0.001, p=loglik.params(rtol=0.0)), ": sigma_max is 0.001", "rtol"),
        ("max_steps 0 + MDT without tokens2", dict(p=loglik.params(max_steps=0), handle=loglik.HANDLE_MDT),
         ": params.max_steps is 0", "tokens2"),
        ("MDT without tokens2 + no training state", dict(handle=loglik.HANDLE_MDT), ": null tokens2", "mdt_train_prepare"),
    ],
}
CASES = [pytest.param(mod, kw, first, second, id=f"{mod.NAME}: {pair}") for mod, rows in PAIRS.items()
         for pair, kw, first, second in rows]


@pytest.mark.parametrize("mod, kw, first, second", CASES)
def test_of_two_faults_the_call_reports_the_one_it_meets_first(mod, kw, first, second):
    st, msg = mod.observe(**kw)
    assert st == INVALID and msg.startswith(mod.NAME + first) and second not in msg, (st, msg)


@pytest.mark.parametrize("mod, kw, first, second", CASES)
def test_each_fault_of_a_pair_is_refused_when_it_stands_alone(mod, kw, first, second):
    """Neither half of a pair passes on its own: the pair's order is between two refusals, not a refusal and a pass."""
    if len(kw) == 1:  # the second fault is the handle's missing training state, which every fake handle has
        st, msg = mod.observe(tokens2=mod.PTR, **kw)
        assert st == STATE and "mdt_train_prepare" in msg, (st, msg)
        return
    for key, value in kw.items():
        st, msg = mod.observe(**{key: value})
        assert st == INVALID and msg.startswith(mod.NAME + ": "), (key, st, msg)
