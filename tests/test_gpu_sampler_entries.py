"""Every fixed-schedule sampler entry point called as a C client calls it (tests/raw_sampler.py), against the Python facade with
the equivalent keywords, bit for bit (pytest -m gpu).  The facade only ever takes the ``_opt`` entries; the other fourteen are
adapters over the same request, and this pins the argument order of each: host and device schedule, plain and guided.

B = 2, the smallest batch at which a swapped ``batch`` / ``n_noise`` or a host / device mix-up cannot pass by accident, three
levels and the final zero, 'heun' with churn (so that its noise rows are read), 'dpmpp_sde' with a two-seed tree for the tree
entries.  No kernel is specific to an entry, so no larger shape is needed."""
import ctypes as C

import pytest
import torch

from mdt_policy_amd import _lib
from tests import raw_sampler as raw
from tests.test_gpu_sampler_bounds import SMAX, SMIN, gs, inputs

pytestmark = pytest.mark.gpu

LAM, N, TOL = 3.0, 3, 1e-6
HEUN = dict(s_churn=1.0)


def case():
    model, state, goal, x = inputs(2)
    torch.manual_seed(23)
    noise = torch.randn(N, *x.shape, device=x.device)
    seeds = torch.tensor([17, 18], dtype=torch.int64, device=x.device)
    return model, state, goal, x, gs.get_sigmas_exponential(N, SMIN, SMAX), noise, seeds


def facade(name, model, state, goal, x, sig, noise, seeds, lam):
    fam = raw.family(name)
    sig = sig.cuda() if raw.device_schedule(name) else sig
    if fam == "ddim":
        return model.sample_ddim(state, x, goal, sig, cond_lambda=lam)
    if fam == "tree":
        return model.sample_native("dpmpp_sde", state, x, goal, sig, cond_lambda=lam, tree=(seeds, TOL))
    return model.sample_native("heun", state, x, goal, sig, noise=noise, cond_lambda=lam, **HEUN)


def entry(name, model, state, goal, x, sig, noise, seeds, **kw):
    fam = raw.family(name)
    if fam == "tree":
        kw["tree"] = _lib.BrownianSource(seeds.data_ptr(), int(seeds.numel()), 0, 0.0, 0.0, TOL)
    elif fam == "plan":
        kw.update(kind="heun", params=HEUN, noise=noise)
    return raw.run(name, model, state, x, goal, sig, **kw)


@pytest.mark.parametrize("name", raw.FIXED)
def test_entry_equals_the_facade(name):
    args = case()
    with torch.no_grad():
        if name.endswith("_opt"):  # the full form: NULL is the plain call, cond_lambda the guided one
            opts = _lib.SampleOpts(C.sizeof(_lib.SampleOpts), LAM, None, None, None, None, None, None)
            pairs = [(entry(name, *args, opts=None), facade(name, *args, None)),
                     (entry(name, *args, opts=opts), facade(name, *args, LAM))]
        elif name.endswith("_guided"):
            pairs = [(entry(name, *args, lam=LAM), facade(name, *args, LAM))]
        else:
            pairs = [(entry(name, *args), facade(name, *args, None))]
        plain = facade(name, *args, None)
    for got, want in pairs:
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want), name
    if not name.endswith(("_guided", "_opt")):
        return
    assert not torch.equal(pairs[-1][0], plain), "guidance changed nothing: the comparison above would not see a dropped weight"


def test_a_tree_entry_without_its_tree_is_refused():
    """Status and text are those a tree without seeds has always been given; the handle then keeps working."""
    model, state, goal, x, sig, noise, seeds = case()
    for name in [n for n in raw.FIXED if raw.family(n) == "tree"]:
        with pytest.raises(_lib.MDTHipError) as err, torch.no_grad():
            raw.run(name, model, state, x, goal, sig, tree=None, lam=LAM)
        assert err.value.status == 1
        assert str(err.value).endswith(f"{name}: bad argument (seeds, n_seeds = 1 or batch, batch, per_row)"), str(err.value)
    with torch.no_grad():
        assert torch.equal(entry("mdt_sample_sde_tree", model, state, goal, x, sig, noise, seeds),
                           facade("mdt_sample_sde_tree", model, state, goal, x, sig, noise, seeds, None))


def test_inputs_that_need_conversion_give_the_bits_of_the_plain_call():
    """Every operand at once in a form the engine has to copy first -- float64 state tokens and goal, a non-contiguous x_T,
    non-contiguous noise rows, a float64 device schedule (all exact in fp32): the copies must live until the call is enqueued, or a
    later copy takes an earlier one's block and the sampler reads that."""
    model, state, goal, x, sig, noise, seeds = case()
    state64 = dict(state, state_images=state["state_images"].double())
    x_nc, noise_nc = torch.stack([x, -x], -1)[..., 0], torch.stack([noise, -noise], -1)[..., 0]
    assert not x_nc.is_contiguous() and not noise_nc.is_contiguous() and torch.equal(x_nc, x)
    sig64 = sig.cuda().double()
    with torch.no_grad():
        want = model.sample_native("heun", state, x, goal, sig.cuda(), noise=noise, **HEUN)
        want_ddim = model.sample_ddim(state, x, goal, sig.cuda())
        for _ in range(3):  # (the allocator's choice of block depends on what earlier calls freed)
            assert torch.equal(model.sample_native("heun", state64, x_nc, goal.double(), sig64, noise=noise_nc, **HEUN), want)
            assert torch.equal(model.sample_ddim(state64, x_nc, goal.double(), sig64), want_ddim)
