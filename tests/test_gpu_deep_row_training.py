"""Whole training steps at the row counts where the training path changes its kernels (pytest -m gpu): the cases and batches of
tests/deep_row_configs.py -- 64-step chunks, 64-element actions and 64-token contexts at 4096 and 8192 rows, the narrow weight
gradients on row slices of 5 and 6 rows -- each against float64 autograd through the oracle.  tests/test_route_table.py ties every
batch to the route it is there for.

One eval-mode step per (case, batch) exactly as tests/test_gpu_wide_actions.py runs it (hip_step: the loss plus the weighted-context
term, backward to every parameter, the state tokens and the goal), at that file's tolerances, which are also those of the
B = 1024 step of tests/test_train_grads.py: the loss to 1e-3 relative, every gradient to rtol 2e-3, atol 2e-3 * max |ref| + 1e-7
per tensor; a second run gives the same bits.  Then one train-mode step against the mask-replaying oracle
(tests/test_gpu_train_dropout.py), one step with the bf16 split forms off, and the Linear backward's scratch, sized once, reused
across batches whose plans have different slice counts."""
import time

import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mdt_oracle as O
from tests.deep_row_configs import DEEP_DROPOUT, DEEP_ENVELOPE, DEEP_REUSE, DEEP_SPEC, DEEP_SPLIT_OFF, DEEP_STEPS, rows_of
from tests.family import Family
from tests.helpers import assert_close, params_of, to
from tests.test_gpu_wide_actions import SEEDS, hip_step

pytestmark = pytest.mark.gpu

_ORACLE = {}   # (name, B) -> the float64 step, computed once and left unchanged
# the step that the split-off test checks again comes last, so that both read one oracle step
STEPS = [s for s in DEEP_STEPS if s != DEEP_SPLIT_OFF] + [DEEP_SPLIT_OFF]
assert sorted(STEPS) == sorted(DEEP_STEPS)


F = Family(DEEP_SPEC, DEEP_ENVELOPE, SEEDS)   # the metas and observations; every test builds its own model (fresh_model)
meta_of = F.meta_of


def fresh_model(name, meta=None):
    """A new GCDenoiser of the case on cuda:0 in eval mode, the 'rich' weights: its own handle, tape pool and scratch."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    m = GCDenoiser(DEEP_ENVELOPE[name]["cfg"], 0.5)
    m.load_state_dict(params_of(meta or meta_of(name)))
    return m.cuda().eval()


def inputs(name, B, seed):
    """(state, goal, loss inputs) on the host; state_obs (B, 1, proprio_dim) when the case switches the token on."""
    state, goal, _ = F.inputs(name, B, seed)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, DEEP_ENVELOPE[name]["cfg"], seed + 1).items()}
    return state, goal, li


def oracle_step(name, B):
    """(loss, {parameter: gradient}, {state key: gradient}, goal gradient) of hip_step's objective in float64, once per (name, B)."""
    if (name, B) not in _ORACLE:
        e = DEEP_ENVELOPE[name]
        cfg, arch = e["cfg"], e["arch"]
        state, goal, li = inputs(name, B, 61)
        t0 = time.perf_counter()
        P = {k: v.requires_grad_(v.dtype.is_floating_point) for k, v in params_of(meta_of(name), torch.float64).items()}
        st64 = to(state, lambda v: v.double().requires_grad_())
        g64 = goal.double().requires_grad_()
        lo, _ = O.loss(P, cfg, st64, li["actions"].double(), g64, li["noise_train"].double(), li["sigma"].double(), arch=arch)
        c = O.encode(P, cfg, st64, g64, arch, "forward", sigma=li["sigma"].double())
        wctx = synthetic.normal("ctx_weight", tuple(c.shape), 63)   # hip_step's weights
        (lo + 0.1 * (c * torch.from_numpy(wctx).double()).sum() / c.numel()).backward()
        print(f"{name} B = {B}: the float64 step took {time.perf_counter() - t0:.2f} s")
        _ORACLE.clear()   # one step's gradients at a time
        _ORACLE[(name, B)] = (lo.item(), {k: v.grad for k, v in P.items()}, {k: v.grad for k, v in st64.items() if torch.is_tensor(v)}, g64.grad)
    return _ORACLE[(name, B)]


def check_against_the_oracle(model, loss, got, name, B):
    lo, pg, sg, gg = oracle_step(name, B)
    what = f"{name} B = {B}"
    assert abs(loss.item() - lo) <= 1e-3 * abs(lo), f"{what}: loss {loss.item()} vs {lo}"
    n, top = 0, (0.0, "")
    for k, p in model.inner_model.named_parameters():
        if not p.requires_grad:  # the rotary frequency buffers
            continue
        ref = pg["inner_model." + k]
        if ref is None:
            assert k not in got, k
            continue
        atol = 2e-3 * float(ref.abs().max()) + 1e-7
        top = max(top, (float(((got[k].cpu().double() - ref).abs() / (atol + 2e-3 * ref.abs())).max()), k))
        assert_close(got[k].cpu(), ref, rtol=2e-3, atol=atol, what=f"{what} {k}")
        n += 1
    print(f"{what}: {n} gradients, largest error {top[0]:.3f} of its tolerance ({top[1]})")
    assert n > 20 and "action_emb.weight" in got and any(k.startswith("action_pred") for k in got)
    for k, v in sg.items():
        assert_close(got["d_" + k].cpu(), v, rtol=2e-3, atol=2e-3 * float(v.abs().max()) + 1e-9, what=f"{what} d_{k}")
    assert_close(got["d_goal"].cpu(), gg, rtol=2e-3, atol=2e-3 * float(gg.abs().max()) + 1e-9, what=f"{what} d_goal")


def same_gradients(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs in bits"


@pytest.mark.parametrize("name,B", STEPS, ids=[f"{n}-B{b}" for n, b in STEPS])
def test_training_step_at_deep_rows_matches_the_float64_oracle(name, B):
    """One eval-mode step: loss, every parameter gradient -- action_emb.weight and the action_pred gradients among them --, the
    state tokens' and the goal's; twice, with the same bits."""
    Me, Md = rows_of(name, B)
    print(f"{name} B = {B}: {Me} encoder rows, {Md} decoder rows")
    model = fresh_model(name)
    state, goal, li = inputs(name, B, 61)
    loss, _, got = hip_step(model, name, state, goal, li)
    loss2, _, again = hip_step(model, name, state, goal, li)
    assert loss.item() == loss2.item()
    same_gradients(got, again, f"{name} B = {B}, two runs")
    check_against_the_oracle(model, loss, got, name, B)


def test_step_with_the_split_forms_off():
    """ta64_a64 at 8192 rows with mdt_op_set_ws_split(0) and mdt_op_set_tn_split(0): the fp32 weight-stationary body and the
    192-wide fp32 k_gemm_tn under chunk attention and the wide head."""
    from mdt_policy_amd import _lib
    name, B = DEEP_SPLIT_OFF
    L = _lib.load()
    state, goal, li = inputs(name, B, 61)
    L.mdt_op_set_ws_split(0)
    L.mdt_op_set_tn_split(0)
    try:
        model = fresh_model(name)
        loss, _, got = hip_step(model, name, state, goal, li)
    finally:
        L.mdt_op_set_ws_split(-1)
        L.mdt_op_set_tn_split(-1)
    check_against_the_oracle(model, loss, got, name, B)


def test_train_mode_step_at_8192_rows_matches_the_masked_float64_oracle():
    """ta64_a64_d192 at B = 128 in train mode at the shipped dropout probabilities: the chunk attention's dropout instantiation at
    a real batch, with the checks of tests/test_gpu_train_dropout.py."""
    from tests.test_gpu_train_dropout import check_step, facade, hip_loss_step, oracle_loss_step
    name, B = DEEP_DROPOUT
    cfg = DEEP_ENVELOPE[name]["cfg"]
    assert (cfg["attn_pdrop"], cfg["resid_pdrop"], cfg["mlp_pdrop"]) == (0.3, 0.1, 0.05)
    meta = meta_of(name)
    state, goal, li = inputs(name, B, 71)
    model, seeds = facade(meta, cfg)
    hip = hip_loss_step(model, meta, state, goal, li, torch_seed=31)
    assert len(seeds) == 1 and seeds[0] > 0
    ref = oracle_loss_step(meta, cfg, state, goal, li, seeds[0], None)
    check_step(hip, ref, f"{name} B = {B}, train mode", at_least=30)


def test_scratch_sized_at_one_batch_serves_a_batch_with_more_slices():
    """The Linear backward's scratch is sized once, and a smaller batch can be cut into more slices than the capacity batch
    (mdt_route_train.h; tests/test_route_table.py: the 384 x 384 weight gradients at B = 105 against B = 128).  A model that steps
    at 128 and then at 105, one that steps at 105 and then at 128, and a model that has only ever seen 105: the same bits in every
    gradient of each batch."""
    name, cap, small = DEEP_REUSE
    meta = meta_of(name)
    at_cap, at_small = inputs(name, cap, 61), inputs(name, small, 61)

    def steps(*batches):
        model, out = fresh_model(name, meta), {}
        for B in batches:
            state, goal, li = at_cap if B == cap else at_small
            loss, _, grads = hip_step(model, name, state, goal, li)
            out[B] = (loss.item(), {k: v.cpu() for k, v in grads.items()})
        return out

    down, alone, up = steps(cap, small), steps(small), steps(small, cap)
    for what, a, b in ((f"{small} after {cap}", down[small], alone[small]), (f"{small} before {cap}", up[small], alone[small]),
                       (f"{cap} after {small}", up[cap], down[cap])):
        assert a[0] == b[0], f"{name}: the loss at {what}"
        same_gradients(a[1], b[1], f"{name} at {what}")
