"""mdt_op_infonce (csrc/mdt_infonce.hip) at the batch, width and input edges it accepts (pytest -m gpu): every case of
tests/infonce_cases.py through clip_auxiliary_loss against the float64 oracle with a per-row gradient floor; the C entry called
directly between guard floats with NaN-filled scratch (bounds, inputs left alone, stale scratch, the value-only call, repeats);
and the Python wrapper's conversions.  The bounds and why each case is there: tests/infonce_cases.py; that a correct float32
implementation meets them with a factor of ten to spare: tests/test_cpu_infonce_abi.py."""
import ctypes as C
import functools
import types

import pytest
import torch

from tests import infonce_cases as IC
from tests.test_gpu_ops import stream

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 1024               # floats in front of and behind every region the op is handed, inside the same allocation
GUARD_BITS = 0x5EA7F00D
CANARY = 12345.678


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


def loss_fn():
    from mdt_policy_amd.models.contrastive import clip_auxiliary_loss
    return clip_auxiliary_loss


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------ the cases, through the wrapper
@pytest.mark.parametrize("cid", IC.IDS)
def test_case_against_the_float64_oracle(cid):
    IC.check(IC.run(loss_fn(), IC.case(cid), device="cuda"), IC.reference(cid), cid)


# ------------------------------------------------------------------------------------ the C entry, called directly
class Guarded:
    """n float32 the op may write, with GUARD sentinel floats on both sides in ONE allocation: an overrun cannot fault, it shows."""

    def __init__(self, n, fill=NAN):
        self.n = n
        self.buf = torch.empty(n + 2 * GUARD, device="cuda", dtype=torch.float32)
        self.buf.view(torch.int32).fill_(GUARD_BITS)
        self.region.fill_(fill)

    @property
    def region(self):
        return self.buf[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def intact(self):
        bits = self.buf.view(torch.int32)
        return bool((bits[:GUARD] == GUARD_BITS).all()) and bool((bits[GUARD + self.n:] == GUARD_BITS).all())


DIRECT = IC.DIRECT


@functools.lru_cache(maxsize=None)
def direct_case(B, D, mode):
    """A shape case that is not in the list (same recipe, seed and temperature) and its float64 Result: shared, never written to."""
    cid = f"B{B}_D{D}_{mode}"
    return IC.case(cid), IC.reference(cid)


def call_op(lib, c, grads=True, scratch=None):
    """One mdt_op_infonce call on the case's inputs.  Every output and the scratch are Guarded regions that start as NaN (a given
    `scratch` is used as it is); without `grads` the three gradient pointers are null and the buffers keep a canary."""
    L = lib.load()
    B, D = c.img.shape
    img, lang = c.img.cuda(), c.lang.cuda()
    ls = torch.tensor([c.logit_scale], device="cuda", dtype=torch.float32)
    before = (img.clone(), lang.clone(), ls.clone())
    n = L.mdt_op_infonce_scratch(B, D)
    scratch = scratch or Guarded(n)
    assert scratch.n >= n
    out = types.SimpleNamespace(loss=Guarded(1), d_img=Guarded(B * D, NAN if grads else CANARY), d_lang=Guarded(B * D, NAN if grads else CANARY),
                                d_ls=Guarded(1, NAN if grads else CANARY), scratch=scratch)
    a = lib.InfoNCEArgs(image_features=img.data_ptr(), lang_features=lang.data_ptr(), logit_scale=ls.data_ptr(), batch=B, dim=D,
                        mode=lib.INFONCE_MODE[c.mode], loss=out.loss.ptr, d_image=out.d_img.ptr if grads else None,
                        d_lang=out.d_lang.ptr if grads else None, d_logit_scale=out.d_ls.ptr if grads else None, scratch=scratch.ptr)
    out.status = L.mdt_op_infonce(C.byref(a), stream())
    torch.cuda.synchronize()
    out.inputs_intact = all(same_bits(x, y) for x, y in zip((img, lang, ls), before))
    out.guards_intact = {k: getattr(out, k).intact() for k in ("loss", "d_img", "d_lang", "d_ls", "scratch")}
    if grads:
        out.result = IC.Result(float(out.loss.region.item()), out.d_img.region.view(B, D).double().cpu(),
                               out.d_lang.region.view(B, D).double().cpu(), float(out.d_ls.region.item()))
    return out


@pytest.mark.parametrize("B,D,mode", DIRECT)
def test_direct_call_stays_inside_its_buffers_and_leaves_its_inputs_alone(lib, B, D, mode):
    """NaN in every float of the scratch and of the outputs before the call: a result that passes read nothing it had not
    written.  Sentinels around the scratch, the scalars and the (B, D) gradients: nothing was written outside them."""
    c, ref = direct_case(B, D, mode)
    r = call_op(lib, c)
    assert r.status == 0, lib.load().mdt_last_error()
    IC.check(r.result, ref, c.id)
    assert all(r.guards_intact.values()), f"wrote outside: {[k for k, ok in r.guards_intact.items() if not ok]}"
    assert r.inputs_intact, "an input changed"


def test_stale_scratch_does_not_reach_the_result(lib):
    """(65, 80), then (17, 48) on the same scratch as the first call left it: bitwise the result of fresh scratch."""
    big, _ = direct_case(65, 80, "symmetric")
    small, ref = direct_case(17, 48, "symmetric")
    first = call_op(lib, big)
    assert first.status == 0
    again = call_op(lib, small, scratch=first.scratch)
    fresh = call_op(lib, small)
    assert again.status == 0 and fresh.status == 0
    IC.check(again.result, ref, small.id)
    for k in ("loss", "d_img", "d_lang", "d_ls"):
        assert same_bits(getattr(again, k).region, getattr(fresh, k).region), k
    assert again.scratch.intact()


@pytest.mark.parametrize("B,D,mode", [(17, 48, "symmetric"), (65, 80, "symmetric"), (63, 16, "text_to_img")])
def test_value_only_call_gives_the_same_loss_and_writes_no_gradient(lib, B, D, mode):
    c, _ = direct_case(B, D, mode)
    full, value = call_op(lib, c), call_op(lib, c, grads=False)
    assert full.status == 0 and value.status == 0
    assert same_bits(full.loss.region, value.loss.region)
    for k in ("d_img", "d_lang", "d_ls"):   # not passed: the canaries stay put
        g = getattr(value, k)
        assert bool((g.region == CANARY).all()) and g.intact(), k
    assert all(value.guards_intact.values()) and value.inputs_intact


@pytest.mark.parametrize("B,D,mode", [(65, 80, "symmetric"), (257, 48, "symmetric")])
def test_a_repeated_call_is_bitwise_equal(lib, B, D, mode):
    """No atomics anywhere in the op and a fixed order in k_pair_sum: two calls, identical bits."""
    c, _ = direct_case(B, D, mode)
    one, two = call_op(lib, c), call_op(lib, c)
    assert one.status == 0 and two.status == 0
    for k in ("loss", "d_img", "d_lang", "d_ls"):
        assert same_bits(getattr(one, k).region, getattr(two, k).region), k


# ------------------------------------------------------------------------------------ the wrapper's conversions (B = 17, D = 48)
WB, WD = 17, 48


def wrapped(img, lang, ls=None, mode="symmetric", grad_img=True, grad_lang=True):
    """clip_auxiliary_loss on detached copies of the given device tensors (layout and dtype kept) -> (loss, img.grad, lang.grad,
    ls.grad)."""
    img, lang = img.detach().requires_grad_(grad_img), lang.detach().requires_grad_(grad_lang)
    ls = torch.tensor(IC.f32(IC.LS_DEFAULT), device="cuda", requires_grad=True) if ls is None else ls
    loss = loss_fn()(img, lang, ls, mode=mode)
    loss.backward()
    return loss.detach(), img.grad, lang.grad, ls.grad


def wrapper_inputs():
    c, ref = direct_case(WB, WD, "symmetric")
    return c.img.cuda(), c.lang.cuda(), ref


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_precision_inputs_are_upcast(dtype):
    img, lang, _ = wrapper_inputs()
    img, lang = img.to(dtype), lang.to(dtype)
    loss, gi, gl, _ = wrapped(img, lang)
    loss32, gi32, gl32, _ = wrapped(img.float(), lang.float())
    assert loss.dtype == torch.float32 and same_bits(loss, loss32)
    assert gi.dtype == dtype and gl.dtype == dtype
    assert torch.equal(gi, gi32.to(dtype)) and torch.equal(gl, gl32.to(dtype))


def test_strided_and_misaligned_views_are_copied():
    img, lang, ref = wrapper_inputs()
    want = wrapped(img, lang)
    img_t, lang_t = img.t().contiguous().t(), lang.t().contiguous().t()          # (B, D) views of (D, B) storage
    assert not img_t.is_contiguous() and torch.equal(img_t, img)
    flat = torch.empty(WB * WD + 1, device="cuda")
    img_m = flat[1:].view(WB, WD).copy_(img)                                       # contiguous, 4 bytes past a 16-byte boundary
    assert img_m.is_contiguous() and img_m.data_ptr() % 16 == 4
    for a, b in ((img_t, lang_t), (img_m, lang), (img, lang_t)):
        got = wrapped(a, b)
        for g, w, what in zip(got, want, ("loss", "d_image", "d_lang", "d_logit_scale")):
            assert same_bits(g, w), what
    IC.check(IC.Result(float(want[0]), want[1].double().cpu(), want[2].double().cpu(), float(want[3])), ref, "B17_D48_symmetric")


def test_a_one_element_parameter_as_logit_scale_gets_a_one_element_gradient():
    img, lang, ref = wrapper_inputs()
    ls = torch.nn.Parameter(torch.full((1,), IC.f32(IC.LS_DEFAULT), device="cuda"))
    loss, _, _, g = wrapped(img, lang, ls=ls)
    assert loss.shape == () and g.shape == (1,)
    assert abs(g.item() - ref.d_scale) <= IC.SCALE_RTOL * abs(ref.d_scale) + IC.SCALE_ATOL


def test_only_lang_requiring_grad_still_gets_its_gradient():
    img, lang, ref = wrapper_inputs()
    ls = torch.tensor(IC.f32(IC.LS_DEFAULT), device="cuda")
    loss, gi, gl, gs = wrapped(img, lang, ls=ls, grad_img=False)
    assert gi is None and gs is None
    full = wrapped(img, lang)
    assert same_bits(loss, full[0]) and same_bits(gl, full[2])
    IC.check(IC.Result(float(loss), ref.d_img, gl.double().cpu(), ref.d_scale), ref, "B17_D48_symmetric")


def test_float64_inputs_are_accepted_and_match_the_float32_path():
    img, lang, _ = wrapper_inputs()
    loss, gi, gl, _ = wrapped(img.double(), lang.double())
    loss32, gi32, gl32, _ = wrapped(img, lang)
    assert same_bits(loss, loss32)
    assert gi.dtype == torch.float64 and torch.equal(gi, gi32.double()) and torch.equal(gl, gl32.double())


def test_shapes_that_are_not_two_equal_matrices_raise():
    img, lang, _ = wrapper_inputs()
    ls = torch.tensor(0.0, device="cuda")
    for a, b in ((img, lang[:-1]), (img, lang[:, :32]), (img[None], lang[None]), (img[0], lang[0]), (img, lang.t())):
        with pytest.raises(ValueError):
            loss_fn()(a, b, ls)
