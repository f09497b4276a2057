"""mdt_op_infonce / mdt_op_infonce_scratch (include/mdt_map_pool.h) as far as they can be seen without a device: what the
call refuses before it touches one -- status and mdt_last_error text per cause, the message naming the entry and the field, as
tests/test_cpu_steer_abi.py does for mdt_sample_ddim_steer -- the scratch size against the carve written out here, and the
tolerances of tests/infonce_cases.py against a float32 run of the oracle: a correct float32 implementation meets each of them
with a factor of ten to spare, so none of the cases is ill-conditioned at the bounds the HIP op is held to
(tests/test_gpu_infonce.py)."""
import ctypes as C
import os
import re

import pytest
import torch

from mdt_policy_amd import _lib
from oracle import cla_oracle as O
from tests import infonce_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mdt_op_infonce"
_BUF = C.create_string_buffer(1 << 16)   # host memory behind every non-null pointer: nothing here is ever launched
PTR = (C.addressof(_BUF) + 15) & ~15
INVALID, UNSUPPORTED = 1, 2


def observe(args=True, **kw):
    """The entry on valid arguments with `kw` replacing fields; pointers are integers or None: no device is needed."""
    f = dict(image_features=PTR, lang_features=PTR, logit_scale=PTR, batch=4, dim=16, mode=0, loss=PTR, d_image=None, d_lang=None,
             d_logit_scale=None, scratch=PTR)
    f.update(kw)
    a = _lib.InfoNCEArgs(**f)
    st = _lib.load().mdt_op_infonce(C.byref(a) if args else None, None)
    return st, _lib.load().mdt_last_error().decode("utf-8", "replace")


# cause -> (fields, status, what the message names)
CAUSES = {
    "null image_features": (dict(image_features=None), INVALID, "image_features"),
    "null lang_features": (dict(lang_features=None), INVALID, "lang_features"),
    "null logit_scale": (dict(logit_scale=None), INVALID, "logit_scale"),
    "null loss": (dict(loss=None), INVALID, "loss"),
    "null scratch": (dict(scratch=None), INVALID, "scratch"),
    "batch 0": (dict(batch=0), INVALID, "batch"),
    "batch -1": (dict(batch=-1), INVALID, "batch"),
    "batch 32769": (dict(batch=32769), INVALID, "batch"),
    "dim 0": (dict(dim=0), UNSUPPORTED, "dim"),
    "dim 8": (dict(dim=8), UNSUPPORTED, "dim"),
    "dim 24": (dict(dim=24), UNSUPPORTED, "dim"),
    "dim -16": (dict(dim=-16), UNSUPPORTED, "dim"),
    "mode -1": (dict(mode=-1), INVALID, "mode"),
    "mode 3": (dict(mode=3), INVALID, "mode"),
    "only d_image": (dict(d_image=PTR), INVALID, "d_image"),
    "only d_lang": (dict(d_lang=PTR), INVALID, "d_lang"),
    "only d_logit_scale": (dict(d_logit_scale=PTR), INVALID, "d_logit_scale"),
    "d_image and d_lang": (dict(d_image=PTR, d_lang=PTR), INVALID, "d_logit_scale"),
    "d_image and d_logit_scale": (dict(d_image=PTR, d_logit_scale=PTR), INVALID, "d_lang"),
    "d_lang and d_logit_scale": (dict(d_lang=PTR, d_logit_scale=PTR), INVALID, "d_image"),
    # what the op's own GEMM calls refuse (mdt_launch_gemm: N, K <= 65536, N * K < 2^30), refused before anything is enqueued
    "dim 65552": (dict(dim=65552), UNSUPPORTED, "dim"),
    "batch 32768 x dim 32768": (dict(batch=32768, dim=32768), UNSUPPORTED, "batch"),
    "batch 32753 x dim 32768": (dict(batch=32753, dim=32768), UNSUPPORTED, "batch"),   # below 2^30 before the padding to 16 rows
}


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_a_refusal_comes_before_any_device_call_and_names_the_entry_and_the_field(cause):
    """(Without a device any HIP call fails: a refusal that came after one would be MDT_ERR_HIP, status 4.)"""
    kw, status, field = CAUSES[cause]
    st, msg = observe(**kw)
    assert st == status and msg.startswith(NAME + ": ") and field in msg, (cause, st, msg)


def test_null_args_are_refused():
    st, msg = observe(args=False)
    assert st == INVALID and msg.startswith(NAME + ": ") and "args" in msg, (st, msg)


def test_the_messages_say_what_was_wrong():
    assert observe(lang_features=None)[1] == NAME + ": null lang_features"
    assert observe(batch=32769)[1] == NAME + ": batch must be 1..32768"
    assert observe(dim=24)[1] == NAME + ": dim must be a multiple of 16"
    assert observe(dim=65552)[1] == NAME + ": dim is 65552, must be at most 65536"
    assert observe(batch=32768, dim=32768)[1] == NAME + ": batch 32768 (padded to a multiple of 16) times dim 32768 must be below 2^30"
    assert observe(mode=3)[1] == NAME + ": invalid mode 3 (symmetric / img_to_text / text_to_img)"
    assert observe(d_lang=PTR)[1] == NAME + ": gradients come together (d_image, d_lang, d_logit_scale) or not at all"


def test_the_largest_sizes_pass_the_size_checks():
    """The size checks refuse no more than the GEMM does: with the largest sizes it takes, the call goes on to the check that
    follows them (the mode's) -- still on the host."""
    for batch, dim in ((16, 65536), (32768, 32752), (32752, 32768), (1, 65536)):
        st, msg = observe(batch=batch, dim=dim, mode=3)
        assert st == INVALID and "invalid mode 3" in msg, (batch, dim, st, msg)


def ceil64(n):
    return (n + 63) // 64 * 64


def carve(B, D):
    """The op's scratch, piece by piece, each rounded up to 64 floats: normalised rows of both sets, the packed weight image
    and both pre-normalisation gradients (Bp x D five times), S and its transpose, the two 1 / norm vectors and the two LSE
    vectors, the per-row (loss, d_logit_scale) partials."""
    Bp = (B + 15) // 16 * 16
    return 5 * ceil64(Bp * D) + 2 * ceil64(Bp * Bp) + 4 * ceil64(Bp) + ceil64(2 * Bp)


SCRATCH_B = (1, 15, 16, 17, 65, 257, 32768)
SCRATCH_D = (16, 48, 384)


def test_the_scratch_size_is_the_carve():
    f = _lib.load().mdt_op_infonce_scratch
    for B in SCRATCH_B:
        for D in SCRATCH_D:
            assert f(B, D) == carve(B, D), (B, D)
    assert carve(1, 16) == 5 * 256 + 2 * 256 + 4 * 64 + 64
    assert carve(32768, 384) > 2 ** 31   # the size is 64-bit


def test_the_scratch_size_refuses_empty_shapes():
    f = _lib.load().mdt_op_infonce_scratch
    for B, D in ((0, 16), (-1, 16), (4, 0), (4, -16), (0, 0)):
        assert f(B, D) == -1, (B, D)


def test_the_scratch_size_never_decreases():
    f = _lib.load().mdt_op_infonce_scratch
    Bs, Ds = sorted(set(SCRATCH_B) | {2, 14, 31, 32, 33, 64, 256}), sorted(set(SCRATCH_D) | {32, 64, 80})
    for D in Ds:
        sizes = [f(B, D) for B in Bs]
        assert sizes == sorted(sizes), (D, sizes)
    for B in Bs:
        sizes = [f(B, D) for D in Ds]
        assert sizes == sorted(sizes), (B, sizes)


def test_the_symbols_are_exported_with_the_headers_prototypes():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_map_pool.h")).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), [" ".join(a.split()) for a in m.group(3).split(",")])
              for m in re.finditer(r"(\w+)\s+(mdt_op_infonce\w*)\s*\(([^)]*)\)\s*;", header)}
    assert protos == {"mdt_op_infonce_scratch": ("int64_t", ["int64_t batch", "int64_t dim"]),
                      "mdt_op_infonce": ("mdt_status", ["const mdt_infonce_args *a", "void *stream"])}
    table = {n: (res, argt) for n, res, argt in _lib.SYMBOLS}
    assert table["mdt_op_infonce_scratch"] == (C.c_int64, [C.c_int64, C.c_int64])
    assert table["mdt_op_infonce"] == (C.c_int32, [C.POINTER(_lib.InfoNCEArgs), C.c_void_p])
    assert C.sizeof(_lib.InfoNCEArgs) == 80
    assert hasattr(_lib.load(), "mdt_op_infonce") and hasattr(_lib.load(), "mdt_op_infonce_scratch")


def test_the_case_list_is_the_one_the_gpu_tests_run():
    ids = [c.id for c in IC.cases()]
    assert ids == list(IC.IDS) and len(set(ids)) == len(ids) == 3 * (len(IC.SHAPES) + len(IC.CASE_NOTES)) == 69
    assert {tuple(c.img.shape) for c in IC.cases() if c.id.startswith("B")} == set(IC.SHAPES)
    assert [B for B, _ in IC.SHAPES] == [2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024, 400]
    assert {D for _, D in IC.SHAPES} == {16, 48, 80}
    for c in IC.cases():
        assert c.img.dtype == c.lang.dtype == torch.float32 and c.img.shape == c.lang.shape
        if not c.id.startswith("B"):
            assert tuple(c.img.shape) == (65, 48)
    z = IC.case("d_zero_rows_symmetric")
    assert not z.img[5].any() and not z.lang[64].any() and z.img[4].any()
    d = IC.case("c_duplicates_symmetric")
    assert torch.equal(d.img[7], d.img[3]) and torch.equal(d.lang[7], d.lang[3]) and torch.equal(d.img[64], d.img[0])
    e = IC.case("e_row_scales_symmetric")
    base = IC.case("B65_D48_symmetric")
    assert 0.9e-6 < float(e.img[0].norm() / base.img[0].norm()) < 1.1e-6 and 0.9e6 < float(e.img[64].norm() / base.img[64].norm()) < 1.1e6
    assert 0.9e6 < float(e.lang[0].norm() / base.lang[0].norm()) < 1.1e6


@pytest.mark.parametrize("cid", IC.IDS + tuple(i for i in IC.DIRECT_IDS if i not in IC.IDS))
def test_a_float32_oracle_meets_a_tenth_of_every_tolerance(cid):
    IC.check(IC.run(O.clip_auxiliary_loss, IC.case(cid), dtype=torch.float32), IC.reference(cid), cid, fraction=0.1)


def test_the_saturated_reference_is_saturated():
    """What the saturated case's own rules rest on: the float64 loss is below 1e-16 and its gradients are far below the bound."""
    for mode in IC.MODES:
        r = IC.reference("g_saturated_" + mode)
        a = IC.reference("a_ceiling_" + mode)
        assert 0 <= r.loss < 1e-16, (mode, r.loss)
        assert float(r.d_img.abs().max()) < 1e-12 * float(a.d_img.abs().max())
        assert float(r.d_lang.abs().max()) < 1e-12 * float(a.d_lang.abs().max())


def test_check_rejects_one_wrong_small_row():
    """The rule this module exists for: an error of 1 % in ONE row whose gradient is tiny beside its neighbours' fails, although
    it is far below 1e-3 of the tensor's largest entry (the rule of tests/test_cla.py)."""
    cid = "e_row_scales_symmetric"
    ref = IC.reference(cid)
    small = int(ref.d_img.abs().amax(dim=1).argmin())
    wrong = ref.d_img.clone()
    wrong[small] *= 1.01
    assert float((wrong - ref.d_img).abs().max()) < 1e-6 * 1e-3 * float(ref.d_img.abs().max())
    IC.check(ref, ref, cid)
    with pytest.raises(AssertionError, match="d_image"):
        IC.check(ref._replace(d_img=wrong), ref, cid)
