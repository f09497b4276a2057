"""mdt_op_linear_bwd -- the backward of every Linear of the project -- at the strides, flags and edges the training step
uses (pytest -m gpu): both accumulate values into NaN-filled / non-zero destinations, bias accumulation, strided operands,
the transposed-copy dW path, argument subsets, the activation backward on the dX epilogue, scratch bounds and reuse, and
refused calls.  Every reference is float64 on the CPU; shapes are far below the workload's (the rows from 8192 on and the
bf16 split form are tests/test_gpu_train_ops.py's)."""
import ctypes as C
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import assert_close
from tests.linear_bwd_shapes import SMALL_SHAPES
from tests.test_gpu_ops import dev, stream
from tests.test_gpu_train_ops import rnd

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 12345.678       # finite: a stale `+=` changes it (NaN would swallow one)
GUARD_BITS = 0x5EA7F00D    # behind the scratch a call may touch


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


# the project's own tolerances: dW / dbias as test_linear_backward_through_the_forward_gemm, dX likewise, the activation
# backward as the aux_mode 2 epilogue in tests/test_gpu_ops.py
def tol_w(M):
    return dict(rtol=1e-3, atol=1e-4 * max(1.0, (M / 64) ** 0.5))


TOL_X = dict(rtol=1e-3, atol=1e-4)
TOL_ACT = dict(rtol=1e-4, atol=2e-4)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def canary(*shape):
    """Fill of an output the call must not touch: NaN in the even elements (an overwrite shows), a finite sentinel in the odd
    ones (an accumulation shows as well)."""
    t = torch.full(shape, NAN)
    t.view(-1)[1::2] = SENTINEL
    return t


def padded(t, ld, col=0):
    """t at columns [col, col + width) of a (rows, ld) device buffer whose other columns hold NaN."""
    buf = torch.full((t.shape[0], ld), NAN)
    buf[:, col:col + t.shape[1]] = t
    return buf.cuda()


def run_linear_bwd(lib, X, W, dY, *, ldx=None, ldy=None, ldxo=None, dW0=None, db0=None, dX0=None, acc_dw=0, acc_dx=0,
                   want=("dW", "db", "dX"), act_u=None, act=0, scratch_fill=NAN, guard=1024, dy_col=0, pass_wt=True,
                   scratch_floats=None):
    """One mdt_op_linear_bwd call.  X (M, K), dY (M, N), the dX destination and act_u sit in device buffers of row stride ldx /
    ldy / ldxo whose padding columns hold NaN (dY at column dy_col of its buffer).  All three destinations exist whatever `want`
    names; only those it names are passed.  One that is passed starts as dW0 / db0 / dX0, or NaN where none is given; one that is
    not passed starts as a canary().  Scratch: mdt_op_linear_bwd_scratch_exact floats (or scratch_floats) of scratch_fill, then
    `guard` floats of GUARD_BITS.  Returns the status, the destinations, their initial values, dX's padding columns, the scratch
    and the guard, all on the CPU."""
    L = lib.load()
    (M, K), N = X.shape, dY.shape[1]
    wx = K if act_u is None else act_u.shape[1]          # SwishGLU: u and dX have 2 K columns
    ldx, ldy, ldxo = ldx or K, ldy or N, ldxo or wx
    pitch = max(ldxo, wx)                                # (a refused ldxo < wx: the buffers still hold whole rows)
    Xd, dYd = padded(X, ldx), padded(dY, ldy, dy_col)

    def start(name, given, *shape):
        return given.clone() if given is not None else (torch.full(shape, NAN) if name in want else canary(*shape))
    init = dict(dW=start("dW", dW0, N, K), db=start("db", db0, N), dX=start("dX", dX0, M, wx))
    dWd, dbd, dXd = dev(init["dW"]), dev(init["db"]), padded(init["dX"], pitch)
    ud = padded(act_u, pitch) if act_u is not None else None
    Wt = None
    if "dX" in want and pass_wt:
        Wt = torch.zeros(N * K, device="cuda")           # (shapes the packer refuses are refused by the call under test too)
        if W is not None and N % 16 == 0 and K % 16 == 0:
            lib.check(L.mdt_op_pack_weight_t(dev(W).data_ptr(), N, K, K, Wt.data_ptr(), 0, N, stream()))
    n = scratch_floats or L.mdt_op_linear_bwd_scratch_exact(M, N, K)
    scratch = torch.empty(n + guard, device="cuda")
    scratch[:n] = scratch_fill
    scratch[n:].view(torch.int32).fill_(GUARD_BITS)
    a = lib.LinearBwdArgs(X=Xd.data_ptr(), ldx=ldx, dY=dYd.data_ptr() + 4 * dy_col, ldy=ldy,
                          Wt=Wt.data_ptr() if Wt is not None else None,
                          dW=dWd.data_ptr() if "dW" in want else None, dbias=dbd.data_ptr() if "db" in want else None,
                          dX=dXd.data_ptr() if "dX" in want else None, ldxo=ldxo, accumulate_dw=acc_dw, accumulate_dx=acc_dx,
                          M=M, N=N, K=K, scratch=scratch.data_ptr(), dx_act_u=ud.data_ptr() if ud is not None else None,
                          dx_act=act)
    status = L.mdt_op_linear_bwd(C.byref(a), stream())
    torch.cuda.synchronize()
    return types.SimpleNamespace(status=status, dW=dWd.cpu(), db=dbd.cpu(), dX=dXd[:, :wx].cpu(), dX_pad=dXd[:, wx:].cpu(),
                                 scratch=scratch[:n].cpu(), guard=scratch[n:].cpu(), init=init, want=want)


def check_bounds(r, what=""):
    """Accepted, nothing written behind the exact scratch, into dX's padding columns or into a destination that was not passed."""
    assert r.status == 0, f"{what}: status {r.status}"
    assert bool((r.guard.view(torch.int32) == GUARD_BITS).all()), f"{what}: wrote behind mdt_op_linear_bwd_scratch_exact floats"
    assert bool(r.dX_pad.isnan().all()), f"{what}: wrote into the padding columns of dX"
    for name in ("dW", "db", "dX"):
        if name not in r.want:
            assert same_bits(getattr(r, name), r.init[name]), f"{what}: {name} was not passed and changed"


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    """Inputs of order one as in test_linear_backward_through_the_forward_gemm, and their float64 gradients (shared: never
    written to)."""
    X, W, dY = rnd(M, K, seed=41), rnd(N, K, seed=42) / K ** 0.5, rnd(M, N, seed=43)
    ref = dict(dW=dY.double().T @ X.double(), db=dY.double().sum(0), dX=dY.double() @ W.double())
    return X, W, dY, ref


def starts(M, N, K, wx=None):
    return dict(dW0=rnd(N, K, seed=44), db0=rnd(N, seed=46), dX0=rnd(M, wx or K, seed=45))


def check_against_float64(r, ref, M, acc_dw, acc_dx, what, tol_x=TOL_X):
    """The wanted destinations of an accepted call against float64; an accumulating call against float64 plus what it started from."""
    check_bounds(r, what)
    for name, acc, tol in (("dW", acc_dw, tol_w(M)), ("db", acc_dw, tol_w(M)), ("dX", acc_dx, tol_x)):
        if name in r.want:
            got = getattr(r, name).double() - (r.init[name].double() if acc else 0.0)
            assert_close(got, ref[name], what=f"{what}: {name} (accumulate {acc})", **tol)


def tn_slices_written(r, N, K):
    """Slices the straight (k_gemm_tn) path cut the rows into, read off a NaN-filled scratch after a call with dW and dbias: it
    writes S (N, K) partial products (only when S > 1: a single slice goes to dW itself) and S rows of N bias partials."""
    written = int((~r.scratch.isnan()).sum())
    if written == N:
        return 1
    assert written % (N * K + N) == 0, f"{written} floats of scratch written: not S x (N K + N)"
    return written // (N * K + N)


# M_EDGES, N_EDGES, K_EDGES, MANY_SLICES: (M, N, K, S) with S = the slices the straight path cuts M rows into, worked out by hand
# (tests/linear_bwd_shapes.py).  mdt_op_linear_bwd_scratch_exact cannot confirm them -- at every shape there the transposed-copy
# path's need is the larger -- so this test reads S off the scratch (tn_slices_written); the route table
# (tests/c_client/route_table.cpp, the lin_bwd/ keys; tests/test_route_table.py) pins the plan's S, kernel and scratch layout for
# the same shapes without a GPU.


@pytest.mark.parametrize("M,N,K,S", SMALL_SHAPES)
def test_dw_small_shapes_against_float64(lib, M, N, K, S):
    """k_gemm_tn below 8192 rows and the sum of its slices: overwrite into NaN-filled dW / dbias with NaN-filled scratch (an
    overwrite path that reads its destination, or a slice it never wrote, gives NaN), then accumulation onto non-zero dW AND
    non-zero dbias."""
    X, W, dY, ref = case(M, N, K)
    r = run_linear_bwd(lib, X, W, dY, want=("dW", "db"), acc_dw=0)
    assert tn_slices_written(r, N, K) == S
    check_against_float64(r, ref, M, 0, 0, "overwrite")
    s = starts(M, N, K)
    r = run_linear_bwd(lib, X, W, dY, want=("dW", "db"), acc_dw=1, dW0=s["dW0"], db0=s["db0"])
    check_against_float64(r, ref, M, 1, 0, "accumulate")


@pytest.mark.parametrize("M,N,K,S", SMALL_SHAPES)
def test_strided_operands_give_the_bits_of_contiguous_ones(lib, M, N, K, S):
    """ldx = K + 4, ldy = N + 8, ldxo = K + 12 with NaN between the rows: the same kernels, the same order of the additions, other
    addresses -- dW, dbias and dX bit for bit those of the contiguous call, dX's padding still NaN."""
    X, W, dY, _ = case(M, N, K)
    for acc in (0, 1):
        s = starts(M, N, K) if acc else {}
        flat = run_linear_bwd(lib, X, W, dY, acc_dw=acc, acc_dx=acc, **s)
        wide = run_linear_bwd(lib, X, W, dY, acc_dw=acc, acc_dx=acc, ldx=K + 4, ldy=N + 8, ldxo=K + 12, **s)
        check_bounds(flat, "contiguous")
        check_bounds(wide, "strided")
        assert not bool(flat.dW.isnan().any() | flat.db.isnan().any() | flat.dX.isnan().any())
        for name in ("dW", "db", "dX"):
            assert same_bits(getattr(wide, name), getattr(flat, name)), f"{name} (accumulate {acc}) differs from the contiguous call's"


def test_dy_as_the_middle_third_of_a_qkv_buffer(lib):
    """ldy = 3 N, dY the middle third of its rows (the other two thirds NaN): the bits of the contiguous call, and float64."""
    M, N, K = 300, 64, 128
    X, W, dY, ref = case(M, N, K)
    flat = run_linear_bwd(lib, X, W, dY)
    qkv = run_linear_bwd(lib, X, W, dY, ldy=3 * N, dy_col=N)
    check_against_float64(qkv, ref, M, 0, 0, "qkv layout")
    for name in ("dW", "db", "dX"):
        assert same_bits(getattr(qkv, name), getattr(flat, name)), f"{name} differs from the contiguous call's"


# (M, N, K, S, L): split_rows' slices, by hand from the host code
TRANSPOSED_SHAPES = [(37, 64, 128, 1, 64),        # one slice, 27 pad rows
                     (130, 48, 80, 1, 160),
                     (2500, 64, 128, 2, 1280),    # two slices, the last of 1220 rows
                     (4100, 16, 16, 8, 544)]      # above the 4096 switch of the slice depth: 8 slices, the last of 292 rows


@pytest.mark.parametrize("strides", ["ldx=K+1", "ldy=N+2"])
@pytest.mark.parametrize("M,N,K,S,L", TRANSPOSED_SHAPES)
def test_transposed_copy_path_against_float64(lib, M, N, K, S, L, strides):
    """A row stride that is no multiple of 4 floats sends dW through transposed copies, a packed image and the batched forward
    GEMM: its own slice split, pad-row zeroing, scratch layout and bias partials, all out of NaN-filled scratch.  Against float64
    and against k_gemm_tn on contiguous copies of the same data (another order of the additions: float64's tolerance, not bits)."""
    X, W, dY, ref = case(M, N, K)
    ld = dict(ldx=K + 1) if strides == "ldx=K+1" else dict(ldy=N + 2)
    s = starts(M, N, K)
    for acc in (0, 1):  # overwrite into NaN-filled dW / dbias, then accumulate onto non-zero dW and non-zero dbias
        kw = dict(want=("dW", "db"), acc_dw=acc, dW0=s["dW0"] if acc else None, db0=s["db0"] if acc else None)
        r = run_linear_bwd(lib, X, W, dY, **ld, **kw)
        check_against_float64(r, ref, M, acc, 0, f"transposed copies ({strides})")
        if not acc:  # the path that ran, by what it left in the scratch: both operands' copies, partial products, bias partials
            assert int((~r.scratch.isnan()).sum()) == (N + K) * S * L + (S * N * K if S > 1 else 0) + (M + 31) // 32 * N
        tn = run_linear_bwd(lib, X, W, dY, **kw)
        check_bounds(tn)
        assert_close(r.dW, tn.dW, what="dW against k_gemm_tn's", **tol_w(M))
        assert_close(r.db, tn.db, what="dbias against k_gemm_tn's", **tol_w(M))


@pytest.mark.parametrize("acc", [0, 1])
def test_argument_subsets(lib, acc):
    """Bias only (the column-sum route), dW without dbias, dX only (what the denoiser's VJP asks for): each against float64, and
    the destinations that were not passed left as they were."""
    M, N, K = 250, 96, 80
    X, W, dY, ref = case(M, N, K)
    s = starts(M, N, K) if acc else {}
    pick = lambda *names: {k: v for k, v in s.items() if k[:2] in names}
    r = run_linear_bwd(lib, X, W, dY, want=("db",), acc_dw=acc, **pick("db"))
    check_against_float64(r, ref, M, acc, acc, "bias only")
    r = run_linear_bwd(lib, X, W, dY, want=("dW",), acc_dw=acc, **pick("dW"))
    check_against_float64(r, ref, M, acc, acc, "dW only")
    r = run_linear_bwd(lib, X, W, dY, want=("dX",), acc_dx=acc, **pick("dX"))
    check_against_float64(r, ref, M, acc, acc, "dX only")
    r = run_linear_bwd(lib, X, W, dY, want=("dW", "dX"), acc_dw=acc, acc_dx=acc, ldxo=K + 12, **pick("dW", "dX"))
    check_against_float64(r, ref, M, acc, acc, "dW and dX, no dbias")
    for n in (7, 100):  # N % 16 != 0: no dW, no dX, but the bias gradient of any width; ldy = N + 1
        dY = rnd(M, n, seed=47)
        r = run_linear_bwd(lib, X, None, dY, want=("db",), acc_dw=acc, ldy=n + 1, db0=rnd(n, seed=48) if acc else None)
        check_against_float64(r, dict(db=dY.double().sum(0)), M, acc, acc, f"bias only, N = {n}")


ACTS = {"gelu": F.gelu, "mish": F.mish, "silu": F.silu}


@pytest.mark.parametrize("M,N,K", [(70, 256, 128), (300, 512, 384), (1, 16, 16)])
@pytest.mark.parametrize("act", sorted(ACTS))
def test_input_gradient_with_the_activation_backward(lib, act, M, N, K):
    """dx_act_u / dx_act: dX = (dY W) * act'(u) on the product's epilogue, overwritten into NaN-filled dX, against float64
    autograd; contiguous and with ldxo = K + 12 (u shares dX's stride); dW and dbias of the same call as ever."""
    X, W, dY, ref = case(M, N, K)
    u = rnd(M, K, seed=49)
    u64 = u.double().requires_grad_()
    ACTS[act](u64).backward(ref["dX"])
    ref = dict(ref, dX=u64.grad)
    for ldxo in (K, K + 12):
        r = run_linear_bwd(lib, X, W, dY, act_u=u, act=lib.ACT[act], ldxo=ldxo)
        check_against_float64(r, ref, M, 0, 0, f"{act}, ldxo = {ldxo}", tol_x=TOL_ACT)


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("M,N,K", [(37, 48, 64), (306, 192, 192)])
def test_input_gradient_with_the_swiglu_backward(lib, M, N, K, pad):
    """MDT_ACT_SWIGLU: u = [p | g] and dX (M, 2 K; ldxo = 2 K + pad); dX = [d silu(g) | d p silu'(g)] with d = dY W."""
    X, W, dY, ref = case(M, N, K)
    u = rnd(M, 2 * K, seed=50)
    u64 = u.double().requires_grad_()
    (u64[:, :K] * F.silu(u64[:, K:])).backward(ref["dX"])
    r = run_linear_bwd(lib, X, W, dY, act_u=u, act=lib.ACT["swiglu"], ldxo=2 * K + pad)
    check_against_float64(r, dict(ref, dX=u64.grad), M, 0, 0, f"swiglu, ldxo = 2 K + {pad}", tol_x=TOL_ACT)


@pytest.mark.parametrize("M,N,K,ld", [(1000, 80, 208, {}),             # k_gemm_tn, 7 slices
                                      (300, 64, 576, {}),              # KT = 3
                                      (130, 48, 80, dict(ldx=81))])    # transposed copies
def test_scratch_bounds_and_stale_contents(lib, M, N, K, ld):
    """One scratch serves every Linear of a training loop: whatever it holds when a call starts, and however much larger than
    this call's need it is, the results are the same bits -- as are those of a second call (the header promises determinism) --,
    and nothing is written behind mdt_op_linear_bwd_scratch_exact floats."""
    X, W, dY, ref = case(M, N, K)
    s = starts(M, N, K)
    run = lambda **kw: run_linear_bwd(lib, X, W, dY, acc_dw=1, acc_dx=1, **s, **ld, **kw)
    first = run()
    check_against_float64(first, ref, M, 1, 1, "NaN-filled scratch")
    others = {"a second call": run(), "scratch filled with 1e30": run(scratch_fill=1e30),
              "scratch sized for 4 M rows": run(scratch_floats=lib.load().mdt_op_linear_bwd_scratch(4 * M, N, K))}
    for what, r in others.items():
        check_bounds(r, what)
        for name in ("dW", "db", "dX"):
            assert same_bits(getattr(r, name), getattr(first, name)), f"{name}: {what} gives other bits"


REFUSED = {"dW with N % 16 != 0": dict(shape=(50, 40, 64)),
           "dX without Wt": dict(shape=(50, 64, 64), pass_wt=False),
           "dx_act_u with accumulate_dx": dict(shape=(50, 64, 64), act="gelu", acc_dx=1),
           "dx_act_u with N > 512": dict(shape=(50, 528, 64), act="gelu"),
           "SwishGLU with ldxo < 2 K": dict(shape=(50, 64, 64), act="swiglu", ldxo=2 * 64 - 4),
           "K % 16 != 0": dict(shape=(50, 64, 24))}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_refused_calls_write_nothing(lib, why):
    """A call refused for its arguments has enqueued nothing: dW, dbias and dX keep their bits, so a caller that corrects the
    arguments and calls again counts no gradient twice."""
    kw = dict(REFUSED[why])
    M, N, K = kw.pop("shape")
    act = kw.pop("act", None)
    wx = 2 * K if act == "swiglu" else K
    X, W, dY = rnd(M, K, seed=41), rnd(N, K, seed=42) / K ** 0.5, rnd(M, N, seed=43)
    full = lambda *shape: torch.full(shape, SENTINEL)
    r = run_linear_bwd(lib, X, W, dY, acc_dw=1, dW0=full(N, K), db0=full(N), dX0=full(M, wx),
                       act_u=rnd(M, wx, seed=49) if act else None, act=lib.ACT[act] if act else 0, **kw)
    assert r.status != 0, "accepted"
    for name in ("dW", "db", "dX"):
        assert same_bits(getattr(r, name), r.init[name]), f"{name} was written before the call was refused"
    assert bool((r.guard.view(torch.int32) == GUARD_BITS).all()) and bool(r.dX_pad.isnan().all())
