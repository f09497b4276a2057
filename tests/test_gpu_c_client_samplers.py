"""The other samplers driven by a plain C host program (tests/c_client/sampler_client.c: mdt_sample with a host schedule and
mdt_sample_dev with the schedule in device memory, the noise rows in a buffer the program hipMalloc's, params passed as a
struct or as NULL) give the actions GCDenoiser.sample_native gives on the same weights, inputs and noise rows."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from tests.helpers import cfg_of, inputs_of, load_fixture, params_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 5


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sampler_client") / "sampler_client"
    lib = _lib.library_path()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([shutil.which("gcc") or "gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "c_client", "sampler_client.c"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(rocm, "include"), "-o", str(exe), lib, "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    return exe


@pytest.mark.parametrize("kind,params", [("heun", None), ("heun", dict(s_churn=1.0, s_noise=1.01)),
                                         ("euler_ancestral", dict(eta=1.0))])
def test_c_host_program_runs_the_sampler_like_the_facade(client, kind, params, tmp_path):
    meta, _ = load_fixture("g1_tiny_mdtv.npz")
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    model = GCDenoiser(cfg_of(meta), 0.5)
    model.load_state_dict(params_of(meta))
    model = model.cuda().eval()
    cfg = model.inner_model._hip_config(0.5)
    state, goal, noise = inputs_of(meta)
    sig = gs.get_sigmas_karras(N_STEPS, 0.01, 80.0)
    x_T = noise * 80.0
    kw = params or {}
    n_noise = N_STEPS if kind == "heun" else N_STEPS - 1  # the loops' draws: eps every step / one per step with sigma_down > 0
    rows = torch.randn((n_noise,) + tuple(x_T.shape), generator=torch.Generator().manual_seed(11))
    blob = tmp_path / "blob.bin"
    allf = [n for n, _ in _lib.MDTConfig._fields_]
    names = allf[:allf.index("sigma_data")]
    with open(blob, "wb") as f:
        f.write(struct.pack("<i", len(names)))
        f.write(struct.pack(f"<{len(names)}i", *[getattr(cfg, n) for n in names]))
        f.write(struct.pack("<f", 0.5))
        sd = {"inner_model." + k: v for k, v in model.inner_model.state_dict().items()}
        wanted = list(model.inner_model.hip_engine(0.5).expected)
        f.write(struct.pack("<i", len(wanted)))
        for k in wanted:
            t = sd[k].detach().cpu().float().contiguous().numpy()
            f.write(struct.pack("<i", len(k)) + k.encode() + struct.pack("<q", t.size) + t.tobytes())
        f.write(struct.pack("<ii", x_T.shape[0], N_STEPS) + sig.numpy().astype(np.float32).tobytes())
        f.write(state["state_images"].numpy().tobytes() + goal.numpy().tobytes() + x_T.numpy().tobytes())
        f.write(struct.pack("<ii", _lib.SAMPLER_KIND[kind], 0 if params is None else 1))
        if params is not None:
            p = _lib.sampler_params(**kw)
            f.write(struct.pack("<6fi", p.eta, p.s_churn, p.s_tmin, p.s_tmax, p.s_noise, p.r, p.order))
        f.write(struct.pack("<i", n_noise) + rows.numpy().astype(np.float32).tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([str(client), str(blob), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "gfx950" in r.stdout
    got = np.fromfile(out, dtype=np.float32).reshape((2,) + tuple(x_T.shape))
    gstate = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
    with torch.no_grad():
        want_host = model.sample_native(kind, gstate, x_T.cuda(), goal.cuda(), sig, noise=rows.cuda(), **kw).cpu().numpy()
        want_dev = model.sample_native(kind, gstate, x_T.cuda(), goal.cuda(), sig.cuda(), noise=rows.cuda(), **kw).cpu().numpy()
        if params is None:  # deterministic settings: the host loop (forced by a callback) gives the same actions
            loop = getattr(gs, "sample_" + kind)(model, gstate, x_T.cuda(), goal.cuda(), sig, callback=lambda d: None)
            np.testing.assert_allclose(got[0], loop.cpu().numpy(), rtol=1e-3, atol=1e-4)
    np.testing.assert_array_equal(got[0], want_host)  # same library, same kernels: bit exact
    np.testing.assert_array_equal(got[1], want_dev)
    np.testing.assert_array_equal(got[0], got[1])    # one device routine builds the plan for both schedule placements
