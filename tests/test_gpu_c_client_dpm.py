"""DPM-Solver-fast and the adaptive DPM-Solver driven by a plain C host program (tests/c_client/dpm_client.c: mdt_sample with the two levels on the host and
mdt_sample_dev with them in device memory, the noise rows in a buffer the program hipMalloc's; mdt_sample_dpm_adaptive) give the actions
GCDenoiser.sample_native('dpm_fast'), gc_sampling.sample_dpm_fast and GCDenoiser.sample_dpm_adaptive_native give on the same
weights, inputs and noise rows."""
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
SIGMA_MAX, SIGMA_MIN = 80.0, 0.001
ORDER = {10: 3, 11: 2}  # the adaptive solver's order run next to each dpm_fast case


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dpm_client") / "dpm_client"
    lib = _lib.library_path()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([shutil.which("gcc") or "gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "c_client", "dpm_client.c"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(rocm, "include"), "-o", str(exe), lib, "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    return exe


@pytest.mark.parametrize("n,eta", [(10, 0.0), (11, 0.0), (11, 0.5)])
def test_c_host_program_runs_dpm_fast_like_the_facade(client, n, eta, tmp_path):
    meta, _ = load_fixture("g1_tiny_mdtv.npz")
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    model = GCDenoiser(cfg_of(meta), 0.5)
    model.load_state_dict(params_of(meta))
    model = model.cuda().eval()
    cfg = model.inner_model._hip_config(0.5)
    state, goal, noise = inputs_of(meta)
    x_T = noise * SIGMA_MAX
    n_noise = n // 3 + 1 if eta else 0  # one row per step: what a device schedule may read
    rows = torch.randn((max(n_noise, 1),) + tuple(x_T.shape), generator=torch.Generator().manual_seed(13))[:n_noise]
    blob = tmp_path / "blob.bin"
    allf = [k for k, _ in _lib.MDTConfig._fields_]
    names = allf[:allf.index("sigma_data")]
    with open(blob, "wb") as f:
        f.write(struct.pack("<i", len(names)))
        f.write(struct.pack(f"<{len(names)}i", *[getattr(cfg, k) for k in names]))
        f.write(struct.pack("<f", 0.5))
        sd = {"inner_model." + k: v for k, v in model.inner_model.state_dict().items()}
        wanted = list(model.inner_model.hip_engine(0.5).expected)
        f.write(struct.pack("<i", len(wanted)))
        for k in wanted:
            t = sd[k].detach().cpu().float().contiguous().numpy()
            f.write(struct.pack("<i", len(k)) + k.encode() + struct.pack("<q", t.size) + t.tobytes())
        f.write(struct.pack("<iiff", x_T.shape[0], n, SIGMA_MAX, SIGMA_MIN))
        f.write(state["state_images"].numpy().tobytes() + goal.numpy().tobytes() + x_T.numpy().tobytes())
        f.write(struct.pack("<ff", eta, 1.0))
        f.write(struct.pack("<i", n_noise) + rows.numpy().astype(np.float32).tobytes())
        ap = _lib.dpm_adaptive_params(order=ORDER[n])
        f.write(struct.pack("<i7d", ap.order, ap.rtol, ap.atol, ap.h_init, ap.pcoeff, ap.icoeff, ap.dcoeff, ap.accept_safety))
    out = tmp_path / "out.bin"
    r = subprocess.run([str(client), str(blob), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "gfx950" in r.stdout
    raw = out.read_bytes()
    nact = x_T.numel()
    got = np.frombuffer(raw[:8 * nact], dtype=np.float32).reshape((2,) + tuple(x_T.shape))
    got_ad = np.frombuffer(raw[8 * nact:12 * nact], dtype=np.float32).reshape(tuple(x_T.shape))
    info_ad = dict(zip(("steps", "nfe", "n_accept", "n_reject"), struct.unpack("<4i", raw[12 * nact:])))
    gstate = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
    nz = rows.cuda() if n_noise else None
    with torch.no_grad():
        want = model.sample_native("dpm_fast", gstate, x_T.cuda(), goal.cuda(), [SIGMA_MAX, SIGMA_MIN], noise=nz, n_steps=n,
                                   eta=eta, s_noise=1.0).cpu().numpy()
        it = iter(list(rows.cuda()))
        loop = gs.sample_dpm_fast(model, gstate, x_T.cuda(), goal.cuda(), SIGMA_MIN, SIGMA_MAX, n, eta=eta,
                                  noise_sampler=lambda s0, s1: next(it), callback=lambda d: None)
    np.testing.assert_array_equal(got[0], want)  # same library, same kernels: bit exact
    np.testing.assert_array_equal(got[0], got[1])  # one device routine builds the plan for both level placements
    np.testing.assert_allclose(got[0], loop.cpu().numpy(), rtol=1e-3, atol=1e-4)
    with torch.no_grad():  # the adaptive solver through the facade: same library, same kernels, same decisions
        want_ad, want_info = model.sample_dpm_adaptive_native(gstate, x_T.cuda(), goal.cuda(), SIGMA_MIN, SIGMA_MAX, order=ORDER[n])
    np.testing.assert_array_equal(got_ad, want_ad.cpu().numpy())
    assert info_ad == want_info
