"""A steered replan driven by a plain C host program (tests/c_client/steer_client.c: mdt_sample_steer with Heun's sampler and K
candidates per observation, no Python / torch in that process): the chunks are the facade's for the same inputs -- both run the
same library code -- and the program's refusal checks of beta = 0 and an unknown kind pass."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from mdt_policy_amd.utils.action_steer import ActionSteer
from tests import test_gpu_guidance as guid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_c_client_steers_heun_as_the_facade_does(tmp_path):
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    B, K, n_steps, beta = 2, 3, 4, 5.0
    exe = tmp_path / "steer_client"
    lib = _lib.library_path()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([shutil.which("gcc") or "gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "c_client", "steer_client.c"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(rocm, "include"), "-o", str(exe), lib, "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-lm", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    model, _ = guid.model_of("mdtv_default")
    cfg = model.inner_model._hip_config(0.5)
    state, goal, _ = guid.inputs("mdtv_default", B, 31)          # per observation
    x_T = guid.inputs("mdtv_default", B * K, 32)[2] * 2.0        # per chunk
    sig = gs.get_sigmas_exponential(n_steps, 0.05, 2.0)
    prev = 0.5 * guid.inputs("mdtv_default", B, 33)[2]           # the previous chunk of every observation
    steer = ActionSteer.overlap(prev, 2, 3, 2, beta=beta, plan_native=True)  # the facade's native route of sample_heun
    known, weight = steer.on("cpu", tuple(x_T.shape), K)         # per chunk, as the entry takes them
    blob = tmp_path / "blob.bin"
    allf = [n for n, _ in _lib.MDTConfig._fields_]
    names = allf[:allf.index("sigma_data")]
    with open(blob, "wb") as f:
        f.write(struct.pack("<i", len(names)))
        f.write(struct.pack(f"<{len(names)}i", *[getattr(cfg, n) for n in names]))
        f.write(struct.pack("<f", 0.5))
        sd = {"inner_model." + k: v_ for k, v_ in model.inner_model.state_dict().items()}
        wanted = list(model.inner_model.hip_engine(0.5).expected)
        f.write(struct.pack("<i", len(wanted)))
        for k in wanted:
            t = sd[k].detach().cpu().float().contiguous().numpy()
            f.write(struct.pack("<i", len(k)) + k.encode() + struct.pack("<q", t.size) + t.tobytes())
        f.write(struct.pack("<iii", B, K, n_steps) + sig.numpy().astype(np.float32).tobytes() + struct.pack("<f", beta))
        f.write(state["state_images"].numpy().tobytes() + goal.numpy().tobytes() + x_T.numpy().tobytes())
        f.write(known.numpy().tobytes() + weight.numpy().tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "gfx950" in r.stdout and f"{K} candidates" in r.stdout and "steered heun" in r.stdout
    got = np.fromfile(out, dtype=np.float32).reshape(tuple(x_T.shape))
    with torch.no_grad():
        want = gs.sample_heun(model, guid.cuda(state), x_T.cuda(), goal.cuda(), sig, extra_args={"steer": steer, "candidates": K})
        plain = gs.sample_heun(model, guid.cuda(state), x_T.cuda(), goal.cuda(), sig, extra_args={"candidates": K})
    np.testing.assert_allclose(got, want.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert float((want - plain).abs().max()) > 1e-2  # ... and the steer moved the chunks
