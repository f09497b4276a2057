"""Replan-and-select driven by a plain C host program (tests/c_client/candidates_client.c: mdt_sample_ddim_multi with a pin, no
Python / torch in that process): K pinned candidate chunks per observation from one encoded context give what the facade gives
for the same inputs, and the program's refusal check of candidates = 0 passes."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from mdt_policy_amd.utils.action_pin import ActionPin
from tests import test_gpu_guidance as guid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("B,K", [(1, 4), (3, 2)])
def test_plain_c_client_with_candidates_matches_the_facade(B, K, tmp_path):
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    exe = tmp_path / "candidates_client"
    lib = _lib.library_path()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([shutil.which("gcc") or "gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "c_client", "candidates_client.c"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(rocm, "include"), "-o", str(exe), lib, "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-lm", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    model, _ = guid.model_of("mdtv_default")
    cfg = model.inner_model._hip_config(0.5)
    n_steps = 5
    state, goal, _ = guid.inputs("mdtv_default", B, 31)          # per observation
    x_T = guid.inputs("mdtv_default", B * K, 32)[2] * 80.0       # per chunk
    prev = guid.inputs("mdtv_default", B, 33)[2]                 # the chunk each observation is executing
    sig = gs.get_sigmas_exponential(n_steps, 0.01, 80.0)
    pin = ActionPin.overlap(prev, executed=4, hard=2, soft=3)    # per observation: the program gets it expanded, per chunk
    known, keep = pin.on("cpu", x_T.shape, K)
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
        f.write(struct.pack("<iii", B, K, n_steps) + sig.numpy().astype(np.float32).tobytes())
        f.write(state["state_images"].numpy().tobytes() + goal.numpy().tobytes() + x_T.numpy().tobytes())
        f.write(known.numpy().tobytes() + keep.numpy().tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "gfx950" in r.stdout and f"{K} candidates" in r.stdout
    raw = np.fromfile(out, dtype=np.uint8)
    got = raw[:x_T.numel() * 4].view(np.float32).reshape(tuple(x_T.shape))
    pick = raw[x_T.numel() * 4:].view(np.int32)
    with torch.no_grad():
        want = model.sample_ddim(guid.cuda(state), x_T.cuda(), goal.cuda(), sig, pin=pin, candidates=K).cpu()
    assert tuple(model.inner_model.latent_encoder_emb.shape)[0] == B
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got[:, :2], known.numpy()[:, :2], rtol=1e-3, atol=1e-4)  # the hard tokens arrive at the old chunk
    free = (keep == 0).double()
    dist = (((want.double() - known.double()) ** 2) * free).reshape(B, K, -1).sum(-1)
    assert pick.shape == (B,) and all(0 <= int(p) < K for p in pick)
    for b in range(B):  # the program's choice is the closest candidate (to rounding: its distance is within 1e-6 of the least)
        assert float(dist[b, int(pick[b])]) <= float(dist[b].min()) * (1 + 1e-6) + 1e-9
