"""Sample-and-select driven by a plain C host program (tests/c_client/loglik_client.c: mdt_sample_ddim_multi, then
mdt_log_likelihood on its chunks with the caller's probes, no Python / torch in that process): the log-likelihoods are the
facade's for the same chunks and probes -- both run the same library code; only the host loop's double sums could differ, and
they may not -- the program's pick is each observation's argmax, and its refusal checks of candidates = 0 and probes = 0 pass."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from tests import test_gpu_guidance as guid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("B,K", [(1, 4), (3, 2)])
def test_plain_c_client_scores_its_candidates_as_the_facade_does(B, K, tmp_path):
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    exe = tmp_path / "loglik_client"
    lib = _lib.library_path()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([shutil.which("gcc") or "gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "c_client", "loglik_client.c"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(rocm, "include"), "-o", str(exe), lib, "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-lm", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    model, _ = guid.model_of("mdtv_default")
    cfg = model.inner_model._hip_config(0.5)
    n_steps, P, smin, smax = 5, 2, 0.001, 80.0
    state, goal, _ = guid.inputs("mdtv_default", B, 31)          # per observation
    x_T = guid.inputs("mdtv_default", B * K, 32)[2] * 80.0       # per chunk
    sig = gs.get_sigmas_exponential(n_steps, 0.01, 80.0)
    gen = torch.Generator().manual_seed(34)
    v = (torch.randint(0, 2, (P,) + tuple(x_T.shape), generator=gen) * 2 - 1).float()
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
        f.write(struct.pack("<iiii", B, K, P, n_steps) + sig.numpy().astype(np.float32).tobytes() + struct.pack("<ff", smin, smax))
        f.write(state["state_images"].numpy().tobytes() + goal.numpy().tobytes() + x_T.numpy().tobytes() + v.numpy().tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "gfx950" in r.stdout and f"{K} candidates" in r.stdout and f"{P} probes" in r.stdout
    raw = np.fromfile(out, dtype=np.uint8)
    n = x_T.numel() * 4
    got = raw[:n].view(np.float32).reshape(tuple(x_T.shape))
    ll = raw[n:n + B * K * 4].view(np.float32)
    pick = raw[n + B * K * 4:].view(np.int32)
    with torch.no_grad():
        chunks = model.sample_ddim(guid.cuda(state), x_T.cuda(), goal.cuda(), sig, candidates=K)
        np.testing.assert_allclose(got, chunks.cpu().numpy(), rtol=1e-5, atol=1e-6)
        # the facade on the program's own chunks and probes
        want, info = gs.log_likelihood(model, guid.cuda(state), torch.from_numpy(got.copy()).cuda(), goal.cuda(), smin, smax,
                                       extra_args={"candidates": K, "probes": v.cuda()})
    assert info["fevals"] == 2 + 6 * info["steps"] and f"{info['fevals']} evaluations in {info['steps']} steps" in r.stdout
    np.testing.assert_allclose(ll, want.cpu().numpy(), rtol=1e-5, atol=1e-4)
    assert pick.shape == (B,)
    assert pick.tolist() == ll.reshape(B, K).argmax(1).tolist()  # (first maximum: ties to the lowest index, as the program breaks them)
    best, index = gs.best_candidates(torch.from_numpy(got.copy()), torch.from_numpy(ll.copy()), K)
    assert index.tolist() == pick.tolist() and torch.equal(best, torch.from_numpy(got.copy()).reshape(B, K, *got.shape[1:])[torch.arange(B), index])
