"""Sample-and-select driven by a plain C host program, forwards only (tests/c_client/score_client.c: mdt_sample_ddim_multi, then
mdt_denoising_score on its chunks with the caller's levels and noise rows, no Python / torch in that process): the scores are the
facade's bits for the same chunks, levels and rows -- both run the same library code in one fixed order --, the program's pick is
each observation's argmax and best_candidates', and its refusal checks of candidates = 0, draws = 0 and n_levels = 65 pass."""
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
    exe = tmp_path / "score_client"
    lib = _lib.library_path()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([shutil.which("gcc") or "gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "c_client", "score_client.c"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(rocm, "include"), "-o", str(exe), lib, "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-lm", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    model, _ = guid.model_of("mdtv_default")
    cfg = model.inner_model._hip_config(0.5)
    n_steps, S, M = 5, 4, 2
    state, goal, _ = guid.inputs("mdtv_default", B, 41)          # per observation
    x_T = guid.inputs("mdtv_default", B * K, 42)[2] * 80.0       # per chunk
    sig = gs.get_sigmas_exponential(n_steps, 0.01, 80.0)
    levels = np.exp(np.linspace(np.log(80.0), np.log(0.001), S)).astype(np.float32)
    noise = torch.randn((S, M) + tuple(x_T.shape[1:]), generator=torch.Generator().manual_seed(44))
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
        f.write(struct.pack("<iiiii", B, K, S, M, n_steps) + sig.numpy().astype(np.float32).tobytes() + levels.tobytes())
        f.write(state["state_images"].numpy().tobytes() + goal.numpy().tobytes() + x_T.numpy().tobytes() + noise.numpy().tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "gfx950" in r.stdout and f"{K} candidates" in r.stdout and f"{S} levels, {M} draws" in r.stdout
    raw = np.fromfile(out, dtype=np.uint8)
    n = x_T.numel() * 4
    got = raw[:n].view(np.float32).reshape(tuple(x_T.shape))
    score = raw[n:n + B * K * 4].view(np.float32)
    pick = raw[n + B * K * 4:].view(np.int32)
    with torch.no_grad():
        chunks = model.sample_ddim(guid.cuda(state), x_T.cuda(), goal.cuda(), sig, candidates=K)
        np.testing.assert_allclose(got, chunks.cpu().numpy(), rtol=1e-5, atol=1e-6)
        # the facade on the program's own chunks, levels and noise rows
        want = gs.denoising_score(model, guid.cuda(state), torch.from_numpy(got.copy()).cuda(), goal.cuda(), [float(v) for v in levels],
                                  extra_args={"candidates": K}, noise=noise.cuda())
    want = want.cpu().numpy()
    print(f"B={B} K={K}: scores {score.tolist()}")
    assert np.isfinite(score).all() and (score < 0).all()
    assert np.array_equal(score.view(np.int32), want.view(np.int32)), (score.tolist(), want.tolist())
    assert pick.shape == (B,)
    assert pick.tolist() == score.reshape(B, K).argmax(1).tolist()  # (first maximum: ties to the lowest index, as the program breaks them)
    best, index = gs.best_candidates(torch.from_numpy(got.copy()), torch.from_numpy(score.copy()), K)
    assert index.tolist() == pick.tolist() and torch.equal(best, torch.from_numpy(got.copy()).reshape(B, K, *got.shape[1:])[torch.arange(B), index])
