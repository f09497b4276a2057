"""Sample, score and select driven by a plain C host program as ONE call (tests/c_client/select_client.c: mdt_sample_ddim_select
with the caller's levels and noise rows, no Python / torch in that process): the program's index, chosen chunk, scores and
candidates are the facade's bits for the same inputs -- both run the same library code in one fixed order --, its printed lines
name the facade's index, and its refusal checks of a NULL select, select.size = 8, a NULL select.index and n_levels = 65 pass."""
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


@pytest.mark.parametrize("B,K", [(1, 8), (3, 2)])
def test_plain_c_client_selects_what_the_facade_selects(B, K, tmp_path):
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    exe = tmp_path / "select_client"
    lib = _lib.library_path()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([shutil.which("gcc") or "gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "c_client", "select_client.c"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(rocm, "include"), "-o", str(exe), lib, "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-lm", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    model, _ = guid.model_of("mdtv_default")
    cfg = model.inner_model._hip_config(0.5)
    n_steps, S, M = 5, 4, 2
    state, goal, _ = guid.inputs("mdtv_default", B, 51)          # per observation
    x_T = guid.inputs("mdtv_default", B * K, 52)[2] * 80.0       # per chunk
    sig = gs.get_sigmas_exponential(n_steps, 0.01, 80.0)
    levels = np.exp(np.linspace(np.log(80.0), np.log(0.001), S)).astype(np.float32)
    noise = torch.randn((S, M) + tuple(x_T.shape[1:]), generator=torch.Generator().manual_seed(54))
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
    per = int(np.prod(x_T.shape[1:]))
    cuts = np.cumsum([0, 4 * B, 4 * B * per, 4 * B * K, 4 * B * K * per])
    assert raw.size == cuts[-1]
    pick = raw[cuts[0]:cuts[1]].view(np.int32)
    best, score, chunks = (raw[cuts[i]:cuts[i + 1]].view(np.int32) for i in (1, 2, 3))
    with torch.no_grad():
        want = gs.sample_select(model, guid.cuda(state), x_T.cuda(), goal.cuda(), sig, [float(v) for v in levels], noise=noise.cuda(),
                                extra_args={"candidates": K})
    wbest, windex, wscore, wchunks = (t.cpu().numpy() for t in want)
    print(r.stdout)
    assert pick.tolist() == windex.tolist()
    assert np.array_equal(best, wbest.reshape(-1).view(np.int32)), "the chosen chunks"
    assert np.array_equal(score, wscore.reshape(-1).view(np.int32)), "the scores"
    assert np.array_equal(chunks, wchunks.reshape(-1).view(np.int32)), "the candidates"
    for b in range(B):
        assert f"observation {b}: candidate {int(windex[b])}," in r.stdout
