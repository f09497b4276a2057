"""world_size-2 gloo test (CPU) of the batch-sharded sampling path with a goal of three tokens, in the style of
tests/test_sharding_gloo.py: a (B, 3, goal_dim) goal shards along the batch with the state and the noise, every rank's slice keeps
its three rows per sample, and the gathered result is the unsharded one.  The per-rank 'sampler' is the CPU oracle -- only the
sharding / collective logic is under test."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mdt_policy_amd import sharding


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, total, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mdt_policy_amd import configs
        from oracle import mdt_oracle as O
        from tests.helpers import cfg_of, inputs_of, params_of
        from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
        ov = dict(goal_seq_len=3)
        sd = GCDenoiser(configs.mdtv_tiny(**ov), 0.5).state_dict()
        meta = dict(config="mdtv_tiny", overrides=ov, arch="mdtv", B=total, modality="lang", weight_seed=11, profile="rich", input_seed=5,
                    state_dict=[[k, list(v.shape)] for k, v in sd.items()])
        cfg, P = cfg_of(meta), params_of(meta)
        state, goal, noise = inputs_of(meta)
        assert tuple(goal.shape) == (total, 3, cfg["goal_dim"])
        sig = O.get_sigmas_exponential(2, 0.01, 80.0)
        lo, hi = sharding.shard_bounds(total, rank, world)
        seen = []

        def fn(s, x, g, sg):
            seen.append(tuple(g.shape))
            return O.sample_ddim(P, cfg, s, x, g, sg, hoist=True)

        full = fn(state, noise * 80.0, goal, sig)
        got = sharding.sample_sharded(fn, state, noise * 80.0, goal, sig)
        local = sharding.sample_sharded(fn, state, noise * 80.0, goal, sig, gather=False)
        ok = (got.shape == full.shape and torch.allclose(got, full, rtol=1e-5, atol=1e-6)
              and torch.allclose(local, full[lo:hi], rtol=1e-5, atol=1e-6)
              and seen == [(total, 3, cfg["goal_dim"])] + 2 * [(hi - lo, 3, cfg["goal_dim"])])
        # the rows of sample b stay with sample b: another goal in one sample of the OTHER rank's slice leaves this rank's slice alone
        other = goal.clone()
        olo, ohi = sharding.shard_bounds(total, 1 - rank, world)
        other[olo, 2] += 1.0
        ok = ok and torch.equal(sharding.sample_sharded(fn, state, noise * 80.0, other, sig, gather=False), local)
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("total", [8, 7])
def test_sample_sharded_world2_gloo_with_a_goal_of_three_tokens(total):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, total, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    res = dict(q.get(timeout=5) for _ in range(2))
    assert res == {0: True, 1: True}


def test_a_three_token_goal_is_sliced_along_the_batch():
    """One process: the slice helper leaves dimension 1 of the goal alone."""
    goal = torch.arange(4 * 3 * 2, dtype=torch.float32).reshape(4, 3, 2)
    fn = lambda s, x, g, sg: g.sum(dim=(1, 2)).reshape(-1, 1, 1) * torch.ones_like(x)
    x = torch.zeros(4, 2, 1)
    assert torch.equal(sharding.sample_sharded(fn, {"modality": "lang"}, x, goal, None)[:, 0, 0], goal.sum(dim=(1, 2)))
