"""The MAP pooling block at 17 .. 64 tokens: the cases tests/test_cpu_map_long_abi.py, tests/test_map_long_golden.py,
tests/test_gpu_map_long.py and tests/test_gpu_map_long_ops.py run, and tests/golden/make_golden_map_long.py records from the
reference (tests/golden/g22_map_long_<name>.npz).

map_long_lds_bytes restates the LDS rule of the (sample, head group) attention kernels from the text of include/mdt_map_pool.h,
NOT from the library: a shape on which the two disagree is a finding."""


def _m(n_latents, embed_dim, n_heads, output_dim, mlp_ratio, tokens, batches, train_b):
    kw = dict(n_latents=n_latents, embed_dim=embed_dim, n_heads=n_heads, output_dim=output_dim, mlp_ratio=mlp_ratio)
    return dict(kwargs=kw, N=tokens, batches=batches, train_b=train_b)


# name -> constructor kwargs of MAPBlock, tokens per sample, inference batches (1, a mid batch, and for the narrow blocks one with
# at least 8192 token rows), the batch of the training step
MAP_LONG = {
    # the shipped head (ClipStyleProjection('map'): one latent, 16 heads of 24) at the two-camera context: 2 x 16 resampler
    # latents + goal + proprio
    "clip_n34": _m(1, 384, 8, 384, 4.0, 34, [1, 40], 3),
    # the widest single head at the token limit: 2 heads of 256, 16 latents -- the largest K / V slice a workgroup stages
    "q16_hd256_n64": _m(16, 64, 1, 512, 0.5, 64, [1, 9], 2),
    # 64 heads of 8: eight groups of eight heads
    "q16_h64_n64": _m(16, 128, 32, 512, 0.5, 64, [1, 9], 2),
    # the first token count of the kernel pair; head dim 3: slices of 24 channels whose rows take the 16-byte loads while the
    # per-head loops are no multiple of 4; 17 * 482 = 8194 token rows
    "hd3_n17": _m(3, 32, 8, 48, 2.0, 17, [1, 30, 482], 5),
    # head dim 1, an odd token count, five latents; 63 * 131 = 8253 token rows
    "hd1_n63": _m(5, 16, 8, 16, 1.0, 63, [1, 20, 131], 4),
    # the contrastive test's 'map' style at an 18-token context
    "clip_n18": _m(1, 384, 8, 384, 4.0, 18, [1, 12], 3),
}

# recorded from the reference: name -> batch of the fixture
MAP_LONG_GOLDEN = {"clip_n34": 2, "q16_hd256_n64": 2, "q16_h64_n64": 2, "hd3_n17": 3, "hd1_n63": 3}
WEIGHT_SEED, INPUT_SEED, COT_SEED = 221, 222, 223

MAP_LONG_LDS_LIMIT = 160 * 1024   # the LDS of a CU: the rule stays inside it for every accepted shape, so nothing is refused
MAP_TOKEN_LIMIT = 64


def head_group(output_dim, heads):
    """include/mdt_map_pool.h: hg = the largest divisor of H with hg <= 8 and hg * hd <= 128, 1 when there is none."""
    hd = output_dim // heads
    return max([g for g in range(1, 9) if heads % g == 0 and g * hd <= 128] or [1])


def map_long_lds_bytes(n_latents, tokens, output_dim, heads, train):
    """include/mdt_map_pool.h, N 17..64, with heads = 2 * n_heads: W = hg * hd, Wp = W | 1;
    inference 4 (Q W + N Wp + Q hg N), training 4 (2 Q W + N Wp + 2 Q hg N)."""
    hg = head_group(output_dim, heads)
    W = hg * (output_dim // heads)
    k = 2 if train else 1
    return 4 * (k * n_latents * W + tokens * (W | 1) + k * n_latents * hg * tokens)


def map_long_fixture(name):
    """(meta, fixture arrays, params, tokens, cotangent) of a g22 fixture: weights and inputs regenerated from the seeds it names."""
    import torch

    from mdt_policy_amd import synthetic
    from tests.helpers import envelope_params, load_fixture
    meta, fx = load_fixture(f"g22_map_long_{name}.npz")
    P = envelope_params(meta["state_dict"], meta["weight_seed"])
    x = torch.from_numpy(synthetic.normal("ctx", (meta["B"], meta["N"], meta["kwargs"]["embed_dim"]), meta["input_seed"]))
    cot = torch.from_numpy(synthetic.normal("cotangent", tuple(fx["out"].shape), meta["cot_seed"]))
    return meta, fx, P, x, cot
