#!/usr/bin/env python3
"""Record the reference's MAPBlock at 17 .. 64 tokens: tests/golden/g22_map_long_<name>.npz for the cases of
tests/map_long_configs.py named in MAP_LONG_GOLDEN.

Runs ONLY where the reference checkout exists, like make_golden.py, whose helpers it imports unchanged (the import stubs, the
gradient summaries, save_fixed); no test imports this file.

    python tests/golden/make_golden_map_long.py

Each fixture holds what the g18_map_* fixtures hold, with 'rich' weights: the block's output, d(x) in full, every parameter's
gradient summary (l2 norm, sum, first 6 entries) and the reference's state_dict names and shapes.  Weights, inputs and the
cotangent are not stored: the tests regenerate them from mdt_policy_amd/synthetic.py.  The script also prints, per case, how far the
reference's float32 results lie from the float64 oracle's (the figure the tests' gates are judged against)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as MG  # noqa: E402
from mdt_policy_amd import synthetic  # noqa: E402
from tests.map_long_configs import COT_SEED, INPUT_SEED, MAP_LONG, MAP_LONG_GOLDEN, WEIGHT_SEED  # noqa: E402


def record(name):
    from mdt.models.networks.transformers.transformer_blocks import MAPBlock
    from oracle import cla_oracle as CO
    c, B = MAP_LONG[name], MAP_LONG_GOLDEN[name]
    kw, N = c["kwargs"], c["N"]
    assert N > 16
    m = MAPBlock(**kw)
    sd = m.state_dict()
    new = synthetic.fill_state_dict([(k, tuple(v.shape)) for k, v in sd.items()], WEIGHT_SEED, "rich")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()}, strict=True)
    x = torch.from_numpy(synthetic.normal("ctx", (B, N, kw["embed_dim"]), INPUT_SEED)).requires_grad_()
    out = m(x)
    cot = torch.from_numpy(synthetic.normal("cotangent", tuple(out.shape), COT_SEED))
    (out * cot).sum().backward()
    meta = dict(kwargs=kw, B=B, N=N, weight_seed=WEIGHT_SEED, input_seed=INPUT_SEED, cot_seed=COT_SEED, profile="rich",
                grads=MG._grad_summaries(m), state_dict=[[k, list(v.shape)] for k, v in sd.items()])
    MG.save_fixed(f"g22_map_long_{name}.npz", meta, out=out.detach().numpy(), d_x=x.grad.numpy())
    # float32 reference against the float64 oracle, as a fraction of each tensor's largest entry
    P64 = {k: torch.from_numpy(v).double().requires_grad_() for k, v in new.items()}
    x64 = x.detach().double().requires_grad_()
    o64 = CO.map_block(P64, "", x64, kw["n_heads"])
    (o64 * cot.double()).sum().backward()
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())  # noqa: E731
    worst = max([rel(out.detach().reshape(o64.shape), o64.detach()), rel(x.grad, x64.grad)]
                + [rel(p.grad, P64[k].grad) for k, p in m.named_parameters()])
    print(f"  {name}: fp32 reference vs fp64 oracle, worst tensor {worst:.2e} of its largest entry")


if __name__ == "__main__":
    assert os.path.isdir(MG.REF), f"{MG.REF} not found: the recorder runs only beside the reference checkout"
    MG.install_stubs()
    torch.manual_seed(0)
    for case in sys.argv[1:] or MAP_LONG_GOLDEN:
        record(case)
