"""What the envelope test modules build before their first test: the models, inputs and oracle calls of a table of cases.

``Family`` serves a test_gpu_<family>.py module (a SPEC table of tests/*_configs.py and its ENVELOPE), ``OptionFamily`` a
test_gpu_<family>_options.py module (the sampler options of tests/sampler_envelope.py on a few cases of such a table).  Every
module builds its own instance, and with it its own models: a model carries its workspace, captured graphs and upload versions,
and which call of a test is "the third identical one" depends on who else has called it.

Two weight recipes exist, and stay apart -- recorded fixtures and tolerances rest on each one's exact bits: helpers.params_of(meta)
(rotary buffers recomputed, lang_emb aliased to goal_emb) and helpers.rich_model(cfg) (neither)."""
import torch

from mdt_policy_amd import configs, synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from oracle import mdt_oracle as O
from tests import sampler_envelope as E
from tests.helpers import cfg_of, cuda, inputs_of, observation, params_of, rich_model, to
from tests.test_gpu_sampler_bounds import no_forward


def fixture_meta(arch, factory, ov, **fields):
    """What a golden fixture's meta holds, for tests/helpers.py (cfg_of, params_of, inputs_of) and the helpers built on them."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    sd = GCDenoiser(configs.NAMED[factory](**ov), 0.5).state_dict()
    return dict(config=factory, overrides=ov, arch=arch, modality="lang", profile="rich",
                state_dict=[[k, list(v.shape)] for k, v in sd.items()], **fields)


def on_cuda(cfg, P):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    m = GCDenoiser(cfg, 0.5)
    m.load_state_dict(P)
    return m.cuda().eval()


class Family:
    """The cases of ``envelope`` (name -> cfg, arch, proprio).  With ``spec`` (name -> arch, factory, overrides, proprio) and the
    recorder's ``seeds`` the weights are params_of(meta_of(name)) and model_of gives (model, meta); without them they are
    rich_model's and model_of gives (model, float32 state dict).  ``recorded_obs``: state_obs is drawn at the recorder's obs_seed
    when the inputs are drawn at its input_seed, so that seed gives the recorded inputs."""

    def __init__(self, spec, envelope, seeds=None, recorded_obs=False):
        self.spec, self.envelope, self.seeds, self.recorded_obs = spec, envelope, seeds, recorded_obs
        self._models = {}

    def meta_of(self, name, overrides=None):
        arch, factory, ov, proprio = self.spec[name]
        return fixture_meta(arch, factory, dict(ov, **(overrides or {})), proprio=proprio, B=2, **self.seeds)

    def model_of(self, name):
        """(GCDenoiser on cuda:0 in eval mode, its meta or its float32 state dict) -- 'rich' synthetic weights."""
        if name not in self._models:
            cfg = self.envelope[name]["cfg"]
            if self.spec is None:
                m, P = rich_model(cfg)
                self._models[name] = (m.cuda().eval(), P)
            else:
                meta = self.meta_of(name)
                self._models[name] = (on_cuda(cfg, params_of(meta)), meta)
        return self._models[name]

    def weights(self, name, dtype):
        _, held = self.model_of(name)
        return O.to_dtype(held, dtype) if self.spec is None else params_of(held, dtype)

    def inputs(self, name, B, seed, dtype=torch.float32, cfg=None):
        """(state, goal, noise) on the host; state_obs (B, 1, proprio_dim) when the case switches the token on."""
        e = self.envelope[name]
        obs_seed = self.seeds["obs_seed"] if self.recorded_obs and seed == self.seeds["input_seed"] else None
        return observation(cfg or e["cfg"], e["arch"], e["proprio"], B, seed, dtype, obs_seed)

    def oracle_sample(self, name, B, seed, sig, sampler=O.sample_ddim, state=None):
        e = self.envelope[name]
        st, goal, noise = self.inputs(name, B, seed, torch.float64)
        return sampler(self.weights(name, torch.float64), e["cfg"], state or st, noise * 80.0, goal, sig, arch=e["arch"], hoist=True)

    def hip_sample(self, name, B, seed, sig):
        model, _ = self.model_of(name)
        state, goal, noise = self.inputs(name, B, seed)
        with torch.no_grad():
            return gs.sample_ddim(model, cuda(state), noise.cuda() * 80.0, goal.cuda(), sig.cuda()).cpu()


class OptionFamily:
    """The cases ``spec`` (name -> arch, factory, overrides, proprio) at batch ``B`` with the weights of params_of(meta_of(name));
    ``seeds``: the seed fields of the meta (weight_seed, input_seed and, where the file draws loss inputs, loss_seed, ctx_seed)."""

    def __init__(self, spec, seeds, B=2):
        self.spec, self.seeds, self.B = spec, seeds, B
        self._meta, self._models, self._oracles, self._loops = {}, {}, {}, {}

    def meta_of(self, name):
        if name not in self._meta:
            arch, factory, ov, _ = self.spec[name]
            self._meta[name] = fixture_meta(arch, factory, ov, B=self.B, **self.seeds)
        return self._meta[name]

    def model_of(self, name):
        if name not in self._models:
            meta = self.meta_of(name)
            self._models[name] = on_cuda(cfg_of(meta), params_of(meta))
        return self._models[name]

    def oracle_of(self, name):
        if name not in self._oracles:
            meta = self.meta_of(name)
            self._oracles[name] = E.EnvelopeOracle(name, case=dict(cfg=cfg_of(meta), arch=meta["arch"]), P=params_of(meta))
        return self._oracles[name]

    def case(self, name, batch=None, seed=E.SEED):
        """(state, goal, x_T, fixed noise) in float32 on the host; x_T = 80 noise."""
        state, goal, noise = inputs_of(dict(self.meta_of(name), input_seed=seed), batch=batch or self.B)
        fixed = torch.from_numpy(synthetic.normal("sde_noise", tuple(noise.shape), seed + 100))
        return state, goal, noise * E.SMAX, fixed

    def float64_loop(self, name, kind, extra=None, repeat=1, tag=""):
        """The float64 host loop of one sampler kind, computed once per (name, kind, options) and left unchanged; ``tag`` tells
        apart options the key cannot (objects: only their names are in it)."""
        key = (name, kind, repeat, tag, tuple(sorted((k, v if isinstance(v, float) else "") for k, v in (extra or {}).items())))
        if key not in self._loops:
            state, goal, _, _ = self.case(name)
            _, _, x, fixed = self.case(name, self.B * repeat)
            if repeat > 1:
                state = to(state, lambda v: v.repeat_interleave(repeat, 0))
                goal = goal.repeat_interleave(repeat, 0)
            self._loops[key] = E.run(kind, self.oracle_of(name), E.wide(state), E.wide(x), E.wide(goal), E.wide(fixed), extra_args=dict(extra or {}))
        return self._loops[key]

    def both_runs(self, name, kind, monkeypatch, extra=None, repeat=1, tag=""):
        """(native result, float64 host-loop result) of one sampler kind; ``repeat`` = K: K chunks per observation."""
        want = self.float64_loop(name, kind, extra, repeat, tag)
        state, goal, _, _ = self.case(name)
        _, _, x, fixed = self.case(name, self.B * repeat)
        ea = dict(extra or {})
        if repeat > 1:
            ea["candidates"] = repeat
        with monkeypatch.context() as mp:
            no_forward(mp)
            got = E.run(kind, self.model_of(name), cuda(state), x.cuda(), goal.cuda(), fixed.cuda(), extra_args=ea).cpu()
        return got, want

    def known_of(self, name):
        """Known actions: the negated unpinned float64 DDIM result of another noise seed."""
        key = (name, "known")
        if key not in self._loops:
            state, goal, _, fixed = self.case(name)
            _, _, x_other, _ = self.case(name, seed=E.OTHER_SEED)
            self._loops[key] = -E.run("ddim", self.oracle_of(name), E.wide(state), E.wide(x_other), E.wide(goal), E.wide(fixed))
        return self._loops[key]
