"""The public face of the replay rings and the learners (CPU): the parameter names and defaults of their public
methods and the names merging_gym exports, pinned so that a change of the classes' internals (shared bases,
moved helpers) cannot move what INTEGRATION.md and README.md document. No GPU: the classes are only inspected."""
import inspect

import pytest

import merging_gym

REQ = inspect.Parameter.empty  # a parameter without a default

EXPORTS = ["MergeEnv", "MergeEnvExtend", "MergeVecEnv", "ReplayRing", "DQNLearner", "RainbowNet", "RainbowReplay",
           "RainbowLearner", "make", "ENV_IDS"]

_SELF = ("self", REQ)
_STORE = [("obs_first", REQ), ("obs", REQ), ("a1", REQ), ("rew", REQ), ("done", None), ("final_obs", None)]
SIGNATURES = {
    "ReplayRing": {
        "__init__": [_SELF, ("capacity", 2000), ("device", None), ("goal", False)],
        "store": [_SELF, *_STORE, ("won_mask", None), ("skip_ego_won", True), ("goal", None), ("next_goal", None),
                  ("reward", None), ("flags", None), ("meta_goal", None)],
        "store_rollout": [_SELF, ("obs_first", REQ), ("traj", REQ), ("skip_ego_won", True), ("goal", None),
                          ("next_goal", None), ("reward", None)],
        "store_meta": [_SELF, ("traj", REQ)],
        "store_transition": [_SELF, ("state", REQ), ("action", REQ), ("reward", REQ), ("next_state", REQ)],
        "sample_rows": [_SELF, ("batch_size", 128), ("seed", 0), ("draw", 0), ("filled_only", False),
                        ("return_index", False)],
        "sample": [_SELF, ("batch_size", 128), ("seed", 0), ("draw", 0), ("filled_only", False)],
    },
    "RainbowReplay": {
        "__init__": [_SELF, ("capacity", 10000), ("device", None)],
        "store": [_SELF, *_STORE, ("flags", None)],
        "store_rollout": [_SELF, ("obs_first", REQ), ("traj", REQ)],
        "push": [_SELF, ("state", REQ), ("action", REQ), ("reward", REQ), ("next_state", REQ), ("done", REQ)],
        "sample_rows": [_SELF, ("batch_size", 32), ("seed", 0), ("draw", 0)],
        "sample": [_SELF, ("batch_size", 32), ("seed", 0), ("draw", 0)],
    },
    "DQNLearner": {
        "__init__": [_SELF, ("net", REQ), ("ring", REQ), ("lr", 0.01), ("gamma", 0.9), ("batch_size", 128),
                     ("target_period", 100), ("betas", (0.9, 0.999)), ("eps", 1e-8), ("seed", 0), ("device", None)],
        "learn": [_SELF, ("num_updates", 1), ("filled_only", False), ("return_loss", False), ("return_rows", False)],
        "load_state_dict": [_SELF, ("sd", REQ)],
    },
    "RainbowLearner": {
        "__init__": [_SELF, ("net", REQ), ("replay", REQ), ("lr", 0.001), ("gamma", 0.99), ("batch_size", 32),
                     ("seed", 0), ("generator", None), ("device", None), ("betas", (0.9, 0.999)), ("eps", 1e-8)],
        "learn": [_SELF, ("num_updates", 1), ("return_loss", False), ("return_rows", False), ("return_proj", False),
                  ("return_grads", False)],
        "sync_target": [_SELF],
        "load_state_dict": [_SELF, ("sd", REQ)],
    },
}
METHODS = [(cls, name) for cls, methods in SIGNATURES.items() for name in methods]


def test_exported_names():
    assert list(merging_gym.__all__) == EXPORTS
    for name in EXPORTS:
        assert getattr(merging_gym, name) is not None


@pytest.mark.parametrize("cls,name", METHODS, ids=[f"{c}.{n}" for c, n in METHODS])
def test_signature(cls, name):
    sig = inspect.signature(getattr(getattr(merging_gym, cls), name))
    got = [(p.name, p.default) for p in sig.parameters.values()]
    assert got == SIGNATURES[cls][name]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
