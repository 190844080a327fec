"""collectivecrossing_amd -- MI355X-native batched CollectiveCrossing step.

``CollectiveCrossingEnv`` (dict API, drop-in for the reference), ``BatchedCollectiveCrossing``
(array API), ``VectorCollectiveCrossing`` (many envs behind per-env dict views) and
``rllib.BatchedMultiAgentEnv`` (the batch as one RLlib ``MultiAgentEnv`` with flat agent ids) all run the step on
the GPU through libccx (``include/ccx.h``); there is no CPU implementation of the step path in this
package.
"""

from .configs import CollectiveCrossingConfig  # noqa: F401

__version__ = "0.4.0"
__all__ = ["CollectiveCrossingConfig", "CollectiveCrossingEnv", "BatchedCollectiveCrossing", "VectorCollectiveCrossing",
           "BatchedMultiAgentEnv", "unpack_action_masks", "GaeResult", "SampleResult", "EvalResult",
           "PpoLossResult", "MlpHead", "MlpGradResult", "DeviceAdam", "SideHeads", "QLearning", "QActions",
           "TdLossResult", "ReplayRing", "ReplayBatch", "PrioritizedReplay", "PrioritizedBatch", "NStepReplay",
           "NStepBatch", "RolloutMinibatches", "OnPolicyBatch", "CategoricalQ", "CategoricalLossResult", "WideMlpHead",
           "DeepMlpHead", "DeepGradResult"]


_LAZY = {"CollectiveCrossingEnv": "env", "BatchedCollectiveCrossing": "batched", "VectorCollectiveCrossing": "vector",
         "BatchedMultiAgentEnv": "rllib", "unpack_action_masks": "batched", "GaeResult": "learner", "SampleResult": "learner",
         "EvalResult": "learner", "PpoLossResult": "learner", "MlpHead": "learner",
         "MlpGradResult": "learner", "DeviceAdam": "learner", "SideHeads": "sides", "QLearning": "qlearn",
         "QActions": "qlearn", "TdLossResult": "qlearn", "ReplayRing": "replay", "ReplayBatch": "replay",
         "PrioritizedReplay": "prioritized", "PrioritizedBatch": "prioritized", "NStepReplay": "nstep", "NStepBatch": "nstep",
         "RolloutMinibatches": "minibatch", "OnPolicyBatch": "minibatch", "CategoricalQ": "categorical",
         "CategoricalLossResult": "categorical", "WideMlpHead": "wide", "DeepMlpHead": "deep",
         "DeepGradResult": "deep"}


def __getattr__(name):  # lazy: importing the configs must not pull in torch
    if name not in _LAZY:
        raise AttributeError(name)
    from importlib import import_module
    return getattr(import_module("." + _LAZY[name], __name__), name)


def _register_with_gymnasium() -> None:
    """Same env id as the reference (collectivecrossing/__init__.py:7-10) when gymnasium exists."""
    try:
        from gymnasium.envs.registration import register, registry
    except Exception:
        return
    env_id = "collectivecrossing/CollectiveCrossing-v0"
    if env_id not in registry:
        register(id=env_id, entry_point="collectivecrossing_amd.env:CollectiveCrossingEnv")


_register_with_gymnasium()
