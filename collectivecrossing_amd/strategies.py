"""Strategy plugin interface of the reference, host side (rewards.py, terminateds.py,
truncateds.py, observations.py: ABC + registry dict + ``get_*_function``).

The four built-in families are executed by libccx: each built-in class carries the enum value the
kernel understands (``kernel_mode``) and ``CollectiveCrossingEnv.step`` never calls its Python
method.  The methods exist because they are part of the reference's plugin surface: callers
(and the reference's own tests, e.g. test_rewards.py:476-527 with hand-rolled mock envs) invoke
``strategy.calculate_*(agent_id, env)`` directly; here they evaluate the same rule on the env's
host mirror of the device state.  A user-registered strategy (no ``kernel_mode``) is evaluated on
that mirror after the GPU step and overrides the corresponding output -- the slow, documented path.
"""

from __future__ import annotations

from abc import ABC, abstractmethod

import numpy as np

from . import _abi
from .spaces import Box


def _done(agent_id, env) -> bool:
    a = env._agents[agent_id]
    return bool(a.terminated or a.truncated)


# ------------------------------------------------------------------------------------- rewards
class RewardFunction(ABC):
    kernel_mode: int | None = None
    # A user class whose value depends on NOTHING but the agent's own type and cell (and is ``None`` once the agent is
    # terminated / truncated, like the built-in ones, rewards.py:64) may say so: the batch path then evaluates it once per
    # (type, cell) on the host and runs it inside the kernels as a table (params.position_only_tables, ccx_set_reward_table).
    position_only: bool = False

    def __init__(self, reward_config):
        self.reward_config = reward_config

    @abstractmethod
    def calculate_reward(self, agent_id, env) -> float | None:
        """Reward of ``agent_id`` in the env's current state; ``None`` once it is done."""


class DefaultRewardFunction(RewardFunction):
    """rewards.py:41-99: destination > door > tram-area constants, else a manhattan term whose
    sign is negative for boarding agents and POSITIVE for exiting agents inside the tram."""

    kernel_mode = _abi.REWARD_MODES["default"]

    def calculate_reward(self, agent_id, env):
        if _done(agent_id, env):
            return None
        cfg = self.reward_config
        x, y = (int(v) for v in env._get_agent_position(agent_id))
        centre = (env.tram_door_left + env.tram_door_right) // 2
        if env._agents[agent_id].is_boarding:
            if env.has_agent_reached_destination(agent_id):
                return cfg.boarding_destination_reward
            if env.is_at_tram_door(agent_id):
                return cfg.tram_door_reward
            if env.is_in_tram_area(agent_id):
                return cfg.tram_area_reward
            return np.float64(-(abs(x - centre) + (env.config.division_y - y))) * cfg.distance_penalty_factor
        if env.is_in_exiting_destination_area(agent_id):
            return cfg.boarding_destination_reward
        if not env.is_in_tram_area(agent_id):
            return cfg.tram_area_reward
        return np.float64(abs(x - centre) + (y - env.config.division_y)) * cfg.distance_penalty_factor


class SimpleDistanceRewardFunction(RewardFunction):
    """rewards.py:102-129: ``-|y - destination_y| * factor`` (the destination has no x)."""

    kernel_mode = _abi.REWARD_MODES["simple_distance"]

    def calculate_reward(self, agent_id, env):
        if _done(agent_id, env):
            return None
        pos = env._get_agent_position(agent_id)
        goal = env.get_agent_destination_position(agent_id)
        axis = 1 if goal[0] is None else 0
        return np.float64(-abs(int(pos[axis]) - int(goal[axis]))) * self.reward_config.distance_penalty_factor


class BinaryRewardFunction(RewardFunction):
    """rewards.py:132-159.  The reference compares the position with ``(None, y)`` via
    ``np.array_equal`` which is never true, so every live agent gets ``no_goal_reward``
    (asserted by the reference's test_rewards.py:95-96); reproduced on purpose."""

    kernel_mode = _abi.REWARD_MODES["binary"]

    def calculate_reward(self, agent_id, env):
        return None if _done(agent_id, env) else self.reward_config.no_goal_reward


class ConstantNegativeRewardFunction(RewardFunction):
    kernel_mode = _abi.REWARD_MODES["constant_negative"]

    def calculate_reward(self, agent_id, env):
        return None if _done(agent_id, env) else self.reward_config.step_penalty


REWARD_FUNCTIONS: dict[str, type[RewardFunction]] = {
    "default": DefaultRewardFunction, "simple_distance": SimpleDistanceRewardFunction,
    "binary": BinaryRewardFunction, "constant_negative": ConstantNegativeRewardFunction,
}


# ------------------------------------------------------------------------------------- termination
class TerminatedFunction(ABC):
    kernel_mode: int | None = None
    position_only: bool = False   # as for RewardFunction: terminateds[id] from the agent's own type and cell alone (ccx_set_terminated_table)

    def __init__(self, terminated_config):
        self.terminated_config = terminated_config

    @abstractmethod
    def calculate_terminated(self, agent_id, env) -> bool | None:
        ...


class AllAtDestinationTerminatedFunction(TerminatedFunction):
    kernel_mode = _abi.TERMINATED_MODES["all_at_destination"]

    def calculate_terminated(self, agent_id, env):
        return all(env.has_agent_reached_destination(a) for a in env._agents)


class IndividualAtDestinationTerminatedFunction(TerminatedFunction):
    kernel_mode = _abi.TERMINATED_MODES["individual_at_destination"]

    def calculate_terminated(self, agent_id, env):
        return env.has_agent_reached_destination(agent_id)


TERMINATED_FUNCTIONS: dict[str, type[TerminatedFunction]] = {
    "all_at_destination": AllAtDestinationTerminatedFunction,
    "individual_at_destination": IndividualAtDestinationTerminatedFunction,
}


# ------------------------------------------------------------------------------------- truncation
class TruncatedFunction(ABC):
    kernel_mode: int | None = None

    def __init__(self, truncated_config):
        self.truncated_config = truncated_config

    @abstractmethod
    def calculate_truncated(self, agent_id, env) -> bool | None:
        ...


class MaxStepsTruncatedFunction(TruncatedFunction):
    kernel_mode = _abi.TRUNCATED_MODES["max_steps"]

    def calculate_truncated(self, agent_id, env):
        if _done(agent_id, env):
            return None
        return env._step_count >= self.truncated_config.max_steps


class CustomTruncatedFunction(MaxStepsTruncatedFunction):
    """truncateds.py:64-95: the shipped "custom" strategy only implements the max-steps rule."""

    def calculate_truncated(self, agent_id, env):
        r = super().calculate_truncated(agent_id, env)
        return None if r is None else bool(r)


TRUNCATED_FUNCTIONS: dict[str, type[TruncatedFunction]] = {
    "max_steps": MaxStepsTruncatedFunction, "custom": CustomTruncatedFunction,
}


# ------------------------------------------------------------------------------------- observation
class ObservationFunction(ABC):
    kernel_mode: int | None = None

    def __init__(self, observation_config):
        self.observation_config = observation_config

    @abstractmethod
    def get_agent_observation(self, agent_id, env) -> np.ndarray:
        ...

    @abstractmethod
    def return_agent_observation_space(self, agent_id, env):
        ...


class DefaultObservationFunction(ObservationFunction):
    """observations.py:40-118: ``[x, y, door_centre, division_y, door_left, door_right]`` then a
    4-tuple ``(x, y, type, active)`` per agent in slot order, ``-1`` x4 in the observer's own slot."""

    kernel_mode = 0

    def get_agent_observation(self, agent_id, env):
        ids = list(env._agents)
        me = ids.index(agent_id)
        out = np.empty(6 + 4 * len(ids), np.float32)
        a = env._agents[agent_id]
        out[:6] = (a.x, a.y, (env.tram_door_left + env.tram_door_right) // 2, env.config.division_y,
                   env.tram_door_left, env.tram_door_right)
        for j, other in enumerate(env._agents.values()):
            out[6 + 4 * j:10 + 4 * j] = (-1, -1, -1, -1) if j == me else (
                other.x, other.y, 1 if other.is_exiting else 0, 1 if other.active else 0)
        return out

    def return_agent_observation_space(self, agent_id, env):
        return Box(low=-1, high=max(env.config.width, env.config.height) - 1,
                   shape=(2 + 4 + 4 * len(env._agents),), dtype=np.float32)


OBSERVATION_FUNCTIONS: dict[str, type[ObservationFunction]] = {"default": DefaultObservationFunction}


def _getter(kind: str, table: dict, name_attr: str):
    def get(config):
        name = getattr(config, name_attr)()
        if name not in table:
            raise ValueError(f"Unknown {kind} function '{name}'. Available: {', '.join(table)}")
        return table[name](config)

    return get


get_reward_function = _getter("reward", REWARD_FUNCTIONS, "get_reward_function_name")
get_terminated_function = _getter("termination", TERMINATED_FUNCTIONS, "get_terminated_function_name")
get_truncated_function = _getter("truncation", TRUNCATED_FUNCTIONS, "get_truncated_function_name")
get_observation_function = _getter("observation", OBSERVATION_FUNCTIONS, "get_observation_function_name")


# ------------------------------------------------------------------------------------- array-form plugins
# A user class may define, NEXT TO its per-agent method, a batched one that evaluates every agent of every env at once on
# torch tensors:
#     RewardFunction.calculate_rewards_batch(self, view)          -> float64 [E, N]
#     TerminatedFunction.calculate_terminateds_batch(self, view)  -> bool or int8 [E, N]   (int8: 1 / 0 / -1, -1 = None)
#     TruncatedFunction.calculate_truncateds_batch(self, view)    -> bool [E, N]
# The batched classes then run it between the two halves of the split step (ccx_step_begin / ccx_step_finish) on the
# handle's stream -- no host synchronisation, any number of envs.  `view` shows the state AFTER the moves and the
# deactivation of this step with the flags of BEFORE it, which is what the reference's step() hands to its strategies
# (collectivecrossing.py:214-227).  Reward and truncation values count for agents that were live before the step only
# (the `None` convention of every built-in class, rewards.py:64, truncateds.py:56): what the method returns elsewhere is
# ignored.  The per-agent method stays the definition for the single-env class.
ARRAY_METHODS = {"reward": "calculate_rewards_batch", "termination": "calculate_terminateds_batch",
                 "truncation": "calculate_truncateds_batch"}


def is_array_form(cls, kind: str) -> bool:
    """Does the strategy class define the batched method of its kind?"""
    return cls is not None and callable(getattr(cls, ARRAY_METHODS[kind], None))


class StrategyView:
    """What an array-form strategy sees: torch tensors over the state of E envs x N agent slots (boarding slots first),
    the config, and the reference's predicates as tensor methods.  On a GPU batch the tensors are zero-copy views of the
    handle's own state; CPU tensors work as well (plugins are testable without a GPU).

    ``x``, ``y`` int32 [E, N]; ``active``, ``terminated``, ``truncated`` bool [E, N]; ``step_count`` int32 [E];
    ``is_boarding`` bool [N].  Treat them as read-only."""

    def __init__(self, config, x, y, active, terminated, truncated, step_count):
        import torch

        from .params import calculate_tram_boundaries
        self.config = config
        self.x, self.y = x, y
        self.active, self.terminated, self.truncated = active, terminated, truncated
        self.step_count = step_count
        E, N = (int(v) for v in x.shape)
        nb, ne = config.num_boarding_agents, config.num_exiting_agents
        if N != nb + ne:
            raise ValueError(f"x has {N} agent slots, the config {nb + ne}")
        for name, t, dt, shape in (("x", x, torch.int32, (E, N)), ("y", y, torch.int32, (E, N)),
                                   ("active", active, torch.bool, (E, N)), ("terminated", terminated, torch.bool, (E, N)),
                                   ("truncated", truncated, torch.bool, (E, N)), ("step_count", step_count, torch.int32, (E,))):
            if t.dtype is not dt or tuple(t.shape) != shape or t.device != x.device:
                raise TypeError(f"StrategyView.{name}: expected {dt} {shape} on {x.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        self.num_envs, self.num_agents = E, N
        self.device = x.device
        tb = calculate_tram_boundaries(config)
        self.tram_left, self.tram_right = tb.tram_left, tb.tram_right
        self.tram_door_left, self.tram_door_right = tb.tram_door_left, tb.tram_door_right
        self.is_boarding = torch.arange(N, device=x.device) < nb
        self._dest_y = torch.where(self.is_boarding, config.boarding_destination_area_y,
                                   config.exiting_destination_area_y).to(torch.int32)

    @property
    def live(self):
        """Not terminated and not truncated before this step: the agents rewards / truncations are handed out for."""
        return ~(self.terminated | self.truncated)

    # the reference's predicates (collectivecrossing.py:551-563, 663-683), bit-equal to the CCX_AF_* flag bits
    def in_tram_area(self):
        return (self.y >= self.config.division_y) & (self.x >= self.tram_left) & (self.x <= self.tram_right)

    def at_door(self):
        return (self.y == self.config.division_y) & ((self.x == self.tram_door_left - 1) | (self.x == self.tram_door_right + 1))

    def at_destination(self):
        return self.y == self._dest_y

    def in_exiting_destination_area(self):
        return self.y == self.config.exiting_destination_area_y


def check_batch_result(kind: str, fn, value, view: StrategyView):
    """Shape / dtype / device check of what an array-form method returned (host-side, no synchronisation); returns the
    tensor in the form ccx_step_finish reads: f64 rewards, int8 terminateds (1 / 0 / -1), uint8 truncateds."""
    import torch
    what = f"{type(fn).__name__}.{ARRAY_METHODS[kind]}"
    shape = (view.num_envs, view.num_agents)
    allowed = {"reward": (torch.float64,), "termination": (torch.bool, torch.int8), "truncation": (torch.bool,)}[kind]
    if not isinstance(value, torch.Tensor):
        raise TypeError(f"{what} must return a torch.Tensor, got {type(value).__name__}")
    if value.dtype not in allowed:
        raise TypeError(f"{what} must return {' or '.join(str(d) for d in allowed)}, got {value.dtype}")
    if tuple(value.shape) != shape:
        raise TypeError(f"{what} must return shape {shape}, got {tuple(value.shape)}")
    if value.device != view.device:
        raise TypeError(f"{what} must return a tensor on {view.device}, got {value.device}")
    value = value.contiguous()
    if value.dtype is torch.bool:
        value = value.to(torch.int8) if kind == "termination" else value.view(torch.uint8)
    return value
