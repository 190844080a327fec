"""Array-form strategy plugins (test tooling, written for this repo).

``make_g12_twins``: the three g12 plugins of custom_strategies.py with their batched methods next to the per-agent ones
(``calculate_rewards_batch`` / ``calculate_terminateds_batch`` / ``calculate_truncateds_batch`` on a
``collectivecrossing_amd.strategies.StrategyView``).

``make_g15``: three plugins g12 lacks -- a reward that counts OTHER ACTIVE agents within Chebyshev distance 1, a
termination rule that reads every agent of the env (everybody is done once half the agents have arrived; ``None`` for
an agent that is already terminated) and a truncation budget that shrinks with the number of agents standing in the tram
area -- each in the per-agent form (what the reference runs: gen_array_golden.py records it) AND in array form.  The
per-agent forms only use the surface both envs offer: ``env._agents[id]`` (``position``, ``active``, ``terminated``,
``truncated``, ``agent_type``), ``env._step_count``, ``env.has_agent_reached_destination``, ``env.is_in_tram_area``.
The batched methods import torch lazily, so the reference-side generator needs none.
"""

import custom_strategies as cs


def make_g12_twins(reward_base, terminated_base, truncated_base):
    import torch
    base = cs.make(reward_base, terminated_base, truncated_base)

    class ArrivalBonusRewardA(base["reward"]):
        def calculate_rewards_batch(self, view):
            step = view.step_count.to(torch.float64)[:, None]
            return torch.where(view.at_destination(), 100.0 - step, -0.25 * step - view.in_tram_area().to(torch.float64))

    class TramAreaTerminatedA(base["terminated"]):
        def calculate_terminateds_batch(self, view):
            t = torch.where(view.is_boarding, view.in_tram_area(), view.at_destination()).to(torch.int8)
            return torch.where(view.terminated, -1, t).to(torch.int8)

    class PerTypeBudgetTruncatedA(base["truncated"]):
        def calculate_truncateds_batch(self, view):
            budget = self.truncated_config.max_steps + torch.where(view.is_boarding, 0, 4)
            return view.step_count[:, None] >= budget[None, :]

    return {"reward": ArrivalBonusRewardA, "terminated": TramAreaTerminatedA, "truncated": PerTypeBudgetTruncatedA}


G15_NAMES = {"reward": "crowding", "terminated": "half_arrived", "truncated": "crowd_budget"}


def make_g15(reward_base, terminated_base, truncated_base):
    class CrowdingReward(reward_base):
        """-0.5 per OTHER ACTIVE agent within Chebyshev distance 1; +10 on the destination row, else -0.125 per step."""

        def calculate_reward(self, agent_id, env):
            a = env._agents[agent_id]
            if a.terminated or a.truncated:
                return None
            x, y = int(a.position[0]), int(a.position[1])
            n = 0
            for other_id, b in env._agents.items():
                if other_id != agent_id and b.active and max(abs(int(b.position[0]) - x), abs(int(b.position[1]) - y)) <= 1:
                    n += 1
            return -0.5 * n + (10.0 if env.has_agent_reached_destination(agent_id) else -0.125 * env._step_count)

        def calculate_rewards_batch(self, view):
            import torch
            dx = (view.x[:, :, None] - view.x[:, None, :]).abs()
            dy = (view.y[:, :, None] - view.y[:, None, :]).abs()
            near = (torch.maximum(dx, dy) <= 1) & view.active[:, None, :]
            near &= ~torch.eye(view.num_agents, dtype=torch.bool, device=view.device)[None]
            n = near.sum(dim=2).to(torch.float64)
            step = view.step_count.to(torch.float64)[:, None]
            tail = torch.where(view.at_destination(), torch.full_like(step, 10.0).expand_as(n), (-0.125 * step).expand_as(n))
            return -0.5 * n + tail

    class HalfArrivedTerminated(terminated_base):
        """Everybody is done once at least half of the env's agents stand on their destination row; before that an
        agent is done on its own row.  No entry (None) for an agent that is already terminated."""

        def calculate_terminated(self, agent_id, env):
            if env._agents[agent_id].terminated:
                return None
            arrived = sum(1 for i in env._agents if env.has_agent_reached_destination(i))
            if 2 * arrived >= len(env._agents):
                return True
            return bool(env.has_agent_reached_destination(agent_id))

        def calculate_terminateds_batch(self, view):
            import torch
            at = view.at_destination()
            half = (2 * at.sum(dim=1, keepdim=True)) >= view.num_agents
            return torch.where(view.terminated, -1, (at | half).to(torch.int8)).to(torch.int8)

    class CrowdBudgetTruncated(truncated_base):
        """The step budget is max_steps minus the number of agents standing in the tram area."""

        def calculate_truncated(self, agent_id, env):
            a = env._agents[agent_id]
            if a.terminated or a.truncated:
                return None
            crowd = sum(1 for i in env._agents if env.is_in_tram_area(i))
            return env._step_count >= self.truncated_config.max_steps - crowd

        def calculate_truncateds_batch(self, view):
            crowd = view.in_tram_area().sum(dim=1)
            u = view.step_count >= (self.truncated_config.max_steps - crowd)
            return u[:, None].expand(view.num_envs, view.num_agents)

    return {"reward": CrowdingReward, "terminated": HalfArrivedTerminated, "truncated": CrowdBudgetTruncated}


C1 = dict(width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9, num_boarding_agents=5,
          num_exiting_agents=3, exiting_destination_area_y=0, boarding_destination_area_y=8)
# the C2 workload's geometry (4096 envs x 8 agents in the benchmark)
C2 = dict(C1)
# a grid whose occupancy tables do not fit in LDS (the geometry of the g14 fixtures)
BIG = dict(width=100, height=100, division_y=50, tram_door_left=25, tram_door_right=35, tram_length=60,
           num_boarding_agents=6, num_exiting_agents=5, exiting_destination_area_y=0, boarding_destination_area_y=100)


def g15_config(cfg_mod, reward_cfg_mod, term_cfg_mod, trunc_cfg_mod, geometry, max_steps):
    """`geometry` with the three g15 plugins; works with the reference's config modules and with
    collectivecrossing_amd.configs (passed four times) alike."""
    return cfg_mod.CollectiveCrossingConfig(
        **geometry, reward_config=reward_cfg_mod.CustomRewardConfig(reward_function=G15_NAMES["reward"]),
        terminated_config=term_cfg_mod.CustomTerminatedConfig(terminated_function=G15_NAMES["terminated"]),
        truncated_config=trunc_cfg_mod.CustomTruncatedConfig(truncated_function=G15_NAMES["truncated"], max_steps=max_steps))


def register(strategies_mod, classes, names):
    """Put the classes into the three registries of `strategies_mod`; returns the undo function."""
    tables = {"reward": strategies_mod.REWARD_FUNCTIONS, "terminated": strategies_mod.TERMINATED_FUNCTIONS,
              "truncated": strategies_mod.TRUNCATED_FUNCTIONS}
    for key, cls in classes.items():
        tables[key][names[key]] = cls

    def undo():
        for key in classes:
            tables[key].pop(names[key], None)
    return undo
