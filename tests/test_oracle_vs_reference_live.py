"""Pinning of the oracle against the reference on random reference-valid configs, step by step --
positions, flags, rewards (bit patterns), observations, and the scripted policies' actions.  The reference's side
of every case at the default seed base is committed data (tests/golden/live_reference/, recorded from the imported
reference by ``gen_golden.py --only=live``), so the comparison runs wherever the repository does.  With
CCX_LIVE_SEED set to another base, and the reference present (CCX_REFERENCE), the cases are redrawn and run through
the IMPORTED reference in the same process instead."""

import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "golden"))
import gen_golden as G  # noqa: E402

# the seed base of the cases (the committed sample is G.LIVE_BASE's)
BASE = int(os.environ.get("CCX_LIVE_SEED", str(G.LIVE_BASE)))


class _Cases:
    """The reference's side of a case: (config dict, arrays), from the committed sample or from a live draw."""

    def __init__(self, live: bool):
        self.live, self._files = live, {}

    def case(self, kind: str, name: str, *args):
        if self.live:
            return getattr(G, f"live_{kind}_case")(BASE, *args)
        if kind not in self._files:
            with np.load(G.LIVE_DIR / f"{kind}.npz") as z:
                assert int(z["base"]) == G.LIVE_BASE
                self._files[kind] = {k: z[k] for k in z.files}
        a, p = self._files[kind], f"{name}__"
        return (json.loads(str(a[p + "config_json"])),
                {k[len(p):]: v for k, v in a.items() if k.startswith(p) and k != p + "config_json"})


@pytest.fixture(scope="module")
def reference():
    if BASE == G.LIVE_BASE:
        return _Cases(live=False)
    if not (G.REF / "src" / "collectivecrossing").is_dir():
        pytest.skip(f"CCX_LIVE_SEED={BASE} redraws the cases through the reference, which is not present (CCX_REFERENCE)")
    G.import_reference()
    return _Cases(live=True)


class _Mem:
    """Recorded arrays with the interface of _fixtures.Golden (no file per case)."""

    def __init__(self, a, cfg):
        from _fixtures import config_from_dict
        from collectivecrossing_amd.params import lower_config

        self.a, self.name = a, "live"
        self.config = config_from_dict(cfg)
        self.params = lower_config(self.config)
        self.K, self.E, self.N = a["actions"].shape

    def __getitem__(self, k):
        return self.a[k]

    def init_state(self):
        return dict(x=self["init_x"], y=self["init_y"], active=self["init_active"],
                    terminated=self["init_terminated"], truncated=self["init_truncated"],
                    step_count=self["init_step_count"])


@pytest.mark.parametrize("index", G.LIVE_RANDOM)
def test_random_config_reference_vs_oracle(reference, oracle, index):
    from _fixtures import assert_step_matches
    from test_oracle_golden import _state

    cfg, a = reference.case("random", f"i{index:02d}", index)
    g = _Mem(a, cfg)
    b = oracle.OracleBatch(g.params, g.E)
    b.set_state(**g.init_state())
    for s in range(g.K):
        obs, rew, af, ef = b.step(g["actions"][s], g["order"][s])
        assert_step_matches(g, s, obs, rew, af, ef, _state(b), label=f"cfg {cfg}")


@pytest.mark.parametrize("index,policy", G.LIVE_POLICY)
def test_random_config_reference_policy_vs_oracle(reference, oracle, index, policy):
    cfg, a = reference.case("policy", f"i{index:02d}_{policy}", index, policy)
    g = _Mem(a, cfg)
    b = oracle.OracleBatch(g.params, 1)
    b.set_state(**g.init_state())
    for s in range(g.K):
        # the reference policy's actions (255 = agent not in its dict) for the state both envs are in
        mine = b.policy_actions(policy)[0]
        np.testing.assert_array_equal(mine, g["actions"][s][0], err_msg=f"{policy} step {s} cfg {cfg}")
        b.step(g["actions"][s], g["order"][s], want_obs=False)


@pytest.mark.parametrize("index,policy,eps", G.LIVE_HOST_POLICY)
def test_host_policy_classes_vs_reference_policies_with_epsilon(reference, index, policy, eps):
    """collectivecrossing_amd.baseline_policies next to the reference's classes, both seeded with 42, on
    the states of one reference env (mirrored into a host view each step): same action every call."""
    from _fixtures import config_from_dict

    from collectivecrossing_amd import baseline_policies as bp
    from collectivecrossing_amd.env import CollectiveCrossingEnv

    cfg, a = reference.case("host_policy", f"i{index:02d}_{policy}", index, policy, eps)
    ours = CollectiveCrossingEnv.host_view(config_from_dict(cfg))
    our_pol = (bp.GreedyPolicy if policy == "greedy" else bp.WaitingPolicy)(randomness_factor=eps, seed=42)
    ids = G.ids_of(cfg)
    assert len(a["agents"]) >= 1
    for s in range(len(a["agents"])):
        m = ours._mirror
        for i in range(len(ids)):
            m.x[i], m.y[i] = int(a["x"][s, i]), int(a["y"][s, i])
            m.active[i], m.terminated[i], m.truncated[i] = (bool(a["active"][s, i]), bool(a["terminated"][s, i]),
                                                            bool(a["truncated"][s, i]))
        m.touch()
        live = [ids[i] for i in a["agents"][s] if i >= 0]
        assert ours.agents == live
        for aid, want in zip(live, a["actions"][s]):
            got = int(our_pol.get_action(aid, None, ours))
            assert got == int(want), f"{policy} eps {eps} step {s} agent {aid} cfg {cfg}"
