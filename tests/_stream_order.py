"""The stream-order harness: does every enqueueing method order its launches against torch's CURRENT
stream when that is not the handle's stream?

A case prepares a :class:`Plan` on a fresh batch whose launches go to ``main``: the tensors the method reads (holding
STALE but valid values, with the real values next to them), the call, and the outputs that exist before the call
(prefilled).  :func:`run` plays it with ``other`` current in one of two directions:

* ``before`` (rule a): a blocker keeps ``other`` busy, the real inputs are copied over the stale ones behind it, a
  snapshot of the outputs is taken there, then the method is called.  Without the order the launch runs at once on the
  idle ``main``: it reads the stale inputs, and it overwrites the outputs before the snapshot has read them.
* ``after`` (rule b): a blocker keeps ``main`` busy, the method is called and every output is cloned at once on ``other``.
  Without the wait the clones hold the prefill.

The expected bytes come from the same plan on a twin batch with ``main`` current throughout (``block=False``); the other
suites pin that path to the specs and the oracle, so this one is about order alone.  A run whose blocker had already ended
when the last piece was enqueued proves nothing: ``Outcome.open`` says so and the tests assert it.  Nothing here reads or
writes outside its own tensors, whatever the order: stale inputs are legal inputs, every buffer is static.

The table at the bottom (``CASES``, ``EXEMPT``) is what tests/test_stream_order_table.py checks for completeness."""

from __future__ import annotations

import inspect
import re
import time
from dataclasses import dataclass, field

import numpy as np
from _reset_obs_spec import make_config

E, N, K, ROWS, H = 64, 8, 4, 257, 16         # envs, agents, steps of a rollout, rows of the row-wise learner ops, hidden width
PREFILL = 0xA5                               # every byte of a prefilled output: no action, no flag byte, no float a case computes
STALE_FLAGS = 0x4C                           # AF_LIVE | AF_OBS | AF_ACTIVE: a legal agent_flags byte

# The blocker: BLOCKER_LINKS products of two f32 [BLOCKER_N, BLOCKER_N] matrices on one stream.  Measured on an MI355X with
# events: one link lasts 7.1 ms, the chain BLOCKER_MS; enqueueing it takes 0.12 ms.  The longest host time
# of any case of the table from enqueueing the blocker to enqueueing the last consumer was BLOCKER_HOST_MS (time.perf_counter;
# the autograd cases of the policy head).  The chain lasts at least 20 times that.  The condition itself is ``Outcome.open``;
# the factor only sets how rarely it can trip.  (Smaller matrices need more links for the same time, and enqueueing the
# links is then the largest part of the host time: 24 links of 4096 last 21.9 ms and take 0.54 ms to enqueue.)
BLOCKER_N = 8192
BLOCKER_LINKS = 5
BLOCKER_MS = 35.6
BLOCKER_HOST_MS = 1.42


class Blocker:
    """A fixed chain of public torch ops that keeps one stream busy, on buffers allocated once."""

    def __init__(self, links: int = BLOCKER_LINKS, n: int = BLOCKER_N):
        import torch

        self.links = links
        self.a = torch.full((n, n), 1.0 / n, dtype=torch.float32, device="cuda")
        self.b = torch.ones((n, n), dtype=torch.float32, device="cuda")
        self.c = torch.empty((n, n), dtype=torch.float32, device="cuda")
        torch.mm(self.a, self.b, out=self.c)                     # (the BLAS library's own first-call work happens here)
        torch.cuda.synchronize()

    def warm(self, *streams) -> None:
        """The one-off host work of a stream's first launch, first event and first wait, outside any measured window."""
        import torch

        for s in streams:
            self.run(s)
        for s in streams:
            for t in streams:
                if s is not t:
                    s.wait_stream(t)
        torch.cuda.synchronize()

    def run(self, stream):
        """Enqueue the chain on ``stream``; returns the event recorded behind it."""
        import torch

        with torch.cuda.stream(stream):
            for _ in range(self.links):
                torch.mm(self.a, self.b, out=self.c)
            ev = torch.cuda.Event()
            ev.record(stream)
        return ev


@dataclass
class Plan:
    inputs: list                    # (buffer the method reads, holding the stale value; the real value), device tensors
    call: object                    # () -> list of every output tensor; enqueues the method and nothing that waits
    outs: list = field(default_factory=list)    # the outputs that exist before the call, prefilled (write after read)
    sanity: object = None           # (list of expected outputs as uint8 arrays) -> None: the case exercised what it names


@dataclass
class Outcome:
    got: list                       # uint8 arrays: the outputs (cloned at once on the current stream for ``after``)
    snaps: list                     # uint8 arrays: ``before``: the outputs as the current stream saw them before the call
    pre: list                       # uint8 arrays: what ``outs`` held when the run began
    open: bool                      # the blocker was still running when the last piece had been enqueued
    host_ms: float                  # host time from enqueueing the blocker to that moment
    keep: object = None             # the output tensors themselves, alive until the comparison is over


class World:
    """A fresh batch of E envs bound to ``main``, in a reproducible state: the same for a case's run and its twin."""

    def __init__(self, kind: str, main):
        import torch
        from collectivecrossing_amd.batched import BatchedCollectiveCrossing

        torch.manual_seed(20261)                                  # (MlpHead draws its parameters from torch's generator)
        self.kind, self.main = kind, main
        self.undo = None
        if kind == "array":
            self.undo, cfg = _array_config()
        else:
            cfg = make_config(N, max_steps=12)
        b = self.batch = BatchedCollectiveCrossing(cfg, E)
        b.use_stream(main)
        b.make_reset_pool(seed0=11, size=128)
        b.reset_from_pool()
        b.set_rng_seed(5)
        # ten steps in: envs differ, some agents are done, and max_steps = 12 truncates inside a K = 4 rollout
        b.rollout(dev(np.random.default_rng(3).integers(0, 5, size=(10, E, N), dtype=np.uint8)), auto_reset=True, want_traj=False)
        if kind == "tracked":
            b.track_episodes(log_capacity=32)

    def close(self) -> None:
        self.batch.use_stream(None)
        self.batch.close()
        if self.undo is not None:
            self.undo()


def _array_config():
    """A config whose reward is a user class in array form (the split step), registered for the life of a World."""
    import torch
    from collectivecrossing_amd import configs as C
    from collectivecrossing_amd import strategies as S

    class CrowdReward(S.RewardFunction):
        def calculate_reward(self, agent_id, env):
            raise NotImplementedError("the stream-order cases run the array form only")

        def calculate_rewards_batch(self, view):
            near = ((view.x[:, :, None] - view.x[:, None, :]).abs() <= 1) & view.active[:, None, :]
            return -0.25 * near.sum(dim=2).to(torch.float64) + view.y.to(torch.float64)

    S.REWARD_FUNCTIONS["stream_order_crowd"] = CrowdReward
    base = make_config(N, max_steps=12)
    cfg = base.model_copy(update={"reward_config": C.CustomRewardConfig(reward_function="stream_order_crowd")})
    return (lambda: S.REWARD_FUNCTIONS.pop("stream_order_crowd", None)), cfg


# ----------------------------------------------------------------------------------------------------------- small helpers
def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tensors(res) -> list:
    """The tensor fields of a result dataclass, in field order."""
    import torch

    return [v for v in vars(res).values() if isinstance(v, torch.Tensor)]


def fill_bytes(*ts) -> None:
    import torch

    for t in ts:
        t.detach().view(torch.uint8).fill_(PREFILL)


def prefilled(shape, dtype):
    import torch

    t = torch.empty(tuple(shape), dtype=dtype, device="cuda")
    fill_bytes(t)
    return t


def inp(real, stale=0):
    """``(buffer holding the stale value, the real value)``: ``stale`` is a tensor like ``real`` or one number for all."""
    import torch

    real = real if isinstance(real, torch.Tensor) else dev(real)
    real = real.detach().clone()
    buf = stale.detach().clone() if isinstance(stale, torch.Tensor) else torch.full_like(real, stale)
    assert buf.shape == real.shape and buf.dtype == real.dtype
    return buf, real


def as_bytes(t) -> np.ndarray:
    import torch

    t = t.detach().contiguous().reshape(-1)
    return (t.view(torch.uint8) if t.numel() else t.to(torch.uint8)).cpu().numpy()


def actions(rng, *lead):
    return rng.integers(0, 5, size=(*lead, E, N), dtype=np.uint8)


def orders(rng, *lead):
    return np.argsort(rng.random((*lead, E, N)), axis=-1).astype(np.uint8)


def identity(*lead):
    return dev(np.broadcast_to(np.arange(N, dtype=np.uint8), (*lead, E, N)))


def normal(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def param_inputs(batch, head) -> list:
    """A head's parameters as inputs: they hold a SECOND seeded initialisation until the real one is copied in."""
    import torch

    other = batch.mlp_head(head.H, head.O, head.activation, head.L)
    pairs = []
    with torch.no_grad():
        for p, q in zip(head.parameters(), other.parameters()):
            real = p.detach().clone()
            p.copy_(q)
            pairs.append((p, real))
    return pairs


# ------------------------------------------------------------------------------------------------------------- the player
def run(case, direction: str, main, other, blocker: Blocker | None, block: bool = True, seed: int = 0) -> Outcome:
    """Play ``case`` in ``direction`` on a fresh World.  ``block=False`` is the twin: ``main`` current throughout, no
    blocker, the same plan from the same seeds."""
    import torch

    assert direction in ("before", "after")
    cur = other if block else main
    rng = np.random.default_rng(seed)
    with torch.cuda.stream(main):
        world = World(case.world, main)
    try:
        with torch.cuda.stream(main), torch.no_grad():
            plan = case.setup(world, rng)
            if direction == "after":
                for buf, real in plan.inputs:
                    buf.copy_(real)
            pre = [as_bytes(o) for o in plan.outs]
        torch.cuda.synchronize()
        snaps, got, ev = [], None, None
        with torch.cuda.stream(cur):
            t0 = time.perf_counter()
            if block:
                ev = blocker.run(other if direction == "before" else main)
            if direction == "before":
                with torch.no_grad():
                    for buf, real in plan.inputs:
                        buf.copy_(real)
                snaps = [o.detach().clone() for o in plan.outs]
            outs = plan.call()
            if direction == "after":
                got = [o.detach().clone() for o in outs]
            host_ms = (time.perf_counter() - t0) * 1e3
            still_open = ev is None or not ev.query()
        torch.cuda.synchronize()
        if got is None:
            got = outs
        out = Outcome([as_bytes(t) for t in got], [as_bytes(t) for t in snaps], pre, still_open, host_ms, keep=(outs, got))
        if plan.sanity is not None and not block:
            plan.sanity(out.got)
        return out
    finally:
        torch.cuda.synchronize()
        world.close()


def differs(a: list, b: list) -> bool:
    return len(a) != len(b) or any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))


def seed_of(case, direction: str) -> int:
    """Different data in the two directions (and in every case): whatever an earlier run left in freed memory is not what
    this run expects."""
    return 1000 * (1 + CASES.index(case)) + (direction == "after")


# ----------------------------------------------------------------------------------------------------------------- the table
@dataclass
class Case:
    name: str
    world: str                      # "sim", "array" (a config with an array-form strategy class) or "tracked"
    covers: tuple                   # "Class.method" of every public method the case calls into the library through
    setup: object                   # (World, numpy Generator) -> Plan
    directions: tuple = ("before", "after")


CASES: list[Case] = []


def case(name, world, covers):
    def add(fn):
        CASES.append(Case(name, world, tuple(("BatchedCollectiveCrossing." + c) if "." not in c else c for c in covers), fn))
        return fn
    return add


# ---- simulator: queries of the current state
def _state_query(method, shape_of, dtype_name, **kw):
    def setup(w, rng):
        import torch

        b = w.batch
        out = prefilled(shape_of(b), getattr(torch, dtype_name))
        return Plan([], lambda: [getattr(b, method)(out=out, **kw)], [out])
    return setup


case("observe", "sim", ["observe"])(_state_query("observe", lambda b: (E, N, b.obs_len), "float32"))
case("action_masks", "sim", ["action_masks"])(_state_query("action_masks", lambda b: (E, N), "uint8"))
case("policy_actions", "sim", ["policy_actions"])(_state_query("policy_actions", lambda b: (E, N), "uint8", policy="waiting"))
case("greedy_actions", "sim", ["greedy_actions"])(_state_query("greedy_actions", lambda b: (E, N), "uint8"))


# ---- simulator: one step.  The first call allocates the batch's static one-step buffers; the case prefills them.
def _step(with_order: bool, **kw):
    def setup(w, rng):
        b = w.batch
        a = inp(actions(rng), 4)
        o = inp(orders(rng), identity()) if with_order else (None, None)
        res = b.step(a[0], o[0], **kw)
        extra = tensors(b.episode_stats()) if w.kind == "tracked" else []
        fill_bytes(*tensors(res))
        return Plan([a] + ([o] if with_order else []), lambda: tensors(b.step(a[0], o[0], **kw)) + extra, tensors(res))
    return setup


case("step", "sim", ["step"])(_step(False))
case("step_order_masks", "sim", ["step"])(_step(True, want_masks=True, want_compact=True))
case("step_tracked_stats_views", "tracked", ["step", "episode_stats"])(_step(False))
case("step_array_strategies", "array", ["step"])(_step(True, want_masks=True))


@case("step_mixed", "sim", ["step_mixed"])
def _step_mixed(w, rng):
    import torch

    b = w.batch
    a, o = inp(actions(rng), 4), inp(orders(rng), identity())
    merged = prefilled((E, N), torch.uint8)
    kw = dict(scripted="exiting", policy="greedy", actions_out=merged, want_masks=True)
    res = b.step_mixed(a[0], order=o[0], **kw)
    fill_bytes(merged, *tensors(res))
    return Plan([a, o], lambda: tensors(b.step_mixed(a[0], order=o[0], **kw)) + [merged], tensors(res) + [merged])


# ---- simulator: rollouts into the caller's buffers
def _saw_reset(flags_at: int):
    def sanity(want):
        assert (want[flags_at] & 0x04).any(), "no env restarted inside the rollout: final_obs was not exercised"
    return sanity


@case("rollout", "sim", ["rollout"])
def _rollout(w, rng):
    import torch

    b = w.batch
    a, o = inp(actions(rng, K), 4), inp(orders(rng, K), identity(K))
    out = b.alloc_rollout(K, want_obs=True, want_compact=True, want_final=True)
    masks = prefilled((E, N), torch.uint8)
    fill_bytes(*tensors(out))
    assert out.final_obs is not None and out.final_compact is not None
    return Plan([a, o], lambda: tensors(b.rollout(a[0], o[0], auto_reset=True, out=out, want_compact=True, masks_out=masks,
                                                   reset_obs="next")) + [masks], tensors(out) + [masks], _saw_reset(3))


@case("rollout_mixed", "sim", ["rollout_mixed"])
def _rollout_mixed(w, rng):
    import torch

    b = w.batch
    a, o = inp(actions(rng, K), 4), inp(orders(rng, K), identity(K))
    out = b.alloc_rollout(K)
    merged, masks = prefilled((K, E, N), torch.uint8), prefilled((E, N), torch.uint8)
    fill_bytes(*tensors(out))
    return Plan([a, o], lambda: tensors(b.rollout_mixed(a[0], "boarding", "waiting", order=o[0], auto_reset=True, out=out,
                                                         actions_out=merged, masks_out=masks)) + [merged, masks],
                tensors(out) + [merged, masks])


def _rollout_scripted(method, *args):
    def setup(w, rng):
        import torch

        b = w.batch
        out = b.alloc_rollout(K)
        acts, masks = prefilled((K, E, N), torch.uint8), prefilled((E, N), torch.uint8)
        fill_bytes(*tensors(out))

        def call():
            res, got = getattr(b, method)(K, *args, auto_reset=True, out=out, actions_out=acts, masks_out=masks)
            return tensors(res) + [got, masks]
        return Plan([], call, tensors(out) + [acts, masks])
    return setup


case("rollout_greedy", "sim", ["rollout_greedy"])(_rollout_scripted("rollout_greedy"))
case("rollout_policy", "sim", ["rollout_policy"])(_rollout_scripted("rollout_policy", "random"))


@case("rollout_array_strategies", "array", ["rollout"])
def _rollout_array(w, rng):
    b = w.batch
    a = inp(actions(rng, K), 4)
    out = b.alloc_rollout(K)
    fill_bytes(*tensors(out))
    return Plan([a], lambda: tensors(b.rollout(a[0], auto_reset=True, out=out)), tensors(out))


# ---- simulator: the split step
@case("split_step_array_strategies", "array", ["step_begin", "run_array_strategies", "step_finish"])
def _split_array(w, rng):
    b = w.batch
    a, o = inp(actions(rng), 4), inp(orders(rng), identity())

    def go():
        b.step_begin(a[0], o[0])
        own = b.run_array_strategies()
        return b.step_finish(*own, want_compact=True), [t for t in own if t is not None]

    res, _ = go()
    fill_bytes(*tensors(res))

    def call():
        res, own = go()
        return tensors(res) + own
    return Plan([a, o], call, tensors(res))


@case("split_step_user_arrays", "sim", ["step_begin", "step_finish"])
def _split_user(w, rng):
    b = w.batch
    a = inp(actions(rng), 4)
    r = inp(rng.standard_normal((E, N)), 0.0)
    t = inp(rng.integers(-1, 2, size=(E, N)).astype(np.int8), 0)
    u = inp(rng.integers(0, 2, size=(E, N)).astype(np.uint8), 0)
    kw = dict(auto_reset=True, reset_obs="next", want_final=True, want_compact=True)

    def go():
        b.step_begin(a[0])
        return b.step_finish(r[0], t[0], u[0], **kw)

    res = go()
    fill_bytes(*tensors(res))
    view = b.strategy_view()
    return Plan([a, r, t, u], lambda: tensors(go()) + [view.x, view.y, view.active], tensors(res))


@case("reset_from_pool_mask", "sim", ["reset_from_pool", "strategy_view"])
def _reset_from_pool(w, rng):
    b = w.batch
    m = inp(rng.integers(0, 2, size=(E,)).astype(np.uint8), 1)
    view = b.strategy_view()
    state = [view.x, view.y, view.active, view.terminated, view.step_count]

    def call():
        b.reset_from_pool(m[0])
        return state
    return Plan([m], call, state)


# ---- simulator: compact rows and frames
def _compact_rows(w, rng):
    b = w.batch
    traj = b.rollout(dev(actions(rng, K)), auto_reset=True, want_obs=False, want_compact=True)
    return inp(traj.obs_compact[K - 1], traj.obs_compact[0])            # stale: the rows of an earlier state


@case("expand_observations", "sim", ["expand_observations"])
def _expand(w, rng):
    import torch

    b = w.batch
    c = _compact_rows(w, rng)
    out = prefilled((E, N, b.obs_len), torch.float32)
    return Plan([c], lambda: [b.expand_observations(c[0], out=out)], [out])


@case("render", "sim", ["render"])
def _render(w, rng):
    import torch

    b = w.batch
    ids = inp(rng.integers(0, E, size=(16,)).astype(np.int32), 0)
    out = prefilled((16, *b.frame_shape(2)), torch.uint8)
    return Plan([ids], lambda: [b.render(ids[0], cell_px=2, out=out)], [out])


@case("render_compact", "sim", ["render_compact"])
def _render_compact(w, rng):
    import torch

    b = w.batch
    c = _compact_rows(w, rng)
    out = prefilled((E, *b.frame_shape(2)), torch.uint8)
    return Plan([c], lambda: [b.render_compact(c[0], cell_px=2, out=out)], [out])


# ---- simulator: episode statistics and counters (the outputs are views of the handle's own memory)
@case("update_episode_stats", "sim", ["update_episode_stats", "episode_stats"])
def _update_stats(w, rng):
    b = w.batch
    traj = b.rollout(dev(actions(rng, K)), auto_reset=True, want_obs=False)
    b.track_episodes(log_capacity=32)
    r, af, ef = inp(traj.reward, 0.0), inp(traj.agent_flags, STALE_FLAGS), inp(traj.env_flags, 0)
    views = tensors(b.episode_stats())

    def call():
        b.update_episode_stats(r[0], af[0], ef[0])
        return views
    return Plan([r, af, ef], call, views)


def _tracked_steps(w, rng):
    b = w.batch
    b.rollout(dev(actions(rng, K)), auto_reset=True, want_obs=False)       # (tracked: episodes end in here, the log fills)
    return tensors(b.episode_stats())


@case("reset_episode_stats", "tracked", ["reset_episode_stats", "episode_stats"])
def _reset_stats(w, rng):
    b = w.batch
    views = _tracked_steps(w, rng)
    m = inp(rng.integers(0, 2, size=(E,)).astype(np.uint8), 1)

    def call():
        b.reset_episode_stats(m[0])
        return views
    return Plan([m], call, views)


@case("clear_episode_log", "tracked", ["clear_episode_log", "episode_stats"])
def _clear_log(w, rng):
    b = w.batch
    _tracked_steps(w, rng)
    count = [b.episode_stats().log_count]

    def call():
        b.clear_episode_log()
        return count
    return Plan([], call, count)


@case("zero_counters", "sim", ["zero_counters", "counters_tensor"])
def _zero_counters(w, rng):
    b = w.batch
    count = [b.counters_tensor()]

    def call():
        b.zero_counters()
        return count
    return Plan([], call, count)


# ---- learner: advantages and sampling
@case("compute_gae", "sim", ["LearnerOps.compute_gae"])
def _gae(w, rng):
    b = w.batch
    traj = b.rollout(dev(actions(rng, K)), auto_reset=True, want_obs=False)
    r, af, ef = inp(traj.reward, 0.0), inp(traj.agent_flags, STALE_FLAGS), inp(traj.env_flags, 0)
    v, lv, fv = inp(normal(rng, K, E, N)), inp(normal(rng, E, N)), inp(normal(rng, K, E, N))
    out = b.alloc_gae(K)
    fill_bytes(*tensors(out))
    return Plan([r, af, ef, v, lv, fv],
                lambda: tensors(b.compute_gae((r[0], af[0], ef[0]), v[0], lv[0], fv[0], gamma=0.97, lam=0.9, out=out)),
                tensors(out))


@case("sample_actions", "sim", ["LearnerOps.sample_actions"])
def _sample(w, rng):
    b = w.batch
    logits, masks = inp(normal(rng, E, N, 5)), inp(b.action_masks(), 0x1F)
    out = b.alloc_sample(True, True)
    fill_bytes(*tensors(out))
    return Plan([logits, masks], lambda: tensors(b.sample_actions(logits[0], masks[0], out=out)), tensors(out))


@case("mlp_sample_actions", "sim", ["LearnerOps.mlp_sample_actions"])
def _mlp_sample(w, rng):
    import torch

    b = w.batch
    head = b.mlp_head(H)
    obs, masks = inp(b.observe(), 0.0), inp(b.action_masks(), 0x1F)
    out = b.alloc_sample(True, True)
    logits = prefilled((E, N, 5), torch.float32)
    fill_bytes(*tensors(out))
    return Plan([obs, masks] + param_inputs(b, head),
                lambda: tensors(b.mlp_sample_actions(head, obs[0], masks[0], logits_out=logits, out=out)) + [logits],
                tensors(out) + [logits])


# ---- learner: the policy head
def _head_nograd(O: int):
    def setup(w, rng):
        import torch

        b = w.batch
        head = b.mlp_head(H, O=O)
        x = inp(normal(rng, ROWS, head.L))
        y, hidden = prefilled((ROWS, O), torch.float32), prefilled((ROWS, H), torch.float32)

        def call():
            with torch.no_grad():
                return [head(x[0], out=y, hidden_out=hidden), hidden]
        return Plan([x] + param_inputs(b, head), call, [y, hidden])
    return setup


case("head_nograd_actor", "sim", ["MlpHead.forward"])(_head_nograd(5))
case("head_nograd_critic", "sim", ["MlpHead.forward"])(_head_nograd(1))


def _head_grad(O: int, backward: str):
    def setup(w, rng):
        import torch

        b = w.batch
        head = b.mlp_head(H, O=O, backward=backward)
        x, gy = inp(normal(rng, ROWS, head.L)), inp(normal(rng, ROWS, O))
        x[0].requires_grad_(True)

        def call():
            with torch.enable_grad():
                y = head(x[0])
                y.backward(gy[0])
            return [y, x[0].grad, *(p.grad for p in head.parameters())]
        return Plan([x, gy] + param_inputs(b, head), call)
    return setup


case("head_grad_torch_backward", "sim", ["MlpHead.forward"])(_head_grad(5, "torch"))
case("head_grad_device_backward", "sim", ["MlpHead.forward", "LearnerOps.mlp_backward"])(_head_grad(5, "device"))
case("head_grad_device_backward_critic", "sim", ["MlpHead.forward", "LearnerOps.mlp_backward"])(_head_grad(1, "device"))


@case("mlp_backward_out", "sim", ["LearnerOps.mlp_backward"])
def _mlp_backward(w, rng):
    import torch

    b = w.batch
    head = b.mlp_head(H)
    xr = dev(normal(rng, ROWS, head.L))
    hid = torch.empty((ROWS, H), dtype=torch.float32, device="cuda")
    head(xr, hidden_out=hid)
    x, hidden, gy = inp(xr), inp(hid), inp(normal(rng, ROWS, 5))
    out = b.alloc_mlp_backward(head, (ROWS,), want_grad_a=True)
    grads = [out.w1t, out.b1, out.w2, out.b2, out.grad_a]
    fill_bytes(*grads)

    def call():
        b.mlp_backward(head, x[0], hidden[0], gy[0], out=out)
        return grads
    return Plan([x, hidden, gy] + param_inputs(b, head), call, grads)


# ---- learner: stored actions under new logits
def _legal(rng, rows):
    """Actions and masks with every action legal under its mask (bit 4, wait, always set)."""
    a = rng.integers(0, 5, size=(rows,), dtype=np.uint8)
    m = (rng.integers(0, 32, size=(rows,)).astype(np.uint8) | 0x10 | (1 << a)).astype(np.uint8)
    return a, m


@case("evaluate_actions_out", "sim", ["LearnerOps.evaluate_actions"])
def _evaluate(w, rng):
    b = w.batch
    a, m = _legal(rng, ROWS)
    logits, acts, masks = inp(normal(rng, ROWS, 5)), inp(a, 4), inp(m, 0x1F)
    out = b.alloc_evaluate((ROWS,))
    fill_bytes(*tensors(out))
    return Plan([logits, acts, masks], lambda: tensors(b.evaluate_actions(logits[0], acts[0], masks[0], out=out)), tensors(out))


@case("evaluate_actions_autograd", "sim", ["LearnerOps.evaluate_actions", "LearnerOps.evaluate_actions_backward"])
def _evaluate_grad(w, rng):
    import torch

    b = w.batch
    a, m = _legal(rng, ROWS)
    logits, acts, masks = inp(normal(rng, ROWS, 5)), inp(a, 4), inp(m, 0x1F)
    c1, c2 = inp(normal(rng, ROWS)), inp(normal(rng, ROWS))
    logits[0].requires_grad_(True)

    def call():
        with torch.enable_grad():
            r = b.evaluate_actions(logits[0], acts[0], masks[0])
            g, = torch.autograd.grad((c1[0] * r.logp + c2[0] * r.entropy).sum(), logits[0])
        return [r.logp, r.entropy, g]
    return Plan([logits, acts, masks, c1, c2], call)


@case("evaluate_actions_backward_out", "sim", ["LearnerOps.evaluate_actions_backward"])
def _evaluate_backward(w, rng):
    import torch

    b = w.batch
    a, m = _legal(rng, ROWS)
    logits, acts, masks = inp(normal(rng, ROWS, 5)), inp(a, 4), inp(m, 0x1F)
    glp, gent = inp(normal(rng, ROWS)), inp(normal(rng, ROWS))
    out = prefilled((ROWS, 5), torch.float32)
    return Plan([logits, acts, masks, glp, gent],
                lambda: [b.evaluate_actions_backward(logits[0], acts[0], masks[0], glp[0], gent[0], out=out)], [out])


# ---- learner: the PPO loss
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, adv_eps=1e-8)


def _ppo_inputs(rng):
    a, m = _legal(rng, ROWS)
    kw = dict(logits=inp(normal(rng, ROWS, 5)), values=inp(normal(rng, ROWS)), actions=inp(a, 4),
              logp_old=inp(-np.abs(normal(rng, ROWS))), advantages=inp(normal(rng, ROWS)), returns=inp(normal(rng, ROWS)),
              masks=inp(m, 0x1F), valid=inp((rng.random(ROWS) < 0.7).astype(np.uint8), 1),
              norm=inp(np.array([7.0, 0.125, 0.75, 0.0], np.float32), dev(np.array([0.0, 0.0, 1.0, 0.0], np.float32))))
    return kw, {k: v[0] for k, v in kw.items()}, {k: v[1] for k, v in kw.items()}


@case("masked_moments", "sim", ["LearnerOps.masked_moments"])
def _moments(w, rng):
    import torch

    b = w.batch
    x, valid = inp(normal(rng, ROWS)), inp((rng.random(ROWS) < 0.7).astype(np.uint8), 1)
    out, ws = prefilled((4,), torch.float32), b.alloc_ppo_loss((ROWS,)).workspace
    return Plan([x, valid], lambda: [b.masked_moments(x[0], valid[0], out=out, workspace=ws)], [out])


@case("ppo_loss_out", "sim", ["LearnerOps.ppo_loss"])
def _ppo(w, rng):
    b = w.batch
    kw, bufs, _ = _ppo_inputs(rng)
    out = b.alloc_ppo_loss((ROWS,))
    fill_bytes(out.stats)
    return Plan(list(kw.values()), lambda: [b.ppo_loss(**bufs, **HYPER, out=out).stats], [out.stats])


@case("ppo_loss_autograd", "sim", ["LearnerOps.ppo_loss", "LearnerOps.ppo_loss_backward"])
def _ppo_grad(w, rng):
    import torch

    b = w.batch
    kw, bufs, _ = _ppo_inputs(rng)
    bufs["logits"].requires_grad_(True)
    bufs["values"].requires_grad_(True)

    def call():
        with torch.enable_grad():
            r = b.ppo_loss(**bufs, **HYPER)
            r.loss.backward()
        return [r.stats, bufs["logits"].grad, bufs["values"].grad]
    return Plan(list(kw.values()), call)


@case("ppo_loss_backward_out", "sim", ["LearnerOps.ppo_loss_backward"])
def _ppo_backward(w, rng):
    b = w.batch
    kw, bufs, reals = _ppo_inputs(rng)
    # the forward's stats are an input of the backward: the stale ones belong to the stale inputs (a legal pair)
    stats = inp(b.ppo_loss(**reals, **HYPER).stats, b.ppo_loss(**bufs, **HYPER).stats.clone())
    gloss = inp(np.array([-1.75], np.float32), 1.0)
    out = b.alloc_ppo_loss((ROWS,))
    grads = [out.grad_logits, out.grad_values]
    fill_bytes(*grads)
    return Plan(list(kw.values()) + [stats, gloss],
                lambda: list(b.ppo_loss_backward(**bufs, **HYPER, stats=stats[0], grad_loss=gloss[0], out=out)), grads)


# ---- learner: the optimiser
def _adam(set_lr: bool):
    def setup(w, rng):
        b = w.batch
        params = [p for head in (b.mlp_head(H), b.mlp_head(H, O=1)) for p in head.parameters()]
        opt = b.adam(params, lr=1e-2, weight_decay=0.01, max_grad_norm=0.5)
        grads = [inp(normal(rng, *p.shape)) for p in params]
        state = [*params, *opt.m, *opt.v, opt.stats, opt.state]

        def call():
            if set_lr:
                opt.lr = 3e-3
            opt.step(grads=[g[0] for g in grads])
            return state
        return Plan(grads, call)
    return setup


case("adam_step_grads", "sim", ["DeviceAdam.step"])(_adam(False))
case("adam_lr_then_step", "sim", ["DeviceAdam.lr", "DeviceAdam.step"])(_adam(True))


# Public methods that reach the library and are NOT in the table, each with its reason: host-synchronous (the call returns
# after the handle's stream has drained, or it reads back to the host), query only, or setting only (a host-side field of
# the handle; no device work).
_SYNC, _QUERY, _SET = "host-synchronous", "query only", "setting only"
EXEMPT = {
    "BatchedCollectiveCrossing.close": _SYNC,
    "BatchedCollectiveCrossing.set_state": _SYNC,
    "BatchedCollectiveCrossing.get_state": _SYNC,
    "BatchedCollectiveCrossing.reset": _SYNC + " (the placement reports failures to the host); its observe() is in the table",
    "BatchedCollectiveCrossing.reset_host": _SYNC + " (set_state); its observe() is in the table",
    "BatchedCollectiveCrossing.set_reset_pool": _SET + " (the pointer; the pool tensor is ordered for later launches)",
    "BatchedCollectiveCrossing.make_reset_pool": _SYNC,
    "BatchedCollectiveCrossing.masks_fused": _QUERY,
    "BatchedCollectiveCrossing.reset_obs_fused": _QUERY,
    "BatchedCollectiveCrossing.step_final_buffers": "allocation on torch's current stream; step_finish orders it",
    "BatchedCollectiveCrossing.track_episodes": _SYNC,
    "BatchedCollectiveCrossing.episode_stats_launches": _QUERY,
    "BatchedCollectiveCrossing.finished_episodes": _SYNC,
    "BatchedCollectiveCrossing.set_rng_seed": _SET,
    "BatchedCollectiveCrossing.set_policy_epsilon": _SET,
    "BatchedCollectiveCrossing.set_policy_stream": _SYNC,
    "BatchedCollectiveCrossing.policy_stream_state": _SYNC,
    "BatchedCollectiveCrossing.counters": _SYNC,
    "BatchedCollectiveCrossing.set_check_inputs": _SET,
    "BatchedCollectiveCrossing.check_inputs": _SYNC,
    "BatchedCollectiveCrossing.set_tunable": _SET,
    "BatchedCollectiveCrossing.set_step_pace_start": _SET,
    "BatchedCollectiveCrossing.pace_start": _QUERY,
    "BatchedCollectiveCrossing.set_pace_calibration": _SET,
    "BatchedCollectiveCrossing.set_timing": _SET,
    "BatchedCollectiveCrossing.last_launch_ms": _SYNC,
    "BatchedCollectiveCrossing.set_launch_shape": _SET,
    "BatchedCollectiveCrossing.set_writers": _SET,
    "BatchedCollectiveCrossing.set_store_throttle": _SET,
    "BatchedCollectiveCrossing.set_step_pace": _SET,
    "BatchedCollectiveCrossing.step_pace_ns": _SYNC,
    "BatchedCollectiveCrossing.pace_state": _SYNC,
    "BatchedCollectiveCrossing.launch_shape": _QUERY,
    "BatchedCollectiveCrossing.set_reward_table": _SYNC,
    "BatchedCollectiveCrossing.set_terminated_table": _SYNC,
    "BatchedCollectiveCrossing.step_shape": _QUERY,
    "BatchedCollectiveCrossing.use_stream": _SYNC,
    "BatchedCollectiveCrossing.synchronize": _SYNC,
    "LearnerOps.alloc_mlp_backward": _QUERY + " (the workspace size) and allocation",
    "LearnerOps.alloc_ppo_loss": _QUERY + " (the workspace size) and allocation",
    "LearnerOps.adam": _QUERY + " (the workspace size) and allocation: DeviceAdam's constructor",
    "DeviceAdam.counts": _SYNC,
    "DeviceAdam.state_dict": "copies on torch's current stream behind a wait for the handle's stream; the values go to the host",
    "DeviceAdam.load_state_dict": "copies on torch's current stream behind a wait for the handle's stream; its lr is in the table",
}


# ----------------------------------------------------------------------------------------------------- the completeness walk
def _classes():
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.learner import DeviceAdam, LearnerOps, MlpHead

    return {"BatchedCollectiveCrossing": BatchedCollectiveCrossing, "LearnerOps": LearnerOps, "MlpHead": MlpHead,
            "DeviceAdam": DeviceAdam}


_DIRECT = re.compile(r"\b(?:self|b|batch)\._lib\.ccx_\w+|\b_(?:MlpForward|EvaluateActions|PpoLoss)\.apply\(")
_CALL_SELF = re.compile(r"\bself\.(\w+)\b")
_CALL_BATCH = re.compile(r"\b(?:b|batch|self\.batch)\.(\w+)\b")


def _functions(cls) -> dict:
    """name -> source of every function, property and static method the class itself defines."""
    out = {}
    for name, obj in vars(cls).items():
        if isinstance(obj, (staticmethod, classmethod)):
            obj = obj.__func__
        if isinstance(obj, property):
            src = "".join(inspect.getsource(f) for f in (obj.fget, obj.fset) if f is not None and f.__name__ != "<lambda>")
            if src:
                out[name] = src
        elif inspect.isfunction(obj) and obj.__name__ != "<lambda>":
            out[name] = inspect.getsource(obj)
    return out


def enqueueing_methods() -> set:
    """``Class.method`` of every public method (or property) of the four classes whose source calls into the library
    (``self._lib.ccx_*`` / ``b._lib.ccx_*``, or one of the autograd Functions), directly or through another method of
    these classes, public or private."""
    classes = _classes()
    src = {c: _functions(cls) for c, cls in classes.items()}
    batch_side = {**src["LearnerOps"], **src["BatchedCollectiveCrossing"]}      # (one object: the batch)

    def scope(c):
        return batch_side if c in ("LearnerOps", "BatchedCollectiveCrossing") else src[c]

    reaches: dict = {}

    def reach(c, name, seen) -> bool:
        key = ("batch" if scope(c) is batch_side else c, name)
        if key in reaches:
            return reaches[key]
        if key in seen or name not in scope(c):
            return False
        seen = seen | {key}
        text = scope(c)[name]
        hit = bool(_DIRECT.search(text))
        hit = hit or any(reach(c, n, seen) for n in set(_CALL_SELF.findall(text)) if n != name)
        hit = hit or any(reach("BatchedCollectiveCrossing", n, seen) for n in set(_CALL_BATCH.findall(text)))
        if len(seen) == 1:
            reaches[key] = hit
        return hit

    return {f"{c}.{name}" for c in classes for name in src[c] if not name.startswith("_") and reach(c, name, frozenset())}


def covered() -> set:
    return {m for c in CASES for m in c.covers}
