"""CCX_GAE as include/ccx.h states it, restated in NumPy on the CPU, plus a generator of adversarial cases.  TEST
INFRASTRUCTURE ONLY: what the GAE kernel is compared with.

Written from the header paragraph, not from the kernel.  The steps run backwards; within a step every column is advanced at
once with elementwise ``np.float32`` operations (one IEEE binary32 rounding each: no reduction, nothing a library could
reassociate or fuse).  What a step does not read is never touched: operands are gathered with boolean masks into arrays of
+0.0, never multiplied by zero and never passed through an ``np.where`` next to a NaN.  ``gae_scalar`` is the header's
pseudo-code literally, one column at a time with ``np.float32`` scalars.  Every comparison against this module is on bit
patterns."""

from __future__ import annotations

import numpy as np
from _episode_stats_spec import make_trajectory

AF_TERMINATED, AF_TRUNCATED, AF_LIVE = 0x01, 0x02, 0x04
EF_ENDS = 0x01 | 0x02 | 0x04          # ALL_TERMINATED | ALL_TRUNCATED | RESET
F32 = np.float32


def step_classes(agent_flags, env_flags):
    """(live, term, cut, cont) bool [K, E, N]: the four cases of the rule.  term / cut / cont partition the live steps
    (term: AF_TERMINATED; cut: not terminated and the episode is cut; cont: the chain goes on into step s + 1)."""
    af = np.asarray(agent_flags, np.uint8)
    ef = np.asarray(env_flags, np.uint8)[..., None]
    live = (af & AF_LIVE) != 0
    term = live & ((af & AF_TERMINATED) != 0)
    cut = live & ~term & (((af & AF_TRUNCATED) != 0) | ((ef & EF_ENDS) != 0))
    return live, term, cut, live & ~term & ~cut


def gae_spec(reward, agent_flags, env_flags, values, last_values, final_values=None, gamma=0.99, lam=0.95):
    """(advantages f32 [K, E, N], returns f32 [K, E, N], valid u8 [K, E, N])."""
    reward = np.asarray(reward, np.float64)
    values = np.asarray(values, F32)
    last_values = np.asarray(last_values, F32)
    K, E, N = reward.shape
    assert values.shape == agent_flags.shape == (K, E, N) and env_flags.shape == (K, E) and last_values.shape == (E, N)
    live, term, cut, cont = step_classes(agent_flags, env_flags)
    g = F32(gamma)
    gl = F32(g * F32(lam))                                        # one f32 multiply
    adv = np.zeros((K, E, N), F32)
    ret = np.zeros((K, E, N), F32)
    carry = np.zeros((E, N), F32)
    for s in range(K - 1, -1, -1):
        lv, ct, co = live[s], cut[s], cont[s]
        nv = np.zeros((E, N), F32)                                # termination, a cut without final_values: +0.0
        c = np.zeros((E, N), F32)
        if final_values is not None:
            nv[ct] = np.asarray(final_values[s], F32)[ct]
        if s == K - 1:
            nv[co] = last_values[co]
        else:
            nv[co] = values[s + 1][co]
            c[co] = carry[co]
        r = np.zeros((E, N), F32)
        v = np.zeros((E, N), F32)
        r[lv] = reward[s][lv].astype(F32)                         # round to nearest even
        v[lv] = values[s][lv]
        delta = (r + g * nv) - v                                  # mul, add, sub
        a = delta + gl * c                                        # mul, add
        t = a + v
        adv[s][lv] = a[lv]
        ret[s][lv] = t[lv]
        carry = adv[s]                                            # +0.0 where the agent was not live
    return adv, ret, live.astype(np.uint8)


def gae_scalar(reward, agent_flags, env_flags, values, last_values, final_values=None, gamma=0.99, lam=0.95):
    """The header's pseudo-code, column by column, with np.float32 scalars."""
    K, E, N = reward.shape
    g = F32(gamma)
    gl = F32(g * F32(lam))
    zero = F32(0.0)
    adv = np.full((K, E, N), np.nan, F32)
    ret = np.full((K, E, N), np.nan, F32)
    valid = np.full((K, E, N), 255, np.uint8)
    for e in range(E):
        for a in range(N):
            carry = zero
            for s in range(K - 1, -1, -1):
                af, ef = int(agent_flags[s, e, a]), int(env_flags[s, e])
                if not af & AF_LIVE:
                    adv[s, e, a] = ret[s, e, a] = zero
                    valid[s, e, a] = 0
                    carry = zero
                    continue
                v = F32(values[s, e, a])
                r = F32(reward[s, e, a])
                cut = bool(af & AF_TRUNCATED) or bool(ef & EF_ENDS)
                if af & AF_TERMINATED:
                    nv, c = zero, zero
                elif cut:
                    nv, c = (F32(final_values[s, e, a]) if final_values is not None else zero), zero
                elif s == K - 1:
                    nv, c = F32(last_values[e, a]), zero
                else:
                    nv, c = F32(values[s + 1, e, a]), carry
                delta = F32(F32(r + F32(g * nv)) - v)
                x = F32(delta + F32(gl * c))
                adv[s, e, a] = x
                ret[s, e, a] = F32(x + v)
                valid[s, e, a] = 1
                carry = x
    return adv, ret, valid


def bits32(a) -> np.ndarray:
    """f32 as u32 bit patterns for exact comparison (the sign of zero and NaN payloads included)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def make_gae_case(K: int, E: int, N: int, seed: int = 0, with_final: bool = True) -> dict:
    """reward f64, agent_flags u8, env_flags u8, values f32, last_values f32, final_values f32 or None.

    Flags: ``make_trajectory``'s env-flag layouts (never finishing, finishing on step 0 and K - 1, an episode per step,
    raised flags that stay raised, random raises and resets, ...) and its LIVE pattern; AF_TERMINATED (8 %) and AF_TRUNCATED
    (8 %) are set at random, on live and other steps alike.
    Values by column (e * N + a) % 4: 0 and 3 normals of mixed magnitude (1e-3 .. 1e3), 1 subnormals around 1e-40, 2 draws
    from {-0.0, +0.0, 0.5, -1.5}.  Rewards: ``make_trajectory``'s classes (1e16 / 1 / -1e16 patterns, signed zeros, inexact
    values, 1e-300 which rounds to zero), with f32-subnormal magnitudes in the columns whose values are subnormal.
    NaN wherever the rule does not read: reward where not live; values[s] unless step s is live or step s - 1 continues
    into it; final_values except at live, not terminated cut steps; last_values unless step K - 1 continues."""
    rng = np.random.default_rng(seed)
    reward, af, ef = make_trajectory(K, E, N, seed=seed)
    af = af & ~np.uint8(AF_TERMINATED | AF_TRUNCATED)
    af |= np.where(rng.random((K, E, N)) < 0.08, AF_TERMINATED, 0).astype(np.uint8)
    af |= np.where(rng.random((K, E, N)) < 0.08, AF_TRUNCATED, 0).astype(np.uint8)
    live, term, cut, cont = step_classes(af, ef)
    cls = ((np.arange(E)[:, None] * N + np.arange(N)[None, :]) % 4)[None]

    def draw(shape_k):
        shape = (shape_k, E, N)
        normal = rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)
        tiny = rng.standard_normal(shape) * 1e-40
        zeros = rng.choice(np.array([-0.0, 0.0, 0.5, -1.5]), size=shape)
        return np.where(cls == 1, tiny, np.where(cls == 2, zeros, normal)).astype(F32)

    values, finals, last = draw(K), draw(K), draw(1)[0]
    tiny_r = rng.standard_normal((K, E, N)) * 1e-40
    reward = np.where(live & (cls == 1) & (rng.random((K, E, N)) < 0.7), tiny_r, reward)
    read_v = live.copy()
    read_v[1:] |= cont[:-1]
    values[~read_v] = np.nan
    finals[~cut] = np.nan
    last[~cont[K - 1]] = np.nan
    return dict(reward=np.ascontiguousarray(reward), agent_flags=af, env_flags=ef, values=values, last_values=last,
                final_values=finals if with_final else None)
