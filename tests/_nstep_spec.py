"""CCX_NSTEP (include/ccx.h) restated in Python integers and NumPy f64 over the ring's arrays, independent of the library:
``cut_push_spec`` / ``mark_cut_spec`` (the cut bytes), ``window_spec`` (one record's window, the header's rule line by line)
and ``nstep_fetch_spec`` (records to an n-step minibatch).  A SECOND, independent statement, ``brute_force``, computes the
same outputs from a rollout's own ``[K, E, N]`` arrays by walking steps and flags directly -- no slots, no ``head`` -- for
one push of K <= S steps into an empty ring.  The ring itself and the rows are tests/_replay_spec.py's."""

import numpy as np
from _replay_spec import AF_LIVE, AF_TERMINATED, ARRAYS, new_ring, rows_spec

NSTEP_MAX = 16
EF_CUT = 0x01 | 0x02 | 0x04                      # all terminated | all truncated | auto-reset
F32, F64 = np.float32, np.float64


def new_cut(S: int, E: int) -> np.ndarray:
    return np.zeros(S * E, np.uint8)


def cut_push_spec(cut: np.ndarray, head_after: int, S: int, E: int, env_flags) -> None:
    """Behind a push of K steps that left ``head_after``: the cut bytes of the K * E slots it wrote, in place."""
    K = env_flags.shape[0]
    head = max(head_after - K, 0)
    for s in range(K):
        for e in range(E):
            cut[((head + s) % S) * E + e] = 1 if env_flags[s, e] & EF_CUT else 0


def mark_cut_spec(cut: np.ndarray, head: int, S: int, E: int, env_mask=None) -> None:
    if head == 0:
        return
    for e in range(E):
        if env_mask is None or env_mask[e] != 0:
            cut[((head - 1) % S) * E + e] = 1


def avail_spec(head: int, p: int, S: int) -> int:
    if head == 0 or (head < S and p >= head):
        return 0
    return (head - 1 - p) % S


def window_spec(ring: dict, cut: np.ndarray, i: int, n: int, gamma) -> dict:
    """The window of record i in [0, R): per agent G f64, discount f32, span, done, valid; and the env-level m_env / last slot.
    ``why`` names what ended the env's window: "n", "cut" or "avail"."""
    S, E, N = ring["S"], ring["E"], ring["N"]
    head = int(ring["state"][0])
    p, e = i // E, i % E
    slot = [((p + k) % S) * E + e for k in range(n)]
    avail = avail_spec(head, p, S)
    m_env = 1
    while m_env < n and m_env <= avail and cut[slot[m_env - 1]] == 0:
        m_env += 1
    why = "n" if m_env == n else ("avail" if m_env > avail else "cut")
    gd = F64(F32(gamma))
    out = dict(m_env=m_env, why=why, last=slot[m_env - 1], wraps=p + m_env - 1 >= S, reward=np.zeros(N, F64),
               discount=np.zeros(N, F32), span=np.zeros(N, np.uint8), done=np.zeros(N, np.uint8), valid=np.zeros(N, np.uint8),
               dropped=np.zeros(N, bool))
    with np.errstate(all="ignore"):
        for a in range(N):
            m = 1
            while m < m_env and ring["done"][slot[m - 1], a] == 0 and ring["valid"][slot[m], a] != 0:
                m += 1
            g, G = F64(1.0), F64(ring["reward"][slot[0], a])
            for k in range(1, m):
                g = F64(g * gd)
                t = F64(g * F64(ring["reward"][slot[k], a]))
                G = F64(G + t)
            g = F64(g * gd)
            done_out = ring["done"][slot[m - 1], a]
            dropped = m < m_env and done_out == 0
            out["reward"][a], out["discount"][a], out["span"][a] = G, F32(g), m
            out["done"][a], out["dropped"][a] = done_out, dropped
            out["valid"][a] = 0 if dropped else ring["valid"][slot[0], a]
    return out


def nstep_fetch_spec(ring: dict, cut: np.ndarray, index, n: int, gamma, consts, details: bool = False) -> dict:
    """The n-step minibatch of record indices ``index``; the EMPTY record with discount = gamma and span = 1 outside [0, R)."""
    index = np.asarray(index, np.int64)
    B, N = len(index), ring["N"]
    R = ring["S"] * ring["E"]
    empty = new_ring(1, 1, N)
    out = {k: np.repeat(empty[k], B, axis=0) for k in ARRAYS}
    out["discount"] = np.full((B, N), F32(F64(F32(gamma))), F32)
    out["span"] = np.ones((B, N), np.uint8)
    windows = []
    for b, i in enumerate(index.tolist()):
        if not 0 <= i < R:
            windows.append(None)
            continue
        w = window_spec(ring, cut, i, n, gamma)
        windows.append(w)
        out["obs_c"][b], out["actions"][b] = ring["obs_c"][i], ring["actions"][i]
        out["next_c"][b], out["masks_next"][b] = ring["next_c"][w["last"]], ring["masks_next"][w["last"]]
        for k in ("reward", "done", "valid", "discount", "span"):
            out[k][b] = w[k]
    out["obs"], out["next_obs"] = rows_spec(out.pop("obs_c"), consts), rows_spec(out.pop("next_c"), consts)
    out["index"] = index.copy()
    if details:
        out["windows"] = windows
    return out


def brute_force(reward, agent_flags, env_flags, n: int, gamma) -> dict:
    """The same outputs for every (step, env) of ONE block of K steps pushed into an empty ring of S >= K steps, from the
    rollout's own arrays: a window runs over the following steps of the block until n steps are taken, the step's env flags
    say the episode ended, or the block ends.  Returns arrays [K, E, N] and ``last`` [K, E] (the step the window ends on)."""
    K, E, N = reward.shape
    done = (agent_flags & AF_TERMINATED).astype(np.uint8)
    live = (agent_flags & AF_LIVE).astype(np.uint8)
    gd = F64(F32(gamma))
    out = dict(reward=np.zeros((K, E, N), F64), discount=np.zeros((K, E, N), F32), span=np.zeros((K, E, N), np.uint8),
               done=np.zeros((K, E, N), np.uint8), valid=np.zeros((K, E, N), np.uint8), last=np.zeros((K, E), np.int64))
    with np.errstate(all="ignore"):
        for s in range(K):
            for e in range(E):
                steps = [s]                                              # the steps of the env's window
                while len(steps) < n and steps[-1] + 1 < K and not env_flags[steps[-1], e] & EF_CUT:
                    steps.append(steps[-1] + 1)
                out["last"][s, e] = steps[-1]
                for a in range(N):
                    mine = [s]                                           # the agent's share of them
                    for t in steps[1:]:
                        if done[mine[-1], e, a] or not live[t, e, a]:
                            break
                        mine.append(t)
                    G, g = F64(reward[s, e, a]), F64(1.0)
                    for t in mine[1:]:
                        g = F64(g * gd)
                        G = F64(G + F64(g * F64(reward[t, e, a])))
                    stopped_early = len(mine) < len(steps) and not done[mine[-1], e, a]
                    out["reward"][s, e, a], out["discount"][s, e, a] = G, F32(F64(g * gd))
                    out["span"][s, e, a], out["done"][s, e, a] = len(mine), done[mine[-1], e, a]
                    out["valid"][s, e, a] = 0 if stopped_early else live[s, e, a]
    return out
