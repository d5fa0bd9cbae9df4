"""Shared by test_fit_windows_host.py / test_fit_windows_gpu.py: replay contents made of episodes, and the validity rule
of a trajectory window written out push by push (the reference the replay's ``sample_windows`` is checked against).

Inside an episode ``next_obs[j] == obs[j+1]`` bit for bit; every other observation is distinct (a counter feeds every
entry), so a window is continuous exactly where it stays inside one episode of one lane."""
import numpy as np

EPISODES_OPEN = (7, 5, 9, 4, 11)               # 36 pushes into capacity 64: not wrapped;  H = 3, stride 1 -> 26 valid starts
EPISODES_FULL = (7, 5, 9, 4, 11, 6, 8)         # 50 pushes into capacity 40: full ring, position 10;         -> 28 valid starts
CASES = {"open": (64, EPISODES_OPEN, 26), "full": (40, EPISODES_FULL, 28)}


def episode_obs(lengths, obs_dim, lanes=1):
    """(obs, next_obs) float32 arrays in push order for ``lanes`` interleaved lanes, each running the episodes
    ``lengths`` (lane l's lengths rotated by l, so the lanes' resets do not coincide).  Push p belongs to lane p % lanes."""
    counter = [0]

    def fresh():
        counter[0] += 1
        return (counter[0] * 0.37 + 0.01 * np.arange(obs_dim)).astype(np.float32)
    per_lane = []
    for lane in range(lanes):
        ls = list(lengths[lane:]) + list(lengths[:lane])
        o, no = [], []
        for n in ls:
            cur = fresh()
            for _ in range(n):
                nxt = fresh()
                o.append(cur)
                no.append(nxt)
                cur = nxt
        per_lane.append((o, no))
    total = sum(lengths)
    obs = np.stack([per_lane[p % lanes][0][p // lanes] for p in range(total * lanes)])
    nobs = np.stack([per_lane[p % lanes][1][p // lanes] for p in range(total * lanes)])
    return obs, nobs


def ref_windows(obs, nobs, cap, starts, H, stride):
    """Push by push: for every start ring row, the pushes (H, n) its window reads (clamped at the newest push where the
    window runs past it) and whether the window is valid.  ``obs`` / ``nobs``: all P pushes in push order; the ring keeps
    the last min(P, cap) of them, push p at ring row p % cap."""
    P = len(obs)
    first = max(0, P - cap)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
    pushes = np.zeros((H, len(starts)), dtype=np.int64)
    valid = np.zeros(len(starts), dtype=bool)
    for i, r in enumerate(starts):
        p = first + ((int(r) - first) % cap)
        assert first <= p < P and p % cap == int(r)
        ok = p + (H - 1) * stride <= P - 1
        for k in range(H):
            pushes[k, i] = min(p + k * stride, P - 1)
        for k in range(H - 1):
            ok = ok and bool((bits(nobs[pushes[k, i]]) == bits(obs[pushes[k + 1, i]])).all())
        valid[i] = ok
    return pushes, valid
