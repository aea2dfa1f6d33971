"""TEST INFRASTRUCTURE ONLY -- the reference of the action repeat (include/sfmi_repeat.h: sf_step_repeat).

The oracle driven ONE ENV AT A TIME through the contract's loop, as a vec-env worker behind a skip wrapper drives SSF_Env:

    total, kill, ticks = 0, False, 0
    for j in range(K):
        obs, r, done, kill_j = env.step(a)
        total += r; kill |= kill_j; ticks += 1
        if done:
            final = obs; obs = env.reset(); break
    return obs, total, done, kill, ticks

Start state: lockstep.fuzz_crowded, then lane i finishes after 1 + i % 41 more ticks (time = 180000 - 34 f), every 7th
lane nowhere near its end (time = 3400).  T = 48 ticks of wall budget, so 48 / K windows.  A run is computed once per argument
tuple and shared (functools.lru_cache); nobody writes into what it returns.
"""
import ctypes as C
import functools

import numpy as np

T_TICKS = 48
KS = (1, 2, 3, 4, 16)


def start_state(gametype, n, finish=None):
    """-> (base snapshots, prev_vlner, rng).  finish: the ticks lane 0 still plays (n = 1: lane 0 is a 7th lane otherwise)."""
    from oracle import oracle as O
    from lockstep import fuzz_crowded

    rng = np.random.default_rng([23, len(gametype), n])
    base, pv = fuzz_crowded(O, gametype, n, rng)
    f = 1 + np.arange(n) % 41
    base["time"] = 180000 - 34 * f
    base["time"][::7] = 3400
    if finish is not None:
        base["time"][0] = 180000 - 34 * int(finish)
    base["tick"] = base["time"] // 34
    return base, pv, rng


def run_windows(gametype, n, K, base, pv, acts, obs_type="features", faithful=True):
    """The loop above on a given start and actions uint8 [W, n] -> dict: obs float64 [W, n, D] (what the wrapper returns), rew
    int32, done, info bool, ticks uint8 [W, n], final float64 [W, n, D] (the finished game's last observation, NaN elsewhere),
    ep_returns / ep_kills (one entry per finished episode: the sums over its played ticks since the start), snaps."""
    from oracle import oracle as O

    orc = O.OracleVecEnv(gametype, n, obs_type=obs_type)
    orc.load_snapshots(base, pv)
    L = orc.L
    hs = [L.sfo_vec_env_at(orc.h, i) for i in range(n)]
    for h in hs:
        L.sfo_env_set_faithful_bugs(h, int(faithful))
    D, W = orc.obs_dim, acts.shape[0]
    obs = np.empty((W, n, D), np.float64)
    final = np.full((W, n, D), np.nan)
    rew, ticks = np.zeros((W, n), np.int32), np.zeros((W, n), np.uint8)
    done, info = np.zeros((W, n), bool), np.zeros((W, n), bool)
    r, d, k = C.c_int(), C.c_int(), C.c_int()
    row = np.empty(D, np.float64)
    rp = row.ctypes.data_as(C.c_void_p)
    run_ret, run_kill = np.zeros(n, np.int64), np.zeros(n, np.int64)
    ep_returns, ep_kills = [], []
    for w in range(W):
        for i, h in enumerate(hs):
            for j in range(K):
                assert L.sfo_env_step(h, int(acts[w, i]), rp, C.byref(r), C.byref(d), C.byref(k)) == 0
                rew[w, i] += r.value
                info[w, i] |= bool(k.value)
                ticks[w, i] += 1
                run_ret[i] += r.value
                run_kill[i] += int(bool(k.value))
                if d.value:
                    final[w, i] = row
                    L.sfo_env_reset(h, rp)  # the worker's env.reset()
                    done[w, i] = True
                    ep_returns.append(int(run_ret[i]))
                    ep_kills.append(int(run_kill[i]))
                    run_ret[i] = run_kill[i] = 0
                    break
            obs[w, i] = row
    out = dict(base=base, pv=pv, acts=acts, K=K, obs=obs, rew=rew, done=done, info=info, ticks=ticks, final=final,
               ep_returns=np.array(ep_returns, np.int64), ep_kills=np.array(ep_kills, np.int64), snaps=orc.snapshots(), D=D)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_windows(gametype, n, K, obs_type="features", faithful=True, finish=None, T=T_TICKS):
    """The constructed run: T // K windows of K.  Asserts its own conditions on the oracle alone."""
    assert T % K == 0
    base, pv, rng = start_state(gametype, n, finish)
    from oracle import oracle as O

    one = O.OracleVecEnv(gametype, 1)
    n_act = one.L.sfo_env_n_actions(one.L.sfo_vec_env_at(one.h, 0))
    acts = rng.integers(0, n_act, (T // K, n)).astype(np.uint8)
    run = run_windows(gametype, n, K, base, pv, acts, obs_type, faithful)
    check_conditions(run, n, K, finish)
    return run


def check_conditions(run, n, K, finish=None):
    done, ticks = run["done"], run["ticks"]
    assert done.sum(0).max() <= 1, "a lane finished twice"
    if finish is None:
        assert done.sum() >= n - -(-n // 7), (n, K, int(done.sum()))
    else:
        assert done[:, 0].sum() == 1 and ticks[done[:, 0], 0] == (int(finish) - 1) % K + 1
    if n >= 63:
        assert set(ticks[done].tolist()) == set(range(1, K + 1)), (n, K, sorted(set(ticks[done].tolist())))
    assert (ticks[~done] == K).all() and int(ticks.sum()) == int(np.where(done, ticks, K).sum())


def expected_stats(run):
    """-> the six of sf_episode_stats' words the run determines: episodes, sum of returns, of their squares, kills, min, max"""
    r, k = run["ep_returns"], run["ep_kills"]
    return dict(episodes=len(r), ret=int(r.sum()), ret2=int((r ** 2).sum()), kills=int(k.sum()),
                lo=int(r.min()) if len(r) else None, hi=int(r.max()) if len(r) else None)


def final_rows(run, upto=None):
    """-> (rows float64 [n, D], finished bool [n]): every lane's final observation after windows 0 .. upto (default: all)"""
    W = run["done"].shape[0] if upto is None else upto + 1
    n, D = run["done"].shape[1], run["D"]
    rows, fin = np.full((n, D), np.nan), np.zeros(n, bool)
    for w in range(W):
        d = run["done"][w]
        rows[d] = run["final"][w][d]
        fin |= d
    return rows, fin
