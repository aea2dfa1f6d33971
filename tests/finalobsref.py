"""TEST INFRASTRUCTURE ONLY -- what the tests of the final-observation output share (sfmi.h: sf_set_final_obs_output).

The reference is the oracle driven ONE ENV AT A TIME, as the vec-env worker drives SSF_Env (rl/train.py:80):
    obs, r, d, i = env.step(a); if d: final = obs; obs = env.reset()
on a constructed batch whose clocks are set as in test_gpu_parity.test_lanes_of_a_tile_finish_at_different_ticks: every lane
finishes at a tick of its own inside the run, every 7th lane nowhere near it.  A run is computed once per (gametype, n,
obs_type, faithful_bugs) and shared (functools.lru_cache); nobody writes into what it returns.
"""
import ctypes as C
import functools

import numpy as np

from lockstep import fuzz_crowded, load_state

T_RUN = 48
SENTINEL_BYTE = 0xA5  # trainerref.guarded's


def set_clocks(base, rng, T):
    """game over (time >= 180000) after 1 .. T-7 more ticks; every 7th lane nowhere near it"""
    n = len(base)
    base["time"] = 180000 - 34 * rng.integers(1, T - 6, n)
    base["time"][::7] = 34 * 100
    base["tick"] = base["time"] // 34


@functools.lru_cache(maxsize=None)
def oracle_run(gametype, n, obs_type="features", faithful=True, T=T_RUN):
    """-> dict: base, pv (the constructed start), acts uint8 [T, n], obs float64 [T, n, D] (what the worker returns: a new
    game's row on done), rew, done, info [T, n], final float64 [T, n, D] (the finished game's last observation at the step it
    finished on, NaN elsewhere), snaps (the oracle's state after the run)."""
    from oracle import oracle as O

    rng = np.random.default_rng([17, len(gametype), n, len(obs_type), int(faithful)])
    base, pv = fuzz_crowded(O, gametype, n, rng)
    set_clocks(base, rng, T)
    orc = O.OracleVecEnv(gametype, n, obs_type=obs_type)
    orc.load_snapshots(base, pv)
    L = orc.L
    hs = [L.sfo_vec_env_at(orc.h, i) for i in range(n)]
    for h in hs:
        L.sfo_env_set_faithful_bugs(h, int(faithful))
    D = orc.obs_dim
    acts = rng.integers(0, L.sfo_env_n_actions(hs[0]), (T, n)).astype(np.uint8)
    obs = np.empty((T, n, D), np.float64)
    final = np.full((T, n, D), np.nan)
    rew, done, info = np.zeros((T, n), np.int32), np.zeros((T, n), bool), np.zeros((T, n), bool)
    r, d, k = C.c_int(), C.c_int(), C.c_int()
    row = np.empty(D, np.float64)
    rp = row.ctypes.data_as(C.c_void_p)
    for t in range(T):
        for i, h in enumerate(hs):
            assert L.sfo_env_step(h, int(acts[t, i]), rp, C.byref(r), C.byref(d), C.byref(k)) == 0
            if d.value:
                final[t, i] = row      # the observation SSF_Env.step returned for the finishing tick
                L.sfo_env_reset(h, rp)  # the worker's env.reset()
            obs[t, i] = row
            rew[t, i], done[t, i], info[t, i] = r.value, bool(d.value), bool(k.value)
    out = dict(base=base, pv=pv, acts=acts, obs=obs, rew=rew, done=done, info=info, final=final, snaps=orc.snapshots(), D=D)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    # the condition of the test, on the oracle alone: enough lanes finish, each once
    assert done.sum(0).max() <= 1 and done.sum() >= n - -(-n // 7), (gametype, n, int(done.sum()))
    return out


def final_rows(run, upto=None):
    """-> (rows float64 [n, D], finished bool [n]): every lane's final observation after steps 0 .. upto (default: all)"""
    T = run["done"].shape[0] if upto is None else upto + 1
    n, D = run["done"].shape[1], run["D"]
    rows, fin = np.full((n, D), np.nan), np.zeros(n, bool)
    for t in range(T):
        d = run["done"][t]
        rows[d] = run["final"][t][d]
        fin |= d
    return rows, fin


def load_env(env, base, pv):
    """the constructed start into a device batch (lockstep.load_both's half)"""
    load_state(env, base, pv)


def make_env(sfa, run, gametype, n, obs_type="features", f64=False, faithful=True, **kw):
    import torch
    env = sfa.SFVecEnv(n, gametype=gametype, obs_type=obs_type, obs_dtype=torch.float64 if f64 else torch.float32,
                       faithful_bugs=faithful, **kw)
    load_env(env, run["base"], run["pv"])
    return env


def is_sentinel(rows):
    """numpy [n, D] of any dtype -> bool [n]: every byte of the row is the sentinel"""
    b = np.ascontiguousarray(rows).view(np.uint8).reshape(rows.shape[0], -1)
    return (b == SENTINEL_BYTE).all(1)
