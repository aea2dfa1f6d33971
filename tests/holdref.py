"""TEST INFRASTRUCTURE ONLY -- the reference of the masked step (include/sfmi_hold.h: sf_step_where).

`HoldModel` is one oracle env per lane, driven ONE ENV AT A TIME: a call steps the ACTIVE lanes through the window loop of
sfmi_repeat.h (frameskipref.run_windows' loop; K = 1 is the plain step of the vec-env worker) and does not touch the others:

    for i in lanes:
        if not active[i]:  reward, done, info, ticks = 0; obs = the lane's last row; continue
        total, kill, ticks = 0, False, 0
        for j in range(K):
            obs, r, done, kill_j = env.step(a)
            total += r; kill |= kill_j; ticks += 1
            if done:
                final = obs
                if auto_reset: obs = env.reset()
                break

A held lane's observation is the last row the lane returned; before its first active step it is the oracle's row of the loaded
state, whose bearing columns (features: 6, 7, 8) are the snapshot's own and say nothing of a constructed position: `seen`
tells which lanes have returned a row of their own.

`inert` is the recipe sf_hold_begin_kernel swaps a held lane for, on oracle snapshots (tests/test_hold_model.py plays it).
"""
import ctypes as C

import numpy as np

BEARING_COLUMNS = (6, 7, 8)  # aim, vdir, ndist of the features / normalized-features row
INERT_DEATH = -(1 << 24)


def inert(snaps):
    """Oracle snapshots -> the same games made inert as the device makes a held lane: ship dead and not due back, no missile,
    no shell, time 0, vlner 0, every counter and key timer zero.  (prev_vlner = 0 is the loader's argument.)  Position,
    velocity, headings, key flags, the fortress and the score stay."""
    s = np.array(snaps, copy=True)
    s["ship_alive"] = 0
    s["ship_death_timer"] = INERT_DEATH
    s["missile_alive"] = 0
    s["shell_alive"] = 0
    s["time"] = 0
    s["tick"] = 0
    s["vlner"] = 0
    s["stats"] = 0
    for k in ("fire_timer", "thrust_timer", "left_timer", "right_timer"):
        s[k] = 0
    return s


class HoldModel:
    def __init__(self, gametype, base, pv, obs_type="features", faithful=True, auto_reset=True):
        from oracle import oracle as O

        n = len(base)
        self.n, self.auto_reset = n, auto_reset
        self.orc = O.OracleVecEnv(gametype, n, obs_type=obs_type)
        self.orc.load_snapshots(base, pv)
        self.L = L = self.orc.L
        self.hs = [L.sfo_vec_env_at(self.orc.h, i) for i in range(n)]
        for h in self.hs:
            L.sfo_env_set_faithful_bugs(h, int(faithful))
        self.D = self.orc.obs_dim
        self.n_actions = L.sfo_env_n_actions(self.hs[0])
        self.row = np.empty((n, self.D), np.float64)
        for i, h in enumerate(self.hs):
            L.sfo_env_features(h, self.row[i].ctypes.data_as(C.c_void_p))
        self.seen = np.zeros(n, bool)
        self.steps = np.zeros(n, np.int64)  # active steps each lane has played
        self.run_ret, self.run_kill = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.ep_returns, self.ep_kills = [], []

    def step_where(self, acts, active, K=1):
        """-> dict: obs float64 [n, D], rew int32, done, info bool, ticks uint8 [n], final float64 [n, D] (the finished game's
        last observation where an ACTIVE lane finished in this call, NaN elsewhere)"""
        L, n, D = self.L, self.n, self.D
        rew, ticks = np.zeros(n, np.int32), np.zeros(n, np.uint8)
        done, info = np.zeros(n, bool), np.zeros(n, bool)
        final = np.full((n, D), np.nan)
        r, d, k = C.c_int(), C.c_int(), C.c_int()
        row = np.empty(D, np.float64)
        rp = row.ctypes.data_as(C.c_void_p)
        for i, h in enumerate(self.hs):
            if not active[i]:
                continue
            for j in range(K):
                assert L.sfo_env_step(h, int(acts[i]), rp, C.byref(r), C.byref(d), C.byref(k)) == 0
                rew[i] += r.value
                info[i] |= bool(k.value)
                ticks[i] += 1
                self.run_ret[i] += r.value
                self.run_kill[i] += int(bool(k.value))
                if d.value:
                    done[i] = True
                    if self.auto_reset:
                        final[i] = row
                        L.sfo_env_reset(h, rp)
                        self.ep_returns.append(int(self.run_ret[i]))
                        self.ep_kills.append(int(self.run_kill[i]))
                        self.run_ret[i] = self.run_kill[i] = 0
                        break
            self.row[i] = row
            self.seen[i] = True
            self.steps[i] += 1
        return dict(obs=self.row.copy(), rew=rew, done=done, info=info, ticks=ticks, final=final)

    def snapshots(self):
        return self.orc.snapshots()

    def expected_stats(self):
        """the words of sf_episode_stats the run determines: episodes, sum of returns, of their squares, kills"""
        r, k = np.array(self.ep_returns, np.int64), np.array(self.ep_kills, np.int64)
        return dict(episodes=len(r), ret=int(r.sum()), ret2=int((r ** 2).sum()), kills=int(k.sum()))


def draw_masks(rng, n, T, p_mixed=0.5, stretch=40):
    """The masks of the lock-step test, bool [T, n], for a batch of whole tiles and a partial last one: tile 0 always all
    active; tile 1 held WHOLE for stretches of `stretch` calls, all active in between; every other tile, the partial last
    one included, mixed lane by lane with probability p_mixed per call."""
    m = rng.random((T, n)) < p_mixed
    m[:, :64] = True
    if n > 64:
        on = (np.arange(T) // stretch) % 2 == 1
        m[:, 64:128] = on[:, None]
    return m
