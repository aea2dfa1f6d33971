"""A numpy model of the episode log (sfmi.h: sf_eplog_*) with the masked restart of sf_eplog_restart_where: four running
sums per env, a record per set byte of `done` in (row, env) order."""
import numpy as np


class EpisodeLogModel:
    def __init__(self, n, fire_action=1):
        self.n, self.fire_action = int(n), int(fire_action)
        self.acc = np.zeros((4, self.n), np.int64)  # return, length, kills, fire actions
        self.rows_seen = 0
        self.records = []  # (env, return, length, kills, fire actions, end_row)

    def update(self, rew, done, info, actions=None):
        rew, done, info = (np.asarray(x).reshape(-1, self.n) for x in (rew, done, info))
        act = None if actions is None else np.asarray(actions).reshape(-1, self.n)
        for k in range(rew.shape[0]):
            self.acc[0] += rew[k]
            self.acc[1] += 1
            self.acc[2] += info[k] != 0
            if act is not None:
                self.acc[3] += act[k] == self.fire_action
            for e in np.flatnonzero(done[k]):
                self.records.append((int(e),) + tuple(int(v) for v in self.acc[:, e]) + (self.rows_seen + k,))
                self.acc[:, e] = 0
        self.rows_seen += rew.shape[0]

    def restart_where(self, mask):
        self.acc[:, np.asarray(mask).reshape(-1) != 0] = 0

    def as_arrays(self):
        r = np.array(self.records, np.int64).reshape(-1, 6)
        return dict(env=r[:, 0], episode_return=r[:, 1], length=r[:, 2], kills=r[:, 3], fire_actions=r[:, 4], end_row=r[:, 5])
