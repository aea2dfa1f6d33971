"""LaneStates -- saved env states of a batch, on the device (include/sfmi.h: sf_save_lanes / sf_load_lanes).

A row is SF_LANE_STATE_BYTES of one env's whole game state, independent of the lane and tile it came from: any row loads
into any lane of a batch with the same preset, seed and spawn table (its 16-byte header says which; a row from another
batch is refused on the device and its lane left alone).  Not in a row: the batch's episode accumulators, the sticky
overflow count, the action sampler, VecNormalize's statistics, the frame stacks and rollout storage of the wrappers (caller
data: index those tensors the same way).
"""
import numpy as np
import torch

from . import _lib


class LaneStates:
    """`rows`: uint8 [n, LANE_STATE_BYTES] (device or host); metadata of the batch the rows came from.  `.to(device)` moves
    them, `states[i]` / `states[idx]` picks rows, `torch.save(states, path)` / `torch.load(path, weights_only=False)` or
    `save(path)` / `LaneStates.load(path)` (plain tensors and ints: a weights-only load) keep them."""

    def __init__(self, rows, gametype, seed, spawn_table_len, version=_lib.LANE_STATE_VERSION, build_id=""):
        if rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != _lib.LANE_STATE_BYTES:
            raise ValueError("LaneStates: rows must be uint8 [n, %d]" % _lib.LANE_STATE_BYTES)
        self.rows = rows
        self.gametype = gametype
        self.seed = int(seed)
        self.spawn_table_len = int(spawn_table_len)
        self.version = int(version)
        self.build_id = build_id

    def _with(self, rows):
        return LaneStates(rows, self.gametype, self.seed, self.spawn_table_len, self.version, self.build_id)

    def __len__(self):
        return self.rows.shape[0]

    def __getitem__(self, idx):
        rows = self.rows[idx]
        return self._with(rows.unsqueeze(0) if rows.dim() == 1 else rows.contiguous())

    @property
    def device(self):
        return self.rows.device

    def to(self, device, non_blocking=False):
        return self._with(self.rows.to(device, non_blocking=non_blocking))

    def cpu(self):
        return self.to("cpu")

    def headers(self):
        """The rows' headers as numpy uint32 [n, 4]: magic | version, preset (bit 0 autoturn, bit 1 shaped), seed, table length
        (synchronises)."""
        return self.rows[:, :16].cpu().numpy().copy().view(np.uint32)

    def state_dict(self):
        return {"rows": self.rows, "gametype": self.gametype, "seed": self.seed, "spawn_table_len": self.spawn_table_len,
                "version": self.version, "build_id": self.build_id}

    @classmethod
    def from_state_dict(cls, d):
        return cls(d["rows"], d["gametype"], d["seed"], d["spawn_table_len"], d["version"], d["build_id"])

    def save(self, path):
        torch.save(self.state_dict(), path)

    @classmethod
    def load(cls, path, map_location=None):
        return cls.from_state_dict(torch.load(path, map_location=map_location, weights_only=True))

    def __repr__(self):
        return "LaneStates(%d rows, %s, seed %d, table %d, device %s)" % (len(self), self.gametype, self.seed, self.spawn_table_len,
                                                                         self.device)
