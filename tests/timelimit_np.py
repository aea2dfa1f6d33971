"""TEST INFRASTRUCTURE ONLY -- the numpy statement of the time limit's bootstrap (sfmi.h: sf_compute_returns_tl).

Every episode of the game ends by the clock, so a zero in masks[t + 1] is a truncation: the reward of that step is read as
rewards[t] + gamma * V(final observation) and the rest is the reference's recursion, untouched (tests/trainerref.py ->
oracle/trainer_np.py).  float32: gamma rounded once, one multiply, then one add; a SELECT on the mask, so the final_value of
an env that never finished cannot leak into anything.
"""
import numpy as np

import trainerref as TR

f32 = np.float32


def rewards2(rewards, masks, final_value, gamma):
    """rewards [T][n], masks [T+1][n], final_value [n] (float32) -> rewards with the bootstrap added where masks[t+1] == 0"""
    assert rewards.dtype == f32 and masks.dtype == f32 and final_value.dtype == f32
    with np.errstate(all="ignore"):
        boot = f32(gamma) * final_value            # one float32 multiply per env
        return np.where(masks[1:] == 0, rewards + boot[None, :], rewards).astype(f32)


def compute_returns_tl(rewards, value_preds, masks, next_value, final_value, use_gae, gamma, tau):
    """-> (returns [T+1][n], value_preds as the reference leaves them): TR.compute_returns on rewards2"""
    return TR.compute_returns(rewards2(rewards, masks, final_value, gamma), value_preds, masks, next_value, use_gae, gamma, tau)


def torch_compute_returns_tl(rewards, value_preds, masks, next_value, final_value, use_gae, gamma, tau):
    """The same through torch CPU tensors: torch.where and TR.torch_compute_returns (the reference's own expressions)"""
    import torch
    r, m, fv = torch.from_numpy(rewards.copy()), torch.from_numpy(masks.copy()), torch.from_numpy(final_value.copy())
    g32 = torch.tensor(gamma, dtype=torch.float32)
    r2 = torch.where(m[1:] == 0, r + g32 * fv, r)
    return TR.torch_compute_returns(r2.numpy(), value_preds, masks, next_value, use_gae, gamma, tau)


def gen_final_value(kind, n, seed=0):
    return TR.gen_values(kind, (n,), seed, 3)


def finished(masks):
    """[n] bool: the envs with a zero in masks[1:]"""
    return (masks[1:] == 0).any(0)
