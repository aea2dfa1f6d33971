"""CPU: the reference runs of the final-observation tests (tests/finalobsref.py) meet those tests' own condition on the oracle
alone -- for the seeds chosen, every lane but each 7th finishes inside the run, exactly once -- and the row kept at a finish is
the finished game's, not the new game's."""
import numpy as np
import pytest

import finalobsref as F

pytest.importorskip("torch")  # (finalobsref builds its start states with test_gpu_parity's generator, which imports it)


@pytest.mark.parametrize("gametype", ["youturn", "autoturn", "test-youturn"])
@pytest.mark.parametrize("n", [1, 63, 65, 128, 130])
def test_oracle_runs_finish_where_the_tests_need_them(oracle_mod, n, gametype):
    for obs_type in ("features", "normalized-features", "monitors"):
        for faithful in (True, False):
            if n == 128 and (gametype, obs_type, faithful) != ("youturn", "features", True):
                continue  # (the one configuration the GPU tests use at this size)
            run = F.oracle_run(gametype, n, obs_type, faithful)
            done = run["done"]
            assert done.sum() == n - -(-n // 7) and done.sum(0).max() <= 1
            assert not done[:, ::7].any() and done[:, np.arange(n) % 7 != 0].any(0).all()
            assert done[-6:].sum() == 0  # the last finish lies at least six ticks before the end
            rows, fin = F.final_rows(run)
            assert np.array_equal(fin, done.any(0)) and np.isfinite(rows[fin]).all() and np.isnan(rows[~fin]).all()
            t, i = np.nonzero(done)
            # a finishing step returns the NEW game's row: the kept row is another one (ten two-valued monitors may coincide)
            if obs_type != "monitors":
                assert (np.abs(run["final"][t, i] - run["obs"][t, i]).max(1) > 0).all()
            assert np.isnan(run["final"][~done]).all()
