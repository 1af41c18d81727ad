"""GPU: the two examples run with --prioritized -- prioritised sampling, importance-weighted losses and the priority updates on one
stream, a few seconds -- and leave a tree whose priorities are the ones the training loop stored."""
import math

import numpy as np
import pytest

from devmem import _example

pytestmark = pytest.mark.gpu


def test_the_self_play_example_trains_with_prioritised_replay_and_reanalyse():
    losses, play = _example("alphazero_selfplay").train(kind=2, envs=32, steps=5, moves=3, iterations=4, paths=2, nodes=64, batch=64, capacity=8,
                                                        reanalyse=16, td_steps=3, prioritized=True, per_alpha=0.5, per_beta=0.4)
    assert len(losses) == 5 and all(math.isfinite(x) for x in losses)
    assert play.moves == 15 and len(play) == 8 * 32 and play.tree is not None and play.tree.draw == 10      # a sample and a reanalyse per step
    w = play.tree.weights().cpu().numpy()
    assert w.shape == (8 * 32,) and (w > 0).sum() >= 3 * 32          # the last moves carry the largest priority; the rest what was stored
    assert len(np.unique(w)) > 2 and play.tree.total() == int(w.sum(dtype=np.uint64))
    assert int(play.refreshed.sum()) > 0


def test_the_dqn_example_runs_with_prioritised_replay():
    lines = []
    losses, returns = _example("dqn_batched").run(envs=256, ticks=40, batch=128, replace=20, prefill=16, log=lines.append, prioritized=True)
    assert len(losses) == 40 and all(np.isfinite(losses)) and len(returns) == 2 and len(lines) == 2
