"""GPU: examples/alphazero_selfplay.py runs -- the ring fills, the loss is finite, a few seconds."""
import importlib.util
import math
import os

import pytest

pytestmark = pytest.mark.gpu


def test_the_self_play_example_trains_for_a_few_steps():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "alphazero_selfplay.py")
    spec = importlib.util.spec_from_file_location("alphazero_selfplay", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, play = mod.train(kind=2, envs=32, steps=5, moves=3, iterations=4, paths=2, nodes=64, batch=64, capacity=8)
    assert len(losses) == 5 and all(math.isfinite(x) for x in losses)
    assert play.moves == 15 and play.valid_moves() == 8 and len(play) == 8 * 32      # the ring wrapped and is full
    pi = play.pi.sum(2)
    assert bool(((pi - 1).abs() < 1e-5).all())                        # every stored policy target is a distribution: every root was searched
    assert bool(play.z.isfinite().all())
