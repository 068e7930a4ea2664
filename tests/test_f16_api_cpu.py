"""The one-term fp16 mode's Python surface, without a GPU: the constant
equals the header's define, ConfigSelfPlay.conv_algo defaults to the exact
arithmetic, and the self-play drop-in passes it to both engines and keeps it
in their cache keys (a changed value builds a new engine)."""
import os
import re

import pytest

from custom_alphazero import engine as az
from custom_alphazero import self_play
from custom_alphazero.config import ConfigSelfPlay
from custom_alphazero.mcts.mcts import SyntheticEvaluator

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constant_is_the_headers():
    text = open(os.path.join(REPO, "include", "az.h")).read()
    assert az.CONV_F16 == 3 == int(re.search(r"#define AZ_CONV_F16 (\d+)", text).group(1))
    assert int(re.search(r"#define AZ_ABI_VERSION (\d+)", text).group(1)) == 10


def test_config_defaults_to_the_exact_arithmetic():
    assert ConfigSelfPlay.conv_algo == 0 == az.CONV_F16X2


class Recorder:
    made = []

    def __init__(self, *a, **kw):
        self.kw = kw
        Recorder.made.append(self)


@pytest.fixture
def recorders(monkeypatch):
    Recorder.made = []
    monkeypatch.setattr(az, "Engine", Recorder)
    monkeypatch.setattr(az, "ChessEngine", Recorder)
    monkeypatch.setattr(self_play, "_ENGINES", {})
    monkeypatch.setattr(self_play, "_CHESS_ENGINES", {})
    return Recorder


@pytest.mark.parametrize("build", ["_batched_engine", "_chess_engine"])
def test_selfplay_engines_take_conv_algo_from_the_config(recorders, monkeypatch, build):
    make = lambda: getattr(self_play, build)(SyntheticEvaluator(), 4, 8)  # noqa: E731
    first = make()
    assert first.kw["conv_algo"] == 0 and make() is first  # cached under the same key
    monkeypatch.setattr(ConfigSelfPlay, "conv_algo", az.CONV_F16)
    second = make()
    assert second is not first and second.kw["conv_algo"] == az.CONV_F16
    assert make() is second and len(recorders.made) == 2
