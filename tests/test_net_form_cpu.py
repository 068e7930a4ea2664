"""The form a network's forward runs in (csrc/az_net_form.h), checked with no
GPU: the library's own rule, az::plan_network through
tests/native/net_form_check.cpp (CUs 256, lanes 1, the network evaluator),
against the table the header states; over every Connect-N shape the tower
takes, the tower exactly where the chooser has a layout, with that layout; and
through the Python binding, each refusal the create calls make before they
open a device."""
import json
import os

import pytest

import forward_ref as fr
from custom_alphazero import engine as az

pytestmark = pytest.mark.skipif(not fr.have_lib(), reason="libaz.so not built")

X2, DIRECT, LAYERS, F16 = az.CONV_F16X2, az.CONV_DIRECT, az.CONV_F16X2_LAYERS, az.CONV_F16
ALGO_TEXT = "conv_algo must be AZ_CONV_F16X2, AZ_CONV_DIRECT, AZ_CONV_F16X2_LAYERS or AZ_CONV_F16"
F16_TEXT = "AZ_CONV_F16 needs the one-launch tower: 1 <= depth <= 16 and value_hidden <= 256"
F16_CHESS_TEXT = "AZ_CONV_F16 needs the one-launch tower: 1 <= depth <= 16"
COLUMNS_TEXT = "AZ_CONV_F16X2_LAYERS supports boards up to 16 columns"
NO_LAYOUT_TEXT = "AZ_CONV_F16 needs the one-launch tower, and this network has no layout for it"


def cn(algo, H, W, depth, hidden=256):
    """A Connect-N request with gravity (A = W)."""
    return (algo, 4, H, W, W, depth, hidden)


def chess(algo, depth, hidden=256):
    return (algo, 118, 8, 8, 1880, depth, hidden)


# request -> (form, terms), or the refusal's text and whether the create call already makes it
TABLE = [
    (cn(X2, 6, 7, 4), ("tower", 3)),
    (cn(F16, 6, 7, 4), ("tower", 1)),
    (cn(DIRECT, 6, 7, 4), ("direct", 3)),
    (cn(LAYERS, 6, 7, 4), ("layers16", 3)),
    (cn(X2, 6, 7, 0), ("direct", 3)),
    (cn(DIRECT, 6, 7, 0), ("direct", 3)),
    (cn(LAYERS, 6, 7, 0), ("direct", 3)),
    (cn(F16, 6, 7, 0), (F16_TEXT, True)),
    (cn(X2, 3, 3, 17), ("layers16", 3)),
    (cn(X2, 2, 20, 17), ("direct", 3)),
    (cn(X2, 3, 3, 1, 300), ("layers16", 3)),
    (cn(F16, 3, 3, 17), (F16_TEXT, True)),
    (cn(F16, 3, 3, 1, 300), (F16_TEXT, True)),
    (cn(X2, 2, 20, 1), ("tower", 3)),  # the tower takes W > 16
    (cn(LAYERS, 2, 20, 1), (COLUMNS_TEXT, True)),
    # outside the engine's limits (128 cells), where the chooser says no
    (cn(X2, 12, 12, 4), ("layers16", 3)),
    (cn(X2, 8, 20, 4), ("direct", 3)),
    (cn(F16, 12, 12, 4), (NO_LAYOUT_TEXT, False)),
    (cn(F16, 8, 20, 4), (NO_LAYOUT_TEXT, False)),
    (chess(X2, 4), ("tower_rows", 3)),
    (chess(F16, 4), ("tower_rows", 1)),
    (chess(LAYERS, 4), ("layers16", 3)),
    (chess(DIRECT, 4), ("direct", 3)),
    (chess(X2, 0), ("direct", 3)),
    (chess(DIRECT, 0), ("direct", 3)),
    (chess(LAYERS, 0), ("direct", 3)),
    (chess(F16, 0), (F16_CHESS_TEXT, True)),
    (chess(X2, 17), ("layers16", 3)),
    (chess(LAYERS, 17), ("layers16", 3)),
    (chess(F16, 17), (F16_CHESS_TEXT, True)),
    (chess(X2, 2, 300), ("tower_rows", 3)),  # no cap on hidden here
    (chess(F16, 2, 300), ("tower_rows", 1)),
    (cn(4, 6, 7, 4), (ALGO_TEXT, True)),
    (cn(-1, 6, 7, 4), (ALGO_TEXT, True)),
    (chess(4, 4), (ALGO_TEXT, True)),
    (chess(-1, 4), (ALGO_TEXT, True)),
]


def test_plan_network_is_the_table(tmp_path):
    args = [str(v) for req, _ in TABLE for v in req]
    rows = json.loads(fr.run_native_check(str(tmp_path), "net_form_check", args))
    assert len(rows) == len(TABLE)
    for (req, want), r in zip(TABLE, rows):
        if isinstance(want[0], str) and want[0] in ("direct", "layers16", "tower", "tower_rows"):
            form, terms = want
            assert (r["status"], r["form"], r["terms"], r["at_create"]) == (0, form, terms, 0), (req, r)
            # the layout is the tower forms' alone, and so is an issued-FLOP figure
            tower = form in ("tower", "tower_rows")
            assert (r["layout"], r["tile_rows"] > 0, r["flop"] > 0) == (tower, tower, tower), (req, r)
        else:
            text, at_create = want
            assert (r["status"], r["message"], r["form"], r["at_create"]) == (-1, text, "refused", at_create), (req, r)
            assert (r["layout"], r["tile_rows"], r["flop"]) == (0, 0, 0), (req, r)


def test_fallback_cases_are_the_forms_their_table_says(tmp_path):
    """tests/forward_ref.py FALLBACK_CASES under the default conv_algo, and the
    explicit algorithm tests/test_forward_forms_gpu.py compares each with."""
    want = {"3x3g_d17_h256": "layers16", "3x3g_d1_h300": "layers16", "2x20g_d17_h256": "direct",
            "3x3g_d0_h256": "direct"}
    assert [c.name for c in fr.FALLBACK_CASES] == list(want)
    explicit = {"layers16": LAYERS, "direct": DIRECT}
    args = [str(v) for c in fr.FALLBACK_CASES for algo in (X2, explicit[want[c.name]])
            for v in (algo, 4, c.H, c.W, fr.action_space(c), c.depth, c.hidden)]
    rows = json.loads(fr.run_native_check(str(tmp_path), "net_form_check", args))
    for c, default, named in zip(fr.FALLBACK_CASES, rows[0::2], rows[1::2]):
        assert default["form"] == named["form"] == want[c.name], (c.name, default, named)


def test_sweep_has_the_tower_exactly_where_the_chooser_has_a_layout(tmp_path):
    """tower_layout_check --sweep's shapes under AZ_CONV_F16X2: the form is the
    tower where tower16_choose_layout says ok, with the chooser's layout (tile
    rows, dbuf, staging, slot plans and skips, issued FLOP of main and alt
    tiles); the shapes without the tower are the golden list's."""
    out = json.loads(fr.run_native_check(str(tmp_path), "net_form_check", ["--sweep"]))
    assert out["shapes"] == 390 * 2 * 3 * 4
    assert out["failures"] == []
    with open(os.path.join(fr.REPO, "tests", "golden", "tower_layout_not_ok.json")) as f:
        assert out["not_ok"] == json.load(f)


def _connect_n(**kw):
    cfg = dict(height=6, width=7, n=4, gravity=True, mcts_iterations=4, slots=2, evaluator=az.EVAL_NETWORK)
    cfg.update(kw)
    return az.Engine(**cfg)


@pytest.mark.parametrize("kw, text", [
    (dict(conv_algo=4), ALGO_TEXT),
    (dict(conv_algo=-1), ALGO_TEXT),
    (dict(conv_algo=F16, depth=0), F16_TEXT),
    (dict(conv_algo=F16, depth=17), F16_TEXT),
    (dict(conv_algo=F16, value_hidden=300), F16_TEXT),
    (dict(conv_algo=LAYERS, height=2, width=20, n=2), COLUMNS_TEXT),
    # the first refusal met stays the same one
    (dict(conv_algo=4, depth=-1), ALGO_TEXT),
    (dict(conv_algo=F16, depth=17, height=2, width=20, n=2), F16_TEXT),
    (dict(conv_algo=LAYERS, height=2, width=20, n=2, evaluator=7), "unknown evaluator"),
    (dict(conv_algo=X2, depth=-1), "need 0 <= depth and value_hidden >= 1"),
])
def test_connect_n_create_refuses_before_it_opens_a_device(kw, text):
    with pytest.raises(az.AzError) as err:
        _connect_n(**kw)
    assert text in str(err.value) and "no HIP device" not in str(err.value), str(err.value)


@pytest.mark.parametrize("kw, text", [
    (dict(conv_algo=4), ALGO_TEXT),
    (dict(conv_algo=-1), ALGO_TEXT),
    (dict(conv_algo=F16, depth=0), F16_CHESS_TEXT),
    (dict(conv_algo=F16, depth=17), F16_CHESS_TEXT),
    (dict(conv_algo=4, evaluator=7), "unknown evaluator"),
    (dict(conv_algo=X2, depth=-1), "negative bound"),
])
def test_chess_create_refuses_before_it_opens_a_device(kw, text):
    with pytest.raises(az.AzError) as err:
        az.ChessEngine(4, slots=2, **kw)
    msg = str(err.value)
    assert text in msg and "no HIP device" not in msg, msg
    if text == F16_CHESS_TEXT:
        assert "value_hidden" not in msg  # chess has no cap on hidden: its own wording


@pytest.mark.parametrize("kw", [dict(), dict(conv_algo=F16), dict(conv_algo=LAYERS), dict(depth=17), dict(depth=0),
                                dict(conv_algo=F16, value_hidden=256, depth=16), dict(value_hidden=300),
                                dict(conv_algo=LAYERS, height=2, width=20, n=2, evaluator=az.EVAL_SYNTHETIC)])
def test_valid_configurations_reach_the_device(kw):
    """What the rule accepts gets as far as opening a device: an engine where
    there is one, "no HIP device" where there is none."""
    makers = [lambda: _connect_n(**kw)]
    if "height" not in kw:
        makers.append(lambda: az.ChessEngine(4, slots=2, **kw))
    for make in makers:
        try:
            eng = make()
        except az.AzError as err:
            assert "no HIP device" in str(err), str(err)
        else:
            eng.close()
