"""The forward tests' case table (tests/forward_ref.py), checked with no GPU:
the table reaches every tower layout load_network can choose (by the library's
own chooser, az::tower16_choose_layout through tests/native/tower_layout_check.cpp),
the chooser keeps its invariants over every board the tower takes, and every case's
weights are lively and its reference separates honest float32 arithmetic from
the mildest mutant by 64x.  tests/test_forward_layouts_gpu.py runs the cases."""
import json
import os

import numpy as np
import pytest

import forward_ref as fr
import keras_ref
from custom_alphazero.model.weights import init_weights, weight_spec

NAMES = [c.name for c in fr.CASES]
FALLBACK_NAMES = [c.name for c in fr.FALLBACK_CASES]


@pytest.mark.skipif(not fr.have_lib(), reason="libaz.so not built")
def test_case_table_reaches_every_tower_layout():
    L = fr.layouts()
    rows = [(fr.CASE_BY_NAME[n], r) for n, r in L.items()]
    assert all(r["tower"] for _, r in rows), [n for n, r in L.items() if not r["tower"]]

    def some(pred):
        return [c.name for c, r in rows if pred(c, r)]

    assert some(lambda c, r: r["tile_rows"] == 96)                      # 96-row primary tiles
    assert some(lambda c, r: r["tile_rows"] == 192)
    assert some(lambda c, r: r["boards"] == 8 and c.H * c.W * 9 <= r["tile_rows"])  # the 8-board cap binds
    assert some(lambda c, r: r["boards"] == 1)                          # 1-board tiles (HW > 96)
    assert some(lambda c, r: r["boards"] == 1 and r["plan"] != "none")
    assert some(lambda c, r: c.H * c.W == 128 and r["pads"] == 0)      # a tile with no pad row
    assert some(lambda c, r: r["tile_rows"] == 128 and not r["dbuf"])   # 128-row tiles in place
    assert some(lambda c, r: r["tile_rows"] == 128 and r["dbuf"])
    assert some(lambda c, r: r["wpd"] == "l2" and r["dbuf"])            # the policy dense from L2
    assert some(lambda c, r: r["wpd"] == "l2" and not r["dbuf"])
    assert some(lambda c, r: r["wv1"] == "l2" and r["dbuf"])            # wv1 from L2 under double buffering
    assert some(lambda c, r: r["wv1"] == "l2" and not r["dbuf"])
    assert some(lambda c, r: r["wv1"] == "xtile")
    assert some(lambda c, r: r["wv1"] == "lds" and r["dbuf"])
    assert some(lambda c, r: r["wv1"] == "lds" and not r["dbuf"])
    for form in ("four_borders", "top_bottom", "none"):                 # the three slot-plan forms
        assert some(lambda c, r: r["plan"] == form), form
    assert not some(lambda c, r: r["plan"] == "other" or r.get("alt_plan") == "other")
    assert some(lambda c, r: c.H == 2 and r["plan"] == "none") and some(lambda c, r: c.W == 2 and r["plan"] == "none")
    assert some(lambda c, r: c.W > 16)
    assert some(lambda c, r: c.hidden == 1)
    assert some(lambda c, r: 512 % c.hidden)                            # P = 512 / hidden leaves idle threads
    assert some(lambda c, r: (c.H * c.W * c.hidden) % 4)
    # the dual launch: the 96-row tiles stage the whole blob, or leave wv1 in L2
    assert some(lambda c, r: r["dual"] and (r["alt_wv1"], r["alt_wpd"]) == ("lds", "lds") and r["wv1"] == "xtile")
    assert some(lambda c, r: r["dual"] and (r["alt_wv1"], r["alt_wpd"]) == ("l2", "lds") and r["wpd"] == "l2")
    assert some(lambda c, r: r["dual"] and r["alt_plan"] == "top_bottom")
    assert some(lambda c, r: r["dual"] and r["alt_plan"] == "four_borders")
    # the cases the GPU file runs as dual are the ones the library makes dual
    assert sorted(some(lambda c, r: r["dual"])) == sorted(fr.DUAL_CASES)
    # what the table says of single cases (the predictions the table was drawn up with)
    expect = {"6x7g_d4_h256": (128, 3, 1, "xtile", "lds", "four_borders"),
              "6x7g_d16_h256": (128, 3, 0, "lds", "lds", "four_borders"),
              "6x7g_d2_h255": (128, 3, 1, "l2", "lds", "four_borders"),
              "6x6g_d2_h64": (128, 3, 1, "lds", "lds", "four_borders"),
              "5x5n_d4_h256": (128, 5, 1, "xtile", "lds", "four_borders"),
              "2x2n_d1_h256": (96, 8, 1, "lds", "lds", "none"),
              "4x4n_d2_h256": (96, 6, 1, "lds", "lds", "none"),
              "6x8g_d2_h256": (96, 2, 1, "l2", "lds", "top_bottom"),
              "2x9g_d2_h256": (128, 7, 1, "xtile", "lds", "none"),
              "8x8n_d2_h256": (128, 2, 1, "l2", "l2", "top_bottom"),
              "8x8n_d16_h256": (128, 2, 0, "l2", "lds", "top_bottom"),
              "9x9n_d2_h256": (192, 2, 0, "l2", "l2", "four_borders"),
              "10x10g_d2_h256": (128, 1, 1, "l2", "lds", "four_borders"),
              "11x11n_d16_h256": (128, 1, 0, "l2", "l2", "none"),
              "8x16g_d1_h256": (128, 1, 1, "l2", "l2", "top_bottom")}
    for name, e in expect.items():
        r = L[name]
        assert (r["tile_rows"], r["boards"], r["dbuf"], r["wv1"], r["wpd"], r["plan"]) == e, (name, r)
    for c, r in rows:  # a plan only ever removes work
        assert r["flop"] <= r["flop_natural"] and (r["flop"] < r["flop_natural"]) == (r["plan"] != "none"), r


@pytest.mark.skipif(not fr.have_lib(), reason="libaz.so not built")
def test_layout_sweep_keeps_the_choosers_invariants(tmp_path):
    """Every Connect-N shape the tower takes (390 boards of H, W >= 2 and
    HW <= 128, A = W or HW, depth 1 / 4 / 16, hidden 1 / 64 / 255 / 256): each
    chosen layout fits the LDS and the heads' scratch, stages one of the three
    blob prefixes, and its slot plans hold every pixel once and only remove
    work.  The shapes without a layout are those of the golden list, which the
    restating check program of the commit before the chooser existed produced
    over the same sweep: none -- the per-layer fallback is not reachable for
    4 input planes within the engine's limits."""
    out = json.loads(fr.run_layout_check(str(tmp_path), ["--sweep"]))
    assert out["shapes"] == 390 * 2 * 3 * 4
    assert out["failures"] == []
    with open(os.path.join(fr.REPO, "tests", "golden", "tower_layout_not_ok.json")) as f:
        assert out["not_ok"] == json.load(f)


def test_old_weights_leave_the_value_head_dead():
    """The gap itself: with init_weights(seed=0, randomize_bn=True) at 6x7
    depth 4 the value conv is negative everywhere after its batch norm and the
    reference value is the same for every board.  The lively weights on the
    same batch are not."""
    x = fr.make_batch(6, 7)
    w = init_weights(weight_spec(6, 7, 7, depth=4), seed=0, randomize_bn=True)
    _, v = keras_ref.forward(w, x, depth=4)
    assert v.max() == v.min() and abs(v[0] - -0.046057602836) < 1e-11, (v.max() - v.min(), v[0])
    assert fr.case_data("6x7g_d4_h256")["v"].std() > 0.2


@pytest.mark.parametrize("name", NAMES + FALLBACK_NAMES)
def test_case_is_lively_and_separates_the_mutants(name):
    d = fr.case_data(name)
    c, p, v = d["case"], d["p"], d["v"]
    kp, kv = keras_ref.forward(d["w"], d["x"], depth=c.depth)
    assert np.abs(kp - p).max() <= 1e-12 and np.abs(kv - v).max() <= 1e-12
    assert len(d["x"]) == fr.BATCH and p.shape == (fr.BATCH, fr.action_space(c))
    assert all(a.dtype == np.float32 for a in d["w"].values())
    print(f"{name}: value std {v.std():.3f} max |v| {np.abs(v).max():.3f} dense1 active {d['dense1_active']:.2f} "
          f"policy max {p.max():.3f}; e32 {d['e32_p']:.2e} {d['e32_v']:.2e} tol {d['tol_p']:.2e} {d['tol_v']:.2e}")
    assert v.std() >= 0.2, v.std()
    assert np.abs(v).max() < 0.95, np.abs(v).max()
    if c.hidden < 4:
        assert d["dense1_units_alive"] == 1.0
    else:
        assert d["dense1_active"] >= 0.25, d["dense1_active"]  # of the (board, unit) pre-activations
    no_block = ["M3"] if c.depth == 0 else []  # (M3 mutates the last block's conv2)
    assert d["moves_p"] == [m for m in fr.MOVES_POLICY if m not in no_block]
    assert d["moves_v"] == [m for m in fr.MOVES_VALUE if m not in no_block]
    for m in d["moves_p"]:
        assert d["mut_p"][m] > d["tol_p"], (m, d["mut_p"][m], d["tol_p"])
    for m in d["moves_v"]:
        assert d["mut_v"][m] > d["tol_v"], (m, d["mut_v"][m], d["tol_v"])
    assert d["tol_p"] > 0 and d["tol_v"] > 0
    assert d["mut_p"]["M4"] == 0.0 and d["mut_v"]["M5"] == 0.0  # each head's mutant is its own
    assert d["tol_p"] >= 8 * d["e32_p"], (d["tol_p"], d["e32_p"])
    assert d["tol_v"] >= 8 * d["e32_v"], (d["tol_v"], d["e32_v"])


def test_lively_weights_only_touch_the_heads():
    c = fr.CASE_BY_NAME["6x7g_d2_h100"]
    x = fr.make_batch(c.H, c.W)
    w = fr.lively_weights(c.H, c.W, c.gravity, c.depth, c.hidden, x, seed=0)
    w0 = init_weights(weight_spec(c.H, c.W, 7, depth=c.depth, hidden=c.hidden), seed=0, randomize_bn=True)
    changed = sorted(k for k in w0 if not np.array_equal(w[k], w0[k]))
    assert changed == ["policy.conv.beta", "policy.dense.kernel", "value.conv.beta", "value.dense1.kernel",
                       "value.dense2.bias", "value.dense2.kernel"]
    _, logits, _, z, u = fr.head_parts(w, fr.trunk(w, x, c.depth))
    # (the two kernels are divided by a deviation that the unscaled biases, +-0.1, are part of)
    assert abs(logits.std() - 1) < 0.1 and abs(z.std() - 1) < 0.1 and abs(u.std() - 0.5) < 1e-3 and abs(u.mean()) < 1e-3
