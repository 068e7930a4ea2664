"""The chess forward tests' reference side (tests/chess_forward_ref.py), checked
with no GPU: the batch feeds every one of the 118 planes, values fp16 cannot
hold among them; every case's weights are lively and its float64 reference
separates honest float32 arithmetic from the mildest of seven mutants by 64x;
and each case gets the layout its row claims from the library's own chooser
(tests/native/tower_layout_check.cpp --rows-stem): double-buffered 128-row tiles
at every depth.  tests/test_chess_forward_layouts_gpu.py runs the cases."""
import numpy as np
import pytest

import chess_forward_ref as cr
import chess_oracle as C
import forward_ref as fr
import keras_ref
from custom_alphazero.model.weights import init_weights, weight_spec

NAMES = [c.name for c in cr.CASES]


def _fp16_exact(a):
    return np.array_equal(a, a.astype(np.float16).astype(np.float32))


def test_old_chess_batch_leaves_84_planes_and_every_second_term_dead():
    """The gap itself: the states of test_chess_forward_matches_keras_restatement
    ([0 x 6, start, cur] or [0 x 7, cur]) never feed planes 0..83 a value, hold
    only values exact in fp16, and seed 3's heads give a flat policy."""
    pos, roots = C.random_positions(29, seed=21)
    x = np.stack([C.full_state(*C.reference_history(p, bool(r)), p) for p, r in zip(pos, roots)]).astype(np.float32)
    assert not x[..., :84].any() and _fp16_exact(x)
    w = init_weights(weight_spec(8, 8, 1880, in_channels=118), seed=3)
    p, _ = keras_ref.forward(w, x, depth=4)
    assert p.max() < 1.5 / 1880 and p.min() > 0.5 / 1880, (p.min(), p.max())


def test_chess_batch_feeds_every_plane():
    x = cr.chess_batch()
    assert x.shape == (cr.BATCH, 8, 8, cr.PLANES) and x.dtype == np.float32 and (x >= 0).all()
    onehot, floats = x[:-cr.N_FLOAT], x[-cr.N_FLOAT:]
    planes = x.reshape(-1, cr.PLANES)
    assert (planes.max(axis=0) > 0).all()                       # every plane is live
    # the boards from the oracle: exact in fp16; by themselves they reach the 84 planes of history
    # steps 0..5, a repetition count and all four castling rights
    assert _fp16_exact(onehot)
    assert (onehot[..., :84].reshape(-1, 84).max(axis=0) > 0).all()
    assert (onehot[..., 13:112:14] > 0).any() and (onehot[..., 112:116].reshape(-1, 4).max(axis=0) == 1).all()
    pieces = np.stack([x[..., 14 * h:14 * h + 13].sum(axis=-1) for h in range(8)], axis=1)  # [B, 8, 8, 8]
    valid = pieces[:-cr.N_FLOAT].reshape(len(onehot), 8, 64)
    assert ((valid == 0).all(axis=2) | (valid == 1).all(axis=2)).all()   # a step is one-hot or empty
    steps = valid[:, :, 0].astype(int)
    assert (steps[:14] == 1).all()                              # about half: eight valid steps
    assert (steps[14:, 7] == 1).all() and (steps[14:21].sum(axis=1) < 8).any()
    assert steps[21].tolist() == [0] * 6 + [1, 1] and steps[22].tolist() == [0] * 7 + [1]  # the search's forms
    # the float boards: nearly every value needs the second split16 term, the counters reach 100+
    assert (floats != floats.astype(np.float16).astype(np.float32)).mean() > 0.9
    assert floats[..., 116].max() > 100 and floats[..., 117].max() > 90
    assert (floats[..., :112].max() < 2) and (floats.reshape(-1, cr.PLANES).min(axis=0) < 0.1 * cr.PLANE_RANGE).all()


@pytest.mark.skipif(not fr.have_lib(), reason="libaz.so not built")
def test_chess_cases_get_the_double_buffered_layout():
    """What the case table says of the layout, by the library's chooser: chess
    runs 128-row tiles of two boards, double-buffered, staging the blob up to
    bpd (the dense heads run in their own kernels), at every depth the tower
    takes -- the in-place input-row instantiations are not reachable."""
    L = cr.layouts()
    for c in cr.CASES:
        r = L[c.name]
        staged = 516 + 256 * c.depth
        assert (r["tower"], r["tile_rows"], r["boards"], r["dbuf"], r["dual"]) == (1, 128, 2, 1, 0), (c.name, r)
        assert r["staged"] == r["off_bpd"] == staged, (c.name, r)
        assert r["lds_bytes"] == (2 * 128 + 8) * 544 + 104 + 4 * staged <= 160 * 1024, (c.name, r)
        # the stat is self-play's stem (input chunks 0-1 skipped); forward() runs all four
        assert r["flop"] == r["flop_chunks2"] < r["flop_chunks4"], (c.name, r)
        # (two chunks more: 9 taps x 4 blocks in each M half less the plan's skipped block-taps, per chunk
        # and N quarter; 6 MFMAs of 16 x 16 x 32 a block-k-step; two boards a tile)
        assert r["flop_chunks4"] - r["flop_chunks2"] == 2 * 4 * (2 * 9 * 4 - r["skipped"]) * 6 * (16 * 16 * 32 * 2) / 2
    depths = L["depths"]
    assert [r["depth"] for r in depths] == list(range(1, 18))
    assert all(r["tower"] and r["dbuf"] and r["tile_rows"] == 128 for r in depths[:16]), depths
    assert not depths[16]["tower"]  # kTowerMaxDepth = 16 (the LDS would hold depth 17 too)
    assert depths[15]["lds_bytes"] + 4 * 256 <= 160 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_chess_case_is_lively_and_separates_the_mutants(name):
    d = cr.case_data(name)
    c, x, p, v = d["case"], d["x"], d["p"], d["v"]
    kp, kv = keras_ref.forward(d["w"], x, depth=c.depth)
    assert np.abs(kp - p).max() <= 1e-12 and np.abs(kv - v).max() <= 1e-12
    assert x is cr.chess_batch() and p.shape == (cr.BATCH, cr.ACTIONS) and v.shape == (cr.BATCH,)
    assert all(a.dtype == np.float32 for a in d["w"].values())
    assert d["w"]["stem.kernel"].shape == (3, 3, cr.PLANES, 128)
    assert d["w"]["value.dense1.kernel"].shape == (64, c.hidden)
    print(f"{name}: value std {v.std():.3f} max |v| {np.abs(v).max():.3f} dense1 alive {d['dense1_units_alive']:.2f} "
          f"policy max {p.max() * cr.ACTIONS:.0f} / A; e32 {d['e32_p']:.2e} {d['e32_v']:.2e} "
          f"tol {d['tol_p']:.2e} {d['tol_v']:.2e}")
    print("  policy", {m: f"{d['mut_p'][m]:.1e}" for m in cr.MOVES_POLICY},
          "value", {m: f"{d['mut_v'][m]:.1e}" for m in cr.MOVES_VALUE})
    assert v.std() > 0.2, v.std()
    assert np.abs(v).max() < 0.98, np.abs(v).max()  # no board in tanh's flat end (slope above 0.04)
    assert p.max() >= 10.0 / cr.ACTIONS, p.max()
    if c.hidden > 1:
        assert d["dense1_units_alive"] >= 0.5, d["dense1_units_alive"]
    else:
        assert d["dense1_units_alive"] == 1.0 and 0.25 <= d["dense1_active"] <= 0.75
    assert d["last_policy_feature_live"]
    for m in cr.MOVES_POLICY:
        assert d["mut_p"][m] > 8 * d["e32_p"] and d["mut_p"][m] > d["tol_p"], (m, d["mut_p"][m], d["e32_p"])
    for m in cr.MOVES_VALUE:
        assert d["mut_v"][m] > 8 * d["e32_v"] and d["mut_v"][m] > d["tol_v"], (m, d["mut_v"][m], d["e32_v"])
    assert d["mut_p"]["M4"] == 0.0 and d["mut_v"]["M5"] == 0.0  # each head's mutant is its own
    assert d["tol_p"] == min(d["mut_p"][m] for m in cr.MOVES_POLICY) / 8 >= 8 * d["e32_p"], (d["tol_p"], d["e32_p"])
    assert d["tol_v"] == min(d["mut_v"][m] for m in cr.MOVES_VALUE) / 8 >= 8 * d["e32_v"], (d["tol_v"], d["e32_v"])


def test_lively_chess_weights_only_touch_the_heads():
    x = cr.chess_batch()
    w = cr.lively_chess_weights(2, 100, x, seed=2)
    w0 = init_weights(weight_spec(8, 8, cr.ACTIONS, depth=2, hidden=100, in_channels=cr.PLANES), seed=2,
                      randomize_bn=True)
    assert list(w) == list(w0)
    changed = sorted(k for k in w0 if not np.array_equal(w[k], w0[k]))
    assert changed == ["policy.conv.beta", "policy.dense.kernel", "value.conv.beta", "value.dense1.kernel",
                       "value.dense2.bias", "value.dense2.kernel"]
    assert all(np.array_equal(w[k], cr.case_data("chess_d2_h100")["w"][k]) for k in w)
