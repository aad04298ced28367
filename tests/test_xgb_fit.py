"""The on-device XGBoost refit's arithmetic contract (tests/xgb_fit_ref.py) on
the CPU: the row-loop restatement against its own brute-force split search,
against the oracle predictor, against one hand-worked case, and the guards that
keep the parity inputs of tests/test_gpu_xgb_fit.py and
tests/test_gpu_xgb_fit_edges.py from being vacuous."""
import numpy as np
import pytest

import xgb_fit_ref as R
from ce_amd.xgb import StackedForests, XgbForest, continued_model, synthetic_model
from oracle import ce_oracle as O
from xgb_users_ref import bits

F32 = np.float32


# brute_check is quadratic in a node's rows: the edge cases of at most 300 rows ("d512" takes 6 s of it)
EDGE_BRUTE = [n for n, c in R.EDGE_CASES.items() if max(c["rows"]) <= 300]


@pytest.mark.parametrize("name", sorted(R.CASES) + EDGE_BRUTE)
def test_restatement_equals_its_brute_force_check(name):
    """Every split node of every grown tree: the best (loss_chg, feature,
    threshold) found by summing each candidate's right side afresh, features in
    descending order, is the scan's choice -- 0 bits."""
    c = R.case(name)
    checked = 0
    for u in range(c["U"]):
        r = c["rows"][c["row_offsets"][u]:c["row_offsets"][u + 1]]
        if r.size == 0 or c["status"][u]:
            continue
        log = []
        R.fit_forest(c["forest"], c["X"][r], c["labels"][c["row_offsets"][u]:c["row_offsets"][u + 1]], c["rounds"],
                     c["max_depth"], log=log, **c["kw"])
        for entry in log:  # every split node of every grown tree
            lc, f, cond = R.brute_check(c["X"][r], entry, **{k: v for k, v in c["kw"].items() if k != "eta"})
            assert (bits(lc), f, bits(cond)) == (bits(entry[4][0]), entry[4][1], bits(entry[4][2])), (name, u)
            checked += 1
    assert checked > 0


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_oracle_predictor_reproduces_the_trainers_margins(name):
    """The grown trees appended to the base, walked by the existing predictors,
    give the trainer's final margins and their softmax on the batch rows."""
    c = R.case(name)
    for u in range(c["U"]):
        a, b = c["row_offsets"][u], c["row_offsets"][u + 1]
        if a == b:
            continue
        Xu = c["X"][c["rows"][a:b]]
        m = R.start_margins(Xu, c["forests"][u])
        assert np.array_equal(bits(m), bits(c["margins"][a:b]))
        model = R.full_model(c["base"], c["per_user"][u], c["info"])
        p = O.oracle_xgb_predict_proba(Xu, model)
        exp = np.array([R.softmax_row(list(row)) for row in c["margins"][a:b]], F32)
        assert np.array_equal(bits(p), bits(exp))


def test_hand_worked_six_rows():
    """6 rows, D = 1, C = 3, uniform start margins: p = 1/3, g = -2/3 or 1/3,
    h = 4/9.  A side needs H >= 1, i.e. three rows, so the only split is 3 | 3
    at x = 2.5.  Class 0 (rows 0-2): left G = -2, H = 4/3, weight 2 / (7/3) =
    6/7, leaf 0.3 * 6/7 = 0.257142...; right G = 1, weight -3/7, leaf
    -0.128571...; class 1 mirrors it; class 2 has no positive row: G = 2, H =
    8/3, the 3 | 3 split loses (2 * (1 / (7/3)) < 4 / (11/3)), one leaf
    0.3 * -2 / (11/3) = -0.163636..."""
    X = np.arange(6, dtype=np.float64).reshape(6, 1)
    y = np.array([0, 0, 0, 1, 1, 1])
    trees, info, m = R.fit_rounds(X, y, np.full((6, 3), 0.5, F32), 1, 5)
    assert info == [0, 1, 2]
    assert [t["left"].tolist() for t in trees] == [[1, -1, -1], [1, -1, -1], [-1]]
    assert [t["right"].tolist() for t in trees] == [[2, -1, -1], [2, -1, -1], [-1]]
    assert trees[0]["default_left"].tolist() == [1, 0, 0] and trees[0]["split"].tolist() == [0, 0, 0]
    assert trees[0]["cond"][0] == F32(2.5) and trees[1]["cond"][0] == F32(2.5)
    # the same numbers in the contract's arithmetic: p = (float)1 / 3, g and h in float, exact double sums
    p = F32(F32(1.0) / F32(3.0))
    g1, g0, h = float(F32(p - F32(1.0))), float(p), float(F32(F32(F32(2.0) * p) * F32(F32(1.0) - p)))
    eta = F32(0.3)

    def leaf(G, H):
        return F32(F32(-G / (H + 1.0)) * eta)

    H3 = h + h + h
    pos_leaf, neg_leaf = leaf(g1 + g1 + g1, H3), leaf(g0 + g0 + g0, H3)
    none_leaf = leaf(g0 + g0 + g0 + g0 + g0 + g0, H3 + h + h + h)
    assert abs(float(pos_leaf) - 0.3 * 6 / 7) < 1e-6 and abs(float(neg_leaf) + 0.3 * 3 / 7) < 1e-6
    assert abs(float(none_leaf) + 0.6 * 3 / 11) < 1e-6
    assert np.array_equal(bits(trees[0]["cond"][1:]), bits([pos_leaf, neg_leaf]))
    assert np.array_equal(bits(trees[1]["cond"][1:]), bits([neg_leaf, pos_leaf]))
    assert np.array_equal(bits(trees[2]["cond"]), bits([none_leaf]))
    hi, lo, no = F32(F32(0.5) + pos_leaf), F32(F32(0.5) + neg_leaf), F32(F32(0.5) + none_leaf)
    assert np.array_equal(bits(m), bits(np.array([[hi, lo, no]] * 3 + [[lo, hi, no]] * 3, F32)))
    # five rows cannot split at all: no side of three
    trees5, _, _ = R.fit_rounds(X[:5], y[:5], np.full((5, 3), 0.5, F32), 1, 5)
    assert all(t["left"].tolist() == [-1] for t in trees5)


def test_log_loss_does_not_rise():
    c = R.case("deep")
    a, b = c["row_offsets"][0], c["row_offsets"][1]
    Xu, yu = c["X"][c["rows"][a:b]], c["labels"][a:b]
    m = R.start_margins(Xu, c["forest"])
    losses = []
    for _ in range(4):
        p = np.array([R.softmax_row(list(row)) for row in m], np.float64)
        losses.append(-np.mean(np.log(p[np.arange(len(yu)), yu])))
        _, _, m = R.fit_rounds(Xu, yu, m, 1, 5)
    assert all(losses[i + 1] <= losses[i] for i in range(3)), losses


def test_rounds_chain():
    """Three rounds at once are one round three times, each from the margins of the last."""
    c = R.case("deep")
    a, b = c["row_offsets"][0], c["row_offsets"][1]
    Xu, yu = c["X"][c["rows"][a:b]], c["labels"][a:b]
    m, trees = R.start_margins(Xu, c["forest"]), []
    for _ in range(3):
        t, _, m = R.fit_rounds(Xu, yu, m, 1, 5)
        trees += t
    assert len(trees) == len(c["per_user"][0]) and all(R.same_tree(x, y) for x, y in zip(trees, c["per_user"][0]))
    assert np.array_equal(bits(m), bits(c["margins"][a:b]))


def _same_forest(a, b):
    return len(a.trees) == len(b.trees) and np.array_equal(a.tree_info, b.tree_info) and \
        all(R.same_tree(x, y) for x, y in zip(a.trees, b.trees))


def test_continued_model_is_the_stacks_forest():
    """The lazy host mirror: a stack that was handed the grown trees as the fit
    hands them over (device arrays; here CPU tensors) gives, per user,
    continued_model(base, the grown rounds) -- as forest(u) and as packed arrays."""
    c = R.case("deep")
    st = StackedForests(c["base"], [None] * c["U"])
    st.ensure_depth(c["max_depth"])  # as the fit does before it launches
    chunk = R.grown_chunk(c["per_user"], c["U"], c["rounds"], c["C"], st.depth)
    before = st.TT
    st.attach(chunk, c["D"] - 1)
    for u in range(c["U"]):
        exp = XgbForest.from_json(R.full_model(c["base"], c["per_user"][u], c["info"]))
        assert _same_forest(st.forest(u), exp), u
        assert st.n_grown(u) == len(c["per_user"][u])
    assert st.forest(1) is st.base  # no row: the base itself
    assert st.TT == before + chunk.T
    # the packed arrays of the stack: every user's logical trees, group by group, are its full model's
    nodes, leaves, ids, goff, depth = st.arrays()
    for u in range(c["U"]):
        en, el, egoff, _ = XgbForest.from_json(R.full_model(c["base"], c["per_user"][u], c["info"])).pack(depth)
        for g in range(c["C"]):
            mine = ids[goff[u * c["C"] + g]:goff[u * c["C"] + g + 1]]
            assert np.array_equal(nodes[mine], en[egoff[g]:egoff[g + 1]])
            assert np.array_equal(bits(leaves[mine]), bits(el[egoff[g]:egoff[g + 1]]))
    # a set replaces the whole tail, grown trees included
    st.set(0, None)
    assert st.forest(0) is st.base and st.n_grown(0) == 0 and st.n_grown(2) == len(c["per_user"][2])
    # a deeper model arrives for another user: the common depth grows, the grown trees are kept
    c2 = R.case("uniform")
    st2 = StackedForests(c2["base"], [None] * c2["U"])
    st2.ensure_depth(c2["max_depth"])
    assert st2.depth == c2["max_depth"]
    st2.attach(R.grown_chunk(c2["per_user"], c2["U"], c2["rounds"], c2["C"], st2.depth), c2["D"] - 1)
    want = st2.forest(0)
    deep = synthetic_model(n_rounds=1, num_class=c2["C"], max_depth=5, num_feature=c2["D"], seed=3, p_stop=0.0)
    st2.set(2, continued_model(c2["base"], deep))
    assert st2.depth == 5 and st2.n_grown(0) == 0 and st2.has_grown(0)
    assert _same_forest(st2.forest(0), want)
    assert st2.arrays()[0].shape[1] == 31


def test_parity_inputs_are_not_vacuous():
    """Asserted on the restatement alone: the inputs of the GPU parity tests
    split, reach max_depth, and resolve exact loss_chg ties by both tie rules."""
    R.TIES.update(feature=0, scan=0)
    R._CACHE.clear()
    n_split = n_trees = 0
    for name in sorted(R.CASES):
        c = R.case(name)
        trees = [t for p in c["per_user"] for t in p]
        n_split += sum(t["left"].size > 1 for t in trees)
        n_trees += len(trees)
        depths = [XgbForest([t], [0], c["C"], 0.5, "multi:softprob", 0).depth() for t in trees]
        assert max(depths) == c["max_depth"], (name, max(depths))
    assert 2 * n_split >= n_trees, (n_split, n_trees)
    assert R.TIES["feature"] > 0 and R.TIES["scan"] > 0, R.TIES


def _levels(t):
    """The depth of every node of a tree (children follow their parent in the arrays)."""
    lev = np.zeros(t["left"].size, np.int64)
    for nid in range(t["left"].size):
        if t["left"][nid] != -1:
            lev[t["left"][nid]] = lev[t["right"][nid]] = lev[nid] + 1
    return lev


def _split_features(c):
    return {int(f) for p in c["per_user"] for t in p for f, l in zip(t["split"], t["left"]) if l != -1}


def test_edge_inputs_are_not_vacuous():
    """Asserted on the restatement alone: the inputs of tests/test_gpu_xgb_fit_edges.py
    reach what they are there for (the 4096-row, 512-feature case apart: its
    one level is all it is there for)."""
    import warnings

    cases = {n: R.case(n) for n in R.EDGE_CASES if n != "d512cap" and n not in R.PARAM_CASES}
    # the parameter cases afresh: no warning, finite margins, both kinds of exact tie
    R.TIES.update(feature=0, scan=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for n in R.PARAM_CASES:
            R._CACHE.pop(n, None)
            cases[n] = c = R.case(n)
            assert np.isfinite(c["margins"]).all(), n
            trees = c["per_user"][0]
            assert 2 * sum(t["left"].size > 1 for t in trees) >= len(trees), n
    assert R.TIES["feature"] > 0 and R.TIES["scan"] > 0, R.TIES
    # lambda = 0 on hessians that cancel: candidates of infinite loss_chg are met and skipped, the margins stay finite
    R.SKIPPED["non_finite"] = 0
    R._CACHE.pop("steep", None)
    cases["steep"] = R.case("steep")
    assert R.SKIPPED["non_finite"] > 0 and np.isfinite(cases["steep"]["margins"]).all()
    assert all(t["left"].size > 1 for t in cases["steep"]["per_user"][0])
    # a full tree: 63 nodes, 16 of them on level 4 (two scans of 8 slots), 32 leaves on level 5
    full = [(t, _levels(t)) for p in cases["full"]["per_user"] for t in p if t["left"].size == R.MAX_NODES]
    assert any((lev == 4).sum() == 16 and ((lev == 5) & (t["left"] == -1)).sum() == 32 for t, lev in full)
    assert any(t["left"].size == R.MAX_NODES for t in cases["cap"]["per_user"][0])
    for n, c in cases.items():
        if c["max_depth"] == 5:
            assert max(_levels(t).max() for p in c["per_user"] for t in p) == 5, n
    # several waves: a split found by a thread of the block's first wave and one by its last
    for n in ("d65", "d257", "d512"):
        feats, last = _split_features(cases[n]), 64 * ((cases[n]["D"] - 1) // 64)
        assert min(feats) < 64 and max(feats) >= last, (n, sorted(feats))
    # the special values decide splits: a cut among the denormals, one on the colliding column
    c = cases["denormal"]
    sub = [t["cond"][i] for p in c["per_user"] for t in p for i in range(t["left"].size)
           if t["left"][i] != -1 and t["split"][i] in (1, 2)]
    assert sub and all(abs(v) < F32(1.17549435e-38) for v in sub), sub
    c = cases["collide"]
    col = c["X"][c["rows"][:c["row_offsets"][1]], 1]
    assert 1 in _split_features(c) and not np.array_equal(np.argsort(col, kind="stable"),
                                                          np.argsort(col.astype(F32), kind="stable"))
    c = cases["twice"]
    assert np.unique(c["rows"]).size == c["rows"].size - 4
    assert cases["overflow"]["status"] == [0, 1, 0] and not cases["overflow"]["per_user"][1]
    assert sum(n > 0 for n in cases["many"]["counts"]) > 256  # more blocks with work than the device has compute units


def test_rejected_configurations():
    """Each refusal by its own message, from host values alone: X here is a CPU
    tensor, which the call would refuse next -- so reaching that refusal shows
    a configuration was let through."""
    import ce_amd.ops as ops
    import torch

    base = synthetic_model(n_rounds=1, num_class=3, max_depth=2, num_feature=4, seed=1)
    st = StackedForests(base, [None])
    X = torch.zeros((4, 4), dtype=torch.float64)
    rows, lab = torch.arange(4), torch.zeros(4, dtype=torch.int32)
    for kw, msg in ((dict(gamma=0.1), "gamma and alpha must be 0"), (dict(alpha=0.5), "gamma and alpha must be 0"),
                    (dict(objective="binary:logistic"), "multi:softprob forests only"),
                    (dict(sample_weight=[1.0] * 4), "sample weights are not supported"),
                    (dict(max_depth=6), "max_depth must lie in"), (dict(max_depth=0), "max_depth must lie in"),
                    (dict(n_rounds=0), "n_rounds must be at least 1"), (dict(eta=0.0), "eta out of range"),
                    (dict(reg_lambda=-1.0), "reg_lambda out of range"),
                    (dict(min_child_weight=float("nan")), "min_child_weight out of range")):
        with pytest.raises(ValueError, match=msg):
            ops.xgb_fit_users(X, rows, lab, st, **kw)
    binary = StackedForests(synthetic_model(n_rounds=1, num_class=2, max_depth=2, num_feature=4, seed=1), [None])
    with pytest.raises(ValueError, match="multi:softprob forests only"):
        ops.xgb_fit_users(X, rows, lab, binary)
    with pytest.raises(ValueError, match="HIP device"):  # the accepted configuration gets as far as the device check
        ops.xgb_fit_users(X, rows, lab, st)
