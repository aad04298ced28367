"""The host side of the XGBoost users form (ce_amd.xgb.stack_forests,
continued_model, ce_amd.DeviceXGBClassifier) and the label rule of
XGBClassifier.predict, without a GPU.  Expected values come from every user's
FULL JSON model: its own XgbForest.pack and the oracle."""
import copy
import ctypes

import numpy as np
import pytest

from ce_amd.xgb import XgbForest, continued_model, stack_forests, synthetic_model
from oracle import ce_oracle as O
from xgb_users_ref import bits, drop_group, leaves_model, predict_labels, user_models


def mk(seed, rounds, depth=5, num_class=4, D=20, **kw):
    return synthetic_model(n_rounds=rounds, num_class=num_class, max_depth=depth, num_feature=D, seed=seed, **kw)


def check_stack(base, models):
    """User u's trees named by tree_ids / group_offsets equal that user's own pack(depth), group by group."""
    nodes, leaves, ids, goff, depth = stack_forests(base, models)
    G = XgbForest.from_json(base).n_groups
    assert goff.dtype == np.int32 and ids.dtype == np.int32 and goff.shape == (len(models) * G + 1,)
    assert goff[0] == 0 and goff[-1] == ids.shape[0] and np.all(np.diff(goff) >= 0)
    assert ids.size == 0 or (ids.min() >= 0 and ids.max() < nodes.shape[0])
    for u, m in enumerate(models):
        en, el, egoff, ed = XgbForest.from_json(base if m is None else m).pack(depth)
        assert ed == depth
        for g in range(G):
            k = ids[goff[u * G + g]:goff[u * G + g + 1]]
            assert np.array_equal(nodes[k], en[egoff[g]:egoff[g + 1]]), (u, g)
            assert np.array_equal(bits(leaves[k]), bits(el[egoff[g]:egoff[g + 1]])), (u, g)
    return nodes, leaves, ids, goff, depth


def test_stack_base_and_tails_share_the_base_rows():
    base = mk(1, 13)
    models = user_models(base, [mk(10 + u, n) for u, n in enumerate([1, 7, 9, 24])])
    nodes, _, ids, goff, depth = check_stack(base, models)
    assert depth == 5 and nodes.shape[0] == 4 * 13 + 4 * (1 + 7 + 9 + 24)  # the base once, the tails
    assert np.array_equal(ids[goff[0]:goff[0] + 13], ids[goff[4]:goff[4] + 13])  # user 0 and 1: the same base rows


def test_stack_base_only_and_none():
    base = mk(2, 5)
    nodes, _, ids, goff, _ = check_stack(base, [None, base, copy.deepcopy(base)])
    assert nodes.shape[0] == 20 and ids.shape[0] == 60


def test_stack_model_that_is_no_continuation():
    base = mk(3, 6)
    other = mk(4, 8)  # other trees from the first on: stored whole
    short = mk(3, 2)  # fewer trees than the base
    changed = copy.deepcopy(continued_model(base, mk(5, 3)))
    changed["learner"]["gradient_booster"]["model"]["trees"][2]["split_conditions"][0] += 1.0
    nodes, _, _, _, _ = check_stack(base, [other, short, changed, continued_model(base, mk(5, 3))])
    assert nodes.shape[0] == 4 * (6 + 8 + 2 + 9 + 3)


def test_stack_pads_a_shallow_tail_and_a_shallow_base():
    base = mk(6, 4, depth=5, p_stop=0.0)
    _, _, _, _, depth = check_stack(base, user_models(base, [mk(7, 3, depth=3), mk(8, 2, depth=0), None]))
    assert depth == 5
    base = mk(6, 4, depth=1)
    _, _, _, _, depth = check_stack(base, user_models(base, [mk(7, 3, depth=4), None]))
    assert depth == 4


def test_pack_depth_pads_without_changing_the_bits():
    model = mk(9, 6, depth=3)
    f = XgbForest.from_json(model)
    n3, l3, goff, d = f.pack()
    n5, l5, goff5, d5 = f.pack(5)
    assert (d, d5) == (f.depth(), 5) and np.array_equal(goff, goff5) and f.pack(5) is f.pack(5)
    assert np.array_equal(n5[:, :7], n3[:, :7]) and np.all(n5[:, 7:] == 0)  # the first levels are the tree's own
    step = 1 << (5 - d)
    assert np.array_equal(bits(l5), bits(np.repeat(l3, step, axis=1)))
    with pytest.raises(ValueError, match="below"):
        f.pack(2)


def test_stack_user_with_an_empty_group():
    base = mk(11, 3)
    only = drop_group(mk(12, 5), 2)  # not a continuation, and group 2 owns no tree
    tail_gap = continued_model(base, drop_group(mk(13, 4), 0))
    _, _, _, goff, _ = check_stack(base, [only, tail_gap])
    assert goff[3] - goff[2] == 0 and goff[5] - goff[4] == 3


def test_stack_mismatch_errors():
    base = mk(14, 2)
    with pytest.raises(ValueError, match="num_class"):
        stack_forests(base, [mk(15, 2, num_class=3)])
    with pytest.raises(ValueError, match="objective|num_class"):
        stack_forests(base, [mk(15, 2, num_class=2)])
    other = copy.deepcopy(base)
    other["learner"]["learner_model_param"]["base_score"] = "2.5E-1"
    with pytest.raises(ValueError, match="base_score"):
        stack_forests(base, [other])
    with pytest.raises(ValueError, match="num_feature"):
        stack_forests(base, [mk(14, 2, D=21)])
    with pytest.raises(ValueError, match="depth 6"):
        stack_forests(base, user_models(base, [mk(16, 2, depth=6, p_stop=0.0)]))
    with pytest.raises(ValueError, match="at least one"):
        stack_forests(base, [])


def test_continued_model_chains_the_margins():
    """Leaves-only forests: the continued model's margin of group g is the base
    margin plus the base's leaves then the tail's, added one after the other in
    float32 -- chained here by hand and pushed through the same softmax."""
    a = leaves_model([[0.25, -0.5, 1.0], [0.125, 0.0625, -2.0]], 3)
    b = leaves_model([[1e-3, 3.0, 0.5]], 3)
    c = continued_model(a, b)
    gb = c["learner"]["gradient_booster"]["model"]
    assert gb["tree_info"] == [0, 1, 2] * 3 and [t["id"] for t in gb["trees"]] == list(range(9))
    assert gb["gbtree_model_param"]["num_trees"] == "9" and len(a["learner"]["gradient_booster"]["model"]["trees"]) == 6
    X = np.zeros((2, 4))
    m = np.full(3, np.float32(0.5))
    for row in ([0.25, -0.5, 1.0], [0.125, 0.0625, -2.0], [1e-3, 3.0, 0.5]):
        m = (m + np.asarray(row, np.float32)).astype(np.float32)
    one = leaves_model([list(m - np.float32(0.5))], 3)  # one round holding the chained sums (exact: see the assert)
    assert np.array_equal(bits(np.float32(0.5) + (m - np.float32(0.5))), bits(m))
    assert np.array_equal(bits(O.oracle_xgb_predict_proba(X, c)), bits(O.oracle_xgb_predict_proba(X, one)))
    with pytest.raises(ValueError, match="num_class|objective"):
        continued_model(a, leaves_model([[0.0]], 2))


def test_label_rule_hand_cases():
    # an exact tie of two float32 probabilities: equal leaves, the first index wins
    tie = leaves_model([[0.75, 0.75, -1.0, 0.75]], 4)
    p = O.oracle_xgb_predict_proba(np.zeros((1, 4)), tie)
    assert bits(p)[0, 0] == bits(p)[0, 1] == bits(p)[0, 3] and predict_labels(p)[0] == 0
    # the argmax is taken of the PROBABILITIES: a later, larger margin can round to the same float32
    assert predict_labels(np.asarray([[0.25, 0.5, 0.5, 0.125]], np.float32))[0] == 1
    # binary p exactly 0.5: base_score 0.5, zero leaves -> class 0
    half = leaves_model([[0.0]], 2)
    p = O.oracle_xgb_predict_proba(np.zeros((1, 4)), half)
    assert p[0, 1] == np.float32(0.5) and predict_labels(p, binary=True)[0] == 0
    assert predict_labels(np.asarray([[0.4, np.nextafter(np.float32(0.5), np.float32(1))]], np.float32), True)[0] == 1
    # NaN probabilities: +inf and -inf leaves
    nanm = leaves_model([[np.inf, 0.0, -np.inf, 1.0]], 4)
    p = O.oracle_xgb_predict_proba(np.zeros((1, 4)), nanm)
    assert np.isnan(p[0, 0]) and predict_labels(p)[0] == 0
    assert predict_labels(np.asarray([[0.1, np.nan, 0.9, np.nan]], np.float32))[0] == 1
    nanb = leaves_model([[np.inf], [-np.inf]], 2)
    p = O.oracle_xgb_predict_proba(np.zeros((1, 4)), nanb)
    assert np.isnan(p[0, 1]) and predict_labels(p, binary=True)[0] == 0


def test_abi_argument_checks():
    from ce_amd import _lib

    lib = _lib.load()
    p, f, E, U = ctypes.c_void_p(16), ctypes.c_float(0.5), _lib.CE_EINVAL, _lib.CE_EUNSUPPORTED

    def proba(X=p, x_dt=1, F=10, D=260, ld=260, table=p, TT=8, ids=p, L=8, goff=p, G=4, depth=5, C=4, Un=2, items=p,
              f_off=p, out=p, out_dt=0, ldo=4):
        return lib.ce_xgb_predict_proba_users(X, x_dt, F, D, ld, table, TT, ids, L, goff, G, depth, f, C, Un, items,
                                              f_off, None, None, out, out_dt, ldo, None)

    def score(X=p, x_dt=1, F=10, D=260, ld=260, L=8, G=4, depth=5, C=4, Un=2, y=p, cm=p, proba=None, ldp=4):
        return lib.ce_xgb_score_users(X, x_dt, F, D, ld, p, 8, p, L, p, G, depth, f, C, Un, p, p, None, None, y, cm,
                                      None, proba, ldp, None)

    assert proba(D=513, ld=513) == E and proba(D=0) == E and proba(ld=259) == E and proba(F=-1) == E
    assert proba(G=3) == E and proba(G=2, C=3) == E and proba(G=9, C=9) == E and proba(ldo=3) == E
    assert proba(x_dt=2) == E and proba(out_dt=2) == E
    assert proba(X=None) == E and proba(out=None) == E and proba(table=None) == E and proba(ids=None) == E
    assert proba(goff=None) == E and proba(items=None) == E and proba(f_off=None) == E
    assert proba(Un=0) == E and proba(L=-1) == E and proba(depth=-1) == E
    assert proba(depth=6) == U and b"depth" in lib.ce_last_error()
    assert proba(F=0) == _lib.CE_OK and proba(F=0, G=1, C=2, ldo=2) == _lib.CE_OK  # nothing is launched
    assert score(G=3) == E and score(x_dt=2) == E and score(Un=0) == E and score(L=-1) == E and score(X=None) == E
    assert score(cm=None) == E and score(y=None) == E and score(proba=p, ldp=3) == E and score(depth=6) == U


def test_python_validation_without_gpu():
    torch = pytest.importorskip("torch")
    import ce_amd
    from ce_amd import ops
    from ce_amd.xgb import StackedForests

    base = mk(20, 2)
    st = StackedForests(base, user_models(base, [mk(21, 1), None]))
    assert (st.U, st.G, st.C, st.depth, st.TT, st.L) == (2, 4, 4, 5, 12, 20) and 0 <= st.max_feature < 20
    X = torch.zeros((4, 20), dtype=torch.float64)
    with pytest.raises(ValueError, match="HIP device"):
        ops.xgb_predict_proba_users(X, st, [0, 1, 2], [0, 2, 4])
    with pytest.raises(ValueError, match="HIP device"):
        ops.xgb_score_users(X, st, [0, 1, 2], [0, 2, 4], torch.zeros(4, dtype=torch.int32))
    member = ce_amd.DeviceXGBClassifier(base, user_models(base, [mk(21, 1), None]), device="cuda:0")
    assert (member.U, member.C, member.G, member.D) == (2, 4, 4, 20)
    assert member.state()["tree_ids"].shape == (20,)
    member.set_model(1, continued_model(base, mk(22, 3)))
    assert member.state()["tree_ids"].shape == (4 * (2 + 1) + 4 * (2 + 3),)
    with pytest.raises(ValueError, match="num_class"):
        member.set_model(0, mk(23, 1, num_class=3))
    assert member.state()["tree_ids"].shape == (32,)  # the refused model changed nothing
    with pytest.raises(ValueError, match="depth 6"):
        member.set_model(0, continued_model(base, mk(24, 1, depth=6, p_stop=0.0)))
    assert member.state()["tree_ids"].shape == (32,) and member.forest(0).depth() <= 5
    with pytest.raises(ValueError, match="outside"):
        member.set_model(2, None)
    with pytest.raises(ValueError, match="model"):
        ce_amd.DeviceXGBClassifier(base, [None], U=2, device="cuda:0")
    assert ce_amd.DeviceXGBClassifier(base, U=3, device="cuda:0").state()["group_offsets"].shape == (13,)


def test_set_model_touches_one_user(monkeypatch):
    """A set_model compares and packs the model it is given and nothing else:
    every other user's packed trees are kept, and the arrays are put together
    once, on the next use -- the epoch's U set_model calls cost U packs, not U^2."""
    pytest.importorskip("torch")
    import ce_amd
    from ce_amd import xgb

    base = mk(30, 3)
    U = 6
    member = ce_amd.DeviceXGBClassifier(base, user_models(base, [mk(31 + u, 2) for u in range(U)]), device="cuda:0")
    before = member.state()
    packs, stacks = [], []
    real_pack, real_arrays = xgb.XgbForest.pack, xgb.StackedForests.arrays

    def counting_pack(self, depth=None):
        if self._packed is None or depth not in self._packed:
            packs.append(len(self.trees))
        return real_pack(self, depth)

    def counting_arrays(self):
        if self._arrays is None:
            stacks.append(1)
        return real_arrays(self)

    monkeypatch.setattr(xgb.XgbForest, "pack", counting_pack)
    monkeypatch.setattr(xgb.StackedForests, "arrays", counting_arrays)
    new = [continued_model(base, mk(40 + u, 1 + u)) for u in range(U)]
    for u in range(U):
        member.set_model(u, new[u])
    assert packs == [] and stacks == []  # nothing is packed or stacked before the next use
    after = member.state()
    assert sorted(packs) == [4 * (1 + u) for u in range(U)] and stacks == [1]  # every new tail once; no other tree
    member.set_model(2, None)
    member.state()
    assert sorted(packs) == sorted([4 * (1 + u) for u in range(U)] + [0]) and stacks == [1, 1]
    assert before["tree_ids"].shape == (U * 4 * 5,) and after["tree_ids"].shape == (4 * (3 * U + sum(range(1, U + 1))),)
    en, el, ids, goff, d = stack_forests(base, new)  # the incremental arrays are those of a fresh stacking
    assert np.array_equal(after["nodes"], en) and np.array_equal(bits(after["leaves"]), bits(el))
    assert np.array_equal(after["tree_ids"], ids) and np.array_equal(after["group_offsets"], goff) and after["depth"] == d
