"""GPU parity of the on-device XGBoost refit (ce_xgb_fit_users,
ops.xgb_fit_users, DeviceXGBClassifier.fit / fit_picks) against the row-loop
restatement of tests/xgb_fit_ref.py: node arrays, leaf values, packed arrays
and margins, 0 differing bits; then the walks over the grown forests against
the one-forest predictor on ``forest(u)``."""
import numpy as np
import pytest

import xgb_fit_ref as R
from ce_amd.xgb import StackedForests, XgbForest, continued_model, synthetic_model
from members_eval_ref import confusion, f1_weighted
from oracle import ce_oracle as O
from xgb_users_ref import bits, predict_labels

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
NAMES = ("left", "right", "split", "default_left", "num_nodes")


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_X(c):
    return dev(c["X"] if c["f64"] else c["X"].astype(np.float32))


def assert_outputs(got, exp, what):
    """The fit's arrays against expected_outputs: 0 differing bits."""
    t = got["trees"].out
    for k in NAMES:
        assert np.array_equal(t[k].cpu().numpy(), exp[k]), (what, k)
    assert np.array_equal(bits(t["cond"].cpu().numpy()), bits(exp["cond"])), (what, "cond")
    assert np.array_equal(t["nodes"].cpu().numpy().view(np.uint32), exp["nodes"]), (what, "nodes")
    assert np.array_equal(bits(t["leaves"].cpu().numpy()), bits(exp["leaves"])), (what, "leaves")


def same_forest(a, b):
    return len(a.trees) == len(b.trees) and np.array_equal(a.tree_info, b.tree_info) and \
        all(R.same_tree(x, y) for x, y in zip(a.trees, b.trees))


def fit_case(ce, c, users=None):
    """One ops.xgb_fit_users call on the case (all users, or only ``users`` with the others' batches empty)."""
    st = StackedForests(c["base"], [None] * c["U"])
    off = c["row_offsets"].copy()
    rows, labels = c["rows"], c["labels"]
    if users is not None:
        keep = np.concatenate([np.arange(off[u], off[u + 1]) for u in users]) if users else np.zeros(0, np.int64)
        counts = np.array([off[u + 1] - off[u] if u in users else 0 for u in range(c["U"])])
        rows, labels, off = rows[keep], labels[keep], np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    got = ce.ops.xgb_fit_users(device_X(c), dev(rows), dev(labels), st, dev(off), c["rounds"], c["max_depth"],
                               return_margins=True)
    return st, got, off


# ---- 1. parity with the restatement ------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_parity(ce, name):
    """U = 3 users in one call, rows out of order, batches of 0 .. 130 rows mixed:
    trees in both forms and the final margins, bit for bit; no flag set; the
    stack's forest(u) is the restatement's forest."""
    c = R.case(name)
    st, got, _ = fit_case(ce, c)
    exp = R.expected_outputs(c["per_user"], c["U"], c["rounds"], c["C"], st.depth)
    assert got["status"].cpu().numpy().tolist() == [0] * c["U"]
    assert got["active"].tolist() == [n > 0 for n in c["counts"]]
    assert_outputs(got, exp, name)
    assert np.array_equal(bits(got["margins"].cpu().numpy()), bits(c["margins"])), name
    for u in range(c["U"]):
        assert same_forest(st.forest(u), c["forests"][u]), (name, u)


@pytest.mark.parametrize("name", ["deep", "tiny"])
def test_users_are_independent(ce, name):
    """A U-user call equals U one-user calls."""
    c = R.case(name)
    _, all_u, _ = fit_case(ce, c)
    per = c["rounds"] * c["C"]
    for u in range(c["U"]):
        _, one, off = fit_case(ce, c, users=[u])
        if c["counts"][u] == 0:  # no row at all: nothing is launched, nothing appended
            assert one["trees"] is None and not one["active"].any()
            continue
        for k in NAMES + ("cond", "nodes", "leaves"):
            a = all_u["trees"].out[k].cpu().numpy()[u * per:(u + 1) * per]
            b = one["trees"].out[k].cpu().numpy()[u * per:(u + 1) * per]
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, u, k)
        a0, a1 = c["row_offsets"][u], c["row_offsets"][u + 1]
        assert np.array_equal(bits(one["margins"].cpu().numpy()[off[u]:off[u + 1]]),
                              bits(all_u["margins"].cpu().numpy()[a0:a1]))


# ---- 2. the member: consecutive fits, walks after a fit, the flags ----------------------
def member_case(ce, c):
    m = ce.DeviceXGBClassifier(c["base"], U=c["U"], device="cuda")
    return m, device_X(c), dev(c["rows"]), dev(c["labels"]), dev(c["row_offsets"])


def geometry_of(c):
    """The batch as a session-like geometry: one song per user (its rows), through a frame_perm."""
    return dict(item_offsets=dev(np.arange(c["U"] + 1, dtype=np.int64)), frame_offsets=dev(c["row_offsets"]),
                frame_perm=dev(c["rows"]))


def test_two_consecutive_fits_and_the_walks(ce):
    """A fit on a base-only forest, then one on the forest with a device-grown
    tail: the restatement run twice.  After each, the users walks
    (predict_proba_users, score_users) equal the one-forest predictor on
    forest(u) and the oracle on the restatement's model."""
    c = R.case("deep")
    m, X, rows, labels, off = member_case(ce, c)
    forests = [c["forest"]] * c["U"]
    per_user = [[] for _ in range(c["U"])]
    for step in range(2):
        assert m.fit(X, rows, labels, off, n_rounds=c["rounds"], max_depth=c["max_depth"]) is m
        for u in range(c["U"]):
            a, b = c["row_offsets"][u], c["row_offsets"][u + 1]
            if a < b:
                forests[u], _ = R.fit_forest(forests[u], c["X"][c["rows"][a:b]], c["labels"][a:b], c["rounds"],
                                             c["max_depth"])
                per_user[u] = forests[u].trees[len(c["forest"].trees):]
            assert same_forest(m.forest(u), forests[u]), (step, u)
        assert m.status.cpu().numpy().tolist() == [0] * c["U"]
        got = ce.ops.xgb_predict_proba_users(X, m.stacked(), **geometry_of(c)).cpu().numpy()
        y = np.zeros(c["X"].shape[0], np.int32)
        y[c["rows"]] = c["labels"]
        cm, pred, _ = ce.ops.xgb_score_users(X, m.stacked(), y=dev(y), return_pred=True, **geometry_of(c))
        exp_cm = np.zeros((c["U"], c["C"], c["C"]), np.int64)
        for u in range(c["U"]):
            r = c["rows"][c["row_offsets"][u]:c["row_offsets"][u + 1]]
            if r.size == 0:
                continue
            one = ce.ops.xgb_predict_proba(X, m.forest(u)).cpu().numpy()
            assert np.array_equal(bits(got[r]), bits(one[r])), (step, u)
            info = [k for _ in range(len(per_user[u]) // c["C"]) for k in range(c["C"])]
            orc = O.oracle_xgb_predict_proba(c["X"][r], R.full_model(c["base"], per_user[u], info))
            assert np.array_equal(bits(got[r]), bits(orc)), (step, u)
            exp_cm[u] = confusion(y[r], predict_labels(orc), c["C"])[0]
        assert np.array_equal(cm.cpu().numpy(), exp_cm), step
    # user 1 never had a row: its forest is the base, bit for bit
    assert m.forest(1) is m.base and m.models[1] is None


def test_evaluate_after_fit_and_untouched_user(ce):
    """evaluate() over a test set after a fit equals the one-forest predictor on
    forest(u); a user the fit did not touch predicts the same bits as before."""
    c = R.case("wide")
    m, X, rows, labels, off = member_case(ce, c)
    rng = np.random.default_rng(4)
    Ft = 90
    Xt = rng.normal(size=(Ft, c["D"]))
    yt = rng.integers(0, c["C"], Ft).astype(np.int32)
    es = ce.EvalSet(dev(Xt), dev(yt), frame_offsets=np.array([0, 30, 60, 90]), item_offsets=np.array([0, 1, 2, 3]))
    before = ce.ops.xgb_predict_proba_users(dev(Xt), m.stacked(), item_offsets=es.item_offsets,
                                            frame_offsets=es.frame_offsets).cpu().numpy()
    only0 = dev(np.array([0, c["row_offsets"][1], c["row_offsets"][1], c["row_offsets"][1]], np.int64))
    m.fit(X, rows, labels, only0, n_rounds=c["rounds"], max_depth=c["max_depth"])
    after = ce.ops.xgb_predict_proba_users(dev(Xt), m.stacked(), item_offsets=es.item_offsets,
                                           frame_offsets=es.frame_offsets).cpu().numpy()
    assert np.array_equal(bits(after[30:]), bits(before[30:]))
    assert not np.array_equal(bits(after[:30]), bits(before[:30]))
    f1, cm = m.evaluate(es)
    exp_cm = np.zeros((3, c["C"], c["C"]), np.int64)
    for u in range(3):
        p = ce.ops.xgb_predict_proba(dev(Xt[30 * u:30 * u + 30]), m.forest(u)).cpu().numpy()
        assert np.array_equal(bits(after[30 * u:30 * u + 30]), bits(p))
        exp_cm[u] = confusion(yt[30 * u:30 * u + 30], predict_labels(p), c["C"])[0]
    assert np.array_equal(cm.cpu().numpy(), exp_cm)
    assert np.array_equal(f1.cpu().numpy().view(np.uint64), np.array([f1_weighted(x) for x in exp_cm]).view(np.uint64))


def test_non_finite_row_flags_its_user_alone(ce):
    c = R.case("deep")
    m, _, rows, labels, off = member_case(ce, c)
    Xbad = c["X"].copy()
    Xbad[c["rows"][c["row_offsets"][2] + 3], 2] = np.inf  # user 2's batch
    m.fit(dev(Xbad), rows, labels, off, n_rounds=c["rounds"], max_depth=c["max_depth"])
    assert m.status.cpu().numpy().tolist() == [0, 0, 1]
    assert m.forest(2) is m.base and m.stacked().n_grown(2) == 0
    assert same_forest(m.forest(0), c["forests"][0])
    with pytest.raises(ValueError):
        m.check_finite()
    Xnan = c["X"].copy()
    Xnan[c["rows"][0], 0] = np.nan
    m2 = ce.DeviceXGBClassifier(c["base"], U=c["U"], device="cuda")
    m2.fit(dev(Xnan), rows, labels, off, n_rounds=1, max_depth=c["max_depth"])
    assert m2.status.cpu().numpy().tolist() == [1, 0, 0] and m2.forest(0) is m2.base


def test_table_capacity_grows_mid_sequence(ce):
    """Four one-round fits: the lane table doubles when full; the forests are the restatement's chain."""
    c = R.case("tiny")
    m, X, rows, labels, off = member_case(ce, c)
    caps, forests = [], [c["forest"]] * c["U"]
    for _ in range(4):
        m.fit(X, rows, labels, off, n_rounds=1, max_depth=c["max_depth"])
        caps.append(int(m.stacked().device(X.device, c["D"])[0].shape[1]))
        for u in range(c["U"]):
            a, b = c["row_offsets"][u], c["row_offsets"][u + 1]
            forests[u], _ = R.fit_forest(forests[u], c["X"][c["rows"][a:b]], c["labels"][a:b], 1, c["max_depth"])
            assert same_forest(m.forest(u), forests[u])
    assert caps[-1] > caps[0] and len(set(caps)) < 4, caps  # grown, and not at every fit
    got = ce.ops.xgb_predict_proba_users(X, m.stacked(), **geometry_of(c)).cpu().numpy()
    for u in range(c["U"]):
        r = c["rows"][c["row_offsets"][u]:c["row_offsets"][u + 1]]
        assert np.array_equal(bits(got[r]), bits(ce.ops.xgb_predict_proba(X, m.forest(u)).cpu().numpy()[r]))


def test_deeper_fit_repacks_and_set_model_replaces_the_tail(ce):
    """max_depth above the stack's depth packs the stack again first; set_model after device fits
    replaces that user's whole tail and leaves the others' grown trees alone."""
    c = R.case("uniform")  # a leaves-only base (depth 0), max_depth 3
    m, X, rows, labels, off = member_case(ce, c)
    assert m.stacked().depth == 0
    m.fit(X, rows, labels, off, n_rounds=c["rounds"], max_depth=c["max_depth"])
    assert m.stacked().depth == 3
    for u in range(c["U"]):
        assert same_forest(m.forest(u), c["forests"][u])
    tail = synthetic_model(n_rounds=1, num_class=c["C"], max_depth=2, num_feature=c["D"], seed=9)
    m.set_model(0, continued_model(c["base"], tail))
    assert same_forest(m.forest(0), XgbForest.from_json(continued_model(c["base"], tail)))
    assert same_forest(m.forest(1), c["forests"][1])
    got = ce.ops.xgb_predict_proba_users(X, m.stacked(), **geometry_of(c)).cpu().numpy()
    for u in range(2):
        r = c["rows"][c["row_offsets"][u]:c["row_offsets"][u + 1]]
        assert np.array_equal(bits(got[r]), bits(ce.ops.xgb_predict_proba(X, m.forest(u)).cpu().numpy()[r]))


# ---- 3. one epoch of the full committee --------------------------------------------------
def test_one_epoch_three_members(ce):
    """predict -> select(frames=...) -> retrain -> evaluate with a
    BatchedSelectionSession (a shuffled frame_perm) and all three members; the
    same loop run on the references from the device's picks: GaussianNB and SGD
    states, the XGB forests and every member's confusion matrix."""
    import gnb_fit_ref as GN
    import sgd_fit_ref as SG
    from members_eval_ref import gnb_jll, sgd_decision
    from members_eval_ref import predict_labels as linear_labels

    rng = np.random.default_rng(77)
    users, C, D, Q, FR = [5, 4, 6], 4, 8, 2, 3
    U, n_songs = len(users), sum(users)
    off = np.concatenate([[0], np.cumsum(users)]).astype(np.int64)
    s_id = rng.permutation(np.repeat(np.arange(n_songs), FR))  # shuffled frames: a frame_perm
    X = rng.normal(size=(len(s_id), D))
    song_labels = rng.integers(0, C, n_songs)
    _, f_off, f_perm = ce.song_groups(s_id)
    sess = ce.BatchedSelectionSession(Q, "mc", off, frame_offsets=f_off, frame_perm=f_perm)
    theta, var = rng.normal(size=(U, C, D)), rng.random((U, C, D)) + 0.5
    count = rng.integers(5, 20, (U, C)).astype(np.float64)
    coef, icpt = rng.normal(size=(U, C, D)) * 0.1, rng.normal(size=(U, C)) * 0.1
    base = synthetic_model(n_rounds=2, num_class=C, max_depth=3, num_feature=D, seed=21)
    nb = ce.DeviceGaussianNB(theta, var, count)
    sgd = ce.DeviceSGDClassifier(coef, icpt, np.ones(U), random_state=[3, 4, 5])
    xgb = ce.DeviceXGBClassifier(base, U=U, device="cuda")
    Xd = dev(X)
    frames = [nb.predict_proba_session(Xd, sess), sgd.predict_proba_session(Xd, sess),
              xgb.predict_proba_session(Xd, sess, out_dtype=torch.float64)]
    picks = sess.select(frames=frames)
    nb.partial_fit_picks(Xd, sess, picks, song_labels)
    sgd.partial_fit_picks(Xd, sess, picks, song_labels)
    assert xgb.fit_picks(Xd, sess, picks, song_labels, n_rounds=2, max_depth=3) is xgb
    sgd.check_finite()
    xgb.check_finite()
    # the member's own predict path after the fit: every row by the one-forest predictor on forest(u)
    after_fit = xgb.predict_proba_session(Xd, sess, skip_excluded=False).cpu().numpy()
    for u in range(U):
        r = np.flatnonzero((s_id >= off[u]) & (s_id < off[u + 1]))
        one = ce.ops.xgb_predict_proba(Xd, xgb.forest(u)).cpu().numpy()
        assert len(xgb.forest(u).trees) == 2 * C + 2 * C and np.array_equal(bits(after_fit[r]), bits(one[r])), u
    # the references, from the device's picks
    Ft = 40
    Xt, yt = rng.normal(size=(U * Ft, D)), rng.integers(0, C, U * Ft).astype(np.int32)
    es = ce.EvalSet(dev(Xt), dev(yt), frame_offsets=np.arange(U + 1) * Ft, item_offsets=np.arange(U + 1))
    got = {"nb": nb.evaluate(es), "sgd": sgd.evaluate(es), "xgb": xgb.evaluate(es)}
    nbs, sgs = nb.state(), sgd.state()
    forest = XgbForest.from_json(base)
    for u in range(U):
        songs = off[u] + np.unique(np.asarray(picks[u])[np.asarray(picks[u]) >= 0])
        r = np.flatnonzero(np.isin(s_id, songs))  # X_train's order
        yb = song_labels[s_id[r]]
        assert r.size == FR * len(songs) > 0
        th, vr, cc, prior, _ = GN.gnb_partial_fit(X[r], yb, theta[u], var[u], count[u])
        for k, e in (("theta", th), ("var", vr), ("class_count", cc), ("class_prior", prior)):
            assert GN.same_bits(nbs[k][u], e), (k, u)
        w, b, t, ok = SG.sgd_partial_fit(X[r], yb, coef[u], icpt[u], 1.0, random_state=3 + u)
        assert ok and SG.same_bits(sgs["coef"][u], w) and SG.same_bits(sgs["intercept"][u], b) and sgs["t"][u] == t
        after, _ = R.fit_forest(forest, X[r], yb, 2, 3)
        assert same_forest(xgb.forest(u), after), u
        xt, y = Xt[u * Ft:(u + 1) * Ft], yt[u * Ft:(u + 1) * Ft]
        exp = {"nb": linear_labels(gnb_jll(xt, th, vr, prior)),
               "sgd": linear_labels(sgd_decision(xt, w, b)),
               "xgb": predict_labels(O.oracle_xgb_predict_proba(xt, R.full_model(
                   base, after.trees[len(forest.trees):], [k for _ in range(2) for k in range(C)])))}
        for name, e in exp.items():
            cm = confusion(y, e, C)[0]
            assert np.array_equal(got[name][1][u].cpu().numpy(), cm), (name, u)
            assert got[name][0][u].cpu().numpy().view(np.uint64) == np.float64(f1_weighted(cm)).view(np.uint64), (name, u)


# ---- 4. refusals before any launch ---------------------------------------------------------
def test_argument_errors(ce):
    c = R.case("tiny")
    st = StackedForests(c["base"], [None] * c["U"])
    X, rows, labels, off = device_X(c), dev(c["rows"]), dev(c["labels"]), dev(c["row_offsets"])
    for kw in (dict(gamma=1.0), dict(alpha=1.0), dict(objective="binary:logistic"), dict(sample_weight=labels),
               dict(max_depth=6), dict(max_depth=0), dict(n_rounds=0), dict(eta=float("nan")), dict(reg_lambda=-1.0)):
        with pytest.raises(ValueError):
            ce.ops.xgb_fit_users(X, rows, labels, st, off, **kw)
    with pytest.raises(ValueError):
        ce.ops.xgb_fit_users(X, rows, labels[:-1], st, off)
    with pytest.raises(ValueError):
        ce.ops.xgb_fit_users(X, rows, labels, st, off[:-1])
    with pytest.raises(ValueError):
        ce.ops.xgb_fit_users(X, rows, labels, st, dev(np.array([0, 9, 3, 14], np.int64)))
    big = torch.zeros(5000, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):  # one user's batch above the row cap
        ce.ops.xgb_fit_users(X, big, big.to(torch.int32), st, dev(np.array([0, 5000, 5000, 5000], np.int64)))
    assert st.TT == len(XgbForest.from_json(c["base"]).trees)  # nothing was appended
    # the entry point itself: CE_EUNSUPPORTED / CE_EINVAL before any launch
    from ce_amd._lib import CE_EUNSUPPORTED, CEError, call

    def raw(D=1, G=3, max_depth=1, n_max=6, depth=1, rounds=1):
        z = ce.ops._p(None)
        return call("ce_xgb_fit_users", z, 0, 20, D, D, z, z, z, 3, 14, n_max, z, 0, z, 0, z, G, depth, 0.5, rounds,
                    max_depth, 0.3, 1.0, 1.0, z, z, z, z, z, z, z, z, z, z, z, 0, z)

    for kw in (dict(D=513), dict(G=9), dict(G=1), dict(max_depth=6, depth=5), dict(n_max=4097)):
        with pytest.raises(CEError) as e:
            raw(**kw)
        assert e.value.code == CE_EUNSUPPORTED, kw
    for kw in (dict(rounds=0), dict(max_depth=0), dict(max_depth=3, depth=2), dict()):  # the last: null pointers
        with pytest.raises(ValueError):
            raw(**kw)
