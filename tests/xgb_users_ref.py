"""Helpers of the XGBoost users-form tests (tests/test_xgb_users.py,
tests/test_gpu_xgb_users.py): the label rule of XGBClassifier.predict
(xgboost/sklearn.py:981-985) restated in numpy, hand-built leaves-only models,
and per-user expected values from each user's full JSON model through the
oracle (oracle.ce_oracle.oracle_xgb_predict_proba)."""
import numpy as np

from ce_amd.xgb import XgbForest, continued_model, synthetic_model
from oracle import ce_oracle as O


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def predict_labels(proba, binary=False):
    """XGBClassifier.predict on the float32 probabilities [F, C]: np.argmax (the
    first maximum; a NaN wins at its first occurrence), or p > 0.5 of the
    positive class for binary:logistic (a NaN is class 0)."""
    proba = np.asarray(proba, np.float32)
    if binary:
        return (proba[:, 1] > np.float32(0.5)).astype(np.int32)
    return np.argmax(proba, axis=1).astype(np.int32)


def leaves_model(leaves, num_class, base_score="5E-1", num_feature=4):
    """A forest of single-leaf trees: leaves[r][g] is the leaf of round r, group g."""
    m = synthetic_model(n_rounds=len(leaves), num_class=num_class, max_depth=0, num_feature=num_feature, seed=1)
    trees = m["learner"]["gradient_booster"]["model"]["trees"]
    groups = 1 if num_class <= 2 else num_class
    for r, row in enumerate(leaves):
        for g in range(groups):
            trees[r * groups + g]["split_conditions"] = [float(row[g])]
    m["learner"]["learner_model_param"]["base_score"] = base_score
    return m


def user_models(base, tails):
    """Every user's full JSON model: ``base`` continued by the user's tail (None: the base itself)."""
    return [base if t is None else continued_model(base, t) for t in tails]


def drop_group(model, g):
    """``model`` without its trees of group g (a user whose group owns no tree)."""
    import copy

    out = copy.deepcopy(model)
    m = out["learner"]["gradient_booster"]["model"]
    keep = [i for i, t in enumerate(m["tree_info"]) if t != g]
    m["trees"] = [m["trees"][i] for i in keep]
    m["tree_info"] = [m["tree_info"][i] for i in keep]
    return out


def plant_thresholds(X, rows, model):
    """Every third of ``rows`` sits exactly on a root threshold of ``model`` (tests/test_gpu_xgb.py::frames)."""
    trees = model["learner"]["gradient_booster"]["model"]["trees"]
    for i, r in enumerate(rows[::3]):
        t = trees[i % len(trees)]
        if t["left_children"][0] != -1:
            X[r, t["split_indices"][0]] = t["split_conditions"][0]


def geometry(frames_per_song, songs_per_user, F=None, shuffled=False, seed=0):
    """(item_offsets, frame_offsets, frame_perm or None, owner [F] (-1: no song
    owns the row)) for songs of the given frame counts: grouped (position = row)
    or through a shuffled frame_perm over F rows."""
    f_off = np.concatenate([[0], np.cumsum(frames_per_song)]).astype(np.int64)
    items = np.concatenate([[0], np.cumsum(songs_per_user)]).astype(np.int64)
    n = int(f_off[-1])
    F = n if F is None else F
    perm = None
    rows = np.arange(n, dtype=np.int64)
    if shuffled:
        perm = np.random.default_rng(seed).permutation(F)[:n].astype(np.int64)
        rows = perm
    owner = np.full(F, -1, np.int64)
    song = np.full(F, -1, np.int64)
    for u in range(len(songs_per_user)):
        a, b = f_off[items[u]], f_off[items[u + 1]]
        owner[rows[a:b]] = u
    for g in range(len(frames_per_song)):
        song[rows[f_off[g]:f_off[g + 1]]] = g
    return items, f_off, perm, owner, song


def expected_proba(X, owner, models):
    """float32 [F, C]: row r by the oracle on models[owner[r]]; rows without an owner NaN."""
    C = XgbForest.from_json(models[0]).n_classes
    exp = np.full((X.shape[0], C), np.nan, np.float32)
    for u, m in enumerate(models):
        rows = np.flatnonzero(owner == u)
        if rows.size:
            exp[rows] = O.oracle_xgb_predict_proba(np.ascontiguousarray(X[rows]), m)
    return exp
