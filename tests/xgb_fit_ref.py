"""XGBClassifier(max_depth=5).fit(X_batch, y, xgb_model=booster) restated row by
row: the boosting rounds the reference grows at amg_test.py:507 on its
'classifier_xgb' member (deam_classifier.py:227-231), as xgboost 1.3.3's exact
grower (grow_colmaker on dense columns, one thread) is read here.  xgboost's
C++ core is in no image of this project, so this file IS the arithmetic
contract of ce_xgb_fit_users (0 differing bits); parity with xgboost 1.3.3
itself is unpinned (DESIGN.md §3 lists every choice, next to the predictor's).

objective multi:softprob, eta 0.3f, lambda 1, alpha 0, gamma 0,
min_child_weight 1, max_delta_step 0, no subsampling, tree_method exact.

Every operation is a numpy float32 or Python float (IEEE double) scalar
operation, or the C library's expf; sums run one term after the other.
``brute_check`` recomputes every split of a grown tree from scratch."""
import math

import numpy as np

from oracle.ce_oracle import libm_expf

F32 = np.float32
RT_EPS = F32(1e-6)      # kRtEps: the least loss_chg that splits a node
MIN_HESS = F32(1e-16)   # multi:softprob's floor of the hessian
MAX_NODES = 63          # a depth-5 tree


def softmax_row(m):
    """common::Softmax, as oracle/ce_oracle.c:ce_ref_xgb_predict_proba: fmaxf
    maximum, expf, a double wsum, each e divided by (float)wsum."""
    mx = m[0]
    for v in m[1:]:
        mx = F32(max(v, mx))
    e = [libm_expf(F32(v - mx)) for v in m]
    ws = 0.0
    for v in e:
        ws += float(v)
    ws = F32(ws)
    return [F32(v / ws) for v in e]


def gradients(m, y):
    """(g, h) float32 [n, C] from the margins m [n, C] and labels y [n]."""
    n, C = m.shape
    g, h = np.empty((n, C), F32), np.empty((n, C), F32)
    for i in range(n):
        p = softmax_row([m[i, k] for k in range(C)])
        for k in range(C):
            g[i, k] = F32(p[k] - (F32(1.0) if int(y[i]) == k else F32(0.0)))
            h[i, k] = F32(max(F32(F32(F32(2.0) * p[k]) * F32(F32(1.0) - p[k])), MIN_HESS))
    return g, h


def gain(G, H, lam):
    """G^2 / (H + lambda) as an IEEE double division: at lambda = 0 a side whose
    hessians cancel to 0.0 gives inf (nan from 0 / 0), which need_replace skips."""
    d = H + lam
    if d == 0.0:
        return math.nan if G == 0.0 else math.inf
    return G * G / d


def need_replace(best, loss_chg, f):
    """SplitEntry::NeedReplace: a candidate replaces the best only when its
    loss_chg is finite; an incumbent of a lower or the same feature only gives
    way to a strictly greater loss_chg, one of a higher feature to an equal one."""
    if not math.isfinite(float(loss_chg)):
        return False
    if best[1] <= f:
        return bool(loss_chg > best[0])
    return not bool(best[0] > loss_chg)


def scan_order(X):
    """Per feature, the batch rows in the order the backward scan meets them:
    sorted by the feature ascending, stable by batch position, from the high end."""
    return [np.argsort(X[:, f], kind="stable")[::-1] for f in range(X.shape[1])]


def node_sums(g, h, pos, nid):
    """double sums of the float g, h over the node's rows in batch order."""
    G = H = 0.0
    for i in range(len(pos)):
        if pos[i] == nid:
            G += float(g[i])
            H += float(h[i])
    return G, H


TIES = {"feature": 0, "scan": 0}  # exact loss_chg ties met so far: between two features / within one feature's scan
SKIPPED = {"non_finite": 0}       # candidates met so far whose loss_chg was inf or nan


def grow_tree(X, order, g, h, max_depth, eta, lam, mcw, log=None):
    """One tree from the gradients (g, h) [n] of its group.  Returns (tree, pos):
    the XgbForest node arrays and each row's leaf.  ``log``: a list that takes,
    per split node, (rows of the node, G, H, root_gain, chosen (loss_chg, f, cond), g, h)."""
    n, D = X.shape
    left, right, split, cond, dl = [-1], [-1], [0], [F32(0.0)], [0]
    pos = np.zeros(n, np.int64)
    is_open = [0]
    lam, mcw, eta = float(F32(lam)), float(F32(mcw)), F32(eta)
    for depth in range(max_depth + 1):
        stats = {}
        for nid in is_open:
            G, H = node_sums(g, h, pos, nid)
            stats[nid] = (G, H, F32(-G / (H + lam)), F32(gain(G, H, lam)))
        if depth == max_depth:
            for nid in is_open:
                cond[nid] = F32(stats[nid][2] * eta)
            break
        best = {nid: (F32(0.0), 0, F32(0.0)) for nid in is_open}
        for f in range(D):
            e = {nid: [0.0, 0.0, F32(0.0), False] for nid in is_open}  # G, H, last, seen
            for i in order[f]:
                nid = int(pos[i])
                if nid not in e:
                    continue
                fv, en = X[i, f], e[nid]
                if en[3] and fv != en[2] and en[1] >= mcw:
                    cG, cH = stats[nid][0] - en[0], stats[nid][1] - en[1]
                    if cH >= mcw:
                        loss_chg = F32(gain(cG, cH, lam) + gain(en[0], en[1], lam) - float(stats[nid][3]))
                        if not math.isfinite(float(loss_chg)):
                            SKIPPED["non_finite"] += 1
                        if loss_chg == best[nid][0] and loss_chg > F32(0.0):
                            TIES["scan" if best[nid][1] == f else "feature"] += 1
                        if need_replace(best[nid], loss_chg, f):
                            best[nid] = (loss_chg, f, F32(F32(fv + en[2]) * F32(0.5)))
                en[0] += float(g[i])
                en[1] += float(h[i])
                en[2], en[3] = fv, True
            # the end-of-column candidate (everything to the right) never fires on a dense
            # column: its left side c = node - e holds no row, so c.H < min_child_weight
        nxt = []
        for nid in is_open:
            lc, f, c = best[nid]
            if lc > RT_EPS:
                if log is not None:
                    log.append((np.flatnonzero(pos == nid), stats[nid][0], stats[nid][1], stats[nid][3], best[nid], g, h))
                l, r = len(left), len(left) + 1
                for a, v in ((left, -1), (right, -1), (split, 0), (cond, F32(0.0)), (dl, 0)):
                    a.extend([v, v])
                left[nid], right[nid], split[nid], cond[nid], dl[nid] = l, r, f, c, 1
                nxt += [l, r]
            else:
                cond[nid] = F32(stats[nid][2] * eta)
        for i in range(n):
            nid = int(pos[i])
            if left[nid] != -1:
                pos[i] = left[nid] if X[i, split[nid]] < cond[nid] else right[nid]
        is_open = nxt
        if not is_open:
            break
    tree = {"left": np.asarray(left, np.int32), "right": np.asarray(right, np.int32),
            "split": np.asarray(split, np.int32), "cond": np.asarray(cond, F32),
            "default_left": np.asarray(dl, np.uint8)}
    return tree, pos


def fit_rounds(X, y, margins, rounds, max_depth=5, eta=0.3, lam=1.0, mcw=1.0, log=None):
    """``rounds`` boosting rounds on the batch X [n, D] (cast to float32, dense
    and finite), labels y [n] in [0, C), start margins [n, C] float32.  Returns
    (trees, tree_info, margins): rounds * C trees, round-major, group inside
    the round, and the batch's final margins.  No row: no tree."""
    X = np.ascontiguousarray(np.asarray(X, np.float64).astype(F32))
    m = np.array(margins, F32)
    n, C = m.shape
    if n == 0:
        return [], [], m
    assert np.isfinite(X).all() and X.shape[0] == n
    order = scan_order(X)
    trees, info = [], []
    for _ in range(rounds):
        g, h = gradients(m, y)
        for k in range(C):
            tree, pos = grow_tree(X, order, g[:, k], h[:, k], max_depth, eta, lam, mcw, log)
            for i in range(n):
                m[i, k] = F32(m[i, k] + tree["cond"][pos[i]])
            trees.append(tree)
            info.append(k)
    return trees, info, m


def start_margins(X, forest):
    """float32 [n, G]: base_margin plus the leaves of the forest's trees of each
    group, in model order (the order the users walk adds them)."""
    X = np.asarray(X, np.float64).astype(F32)
    m = np.full((X.shape[0], forest.n_groups), forest.base_margin, F32)
    for tr, k in zip(forest.trees, forest.tree_info):
        for i in range(X.shape[0]):
            nid = 0
            while tr["left"][nid] != -1:
                nid = tr["left"][nid] if X[i, tr["split"][nid]] < tr["cond"][nid] else tr["right"][nid]
            m[i, k] = F32(m[i, k] + tr["cond"][nid])
    return m


def fit_forest(forest, X, y, rounds, max_depth=5, log=None, **kw):
    """The forest after ``fit(X, y, xgb_model=forest)``: its trees, then the grown rounds; and the final margins."""
    from ce_amd.xgb import XgbForest

    trees, info, m = fit_rounds(X, y, start_margins(X, forest), rounds, max_depth, log=log, **kw)
    out = XgbForest(list(forest.trees) + trees, list(forest.tree_info) + info, forest.num_class, forest.base_score,
                    forest.objective, forest.num_feature)
    return out, m


def tree_json(tr, num_feature):
    """One grown tree in xgboost's JSON schema (what continued_model appends)."""
    n = int(tr["left"].size)
    return {"tree_param": {"num_nodes": str(n), "num_feature": str(num_feature), "size_leaf_vector": "0",
                           "num_deleted": "0"},
            "id": 0, "left_children": tr["left"].tolist(), "right_children": tr["right"].tolist(),
            "parents": [2147483647] + [0] * (n - 1), "split_indices": tr["split"].tolist(),
            "split_conditions": [float(v) for v in tr["cond"]], "default_left": [bool(v) for v in tr["default_left"]],
            "loss_changes": [0.0] * n, "sum_hessian": [1.0] * n, "base_weights": [0.0] * n}


def rounds_model(base_model, trees, info):
    """The grown rounds as a JSON model of their own (continued_model's ``more``)."""
    import copy

    out = copy.deepcopy(base_model)
    m = out["learner"]["gradient_booster"]["model"]
    nf = int(out["learner"]["learner_model_param"].get("num_feature", "0"))
    m["trees"] = [dict(tree_json(t, nf), id=i) for i, t in enumerate(trees)]
    m["tree_info"] = [int(k) for k in info]
    m["gbtree_model_param"]["num_trees"] = str(len(trees))
    return out


def brute_check(X, entry, lam=1.0, mcw=1.0):
    """The independent check of one split node (``entry`` of grow_tree's log):
    for every feature and every threshold between two distinct values of the
    node's rows, the right side summed afresh in scan order, the left side as
    node minus right; the best by the tie rule, the features taken in
    DESCENDING order (so the ``!(best > new)`` half of the rule decides the
    ties between features).  Returns the (loss_chg, f, cond) it finds."""
    X = np.asarray(X, np.float64).astype(F32)
    rows, G, H, root_gain, _, g, h = entry
    lam, mcw = float(F32(lam)), float(F32(mcw))
    inside = set(int(i) for i in rows)
    best = (F32(0.0), 0, F32(0.0))
    for f in range(X.shape[1] - 1, -1, -1):
        seq = [int(i) for i in np.argsort(X[:, f], kind="stable")[::-1] if int(i) in inside]
        own = (F32(0.0), f, F32(0.0))  # within the feature: the first of the descending scan wins a tie
        for cut in range(1, len(seq)):
            hi, lo = X[seq[cut - 1], f], X[seq[cut], f]
            if hi == lo:
                continue
            eG = eH = 0.0
            for i in seq[:cut]:
                eG += float(g[i])
                eH += float(h[i])
            cG, cH = G - eG, H - eH
            if eH < mcw or cH < mcw:
                continue
            lc = F32(gain(cG, cH, lam) + gain(eG, eH, lam) - float(root_gain))
            if math.isfinite(float(lc)) and lc > own[0]:
                own = (lc, f, F32(F32(lo + hi) * F32(0.5)))
        if own[0] > F32(0.0) and need_replace(best, own[0], f):
            best = own
    return best


def batch(n, D, C, kind="ties", seed=0):
    """A batch (X f64 [n, D], y [n]) of the parity tests.  Every kind has
    feature 0 quantised to four values, q and 3 - q on rows 2 j and 2 j + 1 of
    one label (mirrored class counts: exact loss_chg ties within the scan from
    uniform margins), and the last column a copy of it when D > 1 (exact ties
    between two features); the labels follow the features, so trees grow deep.
      ties     further columns rounded to one decimal (many equal values)
      const    one constant column
      single   one label only
      lacking  the last class absent from the batch
      mirror   the labels are the pairs' alone (the mirrored counts hold for every class)
      hand     the hand-worked shape: column 0 counts the rows, the upper half is class 1
      last     the four values sit in the LAST column, column 0 is their upper bit: the cuts 0.5 and
               2.5 exist in the last column alone, the cut 1.5 in both (an exact tie that column 0
               wins); most labels are 0, 1, 1, 2 by the value, so the trees want the outer cuts"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, D))
    q = rng.integers(0, 4, (n + 1) // 2)
    X[:, 0] = np.where(np.arange(n) % 2 == 0, q[np.arange(n) // 2], 3 - q[np.arange(n) // 2]).astype(np.float64)
    yj = rng.integers(0, C, (n + 1) // 2)
    y = yj[np.arange(n) // 2]
    if D > 2:
        rule = (np.floor(2.0 * X[:, 1]).astype(np.int64) + (X[:, D // 2] > 0)) % C
        y = y if kind == "mirror" else np.where(rng.random(n) < 0.5, rule, y)
        X[:, 1:D - 1] = np.round(X[:, 1:D - 1], 1) if kind in ("ties", "last") else X[:, 1:D - 1]
    if D > 1:
        X[:, D - 1] = X[:, 0]
    if kind == "const" and D > 2:
        X[:, D // 2] = 1.25
    if kind == "single":
        y = np.full(n, 1)
    if kind == "lacking":
        y = y % (C - 1)
    if kind == "hand":
        X[:, 0] = np.arange(n)
        y = (2 * np.arange(n) >= n).astype(np.int64)
    if kind == "last":
        y = np.where(rng.random(n) < 0.8, np.array([0, 1, 1, 2])[X[:, D - 1].astype(np.int64)] % C, y)
        X[:, 0] = np.floor(X[:, D - 1] / 2.0)
    return X, y.astype(np.int64)


def same_tree(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("left", "right", "split", "default_left")) \
        and np.array_equal(np.asarray(a["cond"], F32).view(np.uint32), np.asarray(b["cond"], F32).view(np.uint32))


# ---- what the kernel writes, and the inputs the CPU and GPU tests share -------------
def expected_outputs(per_user, U, rounds, G, depth):
    """ce_xgb_fit_users' outputs as numpy arrays, from every user's grown trees
    (``per_user[u]``: rounds * G trees in model order, or an empty list): slot
    (u rounds + r) G + k; the slots of a user without trees stay as the wrapper
    allocates them (zero, children -1)."""
    from ce_amd.xgb import XgbForest

    T, NI, NL = U * rounds * G, max((1 << depth) - 1, 1), 1 << depth
    out = {"nodes": np.zeros((T, NI, 2), np.uint32), "leaves": np.zeros((T, NL), F32),
           "left": np.full((T, MAX_NODES), -1, np.int32), "right": np.full((T, MAX_NODES), -1, np.int32),
           "split": np.zeros((T, MAX_NODES), np.int32), "cond": np.zeros((T, MAX_NODES), F32),
           "default_left": np.zeros((T, MAX_NODES), np.uint8), "num_nodes": np.zeros(T, np.int32)}
    for u, trees in enumerate(per_user):
        for j, tr in enumerate(trees):
            t, n = u * rounds * G + j, tr["left"].size
            nodes, leaves, _, _ = XgbForest([tr], [0], G, 0.5, "multi:softprob", 0).pack(depth)
            out["nodes"][t], out["leaves"][t], out["num_nodes"][t] = nodes[0], leaves[0], n
            for k in ("left", "right", "split", "cond", "default_left"):
                out[k][t, :n] = tr[k]
    return out


def grown_chunk(per_user, U, rounds, G, depth, device="cpu"):
    """The ``ce_amd.xgb.GrownTrees`` a fit that grew ``per_user`` hands to the stack."""
    import torch

    from ce_amd.xgb import GrownTrees

    out = expected_outputs(per_user, U, rounds, G, depth)
    t = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(device) for k, v in out.items()}
    return GrownTrees(t, U, rounds, G, depth, [len(p) > 0 for p in per_user])


# name: D, C, rounds, max_depth, each user's rows, each user's kind of batch, base rounds (0: leaves only,
# so every row starts from the same margins), X as float64
CASES = {
    "deep":    dict(D=5, C=4, rounds=3, max_depth=5, rows=(130, 0, 65), kinds=("ties", "ties", "const"), base=2, f64=True),
    "tiny":    dict(D=1, C=3, rounds=1, max_depth=1, rows=(6, 1, 7), kinds=("hand", "hand", "hand"), base=0, f64=False),
    "wide":    dict(D=70, C=3, rounds=1, max_depth=3, rows=(65, 7, 130), kinds=("single", "lacking", "ties"), base=2,
                    f64=True),
    "uniform": dict(D=5, C=4, rounds=1, max_depth=3, rows=(130, 6, 0), kinds=("mirror", "ties", "ties"), base=0, f64=False),
}
# The edge cases of tests/test_gpu_xgb_fit_edges.py: the kernel's own limits (the 4096-row cap, the rows taken 8
# and blockDim at a time, 63-node trees, the one-wave / two-wave / above-64-KiB-LDS feature counts, 8 groups, the
# three parameters, more users than compute units, a row stride, special values).  As CASES, with EDGE_DEFAULTS and:
#   seeds    each user's batch seed (100 + u when absent)
#   eta, lam, mcw   the fit's parameters
#   pad      padding columns behind X's D (the device test fills them with NaN)
#   values   special feature values, see ``special_values``
#   flagged  users whose batch the fit must flag 1 and leave alone
#   base     "steep": ``steep_model``, start margins 80 apart -- rows whose hessian is the 1e-16 floor next to rows
#            of 0.5, so that at lambda = 0 and min_child_weight = 0 a side's hessians cancel to 0.0 (loss_chg inf)
EDGE_DEFAULTS = dict(C=3, rounds=1, base=0, f64=False, eta=0.3, lam=1.0, mcw=1.0, pad=0, values=None, flagged=())
EDGE_CASES = {
    "rows8":     dict(D=3, max_depth=3, rows=(7, 8, 9)),
    "rows64":    dict(D=3, max_depth=3, rows=(63, 64, 65)),
    "rows512":   dict(D=3, max_depth=3, rows=(255, 256, 257, 0, 513)),
    "cap":       dict(D=4, max_depth=5, rows=(4096, 4095, 1)),
    "full":      dict(D=4, max_depth=5, rounds=2, rows=(1024, 2048), seeds=(8, 0)),
    "d64":       dict(D=64, max_depth=3, rows=(65, 7), kinds=("last", "ties")),
    "d65":       dict(D=65, max_depth=3, rows=(65, 7), kinds=("last", "ties")),
    "d257":      dict(D=257, max_depth=3, rows=(40, 3), kinds=("last", "ties")),
    "d512":      dict(D=512, max_depth=5, rows=(16, 130), kinds=("ties", "last"), seeds=(100, 1)),
    "d512cap":   dict(D=512, max_depth=1, rows=(4096,)),
    "groups8":   dict(D=5, C=8, max_depth=5, rounds=2, rows=(130, 9)),
    "params_a":  dict(D=5, max_depth=5, rounds=2, rows=(257,), eta=1.0, lam=3.5, mcw=2.5),
    "params_b":  dict(D=5, max_depth=5, rows=(257,), eta=0.3, lam=0.0, mcw=0.0),
    "params_c":  dict(D=5, max_depth=5, rows=(257,), eta=0.05, lam=0.0, mcw=1.0),
    "many":      dict(D=3, max_depth=2, rows=tuple(u % 13 for u in range(300))),
    "pad32":     dict(D=5, max_depth=3, rows=(65, 9), pad=3),
    "pad64":     dict(D=5, max_depth=3, rows=(65, 9), pad=3, f64=True),
    "denormal":  dict(D=4, max_depth=3, rows=(64, 9), values="denormal"),
    "collide":   dict(D=4, max_depth=3, rows=(65, 9), values="collide", f64=True),
    "twice":     dict(D=4, max_depth=3, rows=(65, 9), values="twice"),
    "overflow":  dict(D=4, max_depth=3, rows=(65, 9, 16), values="overflow", f64=True, flagged=(1,)),
    "steep":     dict(D=4, max_depth=3, rows=(65, 9), lam=0.0, mcw=0.0, base="steep"),
}
PARAM_CASES = ("params_a", "params_b", "params_c")
_CACHE = {}


def special_values(kind, Xu, yu, C, rng):
    """The batch (Xu, yu) with the special values of ``kind`` written into it; returns the labels.
      denormal  column 1 drawn from signed zeros, denormals and the least normal float, column 2 half of it
                (in float32), most labels following column 1's sign
      collide   column 1: float32 values moved by a few parts in 1e10, so distinct doubles cast to equal
                floats and the stable order (not the doubles' order) decides them
      overflow  one entry of 1e39: a finite double, infinite as a float
    (``twice`` is a matter of the row list, see ``case``.)"""
    n = Xu.shape[0]
    if kind == "denormal":
        vals = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3e-39, 1.17549435e-38, -1.17549435e-38])
        col = vals[rng.integers(0, vals.size, n)]
        Xu[:, 1] = col
        Xu[:, 2] = (col.astype(F32) * F32(0.5)).astype(np.float64)
        follow = np.where(col > 0, 1, np.where(col < 0, 0, 2)) % C
        return np.where(rng.random(n) < 0.7, follow, yu)
    if kind == "collide":
        col = Xu[:, 1].astype(F32).astype(np.float64)
        Xu[:, 1] = col * (1.0 + 1e-10 * rng.integers(-3, 4, n))
        assert np.array_equal(Xu[:, 1].astype(F32), col.astype(F32)) and (Xu[:, 1] != col).any()
    if kind == "overflow":
        Xu[min(3, n - 1), 2] = 1e39
    return yu


def steep_model(C, D):
    """A base of one tree per group: group 0's cuts feature 1 at 0 into leaves of +40 and -40, the others are one
    leaf of 0.  A row left of the cut has p = (1, e^-40, ...) as floats, one right of it (e^-40, 1 / (C - 1), ...)."""
    from ce_amd.xgb import synthetic_model

    cut = {"left": np.array([1, -1, -1], np.int32), "right": np.array([2, -1, -1], np.int32),
           "split": np.array([1, 0, 0], np.int32), "cond": np.array([0.0, 40.0, -40.0], F32),
           "default_left": np.array([1, 0, 0], np.uint8)}
    leaf = {"left": np.array([-1], np.int32), "right": np.array([-1], np.int32), "split": np.array([0], np.int32),
            "cond": np.array([0.0], F32), "default_left": np.array([0], np.uint8)}
    flat = synthetic_model(n_rounds=1, num_class=C, max_depth=0, num_feature=D, seed=11)
    return rounds_model(flat, [cut] + [leaf] * (C - 1), list(range(C)))


def case(name):
    """The inputs of a parity case, and what the restatement grows from them
    (computed once).  A dict: base (JSON), X [F, D] (rows no user owns
    included), rows / labels / row_offsets (every user's rows in a shuffled
    order, stacked), per_user (grown trees), info, margins (final, stacked; a
    flagged user's stay 0), forests (each user's XgbForest after the fit),
    status (the flags the fit must return)."""
    if name in _CACHE:
        return _CACHE[name]
    from ce_amd.xgb import XgbForest, synthetic_model

    c = dict(CASES[name]) if name in CASES else dict(EDGE_DEFAULTS, **EDGE_CASES[name])
    D, C, U = c["D"], c["C"], len(c["rows"])
    kinds, seeds = c.get("kinds", ("ties",) * U), c.get("seeds", tuple(100 + u for u in range(U)))
    kw = {k: c[k] for k in ("eta", "lam", "mcw") if k in c}
    rng = np.random.default_rng(sum(map(ord, name)))
    if c["base"] == "steep":
        base = steep_model(C, D)
    elif c["base"]:
        base = synthetic_model(n_rounds=c["base"], num_class=C, max_depth=3, num_feature=D, seed=11)
    else:
        base = synthetic_model(n_rounds=1, num_class=C, max_depth=0, num_feature=D, seed=11)
    forest = XgbForest.from_json(base)
    F = sum(c["rows"]) + 7
    X = rng.normal(size=(F, D))
    perm = rng.permutation(F)
    rows, labels, off, at = [], [], [0], 0
    per_user, margins, forests = [], [], []
    for u, n in enumerate(c["rows"]):
        r = perm[at:at + n].copy()
        at += n
        Xu, yu = batch(n, D, C, kinds[u], seed=seeds[u])
        if c.get("values") and (c["values"] != "overflow" or u in c["flagged"]):
            yu = special_values(c["values"], Xu, yu, C, rng)
        X[r] = Xu
        if c.get("values") == "twice" and n > 5:  # the batch lists two rows of X twice, under their own labels
            r[5], r[n - 1] = r[2], r[0]
        if not c["f64"]:
            X = X.astype(F32).astype(np.float64)
        rows.append(r)
        labels.append(yu)
        off.append(off[-1] + n)
        if u in c.get("flagged", ()):  # not run: no tree, and its margins stay as they were allocated
            after, m = forest, np.zeros((n, C), F32)
        else:
            after, m = fit_forest(forest, X[r], yu, c["rounds"], c["max_depth"], **kw)
        per_user.append(after.trees[len(forest.trees):])
        margins.append(m)
        forests.append(after)
    c.update(base=base, forest=forest, X=X, U=U, counts=tuple(c["rows"]), rows=np.concatenate(rows).astype(np.int64),
             labels=np.concatenate(labels).astype(np.int32), row_offsets=np.asarray(off, np.int64),
             per_user=per_user, margins=np.concatenate(margins), forests=forests, kw=kw,
             status=[1 if u in c.get("flagged", ()) else 0 for u in range(U)],
             info=[k for _ in range(c["rounds"]) for k in range(C)])
    _CACHE[name] = c
    return c


def full_model(base, trees, info):
    """The JSON model after the fit: ``continued_model`` of the base and the grown rounds."""
    from ce_amd.xgb import continued_model

    return continued_model(base, rounds_model(base, trees, info)) if trees else base
