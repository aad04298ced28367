"""XGBoost forests for the on-device 'classifier_xgb' committee member
(amg_test.py:435/:467 -> xgboost/sklearn.py:991-1029).

The reference's member is ``XGBClassifier(max_depth=5, ...)`` from xgboost
1.3.3 (deam_classifier.py:226-232, requirements.txt:50), read back from
pickles.  Pickles are never loaded here; a forest comes from xgboost's own
JSON model format -- ``booster.save_model("m.json")`` (or ``save_raw`` in
later versions) -- whose schema this module parses:

    learner.learner_model_param.{base_score, num_class, num_feature}
    learner.objective.name                       multi:softprob | binary:logistic
    learner.gradient_booster.model.tree_info     group of tree t
    learner.gradient_booster.model.trees[t].{left_children, right_children,
        split_indices, split_conditions (the leaf value at a leaf), default_left}

``XgbForest.pack`` turns it into the device layout of ce_xgb_predict_proba:
perfect trees of the forest's depth, group-major.  ``synthetic_model`` makes a
random forest in that JSON schema (bench / tests: there is no network to fetch
a trained model, and the reference's pickles are untrusted).
"""
from __future__ import annotations

import ctypes
import ctypes.util
import json
import os

import numpy as np

# the member's limits, each mirroring a constant of csrc/ce_xgb.hpp
MAX_DEPTH = 10        # kXgbMaxDepth: packed perfect trees of at most 2^10 leaves
LANE_TABLE_DEPTH = 5  # kXgbLaneDepth: 2^(d+1) heap entries fit one wave (prebuilt lane tables)
MAX_FEATURES = 512    # kXgbMaxFeat: the LDS tile's columns
MAX_GROUPS = 8        # kXgbMaxGroups: margin chains (waves) per block

_libm = None


def _logf(x):
    """libm's logf (xgboost's ProbToMargin runs in float32 through it)."""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.logf.restype = ctypes.c_float
        _libm.logf.argtypes = [ctypes.c_float]
    return np.float32(_libm.logf(ctypes.c_float(x)))


class XgbForest:
    """A parsed xgboost 1.3 model: per-tree node arrays in model order."""

    def __init__(self, trees, tree_info, num_class, base_score, objective, num_feature):
        self.trees = trees                  # list of dicts of numpy arrays
        self.tree_info = np.asarray(tree_info, dtype=np.int32)
        self.num_class = int(num_class)     # 0 or 1 for binary:logistic (xgboost's convention)
        self.base_score = np.float32(base_score)
        self.objective = objective
        self.num_feature = int(num_feature)
        self._packed = None
        self._dev = {}

    # ---- construction -------------------------------------------------------
    @classmethod
    def from_json(cls, model):
        """``model``: a dict, a JSON string, or a path to ``booster.save_model(*.json)``."""
        if isinstance(model, (str, bytes, os.PathLike)):
            if isinstance(model, (str, os.PathLike)) and os.path.exists(model):
                with open(model) as fh:
                    model = json.load(fh)
            else:
                model = json.loads(model)
        lrn = model["learner"]
        mp = lrn["learner_model_param"]
        objective = lrn.get("objective", {}).get("name", "multi:softprob")
        if objective not in ("multi:softprob", "binary:logistic"):
            # multi:softmax's booster output is the class label; XGBClassifier.predict_proba
            # then returns [1 - label, label] (xgboost/sklearn.py:1025-1029), not probabilities
            raise ValueError(f"objective {objective!r} has no probability output (multi:softprob or "
                             "binary:logistic only)")
        gb = lrn["gradient_booster"]
        if gb.get("name", "gbtree") != "gbtree":
            raise ValueError(f"booster {gb.get('name')!r} unsupported (gbtree only)")
        m = gb["model"]
        trees = []
        for t in m["trees"]:
            tr = {
                "left": np.asarray(t["left_children"], dtype=np.int32),
                "right": np.asarray(t["right_children"], dtype=np.int32),
                "split": np.asarray(t["split_indices"], dtype=np.int32),
                "cond": np.asarray(t["split_conditions"], dtype=np.float32),
                "default_left": np.asarray([bool(v) for v in t["default_left"]], dtype=np.uint8),
            }
            n = tr["left"].size
            if not all(a.size == n for a in tr.values()) or n == 0:
                raise ValueError("inconsistent tree node arrays")
            trees.append(tr)
        return cls(trees, m["tree_info"], int(mp.get("num_class", "0")), float(mp["base_score"]), objective,
                   int(mp.get("num_feature", "0")))

    @classmethod
    def from_booster(cls, booster):  # pragma: no cover - xgboost is not installed in this image
        """From a live ``xgboost.Booster`` (or XGBClassifier): its JSON model."""
        import tempfile

        booster = booster.get_booster() if hasattr(booster, "get_booster") else booster
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "model.json")
            booster.save_model(path)
            return cls.from_json(path)

    # ---- derived geometry ---------------------------------------------------
    @property
    def n_groups(self):
        return 1 if self.objective == "binary:logistic" else self.num_class

    @property
    def n_classes(self):
        return 2 if self.objective == "binary:logistic" else self.num_class

    @property
    def base_margin(self):
        """xgboost's LearnerModelParam base margin: ProbToMargin(base_score)."""
        if self.objective == "binary:logistic":
            b = self.base_score
            return np.float32(-_logf(np.float32(np.float32(1.0) / b - np.float32(1.0))))
        return self.base_score

    def depth(self):
        d = 0
        for tr in self.trees:
            stack = [(0, 0)]
            while stack:
                nid, dep = stack.pop()
                if tr["left"][nid] == -1:
                    d = max(d, dep)
                else:
                    stack.append((int(tr["left"][nid]), dep + 1))
                    stack.append((int(tr["right"][nid]), dep + 1))
        return d

    # ---- the device layout --------------------------------------------------
    def pack(self, depth=None):
        """(nodes u32 [T, 2^d - 1, 2], leaves f32 [T, 2^d], group_offsets i32 [G+1], depth):
        perfect trees, group-major, model order inside a group.  ``depth``: pad
        to a common depth >= the forest's own (a deeper perfect tree repeats
        the leaf below it, so the bits do not change); cached per depth."""
        if self._packed is None:
            self._packed = {}
        if depth in self._packed:
            return self._packed[depth]
        G = self.n_groups
        if G < 1 or G > MAX_GROUPS:
            raise ValueError(f"{G} groups: 1..{MAX_GROUPS} supported")
        if self.tree_info.size != len(self.trees) or (self.tree_info.size and (
                self.tree_info.min() < 0 or self.tree_info.max() >= G)):
            raise ValueError("tree_info does not match the trees / groups")
        d = self.depth()
        if depth is not None:
            if int(depth) < d:
                raise ValueError(f"depth={depth} below the forest's own depth {d}")
            d = int(depth)
        if d > MAX_DEPTH:
            raise ValueError(f"tree depth {d} > {MAX_DEPTH}")
        NI, NL = (1 << d) - 1, 1 << d
        order = np.argsort(self.tree_info, kind="stable")  # group-major, model order kept
        T = len(self.trees)
        nodes = np.zeros((T, max(NI, 1), 2), dtype=np.uint32)
        leaves = np.zeros((T, NL), dtype=np.float32)
        for k, t in enumerate(order):
            tr = self.trees[t]
            # walk the model tree alongside the perfect tree: (model node, perfect index, depth)
            stack = [(0, 0, 0)]
            while stack:
                nid, pi, dep = stack.pop()
                if tr["left"][nid] == -1:
                    # a leaf at depth dep covers perfect leaves [lo, lo + 2^(d-dep))
                    lo = ((pi + 1) << (d - dep)) - 1 - NI
                    leaves[k, lo:lo + (1 << (d - dep))] = tr["cond"][nid]
                    continue  # internal nodes below it stay {0, +0.0}: either branch, same leaf
                f = int(tr["split"][nid])
                if f < 0 or f >= MAX_FEATURES or (self.num_feature and f >= self.num_feature):
                    raise ValueError(f"split feature {f} out of range")
                nodes[k, pi, 0] = np.uint32(f) | (np.uint32(1 << 31) if tr["default_left"][nid] else np.uint32(0))
                nodes[k, pi, 1] = np.float32(tr["cond"][nid]).view(np.uint32)
                stack.append((int(tr["left"][nid]), 2 * pi + 1, dep + 1))
                stack.append((int(tr["right"][nid]), 2 * pi + 2, dep + 1))
        counts = np.bincount(self.tree_info, minlength=G)
        goff = np.zeros(G + 1, dtype=np.int32)
        goff[1:] = np.cumsum(counts)
        self._packed[depth] = (nodes, leaves, goff, d)
        if depth is None:
            self._packed.setdefault(d, self._packed[None])
        return self._packed[depth]

    def max_feature(self):
        return max((int(tr["split"][tr["left"] != -1].max(initial=-1)) for tr in self.trees), default=-1)

    def lane_table(self, device, D):
        """The prebuilt per-tree lane tables of ce_xgb_predict_proba_lanes (depth
        <= 5): int32 [2, T, 64, 2] on ``device`` for X with D columns (with and
        without the default-left bits), built once on the device by
        ce_xgb_lane_table and cached per (device, D)."""
        import torch

        from . import _lib
        from .ops import _p, _stream, call

        key = (torch.device(device), int(D))
        if key not in self._dev:
            nodes, leaves, _, d = self.device_arrays(device)
            T = len(self.trees)
            table = torch.empty((2, T, 64, 2), dtype=torch.int32, device=key[0])
            _lib.load()
            call("ce_xgb_lane_table", _p(nodes), _p(leaves), T, d, int(D), _p(table), _stream(key[0]))
            self._dev[key] = table
        return self._dev[key]

    def device_arrays(self, device):
        """The packed arrays as device tensors (cached per device)."""
        import torch

        key = torch.device(device)
        if key not in self._dev:
            nodes, leaves, goff, d = self.pack()
            self._dev[key] = (torch.from_numpy(nodes.view(np.int32)).to(key),
                              torch.from_numpy(leaves).to(key), torch.from_numpy(goff).to(key), d)
        return self._dev[key]


def _as_forest(model):
    return model if isinstance(model, XgbForest) else XgbForest.from_json(model)


def _same_tree(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("left", "right", "split", "cond", "default_left"))


def continued_model(model, more):
    """What ``XGBClassifier.fit(X, y, xgb_model=booster)`` (amg_test.py:507)
    does to the booster's JSON, given the rounds it grew as a model of their
    own: a copy of ``model`` (a JSON dict) with ``more``'s trees appended, ids
    and ``tree_info`` continued.  ``base_score`` and the objective stay
    ``model``'s, as continued training keeps them."""
    import copy

    out = copy.deepcopy(model)
    m, mm = out["learner"]["gradient_booster"]["model"], more["learner"]["gradient_booster"]["model"]
    for k in ("objective", "learner_model_param"):
        a, b = model["learner"][k], more["learner"][k]
        if k == "objective":
            a, b = a.get("name"), b.get("name")
        else:
            a, b = int(a.get("num_class", "0")), int(b.get("num_class", "0"))
        if a != b:
            raise ValueError(f"continued_model: the models disagree on {k} ({a!r} vs {b!r})")
    for t in copy.deepcopy(mm["trees"]):
        t["id"] = len(m["trees"])
        m["trees"].append(t)
    m["tree_info"] = list(m["tree_info"]) + list(mm["tree_info"])
    m["gbtree_model_param"]["num_trees"] = str(len(m["trees"]))
    return out


def _check_against_base(base, f, u):
    """Raise ValueError where model u cannot share launches with the base."""
    for what in ("objective", "num_class", "num_feature"):
        if getattr(f, what) != getattr(base, what):
            raise ValueError(f"model {u} disagrees with the base on {what}: "
                             f"{getattr(f, what)!r} vs {getattr(base, what)!r}")
    if np.float32(f.base_score).view(np.uint32) != np.float32(base.base_score).view(np.uint32):
        raise ValueError(f"model {u} disagrees with the base on base_score: {f.base_score!r} vs {base.base_score!r}")


def _own_trees(base, f):
    """(continues, own): whether f's first trees are the base's (node arrays and
    tree_info), and the trees stored for it -- its tail then, else all of f --
    as an XgbForest of their own, which keeps their packed arrays per depth."""
    nb = len(base.trees)
    cont = f is base or (len(f.trees) >= nb and np.array_equal(f.tree_info[:nb], base.tree_info) and
                         all(_same_tree(f.trees[t], base.trees[t]) for t in range(nb)))
    own = XgbForest(f.trees[nb:] if cont else f.trees, f.tree_info[nb:] if cont else f.tree_info,
                    f.num_class, f.base_score, f.objective, f.num_feature)
    return cont, own


class StackedForests:
    """Many users' forests over one set of packed trees (csrc/ce_xgb_users.hpp).
    ``base``: the shared pretrained model; ``models[u]``: user u's FULL model
    (JSON, an XgbForest, or None for the base itself).  Where a model's first
    trees equal the base's (node arrays and tree_info) only its tail is stored;
    otherwise the whole forest is stored as the user's own trees.  Raises
    ValueError when a model disagrees with the base on the objective,
    num_class, base_score or the feature range, or when the common depth is
    above LANE_TABLE_DEPTH.

    The arrays -- ``nodes`` u32 [TT, 2^d - 1, 2], ``leaves`` f32 [TT, 2^d],
    ``tree_ids`` i32 [L], ``group_offsets`` i32 [U * G + 1], ``depth`` -- hold
    the base's trees first (group-major, as ``base.pack``), then every user's
    own; user u's group g owns tree_ids[group_offsets[u G + g] :
    group_offsets[u G + g + 1]], in the order the reference adds them to
    preds[g].  They are put together on first use and again after a ``set``:
    a ``set`` compares and packs the one model it is given, every other user's
    packed trees are kept, so the stacking itself is concatenation.
    ``device(device, D)`` builds the lane table for X with D columns
    (ce_xgb_lane_table) and caches it per (device, D) until the next ``set``."""

    def __init__(self, base, models):
        self.base = _as_forest(base)
        if len(models) < 1:
            raise ValueError("stack_forests needs at least one model")
        self.U, self.G, self.C = len(models), self.base.n_groups, self.base.n_classes
        self.base_margin = float(self.base.base_margin)
        self._base_depth, self._base_feature = self.base.depth(), self.base.max_feature()
        self._own = [self._entry(u, m) for u, m in enumerate(models)]
        self._check_depth(self._own)
        self._arrays, self._dev = None, {}

    def _entry(self, u, model):
        f = self.base if model is None else _as_forest(model)
        _check_against_base(self.base, f, u)
        cont, own = _own_trees(self.base, f)
        return cont, own, own.depth(), own.max_feature()  # both walk every tree: once per model

    def _check_depth(self, own):
        depth = max([self._base_depth] + [e[2] for e in own])
        if depth > LANE_TABLE_DEPTH:
            raise ValueError(f"common tree depth {depth} > {LANE_TABLE_DEPTH}: the users form holds lane tables only")
        return depth

    def set(self, u, model):
        """User u's full model from now on; raises before anything changes."""
        entry = self._entry(u, model)
        own = list(self._own)
        own[u] = entry
        self._check_depth(own)
        self._own, self._arrays, self._dev = own, None, {}

    def arrays(self):
        """(nodes, leaves, tree_ids, group_offsets, depth)."""
        if self._arrays is None:
            depth, G = self._check_depth(self._own), self.G
            bn, bl, bgoff, _ = self.base.pack(depth)
            base_ids = [np.arange(bgoff[g], bgoff[g + 1], dtype=np.int64) for g in range(G)]
            nodes, leaves, ids, goff = [bn], [bl], [], [0]
            row0 = len(self.base.trees)
            for cont, t, _, _ in self._own:
                tn, tl, tgoff, _ = t.pack(depth)
                nodes.append(tn)
                leaves.append(tl)
                for g in range(G):
                    if cont:
                        ids.append(base_ids[g])
                    ids.append(row0 + np.arange(tgoff[g], tgoff[g + 1], dtype=np.int64))
                    goff.append(goff[-1] + (len(base_ids[g]) if cont else 0) + int(tgoff[g + 1] - tgoff[g]))
                row0 += len(t.trees)
            if row0 >= 1 << 24 or goff[-1] >= 1 << 31:
                raise ValueError(f"{row0} stored trees / {goff[-1]} logical trees: too many for the users form")
            self._arrays = (np.concatenate(nodes), np.concatenate(leaves), np.concatenate(ids).astype(np.int32),
                            np.asarray(goff, dtype=np.int32), depth)
        return self._arrays

    nodes = property(lambda self: self.arrays()[0])
    leaves = property(lambda self: self.arrays()[1])
    tree_ids = property(lambda self: self.arrays()[2])
    group_offsets = property(lambda self: self.arrays()[3])
    depth = property(lambda self: self.arrays()[4])
    TT = property(lambda self: int(self.arrays()[0].shape[0]))
    L = property(lambda self: int(self.arrays()[2].shape[0]))

    @property
    def max_feature(self):
        """The highest feature a stored tree splits on (-1: none does)."""
        return max([self._base_feature] + [e[3] for e in self._own])

    def device(self, device, D):
        """(table i32 [2, TT, 64, 2], tree_ids i32 [L], group_offsets i32 [U G + 1]) on ``device``."""
        import torch

        from . import _lib
        from .ops import _p, _stream, call

        key = (torch.device(device), int(D))
        if key not in self._dev:
            dev = key[0]
            nodes, leaves, tree_ids, goff, depth = self.arrays()
            TT = int(nodes.shape[0])
            table = torch.zeros((2, max(TT, 1), 64, 2), dtype=torch.int32, device=dev)
            if TT:
                nd = torch.from_numpy(nodes.view(np.int32)).to(dev)
                lv = torch.from_numpy(leaves).to(dev)
                _lib.load()
                call("ce_xgb_lane_table", _p(nd), _p(lv), TT, depth, int(D), _p(table), _stream(dev))
            self._dev[key] = (table, torch.from_numpy(tree_ids).to(dev), torch.from_numpy(goff).to(dev))
        return self._dev[key]


def stack_forests(base, models):
    """``StackedForests(base, models).arrays()``: (nodes, leaves, tree_ids,
    group_offsets, depth) of many users' forests over one set of packed trees."""
    return StackedForests(base, models).arrays()


def synthetic_model(n_rounds=100, num_class=4, max_depth=5, num_feature=260, seed=1987, p_stop=0.15,
                    objective=None, threshold_scale=1.0):
    """A random xgboost-1.3-JSON forest: ``n_rounds`` boosting rounds x groups
    trees (tree t of round r belongs to group t % groups, as xgboost grows
    them), node ids allocated in expansion order, early leaves with
    probability ``p_stop`` per internal node below the root, thresholds and
    leaf weights float32, random default directions.  The reference's member
    is XGBClassifier(max_depth=5) on 260 standardised features, 4 classes."""
    rng = np.random.default_rng(seed)
    if objective is None:
        objective = "binary:logistic" if num_class <= 2 else "multi:softprob"
    groups = 1 if objective == "binary:logistic" else num_class
    trees, tree_info = [], []
    for r in range(n_rounds):
        for g in range(groups):
            left, right, split, cond, dflt = [], [], [], [], []

            def new_node():
                left.append(-1)
                right.append(-1)
                split.append(0)
                cond.append(0.0)
                dflt.append(0)
                return len(left) - 1

            root = new_node()
            frontier = [(root, 0)]
            while frontier:  # breadth-first, like xgboost's depthwise grower
                nxt = []
                for nid, dep in frontier:
                    leaf = dep >= max_depth or (dep > 0 and rng.random() < p_stop)
                    if leaf:
                        cond[nid] = float(np.float32(rng.normal(0.0, 0.2)))
                        continue
                    split[nid] = int(rng.integers(0, num_feature))
                    cond[nid] = float(np.float32(rng.normal(0.0, threshold_scale)))
                    dflt[nid] = int(rng.integers(0, 2))
                    lc, rc = new_node(), new_node()
                    left[nid], right[nid] = lc, rc
                    nxt += [(lc, dep + 1), (rc, dep + 1)]
                frontier = nxt
            n = len(left)
            trees.append({"tree_param": {"num_nodes": str(n), "num_feature": str(num_feature),
                                         "size_leaf_vector": "0", "num_deleted": "0"},
                          "id": len(trees), "left_children": left, "right_children": right,
                          "parents": [2147483647] + [0] * (n - 1), "split_indices": split,
                          "split_conditions": cond, "default_left": [bool(v) for v in dflt],
                          "loss_changes": [0.0] * n, "sum_hessian": [1.0] * n, "base_weights": [0.0] * n})
            tree_info.append(g)
    return {"learner": {
        "learner_model_param": {"base_score": "5E-1", "num_class": str(num_class if groups > 1 else 0),
                                "num_feature": str(num_feature)},
        "objective": {"name": objective},
        "gradient_booster": {"name": "gbtree", "model": {
            "gbtree_model_param": {"num_trees": str(len(trees)), "size_leaf_vector": "0"},
            "trees": trees, "tree_info": tree_info}},
        "attributes": {}, "feature_names": [], "feature_types": []},
        "version": [1, 3, 3]}
