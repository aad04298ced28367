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


class GrownTrees:
    """The trees one ``ops.xgb_fit_users`` call grew, on the device: slot
    (u * rounds + r) * G + k holds round r, group k of user u, in the packed
    form (``nodes``, ``leaves`` at ``depth``) and as the model's own node arrays
    (``left``, ``right``, ``split``, ``cond``, ``default_left`` [T, 63],
    ``num_nodes`` [T]).  ``active[u]``: user u's slots hold trees that are part
    of its forest (it had rows, was not flagged, and no ``set`` replaced them).
    ``host()`` copies the node arrays to the host, once, when someone asks.
    Both forms stay on the device for as long as the stack refers to the call
    (the packed form rebuilds lane tables after a ``set`` or for another D, the
    node arrays are the model): about 1.45 KB per slot, slots of users without
    new trees included -- 290 MB for 500 users x 100 rounds x 4 groups."""

    NAMES = ("left", "right", "split", "cond", "default_left", "num_nodes")

    def __init__(self, out, U, rounds, G, depth, active):
        self.out, self.U, self.rounds, self.G, self.depth = out, int(U), int(rounds), int(G), int(depth)
        self.active = np.array(active, dtype=bool)
        self.T = self.U * self.rounds * self.G
        self._host = self._packed = None

    def host(self):
        if self._host is None:
            self._host = {k: self.out[k].cpu().numpy() for k in self.NAMES}
        return self._host

    def packed(self):
        """(nodes u32 [T, NI, 2], leaves f32 [T, NL]) read back."""
        if self._packed is None:
            self._packed = (self.out["nodes"].cpu().numpy().view(np.uint32), self.out["leaves"].cpu().numpy())
        return self._packed

    def trees(self, u):
        """User u's trees of this call in model order (round-major, group inside the round), and their groups."""
        if not self.active[u]:
            return [], []
        h, trees, info = self.host(), [], []
        for r in range(self.rounds):
            for k in range(self.G):
                t = (u * self.rounds + r) * self.G + k
                n = int(h["num_nodes"][t])
                trees.append({"left": h["left"][t, :n].copy(), "right": h["right"][t, :n].copy(),
                              "split": h["split"][t, :n].copy(), "cond": h["cond"][t, :n].copy(),
                              "default_left": h["default_left"][t, :n].copy()})
                info.append(k)
        return trees, info

    def ids(self, u, g, row0):
        """The table rows of user u's trees of group g, in round order."""
        return row0 + (u * self.rounds + np.arange(self.rounds, dtype=np.int64)) * self.G + g


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
    own, then the trees grown on the device (``grow``: one GrownTrees per fit
    call, in call order); user u's group g owns tree_ids[group_offsets[u G + g]
    : group_offsets[u G + g + 1]], in the order the reference adds them to
    preds[g].  The host-packed part is put together on first use and again
    after a ``set``: a ``set`` compares and packs the one model it is given,
    every other user's packed trees are kept, so the stacking itself is
    concatenation.  ``device(device, D)`` builds the lane table for X with D
    columns (ce_xgb_lane_table) and caches it per (device, D) until the next
    ``set``.

    Device-grown tails: ``grow`` writes the new trees' lane tables straight
    after the existing ones -- the table is kept with spare capacity and grown
    geometrically when full -- and rebuilds ``tree_ids`` / ``group_offsets`` on
    the host from per-user tree counts (index arithmetic; no tree content
    crosses the bus).  ``forest(u)`` and the host arrays read the grown trees
    back only when asked.  ``set(u, ...)`` replaces user u's whole tail, grown
    trees included.  Memory grows with every fit: the lane table by 1 KB
    per new tree (and it doubles when full), and the call's GrownTrees stays
    on the device (1.45 KB per tree slot) until a ``set`` of every user it
    served, or a change of the common depth, releases it."""

    def __init__(self, base, models):
        self.base = _as_forest(base)
        if len(models) < 1:
            raise ValueError("stack_forests needs at least one model")
        self.U, self.G, self.C = len(models), self.base.n_groups, self.base.n_classes
        self.base_margin = float(self.base.base_margin)
        self._base_depth, self._base_feature = self.base.depth(), self.base.max_feature()
        self._min_depth, self._chunks, self._grown_feature, self._merged = 0, [], -1, set()
        self._own = [self._entry(u, m) for u, m in enumerate(models)]
        self._check_depth(self._own)
        self._host, self._arrays, self._dev = None, None, {}

    def _entry(self, u, model):
        f = self.base if model is None else _as_forest(model)
        _check_against_base(self.base, f, u)
        cont, own = _own_trees(self.base, f)
        return cont, own, own.depth(), own.max_feature()  # both walk every tree: once per model

    def _check_depth(self, own):
        depth = max([self._base_depth, self._min_depth] + [e[2] for e in own])
        if depth > LANE_TABLE_DEPTH:
            raise ValueError(f"common tree depth {depth} > {LANE_TABLE_DEPTH}: the users form holds lane tables only")
        return depth

    def _materialise(self):
        """Every device-grown tree becomes a host tree of its user's own forest
        (one read-back): what a change of the common depth needs, since the
        grown trees are packed at the depth of their fit."""
        if not self._chunks:
            return
        own = list(self._own)
        for u in range(self.U):
            trees, info = self.grown_trees(u)
            if trees:
                cont, t, _, _ = own[u]
                f = XgbForest(list(t.trees) + trees, list(t.tree_info) + info, t.num_class, t.base_score, t.objective,
                              t.num_feature)
                own[u] = (cont, f, f.depth(), f.max_feature())
                self._merged.add(u)
        self._own, self._chunks, self._grown_feature = own, [], -1
        self._host, self._arrays, self._dev = None, None, {}

    def set(self, u, model):
        """User u's full model from now on; raises before anything changes."""
        entry = self._entry(u, model)
        own = list(self._own)
        own[u] = entry
        depth = self._check_depth(own)
        if self._chunks and depth != self._check_depth(self._own):
            self._materialise()
            own = list(self._own)
            own[u] = entry
        self._merged.discard(u)
        for c in self._chunks:
            c.active[u] = False
        self._chunks = [c for c in self._chunks if c.active.any()]
        self._own, self._host, self._arrays, self._dev = own, None, None, {}

    def ensure_depth(self, depth):
        """The common depth from now on is at least ``depth`` (a fit of deeper
        trees): the stack is packed again at the new depth on next use."""
        depth = int(depth)
        if depth > LANE_TABLE_DEPTH:
            raise ValueError(f"depth {depth} > {LANE_TABLE_DEPTH}: the users form holds lane tables only")
        if depth > self._check_depth(self._own):
            self._materialise()
            self._min_depth = depth
            self._host, self._arrays, self._dev = None, None, {}

    def grown_trees(self, u):
        """User u's device-grown trees in model order and their groups (read back)."""
        trees, info = [], []
        for c in self._chunks:
            t, i = c.trees(u)
            trees += t
            info += i
        return trees, info

    def n_grown(self, u):
        """How many device-grown trees user u's forest holds (a host number)."""
        return sum(c.rounds * c.G for c in self._chunks if c.active[u])

    def has_grown(self, u):
        """Whether user u's forest holds trees grown on the device (still there, or since merged into its own)."""
        return u in self._merged or self.n_grown(u) > 0

    def forest(self, u):
        """User u's full forest, device-grown trees included: a true XgbForest."""
        cont, own, _, _ = self._own[u]
        trees, info = self.grown_trees(u)
        if cont and not own.trees and not trees:
            return self.base
        head, hinfo = (list(self.base.trees), list(self.base.tree_info)) if cont else ([], [])
        return XgbForest(head + list(own.trees) + trees, hinfo + list(own.tree_info) + info, self.base.num_class,
                         self.base.base_score, self.base.objective, self.base.num_feature)

    def _host_rows(self):
        """(nodes, leaves, [(cont, row0, tgoff) per user], depth, the base's group offsets): the host-packed
        rows, put together once until the next ``set``."""
        if self._host is None:
            depth = self._check_depth(self._own)
            bn, bl, bgoff, _ = self.base.pack(depth)
            nodes, leaves, users = [bn], [bl], []
            row0 = len(self.base.trees)
            for cont, t, _, _ in self._own:
                tn, tl, tgoff, _ = t.pack(depth)
                nodes.append(tn)
                leaves.append(tl)
                users.append((cont, row0, tgoff))
                row0 += len(t.trees)
            self._host = (np.concatenate(nodes), np.concatenate(leaves), users, depth, bgoff)
        return self._host

    def _logical(self):
        """(tree_ids i32 [L], group_offsets i32 [U G + 1]): index arithmetic over per-user tree counts."""
        _, _, users, _, bgoff = self._host_rows()
        G = self.G
        base_ids = [np.arange(bgoff[g], bgoff[g + 1], dtype=np.int64) for g in range(G)]
        bases, row0 = [], users[-1][1] + len(self._own[-1][1].trees)
        for c in self._chunks:
            bases.append(row0)
            row0 += c.T
        ids, goff = [], [0]
        for u, (cont, urow0, tgoff) in enumerate(users):
            for g in range(G):
                n = 0
                if cont:
                    ids.append(base_ids[g])
                    n += len(base_ids[g])
                ids.append(urow0 + np.arange(tgoff[g], tgoff[g + 1], dtype=np.int64))
                n += int(tgoff[g + 1] - tgoff[g])
                for c, b in zip(self._chunks, bases):
                    if c.active[u]:
                        ids.append(c.ids(u, g, b))
                        n += c.rounds
                goff.append(goff[-1] + n)
        if row0 >= 1 << 24 or goff[-1] >= 1 << 31:
            raise ValueError(f"{row0} stored trees / {goff[-1]} logical trees: too many for the users form")
        return np.concatenate(ids).astype(np.int32), np.asarray(goff, dtype=np.int32), row0

    def arrays(self):
        """(nodes, leaves, tree_ids, group_offsets, depth); device-grown trees are read back."""
        if self._arrays is None:
            nodes, leaves, _, depth, _ = self._host_rows()
            ids, goff, _ = self._logical()
            if self._chunks:
                packed = [c.packed() for c in self._chunks]
                nodes = np.concatenate([nodes] + [p[0] for p in packed])
                leaves = np.concatenate([leaves] + [p[1] for p in packed])
            self._arrays = (nodes, leaves, ids, goff, depth)
        return self._arrays

    nodes = property(lambda self: self.arrays()[0])
    leaves = property(lambda self: self.arrays()[1])
    tree_ids = property(lambda self: self.arrays()[2])
    group_offsets = property(lambda self: self.arrays()[3])
    depth = property(lambda self: self._host_rows()[3])
    TT = property(lambda self: int(self._host_rows()[0].shape[0]) + sum(c.T for c in self._chunks))
    L = property(lambda self: int(self._logical()[0].shape[0]))

    @property
    def max_feature(self):
        """The highest feature a stored tree splits on (-1: none does)."""
        return max([self._base_feature, self._grown_feature] + [e[3] for e in self._own])

    def _lane_rows(self, nodes, leaves, T, depth, D, dev):
        """[2, T, 64, 2] lane tables of T packed trees on the device."""
        import torch

        from . import _lib
        from .ops import _p, _stream, call

        table = torch.zeros((2, max(T, 1), 64, 2), dtype=torch.int32, device=dev)
        if T:
            _lib.load()
            call("ce_xgb_lane_table", _p(nodes), _p(leaves), T, depth, int(D), _p(table), _stream(dev))
        return table

    def _device_state(self, device, D):
        import torch

        key = (torch.device(device), int(D))
        if key not in self._dev:
            dev = key[0]
            nodes, leaves, _, depth, _ = self._host_rows()
            ids, goff, TT = self._logical()
            T0 = int(nodes.shape[0])
            table = self._lane_rows(torch.from_numpy(nodes.view(np.int32)).to(dev), torch.from_numpy(leaves).to(dev), T0,
                                    depth, D, dev)
            if self._chunks:  # the grown trees' tables behind the host-packed ones, from their device arrays
                full = torch.zeros((2, TT, 64, 2), dtype=torch.int32, device=dev)
                full[:, :T0] = table[:, :T0]
                row0 = T0
                for c in self._chunks:
                    full[:, row0:row0 + c.T] = self._lane_rows(c.out["nodes"].to(dev), c.out["leaves"].to(dev), c.T,
                                                               depth, D, dev)
                    row0 += c.T
                table = full
            self._dev[key] = {"table": table, "used": TT, "ids": torch.from_numpy(ids).to(dev),
                              "goff": torch.from_numpy(goff).to(dev), "L": int(ids.shape[0])}
        return self._dev[key]

    def device(self, device, D):
        """(table i32 [2, capacity, 64, 2], tree_ids i32 [L], group_offsets i32 [U G + 1]) on ``device``."""
        s = self._device_state(device, D)
        return s["table"], s["ids"], s["goff"]

    def device_args(self, device, D):
        """(table, its capacity in trees, tree_ids, L, group_offsets, depth): what the
        users entry points take, from host numbers alone (nothing is read back)."""
        s = self._device_state(device, D)
        return s["table"], int(s["table"].shape[1]), s["ids"], s["L"], s["goff"], self.depth

    def attach(self, chunk, max_feature):
        """The host half of ``grow``: the chunk's trees join their users' forests
        (counts and index arithmetic only; device tables not built by ``grow``
        are built from the chunk's arrays on their next use)."""
        if chunk.U != self.U or chunk.G != self.G or chunk.depth != self.depth:
            raise ValueError("the grown trees do not fit this stack (users, groups or depth)")
        self._chunks.append(chunk)
        self._grown_feature = max(self._grown_feature, int(max_feature))
        self._arrays = None

    def grow(self, chunk, device, D, max_feature):
        """Append one fit call's trees (a GrownTrees on ``device``): their lane
        tables go straight behind the existing ones (the table doubles when
        full), tree_ids and group_offsets are rebuilt from the tree counts and
        uploaded again.  Other (device, D) tables are dropped and rebuilt on
        their next use."""
        import torch

        if not chunk.active.any():
            return
        key = (torch.device(device), int(D))
        s = self._device_state(device, D)
        self._dev = {key: s}
        table, used = s["table"], s["used"]
        if used + chunk.T > table.shape[1]:
            grown = torch.zeros((2, max(2 * table.shape[1], used + chunk.T), 64, 2), dtype=torch.int32, device=key[0])
            grown[:, :used] = table[:, :used]
            table = grown
        table[:, used:used + chunk.T] = self._lane_rows(chunk.out["nodes"], chunk.out["leaves"], chunk.T, self.depth, D,
                                                         key[0])
        self.attach(chunk, max_feature)
        ids, goff, TT = self._logical()
        s.update(table=table, used=TT, ids=torch.from_numpy(ids).to(key[0]), goff=torch.from_numpy(goff).to(key[0]),
                 L=int(ids.shape[0]))


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
