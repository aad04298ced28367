"""GPU parity of ce_xgb_fit_users with the restatement (tests/xgb_fit_ref.py) at
the kernel's own limits, R.EDGE_CASES: batches of 7 .. 9, 63 .. 65, 255 .. 257
and 513 rows, the 4096-row cap, 63-node trees, D = 64 / 65 / 257 / 512 (one
wave, two, the first shape above 64 KiB of LDS, the largest LDS the entry
accepts), 8 groups, eta / lambda / min_child_weight away from their defaults,
300 users, a row stride above D, denormals, signed zeros, doubles that collide
or overflow as floats, a row listed twice, candidates of infinite loss_chg
(lambda = 0 on hessians that cancel), and the status = 2 guard.  The
standard is test_gpu_xgb_fit.py's: 0 differing bits in the node arrays, the
packed arrays and the margins.  tests/test_xgb_fit.py asserts on the
restatement alone that these inputs reach what they are here for."""
import numpy as np
import pytest

import xgb_fit_ref as R
from ce_amd.xgb import StackedForests
from test_gpu_xgb_fit import NAMES, assert_outputs, dev, same_forest
from xgb_users_ref import bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


def device_X(c):
    """X on the device; with ``pad``, the [:, :D] view of a wider buffer whose other columns are NaN."""
    X = c["X"] if c["f64"] else c["X"].astype(np.float32)
    if not c["pad"]:
        return dev(X)
    buf = np.full((X.shape[0], c["D"] + c["pad"]), np.nan, X.dtype)
    buf[:, :c["D"]] = X
    view = dev(buf)[:, :c["D"]]
    assert view.stride(0) == c["D"] + c["pad"] and view.stride(1) == 1
    return view


def fit_case(ce, c, users=None):
    """One ops.xgb_fit_users call on the case (all users, or only ``users`` with the others' batches empty)."""
    st = StackedForests(c["base"], [None] * c["U"])
    off = c["row_offsets"].copy()
    rows, labels = c["rows"], c["labels"]
    if users is not None:
        keep = np.concatenate([np.arange(off[u], off[u + 1]) for u in users])
        counts = np.array([off[u + 1] - off[u] if u in users else 0 for u in range(c["U"])])
        rows, labels, off = rows[keep], labels[keep], np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    got = ce.ops.xgb_fit_users(device_X(c), dev(rows), dev(labels), st, dev(off), c["rounds"], c["max_depth"],
                               eta=c["eta"], reg_lambda=c["lam"], min_child_weight=c["mcw"], return_margins=True)
    return st, got, off


@pytest.mark.parametrize("name", list(R.EDGE_CASES))
def test_edge_parity(ce, name):
    """Every user of the case in one call (n_max is the largest batch, so most
    users run with LDS sized for another's rows): trees in both forms and the
    final margins bit for bit, the flags, forest(u)."""
    c = R.case(name)
    st, got, _ = fit_case(ce, c)
    assert st.depth == c["max_depth"]  # a leaves-only base: packed at the fit's depth, no entry idle below it
    exp = R.expected_outputs(c["per_user"], c["U"], c["rounds"], c["C"], st.depth)
    assert got["status"].cpu().numpy().tolist() == c["status"]
    assert got["active"].tolist() == [n > 0 and s == 0 for n, s in zip(c["counts"], c["status"])]
    assert_outputs(got, exp, name)
    assert np.array_equal(bits(got["margins"].cpu().numpy()), bits(c["margins"])), name
    for u in range(c["U"]):
        assert same_forest(st.forest(u), c["forests"][u]), (name, u)


def test_many_users_equal_their_own_calls(ce):
    """300 blocks in one launch: a user from the start, the middle and the end equals its one-user call."""
    c = R.case("many")
    _, all_u, _ = fit_case(ce, c)
    per = c["rounds"] * c["C"]
    for u in (5, 150, 298):
        assert c["counts"][u] > 0
        _, one, off = fit_case(ce, c, users=[u])
        for k in NAMES + ("cond", "nodes", "leaves"):
            a = all_u["trees"].out[k].cpu().numpy()[u * per:(u + 1) * per]
            b = one["trees"].out[k].cpu().numpy()[u * per:(u + 1) * per]
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (u, k)
        a0, a1 = c["row_offsets"][u], c["row_offsets"][u + 1]
        assert np.array_equal(bits(one["margins"].cpu().numpy()[off[u]:off[u + 1]]),
                              bits(all_u["margins"].cpu().numpy()[a0:a1]))


def test_understated_n_max_flags_that_user_alone(ce):
    """The entry point itself, with the wrapper's buffers and n_max = 64 for
    batches of 63, 64 and 65 rows: the third user is flagged 2 and its slots and
    margins stay as allocated; the other two are the plain call's, bit for bit."""
    from ce_amd._lib import call, load

    c = R.case("rows64")
    assert c["counts"] == (63, 64, 65)
    U, C, D, rounds, n_max = c["U"], c["C"], c["D"], c["rounds"], 64
    ops, p = ce.ops, ce.ops._p
    st = StackedForests(c["base"], [None] * U)
    st.ensure_depth(c["max_depth"])
    X, rows, labels, off = device_X(c), dev(c["rows"]), dev(c["labels"]), dev(c["row_offsets"])
    table, cap, ids, L, goff, depth = st.device_args(X.device, D)
    n_rows, T = int(c["row_offsets"][-1]), U * rounds * C
    NI, NL = max((1 << depth) - 1, 1), 1 << depth
    kw = dict(device="cuda")
    t = {"nodes": torch.zeros((T, NI, 2), dtype=torch.int32, **kw), "leaves": torch.zeros((T, NL), dtype=torch.float32, **kw),
         "left": torch.full((T, R.MAX_NODES), -1, dtype=torch.int32, **kw),
         "right": torch.full((T, R.MAX_NODES), -1, dtype=torch.int32, **kw),
         "split": torch.zeros((T, R.MAX_NODES), dtype=torch.int32, **kw),
         "cond": torch.zeros((T, R.MAX_NODES), dtype=torch.float32, **kw),
         "default_left": torch.zeros((T, R.MAX_NODES), dtype=torch.uint8, **kw),
         "num_nodes": torch.zeros(T, dtype=torch.int32, **kw)}
    margins = torch.zeros((n_rows, C), dtype=torch.float32, **kw)
    flags = torch.zeros(U, dtype=torch.int32, **kw)
    ws_bytes = int(load().ce_xgb_fit_workspace_bytes(n_rows, n_max, D, C, rounds))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, **kw)
    call("ce_xgb_fit_users", p(X), ops._DT[X.dtype], X.shape[0], D, X.stride(0), p(rows), p(labels), p(off), U, n_rows, n_max,
         p(table), cap, p(ids), L, p(goff), C, depth, float(st.base_margin), rounds, c["max_depth"], c["eta"], c["lam"],
         c["mcw"], p(t["nodes"]), p(t["leaves"]), p(t["left"]), p(t["right"]), p(t["split"]), p(t["cond"]),
         p(t["default_left"]), p(t["num_nodes"]), p(margins), p(flags), p(ws), ws_bytes, ops._stream(X.device))
    assert flags.cpu().numpy().tolist() == [0, 0, 2]
    # the restatement with user 2 left out is both expectations at once: allocated values there, the plain call's elsewhere
    exp = R.expected_outputs(c["per_user"][:2] + [[]], U, rounds, C, depth)
    assert_outputs({"trees": type("Out", (), {"out": t})}, exp, "n_max 64")
    em = c["margins"].copy()
    em[c["row_offsets"][2]:] = 0
    assert np.array_equal(bits(margins.cpu().numpy()), bits(em))
    _, plain, _ = fit_case(ce, c)
    per = rounds * C
    for k in NAMES + ("cond", "nodes", "leaves"):
        a, b = t[k].cpu().numpy()[:2 * per], plain["trees"].out[k].cpu().numpy()[:2 * per]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
