"""Batched sessions on the GPU: every user's mc, hc or mix epoch in one launch.

ce_select_batched_excl, ce_select_batched_mix (k_select_tiles_mix),
ce_mark_selected_batched and ce_amd.BatchedSelectionSession against the CPU
oracle on each user's alive subset: positions bit-equal, values 0 ulp."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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


def bitmap(mask):
    """bool [n] -> the engine's bitmap (int32 words on the device, bit i of word i / 32)."""
    n = len(mask)
    bits = np.zeros(max((n + 31) // 32, 1) * 32, np.uint8)
    bits[:n] = mask
    return torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32).copy()).cuda()


def unbitmap(t, n):
    return np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)


def tie_committee(rng, N, M=4, C=4):
    """[M, N, C] f64 probabilities quantised to 1/8 (+ 1e-3): entropy ties everywhere."""
    e = -np.log(rng.random((M, N, C)))
    return np.floor(e / e.sum(-1, keepdims=True) * 8) / 8 + 1e-3


def tie_table(rng, n):
    hc = np.round(rng.dirichlet(np.ones(4), n), 1).reshape(n, 4)  # few distinct rows
    hc[::5] = 0.25                                                 # the maximal entropy, many times
    return hc


def pad(vals, idx, q):
    v = np.full(q, np.nan)
    i = np.full(q, -1, np.int64)
    v[:len(vals)] = vals
    i[:len(idx)] = idx
    return v, i


def assert_same(got_v, got_i, exp_v, exp_i, what):
    got_v, got_i = got_v.cpu().numpy(), got_i.cpu().numpy()
    assert np.array_equal(got_i, exp_i), (what, np.argwhere(got_i != exp_i)[:5], got_i[got_i != exp_i][:5],
                                          exp_i[got_i != exp_i][:5])
    nan = np.isnan(exp_v)
    assert np.array_equal(np.isnan(got_v), nan), what
    assert np.array_equal(got_v[~nan].view(np.int64), exp_v[~nan].view(np.int64)), what  # 0 ulp


# ---------------------------------------------------------------------------
# batched mc with exclusions
# ---------------------------------------------------------------------------
MC_SIZES = [0, 1, 31, 33, 64, 65, 700, 2048, 2100]  # offsets off multiples of 32; the tile's 2048; the long path
MC_QS = [1, 10, 64, 65, 2049]


@pytest.fixture(scope="module")
def mc_case():
    from oracle import ce_oracle as O

    rng = np.random.default_rng(345)
    off = np.concatenate([[0], np.cumsum(MC_SIZES)]).astype(np.int64)
    total = int(off[-1])
    P64 = tie_committee(rng, total)                                    # the reference's f64 [M, N, C]
    P32 = np.ascontiguousarray(P64.transpose(1, 0, 2)).astype(np.float32)  # f32 [N, M, C]
    mask = rng.random(total) < 0.3
    mask[off[4]:off[5]] = True                  # the 64-item user: fully excluded
    mask[off[6]:off[7]] = True                  # the 700-item user: 5 alive, fewer than q = 10
    for b in off[1:-1]:                         # the bits on either side of every user boundary
        mask[max(b - 1, 0)] = True
        mask[min(b, total - 1)] = True
    mask[off[6] + np.array([3, 64, 65, 350, 698])] = False
    inputs = {"f32_NMC": (P32, "NMC"), "f64_MNC": (P64, "MNC")}
    exp = {}
    for name, (P, lay) in inputs.items():
        for masked in (False, True):
            ents = O.oracle_committee_entropy(P, lay)
            for q in MC_QS:
                ev, ei = np.empty((len(MC_SIZES), q)), np.empty((len(MC_SIZES), q), np.int64)
                for u in range(len(MC_SIZES)):
                    alive = np.flatnonzero(~mask[off[u]:off[u + 1]]) if masked else np.arange(MC_SIZES[u])
                    v, i = O.oracle_topq(ents[off[u] + alive], q) if len(alive) else (np.zeros(0), np.zeros(0, np.int64))
                    ev[u], ei[u] = pad(v, alive[i], q)
                exp[name, masked, q] = (ev, ei)
    return off, mask, inputs, exp


def test_oracle_per_item_entropy_is_subset_invariant(mc_case):
    """The expectation above takes each user's entropies from one oracle pass
    over the whole tensor; the oracle scores items independently, so that is
    oracle_select_mc on the user's alive subset (checked on one user)."""
    from oracle import ce_oracle as O

    off, mask, inputs, exp = mc_case
    P, _ = inputs["f64_MNC"]
    u = 8
    alive = np.flatnonzero(~mask[off[u]:off[u + 1]])
    v, i = O.oracle_select_mc(np.ascontiguousarray(P[:, off[u] + alive]), 64, "MNC")
    ev, ei = exp["f64_MNC", True, 64]
    assert np.array_equal(alive[i], ei[u]) and np.array_equal(v.view(np.int64), ev[u].view(np.int64))


@pytest.mark.parametrize("q", MC_QS)
@pytest.mark.parametrize("name", ["f32_NMC", "f64_MNC"])
def test_batched_mc_with_exclusions(ce, mc_case, name, q):
    off, mask, inputs, exp = mc_case
    P, lay = inputs[name]
    Pd, offd = dev(P), dev(off)
    v, i = ce.ops.select_batched(Pd, offd, q, lay, excl=bitmap(mask))
    assert_same(v, i, *exp[name, True, q], (name, q, "excl"))
    # an all-clear bitmap and excl=None are ce_select_batched
    v0, i0 = ce.ops.select_batched(Pd, offd, q, lay)
    assert_same(v0, i0, *exp[name, False, q], (name, q, "plain"))
    kernel = ce._lib.load().ce_last_kernel()
    vz, iz = ce.ops.select_batched(Pd, offd, q, lay, excl=bitmap(np.zeros(len(mask), bool)))
    assert ce._lib.load().ce_last_kernel() == kernel
    assert torch.equal(iz, i0) and torch.equal(vz.view(torch.int64), v0.view(torch.int64))
    # the entry point itself with excl == NULL: ce_select_batched, kernel and all
    ops, lib = ce.ops, ce._lib.load()
    comm, U = ops._committee_args(Pd, lay), len(MC_SIZES)
    ws = ops.new_workspace(lib.ce_select_batched_workspace_bytes(comm[2], U, q), Pd.device)
    vn, idn = ops._outs(q, Pd.device, (U,))
    ce._lib.call("ce_select_batched_excl", *comm, ops._p(offd), U, None, q, ops._p(ws), ws.numel(), ops._p(vn),
                 ops._p(idn), ops._stream(Pd.device))
    assert lib.ce_last_kernel() == kernel
    assert torch.equal(idn, i0) and torch.equal(vn.view(torch.int64), v0.view(torch.int64))


def test_mark_selected_batched(ce):
    """Every branch of the mark: committee picks, hc picks, the twins through
    both maps, padding and out-of-range slots, words shared by two users."""
    off = np.array([0, 5, 45, 45, 70])          # user 2 is empty
    off_h = np.array([0, 40, 43, 50, 50])       # user 3 has no table
    idx = np.full((4, 6), -1, np.int64)
    idx[0, :4] = [0, 4, 5 + 39, 5 + 40]         # items 0, 4; row 39; 5 + 40 is past the 40 rows: ignored
    idx[1, :3] = [39, 40 + 2, 40 + 3]           # item 39; row 2 of 3; row 3: ignored
    idx[2, :2] = [0, 6]                         # no items: rows 0 and 6 of 7
    idx[3, :3] = [24, 25, 3]                    # items 24, 3; 25 is past the items and the user has no rows
    m2h = np.full(70, -1, np.int64)
    h2m = np.full(50, -1, np.int64)
    m2h[4], h2m[10] = 10, 4                      # user 0: item 4 <-> row 10
    m2h[1], h2m[39] = 39, 1                      # user 0: item 1 <-> row 39
    m2h[5 + 39], h2m[40 + 1] = 41, 44            # user 1: item 39 <-> row 1
    ex, exh = ce.ops.excl_bitmap(70, "cuda"), ce.ops.excl_bitmap(50, "cuda")
    ce.ops.mark_selected_batched(dev(idx), dev(off), ex, dev(off_h), exh, dev(m2h), dev(h2m))
    assert np.flatnonzero(unbitmap(ex, 70)).tolist() == [0, 1, 4, 44, 45 + 3, 45 + 24]
    assert np.flatnonzero(unbitmap(exh, 50)).tolist() == [10, 39, 41, 42, 43, 49]
    # the committee side alone (mc / hc sessions): hc-range slots are ignored
    ex2 = ce.ops.excl_bitmap(70, "cuda")
    ce.ops.mark_selected_batched(dev(idx), dev(off), ex2)
    assert np.flatnonzero(unbitmap(ex2, 70)).tolist() == [0, 4, 44, 45 + 3, 45 + 24]


# ---------------------------------------------------------------------------
# batched mix
# ---------------------------------------------------------------------------
MIX_SIZES = [(0, 0), (0, 5), (5, 0), (1, 1), (300, 1608), (1608, 1300), (2048, 2048), (2049, 10), (10, 2049)]
MIX_QS = [1, 10, 64]


def mix_stacks(sizes, off, off_h, ent, ent_h, mask, mask_h, masked):
    """Per user, the alive rows of [mc_u; hc_u]: their oracle entropies and their user-local positions."""
    out = []
    for u, (n, nh) in enumerate(sizes):
        pos = np.flatnonzero(~mask[off[u]:off[u + 1]]) if masked else np.arange(n)
        hpos = np.flatnonzero(~mask_h[off_h[u]:off_h[u + 1]]) if masked else np.arange(nh)
        out.append((np.concatenate([ent[off[u] + pos], ent_h[off_h[u] + hpos]]),
                    np.concatenate([pos, n + hpos]).astype(np.int64)))
    return out


def mix_expected(stacks, q):
    """The oracle's top q of every user's stack, padded: values [U, q], positions [U, q]."""
    from oracle import ce_oracle as O

    ev, ei = np.empty((len(stacks), q)), np.empty((len(stacks), q), np.int64)
    for u, (stack, where) in enumerate(stacks):
        v, i = O.oracle_topq(stack, q) if len(stack) else (np.zeros(0), np.zeros(0, np.int64))
        ev[u], ei[u] = pad(v, where[i], q)
    return ev, ei


@pytest.fixture(scope="module")
def mix_case():
    from oracle import ce_oracle as O

    rng = np.random.default_rng(473)
    off = np.concatenate([[0], np.cumsum([a for a, _ in MIX_SIZES])]).astype(np.int64)
    off_h = np.concatenate([[0], np.cumsum([b for _, b in MIX_SIZES])]).astype(np.int64)
    total, total_h = int(off[-1]), int(off_h[-1])
    P64 = tie_committee(rng, total)
    hc = tie_table(rng, total_h)
    twin = off[4] + 7          # user 4: committee item 7 IS the uniform row, as every 5th row of the tables is:
    P64[:, twin] = 0.25        # an exact tie across the segments, the committee position must win
    nan_item = off[5] + 100    # user 5: an all-zero consensus row: entropy NaN, first in the order
    P64[:, nan_item] = 0.0
    P32 = np.ascontiguousarray(P64.transpose(1, 0, 2)).astype(np.float32)
    mask, mask_h = rng.random(total) < 0.3, rng.random(total_h) < 0.3
    mask[[twin, nan_item]] = False
    mask_h[off_h[4]:off_h[4] + 11] = False
    inputs = {"f32_NMC": (P32, "NMC"), "f64_MNC": (P64, "MNC")}
    ent_h = O.oracle_table_entropy(hc)
    exp = {}
    for name, (P, lay) in inputs.items():
        ent = O.oracle_committee_entropy(P, lay)
        for masked in (False, True):
            stacks = mix_stacks(MIX_SIZES, off, off_h, ent, ent_h, mask, mask_h, masked)
            for q in MIX_QS:
                exp[name, masked, q] = mix_expected(stacks, q)
    first_uniform = int(-off_h[4] % 5)  # user 4's first uniform hc row (hc[::5] counts stacked rows)
    return off, off_h, hc, mask, mask_h, inputs, exp, (twin - off[4], 300 + first_uniform, nan_item - off[5])


@pytest.mark.parametrize("q", MIX_QS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", ["f32_NMC", "f64_MNC"])
def test_batched_mix(ce, mix_case, name, masked, q):
    off, off_h, hc, mask, mask_h, inputs, exp, (twin, hc_twin, nan_item) = mix_case
    P, lay = inputs[name]
    v, i = ce.ops.select_batched_mix(dev(P), dev(off), dev(hc), dev(off_h), q, lay,
                                     excl=bitmap(mask) if masked else None, excl_h=bitmap(mask_h) if masked else None)
    assert ce._lib.load().ce_last_kernel().startswith(b"ce::k_select_tiles_mix<")
    ev, ei = exp[name, masked, q]
    assert_same(v, i, ev, ei, (name, masked, q))
    # what the inputs were built to show: the committee's uniform item before the table's; NaN first
    if q >= 10:
        row = ei[4].tolist()
        a, b = row.index(twin), row.index(hc_twin)  # the committee item and an hc row: one entropy, bit for bit
        assert a < b and ev[4, a].view(np.int64) == ev[4, b].view(np.int64)
    assert ei[5, 0] == nan_item and np.isnan(ev[5, 0])


# every row uniform: more survivors than a block's LDS holds (1024 at most), the overflow branch of the tile
FLOOD_SIZES = [(1100, 1100), (0, 1100), (1100, 0)]  # under the 2048-slot tile: not the streaming path


@pytest.fixture(scope="module")
def flood_case():
    from oracle import ce_oracle as O

    off = np.concatenate([[0], np.cumsum([a for a, _ in FLOOD_SIZES])]).astype(np.int64)
    off_h = np.concatenate([[0], np.cumsum([b for _, b in FLOOD_SIZES])]).astype(np.int64)
    P64 = np.full((4, int(off[-1]), 4), 0.25)
    hc = np.full((int(off_h[-1]), 4), 0.25)
    P64[:, 7] = [0.7, 0.1, 0.1, 0.1]   # user 0: one item and one hc row below the flood
    hc[3] = [1.0, 0.0, 0.0, 0.0]
    P32 = np.ascontiguousarray(P64.transpose(1, 0, 2)).astype(np.float32)
    mask, mask_h = np.zeros(int(off[-1]), bool), np.zeros(int(off_h[-1]), bool)
    mask[[0, 1]] = True                # user 0's first items and first hc row: the order starts later
    mask_h[0] = True
    inputs = {"f32_NMC": (P32, "NMC"), "f64_MNC": (P64, "MNC")}
    ent_h = O.oracle_table_entropy(hc)
    stacks = {(name, masked): mix_stacks(FLOOD_SIZES, off, off_h, O.oracle_committee_entropy(P, lay), ent_h, mask,
                                         mask_h, masked)
              for name, (P, lay) in inputs.items() for masked in (False, True)}
    exp = {(name, masked, q): mix_expected(s, q) for (name, masked), s in stacks.items() for q in MIX_QS}
    return off, off_h, hc, mask, mask_h, inputs, stacks, exp


@pytest.mark.parametrize("q", MIX_QS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", ["f32_NMC", "f64_MNC"])
def test_batched_mix_overflow(ce, flood_case, name, masked, q):
    """More than CAP = 1024 rows of a block at the floor: exact keys of every
    slot and the tree merge, positions over both segments."""
    off, off_h, hc, mask, mask_h, inputs, stacks, exp = flood_case
    # what the case rests on: in every non-empty user, more than 1024 alive rows carry the maximal entropy
    for (n, nh), (stack, _) in zip(FLOOD_SIZES, stacks[name, masked]):
        assert n + nh > 0 and int((stack == stack.max()).sum()) > 1024
    P, lay = inputs[name]
    v, i = ce.ops.select_batched_mix(dev(P), dev(off), dev(hc), dev(off_h), q, lay,
                                     excl=bitmap(mask) if masked else None, excl_h=bitmap(mask_h) if masked else None)
    assert ce._lib.load().ce_last_kernel().startswith(b"ce::k_select_tiles_mix<")
    ev, ei = exp[name, masked, q]
    assert_same(v, i, ev, ei, (name, masked, q))
    if not masked:  # user 0: positions in order, the one item below the flood left out
        assert ei[0].tolist() == [p for p in range(q + 1) if p != 7][:q]


# ---------------------------------------------------------------------------
# BatchedSelectionSession
# ---------------------------------------------------------------------------
SESS_SIZES = [15, 40, 333, 900, 1608, 1700]
EPOCHS, Q = 5, 10


@pytest.fixture(scope="module")
def sess_case():
    rng = np.random.default_rng(396)
    off = np.concatenate([[0], np.cumsum(SESS_SIZES)]).astype(np.int64)
    committees = [tie_committee(rng, int(off[-1])) for _ in range(EPOCHS)]
    hc_same = tie_table(rng, int(off[-1]))                     # hc mode, and nothing else
    # mix: a partial table per user in its OWN row order (a permuted, partial hc_to_mc)
    n_rows = [int(0.8 * n) for n in SESS_SIZES]
    off_h = np.concatenate([[0], np.cumsum(n_rows)]).astype(np.int64)
    h2m = np.concatenate([rng.permutation(n)[:nh] for n, nh in zip(SESS_SIZES, n_rows)]).astype(np.int64)
    hc = tie_table(rng, int(off_h[-1]))
    # user 2, epoch 0: the song of its first uniform hc row has a uniform committee too -- it is picked
    # through BOTH segments in one epoch (the duplicate the mark and `remaining` must absorb)
    committees[0][:, off[2] + h2m[off_h[2] + (-off_h[2] % 5)]] = 0.25
    return off, committees, hc_same, off_h, h2m, hc


def shrinking_reference(mode, epochs, q, committees, hc):
    """The reference's epoch loop on the host for one user: pools shrink by the
    picks (amg_test.py:455, :484, :521-531), every epoch selects on what is left."""
    from oracle import ce_oracle as O

    N = committees[0].shape[1] if mode == "mc" else hc.shape[0]
    alive = np.ones(N, bool)
    out = []
    for e in range(epochs):
        pos = np.flatnonzero(alive)
        if len(pos) == 0:
            out.append(np.zeros(0, np.int64))
            continue
        if mode == "mc":
            _, i = O.oracle_select_mc(np.ascontiguousarray(committees[e][:, pos]), q, "MNC")
        else:
            _, i = O.oracle_topq(O.oracle_table_entropy(hc[pos]), q)
        alive[pos[i]] = False
        out.append(np.asarray(pos[i], np.int64))
    return out


def shrinking_mix_reference(epochs, q, committees, hc, h2m):
    """The same for the mix with the table in its own row order: a pick through
    either segment drops the song from both pools.  Returns the picks per
    epoch, the committee pool left, and the songs picked through both segments
    in one epoch."""
    from oracle import ce_oracle as O

    N, Nh = committees[0].shape[1], hc.shape[0]
    m2h = np.full(N, -1)
    m2h[h2m[h2m >= 0]] = np.flatnonzero(h2m >= 0)
    alive, alive_h = np.ones(N, bool), np.ones(Nh, bool)
    out, twice = [], 0
    for e in range(epochs):
        pos, hpos = np.flatnonzero(alive), np.flatnonzero(alive_h)
        ent = np.concatenate([O.oracle_committee_entropy(np.ascontiguousarray(committees[e][:, pos]), "MNC")
                              if len(pos) else np.zeros(0),
                              O.oracle_table_entropy(hc[hpos]) if len(hpos) else np.zeros(0)])
        _, i = O.oracle_topq(ent, q) if len(ent) else (None, np.zeros(0, np.int64))
        picks = np.concatenate([pos, N + hpos])[i].astype(np.int64)
        songs = [p if p < N else h2m[p - N] for p in picks]
        twice += len(songs) - len(set(songs))
        for p in picks:
            if p < N:
                alive[p] = False
                if m2h[p] >= 0:
                    alive_h[m2h[p]] = False
            else:
                alive_h[p - N] = False
                if h2m[p - N] >= 0:
                    alive[h2m[p - N]] = False
        out.append(picks)
    return out, int(alive.sum()), twice


@pytest.mark.parametrize("mode", ["mc", "hc"])
def test_batched_session_mc_hc(ce, sess_case, mode):
    off, committees, hc_same, _, _, _ = sess_case
    U = len(SESS_SIZES)
    exp = [shrinking_reference(mode, EPOCHS, Q, [c[:, off[u]:off[u + 1]] for c in committees],
                               hc_same[off[u]:off[u + 1]]) for u in range(U)]
    sess = ce.BatchedSelectionSession(Q, mode, off, hc=hc_same if mode == "hc" else None)
    singles = [ce.SelectionSession(Q, mode, SESS_SIZES[u], hc=hc_same[off[u]:off[u + 1]] if mode == "hc" else None)
               for u in range(U)]
    for e in range(EPOCHS):
        got = sess.select(committee=dev(committees[e]) if mode == "mc" else None)
        assert len(got) == U
        for u in range(U):
            assert got[u].dtype == np.int64 and np.array_equal(got[u], exp[u][e]), (mode, e, u, got[u], exp[u][e])
            one = singles[u].select(committee=dev(committees[e][:, off[u]:off[u + 1]]) if mode == "mc" else None)
            assert np.array_equal(got[u], one), (mode, e, u)
    assert [len(x) for x in exp[0]] == [10, 5, 0, 0, 0]  # the 15-song user runs dry
    assert sess.remaining.shape == (U,)
    assert sess.remaining.tolist() == [n - sum(len(x) for x in exp[u]) for u, n in enumerate(SESS_SIZES)]
    assert sess.remaining.tolist() == [s.remaining for s in singles]


def _mix_session(ce, sess_case, q):
    off, _, _, off_h, h2m, hc = sess_case
    return ce.BatchedSelectionSession(q, "mix", off, hc=hc, hc_offsets=off_h, hc_to_mc=h2m)


def _mix_expected(sess_case, q, epochs):
    off, committees, _, off_h, h2m, hc = sess_case
    return [shrinking_mix_reference(epochs, q, [c[:, off[u]:off[u + 1]] for c in committees],
                                    hc[off_h[u]:off_h[u + 1]], h2m[off_h[u]:off_h[u + 1]])
            for u in range(len(SESS_SIZES))]


def test_batched_session_mix(ce, sess_case):
    off, committees, _, off_h, h2m, hc = sess_case
    U = len(SESS_SIZES)
    exp = _mix_expected(sess_case, Q, EPOCHS)
    sess = _mix_session(ce, sess_case, Q)
    singles = [ce.SelectionSession(Q, "mix", SESS_SIZES[u], hc=hc[off_h[u]:off_h[u + 1]],
                                   hc_to_mc=h2m[off_h[u]:off_h[u + 1]]) for u in range(U)]
    for e in range(EPOCHS):
        got = sess.select(committee=dev(committees[e]))
        assert ce._lib.load().ce_last_kernel().startswith(b"ce::k_select_tiles_mix<")
        for u in range(U):
            assert np.array_equal(got[u], exp[u][0][e]), (e, u, got[u], exp[u][0][e])
            one = singles[u].select(committee=dev(committees[e][:, off[u]:off[u + 1]]))
            assert np.array_equal(got[u], one), (e, u)
    assert sess.remaining.tolist() == [x[1] for x in exp]
    assert sess.remaining.tolist() == [s.remaining for s in singles]
    assert sum(int((p >= SESS_SIZES[u]).sum()) for u in range(U) for p in exp[u][0]) > 0  # the hc segment took part
    assert sum(x[2] for x in exp) >= 1  # a song picked through both segments in one epoch


@pytest.mark.parametrize("q", [10, 64])
def test_mix_composed_path_equals_kernel_path(ce, sess_case, q):
    _, committees, _, _, _, _ = sess_case
    a, b = _mix_session(ce, sess_case, q), _mix_session(ce, sess_case, q)
    for e in range(3):
        Pd = dev(committees[e])
        ka = a.select(committee=Pd)
        kb = b.select(committee=Pd, _compose=True)
        assert all(np.array_equal(x, y) for x, y in zip(ka, kb)), (q, e)
    assert a.remaining.tolist() == b.remaining.tolist()


def test_mix_q65_runs_composed_and_equals_oracle(ce, sess_case):
    _, committees, _, _, _, _ = sess_case
    exp = _mix_expected(sess_case, 65, 2)
    sess = _mix_session(ce, sess_case, 65)
    for e in range(2):
        got = sess.select(committee=dev(committees[e]))
        for u in range(len(SESS_SIZES)):
            assert np.array_equal(got[u], exp[u][0][e]), (e, u)
    assert sess.remaining.tolist() == [x[1] for x in exp]


def _graph_counts(g):
    """(nodes, edges) of a kept captured graph."""
    import ce_amd

    lib = ce_amd._lib.load()
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    f = lib.hipGraphGetNodes
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    assert f(ctypes.c_void_p(g.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    f = lib.hipGraphGetEdges
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    assert f(ctypes.c_void_p(g.raw_cuda_graph()), None, None, ctypes.byref(m)) == 0
    return n.value, m.value


def test_mix_epoch_in_a_hip_graph(ce, sess_case):
    """One mix epoch (select + mark) captured once and replayed per epoch,
    the next committee written into the captured tensor in place: the picks
    are the eager session's.  The workspace comes from the pre-zeroed arena."""
    off, committees, _, off_h, _, _ = sess_case
    ops = ce.ops
    eager, graphed = _mix_session(ce, sess_case, Q), _mix_session(ce, sess_case, Q)
    Pd = dev(committees[0])
    ops.select_mc(Pd, Q, "MNC")  # an eager call first: it creates the device's graph arena
    ops.reserve_graph_workspace(ce._lib.load().ce_select_batched_mix_workspace_bytes(
        int(off[-1]), int(off_h[-1]), len(SESS_SIZES), Q))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the fallback (a captured zero fill) warns
        with torch.cuda.graph(g):
            idx = graphed.step(Pd)
    g.instantiate()
    assert _graph_counts(g) == (2, 1)  # select -> mark: linear, no parallel branches
    for e in range(4):
        Pd.copy_(dev(committees[e]))
        g.replay()
        torch.cuda.synchronize()
        got = graphed.account(idx)
        exp = eager.select(committee=dev(committees[e]))
        assert all(np.array_equal(x, y) for x, y in zip(got, exp)), e
        assert any(len(x) for x in got)
    assert graphed.remaining.tolist() == eager.remaining.tolist()
