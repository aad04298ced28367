"""Pin the CPU oracle's hc tables (oracle_vote_table, oracle_va_table,
oracle_table_entropy) against the reference's own expressions on the inputs
that tests/test_gpu_hc_tables.py feeds the HIP kernels, so that a mismatch there
is the kernel's fault and not the oracle's; and what the two table entry
points answer on the host, before any launch.

Bar: bit for bit.  f64 results are compared as uint64 views (so -0.0 is not
+0.0); a NaN equals any NaN (the rows without a valid vote are 0/0).
"""
import numpy as np
import pytest

from oracle import ce_oracle as O

LATTICE_N = list(range(1, 257)) + [500, 665, 1000, 2000]
LATTICE_A = 2000


def same_bits(got, exp):
    """Equal bit for bit, NaN equal to any NaN, -0.0 different from +0.0."""
    got = np.ascontiguousarray(got, np.float64)
    exp = np.ascontiguousarray(exp, np.float64)
    if got.shape != exp.shape:
        return False
    nan_g, nan_e = np.isnan(got), np.isnan(exp)
    return bool(np.array_equal(nan_g, nan_e) and np.array_equal(got.view(np.uint64)[~nan_e], exp.view(np.uint64)[~nan_e]))


def count_lattice():
    """Every (c, n), 0 <= c <= n, n in LATTICE_N, as C = 2 vote rows: c votes of
    class 0, n - c of class 1, then -1 up to A = 2000.  Returns (votes, c, n)."""
    n = np.concatenate([np.full(k + 1, k) for k in LATTICE_N])
    c = np.concatenate([np.arange(k + 1) for k in LATTICE_N])
    col = np.arange(LATTICE_A)[None, :]
    votes = np.where(col < c[:, None], np.int8(0), np.where(col < n[:, None], np.int8(1), np.int8(-1)))
    return votes, c, n


def exact_halves(c, n):
    """Rows where np.round(x, 3) rounds an exact tie: x * 1000 ends in .5."""
    t0, t1 = c / n * 1000.0, (n - c) / n * 1000.0
    return (t0 - np.floor(t0) == 0.5) | (t1 - np.floor(t1) == 0.5)


def test_count_lattice_is_numpy_round_and_scipy_entropy():
    """round3 over the whole (count, n) lattice: the oracle's frequencies are
    np.round(c / n, 3) and np.round((n - c) / n, 3) computed directly, its
    entropies scipy.stats.entropy of them (amg_test.py:115, :451).  The lattice
    holds the exact ties of rint(x * 1000) -- n with a factor 16 -- that no
    golden fixture contains."""
    from scipy.stats import entropy

    votes, c, n = count_lattice()
    assert votes.shape == (37321, LATTICE_A)
    halves = exact_halves(c, n)
    assert int(halves.sum()) >= 1000, int(halves.sum())
    freq, ent = O.oracle_vote_table(votes, 2)
    want = np.stack([np.round(c / n, 3), np.round((n - c) / n, 3)], axis=1)
    assert same_bits(freq, want)
    assert same_bits(freq[halves], want[halves])  # the ties themselves (a subset, stated)
    assert same_bits(ent, entropy(want, axis=1))
    assert same_bits(O.oracle_table_entropy(want), ent)


@pytest.mark.parametrize("C", range(1, 9))
def test_every_class_count_is_scipy_entropy(C):
    """C = 1..8 on random votes in [-1, C) with a row of no vote at all, a row
    of 127 and a row of -128 (bytes outside [0, C) are missing votes,
    ce_oracle.c ce_ref_vote_table): the frequencies are the reference's
    Counter loop (ref_vote_table, amg_test.py:109-115), the entropies scipy's,
    NaN for the three empty rows; C = 1 gives +0.0, not -0.0."""
    from scipy.stats import entropy

    rng = np.random.default_rng(800 + C)
    votes = rng.integers(-1, C, size=(300, 40)).astype(np.int8)
    votes[7], votes[8], votes[9] = -1, 127, -128
    freq, ent = O.oracle_vote_table(votes, C)
    assert same_bits(freq, O.ref_vote_table(votes, C))
    empty = np.zeros(len(votes), bool)
    empty[7:10] = True
    assert np.isnan(freq[empty]).all() and np.isnan(ent[empty]).all()
    assert not np.isnan(ent[~empty]).any()
    with np.errstate(invalid="ignore"):
        want = entropy(freq, axis=1)
    assert same_bits(ent, want)
    assert same_bits(O.oracle_table_entropy(freq), want)
    if C == 1:
        assert not np.signbit(ent[~empty]).any() and (ent[~empty] == 0.0).all()


VA_SPECIALS = [np.nan, -np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf]


def test_va_specials_follow_the_verbatim_quadrant_rule():
    """Every ordered (valence, arousal) pair of NaN, +-inf, +-1, +-denormal and
    +-0.0: ce_ref_quadrant is the verbatim rule (ref_quadrant, amg_test.py:69-78),
    -1 where either value is NaN (dropna, :101); as single-annotation rows of
    oracle_va_table the frequency row is that quadrant's one-hot with entropy
    +0.0, or NaN for a dropped vote."""
    pairs = [(v, a) for v in VA_SPECIALS for a in VA_SPECIALS]
    quad = []
    for v, a in pairs:
        got = O.lib().ce_ref_quadrant(a, v)
        if np.isnan(v) or np.isnan(a):
            assert got == -1, (v, a)
        else:
            assert got == int(O.ref_quadrant(a, v)[1]) - 1, (v, a)
        quad.append(got)
    quad = np.array(quad)
    assert set(quad.tolist()) == {-1, 0, 1, 2, 3}
    va = np.array(pairs, np.float64).reshape(len(pairs), 1, 2)
    freq, ent = O.oracle_va_table(va)
    want = np.where(quad[:, None] < 0, np.nan, (np.arange(4)[None, :] == quad[:, None]).astype(np.float64))
    assert same_bits(freq, want)
    assert same_bits(ent, np.where(quad < 0, np.nan, 0.0))


def test_table_entry_points_answer_before_any_launch():
    """What ce_vote_entropy and ce_va_entropy answer on the host: an empty
    matrix (N = 0) is no error even with null pointers, as an empty device
    tensor has; a row pitch below A and a valence/arousal array that is not
    16-byte aligned are CE_EINVAL -- raised as an error that is both the
    ValueError it always was and a CEError; C outside [1, 8] is unsupported."""
    import ctypes

    from ce_amd import _lib

    p = ctypes.c_void_p
    lib = _lib.load()
    assert lib.ce_vote_entropy(None, 0, 7, 3, 7, None, None, None) == _lib.CE_OK
    with pytest.raises(ValueError, match="ld=0") as ei:
        _lib.call("ce_vote_entropy", p(16), 10, 5, 4, 0, None, p(16), None)
    assert isinstance(ei.value, _lib.CEError) and ei.value.code == _lib.CE_EINVAL
    with pytest.raises(ValueError, match="null pointer"):
        _lib.call("ce_vote_entropy", None, 10, 5, 4, 5, None, p(16), None)
    with pytest.raises(_lib.CEError, match=r"C=9 outside \[1, 8\]") as ei:
        _lib.call("ce_vote_entropy", p(16), 10, 5, 9, 5, None, p(16), None)
    assert ei.value.code == _lib.CE_EUNSUPPORTED and not isinstance(ei.value, ValueError)
    with pytest.raises(_lib.CEError, match="16-byte aligned") as ei:
        _lib.call("ce_va_entropy", p(24), 10, 3, None, p(16), None)
    assert isinstance(ei.value, ValueError)
