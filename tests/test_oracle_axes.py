"""Pin the CPU oracle's committee entropy at EVERY class count.

tests/test_gpu_committee_axes.py checks the HIP kernels against
oracle.ce_oracle.oracle_committee_entropy for every C in 1..2048, so the oracle
itself must be right there first: its restatement of numpy's pairwise summation
has a different tree for almost every C, and the golden fixtures pin it at six
wide class counts only.  Here every C is compared with the reference's own
expression (ce_oracle.ref_mc: np.mean over the member axis, then
scipy.stats.entropy), means and entropies bit for bit (uint64 patterns, NaN
matching NaN).

Per C and M in {1, 3, 4}: four items of f64 input, four of f32 input and four
of bf16 bit patterns (the reference sees the latter two upcast to float64,
which is exact), rows unnormalised; at a few C an all-zero row, a NaN and a
negative value."""
import warnings

import numpy as np
import pytest

from axes_common import bf16_bits, bf16_to_f64, first_diff, same_bits
from oracle import ce_oracle as O

pytest.importorskip("scipy")

CS = range(1, 2049)
ITEMS = 4
# class counts that also carry special rows: both sides of the leaf size (128), of the 8-accumulator
# block, and the ends of the range
SPECIAL_CS = (1, 2, 7, 8, 9, 127, 128, 129, 136, 1000, 1023, 2047, 2048)


def _inputs(rng, M, C):
    """[ITEMS, M, C] float64 values, unnormalised rows in (0, 2)."""
    e = -np.log(rng.random((ITEMS, M, C)))
    P = e / e.sum(-1, keepdims=True) * rng.uniform(0.25, 2.0, (ITEMS, M, 1))
    if C in SPECIAL_CS:
        P[0] = 0.0                       # all-zero consensus row: 0 / 0
        P[1, M - 1, C - 1] = np.nan      # a NaN member value
        P[2, :, C // 2] = -0.25          # a negative mean (entr(-x) = -inf; C = 1: -x / -x = 1)
        if C > 1:
            P[3, :, 0] = -0.0            # a -0.0 class in an otherwise ordinary row
    return P


@pytest.mark.parametrize("M", [1, 3, 4])
def test_oracle_equals_reference_every_class_count(M):
    rng = np.random.default_rng(20260 + M)
    bad = []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for C in CS:
            P64 = _inputs(rng, M, C)
            P32 = _inputs(rng, M, C).astype(np.float32)
            Pbf = bf16_bits(_inputs(rng, M, C).astype(np.float32))
            # the reference: one call over the three inputs' items, every value a float64
            allp = np.concatenate([P64, P32.astype(np.float64), bf16_to_f64(Pbf)], axis=0)  # [3 * ITEMS, M, C]
            _, ent_r, mean_r = O.ref_mc([allp[:, m, :] for m in range(M)], 1)
            for k, P in enumerate((P64, P32, Pbf)):
                ent, mean = O.oracle_committee_entropy(P, "NMC", want_mean=True)
                sl = slice(k * ITEMS, (k + 1) * ITEMS)
                if not same_bits(mean, mean_r[sl]):
                    bad.append((C, P.dtype.name, "mean") + first_diff(mean, mean_r[sl]))
                if not same_bits(ent, ent_r[sl]):
                    bad.append((C, P.dtype.name, "ent") + first_diff(ent, ent_r[sl]))
    assert not bad, (len(bad), bad[:8])


def test_special_rows_are_what_they_claim():
    """The special rows above reach both sides as NaN / -inf entropies (not as
    ordinary numbers that would make the comparison above vacuous there)."""
    rng = np.random.default_rng(5)
    for C in SPECIAL_CS:
        ent = O.oracle_committee_entropy(_inputs(rng, 3, C), "NMC")
        assert np.isnan(ent[0]) and np.isnan(ent[1]), (C, ent)
        assert C == 1 or np.isnan(ent[2]) or ent[2] == -np.inf, (C, ent)
        assert np.isfinite(ent[3]), (C, ent)
