"""SGDClassifier.partial_fit (amg_test.py:509, the 'classifier_sgd' member)
without a GPU: the row-loop restatement (tests/sgd_fit_ref.py) against the
committed sklearn fixture and, where the installed sklearn is the pinned 1.7.2,
against sklearn itself, bit for bit; the host seed rule; the C-ABI's exports
and refusals."""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import golden
from sgd_fit_ref import chain_seeds, same_bits, sgd_partial_fit, shuffle_order

PINNED = "1.7.2"


def fixture_cases():
    fx = golden("sgd_partial_fit")
    return {name: {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "_")} for name in fx["cases"]}


CASES = fixture_cases()


def test_fixture_covers_the_cases():
    """What the fixture has to hold: C = 2, 3, 4, 8; D = 1, 63, 64, 65, 260; a
    one-row batch; a batch lacking a class; alpha = 1 and 10 from a fresh model;
    rows scaled by 1e3."""
    import os

    from conftest import GOLDEN

    assert os.path.getsize(os.path.join(GOLDEN, "sgd_partial_fit.npz")) < 512 * 1024
    assert {int(c["C"]) for c in CASES.values()} >= {2, 3, 4, 8}
    assert {c["X"].shape[1] for c in CASES.values()} >= {1, 63, 64, 65, 260}
    fresh = {float(c["alpha"]) for c in CASES.values() if float(c["t_init"]) == 1.0 and not c["coef_init"].any()}
    assert fresh >= {1.0, 10.0}
    assert any(float(c["scale"]) == 1e3 for c in CASES.values())
    for c in CASES.values():
        assert len(c["rows0"]) == 1 and 1 not in c["labels1"] and len(c["rows3"]) > 16


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_fixture(name):
    c = CASES[name]
    coef, b, t = c["coef_init"], c["intercept_init"], float(c["t_init"])
    for e in range(4):
        coef, b, t, finite = sgd_partial_fit(c["X"][c[f"rows{e}"]], c[f"labels{e}"], coef, b, t, float(c["alpha"]),
                                             int(c["random_state"]))
        assert finite
        assert same_bits(coef, c[f"coef{e}"]) and same_bits(b, c[f"intercept{e}"]) and t == float(c[f"t{e}"]), (name, e)


@pytest.mark.parametrize("C", [2, 3, 4, 8])
@pytest.mark.parametrize("D", [3, 9, 66, 260])
def test_restatement_equals_sklearn(D, C):
    """Chained batches of 1 .. 130 rows on a fitted model, and alpha = 1 and 10
    on a fresh one (the zero shrink factor and the wscale reset), rows scaled
    by 1e3 for D = 3 (p <= -37)."""
    sklearn = pytest.importorskip("sklearn")
    if sklearn.__version__ != PINNED:
        pytest.skip(f"the restatement is pinned to sklearn {PINNED} (installed: {sklearn.__version__})")
    from sklearn.linear_model import SGDClassifier

    warnings.simplefilter("ignore")
    rng = np.random.default_rng(1000 * C + D)
    K = 1 if C == 2 else C
    scale = 1e3 if D == 3 else 1.0
    for alpha in (1e-4, 0.5, 1.0, 10.0):
        rs = int(rng.integers(0, 100000))
        m = SGDClassifier(loss="log_loss", penalty="l2", random_state=rs, warm_start=True, alpha=alpha)
        if alpha == 1e-4:
            m.fit(rng.normal(size=(5 * C, D)), np.arange(5 * C) % C)
            coef, b, t = m.coef_.copy(), m.intercept_.copy(), float(m.t_)
        else:
            coef, b, t = np.zeros((K, D)), np.zeros(K), 1.0
        for i, n in enumerate((1, 2, 33, 130) if D < 260 else (1, 40)):
            X, y = rng.normal(size=(n, D)) * scale, rng.integers(0, C, n)
            if alpha != 1e-4 and i == 0:
                m.partial_fit(X, y, classes=np.arange(C))
            else:
                m.partial_fit(X, y)
            coef, b, t, finite = sgd_partial_fit(X, y, coef, b, t, alpha, rs)
            assert finite
            assert same_bits(coef, m.coef_) and same_bits(b, m.intercept_) and t == m.t_, (D, C, alpha, n)


@pytest.mark.parametrize("C", [4, 8])
def test_restatement_equals_sklearn_past_128_rows_at_full_width(C):
    """D = 260: chained batches of 129 and 257 rows (the device kernel fetches the
    visiting order's rows in blocks of 64; tests/test_gpu_fit_batch_edges.py
    compares it with the restatement there).  The D = 260 chains above stop at 40 rows."""
    sklearn = pytest.importorskip("sklearn")
    if sklearn.__version__ != PINNED:
        pytest.skip(f"the restatement is pinned to sklearn {PINNED} (installed: {sklearn.__version__})")
    from sklearn.linear_model import SGDClassifier

    warnings.simplefilter("ignore")
    rng = np.random.default_rng(260 + C)
    D, rs = 260, 31 + C
    m = SGDClassifier(loss="log_loss", penalty="l2", random_state=rs, warm_start=True, alpha=1e-4)
    m.fit(rng.normal(size=(5 * C, D)), np.arange(5 * C) % C)
    coef, b, t = m.coef_.copy(), m.intercept_.copy(), float(m.t_)
    for n in (129, 257):
        X, y = rng.normal(size=(n, D)), rng.integers(0, C, n)
        m.partial_fit(X, y)
        coef, b, t, finite = sgd_partial_fit(X, y, coef, b, t, 1e-4, rs)
        assert finite
        assert same_bits(coef, m.coef_) and same_bits(b, m.intercept_) and t == m.t_, (C, n)


def test_restatement_overflow_is_where_sklearn_raises():
    sklearn = pytest.importorskip("sklearn")
    if sklearn.__version__ != PINNED:
        pytest.skip(f"pinned to sklearn {PINNED}")
    from sklearn.linear_model import SGDClassifier

    rng = np.random.default_rng(3)
    X, y = rng.normal(size=(12, 5)) * 1e300, np.arange(12) % 3
    m = SGDClassifier(loss="log_loss", random_state=1)
    with pytest.raises(ValueError, match="Floating-point under-/overflow occurred at epoch #1"):
        m.partial_fit(X, y, classes=np.arange(3))
    *_, finite = sgd_partial_fit(X, y, np.zeros((3, 5)), np.zeros(3), 1.0, 1e-4, 1)
    assert not finite


def test_shuffle_order_equals_sklearn():
    pytest.importorskip("sklearn")
    from sklearn.utils._seq_dataset import ArrayDataset64

    for n, seed in ((1, 5), (2, 0), (7, 1), (130, 2**31 - 2), (400, 123456789)):
        ds = ArrayDataset64(np.arange(n, dtype=np.float64).reshape(n, 1), np.zeros(n), np.ones(n), seed=1)
        ds._shuffle_py(seed)
        got = [int(ds._next_py()[0][0][0]) for _ in range(n)]
        assert got == shuffle_order(n, seed), (n, seed)


@pytest.mark.parametrize("C", [2, 3, 4, 8])
def test_chain_seeds(C):
    from ce_amd import ops

    for rs in (0, 1, 42, 2**31 - 1):
        got = ops.sgd_chain_seeds(rs, C)
        assert got.dtype == np.uint32 and got.shape == (1 if C == 2 else C,)
        assert np.array_equal(got, chain_seeds(rs, C))
    assert np.array_equal(ops.sgd_chain_seeds(np.int64(7), C), chain_seeds(7, C))
    for bad in (None, 1.5, np.random.RandomState(0), True):
        with pytest.raises(ValueError, match="integer random_state"):
            ops.sgd_chain_seeds(bad, C)


def test_optimal_init():
    from ce_amd import ops
    from sgd_fit_ref import optimal_init

    for alpha in (1e-6, 1e-4, 0.5, 1.0, 10.0):
        assert ops.sgd_optimal_init(alpha) == optimal_init(alpha)
        typw = np.sqrt(1.0 / np.sqrt(alpha))
        assert ops.sgd_optimal_init(alpha) == 1.0 / (typw * alpha)  # the gradient at (1, -typw) is negative
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            ops.sgd_optimal_init(bad)


def test_library_exports():
    from ce_amd import _lib

    lib = _lib.load()
    for name in ("ce_sgd_partial_fit", "ce_sgd_partial_fit_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    ws = lib.ce_sgd_partial_fit_workspace_bytes
    assert ws(2048, 4) == 0 and ws(2049, 4) == 2049 * 4 * 4   # K * R indices: in LDS up to 8192
    assert ws(8192, 2) == 0 and ws(8193, 2) == 8193 * 4       # two classes: one problem
    assert ws(0, 4) == 0 and ws(100, 1) == 0 and ws(100, 9) == 0


def test_partial_fit_validates_without_gpu():
    from ce_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(16)

    def rc(D=4, ld=4, U=1, C=4, alpha=1e-4, oi=100.0, grad=0, X=p, rows=p, labels=p, ro=p, seeds=p, coef=p, b=p, t=p,
           status=p, ws=None):
        return lib.ce_sgd_partial_fit(X, 10, D, ld, rows, labels, ro, U, C, alpha, oi, seeds, grad, coef, b, t, status,
                                      ws, 0, None)

    assert rc(D=0, ld=4) == _lib.CE_EINVAL
    assert rc(D=513, ld=513) == _lib.CE_EUNSUPPORTED and b"D <= 512" in lib.ce_last_error()
    assert rc(C=1) == _lib.CE_EINVAL and rc(C=9) == _lib.CE_EUNSUPPORTED
    assert rc(U=0) == _lib.CE_EINVAL and rc(ld=3) == _lib.CE_EINVAL
    for alpha in (0.0, -1e-4, float("nan"), float("inf")):
        assert rc(alpha=alpha) == _lib.CE_EINVAL
    assert rc(oi=0.0) == _lib.CE_EINVAL and rc(grad=2) == _lib.CE_EINVAL and rc(grad=-1) == _lib.CE_EINVAL
    for name in ("X", "rows", "labels", "ro", "seeds", "coef", "b", "t", "status"):
        assert rc(**{name: None}) == _lib.CE_EINVAL, name
    assert rc(ws=ctypes.c_void_p(18)) == _lib.CE_EINVAL  # a misaligned workspace


def test_python_guards_without_gpu():
    torch = pytest.importorskip("torch")
    import ce_amd
    from ce_amd import ops

    z = torch.zeros((4, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match="HIP device"):
        ops.sgd_partial_fit(z, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), z[:3].clone(),
                            z[0, :3].clone(), z[0, :1].clone(), seeds=chain_seeds(0, 3))
    assert "DeviceSGDClassifier" in ce_amd.__all__
    with pytest.raises(ValueError, match="random_state"):
        ce_amd.DeviceSGDClassifier(np.zeros((3, 4)), np.zeros(3), 1.0, device="cpu")
    with pytest.raises(ValueError, match="binary problems"):
        ce_amd.DeviceSGDClassifier(np.zeros((2, 4)), np.zeros(2), 1.0, random_state=0, device="cpu")
    with pytest.raises(ValueError, match="grad"):
        ce_amd.DeviceSGDClassifier(np.zeros((3, 4)), np.zeros(3), 1.0, random_state=0, grad="hinge", device="cpu")
    with pytest.raises(ValueError, match="alpha"):
        ce_amd.DeviceSGDClassifier(np.zeros((3, 4)), np.zeros(3), 1.0, alpha=0.0, random_state=0, device="cpu")
    m = ce_amd.DeviceSGDClassifier(np.zeros((2, 3, 4)), np.zeros((2, 3)), 1.0, random_state=[5, 6], device="cpu")
    assert (m.U, m.K, m.C, m.D) == (2, 3, 3, 4) and m.t.tolist() == [1.0, 1.0]
    assert np.array_equal(m.seeds.numpy().view(np.uint32), np.stack([chain_seeds(5, 3), chain_seeds(6, 3)]))
    st = m.state()
    assert st["coef"].shape == (2, 3, 4) and st["status"].tolist() == [0, 0]
    assert m.check_finite() is m
    m.status[1] = 1
    with pytest.raises(ValueError, match=r"Floating-point under-/overflow occurred at epoch #1.*\[1\]"):
        m.check_finite()
    m.status[0] = 2
    with pytest.raises(RuntimeError, match="not updated"):
        m.check_finite()
