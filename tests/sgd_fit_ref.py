"""SGDClassifier(loss='log_loss', penalty='l2').partial_fit restated row by row:
the update the reference runs at amg_test.py:509 on its 'classifier_sgd' member
(deam_classifier.py:214-217: learning_rate='optimal', fit_intercept, shuffle,
no averaging, no weights), one epoch of sklearn's _plain_sgd64 per binary
problem (K = C one-vs-rest problems for C > 2, class k positive; K = 1 for
C = 2, class 1 positive).

Every operation is an IEEE f64 add, subtract, multiply or true divide, or the C
library's exp; the only reduction is `dot` (the D products added one after the
other, in feature order, onto +0.0).  tests/test_sgd_partial_fit.py pins it to
sklearn 1.7.2 bit for bit.  grad="log_dloss" is the gradient of the
reference's own sklearn 0.24.1 (Log.dloss on +-1 labels), which no installed
sklearn pins."""
import math

import numpy as np

INT32_MAX = int(np.iinfo(np.int32).max)
MAX_DLOSS = 1e12
GRADS = ("half_binomial", "log_dloss")


def chain_seeds(random_state, C):
    """The shuffle seed of each of the K binary problems of one partial_fit
    call, uint32 [K].  An integer random_state re-seeds on every call, so they
    are the same for every call: _fit_multiclass draws one seed per class,
    fit_binary seeds a RandomState with it, make_dataset takes one draw, and the
    next one seeds the shuffle."""
    if C > 2:
        seeds = np.random.RandomState(random_state).randint(INT32_MAX, size=C)
        chains = [np.random.RandomState(int(s)) for s in seeds]
    else:
        chains = [np.random.RandomState(random_state)]
    out = []
    for rs in chains:
        rs.randint(1, INT32_MAX)  # make_dataset's draw
        out.append(rs.randint(INT32_MAX))
    return np.array(out, dtype=np.uint32)


def our_rand_r(seed):
    """sklearn's xorshift on a uint32: (the draw, the new seed)."""
    if seed == 0:
        seed = 1
    seed ^= (seed << 13) & 0xFFFFFFFF
    seed ^= seed >> 17
    seed ^= (seed << 5) & 0xFFFFFFFF
    return seed % 2147483648, seed


def shuffle_order(n, seed):
    """SequentialDataset.shuffle(seed) of the identity over n rows."""
    ind = list(range(n))
    seed = int(seed)
    for i in range(n - 1):
        r, seed = our_rand_r(seed)
        j = i + r % (n - i)
        ind[i], ind[j] = ind[j], ind[i]
    return ind


def optimal_init(alpha):
    """The t offset of learning_rate='optimal', the long way (half-binomial gradient at (1, -typw))."""
    typw = math.sqrt(1.0 / math.sqrt(alpha))
    initial_eta0 = typw / max(1.0, grad_half_binomial(1.0, -typw))
    return 1.0 / (initial_eta0 * alpha)


def grad_half_binomial(y, p):
    """sklearn >= 1.x: cgradient_half_binomial, y in {0, 1}."""
    if p > -37.0:
        e = math.exp(-p)
        return ((1.0 - y) - y * e) / (1.0 + e)
    return math.exp(p) - y


def grad_log_dloss(y, p):
    """sklearn 0.24.1: Log.dloss on labels +-1 (y in {0, 1} here)."""
    ys = 1.0 if y > 0.0 else -1.0
    z = p * ys
    if z > 18.0:
        return math.exp(-z) * -ys
    if z < -18.0:
        return -ys
    return -ys / (math.exp(z) + 1.0)


def dot(w, x):
    """s = 0.0; s += w[j] * x[j] in feature order (np.add.accumulate adds one after the other)."""
    return float(np.add.accumulate(np.concatenate(([0.0], w * x)))[-1])


def plain_sgd(X, y01, w, b, t, alpha, seed, grad="half_binomial"):
    """One epoch of one binary problem.  X [n, D], y01 [n] in {0.0, 1.0}, w [D],
    intercept b, step counter t at entry.  Returns (w, b)."""
    g = {"half_binomial": grad_half_binomial, "log_dloss": grad_log_dloss}[grad]
    w = np.array(w, dtype=np.float64)
    b, t, alpha = float(b), float(t), float(alpha)
    oi = optimal_init(alpha)
    wscale = 1.0
    with np.errstate(all="ignore"):
        for i in shuffle_order(X.shape[0], seed):
            x, y = X[i], float(y01[i])
            p = dot(w, x) * wscale + b
            eta = 1.0 / (alpha * (oi + t - 1.0))
            d = g(y, p)  # no exp argument above 37: math.exp cannot overflow
            d = -MAX_DLOSS if d < -MAX_DLOSS else (MAX_DLOSS if d > MAX_DLOSS else d)
            update = -eta * d
            wscale *= max(0.0, 1.0 - eta * alpha)
            if wscale < 1e-9:
                w = w * wscale
                wscale = 1.0
            if update != 0.0:
                w = w + x * (update / wscale)
                b += update
            t += 1.0
        w = w * wscale
    return w, b


def sgd_partial_fit(X, y, coef, intercept, t, alpha=1e-4, random_state=0, grad="half_binomial", seeds=None):
    """One partial_fit of a model on the batch (X [n, D] in batch order, y [n]
    in [0, C)); coef [K, D], intercept [K].  Returns new (coef, intercept, t,
    finite): the inputs are left alone, an empty batch changes nothing, and
    `finite` is False where sklearn would raise its under-/overflow error."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.asarray(y)
    coef = np.array(coef, dtype=np.float64).reshape(-1, X.shape[1])
    intercept = np.array(intercept, dtype=np.float64).reshape(-1)
    K = coef.shape[0]
    C = 2 if K == 1 else K
    if seeds is None:
        seeds = chain_seeds(random_state, C)
    n = X.shape[0]
    if n == 0:
        return coef, intercept, float(t), True
    for k in range(K):
        pos = 1 if K == 1 else k
        coef[k], intercept[k] = plain_sgd(X, (y == pos).astype(np.float64), coef[k], intercept[k], t, alpha, seeds[k], grad)
    finite = bool(np.isfinite(coef).all() and np.isfinite(intercept).all())
    return coef, intercept, float(t) + float(n), finite


def same_bits(a, b):
    """0 ulp: equal bit patterns, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))
