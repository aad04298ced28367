"""numpy restatements the evaluate step of the linear members is tested
against (ce_gnb_score_users, ce_sgd_score_users, ce_f1_weighted_users):

  gnb_jll       GaussianNB._joint_log_likelihood, the math of
                oracle/ce_oracle.py ref_gnb_predict_proba up to the jll
  sgd_decision  SGDClassifier.decision_function in the kernels' order: lane j
                of a frame's 8 takes the features 8m + j in one fma chain, the
                8 chains are added by the xor butterfly, then the intercept
  f1_weighted   sklearn 1.7.2's f1_score(average='weighted') from a confusion
                matrix, the expression ce_f1_weighted_users states

tests/test_members_eval.py pins them to sklearn; the GPU tests compare the
kernels with them in all 64 bits."""
import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.log, _libm.exp, _libm.fma):
    _f.restype = ctypes.c_double
_libm.log.argtypes = _libm.exp.argtypes = [ctypes.c_double]
_libm.fma.argtypes = [ctypes.c_double] * 3


def libm_log(a):
    """The C library's log, element by element (numpy's own float64 log is SIMD code that may differ by an ulp)."""
    a = np.asarray(a, np.float64)
    return np.array([_libm.log(float(v)) for v in a.reshape(-1)], np.float64).reshape(a.shape)


def libm_exp(a):
    a = np.asarray(a, np.float64)
    return np.array([_libm.exp(float(v)) for v in a.reshape(-1)], np.float64).reshape(a.shape)


def gnb_jll(X, theta, var, class_prior):
    """[F, C] joint log-likelihood of one GaussianNB model: np.log(prior_c) +
    ((-0.5 * np.sum(np.log(2 pi var_c))) - 0.5 * np.sum((X - theta_c)**2 / var_c, 1)),
    the sums numpy's pairwise ones, the logs the C library's."""
    X = np.ascontiguousarray(X, np.float64)
    jll = []
    with np.errstate(all="ignore"):
        for i in range(len(class_prior)):
            jointi = libm_log(np.array([class_prior[i]], np.float64))[0]
            n_ij = -0.5 * np.sum(libm_log(2.0 * np.pi * var[i, :]))
            n_ij = n_ij - 0.5 * np.sum(((X - theta[i, :]) ** 2) / (var[i, :]), 1)
            jll.append(jointi + n_ij)
    return np.array(jll).T.reshape(len(X), len(class_prior))


def sgd_decision(X, coef, intercept):
    """[F, K] decision values of one SGD model in the kernels' order (a row loop)."""
    X, coef = np.asarray(X, np.float64), np.asarray(coef, np.float64)
    F, D = X.shape
    K = coef.shape[0]
    out = np.empty((F, K))
    for r in range(F):
        for k in range(K):
            d = [0.0] * 8
            for f in range(D):
                d[f & 7] = _libm.fma(float(X[r, f]), float(coef[k, f]), d[f & 7])
            with np.errstate(all="ignore"):
                s = np.float64
                v = (s(s(d[0]) + s(d[1])) + s(s(d[2]) + s(d[3]))) + (s(s(d[4]) + s(d[5])) + s(s(d[6]) + s(d[7])))
                out[r, k] = v + s(intercept[k])
    return out


def predict_labels(scores, binary=False):
    """sklearn's label rule over the scores: np.argmax (the first maximum; a NaN
    wins at its first occurrence), or score > 0 for a binary model ([F, 1])."""
    scores = np.asarray(scores, np.float64)
    if binary:
        return (scores[:, 0] > 0).astype(np.int32)
    return np.argmax(scores, axis=1).astype(np.int32)


def confusion(y, pred, C, user=None, U=1):
    """int64 [U, C, C]: np.add.at over the rows with a user and a label in [0, C)."""
    y, pred = np.asarray(y, np.int64), np.asarray(pred, np.int64)
    user = np.zeros(len(y), np.int64) if user is None else np.asarray(user, np.int64)
    ok = (user >= 0) & (y >= 0) & (y < C)
    cm = np.zeros((U, C, C), np.int64)
    np.add.at(cm, (user[ok], y[ok], pred[ok]), 1)
    return cm


def prf(cm):
    """[C, 4] precision, recall, F1 and support of every class from one [C, C]
    confusion matrix; 0.0 on a zero denominator and for an absent class."""
    cm = np.asarray(cm, np.int64)
    C = cm.shape[0]
    out = np.zeros((C, 4))
    for c in range(C):
        true_c, pred_c, tp = int(cm[c, :].sum()), int(cm[:, c].sum()), int(cm[c, c])
        out[c, 0] = float(tp) / float(pred_c) if pred_c else 0.0
        out[c, 1] = float(tp) / float(true_c) if true_c else 0.0
        out[c, 2] = (2.0 * float(tp)) / (float(true_c) + float(pred_c)) if true_c + pred_c > 0 else 0.0
        out[c, 3] = float(true_c)
    return out


def f1_weighted(cm):
    """f1_score(y_true, y_pred, average='weighted') (sklearn 1.7.2) from one
    [C, C] confusion matrix cm[true, predicted], in Python floats (IEEE double):
    the classes present in y_true or y_pred, f_c = 2 tp / (true + pred), the
    terms f_c * true_c in ascending c added one after the other onto 0.0 (fewer
    than 8) or by numpy's 8-accumulator tree (8), over the number of rows.  NaN
    without a row."""
    cm = np.asarray(cm, np.int64)
    C = cm.shape[0]
    terms, total = [], 0
    for c in range(C):
        true_c, pred_c, tp = int(cm[c, :].sum()), int(cm[:, c].sum()), int(cm[c, c])
        total += true_c
        if true_c + pred_c > 0:
            f = (2.0 * float(tp)) / (float(true_c) + float(pred_c))
            terms.append(f * float(true_c))
    if total == 0:
        return math.nan
    if len(terms) == 8:
        t = terms
        s = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))
    else:
        s = 0.0
        for v in terms:
            s += v
    return s / float(total)
