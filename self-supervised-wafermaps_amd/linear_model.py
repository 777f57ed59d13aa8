"""Logistic-regression probes of dumped embeddings: the convex problem solved to a gradient tolerance, a list of C at once.

The linear probe of an embedding is a convex problem with one answer; `LogisticRegression` and
`MultilabelLogisticRegression` return that answer (to `tol` on the gradient) instead of wherever a fixed number of Adam
epochs got (`models/evals.py` keeps those probes as they are).  The objective is sklearn 1.7's, stated here as this
project's own:

    f(W, b) = (1 / S) sum_i s_i l_i(W, b) + ||W||_F^2 / (2 C S),    S = sum_i s_i,

l_i the multinomial (softmax) or binomial (sigmoid) log-loss of row i, s_i = sample_weight_i * class_weight[y_i] (a row
with y == -1 has s_i = 0 and is not counted in S: the project's "-1 = unlabelled"), the intercept b unpenalised.  A
problem stops when max |grad f| <= tol.

One evaluation of all problems is two passes over the rows in float64 on the float32 features (csrc/logreg.hip): the
logits, softmax / sigmoid, residuals and losses, then the gradient resid^T [x | 1] on `wm_gmm_weighted_sums`' launch
path.  Every sum has an order that depends on the sizes alone and a problem's numbers do not depend on which other
problems share the call, so a C fitted alone and the same C fitted inside a list give the same bits, and so do two fits.
The kernels never see C: the penalty, the division by S and the L-BFGS recursion are numpy float64 on [problems, K (d + 1)]
arrays (`lbfgs_lockstep`), one state machine per problem, all unfinished problems evaluated by one call per round.

With a list of C the fitted attributes gain a leading axis (`coef_` [n_C, K, d]) and `model[i]` is the fitted model of
`C_[i]` alone (plain indexing; `best(scores)` is `model[argmax(scores)]`).  Features are taken as given: standardise
them first (`retrieval.standardize`).  Not implemented: L1 / elastic-net, Newton solvers, warm starts, cross-validation.
"""
from __future__ import annotations

import warnings
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

try:  # sklearn is optional: its warning class when it is there, so `filterwarnings` written for sklearn still match
    from sklearn.exceptions import ConvergenceWarning
except Exception:  # pragma: no cover
    class ConvergenceWarning(UserWarning):
        """A problem ended at max_iter (or in its line search) before max |grad f| <= tol."""


MAX_FEATURES = 1024
MAX_COLUMNS = 256
_C1 = 1e-4          # Armijo
_SIGMA = 0.9        # curvature (approximate Wolfe) test near the optimum
_EPS_F = 2.0 ** -46  # relative slack on f where its decrease is below its rounding
_MAX_HALVINGS = 40


# ------------------------------------------------------------------------------------------------ the solver


class _Problem:
    """One L-BFGS run as a state machine: `trial()` is the point it wants evaluated, `feed(loss, grad)` hands it that
    evaluation.  Everything is 1-D numpy float64 of this problem alone."""

    def __init__(self, w0, lam, tol, max_iter, history):
        self.x = np.array(w0, dtype=np.float64).ravel()
        self.lam = np.array(lam, dtype=np.float64).ravel()
        self.tol, self.max_iter, self.m = float(tol), int(max_iter), int(history)
        self.f = self.g = self.d = None
        self.s_hist, self.y_hist = [], []
        self.n_iter, self.done, self.converged, self.t, self.halvings = 0, False, False, 1.0, 0

    def _objective(self, x, loss, grad):
        return float(loss) + 0.5 * float(np.dot(self.lam * x, x)), np.asarray(grad, dtype=np.float64).ravel() + self.lam * x

    def _direction(self):
        q = self.g.copy()
        alphas = []
        for s, y in zip(reversed(self.s_hist), reversed(self.y_hist)):
            a = float(np.dot(s, q)) / float(np.dot(y, s))
            alphas.append(a)
            q -= a * y
        if self.s_hist:
            s, y = self.s_hist[-1], self.y_hist[-1]
            q *= float(np.dot(s, y)) / float(np.dot(y, y))
        for (s, y), a in zip(zip(self.s_hist, self.y_hist), reversed(alphas)):
            b = float(np.dot(y, q)) / float(np.dot(y, s))
            q += (a - b) * s
        d = -q
        gd = float(np.dot(self.g, d))
        if not gd < 0.0:  # not a descent direction (rounding): steepest descent, history dropped
            self.s_hist, self.y_hist = [], []
            d = -self.g
            gd = float(np.dot(self.g, d))
        self.d, self.gd = d, gd
        # the first step of a run (and after a reset) has no curvature yet: a step of length <= 1
        self.t = 1.0 if self.s_hist else min(1.0, 1.0 / max(float(np.abs(self.g).sum()), 1e-300))
        self.halvings = 0

    def trial(self):
        return self.x if self.f is None or self.done else self.x + self.t * self.d

    def _finish_if(self):
        if float(np.abs(self.g).max()) <= self.tol:
            self.done = self.converged = True
        elif self.n_iter >= self.max_iter:
            self.done = True

    def feed(self, loss, grad):
        if self.done:
            return
        if self.f is None:  # the starting point
            self.f, self.g = self._objective(self.x, loss, grad)
            self._finish_if()
            if not self.done:
                self._direction()
            return
        xt = self.x + self.t * self.d
        ft, gt = self._objective(xt, loss, grad)
        gtd = float(np.dot(gt, self.d))
        armijo = ft <= self.f + _C1 * self.t * self.gd
        # where the decrease of f is below its rounding, the slope decides (Hager & Zhang's approximate Wolfe test)
        flat = ft <= self.f + _EPS_F * abs(self.f) and _SIGMA * self.gd <= gtd <= (2.0 * _C1 - 1.0) * self.gd
        if not (np.isfinite(ft) and (armijo or flat)):
            self.halvings += 1
            self.t *= 0.5
            if self.halvings > _MAX_HALVINGS:
                self.done = True  # the line search found no acceptable step: stays where it is, not converged
            return
        s, y = xt - self.x, gt - self.g
        sy = float(np.dot(s, y))
        if sy > 1e-10 * float(np.linalg.norm(s)) * float(np.linalg.norm(y)):  # the update keeps H positive definite
            self.s_hist.append(s)
            self.y_hist.append(y)
            if len(self.s_hist) > self.m:
                self.s_hist.pop(0)
                self.y_hist.pop(0)
        self.x, self.f, self.g = xt, ft, gt
        self.n_iter += 1
        self._finish_if()
        if not self.done:
            self._direction()


def lbfgs_lockstep(evaluate: Callable, w0, penalties, tol: float, max_iter: int, history: int = 10):
    """Minimise P independent problems f_p(w) = loss_p(w) + 0.5 sum_j penalties[p][j] w_j^2 by L-BFGS in numpy float64:
    two-loop recursion over the last `history` pairs, Armijo backtracking (halving from a unit step; near the optimum,
    where f no longer resolves its decrease, the approximate Wolfe test on the slope), a pair kept only when
    s . y > 1e-10 |s| |y|.

    `w0` and `penalties` are [P, m] (a penalty of 0 leaves a coordinate free: the intercept).  `evaluate(W)` takes the
    [P, m] array of every problem's current trial point and returns (loss [P], grad [P, m]) of the unpenalised terms; it
    is called once per round for all problems, a finished problem frozen at its result (its pair is ignored).  Every
    problem is its own state machine on its own 1-D arrays: its trajectory depends on its own evaluations alone, so with
    an evaluator that keeps problems apart it returns the same bits alone and in any list.

    A problem stops when max |grad f_p| <= tol (0 iterations if the start satisfies it), after `max_iter` accepted steps
    (ConvergenceWarning; the `max_iter`-th iterate is returned) or when a line search fails (ConvergenceWarning).
    Returns (W [P, m], n_iter int [P], converged bool [P])."""
    w0 = np.asarray(w0, dtype=np.float64)
    lam = np.broadcast_to(np.asarray(penalties, dtype=np.float64), w0.shape)
    if w0.ndim != 2:
        raise ValueError("lbfgs_lockstep: w0 [problems, parameters] expected")
    if int(max_iter) < 0 or int(history) < 1 or not float(tol) >= 0.0:
        raise ValueError("lbfgs_lockstep: max_iter >= 0, history >= 1 and tol >= 0 required")
    if np.any(lam < 0.0):
        raise ValueError("lbfgs_lockstep: penalties >= 0 required")
    probs = [_Problem(w0[p], lam[p], tol, max_iter, history) for p in range(w0.shape[0])]
    while not all(p.done for p in probs):
        trial = np.stack([p.trial() for p in probs])
        loss, grad = evaluate(trial)
        loss, grad = np.asarray(loss, dtype=np.float64), np.asarray(grad, dtype=np.float64)
        for i, p in enumerate(probs):
            p.feed(loss[i], grad[i])
    late = [i for i, p in enumerate(probs) if not p.converged]
    if late:
        warnings.warn(f"lbfgs_lockstep: problem(s) {late} stopped before max |grad| <= tol = {tol:g} "
                      f"(max_iter = {max_iter}): increase max_iter or scale the features.", ConvergenceWarning)
    return (np.stack([p.x for p in probs]), np.array([p.n_iter for p in probs], dtype=np.int64),
            np.array([p.converged for p in probs], dtype=bool))


# ------------------------------------------------------------------------------------------------ kernel wrappers


def _prep(x):
    """x (device tensor or numpy) as contiguous float32 [n, ld] on the device, ld = d rounded up to a multiple of 4, and d
    (mixture._prep's rule).  Shapes are checked before the device is."""
    import torch

    from ._lib import require_gpu

    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        if x.dim() == 2 and torch.cuda.is_available():
            x = x.cuda()
    if x.dim() != 2:
        raise ValueError("expected [n_samples, n_features]")
    n, d = int(x.shape[0]), int(x.shape[1])
    if n < 1 or d < 1:
        raise ValueError("at least one row and one feature expected")
    if d > MAX_FEATURES:
        raise ValueError(f"at most {MAX_FEATURES} features ({d} given): reduce the matrix first")
    if n > 1 << 24:
        raise ValueError(f"at most {1 << 24} rows ({n} given)")
    require_gpu(x)
    x = x.float()
    if d % 4:
        x = torch.nn.functional.pad(x, (0, 4 - d % 4))
    return x.contiguous(), d


def _residual(xp, d: int, w, mode: int, classes: int, y=None, sw=None, pos_weight=None, want_z: bool = False):
    """wm_logreg_residual on the padded rows xp [n, ld]: w float64 [cols, d + 1] on the device; y int32 [n] (mode 0) or
    int8 [n, classes] (mode 1) or None (prediction).  Returns (resid [n, cols], loss [problems] or None, z or None)."""
    import torch

    from . import _lib
    from ._lib import check, ptr, require_gpu, stream_ptr, workspace

    n, ld = xp.shape
    require_gpu(xp, w, y, sw, pos_weight)
    if w.dim() != 2 or w.shape[1] != d + 1 or w.dtype != torch.float64:
        raise ValueError(f"logreg residual: w float64 [cols, {d + 1}] expected")
    cols = int(w.shape[0])
    if mode not in (0, 1) or classes < 1 or cols % classes:
        raise ValueError("logreg residual: mode 0 / 1 and cols a multiple of classes expected")
    if y is not None:
        want = (torch.int32, (n,)) if mode == 0 else (torch.int8, (n, classes))
        if y.dtype != want[0] or tuple(y.shape) != want[1]:
            raise ValueError(f"logreg residual: y {want[0]} {want[1]} expected")
    if sw is not None and (sw.dtype != torch.float64 or tuple(sw.shape) != (n,)):
        raise ValueError("logreg residual: sample weights float64 [n] expected")
    if pos_weight is not None and (mode != 1 or pos_weight.dtype != torch.float64 or tuple(pos_weight.shape) != (classes,)):
        raise ValueError("logreg residual: pos_weight float64 [labels] in mode 1 expected")
    lib = _lib.load()
    need = lib.wm_logreg_residual_workspace_bytes(n, d, ld, cols, mode, classes)
    ws = workspace(need, f"logreg residual n={n} d={d} cols={cols}: unsupported sizes (at most {MAX_COLUMNS} columns = "
                         "values of C x classes per call)", xp.device)
    resid = torch.empty((n, cols), dtype=torch.float64, device=xp.device)
    problems = cols // classes if mode == 0 else cols
    loss = torch.empty(problems, dtype=torch.float64, device=xp.device) if y is not None else None
    z = torch.empty((n, cols), dtype=torch.float64, device=xp.device) if want_z else None
    check(lib.wm_logreg_residual(ptr(xp), n, d, ld, ptr(w), cols, mode, classes, ptr(y), ptr(sw), ptr(pos_weight), ptr(resid),
                                 ptr(loss), ptr(z), ptr(ws), need, stream_ptr()), "wm_logreg_residual")
    return resid, loss, z


def _gradient(xp, d: int, resid):
    """grad float64 [cols, d + 1] = resid^T [x | 1] (wm_logreg_gradient)."""
    import torch

    from . import _lib
    from ._lib import check, ptr, require_gpu, stream_ptr, workspace

    n, ld = xp.shape
    require_gpu(xp, resid)
    if resid.dim() != 2 or resid.shape[0] != n or resid.dtype != torch.float64:
        raise ValueError("logreg gradient: resid float64 [n_samples, cols] expected")
    cols = int(resid.shape[1])
    lib = _lib.load()
    need = lib.wm_logreg_gradient_workspace_bytes(n, d, ld, cols)
    ws = workspace(need, f"logreg gradient n={n} d={d} cols={cols}: unsupported sizes", xp.device)
    grad = torch.empty((cols, d + 1), dtype=torch.float64, device=xp.device)
    check(lib.wm_logreg_gradient(ptr(xp), n, d, ld, ptr(resid), cols, ptr(grad), ptr(ws), need, stream_ptr()),
          "wm_logreg_gradient")
    return grad


def _device_evaluator(spec):
    """spec -> evaluate(w float64 [cols, d + 1] numpy) -> (loss [problems], grad [cols, d + 1]) numpy float64, the raw sums
    of the two kernels: two launches and one copy each way per call.  spec["x"] is the padded device matrix of _prep."""
    import torch

    xp, d, mode, classes = spec["x"], spec["d"], spec["mode"], spec["classes"]
    dev = xp.device
    y = torch.from_numpy(spec["y"]).to(dev)
    sw = None if spec["sw"] is None else torch.from_numpy(np.ascontiguousarray(spec["sw"], dtype=np.float64)).to(dev)
    pw = None if spec["pos_weight"] is None else torch.from_numpy(np.ascontiguousarray(spec["pos_weight"], dtype=np.float64)).to(dev)

    def evaluate(w):
        resid, loss, _ = _residual(xp, d, torch.from_numpy(w).to(dev), mode, classes, y, sw, pw)
        return loss.cpu().numpy(), _gradient(xp, d, resid).cpu().numpy()

    return evaluate


# ------------------------------------------------------------------------------------------------ host rules


def _c_list(c) -> Tuple[np.ndarray, bool]:
    many = not np.isscalar(c)
    arr = np.atleast_1d(np.asarray(c, dtype=np.float64))
    if arr.ndim != 1 or arr.size < 1 or not np.all(np.isfinite(arr)) or np.any(arr <= 0.0):
        raise ValueError("C: a positive number or a non-empty list of positive numbers expected")
    return arr, many


def balanced_class_weight(y_index: np.ndarray, n_classes: int, sample_weight: Optional[np.ndarray] = None) -> np.ndarray:
    """sklearn's compute_class_weight("balanced"): sum of the (weighted) counts / (n_classes * (weighted) count), over the
    labelled rows (y_index >= 0)."""
    keep = y_index >= 0
    w = None if sample_weight is None else np.asarray(sample_weight, dtype=np.float64)[keep]
    counts = np.bincount(y_index[keep], weights=w, minlength=n_classes).astype(np.float64)
    if np.any(counts <= 0.0):
        raise ValueError("class_weight='balanced': every class needs a row of positive weight")
    return counts.sum() / (n_classes * counts)


def _host_rows(a, dtype):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=dtype)


def _check_common(tol, max_iter):
    if not float(tol) >= 0.0:
        raise ValueError("tol >= 0 required")
    if int(max_iter) < 1:
        raise ValueError("max_iter >= 1 required")


# ------------------------------------------------------------------------------------------------ the estimators


class LogisticRegression:
    """sklearn.linear_model.LogisticRegression(penalty="l2", solver="lbfgs") on device rows, for one C or a list of C in
    one solve.

    fit(x, y, sample_weight=None): y integer labels [n], -1 = unlabelled (weight 0, not counted in S); `classes_` the
    sorted distinct labels (they need not be 0 .. K - 1).  Two classes become ONE sigmoid column, `coef_` [1, d] and
    `intercept_` [1] with sklearn's sign (positive = classes_[1]); K >= 3 classes the multinomial problem, `coef_` [K, d],
    `intercept_` [K].  class_weight: None, "balanced" or {label: weight}.  With a list of C: `coef_` [n_C, K, d],
    `intercept_` [n_C, K], `n_iter_` [n_C], `C_` [n_C], and `model[i]` / `model.best(scores)` give the single-C model.
    `decision_function` and `predict_proba` return float64 device tensors ([n, K], or [n] for the two-class
    decision_function, as sklearn), `predict` numpy labels (a tie goes to the lowest class) and `score` the accuracy."""

    def __init__(self, C=1.0, *, fit_intercept: bool = True, class_weight=None, tol: float = 1e-4, max_iter: int = 100):
        self.C_, self._many = _c_list(C)
        _check_common(tol, max_iter)
        if not (class_weight is None or class_weight == "balanced" or isinstance(class_weight, dict)):
            raise ValueError("class_weight: None, 'balanced' or a dict expected")
        self.C, self.fit_intercept, self.class_weight = C, bool(fit_intercept), class_weight
        self.tol, self.max_iter = float(tol), int(max_iter)

    # ---- host rules, usable without a device

    def _targets(self, y, sample_weight, n: int):
        """(classes, y_index int32 with -1 kept, s float64 [n], S)."""
        y = _host_rows(y, np.int64)
        if y.shape != (n,):
            raise ValueError(f"y: integer labels [{n}] expected, shape {y.shape} given")
        lab = y != -1
        classes = np.unique(y[lab])
        if classes.size < 2:
            raise ValueError("LogisticRegression needs at least 2 classes among the labelled rows")
        idx = np.full(n, -1, dtype=np.int32)
        idx[lab] = np.searchsorted(classes, y[lab]).astype(np.int32)
        sw = None
        if sample_weight is not None:
            sw = _host_rows(sample_weight, np.float64)
            if sw.shape != (n,) or not np.all(np.isfinite(sw)) or np.any(sw < 0.0):
                raise ValueError(f"sample_weight: non-negative float [{n}] expected")
        s = np.ones(n, dtype=np.float64) if sw is None else sw.copy()
        if self.class_weight == "balanced":
            cw = balanced_class_weight(idx, classes.size, sw)
        elif isinstance(self.class_weight, dict):
            unknown = set(self.class_weight) - set(classes.tolist())
            if unknown:
                raise ValueError(f"class_weight: label(s) {sorted(unknown)} are not among the classes {classes.tolist()}")
            cw = np.array([float(self.class_weight.get(c, 1.0)) for c in classes.tolist()])
        else:
            cw = None
        if cw is not None:
            s[lab] *= cw[idx[lab]]
        s[~lab] = 0.0
        total = float(s.sum())
        if not total > 0.0:
            raise ValueError("the weights of the labelled rows sum to 0")
        return classes, idx, s, total

    def _penalties(self, k_cols: int, d: int, total: float) -> np.ndarray:
        lam = np.zeros((self.C_.size, k_cols, d + 1))
        lam[:, :, :d] = (1.0 / (self.C_ * total))[:, None, None]
        return lam.reshape(self.C_.size, -1)

    def _solve(self, evaluate, k_cols: int, d: int, total: float):
        w0 = np.zeros((self.C_.size, k_cols * (d + 1)))
        return lbfgs_lockstep(evaluate, w0, self._penalties(k_cols, d, total), self.tol, self.max_iter)

    def _store(self, w, n_iter, converged, classes, d: int):
        w = w.reshape(self.C_.size, -1, d + 1)
        self.classes_, self.n_features_in_ = classes, d
        self.coef_, self.intercept_ = np.ascontiguousarray(w[:, :, :d]), np.ascontiguousarray(w[:, :, d])
        self.n_iter_, self.converged_ = n_iter, converged
        if not self._many:
            self.coef_, self.intercept_, self.n_iter_, self.converged_ = self.coef_[0], self.intercept_[0], n_iter[:1], converged[:1]
        return self

    # ---- fitting

    def fit(self, x, y, sample_weight=None, *, evaluator=None) -> "LogisticRegression":
        """`evaluator`: a factory spec -> evaluate that replaces the device kernels (`_device_evaluator` by default; the
        CPU tests pass a numpy one and numpy rows).  spec: dict(x, n, d, mode, classes, cols, y, sw, pos_weight)."""
        if evaluator is None:
            x, d = _prep(x)
            n = int(x.shape[0])
        else:
            n, d = (int(v) for v in np.shape(x))
        classes, idx, s, total = self._targets(y, sample_weight, n)
        k, p = int(classes.size), self.C_.size
        if k == 2:  # one sigmoid column per C; an unlabelled row has s = 0 and the label 0
            spec = dict(mode=1, classes=1, y=np.ascontiguousarray((idx == 1).astype(np.int8)[:, None]))
            k_cols = 1
        else:
            spec = dict(mode=0, classes=k, y=idx)
            k_cols = k
        if p * k_cols > MAX_COLUMNS:
            raise ValueError(f"{p} values of C x {k_cols} columns exceed {MAX_COLUMNS} columns per solve: split the list")
        spec.update(x=x, n=n, d=d, cols=p * k_cols, sw=s, pos_weight=None)
        raw = (evaluator or _device_evaluator)(spec)
        fit_intercept = self.fit_intercept

        def evaluate(w_flat):
            loss, grad = raw(np.ascontiguousarray(w_flat.reshape(p * k_cols, d + 1)))
            if not fit_intercept:
                grad[:, d] = 0.0
            return loss / total, grad.reshape(p, -1) / total

        w, n_iter, converged = self._solve(evaluate, k_cols, d, total)
        return self._store(w, n_iter, converged, classes, d)

    # ---- one C of a list

    def __len__(self):
        return self.C_.size

    def __getitem__(self, i: int) -> "LogisticRegression":
        """The fitted model of C_[i] alone (its attributes without the leading axis)."""
        self._fitted()
        if not self._many:
            raise TypeError("this model was fitted for a single C")
        i = int(i)
        one = LogisticRegression(float(self.C_[i]), fit_intercept=self.fit_intercept, class_weight=self.class_weight, tol=self.tol,
                                 max_iter=self.max_iter)
        one.classes_, one.n_features_in_ = self.classes_, self.n_features_in_
        one.coef_, one.intercept_ = self.coef_[i], self.intercept_[i]
        one.n_iter_, one.converged_ = self.n_iter_[i:i + 1], self.converged_[i:i + 1]
        return one

    def best(self, scores) -> "LogisticRegression":
        """model[argmax(scores)], scores one number per C (the first maximum wins a tie: the smallest such C index)."""
        scores = np.asarray(scores, dtype=np.float64)
        if scores.shape != (self.C_.size,):
            raise ValueError(f"best: one score per C expected ({self.C_.size})")
        return self[int(np.argmax(scores))]

    # ---- the fitted model on any rows

    def _fitted(self):
        if not hasattr(self, "coef_"):
            raise RuntimeError(f"{type(self).__name__}: call fit first")

    def _single(self):
        self._fitted()
        if self._many:
            raise TypeError("fitted for a list of C: select one with model[i] or model.best(scores) first")

    def _forward(self, x):
        """(probabilities [n, cols], logits [n, cols]) of the single-C model, device tensors."""
        import torch

        self._single()
        xp, d = _prep(x)
        if d != self.n_features_in_:
            raise ValueError(f"[n_samples, {self.n_features_in_}] expected")
        w = torch.from_numpy(np.ascontiguousarray(np.concatenate([self.coef_, self.intercept_[:, None]], axis=1))).to(xp.device)
        binary = self.classes_.size == 2
        proba, _, z = _residual(xp, d, w, 1 if binary else 0, 1 if binary else int(self.classes_.size), want_z=True)
        return proba, z

    def decision_function(self, x):
        z = self._forward(x)[1]
        return z[:, 0].contiguous() if self.classes_.size == 2 else z

    def predict_proba(self, x):
        import torch

        p = self._forward(x)[0]
        return torch.cat([1.0 - p, p], dim=1) if self.classes_.size == 2 else p

    def predict(self, x) -> np.ndarray:
        z = self._forward(x)[1].cpu().numpy()
        if self.classes_.size == 2:
            return self.classes_[(z[:, 0] > 0.0).astype(np.int64)]
        return self.classes_[np.argmax(z, axis=1)]  # (the first maximum: a tie goes to the lowest class)

    def score(self, x, y) -> float:
        y = _host_rows(y, np.int64)
        keep = y != -1
        return float((self.predict(x)[keep] == y[keep]).mean())


class MultilabelLogisticRegression:
    """One independent sigmoid problem per (C, label) on y [n, L] of 0 / 1: what
    sklearn.multiclass.OneVsRestClassifier(LogisticRegression(C)) fits, all of them in one solve.

    pos_weight: None, "balanced" (models.evals.pos_weight_from_labels' rule: negative / positive frequency per label) or
    an array [L]: the weight of a label's positive rows (BCEWithLogitsLoss' pos_weight; the same as sklearn's
    sample_weight = where(y == 1, pos_weight, 1) for that label).  S is per label: the sum of those weights.
    `coef_` [L, d], `intercept_` [L], `n_iter_` [L] (with a list of C: a leading axis, `model[i]` / `best(scores)`);
    `predict_proba` float64 device tensor [n, L], `predict` int8 numpy [n, L] at threshold 0.5 (logit > 0)."""

    def __init__(self, C=1.0, *, pos_weight=None, fit_intercept: bool = True, tol: float = 1e-4, max_iter: int = 100):
        self.C_, self._many = _c_list(C)
        _check_common(tol, max_iter)
        if isinstance(pos_weight, str) and pos_weight != "balanced":
            raise ValueError("pos_weight: None, 'balanced' or an array [labels] expected")
        self.C, self.pos_weight, self.fit_intercept = C, pos_weight, bool(fit_intercept)
        self.tol, self.max_iter = float(tol), int(max_iter)

    def _targets(self, y, sample_weight, n: int):
        """(y int8 [n, L], pos_weight float64 [L] or None, s [n] or None, S float64 [L])."""
        y = _host_rows(y, np.int64)
        if y.ndim != 2 or y.shape[0] != n or y.shape[1] < 1 or not np.isin(y, (0, 1)).all():
            raise ValueError(f"y: 0 / 1 labels [{n}, n_labels] expected")
        n_labels = y.shape[1]
        if self.pos_weight is None:
            pw = None
        elif isinstance(self.pos_weight, str):
            pos = y.sum(axis=0) / float(n)
            if np.any(pos == 0):
                raise ValueError(f"pos_weight='balanced': label(s) {np.flatnonzero(pos == 0).tolist()} have no positive row")
            pw = (1.0 - pos) / pos
        else:
            pw = _host_rows(self.pos_weight, np.float64)
            if pw.shape != (n_labels,) or not np.all(np.isfinite(pw)) or np.any(pw < 0.0):
                raise ValueError(f"pos_weight: non-negative float [{n_labels}] expected")
        s = None
        if sample_weight is not None:
            s = _host_rows(sample_weight, np.float64)
            if s.shape != (n,) or not np.all(np.isfinite(s)) or np.any(s < 0.0):
                raise ValueError(f"sample_weight: non-negative float [{n}] expected")
        rows = np.ones(n) if s is None else s
        a = np.ones((n, n_labels)) if pw is None else np.where(y == 1, pw[None, :], 1.0)
        total = (rows[:, None] * a).sum(axis=0)
        if np.any(total <= 0.0):
            raise ValueError("the weights of a label sum to 0")
        return y.astype(np.int8), pw, s, total

    def fit(self, x, y, sample_weight=None, *, evaluator=None) -> "MultilabelLogisticRegression":
        """`evaluator`: as LogisticRegression.fit's."""
        if evaluator is None:
            x, d = _prep(x)
            n = int(x.shape[0])
        else:
            n, d = (int(v) for v in np.shape(x))
        y8, pw, s, total = self._targets(y, sample_weight, n)
        n_labels, p = y8.shape[1], self.C_.size
        if p * n_labels > MAX_COLUMNS:
            raise ValueError(f"{p} values of C x {n_labels} labels exceed {MAX_COLUMNS} columns per solve: split the list")
        raw = (evaluator or _device_evaluator)(dict(x=x, n=n, d=d, mode=1, classes=n_labels, cols=p * n_labels,
                                                    y=np.ascontiguousarray(y8), sw=s, pos_weight=pw))
        scale = np.tile(total, p)  # column g * L + l belongs to label l
        fit_intercept = self.fit_intercept

        def evaluate(w_flat):
            loss, grad = raw(np.ascontiguousarray(w_flat))
            if not fit_intercept:
                grad[:, d] = 0.0
            return loss / scale, grad / scale[:, None]

        lam = np.zeros((p * n_labels, d + 1))
        lam[:, :d] = (1.0 / (np.repeat(self.C_, n_labels) * scale))[:, None]
        w, n_iter, converged = lbfgs_lockstep(evaluate, np.zeros((p * n_labels, d + 1)), lam, self.tol, self.max_iter)
        w = w.reshape(p, n_labels, d + 1)
        self.n_features_in_, self.n_labels_ = d, n_labels
        self.coef_, self.intercept_ = np.ascontiguousarray(w[:, :, :d]), np.ascontiguousarray(w[:, :, d])
        self.n_iter_, self.converged_ = n_iter.reshape(p, n_labels), converged.reshape(p, n_labels)
        if not self._many:
            self.coef_, self.intercept_, self.n_iter_, self.converged_ = (self.coef_[0], self.intercept_[0], self.n_iter_[0],
                                                                         self.converged_[0])
        return self

    def __len__(self):
        return self.C_.size

    def __getitem__(self, i: int) -> "MultilabelLogisticRegression":
        if not hasattr(self, "coef_"):
            raise RuntimeError("MultilabelLogisticRegression: call fit first")
        if not self._many:
            raise TypeError("this model was fitted for a single C")
        i = int(i)
        one = MultilabelLogisticRegression(float(self.C_[i]), pos_weight=self.pos_weight, fit_intercept=self.fit_intercept,
                                           tol=self.tol, max_iter=self.max_iter)
        one.n_features_in_, one.n_labels_ = self.n_features_in_, self.n_labels_
        one.coef_, one.intercept_, one.n_iter_, one.converged_ = self.coef_[i], self.intercept_[i], self.n_iter_[i], self.converged_[i]
        return one

    def best(self, scores) -> "MultilabelLogisticRegression":
        scores = np.asarray(scores, dtype=np.float64)
        if scores.shape != (self.C_.size,):
            raise ValueError(f"best: one score per C expected ({self.C_.size})")
        return self[int(np.argmax(scores))]

    def _forward(self, x):
        import torch

        if not hasattr(self, "coef_"):
            raise RuntimeError("MultilabelLogisticRegression: call fit first")
        if self._many:
            raise TypeError("fitted for a list of C: select one with model[i] or model.best(scores) first")
        xp, d = _prep(x)
        if d != self.n_features_in_:
            raise ValueError(f"[n_samples, {self.n_features_in_}] expected")
        w = torch.from_numpy(np.ascontiguousarray(np.concatenate([self.coef_, self.intercept_[:, None]], axis=1))).to(xp.device)
        proba, _, z = _residual(xp, d, w, 1, self.n_labels_, want_z=True)
        return proba, z

    def decision_function(self, x):
        return self._forward(x)[1]

    def predict_proba(self, x):
        return self._forward(x)[0]

    def predict(self, x) -> np.ndarray:
        return (self._forward(x)[1].cpu().numpy() > 0.0).astype(np.int8)
