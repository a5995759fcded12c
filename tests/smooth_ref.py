"""Correct and Smooth restated in numpy float64, with the derived rounding bounds of csl_prop_f32: the
reference of tests/test_smooth_cpu.py and tests/test_gpu_smooth.py.  No device, no cslicer import.

    S = D^-1/2 A D^-1/2 over the neighbour CSR (self loops removed, duplicates counted), dinv the FLOAT32 numbers the
    device holds (1 / sqrt(deg) computed in float64 and rounded once; 0 for a row without neighbours)
    prop(X0, alpha, T, lo, hi, fix):  X = X0;  T times:  X = clamp(alpha S X + (1 - alpha) X0, lo, hi), X[rows] = values
"""
import numpy as np

U32 = 2.0 ** -24                       # unit roundoff of float32
TINY = float(np.finfo(np.float32).tiny)   # the smallest normal: what a flushed or gradually underflowed result may lose


def gamma(n):
    """n roundings: gamma(n) = n u / (1 - n u)"""
    n = np.asarray(n, dtype=np.float64)
    return n * U32 / (1.0 - n * U32)


def neighbour_csr(indptr, indices):
    """(indptr int64, indices int64) without self loops, duplicates and order kept"""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n = indptr.shape[0] - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    keep = indices != rows
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=ip[1:])
    return ip, indices[keep]


def dinv32(indptr):
    deg = np.diff(np.asarray(indptr, dtype=np.int64)).astype(np.float64)
    return np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0).astype(np.float32)


def _row_sums(G, lens):
    """sums of consecutive groups of `lens` rows of G [sum(lens), W] (float64), zero for an empty group"""
    out = np.zeros((lens.shape[0], G.shape[1]), dtype=np.float64)
    ne = lens > 0
    if ne.any():
        starts = (np.cumsum(lens) - lens)[ne]
        out[ne] = np.add.reduceat(G, starts, axis=0)
    return out


def _edges_of(indptr, rows):
    """(edge positions of the CSR rows `rows`, one after the other; their lengths)"""
    lens = indptr[rows + 1] - indptr[rows]
    first = np.cumsum(lens) - lens
    return np.repeat(indptr[rows] - first, lens) + np.arange(int(lens.sum()), dtype=np.int64), lens


def _clamp(y, lo, hi):
    return np.where(y < lo, lo, np.where(y > hi, hi, y))          # (as the kernel: a NaN stays)


def step(indptr, indices, rows, xs, ldx, W, dinv, alpha, base, ldb, beta, lo, hi):
    """One csl_prop_f32 call in float64 on the ABI's flat buffers.  rows: the graph row of every output position; xs: flat,
    row u at u * ldx; base: flat by position (or None), row k at k * ldb.  Returns (y, y_s, bound_y, bound_s), [n, W]
    each: what `out` and `out_s` should hold and how far a correct float32 kernel may be from them.

    The bound.  alpha and beta reach the kernel as float32 (one rounding each of the caller's doubles).  The kernel then
    rounds: the row sum of d terms d - 1 times, alpha * dinv[v] once, its product with the sum once, the fused multiply-add
    of the base term once.  That is d + 3 roundings on the gathered term and 2 on the base term, so
        |y32 - y| <= gamma(d + 3) (|alpha| dinv[v] sum_u |xs[u, j]| + |beta base[k, j]|) + TINY
    the clamp being 1-Lipschitz (lo and hi are taken as float32 numbers: nothing here covers rounding them).  out_s is one
    more product: |s32 - dinv[v] y| <= dinv[v] bound_y + u dinv[v] (|y| + bound_y) + TINY."""
    indptr, rows = np.asarray(indptr, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    n = rows.shape[0]
    X = np.asarray(xs, dtype=np.float64).reshape(-1)
    e, lens = _edges_of(indptr, rows)
    src = np.asarray(indices, dtype=np.int64)[e]
    G = X[src[:, None] * ldx + np.arange(W)[None, :]] if e.shape[0] else np.zeros((0, W))
    acc, mag = _row_sums(G, lens), _row_sums(np.abs(G), lens)
    dv = np.asarray(dinv, dtype=np.float64)[rows][:, None]
    y = alpha * dv * acc
    mag = abs(alpha) * dv * mag
    if base is not None:
        b = np.asarray(base, dtype=np.float64).reshape(-1)[np.arange(n)[:, None] * ldb + np.arange(W)[None, :]]
        y = y + beta * b
        mag = mag + np.abs(beta * b)
    y = _clamp(y, lo, hi)
    by = gamma(lens + 3)[:, None] * mag + TINY
    bs = dv * by + U32 * dv * (np.abs(y) + by) + TINY
    return y, dv * y, by, bs


def prop(indptr, indices, x0, alpha, T, lo, hi, fix=None, bounds=False):
    """prop of the module docstring on a neighbour CSR, float64.  bounds=True: also the list of the T one-step bound
    matrices B_t on the float64 iterate, in X units: the step's bound_y plus the rounding u |X_{t+1}| of the pre-scaled
    operand it hands on (and, as B_-1 in front, u |X0| for the first operand's)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    N, W = x0.shape
    dv = dinv32(indptr).astype(np.float64)
    rows = np.arange(N, dtype=np.int64)
    x0 = np.asarray(x0, dtype=np.float64)
    x, beta = x0.copy(), 1.0 - alpha
    B = [U32 * np.abs(x0)]
    for _ in range(T):
        x, _, by, _ = step(indptr, indices, rows, (dv[:, None] * x).reshape(-1), W, W, dv, alpha,
                           None if alpha == 1.0 else x0.reshape(-1), W, beta, lo, hi)
        if fix is not None:
            x[fix[0]] = fix[1]
        B.append(by + U32 * np.abs(x))
    return (x, B) if bounds else x


def softmax(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def autoscale_factors(sigma, e):
    """s_v = sigma / ||e_v||_1; what is not finite or exceeds 1000 becomes 1.  Returns (s, the raw quotient)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = sigma / np.abs(e).sum(1)
    s = raw.copy()
    s[~np.isfinite(s) | (s > 1000.0)] = 1.0
    return s, raw


def correct_and_smooth(logits, indptr, indices, train, labels, T1=50, a1=0.8, T2=50, a2=0.8, autoscale=True, scale=1.0):
    """{"out": the smoothed [N, C] matrix, "raw_scale": the autoscale quotients before the rule (None for a fixed scale)}
    on a neighbour CSR, float64"""
    P = softmax(logits)
    N, C = P.shape
    train, labels = np.asarray(train, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    Y = np.zeros((train.shape[0], C))
    Y[np.arange(train.shape[0]), labels] = 1.0
    E0 = np.zeros_like(P)
    E0[train] = Y - P[train]
    raw = None
    if autoscale:
        E = prop(indptr, indices, E0, a1, T1, -1.0, 1.0)
        sigma = np.abs(E0[train]).sum() / max(train.shape[0], 1)
        s, raw = autoscale_factors(sigma, E)
        P2 = P + s[:, None] * E
    else:
        E = prop(indptr, indices, E0, a1, T1, -np.inf, np.inf, fix=(train, E0[train]))
        P2 = P + scale * E
    P2[train] = Y
    return {"out": prop(indptr, indices, P2, a2, T2, 0.0, 1.0), "raw_scale": raw}


def label_propagation(indptr, indices, n_classes, train, labels, alpha=0.8, T=50):
    Y = np.zeros((np.asarray(indptr).shape[0] - 1, n_classes))
    Y[np.asarray(train, dtype=np.int64), np.asarray(labels, dtype=np.int64)] = 1.0
    return prop(indptr, indices, Y, alpha, T, 0.0, 1.0)


def margins(out):
    """the gap between every row's two largest entries (inf for a single column)"""
    if out.shape[1] < 2:
        return np.full(out.shape[0], np.inf)
    top = np.sort(out, axis=1)
    return top[:, -1] - top[:, -2]


def planted(n=3000, C=7, seed=0):
    """The planted-partition inputs of both test files: a symmetric stochastic block model with about 6 intra-class and 3
    random edges per node (duplicates and a few self loops left in the raw CSR), logits 1.6 onehot + 1.5 N(0, 1), half the
    nodes labelled.  Returns a dict: raw CSR (indptr, indices), classes, logits float32, train / test node ids."""
    rng = np.random.default_rng(1000 * C + seed)
    cls = rng.integers(0, C, n)
    order = np.argsort(cls, kind="stable")
    first = np.searchsorted(cls[order], np.arange(C + 1))
    size = np.maximum(first[1:] - first[:-1], 1)
    v = np.repeat(np.arange(n), 3)
    mate = order[np.minimum(first[cls[v]] + (rng.random(v.shape[0]) * size[cls[v]]).astype(np.int64), n - 1)]
    w = np.arange(n)[rng.random(n) < 0.5]
    a = np.concatenate([v, np.arange(n), w])
    b = np.concatenate([mate, rng.integers(0, n, n), rng.integers(0, n, w.shape[0])])
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])          # both directions: symmetric
    o = np.argsort(dst, kind="stable")
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=indptr[1:])
    onehot = np.zeros((n, C))
    onehot[np.arange(n), cls] = 1.0
    logits = (1.6 * onehot + 1.5 * rng.standard_normal((n, C))).astype(np.float32)
    perm = rng.permutation(n)
    return {"indptr": indptr, "indices": src[o].astype(np.int64), "cls": cls, "logits": logits, "C": C, "n": n,
            "train": np.sort(perm[:n // 2]), "test": np.sort(perm[n // 2:])}
