"""csl_gemm_f32 and csl_sum_slabs_f32 (include/cslicer_aggr.h, csrc/gemm_lt.hip) restated in float64 over the flat buffers
the C ABI reads: row-major, leading dimensions and batch strides in elements.  No project code, no GPU.

    C[b][i, j] = act( sum_l op(A[b])[i, l] op(B[b])[l, j] + bias[j] )      i < m, j < n, b < batch
    op(A) = A ([m, k], lda) or A^T (A stored [k, m], lda);  op(B) = B ([k, n], ldb) or B^T (B stored [n, k], ldb)
    X[b] starts stride_x elements behind X[b - 1]; every element of the C buffer no C[b] owns keeps its value

gemm() returns the WHOLE C buffer, so that "untouched" is part of the same comparison as the product; bound() returns the
worst-case fp32 error of every owned element (0 for the others: they must keep their bits).

The bound.  An fp32 dot product of k terms plus one bias add, in ANY order of summation (a chain, a tree, split-K, fused
multiply-adds or separate roundings), makes at most k + 1 roundings on the path of any term, so (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., section 3.1)

    |computed - exact| <= gamma(k + 1) (sum_l |a_il| |b_lj| + |bias_j|),    gamma(q) = q u / (1 - q u),  u = 2^-24.

ReLU is 1-Lipschitz and exact, so the bound carries over.  It is derived, not measured: a solution that computes in a
narrower format (u = 2^-11 or 2^-8) or drops a term exceeds it by orders of magnitude.
"""
import numpy as np

U = 2.0 ** -24


def gamma(q):
    return q * U / (1.0 - q * U)


def _mat(flat, off, rows, cols, ld):
    """rows x cols view of the flat float64 array: element (i, j) at off + i * ld + j; the view must lie inside it"""
    if rows == 0 or cols == 0:
        return np.zeros((rows, cols), dtype=np.float64)
    if off < 0 or ld < cols or off + (rows - 1) * ld + cols > flat.shape[0]:
        raise ValueError("a %d x %d matrix (ld %d) at %d does not lie inside a buffer of %d" % (rows, cols, ld, off, flat.shape[0]))
    return np.lib.stride_tricks.as_strided(flat[off:], shape=(rows, cols), strides=(ld * 8, 8), writeable=True)


def _f64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))


def _operands(transa, transb, m, n, k, A, lda, sa, B, ldb, sb, batch):
    """op(A[b]) [m, k] and op(B[b]) [k, n] of every batch, float64"""
    A, B = (_f64(A), _f64(B)) if k else (None, None)
    for b in range(batch):
        if k == 0:
            yield np.zeros((m, 0)), np.zeros((0, n))
            continue
        a = _mat(A, b * sa, k, m, lda).T if transa else _mat(A, b * sa, m, k, lda)
        bb = _mat(B, b * sb, n, k, ldb).T if transb else _mat(B, b * sb, k, n, ldb)
        yield a, bb


def gemm(transa, transb, m, n, k, A, lda, sa, B, ldb, sb, C0, ldc, sc, batch, bias=None, relu=False):
    """the whole flat C buffer after the call, float64: owned elements computed, every other one carried over from C0"""
    out = _f64(C0).copy()
    bv = None if bias is None else _f64(bias)[:n]
    for b, (a, bb) in enumerate(_operands(transa, transb, m, n, k, A, lda, sa, B, ldb, sb, batch)):
        c = a @ bb
        if bv is not None:
            c = c + bv[None, :]
        if relu:
            c = np.maximum(c, 0.0)
        _mat(out, b * sc, m, n, ldc)[...] = c
    return out


def bound(transa, transb, m, n, k, A, lda, sa, B, ldb, sb, C0, ldc, sc, batch, bias=None, relu=False):
    """per element of the flat C buffer: gamma(k + 1) (sum_l |a_il| |b_lj| + |bias_j|) where owned, 0 elsewhere"""
    out = np.zeros(_f64(C0).shape[0], dtype=np.float64)
    bv = None if bias is None else np.abs(_f64(bias)[:n])
    for b, (a, bb) in enumerate(_operands(transa, transb, m, n, k, A, lda, sa, B, ldb, sb, batch)):
        c = np.abs(a) @ np.abs(bb)
        if bv is not None:
            c = c + bv[None, :]
        _mat(out, b * sc, m, n, ldc)[...] = gamma(k + 1) * c
    return out


def owned(m, n, ldc, sc, batch, size):
    """boolean mask over a flat C buffer of `size` elements: the elements some C[b] owns"""
    mask = np.zeros(size, dtype=np.float64)
    for b in range(batch):
        _mat(mask, b * sc, m, n, ldc)[...] = 1.0
    return mask != 0


def bucket(transa, m, k):
    """the size bucket a shape's long dimension is blanked to in its class (and in a recorded plan's line): the rows m
    of a forward / input-gradient GEMM -- 1: fewer than 1024, 2: 1024..4095, 0: 4096 and more --, the reduction length k
    of a weight gradient (transa) -- 1: fewer than 1024, 0: 1024 and more"""
    if transa:
        return 1 if k < 1024 else 0
    return 1 if m < 1024 else (2 if m < 4096 else 0)


def sum_slabs(slabs, n, n_slabs):
    """out[c] = sum_b slabs[b * n + c], float64"""
    return _f64(slabs)[:n * n_slabs].reshape(n_slabs, n).sum(axis=0)


def sum_slabs_bound(slabs, n, n_slabs):
    """n_slabs values are summed with n_slabs - 1 roundings at the most on any path (the kernel's first add is to an exact
    zero), in any order: gamma(n_slabs - 1) sum_b |v_b|"""
    return gamma(n_slabs - 1) * np.abs(_f64(slabs)[:n * n_slabs].reshape(n_slabs, n)).sum(axis=0)


def slabbed_bound(slab_ref, slab_bound, n, n_slabs):
    """the two stages together, against the float64 product of the whole matrices: computed slabs s_b = r_b + e_b with
    |e_b| <= beta_b (bound()), their computed sum = sum_b s_b (1 + t_b) with |t_b| <= gamma(n_slabs - 1):
        |out - sum_b r_b| <= sum_b beta_b + gamma(n_slabs - 1) sum_b (|r_b| + beta_b)"""
    r = np.abs(_f64(slab_ref)[:n * n_slabs].reshape(n_slabs, n))
    beta = _f64(slab_bound)[:n * n_slabs].reshape(n_slabs, n)
    return beta.sum(axis=0) + gamma(n_slabs - 1) * (r + beta).sum(axis=0)
