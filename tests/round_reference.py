"""The comparator of the rounding tests: a numpy restatement of the definitions in include/sdplr_hip_round.h.  It is
neither the code under test nor ``rounding.py`` (whose projection is a BLAS GEMV of unknown summation order):

  * projection  z_it = R_i0·γ_0t, then z = z + R_ik·γ_kt for k = 1 … r−1 — one rounding per multiply and per add;
  * mode 0      x = −1 where z < 0, else +1;
  * mode 1      ``np.argsort(z_t + 0.0, kind="stable")``: the first ⌊n/2⌋ get +1, the rest −1;
  * cuts        the weights of the stored edges i < j with x_i ≠ x_j, added up (exactly, where the weights are ±1).
"""
import numpy as np
import scipy.sparse as sp


def edges_of(A):
    """(I, J, W) of the entries i < j of a sparse matrix, or of an (I, J, W) triple."""
    if isinstance(A, tuple):
        I, J, W = (np.asarray(a) for a in A)
    else:
        co = sp.coo_matrix(A)
        I, J, W = co.row, co.col, co.data
    keep = I < J
    return I[keep].astype(np.int64), J[keep].astype(np.int64), W[keep].astype(np.float64)


def project(R, gauss):
    """z (n, T) of R (n, r) and gauss (T, r)."""
    R, gauss = np.asarray(R, dtype=np.float64), np.asarray(gauss, dtype=np.float64)
    z = R[:, 0, None] * gauss[None, :, 0]
    for k in range(1, R.shape[1]):
        z = z + R[:, k, None] * gauss[None, :, k]
    return z


def labels_of(z, mode):
    """int8 (T, n)."""
    n, T = z.shape
    if mode == 0:
        return np.where(z < 0, -1, 1).astype(np.int8).T.copy()
    out = np.full((T, n), -1, dtype=np.int8)
    for t in range(T):
        perm = np.argsort(z[:, t] + 0.0, kind="stable")
        out[t, perm[: n // 2]] = 1
    return out


def cuts_of(labels, edges):
    I, J, W = edges
    out = np.zeros(labels.shape[0])
    if I.size == 0:
        return out
    for t in range(labels.shape[0]):
        x = labels[t]
        out[t] = float(np.sum(W[x[I] != x[J]]))
    return out


def rounding(R, gauss, A, mode):
    """→ dict(z, labels (T, n), cuts (T,), best, x_best)."""
    z = project(R, gauss)
    lab = labels_of(z, mode)
    cuts = cuts_of(lab, edges_of(A))
    best = int(np.argmax(cuts)) if mode == 0 else int(np.argmin(cuts))     # (both return the first of equals)
    return dict(z=z, labels=lab, cuts=cuts, best=best, x_best=lab[best].copy())


def random_graph(n, E, rng, weights="pm1"):
    """E distinct edges i < j on n vertices (fewer when the graph has no room), weights ±1 (Gset) or uniform in (0, 1);
    given with BOTH triangles, in random order, as an (I, J, W) triple."""
    room = n * (n - 1) // 2
    E = min(E, room)
    if E == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy(), np.zeros(0)
    if room <= 4 * E:
        iu, ju = np.triu_indices(n, 1)
        pick = rng.choice(room, size=E, replace=False)
        I, J = iu[pick], ju[pick]
    else:
        got = set()
        while len(got) < E:
            a = rng.integers(0, n, size=2 * (E - len(got)) + 8)
            b = rng.integers(0, n, size=a.size)
            for i, j in zip(a, b):
                if i != j and len(got) < E:
                    got.add((min(i, j), max(i, j)))
        I, J = (np.array(v, dtype=np.int64) for v in zip(*sorted(got)))
    W = rng.choice([-1.0, 1.0], size=E) if weights == "pm1" else rng.uniform(2.0 ** -20, 1.0, size=E)
    order = rng.permutation(2 * E)
    return np.concatenate([I, J])[order], np.concatenate([J, I])[order], np.concatenate([W, W])[order]
