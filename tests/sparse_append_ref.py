"""Host statement of the recurrence behind SparseGP.append_data, in
NumPy on the oracle's kernel functions, written from the equations and not from the device
code. L = chol(Kuu + su2 I) does not depend on the data, the columns of V0, ell, rt and V of a
point depend on L and that point alone, and everything else the model is made of is a sum
over columns:

    S   = I + V V^T        (p x p)        g   = V rt        (p)
    sum log ell     sum rt^2     sum 1 / ell^2     sum V^2     t = sum (kxx - |V0_j|^2)

`Sums` keeps them; `append` adds the share of new rows, old + new; `finish` turns them into
what the one-shot references of tests/sparse_ref.py and tests/sparse_vfe_ref.py return for
the concatenated data: lZ, the stored factors F1 (FITC _L, DTC/VFE _Ruu), F2 = A L (_R /
_Rux), v (_b = beta / _a = sn2 beta) and VFE's t."""

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as orc
import sparse_ref as sr

FITC, DTC, VFE = 1, 2, 3


class Sums(object):
    """The state an append needs: hypers, U and L, and the sums over the columns so far."""

    def __init__(self, spec, method, theta, U):
        self.method = method
        self.sp = sr._with_hyper(spec, theta)
        self.mean = theta[-1]
        self.sn2 = np.exp(2 * theta[0])
        # FITC divides, DTC and VFE multiply: the two forms are not bitwise equal
        self.su2 = self.sn2 / 1e6 if method == FITC else self.sn2 * 1e-6
        self.U = np.array(U, dtype=float)
        p = self.U.shape[0]
        self.L = sla.cholesky(orc.kernel_get(self.sp, self.U) + self.su2 * np.eye(p))
        self.n = 0
        self.S = np.eye(p)             # "A just needs to be initialized at the identity"
        self.g = np.zeros(p)
        self.logell = self.rt2 = self.iell2 = self.v2 = self.t = 0.0

    def append(self, X, y):
        """The columns of the rows X, y from L alone, added to the sums."""
        V0 = sla.solve_triangular(self.L, orc.kernel_get(self.sp, self.U, X), trans=True)
        resid = orc.kernel_dget(self.sp, X) - np.sum(V0 ** 2, axis=0)
        if self.method == FITC:
            ell = np.sqrt(resid + self.sn2)
        else:
            ell = np.full(X.shape[0], np.sqrt(self.sn2))
        V = V0 / ell
        rt = (y - self.mean) / ell
        self.S = self.S + V.dot(V.T)
        self.g = self.g + V.dot(rt)
        self.logell = self.logell + np.sum(np.log(ell))
        self.rt2 = self.rt2 + rt.dot(rt)
        self.iell2 = self.iell2 + np.sum(1 / ell ** 2)
        self.v2 = self.v2 + np.sum(V ** 2)
        if self.method == VFE:
            self.t = self.t + np.sum(resid)
        self.n += X.shape[0]
        return self

    def finish(self):
        """lZ, F1, F2, v and t of the model on every row appended so far."""
        A = sla.cholesky(self.S)
        beta = sla.solve_triangular(A, self.g, trans=True)
        lZ = -np.sum(np.log(np.diag(A))) - self.logell - 0.5 * (self.rt2 - beta.dot(beta)) - \
            0.5 * self.n * np.log(2 * np.pi)
        if self.method == VFE:
            lZ = lZ - self.t / (2 * self.sn2)
        v = beta if self.method == FITC else self.sn2 * beta
        return dict(lZ=lZ, F1=self.L, F2=A.dot(self.L), v=v, t=self.t, A=A, beta=beta)


def run(spec, method, theta, U, pieces):
    """The recurrence over pieces = [(X, y), ...]: the result of finish() after each."""
    sums = Sums(spec, method, theta, U)
    return [sums.append(X, y).finish() for X, y in pieces]
