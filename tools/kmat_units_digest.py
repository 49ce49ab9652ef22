#!/usr/bin/env python3
"""One line per call with a digest of what it returned, over every entry that reaches the
kernel-matrix units (pygp_amd/csrc/kmat.hip, kgrad.hip, kderiv.hip): input widths on both sides
of the 8 / 16 / 32 instances, ragged sizes that span tile edges, every kernel family. Run it from
two trees (it imports the package of the tree it lies in) on the same device: the outputs must
not differ. The last line counts the arrays and the doubles.
usage: kmat_units_digest.py > out.txt"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pygp_amd import _lib, kernels as K

WIDTHS = (1, 8, 9, 16, 17, 32)
N1, N2, MS = 129, 70, (4, 130)
LSN, MEAN = np.log(0.1), 0.2
count = [0, 0]


def dig(*arrays):                                   # as tools/jitter_check.py
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()[:16]


def families(d):
    ell = 0.5 * np.sqrt(d) * (1.0 + 0.1 * np.arange(d))
    out = [('se_iso', K.SE(1.1, 0.6 * np.sqrt(d), ndim=d)), ('se_ard', K.SE(1.1, ell)),
           ('matern3', K.Matern(0.9, ell, d=3)), ('matern5', K.Matern(1.2, ell, d=5)),
           ('rq', K.RQ(1.1, ell, 1.5)), ('sum', K.SE(0.8, ell) + K.Matern(0.6, 1.3 * ell, d=5)),
           ('product', K.SE(1.1, 1.5 * ell) * K.RQ(0.9, 2.0 * ell, 2.0))]
    if d == 1:
        out.append(('periodic', K.Periodic(1.1, 0.8, 0.7)))
    return out


def put(tag, call):
    try:
        res = call()
    except Exception as e:                           # a refusal is a result too
        print('%-44s refused: %s' % (tag, str(e).split('\n')[0][:80]), flush=True)
        return
    arrays = [np.asarray(a, dtype=np.float64) for a in (res if isinstance(res, tuple) else (res,))]
    count[0] += len(arrays)
    count[1] += sum(a.size for a in arrays)
    print('%-44s %s %d' % (tag, dig(*arrays), sum(a.size for a in arrays)), flush=True)


h = _lib.Handle(0)
for d in WIDTHS:
    rng = np.random.RandomState(1000 + d)
    X, X2 = rng.rand(N1, d), rng.rand(N2, d)
    Xs = {m: rng.rand(m, d) for m in MS}
    y = np.sin(3 * X.sum(axis=1)) + 0.1 * rng.randn(N1)
    Y3 = np.c_[y, np.cos(2 * X[:, 0]), y * y]
    labels = np.where(y > np.median(y), 1.0, -1.0)
    V = rng.randn(N1, 3)
    ng = 9
    Xg, G = rng.rand(ng, d), rng.randn(ng, d)
    Xnew, ynew = rng.rand(5, d), rng.randn(5)
    for name, k in families(d):
        spec, hyp, nh = k._kspec(), k.get_hyper(), k.nhyper
        t = lambda what: 'd=%-2d %-8s %s' % (d, name, what)
        thetas = np.array([np.r_[LSN, hyp, MEAN], np.r_[LSN, hyp, MEAN] + 0.1 * np.cos(np.arange(nh + 2))])
        # the kernel entries
        put(t('kernel_get f64'), lambda: h.kernel_get(spec, X, X2))
        put(t('kernel_get f64 square'), lambda: h.kernel_get(spec, X))
        put(t('kernel_get f32'), lambda: h.kernel_get(spec, X, X2, dtype=np.float32))
        put(t('kernel_grad'), lambda: h.kernel_grad(spec, X, X2))
        put(t('kernel_gradx wrt 1'), lambda: h.kernel_gradx(spec, X, X2, wrt=1))
        put(t('kernel_gradx wrt 2'), lambda: h.kernel_gradx(spec, X, X2, wrt=2))
        put(t('kernel_gradxy'), lambda: h.kernel_gradxy(spec, X2, X2[:33]))
        put(t('kernel_matvec'), lambda: h.kernel_matvec(spec, X, V))
        # ExactGP and the member-batched group
        h.set_data(X, y)
        put(t('select_pivots'), lambda: h.select_pivots(spec, X, 20))
        put(t('exact_eval grad'), lambda: h.exact_eval(spec, LSN, MEAN, True))
        put(t('exact_update'), lambda: (h.exact_update(spec, LSN, MEAN), h.exact_loglik(nh, True))[1])
        for m in MS:
            put(t('exact_posterior_grad m=%d' % m), lambda: h.exact_posterior_grad(Xs[m]))
            put(t('exact_posterior_gradient m=%d' % m), lambda: h.exact_posterior_gradient(Xs[m]))
        put(t('exact_append'), lambda: (float(h.exact_append(Xnew, ynew)),) + h.exact_posterior_grad(Xs[4]))
        h.set_data(X, y)
        put(t('loglik_batch grad'), lambda: h.loglik_batch(spec, thetas, grad=True))
        put(t('posterior_batch grad'), lambda: h.posterior_batch(spec, thetas, Xs[4], grad=True))

        def multiout():                              # MultiOutputGP, T = 3
            h.mo_set_data(X, Y3)
            h.mo_update(spec, LSN, MEAN)
            return h.mo_loglik(nh, True) + h.mo_posterior(Xs[130])

        def gradobs():                               # GradientGP: 40 values and 9 gradients
            h.gradobs_set_data(X[:40], y[:40], Xg, G)
            h.gradobs_update(spec, LSN, 0.05, MEAN)
            return (h.gradobs_loglik(),) + h.gradobs_posterior(Xs[130])

        def sparse(method):                          # 70 pseudo-inputs, with their gradients
            h.sparse_update(spec, method, X2, LSN, MEAN)
            return (h.sparse_loglik(nh, True) + h.sparse_loglik_pseudo(nh, N2, d)
                    + h.sparse_posterior(Xs[4], grad=True))

        def laplace():                               # LaplaceGP, Probit
            h.laplace_set_data(X, labels)
            steps = h.laplace_update(spec, 2, MEAN)
            return ((float(steps),) + h.laplace_loglik(nh, True) + h.laplace_posterior(Xs[130])
                    + h.laplace_get_mode(N1))

        put(t('multiout'), multiout)
        put(t('gradobs'), gradobs)
        h.set_data(X, y)
        for mname, method in (('fitc', _lib.GPX_FITC), ('dtc', _lib.GPX_DTC), ('vfe', _lib.GPX_VFE)):
            put(t(mname), lambda: sparse(method))
        put(t('laplace'), laplace)
h.close()
print('%d arrays, %d doubles' % tuple(count))
