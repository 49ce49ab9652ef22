"""The C entries that ask what a handle holds (require_state in pygp_amd/csrc/gpx_handle.hip), each
with valid arguments: the one table of the refusal tests (helpers.assert_refused)."""

import ctypes as C

import numpy as np

from pygp_amd import _lib


def handle_calls(h, spec, theta, X, y, Xs):
    """{family: {entry: callable returning the entry's code}} on the handle h; the families are
    'plain', 'gradobs', 'mo' and 'laplace'. spec: the kernel; theta = [log sn, its hypers, mean];
    X (n, d), y (n,) and Xs (m, d) feed the entries that take points."""
    ptr, k = _lib._ptr, spec.ref()
    (n, d), m, sn, mean = X.shape, len(Xs), float(theta[0]), float(theta[-1])
    lZ, info, cnt, ms = C.c_double(0), C.c_int(0), C.c_int64(0), C.c_double(0)
    b = [np.zeros(max(n * n, m * m * d, 1024)) for _ in range(4)]
    idx, plan = np.zeros(4, dtype=np.int64), (C.c_int * 64)()
    X2, y2, U, th = X[:2].copy(), y[:2].copy(), X[:4].copy(), np.array(theta)
    post, inf, plZ = (ptr(Xs), m, ptr(b[0]), ptr(b[1])), C.byref(info), C.byref(lZ)
    rows = {'plain': {                              # entry: its arguments behind the handle
        'gpx_kernel_build_resident': (k, _lib.F64, 1, C.byref(ms)),
        'gpx_exact_update': (k, sn, mean, inf),
        'gpx_exact_loglik': (plZ, None),
        'gpx_exact_loglik dlZ': (plZ, ptr(b[0])),
        'gpx_exact_eval': (k, sn, mean, 1, plZ, ptr(b[0]), inf),
        'gpx_exact_append': (ptr(X2), ptr(y2), 2, inf),
        'gpx_exact_loo': (plZ, None, None, None),
        'gpx_exact_posterior': post,
        'gpx_exact_posterior_grad': post + (ptr(b[2]), ptr(b[3])),
        'gpx_exact_posterior_full': post,
        'gpx_exact_posterior_gradient': post,
        'gpx_exact_get_factor': (n, ptr(b[0]), ptr(b[1])),
        'gpx_batch_plan': (4, 0, plan),
        'gpx_loglik_batch': (k, ptr(th), 1, 0, ptr(b[0]), None, None),
        'gpx_posterior_batch': (k, ptr(th), 1) + post + (None, None, None),
        'gpx_sparse_update': (k, _lib.GPX_DTC, ptr(U), 4, sn, mean, inf),
        'gpx_sparse_append': (ptr(X2), ptr(y2), 2, inf),
        'gpx_select_pivots': (k, None, n, d, 4, 0.0, ptr(idx), None, None, C.byref(cnt)),
    }, 'gradobs': {
        'gpx_gradobs_update': (k, sn, 0.05, mean, inf),
        'gpx_gradobs_loglik': (plZ,),
        'gpx_gradobs_posterior': post,
        'gpx_gradobs_posterior_full': post,
    }, 'mo': {
        'gpx_mo_update': (k, sn, mean, inf),
        'gpx_mo_loglik': (plZ, None),
        'gpx_mo_loglik dlZ': (plZ, ptr(b[0])),
        'gpx_mo_posterior': post,
        'gpx_mo_posterior_full': post,
    }, 'laplace': {
        'gpx_laplace_update': (k, 2, mean, 1e-8, 50, 0, inf, inf),
        'gpx_laplace_loglik': (plZ, None),
        'gpx_laplace_loglik dlZ': (plZ, ptr(b[0])),
        'gpx_laplace_posterior': post,
        'gpx_laplace_posterior_full': post,
        'gpx_laplace_get_mode': (n, ptr(b[0]), ptr(b[1])),
    }}
    keep = (spec, b, idx, plan, X2, y2, U, th, Xs, lZ, info, cnt, ms)   # alive with the callables
    return {fam: {name: (lambda f=getattr(h._L, name.split()[0]), a=args, keep=keep: f(h._h, *a))
                  for name, args in entries.items()} for fam, entries in rows.items()}
