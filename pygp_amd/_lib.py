"""
ctypes binding of libgpx.so (include/gpx.h). This is the only place the Python
side touches native code; there is no CPU fallback: if the library or an
MI355X is missing, the product path raises.
"""

import ctypes as C
import os
import threading

import numpy as np

__all__ = ['lib', 'Handle', 'default_handle', 'kspec_of', 'GpxError', 'device_count',
           'loglik_batch_multi', 'batch_partition',
           'KIND_SE', 'KIND_MATERN', 'KIND_PERIODIC', 'KIND_SUM', 'KIND_RQ', 'KIND_PRODUCT',
           'F64',
           'F32']

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.path.join(_HERE, 'libgpx.so')

KIND_SE = 1
KIND_MATERN = {1: 2, 3: 3, 5: 4}
KIND_PERIODIC = 5
KIND_SUM = 6
KIND_RQ = 7
KIND_PRODUCT = 8
F64, F32 = 0, 1
NTIMERS = 11


class GpxError(RuntimeError):
    pass


class _KSpec(C.Structure):
    pass


_KSpec._fields_ = [
    ('kind', C.c_int32), ('iso', C.c_int32), ('ndim', C.c_int32),
    ('nhyper', C.c_int32), ('hyper', C.POINTER(C.c_double)),
    ('nparts', C.c_int32), ('parts', C.POINTER(_KSpec)),
]

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_vp = C.c_void_p
_i64 = C.c_int64

# name -> (restype, argtypes); mirrors include/gpx.h one to one
GPX_FITC, GPX_DTC, GPX_VFE = 1, 2, 3          # enum gpx_sparse_method
GPX_SPARSE_MAX_P = 4096


class _GemmExArgs(C.Structure):
    """gpx_gemm_ex_args of include/gpx.h."""
    _INTS1 = ('ta', 'tb', 'M', 'N', 'K', 'lda', 'ldb', 'ldc')
    _INTS2 = ('flags', 'tile', 'waves', 'order', 'swizzle', 'use_lists', 'kshift', 'beta0_from',
              'batch', 'strideA', 'strideB', 'strideC', 'strideC2',
              'kchunk', 'nsplit', 'mstrideA', 'mstrideB', 'mstrideC',
              'offA', 'offB', 'offC', 'offC2', 'b_is_c')
    _fields_ = ([(n, _i64) for n in _INTS1] + [('alpha', C.c_double), ('beta', C.c_double)] +
                [(n, _i64) for n in _INTS2])


SIGNATURES = {
    'gpx_version': (C.c_int, []),
    'gpx_last_error': (C.c_char_p, []),
    'gpx_device_count': (C.c_int, [_ip]),
    'gpx_create': (C.c_int, [C.c_int, C.POINTER(_vp)]),
    'gpx_destroy': (C.c_int, [_vp]),
    'gpx_synchronize': (C.c_int, [_vp]),
    'gpx_kernel_get': (C.c_int, [_vp, C.POINTER(_KSpec), _vp, _i64, _vp, _i64,
                                 _i64, C.c_int, _vp]),
    'gpx_kernel_grad': (C.c_int, [_vp, C.POINTER(_KSpec), _vp, _i64, _vp, _i64,
                                  _i64, _vp]),
    'gpx_kernel_build_resident': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_int,
                                            C.c_int, _dp]),
    'gpx_set_data': (C.c_int, [_vp, _vp, _i64, _i64, _vp]),
    'gpx_exact_update': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_double,
                                   C.c_double, _ip]),
    'gpx_exact_append': (C.c_int, [_vp, _vp, _vp, _i64, _ip]),
    'gpx_exact_loglik': (C.c_int, [_vp, _dp, _vp]),
    'gpx_exact_loo': (C.c_int, [_vp, _dp, _vp, _vp, _vp]),
    'gpx_exact_eval': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_double, C.c_double,
                                 C.c_int, _dp, _vp, _ip]),
    'gpx_exact_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_exact_posterior_grad': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'gpx_exact_posterior_full': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_kernel_gradx': (C.c_int, [_vp, C.POINTER(_KSpec), _vp, _i64, _vp, _i64, _i64,
                                   C.c_int, _vp]),
    'gpx_kernel_gradxy': (C.c_int, [_vp, C.POINTER(_KSpec), _vp, _i64, _vp, _i64, _i64, _vp]),
    'gpx_exact_posterior_gradient': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_gradobs_set_data': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64]),
    'gpx_gradobs_update': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_double, C.c_double,
                                     C.c_double, _ip]),
    'gpx_gradobs_loglik': (C.c_int, [_vp, _dp]),
    'gpx_gradobs_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_gradobs_posterior_full': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_kernel_matvec': (C.c_int, [_vp, C.POINTER(_KSpec), _vp, _i64, _i64, _vp, _i64, _vp]),
    'gpx_laplace_set_data': (C.c_int, [_vp, _vp, _i64, _i64, _vp]),
    'gpx_laplace_update': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_int, C.c_double, C.c_double,
                                     C.c_int, C.c_int, _ip, _ip]),
    'gpx_laplace_loglik': (C.c_int, [_vp, _dp, _vp]),
    'gpx_laplace_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_laplace_posterior_full': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_laplace_get_mode': (C.c_int, [_vp, _i64, _vp, _vp]),
    'gpx_laplace_timings': (C.c_int, [_vp, _vp]),
    'gpx_softmax_set_data': (C.c_int, [_vp, _vp, _i64, _i64, _vp, C.c_int]),
    'gpx_softmax_update': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_double, C.c_int, _ip, _ip]),
    'gpx_softmax_loglik': (C.c_int, [_vp, _dp, _vp]),
    'gpx_softmax_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_softmax_get_mode': (C.c_int, [_vp, _i64, _vp, _vp]),
    'gpx_softmax_timings': (C.c_int, [_vp, _vp]),
    'gpx_ep_update': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_double, C.c_double, C.c_int,
                                C.c_double, _ip, _ip]),
    'gpx_ep_loglik': (C.c_int, [_vp, _dp, _vp]),
    'gpx_ep_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_ep_posterior_full': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_ep_get_sites': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    'gpx_ep_timings': (C.c_int, [_vp, _vp]),
    'gpx_mo_set_data': (C.c_int, [_vp, _vp, _i64, _vp, _i64, _i64]),
    'gpx_mo_update': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_double, C.c_double, _ip]),
    'gpx_mo_loglik': (C.c_int, [_vp, _dp, _vp]),
    'gpx_mo_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_mo_posterior_full': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_icm_set_data': (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64]),
    'gpx_icm_update': (C.c_int, [_vp, C.POINTER(_KSpec), _vp, _vp, _vp, _ip]),
    'gpx_icm_loglik': (C.c_int, [_vp, _dp, _vp]),
    'gpx_icm_posterior': (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    'gpx_icm_posterior_full': (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    'gpx_exact_get_factor': (C.c_int, [_vp, _i64, _vp, _vp]),
    'gpx_sparse_update': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_int, _vp, _i64, C.c_double,
                                    C.c_double, _ip]),
    'gpx_sparse_append': (C.c_int, [_vp, _vp, _vp, _i64, _ip]),
    'gpx_sparse_loglik': (C.c_int, [_vp, _vp, _vp]),
    'gpx_sparse_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'gpx_sparse_posterior_full': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_sparse_get_state': (C.c_int, [_vp, _vp, _vp, _vp]),
    'gpx_sparse_timings': (C.c_int, [_vp, _vp]),
    'gpx_sparse_loglik_pseudo': (C.c_int, [_vp, _vp, _vp, _vp]),
    'gpx_sparse_pseudo_timing': (C.c_int, [_vp, _vp]),
    'gpx_sparse_laplace_update': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_int, C.c_double, _vp,
                                            _i64, C.c_double, C.c_double, C.c_int, _ip, _ip]),
    'gpx_sparse_laplace_loglik': (C.c_int, [_vp, _dp, _vp]),
    'gpx_sparse_laplace_loglik_pseudo': (C.c_int, [_vp, _vp, _vp, _vp]),
    'gpx_sparse_laplace_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'gpx_sparse_laplace_posterior_full': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_sparse_laplace_get_mode': (C.c_int, [_vp, _vp, _vp, _vp]),
    'gpx_sparse_laplace_timings': (C.c_int, [_vp, _vp]),
    'gpx_sparse_ep_update': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_double, _vp, _i64, C.c_double,
                                       C.c_double, C.c_int, C.c_double, _ip, _ip]),
    'gpx_sparse_ep_loglik': (C.c_int, [_vp, _dp, _vp]),
    'gpx_sparse_ep_loglik_pseudo': (C.c_int, [_vp, _vp, _vp, _vp]),
    'gpx_sparse_ep_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'gpx_sparse_ep_posterior_full': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_sparse_ep_get_sites': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    'gpx_sparse_ep_timings': (C.c_int, [_vp, _vp]),
    'gpx_select_pivots': (C.c_int, [_vp, C.POINTER(_KSpec), _vp, _i64, _i64, _i64, C.c_double,
                                    _vp, _vp, _vp, C.POINTER(_i64)]),
    'gpx_select_timing': (C.c_int, [_vp, _vp]),
    'gpx_fourier_fit': (C.c_int, [_vp, _vp, _i64, _i64, _vp, C.c_double, C.c_double, C.c_double,
                                  _vp, _i64, _vp, _vp, _i64, _vp, _ip]),
    'gpx_fourier_set': (C.c_int, [_vp, _vp, _i64, _i64, _vp, C.c_double, C.c_double, _vp, _i64]),
    'gpx_fourier_eval': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_fourier_timings': (C.c_int, [_vp, _vp]),
    'gpx_path_fit': (C.c_int, [_vp, _vp, _i64, _i64, _vp, C.c_double, _vp, _vp, _i64, _i64, _vp,
                               _ip]),
    'gpx_path_set': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_double, _vp, _i64, _i64, _vp, _i64,
                               _vp, C.c_double, _vp, _vp, _i64]),
    'gpx_path_eval': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_path_timings': (C.c_int, [_vp, _vp]),
    'gpx_ssgp_update': (C.c_int, [_vp, _vp, _i64, _i64, _vp, C.c_double, C.c_double, C.c_double,
                                  _dp, _ip]),
    'gpx_ssgp_loglik': (C.c_int, [_vp, _dp, _vp, _vp, _vp, _vp]),
    'gpx_ssgp_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'gpx_ssgp_posterior_full': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_ssgp_get': (C.c_int, [_vp, _vp]),
    'gpx_ssgp_timings': (C.c_int, [_vp, _vp]),
    'gpx_iter_set_probes': (C.c_int, [_vp, _vp, _vp, _i64, _i64]),
    'gpx_iter_update': (C.c_int, [_vp, C.POINTER(_KSpec), C.c_double, C.c_double, _i64,
                                  C.c_double, _i64, C.POINTER(_i64), _ip]),
    'gpx_iter_loglik': (C.c_int, [_vp, _dp, _vp]),
    'gpx_iter_posterior': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_iter_posterior_full': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'gpx_iter_solve': (C.c_int, [_vp, _vp, _i64, _vp, C.POINTER(_i64)]),
    'gpx_iter_apply': (C.c_int, [_vp, _vp, _i64, _vp]),
    'gpx_iter_get': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dp]),
    'gpx_iter_timings': (C.c_int, [_vp, _vp]),
    'gpx_icache_build': (C.c_int, [_vp, _i64, C.POINTER(_i64)]),
    'gpx_icache_eval': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'gpx_icache_cross_apply': (C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp]),
    'gpx_icache_get': (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    'gpx_icache_timings': (C.c_int, [_vp, _vp]),
    'gpx_loglik_batch': (C.c_int, [_vp, C.POINTER(_KSpec), _vp, _i64, C.c_int,
                                   _vp, _vp, _vp]),
    'gpx_batch_plan': (C.c_int, [_vp, _i64, C.c_int, _ip]),
    'gpx_loglik_batch_multi': (C.c_int, [C.POINTER(_KSpec), _vp, _i64, _vp, _vp, _i64, _i64,
                                         C.c_int, C.c_int, _vp, _vp, _vp]),
    'gpx_posterior_batch_multi': (C.c_int, [C.POINTER(_KSpec), _vp, _i64, _vp, _vp, _i64, _i64,
                                            _vp, _i64, C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                                            _vp]),
    'gpx_batch_partition': (None, [_i64, C.c_int, C.c_int, C.POINTER(_i64),
                                   C.POINTER(_i64)]),
    'gpx_multi_slot': (_i64, [_i64, C.c_int]),
    'gpx_multi_comm_size': (C.c_int, []),
    'gpx_multi_pack': (C.c_int, [_vp, _i64, C.c_int, _i64, _vp]),
    'gpx_multi_scatter': (C.c_int, [_vp, _i64, C.c_int, C.c_int, _vp]),
    'gpx_posterior_batch': (C.c_int, [_vp, C.POINTER(_KSpec), _vp, _i64, _vp, _i64, _vp,
                                      _vp, _vp, _vp, _vp]),
    'gpx_enable_timing': (C.c_int, [_vp, C.c_int]),
    'gpx_get_timings': (C.c_int, [_vp, _vp, C.c_int]),
    'gpx_batch_timings': (C.c_int, [_vp, _dp, C.POINTER(_i64)]),
    'gpx_timing_name': (C.c_char_p, [C.c_int]),
    'gpx_la_gemm': (C.c_int, [_vp, C.c_int, C.c_int, _i64, _i64, _i64,
                              C.c_double, _vp, _i64, _vp, _i64, C.c_double, _vp,
                              _i64]),
    'gpx_set_safe_mode': (C.c_int, [_vp, C.c_int]),
    'gpx_get_safe_mode': (C.c_int, [_vp, _ip]),
    'gpx_multi_enable_timing': (C.c_int, [C.c_int, C.c_int]),
    'gpx_multi_batch_info': (C.c_int, [C.c_int, _i64, C.c_int, _dp, C.POINTER(_i64), _ip]),
    'gpx_panel_grid_check': (C.c_int, [C.c_int, C.c_int, _ip, _ip]),
    'gpx_panel_grid_rule': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip]),
    'gpx_la_gemm_ex': (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64]),
    'gpx_la_potrf': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _ip]),
    'gpx_la_gemm_bench': (C.c_int, [_vp, C.c_int, C.c_int, _i64, C.c_int, _dp]),
    'gpx_la_gemm_bench_ex': (C.c_int, [_vp, C.c_int, C.c_int, _i64, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       _dp]),
    'gpx_la_gemm_bench_mnk': (C.c_int, [_vp, C.c_int, C.c_int, _i64, _i64, _i64, C.c_int,
                                        C.c_double, C.c_int, C.c_int, _dp]),
    'gpx_la_potrf_bench': (C.c_int, [_vp, _i64, C.c_int, C.c_int, _dp]),
    'gpx_panel_graph_check': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    'gpx_panel_graph_check_wide': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    'gpx_panel_graph_check_rhs': (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    'gpx_panel_graph_check_full': (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    'gpx_panel_solo_check': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    'gpx_sweep_check': (C.c_int, [C.c_int, C.c_int]),
    'gpx_sweep_check_lite': (C.c_int, [C.c_int, C.c_int, C.c_int]),
}

_lib = None
_lock = threading.RLock()


def lib():
    """Load libgpx.so (once). Raises GpxError if it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(_LIBPATH):
                    raise GpxError(
                        'pygp_amd/libgpx.so is missing: build it with '
                        '`python -m pygp_amd.build` (there is no CPU fallback)')
                L = C.CDLL(_LIBPATH)
                for name, (res, args) in SIGNATURES.items():
                    f = getattr(L, name)
                    f.restype, f.argtypes = res, args
                _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _f64(a, ndim=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if ndim is not None and a.ndim != ndim:
        raise ValueError('expected a %d-d array' % ndim)
    return a


def _pair(X1, X2, dtype=np.float64):
    """The inputs of a kernel entry as (X1, n1, X2, n2, d); X2 None: X1 against itself."""
    X1 = np.ascontiguousarray(X1, dtype=dtype)
    if X1.ndim != 2:
        raise ValueError('expected a 2-d array')
    n1, d = X1.shape
    if X2 is None:
        return X1, n1, None, n1, d
    X2 = np.ascontiguousarray(X2, dtype=dtype)
    if X2.ndim != 2 or X2.shape[1] != d:
        raise ValueError('X1 and X2 have different dimensions')
    return X1, n1, X2, X2.shape[0], d


def check(code):
    """Map a C return code to the reference's exceptions: >0 is the LinAlgError
    scipy.linalg.cholesky raises at pygp/inference/exact.py:54."""
    if code == 0:
        return
    msg = lib().gpx_last_error().decode('utf-8', 'replace')
    if code > 0:
        raise np.linalg.LinAlgError(
            '%d-th leading minor of the array is not positive definite' % code)
    raise GpxError(msg or 'libgpx error %d' % code)


class KSpecHolder(object):
    """Owns the ctypes structs + hyper arrays of one kernel description."""

    def __init__(self, kind, iso, ndim, hyper=None, parts=()):
        self.parts = list(parts)
        self.hyper = None if hyper is None else _f64(np.atleast_1d(hyper))
        self.c = _KSpec()
        self.c.kind, self.c.iso, self.c.ndim = kind, int(bool(iso)), int(ndim)
        if self.parts:
            self.arr = (_KSpec * len(self.parts))(*[p.c for p in self.parts])
            self.c.nparts = len(self.parts)
            self.c.parts = C.cast(self.arr, C.POINTER(_KSpec))
            self.c.nhyper = sum(p.c.nhyper for p in self.parts)
            self.c.hyper = None
        else:
            self.c.nparts = 0
            self.c.parts = None
            self.c.nhyper = self.hyper.size
            self.c.hyper = self.hyper.ctypes.data_as(_dp)

    def ref(self):
        return C.byref(self.c)


def kspec_of(kernel):
    """Ask a pygp_amd kernel object for its C description."""
    return kernel._kspec()


def _serialised(method):
    """Calls on one handle must not interleave (include/gpx.h): ctypes drops the GIL
    during a call, so two Python threads sharing a handle -- the process-wide
    default handle behind Kernel.get() in particular -- take turns.

    A task-queue launch that runs into its wait bound ("... timed out waiting ...") is an
    ERROR by default: within one process the launches are ordered on the device, so the
    bound is only met when another process uses the same GPU -- or by a scheduling bug, which
    must not hide behind a retry. Only a handle made with auto_safe_mode=True (or
    GPX_AUTO_SAFE_MODE=1) switches to safe mode -- no kernel that waits for another
    workgroup; another order of arithmetic, same tolerances -- and repeats the call, once
    per handle, with a RuntimeWarning that carries the original error; `safe_mode` and
    `safe_mode_switches` on the handle say that it happened."""
    def call(self, *args, **kwargs):
        with self._lock:
            try:
                return method(self, *args, **kwargs)
            except GpxError as e:
                if 'timed out waiting' not in str(e) or not getattr(self, '_auto_safe', False) \
                        or getattr(self, 'safe_mode_switches', 0) or not getattr(self, '_h', None):
                    raise
                import warnings
                warnings.warn('pygp_amd: %s (is another process using this GPU?); this handle '
                              'continues in safe mode: same tolerances, not the same bits' % e,
                              RuntimeWarning)
                self.safe_mode_switches = 1
                check(self._L.gpx_set_safe_mode(self._h, 1))
                return method(self, *args, **kwargs)
    call.__name__ = method.__name__
    call.__doc__ = method.__doc__
    return call


class Handle(object):
    """One device context (gpx_t*): a GPU, a stream and its HBM buffers."""

    def __init__(self, device=None, auto_safe_mode=None):
        """auto_safe_mode: switch this handle to safe mode and repeat the call when a
        diagonal-block launch runs into its wait bound (see _serialised); default: the
        environment's GPX_AUTO_SAFE_MODE, else off -- the error is raised."""
        L = lib()
        if auto_safe_mode is None:
            auto_safe_mode = os.environ.get('GPX_AUTO_SAFE_MODE', '0') not in ('', '0')
        self._auto_safe = bool(auto_safe_mode)
        self.safe_mode_switches = 0          # automatic switches so far (0 or 1)
        if device is None:
            device = int(os.environ.get('GPX_DEVICE',
                                        os.environ.get('LOCAL_RANK', '0')))
            n = C.c_int(0)
            check(L.gpx_device_count(C.byref(n)))
            if n.value > 0:
                device %= n.value
        self.device = device
        h = _vp()
        check(L.gpx_create(device, C.byref(h)))
        self._h = h
        self._L = L
        self._lock = threading.RLock()

    @property
    def safe_mode(self):
        """True if the handle factors diagonal blocks by recursion (gpx_set_safe_mode: set by
        the caller, or by the automatic switch) -- another order of arithmetic."""
        on = C.c_int(0)
        check(self._L.gpx_get_safe_mode(self._h, C.byref(on)))
        return bool(on.value)

    def set_safe_mode(self, on=True):
        check(self._L.gpx_set_safe_mode(self._h, int(bool(on))))

    def close(self):
        if getattr(self, '_h', None):
            self._L.gpx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- what the families' result entries share; `entry` is the family's own C function --
    def _posterior(self, entry, Xs, full, lead=None):
        """Xs -> (mu, s2), or (mu, Sigma) when full; lead: the mean comes back from the
        device as (lead, m) and goes to the caller as (m, lead)."""
        Xs = _f64(Xs, 2)
        m = Xs.shape[0]
        mu = np.empty(m) if lead is None else np.empty((lead, m))
        cov = np.empty((m, m)) if full else np.empty(m)
        check(entry(self._h, _ptr(Xs), m, _ptr(mu), _ptr(cov)))
        return (mu if lead is None else np.ascontiguousarray(mu.T)), cov

    def _loglik(self, entry, ngrad, grad):
        """lZ, or (lZ, dlZ) with ngrad entries."""
        lZ = C.c_double(0)
        dlZ = np.empty(ngrad) if grad else None
        check(entry(self._h, C.byref(lZ), _ptr(dlZ)))
        return (lZ.value, dlZ) if grad else lZ.value

    def _append(self, entry, Xnew, ynew):
        Xnew, ynew = _f64(Xnew, 2), _f64(ynew, 1)
        if Xnew.shape[0] != ynew.shape[0]:
            raise ValueError('X and y disagree')
        info = C.c_int(0)
        code = entry(self._h, _ptr(Xnew), _ptr(ynew), Xnew.shape[0], C.byref(info))
        if code == -3:
            return False
        check(code)
        return True

    # -- kernels --
    def kernel_get(self, spec, X1, X2=None, dtype=np.float64):
        dt = F32 if np.dtype(dtype) == np.float32 else F64
        X1, n1, X2, n2, d = _pair(X1, X2, dtype)
        out = np.empty((n1, n2), dtype=dtype)
        if out.size == 0:
            return out
        check(self._L.gpx_kernel_get(self._h, spec.ref(), _ptr(X1), n1, _ptr(X2),
                                     n2, d, dt, _ptr(out)))
        return out

    def kernel_grad(self, spec, X1, X2=None):
        X1, n1, X2, n2, d = _pair(X1, X2)
        out = np.empty((spec.c.nhyper, n1, n2))
        if out.size == 0:
            return out
        check(self._L.gpx_kernel_grad(self._h, spec.ref(), _ptr(X1), n1, _ptr(X2),
                                      n2, d, _ptr(out)))
        return out

    def kernel_matvec(self, spec, X, V):
        """K(X, X) V for V (n,) or (n, nv <= 4), without storing K."""
        X, V = _f64(X, 2), _f64(V)
        flat = V.ndim == 1
        V2 = np.ascontiguousarray(V.reshape(len(V), -1))
        if V2.ndim != 2 or V2.shape[0] != X.shape[0] or not 1 <= V2.shape[1] <= 4:
            raise ValueError('V must have a row per point and one to four columns')
        out = np.empty_like(V2)
        if out.size:
            check(self._L.gpx_kernel_matvec(self._h, spec.ref(), _ptr(X), X.shape[0], X.shape[1],
                                            _ptr(V2), V2.shape[1], _ptr(out)))
        return out[:, 0] if flat else out

    def kernel_build_resident(self, spec, dtype=np.float64, reps=5):
        ms = C.c_double(0)
        dt = F32 if np.dtype(dtype) == np.float32 else F64
        check(self._L.gpx_kernel_build_resident(self._h, spec.ref(), dt, reps,
                                                C.byref(ms)))
        return ms.value

    # -- exact GP --
    def set_data(self, X, y):
        X, y = _f64(X, 2), _f64(y, 1)
        if X.shape[0] != y.shape[0]:
            raise ValueError('X and y disagree')
        check(self._L.gpx_set_data(self._h, _ptr(X), X.shape[0], X.shape[1],
                                   _ptr(y)))
        self._data_shape = X.shape
        self._iter_cache_rank = 0

    def exact_update(self, spec, log_sn, mean):
        info = C.c_int(0)
        check(self._L.gpx_exact_update(self._h, spec.ref(), float(log_sn),
                                       float(mean), C.byref(info)))

    def exact_append(self, Xnew, ynew):
        """True if the factor was extended in place, False if the caller has to
        refactorise (the points do not fit / nothing to extend)."""
        return self._append(self._L.gpx_exact_append, Xnew, ynew)

    def exact_loglik(self, nhyper_kernel, grad=False):
        return self._loglik(self._L.gpx_exact_loglik, nhyper_kernel + 2, grad)

    def exact_loo(self, nhyper_kernel, n, grad=False, points=False):
        """Leave-one-out log predictive probability L of the last update; grad: (L, dL);
        points: (mu, s2), the n leave-one-out predictive means and variances, instead."""
        if points:
            mu, s2 = np.empty(n), np.empty(n)
            check(self._L.gpx_exact_loo(self._h, None, None, _ptr(mu), _ptr(s2)))
            return mu, s2
        L = C.c_double(0)
        dL = np.empty(nhyper_kernel + 2) if grad else None
        check(self._L.gpx_exact_loo(self._h, C.byref(L), _ptr(dL), None, None))
        return (L.value, dL) if grad else L.value

    def exact_eval(self, spec, log_sn, mean, grad=True):
        lZ, info = C.c_double(0), C.c_int(0)
        dlZ = np.empty(spec.c.nhyper + 2) if grad else None
        check(self._L.gpx_exact_eval(self._h, spec.ref(), float(log_sn),
                                     float(mean), int(grad), C.byref(lZ),
                                     _ptr(dlZ), C.byref(info)))
        return (lZ.value, dlZ) if grad else lZ.value

    def exact_posterior(self, Xs):
        return self._posterior(self._L.gpx_exact_posterior, Xs, False)

    def exact_posterior_full(self, Xs):
        return self._posterior(self._L.gpx_exact_posterior_full, Xs, True)

    # -- exact GP with gradient observations --
    def gradobs_set_data(self, X, y, Xg, G):
        """n >= 0 function values y at X and ng >= 1 gradients G (ng, d) at Xg."""
        Xg, G = _f64(Xg, 2), _f64(G, 2)
        if G.shape != Xg.shape:
            raise ValueError('Xg and G disagree')
        n = 0 if X is None else len(X)
        if n:
            X, y = _f64(X, 2), _f64(y, 1)
            if X.shape[0] != y.shape[0] or X.shape[1] != Xg.shape[1]:
                raise ValueError('X, y and Xg disagree')
        else:
            X = y = None
        check(self._L.gpx_gradobs_set_data(self._h, _ptr(X), n, _ptr(y), _ptr(Xg), Xg.shape[0],
                                           _ptr(G), Xg.shape[1]))

    def gradobs_update(self, spec, log_sn, grad_noise, mean):
        info = C.c_int(0)
        check(self._L.gpx_gradobs_update(self._h, spec.ref(), float(log_sn), float(grad_noise),
                                         float(mean), C.byref(info)))

    def gradobs_loglik(self):
        lZ = C.c_double(0)
        check(self._L.gpx_gradobs_loglik(self._h, C.byref(lZ)))
        return lZ.value

    def gradobs_posterior(self, Xs):
        return self._posterior(self._L.gpx_gradobs_posterior, Xs, False)

    def gradobs_posterior_full(self, Xs):
        return self._posterior(self._L.gpx_gradobs_posterior_full, Xs, True)

    # -- binary classification by Laplace's approximation (LaplaceGP) --
    def laplace_set_data(self, X, y):
        """Labels y in {-1, +1} at X."""
        X, y = _f64(X, 2), _f64(y, 1)
        if X.shape[0] != y.shape[0]:
            raise ValueError('X and y disagree')
        check(self._L.gpx_laplace_set_data(self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(y)))

    def laplace_update(self, spec, lik, mean, tol=1e-8, max_iter=50, warm=False):
        """Newton's method to the mode; returns the number of steps."""
        iters, info = C.c_int(0), C.c_int(0)
        check(self._L.gpx_laplace_update(self._h, spec.ref(), int(lik), float(mean), float(tol),
                                         int(max_iter), int(bool(warm)), C.byref(iters),
                                         C.byref(info)))
        return iters.value

    def laplace_loglik(self, nhyper_kernel, grad=False):
        return self._loglik(self._L.gpx_laplace_loglik, nhyper_kernel + 1, grad)

    def laplace_posterior(self, Xs):
        return self._posterior(self._L.gpx_laplace_posterior, Xs, False)

    def laplace_posterior_full(self, Xs):
        return self._posterior(self._L.gpx_laplace_posterior_full, Xs, True)

    def laplace_get_mode(self, n):
        """(f, g): the mode and the gradient of log p(y | f) there."""
        f, g = np.empty(n), np.empty(n)
        check(self._L.gpx_laplace_get_mode(self._h, n, _ptr(f), _ptr(g)))
        return f, g

    def laplace_timings(self):
        """HIP-event ms of the last laplace_update (enable_timing): the whole update, then of
        its first Newton step the build + scaling, the factorisation, the two products with K
        and the solves."""
        ms = np.zeros(5)
        check(self._L.gpx_laplace_timings(self._h, _ptr(ms)))
        return dict(zip(('update', 'build_scale', 'factor', 'matvec', 'solve'), ms))

    # -- multi-class classification by Laplace's approximation (MulticlassLaplaceGP) --
    def softmax_set_data(self, X, labels, nclass):
        """Labels 0 .. nclass - 1 at X."""
        X = _f64(X, 2)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.ndim != 1 or X.shape[0] != labels.shape[0]:
            raise ValueError('X and the labels disagree')
        check(self._L.gpx_softmax_set_data(self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(labels),
                                           int(nclass)))

    def softmax_update(self, spec, tol=1e-8, max_iter=50):
        """Newton's method to the mode; returns the number of steps."""
        iters, info = C.c_int(0), C.c_int(0)
        check(self._L.gpx_softmax_update(self._h, spec.ref(), float(tol), int(max_iter),
                                         C.byref(iters), C.byref(info)))
        return iters.value

    def softmax_loglik(self, nhyper_kernel, grad=False):
        return self._loglik(self._L.gpx_softmax_loglik, nhyper_kernel, grad)

    def softmax_posterior(self, Xs, nclass):
        """(mu (m, C), Sigma (m, C, C)) of the latents at the rows of Xs."""
        Xs = _f64(Xs, 2)
        m = Xs.shape[0]
        mu, Sigma = np.empty((m, nclass)), np.empty((m, nclass, nclass))
        check(self._L.gpx_softmax_posterior(self._h, _ptr(Xs), m, _ptr(mu), _ptr(Sigma)))
        return mu, Sigma

    def softmax_get_mode(self, n, nclass):
        """(F, G), each (n, C): the mode and Y - Pi there."""
        F, G = np.empty((n, nclass)), np.empty((n, nclass))
        check(self._L.gpx_softmax_get_mode(self._h, n, _ptr(F), _ptr(G)))
        return F, G

    def softmax_timings(self):
        """HIP-event ms (enable_timing): the last softmax_update and its build of K, of its
        first Newton step the class blocks, the factor and inverse of sum_c E_c and the products
        and vector work; the last gradient; the last posterior call."""
        ms = np.zeros(7)
        check(self._L.gpx_softmax_timings(self._h, _ptr(ms)))
        return dict(zip(('update', 'build', 'class_blocks', 'm_block', 'vectors', 'gradient',
                         'posterior'), ms))

    # -- binary classification by expectation propagation (EPGP); the labels come in through
    # laplace_set_data --
    def ep_update(self, spec, mean, tol=1e-10, max_iter=200, damping=0.8):
        """Damped parallel EP to a fixed point of the sites; returns the number of sweeps."""
        iters, info = C.c_int(0), C.c_int(0)
        check(self._L.gpx_ep_update(self._h, spec.ref(), float(mean), float(tol), int(max_iter),
                                    float(damping), C.byref(iters), C.byref(info)))
        return iters.value

    def ep_loglik(self, nhyper_kernel, grad=False):
        return self._loglik(self._L.gpx_ep_loglik, nhyper_kernel + 1, grad)

    def ep_posterior(self, Xs):
        return self._posterior(self._L.gpx_ep_posterior, Xs, False)

    def ep_posterior_full(self, Xs):
        return self._posterior(self._L.gpx_ep_posterior_full, Xs, True)

    def ep_get_sites(self, n):
        """(tau, nu, mu, s2): the sites and the marginals of the latent at the data."""
        out = [np.empty(n) for _ in range(4)]
        check(self._L.gpx_ep_get_sites(self._h, n, *[_ptr(a) for a in out]))
        return tuple(out)

    def ep_timings(self):
        """HIP-event ms of the last ep_update (enable_timing): the whole update, then of its
        first sweep the build + scaling, the factorisation, the two products with K, the solve
        and the row-norm and site passes."""
        ms = np.zeros(6)
        check(self._L.gpx_ep_timings(self._h, _ptr(ms)))
        return dict(zip(('update', 'build_scale', 'factor', 'matvec', 'solve', 'sites'), ms))

    # -- T outputs at the same inputs (MultiOutputGP) --
    def mo_set_data(self, X, Y):
        """X (n, d) and Y (n, T), 1 <= T <= 32."""
        X, Y = _f64(X, 2), _f64(Y, 2)
        if X.shape[0] != Y.shape[0]:
            raise ValueError('X and Y disagree')
        Yt = np.ascontiguousarray(Y.T)              # the C entry takes column t contiguous
        self._mo_T = Y.shape[1]
        check(self._L.gpx_mo_set_data(self._h, _ptr(X), X.shape[0], _ptr(Yt), Y.shape[1],
                                      X.shape[1]))

    def mo_update(self, spec, log_sn, mean):
        info = C.c_int(0)
        check(self._L.gpx_mo_update(self._h, spec.ref(), float(log_sn), float(mean),
                                    C.byref(info)))

    def mo_loglik(self, nhyper_kernel, grad=False):
        return self._loglik(self._L.gpx_mo_loglik, nhyper_kernel + 2, grad)

    def mo_posterior(self, Xs):
        return self._posterior(self._L.gpx_mo_posterior, Xs, False, self._mo_T)

    def mo_posterior_full(self, Xs):
        return self._posterior(self._L.gpx_mo_posterior_full, Xs, True, self._mo_T)

    # -- correlated outputs at their own inputs (CoregionalGP) --
    ICM_TMAX = 8                                     # GPX_ICM_TMAX

    def icm_set_data(self, X, y, task, T):
        """X (n, d), y (n,) and task (n,) ints in [0, T), 1 <= T <= 8."""
        X, y = _f64(X, 2), _f64(y, 1)
        task = np.ascontiguousarray(task, dtype=np.int32)
        if not X.shape[0] == y.shape[0] == task.shape[0] or task.ndim != 1:
            raise ValueError('X, y and task disagree')
        check(self._L.gpx_icm_set_data(self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(y),
                                       _ptr(task), int(T)))
        self._icm_T = int(T)

    def icm_update(self, spec, log_sn, B, mean):
        """log_sn (T,), B (T, T) symmetric, mean (T,)."""
        T = self._icm_T
        log_sn, B, mean = _f64(log_sn, 1), _f64(B, 2), _f64(mean, 1)
        if log_sn.shape != (T,) or B.shape != (T, T) or mean.shape != (T,):
            raise ValueError('log_sn, B and mean must have T = %d entries a side' % T)
        info = C.c_int(0)
        check(self._L.gpx_icm_update(self._h, spec.ref(), _ptr(log_sn), _ptr(B), _ptr(mean),
                                     C.byref(info)))

    def icm_loglik(self, nhyper_kernel, grad=False):
        """lZ, or (lZ, dlZ): dlZ = [noise (T) | kernel | S (T*T) | mean sums (T)]."""
        T = self._icm_T
        return self._loglik(self._L.gpx_icm_loglik, 2 * T + T * T + nhyper_kernel, grad)

    def _icm_posterior(self, entry, Xs, ts, full):
        Xs = _f64(Xs, 2)
        ts = np.ascontiguousarray(ts, dtype=np.int32)
        m = Xs.shape[0]
        if ts.shape != (m,):
            raise ValueError('one task per test point')
        mu = np.empty(m)
        cov = np.empty((m, m)) if full else np.empty(m)
        check(entry(self._h, _ptr(Xs), _ptr(ts), m, _ptr(mu), _ptr(cov)))
        return mu, cov

    def icm_posterior(self, Xs, ts):
        return self._icm_posterior(self._L.gpx_icm_posterior, Xs, ts, False)

    def icm_posterior_full(self, Xs, ts):
        return self._icm_posterior(self._L.gpx_icm_posterior_full, Xs, ts, True)

    # -- sparse pseudo-input models (FITC / DTC / VFE) on the resident data --
    def sparse_update(self, spec, method, U, log_sn, mean):
        U = _f64(U, 2)
        info = C.c_int(0)
        check(self._L.gpx_sparse_update(self._h, spec.ref(), int(method), _ptr(U), U.shape[0],
                                        float(log_sn), float(mean), C.byref(info)))

    def sparse_append(self, Xnew, ynew):
        """True if the sparse model took the new observations in place, False if the caller
        has to upload everything and refactor (no current model / they do not fit)."""
        return self._append(self._L.gpx_sparse_append, Xnew, ynew)

    def sparse_loglik(self, nhyper_kernel, grad=False):
        return self._loglik(self._L.gpx_sparse_loglik, nhyper_kernel + 2, grad)

    def sparse_posterior(self, Xs, grad=False):
        Xs = _f64(Xs, 2)
        m, d = Xs.shape
        mu, s2 = np.empty(m), np.empty(m)
        dmu, ds2 = (np.empty((m, d)), np.empty((m, d))) if grad else (None, None)
        if m:
            check(self._L.gpx_sparse_posterior(self._h, _ptr(Xs), m, _ptr(mu), _ptr(s2),
                                               _ptr(dmu), _ptr(ds2)))
        return (mu, s2, dmu, ds2) if grad else (mu, s2)

    def sparse_posterior_full(self, Xs):
        return self._posterior(self._L.gpx_sparse_posterior_full, Xs, True)

    def sparse_timings(self):
        """HIP-event ms of the last [update, gradient stage, contraction pass]."""
        ms = np.zeros(3)
        check(self._L.gpx_sparse_timings(self._h, _ptr(ms)))
        return ms

    def sparse_loglik_pseudo(self, nhyper_kernel, p, d):
        """lZ, dlZ (as sparse_loglik with grad) and dU = d lZ / d U (p x d)."""
        lZ = C.c_double(0)
        dlZ, dU = np.empty(nhyper_kernel + 2), np.empty((p, d))
        check(self._L.gpx_sparse_loglik_pseudo(self._h, C.byref(lZ), _ptr(dlZ), _ptr(dU)))
        return lZ.value, dlZ, dU

    def sparse_pseudo_timing(self):
        """HIP-event ms of the dU pass of the last sparse_loglik_pseudo."""
        ms = np.zeros(1)
        check(self._L.gpx_sparse_pseudo_timing(self._h, _ptr(ms)))
        return float(ms[0])

    # -- sparse Laplace classification (SparseLaplaceGP) on the resident data: labels as y --
    def sparse_laplace_update(self, spec, lik, mean, U, jitter=1e-6, tol=1e-8, max_iter=50):
        """Newton's method in the p-dimensional space to the mode; returns the number of steps."""
        U = _f64(U, 2)
        iters, info = C.c_int(0), C.c_int(0)
        check(self._L.gpx_sparse_laplace_update(self._h, spec.ref(), int(lik), float(mean),
                                                _ptr(U), U.shape[0], float(jitter), float(tol),
                                                int(max_iter), C.byref(iters), C.byref(info)))
        return iters.value

    def sparse_laplace_loglik(self, nhyper_kernel, grad=False):
        return self._loglik(self._L.gpx_sparse_laplace_loglik, nhyper_kernel + 1, grad)

    def sparse_laplace_loglik_pseudo(self, nhyper_kernel, p, d):
        """lZ, dlZ (as sparse_laplace_loglik with grad) and dU = d lZ / d U (p x d)."""
        lZ = C.c_double(0)
        dlZ, dU = np.empty(nhyper_kernel + 1), np.empty((p, d))
        check(self._L.gpx_sparse_laplace_loglik_pseudo(self._h, C.byref(lZ), _ptr(dlZ),
                                                       _ptr(dU)))
        return lZ.value, dlZ, dU

    def sparse_laplace_posterior(self, Xs, grad=False):
        Xs = _f64(Xs, 2)
        m, d = Xs.shape
        mu, s2 = np.empty(m), np.empty(m)
        dmu, ds2 = (np.empty((m, d)), np.empty((m, d))) if grad else (None, None)
        if m:
            check(self._L.gpx_sparse_laplace_posterior(self._h, _ptr(Xs), m, _ptr(mu), _ptr(s2),
                                                       _ptr(dmu), _ptr(ds2)))
        return (mu, s2, dmu, ds2) if grad else (mu, s2)

    def sparse_laplace_posterior_full(self, Xs):
        return self._posterior(self._L.gpx_sparse_laplace_posterior_full, Xs, True)

    def sparse_laplace_get_mode(self, p, n):
        """(z, f, g): the mode in the p-dimensional space, the latent at the data and the gradient
        of log p(y | f) there."""
        z, f, g = np.empty(p), np.empty(n), np.empty(n)
        check(self._L.gpx_sparse_laplace_get_mode(self._h, _ptr(z), _ptr(f), _ptr(g)))
        return z, f, g

    def sparse_laplace_timings(self):
        """HIP-event ms of the last update, its first Newton step and that step's two panel
        passes, the last gradient stage, its contraction pass and the dU pass; then the Newton
        steps and halvings of the last update."""
        ms = np.zeros(8)
        check(self._L.gpx_sparse_laplace_timings(self._h, _ptr(ms)))
        out = dict(zip(('update', 'step', 'panel_passes', 'gradient', 'contraction', 'pseudo'),
                       ms))
        out.update(iters=int(ms[6]), halvings=int(ms[7]))
        return out

    # -- sparse EP classification (SparseEPGP) on the resident data: labels as y --
    def sparse_ep_update(self, spec, mean, U, jitter=1e-6, tol=1e-10, max_iter=200, damping=0.8):
        """Damped parallel EP on the pseudo-inputs to a fixed point of the sites; returns the
        number of sweeps."""
        U = _f64(U, 2)
        iters, info = C.c_int(0), C.c_int(0)
        check(self._L.gpx_sparse_ep_update(self._h, spec.ref(), float(mean), _ptr(U), U.shape[0],
                                           float(jitter), float(tol), int(max_iter),
                                           float(damping), C.byref(iters), C.byref(info)))
        return iters.value

    def sparse_ep_loglik(self, nhyper_kernel, grad=False):
        return self._loglik(self._L.gpx_sparse_ep_loglik, nhyper_kernel + 1, grad)

    def sparse_ep_loglik_pseudo(self, nhyper_kernel, p, d):
        """lZ, dlZ (as sparse_ep_loglik with grad) and dU = d lZ / d U (p x d)."""
        lZ = C.c_double(0)
        dlZ, dU = np.empty(nhyper_kernel + 1), np.empty((p, d))
        check(self._L.gpx_sparse_ep_loglik_pseudo(self._h, C.byref(lZ), _ptr(dlZ), _ptr(dU)))
        return lZ.value, dlZ, dU

    def sparse_ep_posterior(self, Xs, grad=False):
        Xs = _f64(Xs, 2)
        m, d = Xs.shape
        mu, s2 = np.empty(m), np.empty(m)
        dmu, ds2 = (np.empty((m, d)), np.empty((m, d))) if grad else (None, None)
        if m:
            check(self._L.gpx_sparse_ep_posterior(self._h, _ptr(Xs), m, _ptr(mu), _ptr(s2),
                                                  _ptr(dmu), _ptr(ds2)))
        return (mu, s2, dmu, ds2) if grad else (mu, s2)

    def sparse_ep_posterior_full(self, Xs):
        return self._posterior(self._L.gpx_sparse_ep_posterior_full, Xs, True)

    def sparse_ep_get_sites(self, n):
        """(tau, nu, mu, s2): the sites and the marginals at the data."""
        out = [np.empty(n) for _ in range(4)]
        check(self._L.gpx_sparse_ep_get_sites(self._h, n, *[_ptr(a) for a in out]))
        return tuple(out)

    def sparse_ep_timings(self):
        """HIP-event ms of the last update, its first sweep and that sweep's stages (scaled
        panel, A, factorisation, T0 product, fused pass), the last gradient stage, its contraction
        pass and the dU pass; then the sweeps of the last update."""
        ms = np.zeros(12)
        check(self._L.gpx_sparse_ep_timings(self._h, _ptr(ms)))
        out = dict(zip(('update', 'sweep', 'scale', 'product_a', 'factor', 'product_t0',
                        'fused_pass', 'gradient', 'contraction', 'pseudo'), ms))
        out.update(sweeps=int(ms[10]))
        return out

    def select_pivots(self, spec, X, p, tol=0.0):
        """Greedy conditional-variance selection (pivoted partial Cholesky of K(X, X)) of at
        most p rows of X (n x d, host), or of the handle's resident data when X is None:
        (idx, piv, trace), each of length count <= p."""
        p = int(p)
        if X is None:
            n = d = 0
        else:
            X = _f64(X, 2)
            n, d = X.shape
        size = max(p, 0)
        idx = np.empty(size, dtype=np.int64)
        piv, trace = np.empty(size), np.empty(size)
        count = _i64(0)
        check(self._L.gpx_select_pivots(self._h, spec.ref(), _ptr(X), n, d, p, float(tol),
                                        _ptr(idx), _ptr(piv), _ptr(trace), C.byref(count)))
        c = count.value
        return idx[:c].copy(), piv[:c].copy(), trace[:c].copy()

    def select_timing(self):
        """HIP-event ms around the launches of the last select_pivots."""
        ms = np.zeros(1)
        check(self._L.gpx_select_timing(self._h, _ptr(ms)))
        return float(ms[0])

    # -- Fourier-feature function samples (a state of the handle's own) --
    def fourier_fit(self, W, b, a, log_sn, mean, X, y, P):
        """theta (S, M) of the S rows of P: the posterior weights given (X, y); X None: the
        handle's resident data; X with no rows: theta = P."""
        W, b, P = _f64(W, 2), _f64(b, 1), _f64(P, 2)
        M, d = W.shape
        if X is None:
            n, y = -1, None
        else:
            X, y = _f64(X, 2), _f64(y, 1)
            n = X.shape[0]
            if n and X.shape[1] != d:
                raise ValueError('X and W have different dimensions')
        if b.shape[0] != M or P.shape[1] != M or (n > 0 and y.shape[0] != n):
            raise ValueError('shapes of W, b, P, X and y do not agree')
        theta = np.empty_like(P)
        info = C.c_int(0)
        check(self._L.gpx_fourier_fit(self._h, _ptr(W), M, d, _ptr(b), float(a), float(log_sn),
                                      float(mean), _ptr(X), n, _ptr(y), _ptr(P), P.shape[0],
                                      _ptr(theta), C.byref(info)))
        self._fourier_shape = (P.shape[0], d)
        return theta

    def fourier_set(self, W, b, a, mean, theta):
        W, b, theta = _f64(W, 2), _f64(b, 1), _f64(theta, 2)
        M, d = W.shape
        if b.shape[0] != M or theta.shape[1] != M:
            raise ValueError('shapes of W, b and theta do not agree')
        check(self._L.gpx_fourier_set(self._h, _ptr(W), M, d, _ptr(b), float(a), float(mean),
                                      _ptr(theta), theta.shape[0]))
        self._fourier_shape = (theta.shape[0], d)

    def fourier_eval(self, Xs, grad=False):
        """F (S, n), or (F, G) with G (S, n, d), of the installed sample at the rows of Xs."""
        Xs = _f64(Xs, 2)
        n, d = Xs.shape
        S, dim = getattr(self, '_fourier_shape', (0, d))
        if S == 0:
            raise GpxError('fourier_eval: no sample (call fourier_fit or fourier_set)')
        if d != dim:
            raise ValueError('test inputs have the wrong dimension')
        F = np.empty((S, n))
        G = np.empty((S, n, d)) if grad else None
        check(self._L.gpx_fourier_eval(self._h, _ptr(Xs), n, _ptr(F), _ptr(G)))
        return (F, G) if grad else F

    def fourier_timings(self):
        """HIP-event ms of the last [fit, evaluation]."""
        ms = np.zeros(2)
        check(self._L.gpx_fourier_timings(self._h, _ptr(ms)))
        return ms

    # -- pathwise posterior function samples (a state of the handle's own) --
    def path_fit(self, W, b, a, P, E):
        """V (S, n) of the pathwise sample with theta = P (S, M) and noise draws E (S, n), behind
        the handle's exact factorisation (set_data, exact_update): its kernel, noise and mean."""
        W, b, P, E = _f64(W, 2), _f64(b, 1), _f64(P, 2), _f64(E, 2)
        M, d = W.shape
        if b.shape[0] != M or P.shape[1] != M or E.shape[0] != P.shape[0]:
            raise ValueError('shapes of W, b, P and E do not agree')
        V = np.empty_like(E)
        info = C.c_int(0)
        check(self._L.gpx_path_fit(self._h, _ptr(W), M, d, _ptr(b), float(a), _ptr(P), _ptr(E),
                                   E.shape[1], P.shape[0], _ptr(V), C.byref(info)))
        self._path_shape = (P.shape[0], d)
        return V

    def path_set(self, spec, mean, X, W, b, a, theta, V):
        """Install a given sample: X (n, d) or None, theta (S, M) and V (S, n)."""
        W, b, theta = _f64(W, 2), _f64(b, 1), _f64(theta, 2)
        M, d = W.shape
        S = theta.shape[0]
        if X is None or len(X) == 0:
            X, V, n = None, None, 0
        else:
            X, V = _f64(X, 2), _f64(V, 2)
            n = X.shape[0]
            if X.shape[1] != d or V.shape != (S, n):
                raise ValueError('shapes of X, W, theta and V do not agree')
        if b.shape[0] != M or theta.shape[1] != M:
            raise ValueError('shapes of W, b and theta do not agree')
        check(self._L.gpx_path_set(self._h, spec.ref(), float(mean), _ptr(X), n, d, _ptr(W), M,
                                   _ptr(b), float(a), _ptr(theta), _ptr(V), S))
        self._path_shape = (S, d)

    def path_eval(self, Xs, grad=False):
        """F (S, m), or (F, G) with G (S, m, d), of the installed sample at the rows of Xs."""
        Xs = _f64(Xs, 2)
        m, d = Xs.shape
        S, dim = getattr(self, '_path_shape', (0, d))
        if S == 0:
            raise GpxError('path_eval: no sample (call path_fit or path_set)')
        if d != dim:
            raise ValueError('test inputs have the wrong dimension')
        F = np.empty((S, m))
        G = np.empty((S, m, d)) if grad else None
        check(self._L.gpx_path_eval(self._h, _ptr(Xs), m, _ptr(F), _ptr(G)))
        return (F, G) if grad else F

    def path_timings(self):
        """HIP-event ms of the last [fit, evaluation, its feature term, its data term]."""
        ms = np.zeros(4)
        check(self._L.gpx_path_timings(self._h, _ptr(ms)))
        return ms

    # -- sparse-spectrum GP on the resident data (a state of the handle's own) --
    _ssgp_shape = (0, 0)        # (M, d) of the last ssgp_update of this handle
    def ssgp_update(self, W, b, a, log_sn, mean):
        """Factor the feature model of the resident data; returns lZ."""
        W, b = _f64(W, 2), _f64(b, 1)
        M, d = W.shape
        if b.shape[0] != M:
            raise ValueError('shapes of W and b do not agree')
        lZ, info = C.c_double(0), C.c_int(0)
        check(self._L.gpx_ssgp_update(self._h, _ptr(W), M, d, _ptr(b), float(a), float(log_sn),
                                      float(mean), C.byref(lZ), C.byref(info)))
        self._ssgp_shape = (M, d)
        return lZ.value

    def ssgp_loglik(self, grad=False, spectrum=False):
        """lZ; with grad (lZ, dlZ3, dW_W): d lZ / d (log sn, log sf, mean) and -sum_j D_jc W_jc
        per column c; with spectrum also D = d lZ / d W (M, d) and d lZ / d b (M)."""
        lZ = C.c_double(0)
        if not (grad or spectrum):
            check(self._L.gpx_ssgp_loglik(self._h, C.byref(lZ), None, None, None, None))
            return lZ.value
        M, d = self._ssgp_shape
        if M == 0:
            raise GpxError('ssgp_loglik: no model (call ssgp_update)')
        dlZ3, dW_W = np.empty(3), np.empty(d)
        dW, db = (np.empty((M, d)), np.empty(M)) if spectrum else (None, None)
        check(self._L.gpx_ssgp_loglik(self._h, C.byref(lZ), _ptr(dlZ3), _ptr(dW_W), _ptr(dW),
                                      _ptr(db)))
        return (lZ.value, dlZ3, dW_W, dW, db) if spectrum else (lZ.value, dlZ3, dW_W)

    def _ssgp_points(self, Xs):
        """Xs as the entries read it: m rows of the model's width."""
        Xs = _f64(Xs, 2)
        if self._ssgp_shape[0] == 0:
            raise GpxError('no sparse-spectrum model (call ssgp_update)')
        if Xs.shape[1] != self._ssgp_shape[1]:
            raise ValueError('test inputs have the wrong dimension')
        return Xs

    def ssgp_posterior(self, Xs, grad=False):
        Xs = self._ssgp_points(Xs)
        m, d = Xs.shape
        mu, s2 = np.empty(m), np.empty(m)
        dmu, ds2 = (np.empty((m, d)), np.empty((m, d))) if grad else (None, None)
        if m:
            check(self._L.gpx_ssgp_posterior(self._h, _ptr(Xs), m, _ptr(mu), _ptr(s2), _ptr(dmu),
                                             _ptr(ds2)))
        return (mu, s2, dmu, ds2) if grad else (mu, s2)

    def ssgp_posterior_full(self, Xs):
        return self._posterior(self._L.gpx_ssgp_posterior_full, self._ssgp_points(Xs), True)

    def ssgp_get(self):
        """beta (M,), the posterior mean of the weights."""
        M = self._ssgp_shape[0]
        if M == 0:
            raise GpxError('ssgp_get: no model (call ssgp_update)')
        beta = np.empty(M)
        check(self._L.gpx_ssgp_get(self._h, _ptr(beta)))
        return beta

    def ssgp_timings(self):
        """HIP-event ms of the last [panel, Gram, factorisation, A^-1 Phi^T, contraction,
        posterior, A^-1]."""
        ms = np.zeros(7)
        check(self._L.gpx_ssgp_timings(self._h, _ptr(ms)))
        return ms

    # -- matrix-free exact regression on the resident data (a state of the handle's own) --
    # the order of gpx.h's GPX_ITER_MS_* (tests/test_iter_host.py holds the two together)
    ITER_TIMES = ('select', 'update', 'iters', 'product', 'precond', 'vector', 'trace',
                  'posterior', 'apply')
    _data_shape = (0, 0)            # (n, d) of the last set_data of this handle
    _iter_probes = None             # probes of the last iter_set_probes, for _data_shape's rows
    _iter_shape = (0, 0, 0, 0)      # (n, d, probes, nhyper) of the last iter_update
    _iter_iters = 0

    def iter_set_probes(self, G1, G2):
        """The standard-normal draws g1 (probes, rank) and g2 (probes, n) of the resident rows."""
        G1, G2 = _f64(G1, 2), _f64(G2, 2)
        if G1.shape[0] != G2.shape[0]:
            raise ValueError('shapes of G1 and G2 do not agree')
        if G2.shape[1] != self._data_shape[0]:
            raise ValueError('G2 has %d columns, the resident data %d rows'
                             % (G2.shape[1], self._data_shape[0]))
        self._iter_probes = None
        self._iter_shape = (0, 0, 0, 0)
        self._iter_cache_rank = 0
        check(self._L.gpx_iter_set_probes(self._h, _ptr(G1) if G1.size else None,
                                          _ptr(G2) if G2.size else None, G2.shape[0],
                                          G1.shape[1]))
        self._iter_probes = G2.shape[0]

    def iter_update(self, spec, log_sn, mean, rank, tol, max_iter):
        """One batched PCG run on the resident data; returns (iterations, info): info 0, or
        1 + the worst column that did not reach tol. The sizes every later result is read with
        are the handle's own: the rows of set_data and the probes of iter_set_probes."""
        if self._iter_probes is None:
            raise GpxError('iter_update: no probes (call iter_set_probes)')
        iters, info = _i64(0), C.c_int(0)
        self._iter_shape = (0, 0, 0, 0)
        self._iter_cache_rank = 0
        check(self._L.gpx_iter_update(self._h, spec.ref(), float(log_sn), float(mean), int(rank),
                                      float(tol), int(max_iter), C.byref(iters), C.byref(info)))
        self._iter_shape = tuple(self._data_shape) + (self._iter_probes, spec.c.nhyper)
        self._iter_iters = int(iters.value)
        return self._iter_iters, info.value

    def iter_loglik(self, grad=False):
        return self._loglik(self._L.gpx_iter_loglik, self._iter_shape[3] + 2, grad)

    def _iter_points(self, Xs):
        Xs = _f64(Xs, 2)
        if self._iter_shape[0] == 0:
            raise GpxError('no iterative model (call iter_update)')
        if Xs.shape[1] != self._iter_shape[1]:
            raise ValueError('test inputs have the wrong dimension')
        return Xs

    def iter_posterior(self, Xs):
        return self._posterior(self._L.gpx_iter_posterior, self._iter_points(Xs), False)

    def iter_posterior_full(self, Xs):
        return self._posterior(self._L.gpx_iter_posterior_full, self._iter_points(Xs), True)

    def _iter_columns(self, B):
        """B (n,) or (n, nb) -> (flat, its columns as contiguous rows)."""
        B = _f64(B)
        n = self._iter_shape[0]
        if n == 0:
            raise GpxError('no iterative model (call iter_update)')
        if B.ndim not in (1, 2) or B.shape[0] != n:
            raise ValueError('expected %d rows' % n)
        return B.ndim == 1, np.ascontiguousarray(B.reshape(n, -1).T)

    def iter_solve(self, B):
        """(K + sn^2 I)^-1 B for B (n,) or (n, nb)."""
        flat, Bt = self._iter_columns(B)
        out, iters = np.empty_like(Bt), _i64(0)
        check(self._L.gpx_iter_solve(self._h, _ptr(Bt), Bt.shape[0], _ptr(out), C.byref(iters)))
        return out[0].copy() if flat else np.ascontiguousarray(out.T)

    def iter_apply(self, V):
        """(K + sn^2 I) V for V (n,) or (n, nv <= 32), without storing K."""
        flat, Vt = self._iter_columns(V)
        out = np.empty_like(Vt)
        check(self._L.gpx_iter_apply(self._h, _ptr(Vt), Vt.shape[0], _ptr(out)))
        return out[0].copy() if flat else np.ascontiguousarray(out.T)

    def iter_get(self):
        """What the last update left: dict of alpha (n,), U, V (n, probes), the coefficients a, b
        (iterations, 1 + probes), nit, rz0 (1 + probes,) and logdetP."""
        n, _, t, _ = self._iter_shape
        if n == 0:
            raise GpxError('no iterative model (call iter_update)')
        k = self._iter_iters
        alpha, U, V = np.empty(n), np.empty((t, n)), np.empty((t, n))
        a, b = np.zeros((k, 1 + t)), np.zeros((k, 1 + t))
        nit, rz0, ldp = np.empty(1 + t), np.empty(1 + t), C.c_double(0)
        check(self._L.gpx_iter_get(self._h, _ptr(alpha), _ptr(U), _ptr(V), _ptr(a), _ptr(b),
                                   _ptr(nit), _ptr(rz0), C.byref(ldp)))
        return dict(alpha=alpha, U=np.ascontiguousarray(U.T), V=np.ascontiguousarray(V.T), a=a,
                    b=b, nit=nit.astype(int), rz0=rz0, logdetP=ldp.value)

    def iter_timings(self):
        """HIP-event ms of the last calls by name (ITER_TIMES; 'iters' is a count)."""
        ms = np.zeros(len(self.ITER_TIMES))
        check(self._L.gpx_iter_timings(self._h, _ptr(ms)))
        return dict(zip(self.ITER_TIMES, ms))

    # -- the variance cache of the iterative model --
    # the order of gpx.h's GPX_ITER_CACHE_MS_*
    ITER_CACHE_TIMES = ('select', 'orth', 'kq', 'h', 'c', 'cross', 'finish', 'grad')
    ITER_CACHE_KMAX = 1024
    ITER_CACHE_POINTS = 1 << 20
    _iter_cache_rank = 0            # pivots of the last iter_cache_build (0: no cache)

    def iter_cache_build(self, k):
        """The cache of the last iter_update with at most k pivots; returns their count."""
        n = self._iter_shape[0]
        if n == 0:
            raise GpxError('no iterative model (call iter_update)')
        k = int(k)
        if not 1 <= k <= min(n, self.ITER_CACHE_KMAX):
            raise ValueError('need 1 <= k <= min(n, %d) (got %d)' % (self.ITER_CACHE_KMAX, k))
        self._iter_cache_rank = 0
        keff = _i64(0)
        check(self._L.gpx_icache_build(self._h, k, C.byref(keff)))
        # (the rank every later result is sized with: at most k, whatever the entry reports)
        self._iter_cache_rank = max(1, min(int(keff.value), k))
        return self._iter_cache_rank

    def _iter_cache_points(self, Xs):
        Xs = self._iter_points(Xs)
        if not 1 <= Xs.shape[0] <= self.ITER_CACHE_POINTS:
            raise ValueError('one call covers 1 .. %d points (got %d)'
                             % (self.ITER_CACHE_POINTS, Xs.shape[0]))
        return Xs

    def iter_cache_eval(self, Xs, grad=False):
        """(mu, s2), with grad (mu, s2, dmu, ds2), at the rows of Xs from the cache."""
        Xs = self._iter_cache_points(Xs)
        if self._iter_cache_rank == 0:
            raise GpxError('no cache (call iter_cache_build)')
        m, d = Xs.shape
        mu, s2 = np.empty(m), np.empty(m)
        dmu, ds2 = (np.empty((m, d)), np.empty((m, d))) if grad else (None, None)
        check(self._L.gpx_icache_eval(self._h, _ptr(Xs), m, _ptr(mu), _ptr(s2), _ptr(dmu),
                                          _ptr(ds2)))
        return (mu, s2, dmu, ds2) if grad else (mu, s2)

    def iter_cross_apply(self, Xs, W):
        """K(Xs, X) W^T (m, nw) for W (nw, n), nw <= 1025, without storing K(Xs, X)."""
        Xs, W = self._iter_cache_points(Xs), _f64(W, 2)
        if W.shape[1] != self._iter_shape[0] or not 1 <= W.shape[0] <= 1 + self.ITER_CACHE_KMAX:
            raise ValueError('W must be (1 .. %d, %d)'
                             % (1 + self.ITER_CACHE_KMAX, self._iter_shape[0]))
        out = np.empty((Xs.shape[0], W.shape[0]))
        check(self._L.gpx_icache_cross_apply(self._h, _ptr(Xs), Xs.shape[0], _ptr(W), W.shape[0],
                                           _ptr(out)))
        return out

    def iter_cache_get(self):
        """dict of pivots (k_eff,), Q (k_eff, n), H (k_eff, k_eff), C (k_eff, n)."""
        k, n = self._iter_cache_rank, self._iter_shape[0]
        if k == 0 or n == 0:
            raise GpxError('no cache (call iter_cache_build)')
        piv = np.zeros(k, dtype=np.int64)
        Q, H, Cm = np.empty((k, n)), np.empty((k, k)), np.empty((k, n))
        check(self._L.gpx_icache_get(self._h, _ptr(piv), _ptr(Q), _ptr(H), _ptr(Cm)))
        return dict(pivots=piv, Q=Q, H=H, C=Cm)

    def iter_cache_timings(self):
        """ms of the last build and eval by name (ITER_CACHE_TIMES)."""
        ms = np.zeros(len(self.ITER_CACHE_TIMES))
        check(self._L.gpx_icache_timings(self._h, _ptr(ms)))
        return dict(zip(self.ITER_CACHE_TIMES, ms))

    def sparse_get_state(self, p):
        F1, F2, v = np.empty((p, p)), np.empty((p, p)), np.empty(p)
        check(self._L.gpx_sparse_get_state(self._h, _ptr(F1), _ptr(F2), _ptr(v)))
        return F1, F2, v

    def exact_posterior_grad(self, Xs):
        Xs = _f64(Xs, 2)
        m, d = Xs.shape
        mu, s2 = np.empty(m), np.empty(m)
        dmu, ds2 = np.empty((m, d)), np.empty((m, d))
        if m:
            check(self._L.gpx_exact_posterior_grad(self._h, _ptr(Xs), m, _ptr(mu),
                                                   _ptr(s2), _ptr(dmu), _ptr(ds2)))
        return mu, s2, dmu, ds2

    def kernel_gradx(self, spec, X1, X2=None, wrt=1):
        X1, n1, X2, n2, d = _pair(X1, X2)
        out = np.empty((n1, n2, d))
        if out.size:
            check(self._L.gpx_kernel_gradx(self._h, spec.ref(), _ptr(X1), n1, _ptr(X2),
                                           n2, d, wrt, _ptr(out)))
        return out

    def kernel_gradxy(self, spec, X1, X2=None):
        X1, n1, X2, n2, d = _pair(X1, X2)
        out = np.empty((n1, n2, d, d))
        if out.size:
            check(self._L.gpx_kernel_gradxy(self._h, spec.ref(), _ptr(X1), n1, _ptr(X2), n2, d,
                                            _ptr(out)))
        return out

    def exact_posterior_gradient(self, Xs):
        """mu (m, d) and S (m, d, d): mean and covariance of grad f at the rows of Xs."""
        Xs = _f64(Xs, 2)
        m, d = Xs.shape
        mu, S = np.empty((m, d)), np.empty((m, d, d))
        if m:
            check(self._L.gpx_exact_posterior_gradient(self._h, _ptr(Xs), m, _ptr(mu), _ptr(S)))
        return mu, S

    def exact_get_factor(self, n, want_R=True):
        R = np.empty((n, n)) if want_R else None
        a = np.empty(n)
        check(self._L.gpx_exact_get_factor(self._h, n, _ptr(R), _ptr(a)))
        return R, a

    def loglik_batch(self, spec, thetas, grad=False):
        thetas = _f64(thetas, 2)
        B, nth = thetas.shape
        if nth != spec.c.nhyper + 2:
            raise ValueError('thetas must have %d columns' % (spec.c.nhyper + 2))
        lZ = np.empty(B)
        dlZ = np.empty((B, nth)) if grad else None
        info = np.zeros(B, dtype=np.int32)
        check(self._L.gpx_loglik_batch(self._h, spec.ref(), _ptr(thetas), B,
                                       int(grad), _ptr(lZ), _ptr(dlZ),
                                       _ptr(info)))
        return (lZ, dlZ) if grad else lZ

    def batch_plan(self, B, grad=False):
        """How a batch of B thetas would run (gpx_batch_plan): dict with the arrangement
        ('contexts', 'groups/panel', 'groups/lockstep' or 'groups/solo'), members per group and groups in
        flight."""
        plan = (C.c_int * 4)()
        check(self._L.gpx_batch_plan(self._h, int(B), int(grad), plan))
        return {'arrangement': ('contexts', 'groups/panel', 'groups/lockstep', 'groups/solo')[plan[0]],
                'members_per_group': int(plan[1]), 'groups_in_flight': int(plan[2]),
                'safe_mode': bool(plan[3])}

    def posterior_batch(self, spec, thetas, Xs, grad=False):
        """Posterior at Xs of every model theta on the resident data: arrays
        mu, s2 of shape (B, m) [and dmu, ds2 of shape (B, m, d)]."""
        thetas = _f64(thetas, 2)
        B, nth = thetas.shape
        if nth != spec.c.nhyper + 2:
            raise ValueError('thetas must have %d columns' % (spec.c.nhyper + 2))
        Xs = _f64(Xs, 2)
        m, d = Xs.shape
        mu, s2 = np.empty((B, m)), np.empty((B, m))
        dmu = np.empty((B, m, d)) if grad else None
        ds2 = np.empty((B, m, d)) if grad else None
        info = np.zeros(B, dtype=np.int32)
        check(self._L.gpx_posterior_batch(self._h, spec.ref(), _ptr(thetas), B, _ptr(Xs), m,
                                          _ptr(mu), _ptr(s2), _ptr(dmu), _ptr(ds2),
                                          _ptr(info)))
        return (mu, s2, dmu, ds2) if grad else (mu, s2)

    # -- instrumentation --
    def enable_timing(self, on=True):
        check(self._L.gpx_enable_timing(self._h, int(on)))

    def timings(self):
        ms = np.zeros(NTIMERS)
        check(self._L.gpx_get_timings(self._h, _ptr(ms), NTIMERS))
        names = [self._L.gpx_timing_name(i).decode() for i in range(NTIMERS)]
        return dict(zip(names, ms))

    def batch_timings(self):
        """(ms, members): event time of the factor (+ inverse) stages of the groups that
        gpx_loglik_batch ran since enable_timing(True), and the members they held."""
        ms, mem = C.c_double(0), _i64(0)
        check(self._L.gpx_batch_timings(self._h, C.byref(ms), C.byref(mem)))
        return ms.value, mem.value

    def synchronize(self):
        check(self._L.gpx_synchronize(self._h))

    # -- dense building blocks --
    def la_gemm(self, A, B, ta=False, tb=False, alpha=1.0, beta=0.0, Cin=None):
        A, B = _f64(A, 2), _f64(B, 2)
        M = A.shape[1] if ta else A.shape[0]
        K = A.shape[0] if ta else A.shape[1]
        N = B.shape[0] if tb else B.shape[1]
        out = np.zeros((M, N)) if Cin is None else _f64(Cin, 2).copy()
        check(self._L.gpx_la_gemm(self._h, int(ta), int(tb), M, N, K, alpha,
                                  _ptr(A), A.shape[1], _ptr(B), B.shape[1], beta,
                                  _ptr(out), N))
        return out

    def la_gemm_ex(self, A, B, Cin, C2=None, **args):
        """One call of the tile engine with every GemmArgs field given (gpx_la_gemm_ex): the
        flat float64 buffers A, B, Cin and C2 go to the device verbatim, `args` are the fields
        of gpx_gemm_ex_args (unnamed ones: use_lists = 1, beta0_from = -1, batch = 1, alpha =
        1, the rest 0). B is None with b_is_c = 1. Returns the whole C and C2 buffers."""
        a = _GemmExArgs(use_lists=1, beta0_from=-1, batch=1, alpha=1.0)
        names = {n for n, _ in _GemmExArgs._fields_}
        for k, v in args.items():
            if k not in names:
                raise TypeError('la_gemm_ex: unknown field %r' % k)
            setattr(a, k, float(v) if k in ('alpha', 'beta') else int(v))
        A = _f64(A, 1)
        B = None if B is None else _f64(B, 1)
        out = _f64(Cin, 1).copy()
        out2 = None if C2 is None else _f64(C2, 1).copy()
        check(self._L.gpx_la_gemm_ex(self._h, C.byref(a), _ptr(A), A.size,
                                     _ptr(B), 0 if B is None else B.size, _ptr(out), out.size,
                                     _ptr(out2), 0 if out2 is None else out2.size))
        return out, out2

    def la_potrf(self, A, inverse=False):
        A = _f64(A, 2)
        n = A.shape[0]
        R = np.empty((n, n))
        Rinv = np.empty((n, n)) if inverse else None
        Ainv = np.empty((n, n)) if inverse else None
        info = C.c_int(0)
        check(self._L.gpx_la_potrf(self._h, _ptr(A), n, _ptr(R), _ptr(Rinv),
                                   _ptr(Ainv), C.byref(info)))
        return (R, Rinv, Ainv) if inverse else R

    def la_gemm_bench(self, n, ta=False, tb=False, reps=5):
        ms = C.c_double(0)
        check(self._L.gpx_la_gemm_bench(self._h, int(ta), int(tb), n, reps,
                                        C.byref(ms)))
        return ms.value

    def la_gemm_bench_ex(self, n, ta=0, tb=0, flags=0, order=0, swizzle=0, tile=0,
                         waves=0, same_ab=0, reps=1):
        ms = C.c_double(0)
        check(self._L.gpx_la_gemm_bench_ex(self._h, int(ta), int(tb), n, flags, order,
                                           swizzle, tile, waves, same_ab, reps,
                                           C.byref(ms)))
        return ms.value

    def la_gemm_bench_mnk(self, M, N, K, ta=0, tb=0, flags=0, beta=0.0, tile=0, reps=3):
        ms = C.c_double(0)
        check(self._L.gpx_la_gemm_bench_mnk(self._h, int(ta), int(tb), M, N, K, flags,
                                            float(beta), tile, reps, C.byref(ms)))
        return ms.value

    def la_potrf_bench(self, n, inverse=False, reps=3):
        ms = C.c_double(0)
        check(self._L.gpx_la_potrf_bench(self._h, n, int(inverse), reps,
                                         C.byref(ms)))
        return ms.value


for _name in [n for n, f in list(vars(Handle).items())
              if callable(f) and not n.startswith('_') and n != 'close']:
    setattr(Handle, _name, _serialised(getattr(Handle, _name)))


def device_count():
    n = C.c_int(0)
    check(lib().gpx_device_count(C.byref(n)))
    return n.value


# Whose data the library's per-device handles hold (they are process-wide): a caller
# that passes a `token` with its data uploads X, y only when another data set, another
# caller or fewer devices were there last, and NULL (resident data) otherwise.
_multi_resident = (None, 0)          # (token, ndev)


def _multi_call(call, X, y, token, ndev):
    """One multi-device call under the library lock: decide whether X, y have to go down
    (they do unless the devices hold the data of `token` already), call, and record what
    is resident afterwards -- all three inside the lock, so that two threads cannot
    interleave the decision and the update; a call that fails leaves the record empty
    (the C side drops its resident data on an error path too)."""
    global _multi_resident
    with _lock:
        tok, have = _multi_resident
        if X is not None and token is not None and tok == token and have >= ndev:
            X = y = None
        uploaded = X is not None
        try:
            out = call(X, y)
        except Exception:
            _multi_resident = (None, 0)
            raise
        if uploaded:
            _multi_resident = (token, ndev)
    return out


def loglik_batch_multi(spec, thetas, X=None, y=None, grad=False, ndev=1, token=None):
    """gpx_loglik_batch_multi: B thetas over the first `ndev` GPUs of the node from
    this one process (one host thread and handle per device inside the library, ONE
    RCCL all-gather; no torch). X = y = None evaluates on the data a previous call
    left resident. token (hashable, with X and y): upload X, y only if the devices do
    not already hold the data of this token (one upload per data set instead of one
    per call). Returns lZ (B,) [and dlZ (B, nth)]; members that are not positive
    definite come back as -inf / NaN."""
    return _multi_call(lambda X_, y_: _loglik_batch_multi(spec, thetas, X_, y_, grad, ndev),
                       X, y, token, ndev)


def _loglik_batch_multi(spec, thetas, X, y, grad, ndev):
    thetas = _f64(thetas, 2)
    B, nth = thetas.shape
    if nth != spec.c.nhyper + 2:
        raise ValueError('thetas must have %d columns' % (spec.c.nhyper + 2))
    if (X is None) != (y is None):
        raise ValueError('pass both X and y, or neither')
    n = d = 0
    if X is not None:
        X, y = _f64(X, 2), _f64(y, 1)
        if X.shape[0] != y.shape[0]:
            raise ValueError('X and y disagree')
        n, d = X.shape
    lZ = np.empty(B)
    dlZ = np.empty((B, nth)) if grad else None
    info = np.zeros(B, dtype=np.int32)
    check(lib().gpx_loglik_batch_multi(spec.ref(), _ptr(thetas), B, _ptr(X), _ptr(y), n, d,
                                       int(grad), int(ndev), _ptr(lZ), _ptr(dlZ),
                                       _ptr(info)))
    return (lZ, dlZ) if grad else lZ


def posterior_batch_multi(spec, thetas, Xs, X=None, y=None, grad=False, ndev=1, token=None):
    """gpx_posterior_batch_multi: the posteriors at Xs of the B models theta over the first
    `ndev` GPUs of the node from this one process (see loglik_batch_multi, also for
    `token`). Returns mu, s2 of shape (B, m) [and dmu, ds2 of shape (B, m, d)]; rows of
    members that are not positive definite are NaN."""
    return _multi_call(lambda X_, y_: _posterior_batch_multi(spec, thetas, Xs, X_, y_, grad, ndev),
                       X, y, token, ndev)


def _posterior_batch_multi(spec, thetas, Xs, X, y, grad, ndev):
    thetas = _f64(thetas, 2)
    B, nth = thetas.shape
    if nth != spec.c.nhyper + 2:
        raise ValueError('thetas must have %d columns' % (spec.c.nhyper + 2))
    if (X is None) != (y is None):
        raise ValueError('pass both X and y, or neither')
    Xs = _f64(Xs, 2)
    m, d = Xs.shape
    n = 0
    if X is not None:
        X, y = _f64(X, 2), _f64(y, 1)
        if X.shape[0] != y.shape[0] or X.shape[1] != d:
            raise ValueError('X, y and Xs disagree')
        n = X.shape[0]
    mu, s2 = np.empty((B, m)), np.empty((B, m))
    dmu = np.empty((B, m, d)) if grad else None
    ds2 = np.empty((B, m, d)) if grad else None
    info = np.zeros(B, dtype=np.int32)
    check(lib().gpx_posterior_batch_multi(spec.ref(), _ptr(thetas), B, _ptr(X), _ptr(y), n,
                                          d if X is not None else 0, _ptr(Xs), m, int(grad),
                                          int(ndev), _ptr(mu), _ptr(s2), _ptr(dmu), _ptr(ds2),
                                          _ptr(info)))
    return (mu, s2, dmu, ds2) if grad else (mu, s2)


def batch_partition(B, world, rank):
    lo, hi = _i64(0), _i64(0)
    lib().gpx_batch_partition(B, world, rank, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def multi_comm_size():
    """Ranks of the RCCL communicator of the last multi-device call (0: none yet)."""
    return int(lib().gpx_multi_comm_size())


def multi_enable_timing(ndev, on=True):
    """HIP-event timing of the groups on the library's handles of the first ndev devices
    (they exist after the first multi-device call with that many devices)."""
    check(lib().gpx_multi_enable_timing(int(ndev), int(bool(on))))


def multi_batch_info(ndev, B_per_dev, grad=False):
    """Per device of the in-library multi-device path: the event time (ms) of its groups'
    dense stages and the members they held since multi_enable_timing(ndev, True), and how its
    handle cuts a block of B_per_dev thetas (batch_plan's dict, safe_mode included)."""
    ms = (C.c_double * ndev)()
    mem = (_i64 * ndev)()
    plans = (C.c_int * (4 * ndev))()
    check(lib().gpx_multi_batch_info(int(ndev), int(B_per_dev), int(grad), ms, mem, plans))
    return [{'device': i, 'dense_ms': float(ms[i]), 'members': int(mem[i]),
             'arrangement': ('contexts', 'groups/panel', 'groups/lockstep', 'groups/solo')[plans[4 * i]],
             'members_per_group': int(plans[4 * i + 1]),
             'groups_in_flight': int(plans[4 * i + 2]),
             'safe_mode': bool(plans[4 * i + 3])} for i in range(ndev)]


def panel_grid_check(nmem, ncu=256):
    """(spine workgroups per member, workers) of a panel launch over nmem members on a device
    of ncu CUs for the graph with the fused spine task -- the fewest spines any graph gets --,
    or RuntimeError if even one spine workgroup per member does not fit
    (gpx_panel_grid_check; host only)."""
    sp, wk = C.c_int(0), C.c_int(0)
    check(lib().gpx_panel_grid_check(int(nmem), int(ncu), C.byref(sp), C.byref(wk)))
    return sp.value, wk.value


def panel_grid_rule(nmem, ncu=256, tiles=8, split=True, fold=True):
    """(spine workgroups per member, workers) of a member-batched panel launch over `tiles`
    tiles (more than 8: a whole matrix) of the graph with / without the split spine and the
    fold, or RuntimeError if it cannot fit (gpx_panel_grid_rule; host only)."""
    sp, wk = C.c_int(0), C.c_int(0)
    check(lib().gpx_panel_grid_rule(int(nmem), int(ncu), int(tiles), int(split), int(fold),
                                    C.byref(sp), C.byref(wk)))
    return sp.value, wk.value


def multi_pack(rows, slot):
    """gpx_multi_pack: one device's member rows [cnt][width] as its NaN-padded gather
    slot [slot][width] (host only)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    cnt, width = rows.shape
    pack = np.empty((int(slot), width))
    check(lib().gpx_multi_pack(_ptr(rows) if cnt else None, cnt, width, int(slot), _ptr(pack)))
    return pack


def multi_scatter(gathered, B, ndev, width):
    """gpx_multi_scatter: the gathered [ndev][slot][width] image -> out[B][width]."""
    gathered = np.ascontiguousarray(gathered, dtype=np.float64)
    out = np.full((int(B), int(width)), np.nan)
    check(lib().gpx_multi_scatter(_ptr(gathered) if B else None, int(B), int(ndev), int(width),
                                  _ptr(out) if B else None))
    return out


def sweep_check(T, aug=False):
    """Host-side replay of the lock-step sweep of a block of T tiles (gpx_sweep_check);
    raises RuntimeError naming the first violation."""
    check(lib().gpx_sweep_check(int(T), int(bool(aug))))


def panel_solo_check(T, aug=False, full=False, value_only=False):
    """Host-side check that the task graph of T tiles in generation order is a sequential
    order (the list of a solo launch, gpx_panel_solo_check): number of tasks, or RuntimeError."""
    n = C.c_int(0)
    check(lib().gpx_panel_solo_check(int(T), int(bool(aug)), int(bool(full)), int(bool(value_only)),
                                     C.byref(n)))
    return n.value


def sweep_check_lite(T, aug=False, depth=-1):
    """... with the dense row panels of round 5 (gpx_sweep_check_lite): each tile right of
    (s, s+1) applies its last `depth` trailing updates itself (-1: the library's rule)."""
    check(lib().gpx_sweep_check_lite(int(T), int(bool(aug)), int(depth)))


def panel_graph_check_rhs(T, workers=64):
    """The task graph of a launch over a whole matrix of T tiles with a right-hand-side
    tile column (gpx_panel_graph_check_rhs): number of tasks, or RuntimeError."""
    n = C.c_int(0)
    check(lib().gpx_panel_graph_check_rhs(int(T), int(workers), C.byref(n)))
    return n.value


def panel_graph_check_full(T, workers=64):
    """... with the whole of R^-1 assembled inside the launch (gpx_panel_graph_check_full)."""
    n = C.c_int(0)
    check(lib().gpx_panel_graph_check_full(int(T), int(workers), C.byref(n)))
    return n.value


def panel_graph_check(T, workers=64, stream=True, extra=0):
    """Host-side self-check of the diagonal-panel kernel's task graph for a block of T
    128-tiles (no GPU), optionally as a wide panel with `extra` more tile columns:
    returns the number of tasks, raises RuntimeError naming the first violation (see
    gpx_panel_graph_check in include/gpx.h)."""
    n = C.c_int(0)
    if extra:
        check(lib().gpx_panel_graph_check_wide(int(T), int(extra), int(workers), C.byref(n)))
    else:
        check(lib().gpx_panel_graph_check(int(T), int(workers), int(bool(stream)), C.byref(n)))
    return n.value


_default = None


def default_handle():
    """Process-wide handle used by Kernel.get()/grad() (device from GPX_DEVICE
    or LOCAL_RANK, default 0)."""
    global _default
    if _default is None:
        with _lock:
            if _default is None:
                _default = Handle()
    return _default
