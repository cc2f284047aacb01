"""ctypes binding of libtpe_engine.so (include/tpe_engine.h).

This is the only place the Python host touches the HIP engine.  There is no
CPU fallback: if the library or a gfx950 device is missing, ``Engine()``
raises ``EngineUnavailable`` and the TPE suggest path fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TPE_ENGINE_LIB', os.path.join(_HERE, 'libtpe_engine.so'))

# ---- constants mirrored from include/tpe_engine.h -----------------------
TPE_OK = 0
TPE_E_INVALID = -1
TPE_E_BOUNDS = -2
TPE_E_NEGATIVE = -3
TPE_E_NOMEM = -4
TPE_E_HIP = -5
TPE_E_NODEVICE = -6
TPE_E_INDEX = -7

GMM, LGMM, CAT = 0, 1, 2
HAS_LOW, HAS_HIGH, HAS_Q, PCHOICE = 1, 2, 4, 8
OBS_IDENT, OBS_LOG, OBS_LOG_CLIP_EXPLOW, OBS_LOG_CLIP_EPS = 0, 1, 2, 3
KIND_NAMES = ('lse_gmm', 'lse_lgmm', 'erf_gmm', 'erf_lgmm', 'categorical')

# every symbol include/tpe_engine.h declares (checked by tests)
EXPORTS = (
    'tpe_version', 'tpe_device_count', 'tpe_create', 'tpe_destroy', 'tpe_last_error',
    'tpe_synchronize', 'tpe_split', 'tpe_parzen_fit', 'tpe_categorical_posterior',
    'tpe_lpdf', 'tpe_score', 'tpe_sample', 'tpe_plan_create', 'tpe_plan_destroy',
    'tpe_plan_num_levels', 'tpe_plan_set_history', 'tpe_plan_fit', 'tpe_plan_get_mixture',
    'tpe_plan_get_table',
    'tpe_plan_suggest', 'tpe_plan_suggest_shard', 'tpe_plan_merge', 'tpe_plan_score_candidates', 'tpe_plan_last_stats',
    'tpe_plan_profile', 'tpe_plan_profile_read', 'tpe_microbench', 'tpe_plan_get_results',
    'tpe_plan_results_device', 'tpe_plan_census', 'tpe_plan_fit_suggest',
    'tpe_plan_set_lattice', 'tpe_plan_update_history', 'tpe_plan_set_prune',
    'tpe_plan_sample_prior', 'tpe_plan_score_candidates_sorted', 'tpe_plan_census_n',
    'tpe_plan_tie_counts', 'tpe_plan_tab_wmax', 'tpe_plan_anneal', 'tpe_plan_anneal_trace',
    'tpe_plan_set_anneal_order', 'tpe_plan_tab_bound', 'tpe_plan_tab_hot',
    'tpe_plan_tab_panels', 'tpe_plan_tab_cert', 'tpe_plan_tie_list',
    'tpe_plan_cand_dump', 'tpe_plan_draw_screen_stats', 'tpe_plan_score_points',
    'tpe_plan_sample_points', 'tpe_plan_topk_points', 'tpe_plan_gather_points',
    'tpe_plan_joint_fit', 'tpe_plan_joint_get_mixture', 'tpe_plan_joint_score_points',
    'tpe_plan_joint_sides', 'tpe_plan_joint_sample_points', 'tpe_math_probe',
    'tpe_plan_group_info', 'tpe_plan_group_fit', 'tpe_plan_group_get_mixture',
    'tpe_plan_group_score_points', 'tpe_plan_group_sides', 'tpe_plan_group_sample_points',
    'tpe_plan_group_batch_points',
    'tpe_plan_set_objectives', 'tpe_plan_pareto_get', 'tpe_plan_pareto_shape',
    'tpe_plan_set_hv', 'tpe_plan_hv_get',
)

BATCH_MAX = 1024            # tpe_plan_group_batch_points' largest k
MAX_OBJ = 8                 # include/tpe_engine.h TPE_MAX_OBJ

# include/tpe_engine.h TPE_SHARD_ALIGN: candidate splits at multiples of this
# give byte-identical suggests (the large-draw value-bucketing block)
SHARD_ALIGN = 8192


class EngineUnavailable(RuntimeError):
    """The HIP engine library or an MI355X (gfx950) device is not available."""


class EngineError(RuntimeError):
    pass


class TpeHp(C.Structure):
    _fields_ = [('family', C.c_int32), ('flags', C.c_uint32), ('obs_transform', C.c_int32),
                ('upper', C.c_int32), ('prior_mu', C.c_double), ('prior_sigma', C.c_double),
                ('low', C.c_double), ('high', C.c_double), ('q', C.c_double),
                ('cond_begin', C.c_int32), ('cond_count', C.c_int32),
                ('pprior_begin', C.c_int64)]


class TpeSpace(C.Structure):
    _fields_ = [('n_hp', C.c_int32), ('hp', C.POINTER(TpeHp)), ('n_cond', C.c_int32),
                ('cond_parent', C.POINTER(C.c_int32)), ('cond_branch', C.POINTER(C.c_int32)),
                ('n_pprior', C.c_int64), ('pprior', C.POINTER(C.c_double))]


RESULT_DTYPE = np.dtype([('score', '<f8'), ('value', '<f8'), ('index', '<i8'),
                         ('active', '<i4'), ('pad', '<i4')])
# tpe_anneal_trace
ANNEAL_TRACE_DTYPE = np.dtype([('row', '<i4'), ('rank', '<i4'), ('u', '<f8', (4,))])

_D = C.POINTER(C.c_double)
_lib = None
_lib_lock = threading.Lock()


def _share_hip_runtime():
    """Make the engine and PyTorch use ONE HIP runtime.

    libtpe_engine.so needs ``libamdhip64.so.7``; PyTorch-ROCm ships its own
    copy (same soname) and loads it by file name.  Whichever loads second
    would bring a second runtime into the process, and the second one sees no
    GPU.  Pre-loading torch's copy (without importing torch) makes the engine
    bind to it, so torch tensors and engine launches share one runtime.
    TPE_ENGINE_HIP_RUNTIME=system keeps /opt/rocm's runtime instead."""
    if os.environ.get('TPE_ENGINE_HIP_RUNTIME', '') == 'system':
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    hip = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if os.path.exists(hip):
        C.CDLL(hip, mode=C.RTLD_GLOBAL)


def load_library(path: str = LIB_PATH):
    """Load libtpe_engine.so and declare its signatures (no device needed)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise EngineUnavailable(
                'libtpe_engine.so not found at %s: build it with `make -C '
                'hyperopt_amd/csrc` or __graft_entry__.build()' % path)
        _share_hip_runtime()
        lib = C.CDLL(path)
        vp, i32, i64, u32, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
        sig = {
            'tpe_version': (C.c_char_p, []),
            'tpe_device_count': (C.c_int, [C.POINTER(i32)]),
            'tpe_create': (C.c_int, [i32, C.POINTER(vp)]),
            'tpe_destroy': (C.c_int, [vp]),
            'tpe_last_error': (C.c_char_p, [vp]),
            'tpe_synchronize': (C.c_int, [vp]),
            'tpe_split': (C.c_int, [vp, _D, i64, dbl, i32, C.POINTER(C.c_uint8)]),
            'tpe_parzen_fit': (C.c_int, [vp, _D, i64, dbl, dbl, dbl, i32, _D, _D, _D]),
            'tpe_categorical_posterior': (C.c_int, [vp, C.POINTER(i64), i64, i32, dbl, _D, i32, _D]),
            'tpe_lpdf': (C.c_int, [vp, i32, _D, i64, _D, _D, _D, i64, dbl, dbl, dbl, u32, _D]),
            'tpe_score': (C.c_int, [vp, i32, _D, i64, _D, _D, _D, i64, _D, _D, _D, i64,
                                    dbl, dbl, dbl, u32, _D, _D, C.POINTER(i64), _D]),
            'tpe_sample': (C.c_int, [vp, i32, _D, _D, _D, i64, dbl, dbl, dbl, u32, u64, u64,
                                     i64, i64, _D]),
            'tpe_plan_create': (C.c_int, [vp, C.POINTER(TpeSpace), i64, C.POINTER(vp)]),
            'tpe_plan_destroy': (C.c_int, [vp]),
            'tpe_plan_num_levels': (C.c_int, [vp, C.POINTER(i32)]),
            'tpe_plan_set_history': (C.c_int, [vp, vp, vp, vp, i64, i32, vp]),
            'tpe_plan_update_history': (C.c_int, [vp, i64, i64, i64, vp, vp, i64, i64, vp, i32,
                                                  vp]),
            'tpe_plan_fit': (C.c_int, [vp, dbl, i32, dbl, i32, vp]),
            'tpe_plan_get_mixture': (C.c_int, [vp, i32, i32, _D, _D, _D, i64, C.POINTER(i64)]),
            'tpe_plan_get_table': (C.c_int, [vp, i32, i32, i32, vp, i64, C.POINTER(i64)]),
            'tpe_plan_suggest': (C.c_int, [vp, C.POINTER(u64), i64, i64, i64, i32, vp, i32, vp]),
            'tpe_plan_suggest_shard': (C.c_int, [vp, C.POINTER(u64), i64, i64, i64, i64, i32, vp,
                                                 i32, vp]),
            'tpe_plan_fit_suggest': (C.c_int, [vp, dbl, i32, dbl, i32, C.POINTER(u64), i64, i64,
                                               vp, i32, vp]),
            'tpe_plan_merge': (C.c_int, [vp, vp, i32, i32, vp, i32, vp]),
            'tpe_plan_score_candidates': (C.c_int, [vp, i32, _D, i64, _D, _D, C.POINTER(i64), _D]),
            'tpe_plan_score_candidates_sorted': (C.c_int, [vp, i32, i32, _D, i64, _D, _D,
                                                           C.POINTER(i64), _D]),
            'tpe_plan_score_points': (C.c_int, [vp, vp, i64, i64, vp, vp, vp, i32, vp]),
            'tpe_plan_sample_points': (C.c_int, [vp, u64, i64, i64, i64, vp, vp, vp, vp, i32, vp]),
            'tpe_plan_topk_points': (C.c_int, [vp, vp, vp, i64, i32, vp, i32, vp]),
            'tpe_plan_joint_fit': (C.c_int, [vp, vp]),
            'tpe_plan_joint_get_mixture': (C.c_int, [vp, i32, i32, _D, _D, _D, vp, i64,
                                                     C.POINTER(i64)]),
            'tpe_plan_joint_score_points': (C.c_int, [vp, vp, i64, i64, vp, vp, vp, vp, i32, vp]),
            'tpe_plan_joint_sides': (C.c_int, [vp, vp, vp, i64]),
            'tpe_plan_joint_sample_points': (C.c_int, [vp, u64, i64, i64, i64, vp, vp, vp, vp, vp,
                                                       vp, i32, vp]),
            'tpe_plan_group_info': (C.c_int, [vp, vp, C.POINTER(i32)]),
            'tpe_plan_group_fit': (C.c_int, [vp, vp]),
            'tpe_plan_group_get_mixture': (C.c_int, [vp, i32, i32, i32, _D, _D, _D, vp, i64,
                                                     C.POINTER(i64)]),
            'tpe_plan_group_score_points': (C.c_int, [vp, vp, i64, i64, vp, vp, vp, i32, vp]),
            'tpe_plan_group_sides': (C.c_int, [vp, i32, vp, vp, i64]),
            'tpe_plan_group_sample_points': (C.c_int, [vp, u64, i64, i64, i64, vp, vp, vp, vp, vp,
                                                       i32, vp]),
            'tpe_plan_group_batch_points': (C.c_int, [vp, vp, i64, i64, vp, i32, vp, vp, vp, i32,
                                                      vp]),
            'tpe_plan_gather_points': (C.c_int, [vp, vp, i64, vp, i32, vp, i32, vp]),
            'tpe_plan_set_objectives': (C.c_int, [vp, vp, i32, i64, i64, i64, i32, vp]),
            'tpe_plan_pareto_get': (C.c_int, [vp, vp, vp, vp, i64]),
            'tpe_plan_pareto_shape': (C.c_int, [vp, i64, i32, i64, C.POINTER(i64)]),
            'tpe_plan_set_hv': (C.c_int, [vp, i32, vp, i32, i32, i32, C.c_uint64, i32]),
            'tpe_plan_hv_get': (C.c_int, [vp, vp, vp, vp, C.POINTER(i32), i32]),
            'tpe_plan_last_stats': (C.c_int, [vp, _D, _D]),
            'tpe_plan_profile': (C.c_int, [vp, i32]),
            'tpe_plan_profile_read': (C.c_int, [vp, i32, _D, C.POINTER(i64), _D]),
            'tpe_microbench': (C.c_int, [vp, i32, _D]),
            'tpe_math_probe': (C.c_int, [vp, i32, _D, i64, _D]),
            'tpe_plan_get_results': (C.c_int, [vp, vp, i32, vp]),
            'tpe_plan_results_device': (vp, [vp]),
            'tpe_plan_census': (C.c_int, [vp, i32, C.POINTER(i64)]),
            'tpe_plan_census_n': (C.c_int, [vp, i32, C.POINTER(i64), i32]),
            'tpe_plan_tie_counts': (C.c_int, [vp, i32, vp]),
            'tpe_plan_tab_wmax': (C.c_int, [vp, i32, vp]),
            'tpe_plan_tab_bound': (C.c_int, [vp, i32, vp]),
            'tpe_plan_tab_hot': (C.c_int, [vp, i32, vp]),
            'tpe_plan_tab_panels': (C.c_int, [vp, i32, i32, vp, vp, vp, vp]),
            'tpe_plan_tab_cert': (C.c_int, [vp, i32, i32, vp]),
            'tpe_plan_tie_list': (C.c_int, [vp, i32, i32, vp]),
            'tpe_plan_cand_dump': (C.c_int64, [vp, i32, i32, vp, vp]),
            'tpe_plan_draw_screen_stats': (C.c_int, [vp, vp]),
            'tpe_plan_set_lattice': (C.c_int, [vp, i32]),
            'tpe_plan_set_prune': (C.c_int, [vp, i32]),
            'tpe_plan_sample_prior': (C.c_int, [vp, C.POINTER(u64), i64, vp, i32, vp]),
            'tpe_plan_anneal': (C.c_int, [vp, dbl, dbl, C.POINTER(u64), i64, vp, i32, vp]),
            'tpe_plan_anneal_trace': (C.c_int, [vp, i32, vp]),
            'tpe_plan_set_anneal_order': (C.c_int, [vp, C.POINTER(i32), i32]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def _seeds(seeds):
    """uint64 seed array (exact: a mixed list of Python ints would round
    through float64 in np.asarray)."""
    seeds = [int(x) & (2 ** 64 - 1) for x in np.atleast_1d(np.asarray(seeds, dtype=object))]
    return np.fromiter(seeds, dtype=np.uint64, count=len(seeds))


def _dp(a):
    return None if a is None else a.ctypes.data_as(_D)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Engine(object):
    """One HIP device bound to the TPE engine (tpe_create)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        n = C.c_int32(0)
        self.lib.tpe_device_count(C.byref(n))
        if n.value <= 0:
            raise EngineUnavailable('no HIP device visible (TPE engine needs an MI355X)')
        h = C.c_void_p()
        rc = self.lib.tpe_create(int(device), C.byref(h))
        if rc != TPE_OK:
            raise EngineUnavailable('tpe_create(%d) failed (%d): not a gfx950 device?' % (device, rc))
        self.h = h
        self.device = device
        self.lock = threading.RLock()

    def close(self):
        if getattr(self, 'h', None):
            self.lib.tpe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- error mapping onto the reference's exceptions ---------------------
    def check(self, rc):
        if rc == TPE_OK:
            return
        msg = (self.lib.tpe_last_error(self.h) or b'').decode()
        if rc == TPE_E_BOUNDS:
            raise ValueError('low >= high', msg)                 # tpe.py:80-81
        if rc == TPE_E_NEGATIVE:
            raise ValueError('negative arg to lognormal_cdf', msg)  # tpe.py:181-182
        if rc == TPE_E_INDEX:
            raise IndexError(msg)
        if rc == TPE_E_INVALID:
            raise ValueError(msg)
        raise EngineError('TPE engine error %d: %s' % (rc, msg))

    def synchronize(self):
        """Wait for all of this engine's device work (tpe_synchronize)."""
        with self.lock:
            self.check(self.lib.tpe_synchronize(self.h))

    def microbench(self, which):
        r = C.c_double(0)
        with self.lock:
            self.check(self.lib.tpe_microbench(self.h, int(which), C.byref(r)))
        return r.value

    def math_probe(self, which, x):
        """A device math helper on the arguments x (tpe_math_probe): 0
        fast_log, 1 fast_log2, 2 erfcinv_fast, 3 erfc; wave j evaluates
        x.ravel()[64 j : 64 j + 64]."""
        xa = _f64(x)
        xs = xa.ravel()
        out = np.empty(xs.size)
        with self.lock:
            self.check(self.lib.tpe_math_probe(self.h, int(which), _dp(xs), xs.size, _dp(out)))
        return out.reshape(xa.shape)

    # -- operator level ----------------------------------------------------
    def split(self, losses, gamma, gamma_cap=25):
        losses = _f64(losses)
        out = np.zeros(losses.size, dtype=np.uint8)
        with self.lock:
            self.check(self.lib.tpe_split(self.h, _dp(losses), losses.size, float(gamma),
                                          int(gamma_cap), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.astype(bool)

    def parzen_fit(self, obs, prior_weight, prior_mu, prior_sigma, lf=25):
        obs = _f64(obs).ravel()
        k = obs.size + 1
        w, mu, sg = np.empty(k), np.empty(k), np.empty(k)
        with self.lock:
            self.check(self.lib.tpe_parzen_fit(self.h, _dp(obs), obs.size, float(prior_weight),
                                               float(prior_mu), float(prior_sigma), int(lf),
                                               _dp(w), _dp(mu), _dp(sg)))
        return w, mu, sg

    def categorical_posterior(self, obs, upper, prior_weight, p_prior=None, lf=25):
        obs = np.ascontiguousarray(obs, dtype=np.int64).ravel()
        p = np.empty(int(upper))
        pp = None if p_prior is None else _f64(p_prior)
        with self.lock:
            self.check(self.lib.tpe_categorical_posterior(
                self.h, obs.ctypes.data_as(C.POINTER(C.c_int64)), obs.size, int(upper),
                float(prior_weight), _dp(pp), int(lf), _dp(p)))
        return p

    @staticmethod
    def _flags(low, high, q):
        f = 0
        if low is not None:
            f |= HAS_LOW
        if high is not None:
            f |= HAS_HIGH
        if q is not None:
            f |= HAS_Q
        return f

    def score(self, family, x, below, above, low=None, high=None, q=None, want_llik=True):
        """Fused lpdf(below), lpdf(above), argmax(below - above)."""
        x = _f64(x).ravel()
        if family == CAT:
            wb, mb, sb = _f64(below), None, None
            wa, ma, sa = _f64(above), None, None
        else:
            wb, mb, sb = (_f64(a) for a in below)
            wa, ma, sa = (_f64(a) for a in above)
        lb = np.empty(x.size) if want_llik else None
        la = np.empty(x.size) if want_llik else None
        bi, bs = C.c_int64(-1), C.c_double(np.nan)
        with self.lock:
            self.check(self.lib.tpe_score(
                self.h, family, _dp(x), x.size, _dp(wb), _dp(mb), _dp(sb), wb.size,
                _dp(wa), _dp(ma), _dp(sa), wa.size,
                float(low) if low is not None else 0.0, float(high) if high is not None else 0.0,
                float(q) if q is not None else 0.0, self._flags(low, high, q),
                _dp(lb), _dp(la), C.byref(bi), C.byref(bs)))
        return lb, la, bi.value, bs.value

    def lpdf(self, family, x, w, mu=None, sigma=None, low=None, high=None, q=None):
        xa = _f64(x)
        xs = xa.ravel()
        w = _f64(w)
        mu = None if mu is None else _f64(mu)
        sigma = None if sigma is None else _f64(sigma)
        out = np.empty(xs.size)
        with self.lock:
            self.check(self.lib.tpe_lpdf(
                self.h, family, _dp(xs), xs.size, _dp(w), _dp(mu), _dp(sigma), w.size,
                float(low) if low is not None else 0.0, float(high) if high is not None else 0.0,
                float(q) if q is not None else 0.0, self._flags(low, high, q), _dp(out)))
        return out.reshape(xa.shape)

    def sample(self, family, w, mu=None, sigma=None, low=None, high=None, q=None, seed=0,
               stream=0, offset=0, n=1):
        w = _f64(w)
        mu = None if mu is None else _f64(mu)
        sigma = None if sigma is None else _f64(sigma)
        out = np.empty(int(n))
        with self.lock:
            self.check(self.lib.tpe_sample(
                self.h, family, _dp(w), _dp(mu), _dp(sigma), w.size,
                float(low) if low is not None else 0.0, float(high) if high is not None else 0.0,
                float(q) if q is not None else 0.0, self._flags(low, high, q),
                int(seed) & (2 ** 64 - 1), int(stream), int(offset), int(n), _dp(out)))
        return out


class DeviceBuffer(object):
    """A plain device allocation on ``engine``'s GPU, through the HIP runtime
    the engine library itself is linked against (resolved through the library's
    handle, so both use one runtime).  For data that stays on the device
    between engine calls -- a candidate pool -- without PyTorch.  ``upload`` /
    ``download`` are blocking copies; call ``engine.synchronize()`` before
    reading what a stream-ordered engine call wrote."""

    def __init__(self, engine: Engine, nbytes: int):
        self.engine = engine
        self.nbytes = int(nbytes)
        lib = engine.lib
        lib.hipMalloc.restype = C.c_int
        lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        lib.hipFree.restype = C.c_int
        lib.hipFree.argtypes = [C.c_void_p]
        lib.hipMemcpy.restype = C.c_int
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        p = C.c_void_p()
        with engine.lock:
            engine.check(lib.tpe_synchronize(engine.h))     # (makes the engine's device current)
            rc = lib.hipMalloc(C.byref(p), max(self.nbytes, 1))
        if rc != 0 or not p.value:
            raise EngineError('hipMalloc of %d bytes failed (%d)' % (self.nbytes, rc))
        self.ptr = p.value

    def _copy(self, dst, src, nbytes, kind):
        if nbytes > self.nbytes:
            raise ValueError('copy of %d bytes exceeds the buffer (%d)' % (nbytes, self.nbytes))
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_synchronize(e.h))
            rc = e.lib.hipMemcpy(dst, src, nbytes, kind)
        if rc != 0:
            raise EngineError('hipMemcpy failed (%d)' % rc)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        self._copy(self.ptr, arr.ctypes.data, arr.nbytes, 1)     # hipMemcpyHostToDevice
        return self

    def download(self, out):
        assert out.flags.c_contiguous
        self._copy(out.ctypes.data, self.ptr, out.nbytes, 2)     # hipMemcpyDeviceToHost
        return out

    def close(self):
        if getattr(self, 'ptr', None):
            if getattr(self.engine, 'h', None):     # (a closed engine has released its device)
                self.engine.lib.hipFree(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan(object):
    """A compiled search space with a device-resident history (tpe_plan_*)."""

    def __init__(self, engine: Engine, hps, conds, pprior, max_trials):
        self.engine = engine
        lib = engine.lib
        self.n_hp = len(hps)
        arr = (TpeHp * self.n_hp)(*hps)
        cp = np.ascontiguousarray([c[0] for c in conds], dtype=np.int32)
        cb = np.ascontiguousarray([c[1] for c in conds], dtype=np.int32)
        pp = _f64(pprior if len(pprior) else np.zeros(0))
        sp = TpeSpace(self.n_hp, arr, len(conds), cp.ctypes.data_as(C.POINTER(C.c_int32)),
                      cb.ctypes.data_as(C.POINTER(C.c_int32)), pp.size, _dp(pp))
        self._keep = (arr, cp, cb, pp)
        p = C.c_void_p()
        with engine.lock:
            engine.check(lib.tpe_plan_create(engine.h, C.byref(sp), int(max_trials), C.byref(p)))
        self.p = p
        self.max_trials = int(max_trials)
        self.anneal_order = None
        nl = C.c_int32(0)
        lib.tpe_plan_num_levels(p, C.byref(nl))
        self.n_levels = nl.value

    def close(self):
        if getattr(self, 'p', None):
            self.engine.lib.tpe_plan_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_history(self, losses, vals, active, stream=None):
        """Whole history from host arrays: losses[n], vals[n_hp, n] float64,
        active[n_hp, n] uint8."""
        losses = _f64(losses)
        vals = _f64(vals)
        active = np.ascontiguousarray(active, dtype=np.uint8)
        n = losses.size
        assert vals.shape == (self.n_hp, n) and active.shape == (self.n_hp, n)
        self.update_history(n, 0, vals, active, n, 0, losses, stream=stream)

    def update_history(self, n, row0, vals, active, ld, loss0, losses, stream=None):
        """Incremental history (tpe_plan_update_history): rows [row0, n) of
        the host columns vals[n_hp, ld] / active[n_hp, ld] (C-contiguous) and
        losses[loss0:n]; rows below row0 stay as the device has them."""
        e = self.engine
        if n > self.max_trials:
            raise ValueError('history of %d trials exceeds the plan capacity %d'
                             % (n, self.max_trials))
        if vals.dtype != np.float64 or active.dtype != np.uint8 or \
                not vals.flags.c_contiguous or not active.flags.c_contiguous or \
                vals.shape != (self.n_hp, ld) or active.shape != (self.n_hp, ld):
            raise ValueError('history columns must be C-contiguous [n_hp, ld] f64 / u8')
        losses = np.asarray(losses)
        if losses.dtype != np.float64 or not losses.flags.c_contiguous:
            raise ValueError('losses must be C-contiguous float64')
        nr = n - row0
        vp = vals.ctypes.data + 8 * row0 if nr > 0 else None
        ap = active.ctypes.data + row0 if nr > 0 else None
        lp = losses.ctypes.data + 8 * loss0 if loss0 < n else None
        self._hist = (vals, active, losses)   # keep the host memory alive
        with e.lock:
            e.check(e.lib.tpe_plan_update_history(self.p, int(n), int(row0), int(nr), vp, ap,
                                                  int(ld), int(loss0), lp, 0, stream))
        self.n = int(n)

    def set_history_device(self, losses_ptr, vals_ptr, active_ptr, n, stream=None):
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_set_history(self.p, losses_ptr, vals_ptr, active_ptr, int(n),
                                               1, stream))
        self.n = int(n)

    # ---- multi-objective TPE: the loss column from a Pareto ranking
    def set_objectives(self, Y, n=None, obj0=0, stream=None):
        """Rank the history by Pareto dominance (tpe_plan_set_objectives):
        ``Y`` float64 [M, ld] C-contiguous, objective m of row r at
        ``Y[m, r]``; rows [obj0, n) are copied (the rows below are the last
        call's), all n rows are counted and the loss column of rows [0, n)
        becomes the surrogate loss.  ``n`` (default ld) must be the history
        length."""
        e = self.engine
        Y = np.asarray(Y)
        if Y.ndim != 2 or Y.dtype != np.float64 or not Y.flags.c_contiguous:
            raise ValueError('objectives must be a C-contiguous float64 [M, ld] array')
        m, ld = Y.shape
        n = ld if n is None else int(n)
        obj0 = int(obj0)
        if n > ld or not 0 <= obj0 <= n:
            raise ValueError('need 0 <= obj0 <= n <= ld')
        # (the source rows start at obj0: the leading dimension stays ld)
        ptr = (Y.ctypes.data + 8 * obj0) if ld > 0 else None
        with e.lock:
            e.check(e.lib.tpe_plan_set_objectives(self.p, ptr, int(m), n, int(ld), obj0, 0,
                                                  stream))

    def set_objectives_device(self, y_ptr, n_obj, n, ld, obj0=0, stream=None):
        """The same from device memory: ``y_ptr`` points at row obj0 of
        objective 0, objective m of row r at y_ptr[m * ld + (r - obj0)].
        Stream-ordered, no host synchronisation."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_set_objectives(self.p, y_ptr, int(n_obj), int(n), int(ld),
                                                  int(obj0), 1, stream))

    def pareto_get(self, n):
        """(dominated_by int32[n], dominates int32[n], surrogate float64[n])
        of the last ``set_objectives`` (tpe_plan_pareto_get)."""
        e = self.engine
        n = int(n)
        by = np.empty(max(n, 0), dtype=np.int32)
        of = np.empty(max(n, 0), dtype=np.int32)
        s = np.empty(max(n, 0))
        with e.lock:
            e.check(e.lib.tpe_plan_pareto_get(self.p, by.ctypes.data, of.ctypes.data,
                                              s.ctypes.data, n))
        return by, of, s

    def pareto_shape(self, n, n_obj, force_splits=-1):
        """(rows per tile, TPE_MAX_OBJ, j-splits, tiles) of the ranking launch
        for ``n`` rows of ``n_obj`` objectives (tpe_plan_pareto_shape).
        ``force_splits`` > 0 makes this plan's later ``set_objectives`` calls
        take that many j-splits (tests), 0 restores the default, -1 leaves the
        setting."""
        e = self.engine
        out = (C.c_int64 * 4)()
        with e.lock:
            e.check(e.lib.tpe_plan_pareto_shape(self.p, int(n), int(n_obj), int(force_splits),
                                                out))
        return tuple(int(v) for v in out)

    # ---- hypervolume subset selection inside the front
    def set_hv(self, ref, n_obj=None, n_pick=32, n_samples=1024, seed=0, method=0):
        """The setting the next ``set_objectives`` reads (tpe_plan_set_hv):
        ``ref`` None turns the mode off; a sequence of ``n_obj`` (default its
        length) finite floats is the reference point of the greedy hypervolume
        subset selection inside the Pareto front, ``n_pick`` rounds,
        ``n_samples`` Monte-Carlo samples per row from the Philox stream of
        ``seed``; ``method`` 0 auto (exact with two objectives), 1 exact,
        2 Monte-Carlo."""
        e = self.engine
        with e.lock:
            if ref is None:
                e.check(e.lib.tpe_plan_set_hv(self.p, 0, None, 0, 0, 0, 0, 0))
                self._hv_on = False
                return
            r = np.ascontiguousarray(ref, dtype=np.float64).reshape(-1)
            m = len(r) if n_obj is None else int(n_obj)
            if m > len(r):
                raise ValueError('the reference point has fewer than n_obj entries')
            e.check(e.lib.tpe_plan_set_hv(self.p, 1, r.ctypes.data, m, int(n_pick),
                                          int(n_samples), int(seed) & (2 ** 64 - 1),
                                          int(method)))
            self._hv_on = True

    def hv_get(self, cap=256):
        """(picks int32[k], keys float64[k], counts int32[k], R) of the last
        ranking's selection (tpe_plan_hv_get), k = min(cap, its n_pick): rows in
        pick order (-1 from round R on), each pick's key as the device holds it
        (Monte-Carlo: vol * alive, not divided by the sample count) and its
        alive samples (-1 on the exact path).  R = 0 and empty arrays when that
        ranking ran no selection."""
        e = self.engine
        cap = int(cap)
        picks = np.full(max(cap, 0), -2, dtype=np.int32)
        keys = np.zeros(max(cap, 0))
        counts = np.zeros(max(cap, 0), dtype=np.int32)
        R = C.c_int32(0)
        with e.lock:
            e.check(e.lib.tpe_plan_hv_get(self.p, picks.ctypes.data, keys.ctypes.data,
                                          counts.ctypes.data, C.byref(R), cap))
        k = int(np.count_nonzero(picks != -2))      # (entries the engine wrote)
        return picks[:k], keys[:k], counts[:k], int(R.value)

    def fit(self, gamma=0.25, prior_weight=1.0, lf=25, gamma_cap=25, stream=None):
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_fit(self.p, float(gamma), int(gamma_cap), float(prior_weight),
                                       int(lf), stream))

    def mixture(self, hp, side=0):
        e = self.engine
        cap = max(self.max_trials + 1, 1)
        # categorical hps may have more categories than trials
        cap = max(cap, 1 << 16)
        w, mu, sg = np.empty(cap), np.empty(cap), np.empty(cap)
        k = C.c_int64(0)
        with e.lock:
            e.check(e.lib.tpe_plan_get_mixture(self.p, int(hp), int(side), _dp(w), _dp(mu),
                                               _dp(sg), cap, C.byref(k)))
        k = k.value
        return w[:k].copy(), mu[:k].copy(), sg[:k].copy()

    def table(self, hp, side=0, which=2):
        """Raw scoring table of slot (hp, side) as bytes (tpe_plan_get_table:
        0 coefficients, 1 block-local fp32, 2 moment chunks, 3 8-wide moment
        blocks, 4 degree-15 moment chunks; diagnostics)."""
        e = self.engine
        n = C.c_int64(0)
        with e.lock:
            e.check(e.lib.tpe_plan_get_table(self.p, int(hp), int(side), int(which), None, 0,
                                             C.byref(n)))
            buf = np.empty(n.value, dtype=np.uint8)
            e.check(e.lib.tpe_plan_get_table(self.p, int(hp), int(side), int(which),
                                             buf.ctypes.data, buf.size, C.byref(n)))
        return buf

    def suggest(self, seeds, n_cand, cand_begin=0, level=-1, out=None, stream=None, fetch=True,
                n_total=None):
        """Returns a structured array [n_suggest, n_hp] of RESULT_DTYPE (host)
        unless ``out`` is a device pointer (int) or ``fetch`` is False (the
        results stay in the plan: ``results_device_ptr()`` / ``results()``).
        ``n_total``: the candidate count of the whole suggestion when this
        call is a shard [cand_begin, cand_begin + n_cand) of it
        (tpe_plan_suggest_shard; default cand_begin + n_cand)."""
        e = self.engine
        seeds = _seeds(seeds)
        host = out is None and fetch
        res = np.empty((seeds.size, self.n_hp), dtype=RESULT_DTYPE) if host else None
        optr = res.ctypes.data if host else out
        total = int(cand_begin) + int(n_cand) if n_total is None else int(n_total)
        with e.lock:
            e.check(e.lib.tpe_plan_suggest_shard(
                self.p, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), seeds.size, total,
                int(cand_begin), int(n_cand), int(level), optr, 0 if host else 1, stream))
        self._last_nsug = seeds.size
        self._last_ncand = int(n_cand)
        return res

    def fit_suggest(self, seeds, n_cand, gamma=0.25, prior_weight=1.0, lf=25, gamma_cap=25,
                    out=None, stream=None, fetch=True):
        """fit() + suggest() over all levels in one engine call; repeated calls
        of one shape replay a captured hipGraph of the step (tpe_engine.h)."""
        e = self.engine
        seeds = _seeds(seeds)
        host = out is None and fetch
        res = np.empty((seeds.size, self.n_hp), dtype=RESULT_DTYPE) if host else None
        optr = res.ctypes.data if host else out
        with e.lock:
            e.check(e.lib.tpe_plan_fit_suggest(
                self.p, float(gamma), int(gamma_cap), float(prior_weight), int(lf),
                seeds.ctypes.data_as(C.POINTER(C.c_uint64)), seeds.size, int(n_cand),
                optr, 0 if host else 1, stream))
        self._last_nsug = seeds.size
        self._last_ncand = int(n_cand)
        return res

    def sample_prior(self, seeds, stream=None):
        """Prior draws of len(seeds) whole suggestions (rand.suggest on the
        device): [S, n_hp] RESULT_DTYPE, value/active per hp."""
        e = self.engine
        seeds = _seeds(seeds)
        res = np.empty((seeds.size, self.n_hp), dtype=RESULT_DTYPE)
        with e.lock:
            e.check(e.lib.tpe_plan_sample_prior(self.p, seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                seeds.size, res.ctypes.data, 0, stream))
        self._last_nsug = seeds.size
        return res

    def set_anneal_order(self, hp_order):
        """The order in which an anneal call walks the hps (hp indices of
        CompiledSpace.draw_order; tpe_plan_set_anneal_order), once per plan."""
        e = self.engine
        order = np.ascontiguousarray(hp_order, dtype=np.int32)
        with e.lock:
            e.check(e.lib.tpe_plan_set_anneal_order(
                self.p, order.ctypes.data_as(C.POINTER(C.c_int32)), order.size))
        self.anneal_order = order

    def anneal(self, seeds, avg_best_idx=2.0, shrink_coef=0.1, stream=None):
        """Annealing suggestions of len(seeds) independent annealers on the
        plan's history (tpe_plan_anneal): [S, n_hp] RESULT_DTYPE -- value,
        index = the anchor row, score = its loss (0, 0 for a prior draw)."""
        e = self.engine
        seeds = _seeds(seeds)
        res = np.empty((seeds.size, self.n_hp), dtype=RESULT_DTYPE)
        with e.lock:
            e.check(e.lib.tpe_plan_anneal(self.p, float(avg_best_idx), float(shrink_coef),
                                          seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          seeds.size, res.ctypes.data, 0, stream))
        self._last_nsug = seeds.size
        return res

    def anneal_trace(self, n_suggest):
        """Debug (tpe_plan_anneal_trace): [n_suggest, n_hp] ANNEAL_TRACE_DTYPE
        of the last anneal call -- anchor row, clipped rank of a fresh anchor,
        the uniforms each hp consumed."""
        e = self.engine
        out = np.empty((int(n_suggest), self.n_hp), dtype=ANNEAL_TRACE_DTYPE)
        with e.lock:
            e.check(e.lib.tpe_plan_anneal_trace(self.p, int(n_suggest), out.ctypes.data))
        return out

    def results(self):
        e = self.engine
        res = np.empty((getattr(self, '_last_nsug', 1), self.n_hp), dtype=RESULT_DTYPE)
        with e.lock:
            e.check(e.lib.tpe_plan_get_results(self.p, res.ctypes.data, 0, None))
        return res

    def get_results(self, out, stream=None):
        """Copy the last suggest's records to the device pointer ``out``
        (tpe_plan_get_results, stream-ordered)."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_get_results(self.p, out, 1, stream))

    def results_device_ptr(self):
        return self.engine.lib.tpe_plan_results_device(self.p)

    def merge(self, gathered_ptr, world, level, out=None, stream=None, n_suggest=1,
              in_place=False):
        """tpe_plan_merge; in_place: ``out`` (device) already holds the
        level's suggest records (suggest(..., out=out)), only the merged
        slots are stored into it (out_on_device 2, no copy launch)."""
        e = self.engine
        host = out is None
        res = np.empty((n_suggest, self.n_hp), dtype=RESULT_DTYPE) if host else None
        optr = res.ctypes.data if host else out
        mode = 0 if host else (2 if in_place else 1)
        with e.lock:
            e.check(e.lib.tpe_plan_merge(self.p, gathered_ptr, int(world), int(level), optr,
                                         mode, stream))
        return res

    def score_candidates(self, hp, x, sorted_mode=None, want_llik=True):
        """Below / above lpdf and argmax of given candidates of one hp with
        the fitted mixtures.  sorted_mode None: each candidate scored on its
        own (exact sums); 0 / 1 / 2 / 3: the large-draw production form
        (tpe_plan_score_candidates_sorted: value-bucketed blocks, log-sum-exp
        prune mode 0 / 1 / 2 / 3; 4: mode 3's tiles scored from the hp's
        certified Chebyshev tables, an error if either is not).  want_llik False: no lpdf outputs -- the
        scorer then takes the suggest's EI-only finalize (one log2 of the
        ratio of the two sums) and (None, None, index, score) is returned."""
        e = self.engine
        x = _f64(x).ravel()
        lb, la = (np.empty(x.size), np.empty(x.size)) if want_llik else (None, None)
        bi, bs = C.c_int64(-1), C.c_double(np.nan)
        mode = -1 if sorted_mode is None else int(sorted_mode)
        with e.lock:
            e.check(e.lib.tpe_plan_score_candidates_sorted(
                self.p, int(hp), mode, _dp(x), x.size, _dp(lb) if want_llik else None,
                _dp(la) if want_llik else None, C.byref(bi), C.byref(bs)))
        return lb, la, bi.value, bs.value

    def score_points(self, vals, want_terms=False, want_active=False, stream=None):
        """EI of M whole configurations under the last fit
        (tpe_plan_score_points): ``vals`` float64 [n_hp, M] in the history's
        columnar layout, values of inactive hps ignored (NaN allowed).
        Returns total[M], or (total[, terms[n_hp, M]][, active[n_hp, M]
        uint8]) with the ``want_`` flags: terms[i] = below_llik - above_llik
        of hp i (+0.0 where inactive), total their sum in hp order."""
        e = self.engine
        vals = _f64(vals)
        if vals.ndim != 2 or vals.shape[0] != self.n_hp:
            raise ValueError('configurations must be a [n_hp, M] array')
        m = vals.shape[1]
        total = np.empty(m)
        terms = np.empty((self.n_hp, m)) if want_terms else None
        active = np.empty((self.n_hp, m), dtype=np.uint8) if want_active else None
        with e.lock:
            e.check(e.lib.tpe_plan_score_points(
                self.p, vals.ctypes.data, m, m, total.ctypes.data,
                terms.ctypes.data if want_terms else None,
                active.ctypes.data if want_active else None, 0, stream))
        out = (total,) + ((terms,) if want_terms else ()) + ((active,) if want_active else ())
        return out[0] if len(out) == 1 else out

    def score_points_device(self, vals_ptr, m, ld, total_ptr, terms_ptr=0, active_ptr=0,
                            stream=None):
        """The same on device memory (e.g. torch tensors' data_ptr()):
        vals[n_hp][ld] float64, total[m], optional terms[n_hp][ld] float64 and
        active[n_hp][ld] uint8.  Stream-ordered, no host synchronisation."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_score_points(
                self.p, vals_ptr, int(m), int(ld), total_ptr, terms_ptr or None,
                active_ptr or None, 1, stream))

    def sample_points(self, seed, m, begin=0, want_terms=False, want_active=False, stream=None):
        """``m`` whole configurations drawn from the below mixtures of the
        last fit, with their EI (tpe_plan_sample_points): configuration j is
        draw ``begin + j`` under Philox key ``seed``.  Returns (vals[n_hp, m]
        with NaN where inactive, total[m][, terms[n_hp, m]][, active[n_hp, m]
        uint8]) -- vals is a pool array, the rest what ``score_points``
        returns for it."""
        e = self.engine
        m = int(m)
        if m < 0:
            raise ValueError('the number of configurations must not be negative')
        vals = np.empty((self.n_hp, m))
        total = np.empty(m)
        terms = np.empty((self.n_hp, m)) if want_terms else None
        active = np.empty((self.n_hp, m), dtype=np.uint8) if want_active else None
        with e.lock:
            e.check(e.lib.tpe_plan_sample_points(
                self.p, int(seed) & (2 ** 64 - 1), int(begin), m, m, vals.ctypes.data,
                total.ctypes.data, terms.ctypes.data if want_terms else None,
                active.ctypes.data if want_active else None, 0, stream))
        return (vals, total) + ((terms,) if want_terms else ()) + ((active,) if want_active else ())

    def sample_points_device(self, seed, begin, m, ld, vals_ptr, total_ptr, terms_ptr=0,
                             active_ptr=0, stream=None):
        """The same into device memory: vals[n_hp][ld] float64, total[m],
        optional terms[n_hp][ld] float64 and active[n_hp][ld] uint8.
        Stream-ordered, no host synchronisation."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_sample_points(
                self.p, int(seed) & (2 ** 64 - 1), int(begin), int(m), int(ld), vals_ptr,
                total_ptr, terms_ptr or None, active_ptr or None, 1, stream))

    # ---- multivariate TPE: the joint model over the root hps (tpe_plan_joint_*)
    def joint_fit(self, stream=None):
        """Build the joint Parzen model over the unconditional hps from the
        last ``fit`` (tpe_plan_joint_fit); a later ``fit`` invalidates it."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_joint_fit(self.p, stream))

    def joint_mixture(self, hp, side=0):
        """(w, mu, sigma, rows) of root hp ``hp`` in component order
        (tpe_plan_joint_get_mixture): component 0 is the prior (rows[0] = -1),
        component k the side's k-th row; the entries are those of
        ``mixture(hp, side)`` that the row owns.  A categorical hp: mu = the
        observed option, sigma = the smoothing a.  ``hp = -1``: the component
        weights (mu and sigma empty)."""
        e = self.engine
        cap = max(self.max_trials + 1, 1)
        w, mu, sg = np.empty(cap), np.empty(cap), np.empty(cap)
        rows = np.empty(cap, dtype=np.int32)
        k = C.c_int64(0)
        with e.lock:
            e.check(e.lib.tpe_plan_joint_get_mixture(self.p, int(hp), int(side), _dp(w), _dp(mu),
                                                     _dp(sg), rows.ctypes.data, cap, C.byref(k)))
        k = k.value
        if int(hp) < 0:
            return w[:k].copy(), np.empty(0), np.empty(0), rows[:k].copy()
        return w[:k].copy(), mu[:k].copy(), sg[:k].copy(), rows[:k].copy()

    def joint_score_points(self, vals, want_terms=False, want_active=False, want_joint=False,
                           stream=None):
        """``score_points`` under the joint model (tpe_plan_joint_score_points):
        total = joint + the conditional hps' terms in hp order; the root hps'
        terms are +0.0.  Returns total[M], or (total[, terms][, active]
        [, joint[M]]) with the ``want_`` flags."""
        e = self.engine
        vals = _f64(vals)
        if vals.ndim != 2 or vals.shape[0] != self.n_hp:
            raise ValueError('configurations must be a [n_hp, M] array')
        m = vals.shape[1]
        total = np.empty(m)
        joint = np.empty(m) if want_joint else None
        terms = np.empty((self.n_hp, m)) if want_terms else None
        active = np.empty((self.n_hp, m), dtype=np.uint8) if want_active else None
        with e.lock:
            e.check(e.lib.tpe_plan_joint_score_points(
                self.p, vals.ctypes.data, m, m, total.ctypes.data,
                joint.ctypes.data if want_joint else None,
                terms.ctypes.data if want_terms else None,
                active.ctypes.data if want_active else None, 0, stream))
        out = (total,) + ((terms,) if want_terms else ()) + ((active,) if want_active else ()) \
            + ((joint,) if want_joint else ())
        return out[0] if len(out) == 1 else out

    def joint_score_points_device(self, vals_ptr, m, ld, total_ptr, joint_ptr=0, terms_ptr=0,
                                  active_ptr=0, stream=None):
        """The same on device memory, as ``score_points_device``; joint[m]
        optional.  Stream-ordered, no host synchronisation."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_joint_score_points(
                self.p, vals_ptr, int(m), int(ld), total_ptr, joint_ptr or None,
                terms_ptr or None, active_ptr or None, 1, stream))

    def joint_sides(self, m):
        """(J_below[m], J_above[m]) of the last joint score or draw
        (tpe_plan_joint_sides; diagnostics)."""
        e = self.engine
        jb, ja = np.empty(int(m)), np.empty(int(m))
        with e.lock:
            e.check(e.lib.tpe_plan_joint_sides(self.p, jb.ctypes.data, ja.ctypes.data, int(m)))
        return jb, ja

    def joint_sample_points(self, seed, m, begin=0, want_terms=False, want_active=False,
                            want_joint=False, want_comp=False, stream=None):
        """``sample_points`` under the joint model
        (tpe_plan_joint_sample_points): every configuration picks one below
        component and draws all its root values from it.  Returns (vals,
        total[, terms][, active][, joint][, comp int32[m]])."""
        e = self.engine
        m = int(m)
        if m < 0:
            raise ValueError('the number of configurations must not be negative')
        vals = np.empty((self.n_hp, m))
        total = np.empty(m)
        joint = np.empty(m) if want_joint else None
        comp = np.empty(m, dtype=np.int32) if want_comp else None
        terms = np.empty((self.n_hp, m)) if want_terms else None
        active = np.empty((self.n_hp, m), dtype=np.uint8) if want_active else None
        with e.lock:
            e.check(e.lib.tpe_plan_joint_sample_points(
                self.p, int(seed) & (2 ** 64 - 1), int(begin), m, m, vals.ctypes.data,
                comp.ctypes.data if want_comp else None, total.ctypes.data,
                joint.ctypes.data if want_joint else None,
                terms.ctypes.data if want_terms else None,
                active.ctypes.data if want_active else None, 0, stream))
        return (vals, total) + ((terms,) if want_terms else ()) + \
            ((active,) if want_active else ()) + ((joint,) if want_joint else ()) + \
            ((comp,) if want_comp else ())

    def joint_sample_points_device(self, seed, begin, m, ld, vals_ptr, total_ptr, comp_ptr=0,
                                   joint_ptr=0, terms_ptr=0, active_ptr=0, stream=None):
        """The same into device memory, as ``sample_points_device``."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_joint_sample_points(
                self.p, int(seed) & (2 ** 64 - 1), int(begin), int(m), int(ld), vals_ptr,
                comp_ptr or None, total_ptr, joint_ptr or None, terms_ptr or None,
                active_ptr or None, 1, stream))

    # ---- multivariate TPE over conditional spaces: one joint model per group
    # of hps that are active together (tpe_plan_group_*)
    def group_info(self):
        """group_of_hp int32[n_hp] and the number of groups G
        (tpe_plan_group_info): group 0 the unconditional hps, the others in
        ascending order of their smallest hp index."""
        e = self.engine
        g = np.empty(self.n_hp, dtype=np.int32)
        n = C.c_int32(0)
        with e.lock:
            e.check(e.lib.tpe_plan_group_info(self.p, g.ctypes.data, C.byref(n)))
        return g, n.value

    def group_fit(self, stream=None):
        """Build every group's joint Parzen model from the last ``fit``
        (tpe_plan_group_fit); a later ``fit`` invalidates them."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_group_fit(self.p, stream))

    def group_mixture(self, group, hp, side=0):
        """``joint_mixture`` of hp ``hp`` of group ``group``
        (tpe_plan_group_get_mixture): (w, mu, sigma, rows) in component
        order, rows[0] = -1; ``hp = -1``: the group's component weights."""
        e = self.engine
        cap = max(self.max_trials + 1, 1)
        w, mu, sg = np.empty(cap), np.empty(cap), np.empty(cap)
        rows = np.empty(cap, dtype=np.int32)
        k = C.c_int64(0)
        with e.lock:
            e.check(e.lib.tpe_plan_group_get_mixture(self.p, int(group), int(hp), int(side),
                                                     _dp(w), _dp(mu), _dp(sg), rows.ctypes.data,
                                                     cap, C.byref(k)))
        k = k.value
        if int(hp) < 0:
            return w[:k].copy(), np.empty(0), np.empty(0), rows[:k].copy()
        return w[:k].copy(), mu[:k].copy(), sg[:k].copy(), rows[:k].copy()

    def group_score_points(self, vals, want_active=False, want_joint=False, stream=None):
        """``score_points`` under the group models
        (tpe_plan_group_score_points): total = the active groups' joint in
        group order.  Returns total[M], or (total[, active][, joint[G, M]])
        with the ``want_`` flags; there are no per-hp terms."""
        e = self.engine
        vals = _f64(vals)
        if vals.ndim != 2 or vals.shape[0] != self.n_hp:
            raise ValueError('configurations must be a [n_hp, M] array')
        m = vals.shape[1]
        total = np.empty(m)
        joint = np.empty((self.group_info()[1], m)) if want_joint else None
        active = np.empty((self.n_hp, m), dtype=np.uint8) if want_active else None
        with e.lock:
            e.check(e.lib.tpe_plan_group_score_points(
                self.p, vals.ctypes.data, m, m, total.ctypes.data,
                joint.ctypes.data if want_joint else None,
                active.ctypes.data if want_active else None, 0, stream))
        out = (total,) + ((active,) if want_active else ()) + ((joint,) if want_joint else ())
        return out[0] if len(out) == 1 else out

    def group_score_points_device(self, vals_ptr, m, ld, total_ptr, joint_ptr=0, active_ptr=0,
                                  stream=None):
        """The same on device memory, as ``score_points_device``; joint[G][ld]
        optional.  Stream-ordered, no host synchronisation."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_group_score_points(
                self.p, vals_ptr, int(m), int(ld), total_ptr, joint_ptr or None,
                active_ptr or None, 1, stream))

    def group_sides(self, group, m):
        """(J_below[m], J_above[m]) of ``group`` in the last group score or
        draw, NaN where the group was inactive (tpe_plan_group_sides)."""
        e = self.engine
        jb, ja = np.empty(int(m)), np.empty(int(m))
        with e.lock:
            e.check(e.lib.tpe_plan_group_sides(self.p, int(group), jb.ctypes.data,
                                               ja.ctypes.data, int(m)))
        return jb, ja

    def group_sample_points(self, seed, m, begin=0, want_active=False, want_joint=False,
                            want_comp=False, stream=None):
        """``sample_points`` under the group models
        (tpe_plan_group_sample_points): every active group picks one of its
        below components and draws all its hps from it.  Returns (vals,
        total[, active][, joint[G, m]][, comp int32[G, m], -1 where the group
        is inactive])."""
        e = self.engine
        m = int(m)
        if m < 0:
            raise ValueError('the number of configurations must not be negative')
        G = self.group_info()[1]
        vals = np.empty((self.n_hp, m))
        total = np.empty(m)
        joint = np.empty((G, m)) if want_joint else None
        comp = np.empty((G, m), dtype=np.int32) if want_comp else None
        active = np.empty((self.n_hp, m), dtype=np.uint8) if want_active else None
        with e.lock:
            e.check(e.lib.tpe_plan_group_sample_points(
                self.p, int(seed) & (2 ** 64 - 1), int(begin), m, m, vals.ctypes.data,
                comp.ctypes.data if want_comp else None, total.ctypes.data,
                joint.ctypes.data if want_joint else None,
                active.ctypes.data if want_active else None, 0, stream))
        return (vals, total) + ((active,) if want_active else ()) + \
            ((joint,) if want_joint else ()) + ((comp,) if want_comp else ())

    def group_sample_points_device(self, seed, begin, m, ld, vals_ptr, total_ptr, comp_ptr=0,
                                   joint_ptr=0, active_ptr=0, stream=None):
        """The same into device memory, as ``sample_points_device``;
        comp[G][ld] int32 and joint[G][ld] optional."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_group_sample_points(
                self.p, int(seed) & (2 ** 64 - 1), int(begin), int(m), int(ld), vals_ptr,
                comp_ptr or None, total_ptr, joint_ptr or None, active_ptr or None, 1, stream))

    def group_batch_points(self, vals, k, eligible=None, want_trace=False, stream=None):
        """A batch of ``k`` configurations for parallel workers
        (tpe_plan_group_batch_points): greedy picks over ``vals[n_hp, M]`` --
        the configurations of the plan's last ``group_score_points`` /
        ``group_sample_points`` call -- each pick joining the above side of its
        active groups as a pending component before the next round.  Returns
        (idx int32[k], gain[k]) with gain[t] the pick's score in its round;
        ``want_trace`` adds trace[k, M], every configuration's score in every
        round.  ValueError when fewer than ``k`` selectable ones remain."""
        e = self.engine
        vals = _f64(vals)
        if vals.ndim != 2 or vals.shape[0] != self.n_hp:
            raise ValueError('configurations must be a [n_hp, M] array')
        m, k = vals.shape[1], int(k)
        el = None if eligible is None else np.ascontiguousarray(
            np.asarray(eligible).ravel() != 0, dtype=np.uint8)
        if el is not None and el.size != m:
            raise ValueError('eligible must have one entry per configuration')
        idx = np.empty(max(k, 0), dtype=np.int32)
        gain = np.empty(max(k, 0))
        trace = np.empty((max(k, 0), m)) if want_trace else None
        with e.lock:
            e.check(e.lib.tpe_plan_group_batch_points(
                self.p, vals.ctypes.data, m, m, None if el is None else el.ctypes.data, k,
                idx.ctypes.data, gain.ctypes.data, trace.ctypes.data if want_trace else None,
                0, stream))
        return (idx, gain, trace) if want_trace else (idx, gain)

    def group_batch_points_device(self, vals_ptr, m, ld, k, idx_ptr, gain_ptr=0, eligible_ptr=0,
                                  trace_ptr=0, stream=None):
        """The same on device memory: vals[n_hp][ld], eligible[m] (0: all),
        idx int32[k], gain[k] and trace[k][ld] (0: not wanted).  Stream-ordered
        but for the read-back that reports a short batch."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_group_batch_points(
                self.p, vals_ptr, int(m), int(ld), eligible_ptr or None, int(k), idx_ptr,
                gain_ptr or None, trace_ptr or None, 1, stream))

    def topk_points(self, total, k, eligible=None, m=None, out=None, stream=None):
        """The ``k`` eligible entries that rank first, as ``tpe.rank_pool``
        ranks them (tpe_plan_topk_points).  Host arrays ``total[m]`` /
        ``eligible[m]`` return an int32 array [k]; with ``m`` given, ``total``,
        ``eligible`` (0: none) and ``out`` are device pointers and the picks
        stay on the device."""
        e = self.engine
        if m is not None:
            with e.lock:
                e.check(e.lib.tpe_plan_topk_points(self.p, total, eligible or None, int(m), int(k),
                                                   out, 1, stream))
            return None
        total = _f64(total).ravel()
        el = None if eligible is None else np.ascontiguousarray(
            np.asarray(eligible).ravel() != 0, dtype=np.uint8)
        if el is not None and el.size != total.size:
            raise ValueError('eligible must have one entry per total')
        idx = np.empty(max(int(k), 0), dtype=np.int32)
        with e.lock:
            e.check(e.lib.tpe_plan_topk_points(
                self.p, total.ctypes.data, None if el is None else el.ctypes.data, total.size,
                int(k), idx.ctypes.data, 0, stream))
        return idx

    def gather_points(self, vals, idx, k=None, ld=None, out=None, stream=None):
        """The columns ``idx`` of ``vals`` (tpe_plan_gather_points): host
        arrays vals[n_hp, ld] / idx[k] return [n_hp, k]; with ``k`` and ``ld``
        given, ``vals``, ``idx`` and ``out`` are device pointers."""
        e = self.engine
        if k is not None:
            with e.lock:
                e.check(e.lib.tpe_plan_gather_points(self.p, vals, int(ld), idx, int(k), out, 1,
                                                     stream))
            return None
        vals = _f64(vals)
        if vals.ndim != 2 or vals.shape[0] != self.n_hp:
            raise ValueError('configurations must be a [n_hp, M] array')
        idx = np.ascontiguousarray(idx, dtype=np.int32).ravel()
        res = np.empty((self.n_hp, idx.size))
        with e.lock:
            e.check(e.lib.tpe_plan_gather_points(self.p, vals.ctypes.data, vals.shape[1],
                                                 idx.ctypes.data, idx.size, res.ctypes.data, 0,
                                                 stream))
        return res

    def profile(self, capacity):
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_profile(self.p, int(capacity)))

    def profile_read(self, kind):
        """(avg_ms, launches, pairs_per_launch) of one scoring kind."""
        e = self.engine
        ms, n, pairs = C.c_double(0), C.c_int64(0), C.c_double(0)
        with e.lock:
            e.check(e.lib.tpe_plan_profile_read(self.p, int(kind), C.byref(ms), C.byref(n),
                                                C.byref(pairs)))
        return ms.value, n.value, pairs.value

    def set_lattice(self, enable):
        """Score bounded quantized hps on their value lattice (default) or
        every candidate on its own (tpe_plan_set_lattice)."""
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_set_lattice(self.p, int(bool(enable))))

    def set_prune(self, mode):
        """Log-sum-exp on bucketed large draws (tpe_plan_set_prune): 0 / False
        every pair, 1 skip negligible component blocks, 2 skip + one exponent
        per wave, 3 / True (default) the same with block-local fp32 pairs."""
        mode = 3 if mode is True else int(mode)
        e = self.engine
        with e.lock:
            e.check(e.lib.tpe_plan_set_prune(self.p, mode))

    def census(self, enable, n=7):
        """Pair census since the last call: (quantized total, live, evaluated,
        log-sum-exp total, log-sum-exp evaluated in the one-exponent form,
        log-sum-exp evaluated, of those in the fp32 per-group-lift form[,
        one-exponent pairs re-evaluated by a wave's second attempt,
        one-exponent pairs of wide blocks (mode 3's fp64 loop), one-exponent
        pairs evaluated in the moment form of their chunk, of those the
        8-wide form, of those the 16-wide degree-15 form, pairs credited to
        candidates scored from the Chebyshev tables]) -- the first
        ``n`` (7 .. 13); enable it for the following suggests."""
        if not 0 <= n <= 13:
            raise ValueError('the census has 13 counters')
        e = self.engine
        out = (C.c_int64 * 13)()
        with e.lock:
            e.check(e.lib.tpe_plan_census_n(self.p, int(bool(enable)), out, int(n)))
        return tuple(int(v) for v in out[:n])

    def tie_counts(self, n_suggest):
        """Debug (tpe_plan_tie_counts): int32 [n_suggest][n_hp], the 128-candidate
        wave tiles the direct pass behind the Chebyshev tables scored per hp in
        the last scoring launch that took them -- the tiles in the tie window
        of a certified slot, every tile of another, 0 for an inactive hp, -1
        where no such launch has scored the hp."""
        e = self.engine
        out = np.empty((int(n_suggest), self.n_hp), dtype=np.int32)
        with e.lock:
            e.check(e.lib.tpe_plan_tie_counts(self.p, int(n_suggest), out.ctypes.data))
        return out

    def tab_wmax(self, n_suggest):
        """Debug (tpe_plan_tab_wmax): float64 [n_suggest][n_hp][8 * tiles per
        slot], every 128-candidate wave tile's best table score as the table
        pass of the last scoring launch that took the Chebyshev tables left
        it; entries of hps without two certified tables, of inactive hps and
        of wave tiles never written are unspecified."""
        e = self.engine
        with e.lock:
            w = e.lib.tpe_plan_tab_wmax(self.p, int(n_suggest), None)
            e.check(min(w, 0))
            out = np.empty((int(n_suggest), self.n_hp, w), dtype=np.float64)
            e.check(e.lib.tpe_plan_tab_wmax(self.p, int(n_suggest), out.ctypes.data))
        return out

    def tab_bound(self, hp):
        """Debug (tpe_plan_tab_bound): float64 [4096], the bound lattice of one
        hp as the last fit left it -- an upper bound of the table score over
        each of 4096 equal cells of the hp's range; an error when the hp takes
        no table, a side is not certified or the prefilter is off."""
        e = self.engine
        with e.lock:
            n = e.lib.tpe_plan_tab_bound(self.p, int(hp), None)
            e.check(min(n, 0))
            out = np.empty(n, dtype=np.float64)
            e.check(e.lib.tpe_plan_tab_bound(self.p, int(hp), out.ctypes.data))
        return out

    def tab_panels(self, hp, side):
        """Debug (tpe_plan_tab_panels): the Chebyshev table of (hp, side; 0 below,
        1 above) as the last fit left it: dict(y_lo, inv_w, P, ncert, panels) with
        panels uint8 [P][144], the raw records (16 coefficients, M, one unused
        double)."""
        e = self.engine
        y_lo, inv_w, ncert = C.c_double(), C.c_double(), C.c_int32()
        buf = np.zeros((64, 144), dtype=np.uint8)
        with e.lock:
            n = e.lib.tpe_plan_tab_panels(self.p, int(hp), int(side), C.addressof(y_lo),
                                          C.addressof(inv_w), C.addressof(ncert), buf.ctypes.data)
            e.check(min(n, 0))
        return dict(y_lo=y_lo.value, inv_w=inv_w.value, P=int(n), ncert=int(ncert.value),
                    panels=buf[:n].copy())

    def tab_cert(self, hp, side):
        """Debug (tpe_plan_tab_cert): float64 [P][3] = (le, lr, lg), the log2 of
        each panel's interpolation bound, rounding bound and lower bound of the
        mixture as the last build computed them (certified: max(le, lr) + 1 <=
        lg - 28)."""
        e = self.engine
        out = np.zeros((64, 3), dtype=np.float64)
        with e.lock:
            n = e.lib.tpe_plan_tab_cert(self.p, int(hp), int(side), out.ctypes.data)
            e.check(min(n, 0))
        return out[:n].copy()

    def tie_list(self, s, hp):
        """Debug (tpe_plan_tie_list): int32 [tie_counts[s][hp]], the wave tiles of
        (suggestion s, hp) the direct pass of the last scoring launch that took
        the tables was given, in list order."""
        e = self.engine
        with e.lock:
            n = e.lib.tpe_plan_tie_list(self.p, int(s), int(hp), None)
            e.check(min(n, 0))
            out = np.empty(n, dtype=np.int32)
            if n:
                e.check(min(e.lib.tpe_plan_tie_list(self.p, int(s), int(hp), out.ctypes.data), 0))
        return out

    def tab_hot(self, n_suggest):
        """Debug (tpe_plan_tab_hot): float64 [n_suggest][n_hp][18] = y_lo,
        y_hi, lo[8], hi[8], the hot intervals of the last scoring launch that
        ran the prefilter's pilot; entries of slots it skipped are
        unspecified."""
        e = self.engine
        out = np.empty((int(n_suggest), self.n_hp, 18), dtype=np.float64)
        with e.lock:
            e.check(e.lib.tpe_plan_tab_hot(self.p, int(n_suggest), out.ctypes.data))
        return out

    def cand_dump(self, s, hp):
        """Debug (tpe_plan_cand_dump): (values float64 [n], positions int32
        [n]) of one (suggestion, hp) as the last sorted draw left them.  Wave
        tiles the pruning draw dropped (-inf in tab_wmax; TPE_DRAW_PRUNE=0:
        none) were never written: their entries are unspecified."""
        e = self.engine
        with e.lock:
            n = e.lib.tpe_plan_cand_dump(self.p, int(s), int(hp), None, None)
            e.check(int(min(n, 0)))
            vals = np.empty(n, dtype=np.float64)
            pos = np.empty(n, dtype=np.int32)
            e.check(int(min(e.lib.tpe_plan_cand_dump(self.p, int(s), int(hp), vals.ctypes.data,
                                                     pos.ctypes.data), 0)))
        return vals, pos

    def draw_screen_stats(self):
        """Debug (tpe_plan_draw_screen_stats): (sort blocks screened, sort
        blocks fallen back to the full draw, candidates inverted in the
        screened blocks) since the last read; reset on read."""
        e = self.engine
        out = np.zeros(3, dtype=np.int64)
        with e.lock:
            e.check(e.lib.tpe_plan_draw_screen_stats(self.p, out.ctypes.data))
        return int(out[0]), int(out[1]), int(out[2])

    def last_stats(self):
        e = self.engine
        ms, pairs = C.c_double(0), C.c_double(0)
        with e.lock:
            e.check(e.lib.tpe_plan_last_stats(self.p, C.byref(ms), C.byref(pairs)))
        return ms.value, pairs.value


_default = {}
_default_lock = threading.Lock()


def default_engine(device: int | None = None) -> Engine:
    """Process-wide engine for ``device`` (default: LOCAL_RANK or 0)."""
    if device is None:
        device = int(os.environ.get('LOCAL_RANK', '0'))
    with _default_lock:
        eng = _default.get(device)
        if eng is None:
            eng = Engine(device)
            _default[device] = eng
        return eng
