"""ctypes binding of libinstagraal_hip.so (the C ABI of include/instagraal_hip.h).

``lib()`` gives every entry point the ``restype`` / ``argtypes`` the header declares (``abi.py``), so the calls below pass plain Python
values, arrays by ``_p(...)`` and outputs by ``byref``; an argument of the wrong C type raises ``ctypes.ArgumentError``.

There is no CPU fallback: if the shared library or a HIP device is missing, every entry
point raises.  The library is built in-tree by ``__graft_entry__.build()`` / ``build_lib()``.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, "libinstagraal_hip.so")
SRC = os.path.join(HERE, "csrc", "ig_hip.hip")
SRC_HOST = os.path.join(HERE, "csrc", "ig_draw.cpp")  # host-only part: the candidate draw
HEADER = os.path.join(ROOT, "include", "instagraal_hip.h")  # the C ABI: abi.declarations reads the signatures out of it
# what a rebuild depends on: the two sources, every kernel file and host part beside them, the headers
DEPS = [SRC, SRC_HOST] + sorted(glob.glob(os.path.join(HERE, "csrc", "*.cuh")) + glob.glob(os.path.join(HERE, "csrc", "*.inc"))) + \
       [os.path.join(ROOT, "include", f) for f in ("ig_detmath.h", "ig_detmath_tables.h")] + [HEADER]

N_TMP_STRUCT = 24
ASSEMBLY_CONTACTS_PASSES = ("count", "scan", "scatter", "sort_short", "sort_lds", "sort_long", "reduce")  # ig_debug_assembly_contacts_time
JOIN_SUPPORT_PASSES = ("ends", "count", "scan", "scatter", "sort_short", "sort_lds", "sort_long", "reduce", "model")  # ig_debug_join_support_time
PLACEMENT_SUPPORT_PASSES = ("records", "count", "rows", "scatter", "sort_short", "sort_lds", "sort_long", "reduce", "prefix", "scan")  # ig_debug_placement_support_time
PLACEMENT_SUPPORT_FORMS = ("default", "thread", "wave")  # ig_debug_placement_support_form
SEGMENT_PLACEMENT_PASSES = PLACEMENT_SUPPORT_PASSES + ("quadrants",)  # ig_debug_segment_placement_time
ORIENTATION_SUPPORT_WAVE_PAIRS = 4096  # ORIENT_WAVE_PAIRS (csrc/ig_kernels_orient.cuh): 2 * pairs beyond this take a workgroup in the model pass
ORIENTATION_SUPPORT_FORMS = {"observed": ("atomic", "combined"), "model": ("default", "wave", "workgroup")}  # ig_debug_orientation_support_time: pass -> forms
GAP_SUPPORT_WAVE_TERMS = 8192  # GAP_WAVE_TERMS (csrc/ig_kernels_gap.cuh): pairs * gaps beyond this take a workgroup in the model pass
GAP_SUPPORT_PASSES = ("observed", "model", "model_wave", "model_workgroup")  # ig_debug_gap_support_time
BALANCE_BUILD_PASSES = ("units", "count", "rows", "scatter", "sort_short", "sort_lds", "sort_long", "reduce")  # ig_debug_balance_build_time
BALANCE_SNAPSHOT_PASSES = ("count", "rows", "scatter", "sort_short", "sort_lds", "sort_long", "gather")  # ig_debug_balance_snapshot_time
ZOOM_PASSES = ("rowstart", "words", "sort_short", "sort_lds", "sort_long", "reduce")  # the passes of ig_assembly_contacts_coarsen
BALANCE_FORMS = ("default", "wave", "packed")  # ig_debug_balance_form
EDIT_PASSES = ("plan", "state", "tables", "delta", "zero", "whole")  # ig_debug_edit_time
CUT_JOIN_PASSES = ("span", "scan", "zero", "count", "rowscan", "scatter", "sort_short", "sort_lds", "sort_long", "reduce", "terms", "join_zero")  # ig_debug_cut_join_time
CUT_JOIN_LDS_PAIRS = 256  # CJ_LDS_PAIRS (csrc/ig_kernels_cutjoin.cuh): pairs up to which the join pass keeps its accumulators in LDS
PAIRS_PASSES = ("lift",) + ASSEMBLY_CONTACTS_PASSES + ("law",)  # ig_debug_pairs_time
PRE_DIGEST_PASSES = ("sites", "scan", "cuts", "fragments")  # ig_pre_digest
TEXT_PASSES = ("mark", "scan", "parse", "compact")  # ig_text_parse
SEQ_CLASSES = 8  # SEQ_NC (csrc/ig_kernels_seq.cuh): scaffold_polish.CLASSES
CONTIG_ARRAYS = ("head_bin", "tail_bin", "n_sub", "length_bp")  # ig_join_scores_fetch: per linear contig
MAX_CANDIDATES = 16

FRAG_FIELDS = ("pos", "sub_pos", "id_c", "start_bp", "len_bp", "sub_len", "circ", "id", "prev", "next", "l_cont",
               "sub_l_cont", "l_cont_bp", "ori", "rep", "activ", "id_d")  # kernel_sparse_adapt.cu:40-58


class MoveResult(C.Structure):
    _fields_ = [("o", C.c_double), ("dist", C.c_double), ("mean_len", C.c_double), ("op_sampled", C.c_int32),
                ("id_f_sampled", C.c_int32), ("n_contigs", C.c_int32), ("n_candidates", C.c_int32),
                ("n_slice", C.c_int64), ("n_evals", C.c_int64), ("bytes_min", C.c_int64), ("error", C.c_int32),
                ("pad", C.c_int32)]


MOVE_RESULT_DTYPE = np.dtype([("o", np.float64), ("dist", np.float64), ("mean_len", np.float64),
                              ("op_sampled", np.int32), ("id_f_sampled", np.int32), ("n_contigs", np.int32),
                              ("n_candidates", np.int32), ("n_slice", np.int64), ("n_evals", np.int64),
                              ("bytes_min", np.int64), ("error", np.int32), ("pad", np.int32)])
assert MOVE_RESULT_DTYPE.itemsize == C.sizeof(MoveResult)


def build_lib(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(d) <= os.path.getmtime(LIB_PATH) for d in DEPS):
        return LIB_PATH
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
           "-Wno-unused-result", "-Wno-unused-value", "-pthread", "-o", LIB_PATH, SRC, SRC_HOST]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libinstagraal_hip.so is missing (%s): run __graft_entry__.build(); "
                               "the MI355X path has no CPU fallback" % LIB_PATH)
        if not os.path.exists(HEADER):
            raise RuntimeError("instagraal_hip.h is missing (%s): the library's signatures are read from it" % HEADER)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same SONAME, requested under an
        # unversioned name), so if our library pulled in /opt/rocm's copy first a later `import torch` would bring a
        # second runtime that sees no devices.  Loading torch first makes our NEEDED entry resolve to its copy.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        # the product library, nothing else -- unless the caller says in so many words that this is a tuning session
        # (IG_DEBUG_TUNING=1 IG_HIP_LIB=<a build of the same source with other -D constants>: tools/diff_pass_time.py)
        path = LIB_PATH
        if os.environ.get("IG_HIP_LIB"):
            if os.environ.get("IG_DEBUG_TUNING") == "1":
                path = os.environ["IG_HIP_LIB"]
            else:  # (said out loud: a deployment that used to point IG_HIP_LIB somewhere else would load another build silently)
                import warnings

                warnings.warn("IG_HIP_LIB=%s is ignored without IG_DEBUG_TUNING=1: loading the product library %s"
                              % (os.environ["IG_HIP_LIB"], LIB_PATH), RuntimeWarning, stacklevel=2)
        loaded = C.CDLL(path)
        with open(HEADER) as header:
            abi.apply(loaded, header.read())  # restype and argtypes of every entry point, as the header declares it
        _lib = loaded
    return _lib


class HipError(RuntimeError):
    pass


def model_values_host(params, s):
    """the two quantised model values of the separations ``s`` (f32) on the CPU, from include/ig_detmath.h (``ig_model_values_host``:
    no context, no GPU) -> (e_q, l_q), int64 arrays of the shape of ``s``: ig_quantize(ig_rippe(s, params)) and ig_quantize(ig_log10
    of that value).  ``params``: the eight floats of ig_params in its order (``sampler.PARAM_NAMES``)"""
    p = np.ascontiguousarray(params, np.float32).ravel()
    if p.size != 8:
        raise HipError("model_values_host: eight parameters in the order of ig_params (got %d)" % p.size)
    sep = np.ascontiguousarray(s, np.float32)
    e_q, l_q = np.zeros(sep.shape, np.int64), np.zeros(sep.shape, np.int64)
    _ck(lib().ig_model_values_host(_p(p), _p(sep), sep.size, _p(e_q), _p(l_q)))
    return e_q, l_q


def _params8(params, who):
    p = np.ascontiguousarray(params, np.float32).ravel()
    if p.size != 8:
        raise HipError("%s: eight parameters in the order of ig_params (got %d)" % (who, p.size))
    return p


def contact_terms_host(params, mean_kb, s, d, trans, count):
    """the quantised likelihood terms of contacts on the CPU (``ig_contact_terms_host``: eval_q's ring-free branch restated from
    include/ig_detmath.h, hot path selection included; no context, no GPU) -> int64 of the shape of ``s``.  ``s``: separation in kb
    (f32), ``d``: rank distance, ``trans``: non-zero for a trans pair (s and d play no part then), ``count``: the observed count."""
    p = _params8(params, "contact_terms_host")
    sep = np.ascontiguousarray(s, np.float32)
    dd, tt, cc = (np.ascontiguousarray(np.broadcast_to(np.asarray(a), sep.shape), np.int32) for a in (d, trans, count))
    q = np.zeros(sep.shape, np.int64)
    _ck(lib().ig_contact_terms_host(_p(p), float(np.float32(mean_kb)), _p(sep), _p(dd), _p(tt), _p(cc), sep.size, _p(q)))
    return q


def zero_terms_host(params, mean_kb, pos, length):
    """the quantised zero-pixel terms of sub-fragments of linear contigs on the CPU (``ig_zero_terms_host``: zero_q with s_tot == 0) ->
    int64 of the shape of ``pos``: rank ``pos`` in a contig of ``length`` sub-fragments"""
    p = _params8(params, "zero_terms_host")
    pp = np.ascontiguousarray(pos, np.int32)
    ll = np.ascontiguousarray(np.broadcast_to(np.asarray(length), pp.shape), np.int32)
    q = np.zeros(pp.shape, np.int64)
    _ck(lib().ig_zero_terms_host(_p(p), float(np.float32(mean_kb)), _p(pp), _p(ll), pp.size, _p(q)))
    return q


def as_int32_exact(a, name="array"):
    """``a`` as a contiguous int32 array; ValueError unless every value survives the conversion: a whole number within
    -2^31 .. 2^31 - 1 (a count of 2^31 would wrap to -2^31, 2.5 would truncate to 2).  No device, no library."""
    src = np.asarray(a)
    if src.dtype == np.int32:
        return np.ascontiguousarray(src)
    if src.dtype == object or not (np.issubdtype(src.dtype, np.integer) or np.issubdtype(src.dtype, np.floating) or src.dtype == np.bool_):
        raise ValueError("%s: integers expected (got dtype %s)" % (name, src.dtype))
    if np.issubdtype(src.dtype, np.floating):
        bad = ~np.isfinite(src) | (src != np.floor(np.where(np.isfinite(src), src, 0))) | (src < -2.0 ** 31) | (src >= 2.0 ** 31)
    else:
        bad = np.zeros(src.shape, bool)
        if src.dtype != np.bool_:
            info = np.iinfo(src.dtype)
            if info.max > 2 ** 31 - 1:
                bad |= src > 2 ** 31 - 1
            if info.min < -2 ** 31:
                bad |= src < -2 ** 31
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError("%s: %d of %d values do not fit int32 (the first: %r at index %d)" % (name, int(bad.sum()), src.size, src.ravel()[k].item(), k))
    return np.ascontiguousarray(src, np.int32)


def _ck(rc):
    if rc != 0:
        raise HipError(lib().ig_last_error().decode())


def _p(a):
    return C.c_void_p(0) if a is None else C.c_void_p(a.ctypes.data)


class _NoLock:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NO_LOCK = _NoLock()


class Neighbours:
    """The jump distributions of setup_distri_frags (CL:3053-3101) in the library's host memory + the draw of
    return_neighbours (CL:3103-3141) on numpy's legacy MT19937 stream (csrc/ig_draw.cpp).  Needs no GPU."""

    def __init__(self, indptr, xk, pk, n_frags, blacklisted=()):
        self._h = C.c_void_p()
        ip = np.ascontiguousarray(indptr, np.int64)
        x = np.ascontiguousarray(xk, np.int32)
        p = np.ascontiguousarray(pk, np.float32)
        b = np.ascontiguousarray(list(blacklisted), np.int32)
        assert ip.size == n_frags + 1 and x.size == p.size == ip[-1]
        _ck(lib().ig_neighbours_create(_p(ip), _p(x), _p(p), int(n_frags), _p(b) if b.size else None, b.size, C.byref(self._h)))
        self.n_frags = int(n_frags)

    def __del__(self):
        try:
            if self._h:
                lib().ig_neighbours_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    @staticmethod
    def take_numpy_state():
        """(key[624] uint32 copy, pos, rest) of numpy's GLOBAL legacy generator"""
        st = np.random.get_state()
        assert st[0] == "MT19937"
        return np.array(st[1], dtype=np.uint32, copy=True), int(st[2]), st[3:]

    @staticmethod
    def put_numpy_state(key, pos, rest):
        np.random.set_state(("MT19937", key, int(pos)) + tuple(rest))

    _mt_cache = [None, 0, None]

    @staticmethod
    def numpy_mt_address():
        """address of numpy's GLOBAL legacy generator's mt19937_state {uint32 key[624]; int pos} (numpy/random/src/mt19937/mt19937.h),
        through the bit generator's own ctypes interface -- or 0 where the layout check fails.  np.random.get_state() +
        set_state() cost 50 - 130 us per pair (a tuple and a 2.5 KB copy each way): more than the draw of one move's candidates
        through numpy itself; on the state in place a draw is a few microseconds.  (np.random.seed / set_state work in place.)"""
        bg = np.random.mtrand._rand._bit_generator
        if Neighbours._mt_cache[0] is not bg:
            addr = 0
            try:
                a = int(bg.ctypes.state_address)
                st = np.random.get_state()
                key = np.frombuffer((C.c_uint32 * 624).from_address(a), np.uint32)
                if st[0] == "MT19937" and np.array_equal(key, st[1]) and C.c_int32.from_address(a + 624 * 4).value == int(st[2]):
                    addr = a
            except Exception:
                addr = 0
            Neighbours._mt_cache = [bg, addr, getattr(bg, "lock", None)]
        return Neighbours._mt_cache[1]

    @staticmethod
    def numpy_mt_lock():
        """the bit generator's own lock (numpy's legacy functions take it around every draw): held around the library calls that
        work on the state in place -- they run with the GIL released, and ig_step_batch_draw's drawing thread writes key / pos for
        the whole call, so another Python thread's np.random.* would race with it.  (Where the layout probe of numpy_mt_address
        fails the callers fall back to get_state / set_state copies, which need no lock.)"""
        Neighbours.numpy_mt_address()
        lk = Neighbours._mt_cache[2]
        return lk if lk is not None else _NO_LOCK

    def draw(self, frags, n_neighbours):
        """candidate lists of consecutive moves, consuming numpy's global generator exactly as successive
        return_neighbours calls would -> (n, n_neighbours) int32, sorted, -1 padded"""
        f = np.ascontiguousarray(frags, np.int32)
        out = np.full((f.size, int(n_neighbours)), -1, np.int32)
        addr = self.numpy_mt_address()
        if addr:  # on numpy's state in place
            with self.numpy_mt_lock():
                rc = lib().ig_neighbours_draw(self._h, addr, addr + 624 * 4, _p(f), f.size, int(n_neighbours), _p(out))
            _ck(rc)
            return out
        key, pos, rest = self.take_numpy_state()
        cpos = C.c_int32(pos)
        rc = lib().ig_neighbours_draw(self._h, _p(key), C.byref(cpos), _p(f), f.size, int(n_neighbours), _p(out))
        self.put_numpy_state(key, cpos.value, rest)
        _ck(rc)
        return out


def _neighbours_draw_nuisance(self, frags, n_neighbours, skip_normal_3=False):
    """the generator stream of a run of moves with nuisance sampling: per move the candidate list, then choice(4), the
    standard normal behind normal(0, sigma), rand() -- numpy's global generator is advanced exactly as the reference's loop
    (step_sampler; step_nuisance_parameters) would -> (cands, id_modif, normal, uniform)"""
    f = np.ascontiguousarray(frags, np.int32)
    n = f.size
    cands = np.full((n, int(n_neighbours)), -1, np.int32)
    idm = np.zeros(n, np.int32)
    g = np.zeros(n, np.float64)
    u = np.zeros(n, np.float64)
    key, pos, rest = self.take_numpy_state()
    cpos, hg, gz = C.c_int32(pos), C.c_int32(int(rest[0])), C.c_double(float(rest[1]))
    rc = lib().ig_neighbours_draw_nuisance(self._h, _p(key), C.byref(cpos), C.byref(hg), C.byref(gz), _p(f), n,
                                           int(n_neighbours), int(bool(skip_normal_3)), _p(cands), _p(idm), _p(g), _p(u))
    self.put_numpy_state(key, cpos.value, (hg.value, gz.value))
    _ck(rc)
    return cands, idm, g, u


Neighbours.draw_nuisance = _neighbours_draw_nuisance


def set_batch_width(w):
    """moves scored per launch by ``Context.step_batch`` (1 = one move at a time; results do not depend on it)"""
    _ck(lib().ig_set_batch_width(int(w)))


def set_window(w):
    """slots of the window of scored moves ig_step_batch keeps from launch to launch (0: off -- the batches of rounds 1 - 4)"""
    _ck(lib().ig_set_window(int(w)))


def set_nuis_width(w):
    """moves scored ahead per launch by the nuisance-on loop (``Context.nuis_step_begin``); 0 = follow the run lengths"""
    _ck(lib().ig_set_nuis_width(int(w)))


def set_nuis_screen(on):
    """the Metropolis test of the nuisance steps from the screened pass where it decides (default), or always from the exact one"""
    _ck(lib().ig_set_nuis_screen(int(on)))


def set_nuis_hist(on):
    """the screened pass starts from the histogram of the cis contacts' distances where that pays (1, default: a cost model decides),
    always (2), or never (0)"""
    _ck(lib().ig_set_nuis_hist(int(on)))


def set_nuis_chain(on):
    """runs of (move, nuisance step) pairs decided on the device, as far as they need no host (default), or one pair per library call"""
    global _nuis_chain
    _nuis_chain = bool(on)
    _ck(lib().ig_set_nuis_chain(int(on)))


_nuis_chain = None


def nuis_chain_wanted():
    """what ``set_nuis_chain`` / IG_NUIS_CHAIN say (default: on)"""
    if _nuis_chain is not None:
        return bool(_nuis_chain)
    return os.environ.get("IG_NUIS_CHAIN", "1") != "0"


CHAIN_MAX = 64  # test parameter sets per ig_nuis_chain_begin (csrc/ig_common.cuh)
CHAIN_REASONS = ("sets used up", "test", "conflict", "pending", "overflow", "no scored slots", "unsupported")


def debug_set_zero_inject(every):
    """tests: the decide step treats every n-th move of a two-tier batch as one whose contenders hold a score of exactly 0.0
    (the move is scored again with every column exact); 0 = off"""
    _ck(lib().ig_debug_set_zero_inject(int(every)))


ROUND_CENSUS = ("launches", "rounds", "committed", "full", "tail_full", "tail_short", "changed", "flags", "stop1_first", "stop1_mid",
                "stop3_first", "stop3_mid", "pend_first", "pend_mid", "resumed", "unclassed")  # IG_RC_* (csrc/ig_common.cuh)
ROUND_CLASSES = ROUND_CENSUS[3:14] + ROUND_CENSUS[15:]  # one of them per round


def debug_set_round_census(on):
    """tests: the decide rounds (k_decide_commit_par) count how each round ended (``Context.debug_round_census``); off by default"""
    _ck(lib().ig_debug_set_round_census(int(bool(on))))


def debug_set_full_hist(on):
    """from-scratch pass over all contacts: tiles of trans pairs only from their count histograms (default) or contact by
    contact -- same exact sums (tests)"""
    _ck(lib().ig_debug_set_full_hist(int(on)))


class Context:
    """One handle per sampler (ig_create .. ig_destroy)."""

    def __init__(self, device_id=0):
        self._h = C.c_void_p()
        _ck(lib().ig_create(device_id, C.byref(self._h)))
        self.N = 0
        self.M = 0

    def close(self):
        if self._h:
            lib().ig_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- upload
    def upload_contacts(self, row, col, cnt, M, rank=0, world=1):
        row, col, cnt = as_int32_exact(row, "row"), as_int32_exact(col, "col"), as_int32_exact(cnt, "cnt")
        _ck(lib().ig_upload_contacts(self._h, _p(row), _p(col), _p(cnt), row.size, M, rank, world))
        self.M = int(M)

    def upload_subfrag_table(self, table):
        """table: (M,) structured float4 or (M, 4) float32"""
        t = np.ascontiguousarray(table)
        if t.dtype.names:
            t = np.stack([t["x"], t["y"], t["z"], t["w"]], axis=1)
        t = np.ascontiguousarray(t, np.float32)
        _ck(lib().ig_upload_subfrag_table(self._h, _p(t), t.shape[0]))
        self.M = int(t.shape[0])

    def upload_state(self, soa17):
        s = np.ascontiguousarray(soa17, np.int32)
        assert s.ndim == 2 and s.shape[0] == 17
        _ck(lib().ig_upload_state(self._h, _p(s), s.shape[1]))
        self.N = int(s.shape[1])

    def download_state(self):
        out = np.zeros((17, self.N), np.int32)
        _ck(lib().ig_download_state(self._h, _p(out)))
        return out

    def set_params(self, p8, mean_subfrag_kb, which=0):
        p = np.ascontiguousarray(p8, np.float32)
        assert p.size == 8
        _ck(lib().ig_set_params(self._h, _p(p), float(mean_subfrag_kb), which))

    def set_insert_config(self, list_bounds6, max_bounds_insert):
        b = np.ascontiguousarray(list_bounds6, np.int32)
        assert b.size == 6
        _ck(lib().ig_set_insert_config(self._h, _p(b), int(max_bounds_insert)))

    def set_initial_genome(self, init_prev, init_next, orientable, blacklisted=()):
        ip = np.ascontiguousarray(init_prev, np.int32)
        inn = np.ascontiguousarray(init_next, np.int32)
        o = np.ascontiguousarray(orientable, np.int32)
        b = np.ascontiguousarray(list(blacklisted), np.int32)
        _ck(lib().ig_set_initial_genome(self._h, _p(ip), _p(inn), _p(o), _p(b) if b.size else None, b.size))

    # ---- likelihood
    def full_likelihood(self, which=0, use_prev_tables=False):
        nz = C.c_double()
        z = C.c_double()
        limbs = np.zeros(5, np.int64)
        _ck(lib().ig_full_likelihood(self._h, which, int(use_prev_tables), C.byref(nz), C.byref(z), _p(limbs)))
        return nz.value, z.value, limbs

    # ---- moves
    def score_move(self, frag_a, cands):
        c = np.ascontiguousarray(cands, np.int32)
        out = np.zeros(c.size * N_TMP_STRUCT, np.float64)
        _ck(lib().ig_score_move(self._h, int(frag_a), _p(c), c.size, _p(out)))
        return out

    def apply(self, frag_a, frag_b, op):
        _ck(lib().ig_apply(self._h, int(frag_a), int(frag_b), int(op)))

    def step(self, frag_a, cands, want_scores=True):
        c = np.ascontiguousarray(cands, np.int32)
        res = MoveResult()
        sc = np.zeros(c.size * N_TMP_STRUCT, np.float64) if want_scores else None
        _ck(lib().ig_step(self._h, int(frag_a), _p(c), c.size, C.byref(res), _p(sc)))
        return res, sc

    def step_draw(self, neighbours, frag_a, n_neighbours, cands=None, want_scores=True):
        """ONE complete step_sampler call in one library call (ig_step_draw): the candidate draw on numpy's generator state in
        place (``cands`` given: the caller's list), lists and results through mapped host memory, the move decided and applied as a
        batch of one -> (MoveResult, scores [C x 24], candidate list).  ``want_scores=False`` -> scores None, and the library is free to
        score the move in two tiers (the exact kernel for the columns that can still win only)"""
        io = self.__dict__.get("_step_io")
        if io is None:
            sc = np.zeros(MAX_CANDIDATES * N_TMP_STRUCT, np.float64)
            io = self._step_io = (sc, sc.ctypes.data, (C.c_int32 * MAX_CANDIDATES)(), C.c_int32(0))
        sc, sc_addr, cbuf, ncand = io
        res = MoveResult()
        if cands is None:
            addr = Neighbours.numpy_mt_address()
            if not addr:  # (a numpy whose generator state cannot be reached in place: two calls)
                row = neighbours.draw(np.array([frag_a], np.int32), int(n_neighbours))[0]
                lst = [int(x) for x in row if x >= 0]
                r, s2 = self.step(int(frag_a), lst, want_scores=want_scores)
                return r, s2, lst
            with Neighbours.numpy_mt_lock():
                rc = lib().ig_step_draw(self._h, neighbours._h, addr, addr + 624 * 4, int(frag_a), int(n_neighbours), cbuf, C.byref(ncand),
                                            C.byref(res), sc_addr if want_scores else None)
        else:
            n = len(cands)
            if n > MAX_CANDIDATES:
                raise HipError("a move needs 1..%d candidates (got %d)" % (MAX_CANDIDATES, n))
            cbuf[:n] = [int(x) for x in cands]
            ncand.value = n
            rc = lib().ig_step_draw(self._h, None, None, None, int(frag_a), 0, cbuf, C.byref(ncand), C.byref(res), sc_addr if want_scores else None)
        if rc != 0:
            _ck(rc)
        n = ncand.value
        return res, (sc[:n * N_TMP_STRUCT].copy() if want_scores else None), cbuf[:n]

    def debug_step_stats(self):
        """ig_step_draw: calls that went through mapped memory, and how many of them the one-move tail finished"""
        o = np.zeros(2, np.int64)
        _ck(lib().ig_debug_step_stats(self._h, _p(o)))
        return dict(calls=int(o[0]), tails=int(o[1]))

    def step_batch(self, frags, cands):
        """frags: (n,), cands: (n, max_c) -1 padded -> structured array of MOVE_RESULT_DTYPE"""
        f = np.ascontiguousarray(frags, np.int32)
        c = np.ascontiguousarray(cands, np.int32)
        assert c.ndim == 2 and c.shape[0] == f.size
        res = np.zeros(f.size, MOVE_RESULT_DTYPE)
        _ck(lib().ig_step_batch(self._h, f.size, _p(f), _p(c), c.shape[1], _p(res)))
        return res

    def step_batch_draw(self, neighbours, frags, n_neighbours):
        """len(frags) complete step_sampler calls, candidate draw included (numpy's global generator is advanced exactly as
        the reference's loop would) -> (results, candidate lists)"""
        f = np.ascontiguousarray(frags, np.int32)
        res = np.zeros(f.size, MOVE_RESULT_DTYPE)
        cands = np.full((f.size, int(n_neighbours)), -1, np.int32)
        addr = Neighbours.numpy_mt_address()
        if addr:  # on numpy's generator state in place (this thread waits inside the call while the library's thread draws)
            with Neighbours.numpy_mt_lock():
                rc = lib().ig_step_batch_draw(self._h, neighbours._h, addr, addr + 624 * 4, f.size, _p(f), int(n_neighbours), _p(cands), _p(res))
            _ck(rc)
            return res, cands
        key, pos, rest = Neighbours.take_numpy_state()
        cpos = C.c_int32(pos)
        rc = lib().ig_step_batch_draw(self._h, neighbours._h, _p(key), C.byref(cpos), f.size, _p(f), int(n_neighbours), _p(cands), _p(res))
        Neighbours.put_numpy_state(key, cpos.value, rest)
        _ck(rc)
        return res, cands

    # ---- a move and the nuisance step behind it, in flight together
    def nuis_begin(self, frag_a, cands, p_test8, mean_subfrag_kb):
        c = np.ascontiguousarray(cands, np.int32)
        p = np.ascontiguousarray(p_test8, np.float32)
        _ck(lib().ig_nuis_begin(self._h, int(frag_a), _p(c), c.size, _p(p), float(mean_subfrag_kb)))

    def links_inverse(self):
        return bool(lib().ig_links_inverse(self._h))

    def nuis_run_begin(self, frags, cands):
        """the lists of a run of (move, nuisance step) pairs: the moves are scored ahead in batches (ig_nuis_run_begin)"""
        f = np.ascontiguousarray(frags, np.int32)
        c = np.ascontiguousarray(cands, np.int32)
        assert c.ndim == 2 and c.shape[0] == f.size
        _ck(lib().ig_nuis_run_begin(self._h, f.size, _p(f), _p(c), c.shape[1]))

    def nuis_step_begin(self, move, p_test8, mean_subfrag_kb):
        p = np.ascontiguousarray(p_test8, np.float32)
        _ck(lib().ig_nuis_step_begin(self._h, int(move), _p(p), float(mean_subfrag_kb)))

    def nuis_step_next(self, temperature, u, p_next_rejected, p_next_accepted, mean_subfrag_kb, has_next):
        """end of the step in flight + acceptance test + promotion + begin of the next step (ig_nuis_step_next)
        -> (move result, nz_test, z_test, accepted: 0 / 1 / 2 = undecided / 3 = accepted ahead of its exact pass: nz_test is the
        screened midpoint, the exact value comes from ``nuis_exact_result``)"""
        res = MoveResult()
        nz, z, acc = C.c_double(), C.c_double(), C.c_int32()
        pr = None if p_next_rejected is None else np.ascontiguousarray(p_next_rejected, np.float32)
        pa = None if p_next_accepted is None else np.ascontiguousarray(p_next_accepted, np.float32)
        _ck(lib().ig_nuis_step_next(self._h, float(temperature), float(u), _p(pr), _p(pa),
                                    float(mean_subfrag_kb), int(has_next), C.byref(res), C.byref(nz), C.byref(z), C.byref(acc)))
        return res, nz.value, z.value, acc.value

    def nuis_chain_begin(self, move, p_tests, u, temperature, mean_subfrag_kb):
        """the pairs move .. move + K - 1 of the run as far as the device can take them alone (ig_nuis_chain_begin; asynchronous):
        p_tests (K, 8) float32, u / temperature (K,) float64"""
        p = np.ascontiguousarray(p_tests, np.float32)
        uu = np.ascontiguousarray(u, np.float64)
        tt = np.ascontiguousarray(temperature, np.float64)
        assert p.ndim == 2 and p.shape[1] == 8 and uu.size == p.shape[0] == tt.size
        _ck(lib().ig_nuis_chain_begin(self._h, int(move), p.shape[0], _p(p), _p(uu), _p(tt), float(mean_subfrag_kb)))

    def nuis_chain_done(self):
        return bool(lib().ig_nuis_chain_done(self._h))

    def nuis_chain_end(self):
        """-> (pairs completed: each a move decided and a step rejected, index into CHAIN_REASONS of why the chain ended)"""
        n, r = C.c_int32(), C.c_int32()
        _ck(lib().ig_nuis_chain_end(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def debug_nuis_chain_stats(self):
        o = np.zeros(10, np.int64)
        _ck(lib().ig_debug_nuis_chain_stats(self._h, _p(o)))
        return dict(calls=int(o[0]), segments=int(o[1]), pairs=int(o[2]), ends={k: int(v) for k, v in zip(CHAIN_REASONS, o[3:10])})

    def nuis_exact_result(self):
        """exact nz_test of the last step ``nuis_step_next`` reported as accepted = 3 (decided from the screened interval)"""
        nz = C.c_double()
        _ck(lib().ig_nuis_exact_result(self._h, C.byref(nz)))
        return nz.value

    def nuis_end(self):
        res = MoveResult()
        nz, z = C.c_double(), C.c_double()
        _ck(lib().ig_nuis_end(self._h, C.byref(res), C.byref(nz), C.byref(z), None))
        return res, nz.value, z.value

    def nuis_accept(self):
        _ck(lib().ig_nuis_accept(self._h))

    # ---- speculative batches in steps (slots of a batch split over several GPUs)
    def batch_max_width(self, max_c=5):
        return int(lib().ig_batch_max_width(self._h, int(max_c)))

    def batch_upload(self, frags, cands, max_w):
        f = np.ascontiguousarray(frags, np.int32)
        c = np.ascontiguousarray(cands, np.int32)
        assert c.ndim == 2 and c.shape[0] == f.size
        _ck(lib().ig_batch_upload(self._h, f.size, _p(f), _p(c), c.shape[1], int(max_w)))

    def batch_score(self, move0, w, slot_begin, slot_end):
        _ck(lib().ig_batch_score(self._h, int(move0), int(w), int(slot_begin), int(slot_end)))

    def batch_records(self):
        """-> (device pointer, bytes per slot) of the slot-major score records: slot w lives at pointer + w * bytes"""
        p1 = C.c_void_p()
        b1 = C.c_int64()
        _ck(lib().ig_batch_records(self._h, C.byref(p1), C.byref(b1)))
        return p1.value, b1.value

    def batch_commit(self, move0, w):
        n = C.c_int32()
        _ck(lib().ig_batch_commit(self._h, int(move0), int(w), C.byref(n)))
        return n.value

    def batch_results(self, n_moves):
        res = np.zeros(int(n_moves), MOVE_RESULT_DTYPE)
        _ck(lib().ig_batch_results(self._h, int(n_moves), _p(res)))
        return res

    def debug_tile_trace(self):
        """one from-scratch pass -> (n, 4) int64: start, end (100 MHz clock), XCC_ID << 32 | HW_ID, contacts of every workgroup"""
        n = C.c_int64()
        _ck(lib().ig_debug_tile_trace(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), np.int64)
        _ck(lib().ig_debug_tile_trace(self._h, _p(out), n.value, C.byref(n)))
        return out

    def debug_diff_trace(self, p_test8, mean_subfrag_kb):
        """one screened nuisance pass under p_test -> ((n, 8) int64 per-workgroup clocks, the pass's 8 output words)"""
        p = np.ascontiguousarray(p_test8, np.float32)
        n = C.c_int64()
        _ck(lib().ig_debug_diff_trace(self._h, _p(p), float(mean_subfrag_kb), None, 0, C.byref(n), None))
        out = np.zeros((n.value, 8), np.int64)
        sums = np.zeros(8, np.int64)
        _ck(lib().ig_debug_diff_trace(self._h, _p(p), float(mean_subfrag_kb), _p(out), n.value, C.byref(n), _p(sums)))
        return out, sums

    def debug_nuis_wait(self):
        s = C.c_double()
        _ck(lib().ig_debug_nuis_wait(self._h, C.byref(s)))
        return s.value

    def debug_nuis_screen_stats(self):
        """the screened nuisance pass (csrc/ig_kernels_nuis.cuh): steps screened, rejected from the interval alone, exact passes
        run behind a screened one, void, largest bound, largest |screened - exact| / bound, mean bound, undecided"""
        o = np.zeros(12, np.float64)
        _ck(lib().ig_debug_nuis_screen_stats(self._h, _p(o)))
        n = max(o[0] - o[3], 1.0)
        return dict(screened=int(o[0]), rejected_screened=int(o[1]), exact_passes=int(o[2]), void=int(o[3]), largest_bound=float(o[4]),
                    largest_used_fraction=float(o[5]), mean_bound=float(o[6] / n), undecided=int(o[7]),
                    void_why=dict(parameters=int(o[8]), contact=int(o[9]), sums=int(o[10]), no_record=int(o[11])))

    def debug_nuis_hist_stats(self):
        """the histogram tier of the screened nuisance pass: evaluations, steps rejected / accepted there, void, mean bound, largest
        |screened - exact| / bound, moves walked into the histogram, builds from scratch"""
        o = np.zeros(12, np.float64)
        _ck(lib().ig_debug_nuis_hist_stats(self._h, _p(o)))
        n = max(o[0] - o[3], 1.0)
        return dict(evaluated=int(o[0]), rejected=int(o[1]), accepted=int(o[2]), void=int(o[3]), mean_bound=float(o[4] / n),
                    largest_used_fraction=float(o[5]), walks=int(o[6]), builds=int(o[7]),
                    void_why=dict(parameters=int(o[8]), contact=int(o[9]), sums=int(o[10]), no_record=int(o[11])))

    def debug_zero_fallbacks(self):
        """moves that were scored again with every column exact because a contender's score came out as exactly 0.0"""
        n = C.c_int64()
        _ck(lib().ig_debug_zero_fallbacks(self._h, C.byref(n)))
        return int(n.value)

    def debug_round_census(self, clear=False):
        """how the decide rounds of this handle ended since the census was switched on (``debug_set_round_census``) -> dict over
        ROUND_CENSUS; counts depend on timing, the identities between them do not"""
        o = np.zeros(16, np.int32)
        _ck(lib().ig_debug_round_census(self._h, _p(o), int(bool(clear))))
        return dict(zip(ROUND_CENSUS, (int(x) for x in o)))

    def debug_pool_retries(self):
        """moves of the one-move path repeated with a larger slice pool (their lists did not fit)"""
        n = C.c_int64()
        _ck(lib().ig_debug_pool_retries(self._h, C.byref(n)))
        return int(n.value)

    def debug_window_budget(self, nbytes=0.0):
        """set the bytes the per-window arrays of this handle's move buffers may take (<= 0: the default, 64e9) and size them again ->
        the move slots they hold now (0: no move buffers yet)"""
        n = C.c_int32()
        _ck(lib().ig_debug_window_budget(self._h, float(nbytes), C.byref(n)))
        return int(n.value)

    def debug_nuis_hist_check(self):
        """words of the maintained histogram that differ from one built from scratch (-1: no histogram kept)"""
        n = C.c_int64()
        _ck(lib().ig_debug_nuis_hist_check(self._h, C.byref(n)))
        return int(n.value)

    def batch_stats(self):
        o = np.zeros(4, np.int64)
        _ck(lib().ig_batch_stats(self._h, _p(o)))
        w = np.zeros(2, np.int64)  # contacts in the CSR rows the slice kernel walked / that a walk per candidate would have read
        _ck(lib().ig_slice_walk_stats(self._h, _p(w)))
        return dict(batches=int(o[0]), committed_in_batch=int(o[1]), one_move_tails=int(o[2]), predicted_deltas=int(o[3]),
                    slice_contacts_walked=int(w[0]), slice_contacts_walked_per_candidate=int(w[1]))

    def scratch_bytes(self):
        """bytes of the move buffers: (per-window arrays, slice pool, the rest)"""
        o = np.zeros(3, np.int64)
        _ck(lib().ig_scratch_bytes(self._h, _p(o)))
        return int(o[0]), int(o[1]), int(o[2])

    # ---- the contact map of the current genome (display_current_matrix CL:2555-2605)
    def contact_map_order(self):
        """the placed sub-fragments in the order of the genome (the reference's full_order_high) -> int32 array"""
        out = np.zeros(max(self.M, 1), np.int32)
        n = C.c_int32()
        _ck(lib().ig_contact_map_order(self._h, _p(out), C.byref(n)))
        return out[:n.value].copy()

    def contact_map(self, max_side):
        """the contacts under that order, ``bin`` positions per pixel so that the side stays within ``max_side``
        -> (image int64 [side, side], bin); self-contacts are not in it (the device holds the strict upper triangle)"""
        from .contact_map import binning

        max_side = int(max_side)
        if not 1 <= max_side <= 2 ** 31 - 1:
            raise HipError("contact_map: max_side must be >= 1 (got %d)" % max_side)
        cap = min(max_side, max(self.M, 1))  # side <= min(max_side, T), T <= M
        if cap * cap > 1 << 26:  # (a buffer of that many entries only if the image really has them)
            cap = max(binning(self.contact_map_order().size, max_side)[1], 1)
        img = np.empty(cap * cap, np.int64)
        side, b = C.c_int32(), C.c_int32()
        _ck(lib().ig_contact_map(self._h, max_side, _p(img), img.size, C.byref(side), C.byref(b)))
        n = side.value
        return img[:n * n].reshape(n, n).copy(), b.value

    def debug_contact_map_time(self, max_side, combine=True, n=1):
        """the map's pass n times with hipEvents around each -> (milliseconds [n], sum of the last image)"""
        ms = np.zeros(int(n), np.float32)
        tot = C.c_int64()
        _ck(lib().ig_debug_contact_map_time(self._h, int(max_side), int(bool(combine)), int(n), _p(ms), C.byref(tot)))
        return ms, int(tot.value)

    # ---- the distance law of the current genome (the rule: distance_law.py)
    def distance_law(self, edges, pairs=True):
        """observed contacts and sub-fragment pairs per bin of separation under ``edges`` (ascending f32, kb) -> dict: edges,
        observed, pairs (int64 [len(edges) - 1]; None with ``pairs=False``) and the int64 scalars of ``distance_law.SCALARS``"""
        from .distance_law import SCALARS

        e = np.ascontiguousarray(edges, np.float32).ravel()
        nb = max(int(e.size) - 1, 1)
        obs = np.zeros(nb, np.int64)
        prs = np.zeros(nb, np.int64) if pairs else None
        sc = np.zeros(8, np.int64)
        _ck(lib().ig_distance_law(self._h, _p(e), int(e.size), _p(obs), _p(prs), _p(sc)))
        out = dict(edges=e, observed=obs, pairs=prs)
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def debug_distance_law_time(self, edges, privatised=True, n=1, pairs=True):
        """the law's passes n times each with hipEvents around each -> (ms observed [n], ms pairs [n] or None, checksum of the
        last observed pass)"""
        e = np.ascontiguousarray(edges, np.float32).ravel()
        ms_o = np.zeros(int(n), np.float32)
        ms_p = np.zeros(int(n), np.float32) if pairs else None
        ck = C.c_int64()
        _ck(lib().ig_debug_distance_law_time(self._h, _p(e), int(e.size), int(bool(privatised)), int(n), _p(ms_o), _p(ms_p), C.byref(ck)))
        return ms_o, ms_p, int(ck.value)

    # ---- the junction support profile of the current genome (the rule: junction_profile.py)
    def junction_profile(self, window, model=True):
        """per junction of the genome order the contacts that span it inside ``window`` positions, the pairs that could and the
        model's quantised expectation -> dict: window, n_placed, observed, pairs, expected_q (int64 [n_placed]; the last two None
        with ``model=False``) and the int64 scalars of ``junction_profile.SCALARS``"""
        from .junction_profile import SCALARS

        cap = max(self.M, 1)
        obs = np.zeros(cap, np.int64)
        prs = np.zeros(cap, np.int64) if model else None
        exq = np.zeros(cap, np.int64) if model else None
        sc = np.zeros(8, np.int64)
        n = C.c_int32()
        _ck(lib().ig_junction_profile(self._h, int(window), _p(obs), _p(prs), _p(exq), cap, C.byref(n), _p(sc)))
        T = n.value
        out = dict(window=int(window), n_placed=T, observed=obs[:T].copy(), pairs=prs[:T].copy() if model else None,
                   expected_q=exq[:T].copy() if model else None)
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def debug_junction_profile_time(self, window, combine=True, n=1, model=True, scan=True):
        """the profile's passes n times each with hipEvents around each -> (ms observed [n], ms model [n] or None, ms scan [n] or
        None, checksum of the observed profile behind the last pass)"""
        ms_o = np.zeros(int(n), np.float32)
        ms_m = np.zeros(int(n), np.float32) if model else None
        ms_s = np.zeros(int(n), np.float32) if scan else None
        ck = C.c_int64()
        _ck(lib().ig_debug_junction_profile_time(self._h, int(window), int(bool(combine)), int(n), _p(ms_o), _p(ms_m), _p(ms_s), C.byref(ck)))
        return ms_o, ms_m, ms_s, int(ck.value)

    # ---- the expected contact map of the current genome (the rule: expected_map.py)
    def expected_map(self, max_side):
        """what the model in use predicts for the pixels of ``contact_map(max_side)`` -> dict: side, bin, the int64 [side, side]
        images ``cis_q``, ``cis_pairs``, ``ring_pairs`` and the int64 scalars of ``expected_map.SCALARS``"""
        from .contact_map import binning
        from .expected_map import IMAGES, SCALARS

        max_side = int(max_side)
        if not 1 <= max_side <= 2 ** 31 - 1:
            raise HipError("expected_map: max_side must be >= 1 (got %d)" % max_side)
        cap = min(max_side, max(self.M, 1))  # side <= min(max_side, T), T <= M
        if cap * cap > 1 << 24:  # (three buffers of that many entries only if the images really have them)
            cap = max(binning(self.contact_map_order().size, max_side)[1], 1)
        img = np.empty((3, cap * cap), np.int64)
        side, b = C.c_int32(), C.c_int32()
        sc = np.zeros(8, np.int64)
        _ck(lib().ig_expected_map(self._h, max_side, _p(img[0]), _p(img[1]), _p(img[2]), cap * cap, C.byref(side), C.byref(b), _p(sc)))
        n = side.value
        out = dict(side=n, bin=b.value)
        out.update((k, img[i, :n * n].reshape(n, n).copy()) for i, k in enumerate(IMAGES))
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def debug_expected_map_form(self, form=0):
        """the form of this handle's builds: 0 / "default", 1 / "rows", 2 / "tiles", 3 / "tiles_plain" (``expected_map.FORMS``)"""
        from .expected_map import FORMS

        _ck(lib().ig_debug_expected_map_form(self._h, FORMS.index(form) if form in FORMS else int(form)))

    def debug_expected_map_time(self, max_side, form=0, n=1):
        """the build under ``form`` n times with hipEvents around each -> (milliseconds [n], checksum of the last build)"""
        from .expected_map import FORMS

        ms = np.zeros(int(n), np.float32)
        ck = C.c_int64()
        _ck(lib().ig_debug_expected_map_time(self._h, int(max_side), FORMS.index(form) if form in FORMS else int(form), int(n), _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- the contacts in the coordinates of the current genome (the rule: assembly_contacts.py)
    def assembly_contacts(self, level="sub"):
        """builds the contacts re-indexed to the units of the genome order (``"sub"``: positions, ``"bin"``: placed bins) and
        sorted, as a snapshot on the device -> dict: level, rowptr (int64 [n_units + 1]), n_entries and the int64 scalars of
        ``assembly_contacts.SCALARS``; the entries come through ``assembly_contacts_fetch``"""
        from .assembly_contacts import LEVELS, SCALARS

        lv = LEVELS.index(level) if level in LEVELS else int(level)
        nu, ne = C.c_int64(), C.c_int64()
        sc = np.zeros(8, np.int64)
        _ck(lib().ig_assembly_contacts_build(self._h, lv, C.byref(nu), C.byref(ne), _p(sc)))
        rowptr = np.zeros(nu.value + 1, np.int64)
        _ck(lib().ig_assembly_contacts_rows(self._h, _p(rowptr), rowptr.size))
        out = dict(level=LEVELS[lv], rowptr=rowptr, n_entries=int(ne.value))
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def assembly_contacts_fetch(self, first, n):
        """entries first .. first + n - 1 of the built result -> (col int32 [n], count int64 [n])"""
        n = int(n)
        col, cnt = np.zeros(max(n, 0), np.int32), np.zeros(max(n, 0), np.int64)
        _ck(lib().ig_assembly_contacts_fetch(self._h, int(first), n, _p(col), _p(cnt)))
        return col, cnt

    def assembly_contacts_release(self):
        _ck(lib().ig_assembly_contacts_release(self._h))

    def debug_assembly_contacts_limits(self, short_max=0, lds_max=0):
        """the row lengths up to which the build sorts a row with a wave / with a workgroup in LDS (0: the default)"""
        _ck(lib().ig_debug_assembly_contacts_limits(self._h, int(short_max), int(lds_max)))

    def debug_assembly_contacts_combine(self, combine=True):
        """the two passes over the contacts: one atomic per run of a wave's lanes with the same row (True, the default) or one per
        contact (False, the yardstick)"""
        _ck(lib().ig_debug_assembly_contacts_combine(self._h, int(bool(combine))))

    def debug_assembly_contacts_forms(self):
        """the last build's work lists -> dict of (rows, entries) per sort form, the runs of the long rows, the longest long row"""
        o = np.zeros(8, np.int64)
        _ck(lib().ig_debug_assembly_contacts_forms(self._h, _p(o)))
        return dict(short=(int(o[0]), int(o[1])), lds=(int(o[2]), int(o[3])), long=(int(o[4]), int(o[5])), runs=int(o[6]), longest=int(o[7]))

    def debug_set_bin_active(self, bin_id, active):
        """tests: the ``activ`` flag of one bin on the device (a contig with an inactive bin is not placed in the genome order)"""
        _ck(lib().ig_debug_set_bin_active(self._h, int(bin_id), int(bool(active))))

    def debug_assembly_contacts_time(self, level="sub", n=1):
        """the build n times with hipEvents around each pass -> (ms [n, 7]: ``ASSEMBLY_CONTACTS_PASSES``, checksum of the last result)"""
        from .assembly_contacts import LEVELS

        ms = np.zeros((int(n), len(ASSEMBLY_CONTACTS_PASSES)), np.float32)
        ck = C.c_int64()
        _ck(lib().ig_debug_assembly_contacts_time(self._h, LEVELS.index(level), int(n), _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- fixed-resolution maps: a caller's unit per position, and a built level coarsened (the rule: zoom_levels.py)
    @staticmethod
    def _unit_table(unit, n_units, what):
        from .zoom_levels import MAX_UNITS

        src = np.asarray(unit)
        if src.ndim != 1 or not (src.size == 0 or np.issubdtype(src.dtype, np.integer)):
            raise HipError("%s: one vector of integers" % what)
        if int(n_units) < 0 or int(n_units) > MAX_UNITS:
            raise HipError("%s: n_units is 0 .. 2^31 - 1 (got %d)" % (what, int(n_units)))
        if src.size and (int(src.min()) < -(1 << 31) or int(src.max()) >= 1 << 31):
            raise HipError("%s: out of range (a unit is 32 bits)" % what)
        return np.ascontiguousarray(src, np.int32)

    def _lift_result(self, n_units, ne, sc):
        from .assembly_contacts import SCALARS

        rowptr = np.zeros(int(n_units) + 1, np.int64)
        _ck(lib().ig_assembly_contacts_rows(self._h, _p(rowptr), rowptr.size))
        out = dict(rowptr=rowptr, n_entries=int(ne.value))
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def assembly_contacts_units(self, unit, n_units):
        """``assembly_contacts("bin")`` with the caller's unit of every position of ``contact_map_order`` (non-decreasing, inside
        0 .. n_units - 1, gaps allowed) -> dict: rowptr (int64 [n_units + 1]), n_entries and the scalars of
        ``assembly_contacts.SCALARS``; a snapshot: the entries come through ``assembly_contacts_fetch``"""
        t = self._unit_table(unit, n_units, "assembly_contacts_units: unit table")
        ne, sc = C.c_int64(), np.zeros(8, np.int64)
        _ck(lib().ig_assembly_contacts_build_units(self._h, _p(t), t.size, int(n_units), C.byref(ne), _p(sc)))
        return self._lift_result(n_units, ne, sc)

    def assembly_contacts_coarsen(self, coarse_of_unit, n_coarse):
        """replaces the built, summed snapshot by its coarsening under ``coarse_of_unit`` (one entry per unit of the snapshot,
        non-decreasing, inside 0 .. n_coarse - 1) without reading the contacts again -> dict as ``assembly_contacts_units``; a
        refusal leaves nothing built"""
        t = self._unit_table(coarse_of_unit, n_coarse, "assembly_contacts_coarsen: coarse map")
        ne, sc = C.c_int64(), np.zeros(8, np.int64)
        _ck(lib().ig_assembly_contacts_coarsen(self._h, _p(t), t.size, int(n_coarse), C.byref(ne), _p(sc)))
        return self._lift_result(n_coarse, ne, sc)

    # ---- read pairs lifted onto the current genome (the rule: pairs_lift.py)
    @staticmethod
    def _i32(a, what):
        src = np.asarray(a)
        if src.ndim != 1 or not (src.size == 0 or src.dtype.kind in "iu"):
            raise HipError("%s: one vector of integers" % what)
        if src.size and (int(src.min()) < -(1 << 31) or int(src.max()) >= 1 << 31):
            raise HipError("%s: out of range (32 bits)" % what)
        return np.ascontiguousarray(src, np.int32)

    def pairs_begin(self, table, reserve_pairs=0):
        """opens the session over ``pairs_lift.source_table``'s dict: the table goes to the device, the store is empty"""
        iv = table["intervals"]
        rowptr = self._i32(table["src_rowptr"], "pairs_begin: src_rowptr")
        cols = [self._i32(iv[k], "pairs_begin: " + k) for k in ("src_start", "src_end", "new_start", "scaffold", "position")]
        rev = np.ascontiguousarray(iv["reversed"] != 0, np.uint8)
        slen = np.ascontiguousarray(table["scaffold_len"], np.int64)
        unit = self._i32(table["bin_unit"], "pairs_begin: bin_unit")
        _ck(lib().ig_pairs_begin(self._h, _p(rowptr), rowptr.size - 1, _p(cols[0]), _p(cols[1]), _p(cols[2]), _p(cols[3]), _p(rev), _p(cols[4]),
                                 iv.size, _p(slen), slen.size, _p(unit), unit.size, int(table["n_bin_units"]), int(reserve_pairs)))

    def pairs_lift(self, c1, p1, c2, p2, strands=None, outputs=True):
        """one chunk: contig ids and 1-based positions (a position outside 1 .. 2^31 - 1 is covered by nothing), ``strands``: uint8 codes
        or None -> the dict ``pairs_lift.lift_host`` returns (without the per-pair arrays where ``outputs`` is False) plus
        ``pairs_stored``; the kept pairs are appended to the session's store"""
        from .pairs_lift import SCALARS

        def ids(a):
            if isinstance(a, np.ndarray) and a.dtype == np.int32:  # (as they are: a negative id is an unknown contig)
                return np.ascontiguousarray(a.ravel())
            a = np.asarray(a, np.int64).ravel()
            return np.ascontiguousarray(np.where((a < 0) | (a >= 1 << 31), -1, a), np.int32)

        def pos(a):
            if isinstance(a, np.ndarray) and a.dtype == np.int32:  # (as they are: a position below 1 is covered by nothing)
                return np.ascontiguousarray(a.ravel())
            a = np.asarray(a, np.int64).ravel()
            return np.ascontiguousarray(np.where((a < 1) | (a >= 1 << 31), 0, a), np.int32)

        a = [ids(c1), pos(p1), ids(c2), pos(p2)]
        n = a[0].size
        if any(x.size != n for x in a):
            raise HipError("pairs_lift: the four arrays of the pairs have one length")
        st = None
        if strands is not None:
            st = np.ascontiguousarray(strands, np.uint8).ravel()
            if st.size != n:
                raise HipError("pairs_lift: one strand code per pair")
        sc = np.zeros(8, np.int64)
        out = {}
        if outputs:
            for k in ("scaffold1", "pos1", "unit1", "scaffold2", "pos2", "unit2"):
                out[k] = np.zeros(n, np.int32)
            for k in ("rev1", "rev2", "status"):
                out[k] = np.zeros(n, np.uint8)
        o = lambda k: _p(out[k]) if outputs else None  # noqa: E731
        _ck(lib().ig_pairs_lift(self._h, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), None if st is None else _p(st), n, o("scaffold1"), o("pos1"), o("unit1"),
                                o("rev1"), o("scaffold2"), o("pos2"), o("unit2"), o("rev2"), o("status"), _p(sc)))
        out.update((k, int(v)) for k, v in zip(SCALARS[:6], sc))
        return out

    def pairs_pixels(self, kind, binsize=0):
        """the pixels of the stored pairs (``kind``: one of ``pairs_lift.UNIT_KINDS``) as the handle's assembly-contacts snapshot -> dict
        as ``assembly_contacts_units``; the entries come through ``assembly_contacts_fetch``, a zoom chain through
        ``assembly_contacts_coarsen``"""
        from .pairs_lift import UNIT_KINDS

        nu, ne, sc = C.c_int64(), C.c_int64(), np.zeros(8, np.int64)
        _ck(lib().ig_pairs_pixels_build(self._h, UNIT_KINDS.index(kind) if kind in UNIT_KINDS else int(kind), int(binsize), C.byref(nu),
                                        C.byref(ne), _p(sc)))
        return self._lift_result(nu.value, ne, sc)

    def pairs_law(self, edges_bp, flip_strands=True):
        """-> (counts int64 [4][n_edges - 1], dict of pairs_stored, pairs_cis, pairs_trans)"""
        e = np.ascontiguousarray(edges_bp, np.int64).ravel()
        counts, sc = np.zeros((4, max(e.size - 1, 1)), np.int64), np.zeros(8, np.int64)
        _ck(lib().ig_pairs_law(self._h, _p(e), e.size, int(bool(flip_strands)), _p(counts), _p(sc)))
        return counts, dict(pairs_stored=int(sc[0]), pairs_cis=int(sc[1]), pairs_trans=int(sc[2]))

    def pairs_clear(self):
        _ck(lib().ig_pairs_clear(self._h))

    def pairs_end(self):
        _ck(lib().ig_pairs_end(self._h))

    def debug_pairs_time(self, c1, p1, c2, p2, strands, kind, binsize, edges_bp, n=1):
        """the lift of the chunk, the law and the pixel build n times with hipEvents around each pass -> (ms [n, 9]: ``PAIRS_PASSES``,
        checksum)"""
        from .pairs_lift import UNIT_KINDS

        a = [self._i32(x, "debug_pairs_time") for x in (c1, p1, c2, p2)]
        st = None if strands is None else np.ascontiguousarray(strands, np.uint8).ravel()
        e = np.ascontiguousarray(edges_bp, np.int64).ravel()
        ms = np.zeros((int(n), len(PAIRS_PASSES)), np.float32)
        ck = C.c_int64()
        _ck(lib().ig_debug_pairs_time(self._h, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), None if st is None else _p(st), a[0].size,
                                      UNIT_KINDS.index(kind), int(binsize), _p(e), e.size, int(n), _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- the input folder from a FASTA and read pairs (the rule: pre.py)
    def pre_begin(self, seq, rec_off, rec_len):
        """opens the session over ``pre.concatenate``'s arrays: the records one behind the other, a zero byte behind each"""
        s = np.ascontiguousarray(seq, np.uint8).ravel()
        off = np.ascontiguousarray(rec_off, np.int64).ravel()
        ln = self._i32(rec_len, "pre_begin: rec_len")
        if off.size != ln.size:
            raise HipError("pre_begin: one offset and one length per record")
        _ck(lib().ig_pre_begin(self._h, _p(s), s.size, _p(off), _p(ln), ln.size))
        self._pre_records = int(ln.size)

    def pre_digest(self, enzymes, piece=1 << 22, times=False):
        """``enzymes``: [(site, cut)] -> the dict ``pre.digest`` returns without the names, plus ``gc_count`` (int64 [n_frags]) and
        with ``times`` ``ms`` (float32 [4]: ``PRE_DIGEST_PASSES``)"""
        from . import pre

        enzymes = pre.expand_enzymes(enzymes)
        R = getattr(self, "_pre_records", 0)
        ln = np.array([len(s) for s, _ in enzymes], np.int32)
        cut = np.array([c for _, c in enzymes], np.int32)
        masks = np.ascontiguousarray(np.stack([pre.site_masks(s) for s, _ in enzymes]), np.uint8)
        per, nf = np.zeros(R, np.int64), C.c_int64()
        ms = np.zeros(len(PRE_DIGEST_PASSES), np.float32) if times else None
        _ck(lib().ig_pre_digest(self._h, ln.size, _p(ln), _p(cut), _p(masks), _p(per), C.byref(nf), _p(ms)))
        n = int(nf.value)
        cols = [np.zeros(n, np.int32) for _ in range(4)]
        for a in range(0, n, int(piece)):
            m = min(int(piece), n - a)
            v = [x[a:a + m] for x in cols]
            _ck(lib().ig_pre_fragments(self._h, a, m, _p(v[0]), _p(v[1]), _p(v[2]), _p(v[3])))
        out = dict(rec_first=np.concatenate(([0], np.cumsum(per))).astype(np.int64), frag_rec=cols[0], start=cols[1].astype(np.int64), end=cols[2].astype(np.int64),
                   gc_count=cols[3].astype(np.int64), n_frags=n, enzymes=enzymes)
        out["rec_len"] = np.zeros(R, np.int64)
        last = out["rec_first"][1:] - 1
        out["rec_len"][:] = out["end"][last]
        if times:
            out["ms"] = ms
        return out

    def pre_add_pairs(self, c1, p1, c2, p2, times=False):
        """one chunk: record (-1: unknown) and 1-based position of both ends -> the chunk's scalars (``pre.SCALARS[:5]``, ``pairs_stored``)"""
        from .pre import SCALARS

        a = [self._i32(x, "pre_add_pairs") for x in (c1, p1, c2, p2)]
        if len({x.size for x in a}) != 1:
            raise HipError("pre_add_pairs: the four arrays of the pairs have one length")
        sc = np.zeros(8, np.int64)
        ms = np.zeros(1, np.float32) if times else None
        _ck(lib().ig_pre_add_pairs(self._h, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), a[0].size, _p(sc), _p(ms)))
        out = {k: int(sc[i]) for i, k in enumerate(SCALARS[:5])}
        out["pairs_stored"] = int(sc[5])
        if times:
            out["ms"] = float(ms[0])
        return out

    def pre_pixels(self, piece=1 << 22, times=False):
        """the pixels of the stored pairs -> the dict ``pre.pixels_host`` returns, plus ``n_frags`` and ``pairs_stored``"""
        from .pre import SCALARS

        npx, sc = C.c_int64(), np.zeros(8, np.int64)
        ms = np.zeros(len(ASSEMBLY_CONTACTS_PASSES), np.float32) if times else None
        _ck(lib().ig_pre_pixels_build(self._h, C.byref(npx), _p(sc), _p(ms)))
        U, n = int(sc[6]), int(npx.value)
        rowptr, col, count = np.zeros(U + 1, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int64)
        _ck(lib().ig_pre_pixels_rows(self._h, _p(rowptr), rowptr.size))
        for a in range(0, n, int(piece)):
            m = min(int(piece), n - a)
            vc, vn = col[a:a + m], count[a:a + m]
            _ck(lib().ig_pre_pixels_fetch(self._h, a, m, _p(vc), _p(vn)))
        out = dict(rowptr=rowptr, col=col.astype(np.int64), count=count)
        out.update({k: int(sc[i]) for i, k in enumerate(SCALARS)})
        out.update(n_frags=U, pairs_stored=int(sc[7]))
        if times:
            out["ms"] = ms
        return out

    def pre_clear(self):
        _ck(lib().ig_pre_clear(self._h))

    def pre_end(self):
        _ck(lib().ig_pre_end(self._h))

    # ---- 4DN pairs text (the rule: pairs_text.py)
    def text_begin(self, names):
        """opens the session over the vocabulary ``names``: {contig name: id}"""
        from . import pairs_text

        b, off, ids = pairs_text.vocabulary(names)
        b = np.ascontiguousarray(b, np.uint8)
        _ck(lib().ig_text_begin(self._h, _p(b), _p(off), _p(ids), ids.size))

    def text_parse(self, buf, cols=(1, 2, 3, 4, 5, 6), times=False):
        """one chunk of whole lines (bytes or uint8) under the six column indices -> dict: ``counts`` (lines, data, comment, malformed,
        deferred), ``first_columns_line``, ``to_host`` and with ``times`` ``ms`` (float32 [4]: ``TEXT_PASSES``); the arrays stay on the
        device for ``text_fetch`` / ``text_feed_pre`` / ``text_feed_pairs``"""
        a = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.ascontiguousarray(buf, np.uint8).ravel()
        cc = np.ascontiguousarray(cols, np.int32).ravel()
        if cc.size != 6:
            raise HipError("text_parse: six column indices (got %d)" % cc.size)
        sc = np.zeros(8, np.int64)
        ms = np.zeros(len(TEXT_PASSES), np.float32) if times else None
        _ck(lib().ig_text_parse(self._h, _p(a) if a.size else None, a.size, _p(cc), _p(sc), _p(ms)))
        out = dict(counts=dict(lines=int(sc[0]), data=int(sc[1]), comment=int(sc[2]), malformed=int(sc[3]), deferred=int(sc[4])),
                   first_columns_line=int(sc[5]), to_host=bool(sc[6]))
        if times:
            out["ms"] = ms
        return out

    def text_fetch(self, res, only=None):
        """the arrays of the last chunk, ``res`` being what ``text_parse`` returned for it -> ``res`` with ``status``, ``line_start``,
        ``c1``, ``p1``, ``c2``, ``p2``, ``strands``, ``deferred`` added (``only``: the names wanted): the dict of ``pairs_text.parse_chunk``"""
        if res["to_host"]:
            return res
        n, d, f = (res["counts"][k] for k in ("lines", "data", "deferred"))
        shape = dict(status=(n, np.uint8), line_start=(n + 1, np.int32), c1=(d, np.int32), p1=(d, np.int64), c2=(d, np.int32), p2=(d, np.int64),
                     strands=(d, np.uint8), deferred=(f, np.int32))
        got = {k: np.zeros(s, t) for k, (s, t) in shape.items() if only is None or k in only}
        g = lambda k: _p(got.get(k))  # noqa: E731
        _ck(lib().ig_text_fetch(self._h, g("status"), g("line_start"), g("c1"), g("p1"), g("c2"), g("p2"), g("strands"), g("deferred")))
        res.update(got)
        return res

    def text_feed_pre(self, times=False):
        """the DATA pairs of the last chunk into the live ``pre`` store, without a round trip -> as ``pre_add_pairs``"""
        from .pre import SCALARS

        sc = np.zeros(8, np.int64)
        ms = np.zeros(1, np.float32) if times else None
        _ck(lib().ig_text_feed_pre(self._h, _p(sc), _p(ms)))
        out = {k: int(sc[i]) for i, k in enumerate(SCALARS[:5])}
        out["pairs_stored"] = int(sc[5])
        if times:
            out["ms"] = float(ms[0])
        return out

    def text_feed_pairs(self):
        """the DATA pairs of the last chunk into the live pairs session, without a round trip -> the scalars of ``pairs_lift``"""
        from .pairs_lift import SCALARS

        sc = np.zeros(8, np.int64)
        _ck(lib().ig_text_feed_pairs(self._h, _p(sc)))
        return {k: int(v) for k, v in zip(SCALARS[:6], sc)}

    def text_end(self):
        _ck(lib().ig_text_end(self._h))

    # ---- the polished FASTA of the polish step (the rule: scaffold_polish.py)
    def seq_begin(self, seq, rec_off, rec_len):
        """opens the session over ``pre.concatenate``'s arrays, like ``pre_begin``"""
        s = np.ascontiguousarray(seq, np.uint8).ravel()
        off = np.ascontiguousarray(rec_off, np.int64).ravel()
        ln = self._i32(rec_len, "seq_begin: rec_len")
        if off.size != ln.size:
            raise HipError("seq_begin: one offset and one length per record")
        _ck(lib().ig_seq_begin(self._h, _p(s), s.size, _p(off), _p(ln), ln.size))
        self._seq_records = int(ln.size)

    def seq_composition(self, times=None):
        """-> int64 [R, 8] (``scaffold_polish.CLASSES``); ``times``: a dict whose ``composition`` list gets the kernel's ms"""
        counts = np.zeros((getattr(self, "_seq_records", 0), SEQ_CLASSES), np.int64)
        ms = np.zeros(1, np.float32) if times is not None else None
        _ck(lib().ig_seq_composition(self._h, _p(counts), _p(ms)))
        if times is not None:
            times.setdefault("composition", []).append(float(ms[0]))
        return counts

    def seq_plan(self, plan):
        """uploads the tables of ``scaffold_polish.stitch_plan``"""
        a = {k: np.ascontiguousarray(plan[k], np.int64).ravel() for k in ("rec_off", "hdr_lit", "body_len", "piece_first", "start", "length", "body")}
        b = {k: np.ascontiguousarray(plan[k], np.int32).ravel() for k in ("hdr_len", "src", "ori")}
        lit = np.ascontiguousarray(plan["literal"], np.uint8).ravel()
        n_out = b["hdr_len"].size
        if a["rec_off"].size != n_out + 1 or a["piece_first"].size != n_out + 1 or a["hdr_lit"].size != n_out or a["body_len"].size != n_out:
            raise HipError("seq_plan: the tables of the output records have %d and %d + 1 entries" % (n_out, n_out))
        if len({b["src"].size, b["ori"].size, a["start"].size, a["length"].size, a["body"].size}) != 1:
            raise HipError("seq_plan: the five arrays of the pieces have one length")
        _ck(lib().ig_seq_plan(self._h, n_out, int(plan["width"]), _p(a["rec_off"]), _p(b["hdr_len"]), _p(a["hdr_lit"]), _p(a["body_len"]),
                              _p(a["piece_first"]), b["src"].size, _p(b["src"]), _p(a["start"]), _p(a["length"]), _p(b["ori"]), _p(a["body"]), _p(lit),
                              lit.size))

    def seq_window(self, first_byte, out, times=None):
        """fills ``out`` (a contiguous uint8 array) with the file's bytes from ``first_byte`` on; ``times``: ``stitch`` gets the kernel's ms"""
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable):
            raise HipError("seq_window: the window is a contiguous writeable uint8 array")
        ms = np.zeros(1, np.float32) if times is not None else None
        _ck(lib().ig_seq_window(self._h, int(first_byte), out.size, _p(out), _p(ms)))
        if times is not None:
            times.setdefault("stitch", []).append(float(ms[0]))

    def seq_out_composition(self, n_out):
        """-> int64 [n_out, 8] of the stitched bodies, once every window has been fetched in file order"""
        counts = np.zeros((int(n_out), SEQ_CLASSES), np.int64)
        _ck(lib().ig_seq_out_composition(self._h, _p(counts), counts.size))
        return counts

    def seq_end(self):
        _ck(lib().ig_seq_end(self._h))

    # ---- the contact levels of the pyramid (the rule: pyramid_levels.py)
    def pyr_begin(self, n_frags, a, b, count):
        """opens the session over the level-0 list (0-based ids, file order) -> whether the list is canonical (its own level)"""
        a, b = self._i32(a, "pyr_begin: a"), self._i32(b, "pyr_begin: b")
        cnt = np.ascontiguousarray(count, np.int64).ravel()
        if not (a.size == b.size == cnt.size):
            raise HipError("pyr_begin: one a, one b and one count per entry")
        flag = C.c_int32()
        _ck(lib().ig_pyr_begin(self._h, int(n_frags), _p(a), _p(b), _p(cnt), a.size, C.byref(flag)))
        self._pyr_frags = int(n_frags)
        return bool(flag.value)

    def pyr_matrix(self, times=None):
        """the level of the uploaded list becomes the current level -> its pixels; ``times``: a list that gets the passes' ms
        (float32 [7]: ``ASSEMBLY_CONTACTS_PASSES``)"""
        n = C.c_int64()
        ms = np.zeros(len(ASSEMBLY_CONTACTS_PASSES), np.float32) if times is not None else None
        _ck(lib().ig_pyr_matrix(self._h, C.byref(n), _p(ms)))
        if times is not None:
            times.append(ms)
        return int(n.value)

    def pyr_degrees(self):
        """-> int64 [n_frags]: the partners of every fragment of the current level (``pyramid_levels.degrees``)"""
        deg = np.zeros(getattr(self, "_pyr_frags", 0), np.int32)
        _ck(lib().ig_pyr_degrees(self._h, _p(deg)))
        return deg.astype(np.int64)

    def pyr_remap(self, lut, n_new, skip_first, times=None):
        """the next level from the current one through ``lut`` (int [n_old]: the new id or -1) -> the dict of
        ``pyramid_levels.SCALARS``; ``times`` as in ``pyr_matrix``"""
        from .pyramid_levels import SCALARS

        t = self._i32(lut, "pyr_remap: lut")
        n, sc = C.c_int64(), np.zeros(8, np.int64)
        ms = np.zeros(len(ASSEMBLY_CONTACTS_PASSES), np.float32) if times is not None else None
        _ck(lib().ig_pyr_remap(self._h, _p(t), t.size, int(n_new), 1 if skip_first else 0, C.byref(n), _p(sc), _p(ms)))
        self._pyr_frags = int(n_new)
        if times is not None:
            times.append(ms)
        return {k: int(sc[i]) for i, k in enumerate(SCALARS)}

    def pyr_level(self, piece=1 << 22):
        """the current level -> (data3: int32 [3, nnz] = rows, columns, counts; rowptr: int64 [n_frags + 1])"""
        U = getattr(self, "_pyr_frags", 0)
        rowptr = np.zeros(U + 1, np.int64)
        _ck(lib().ig_pyr_rows(self._h, _p(rowptr), rowptr.size))
        n = int(rowptr[-1])
        data3 = np.zeros((3, n), np.int32)
        for a in range(0, n, int(piece)):
            m = min(int(piece), n - a)
            v = [np.zeros(m, np.int32) for _ in range(3)]
            _ck(lib().ig_pyr_fetch(self._h, a, m, _p(v[0]), _p(v[1]), _p(v[2])))
            for k in range(3):
                data3[k, a:a + m] = v[k]
        return data3, rowptr

    def pyr_end(self):
        _ck(lib().ig_pyr_end(self._h))

    def debug_pyr_piece(self, entries):
        """entries per upload piece of ``pyr_begin`` (0: the default)"""
        _ck(lib().ig_debug_pyr_piece(self._h, int(entries)))

    def balance_build_units(self, unit, n_units, ignore_diags=2):
        """``balance_build("bin")`` with the caller's unit of every position -> the dict ``balance_build`` returns (level: "units")"""
        from .balance import SCALARS

        t = self._unit_table(unit, n_units, "balance_build_units: unit table")
        ne, sc = C.c_int64(), np.zeros(8, np.int64)
        _ck(lib().ig_balance_build_units(self._h, _p(t), t.size, int(n_units), int(ignore_diags), C.byref(ne), _p(sc)))
        U = int(n_units)
        rowptr, nnz, total = np.zeros(U + 1, np.int64), np.zeros(U, np.int64), np.zeros(U, np.int64)
        _ck(lib().ig_balance_rows(self._h, _p(rowptr), _p(nnz), _p(total), rowptr.size))
        out = dict(level="units", rowptr=rowptr, nnz=nnz, total=total, n_entries=int(ne.value))
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def debug_zoom_coarsen(self, rowptr, col, count, coarse_of_unit, n_coarse):
        """the coarsening over caller CSR data on a bare handle (tests/test_hip_zoom_levels.py) -> dict: rowptr (int64 [n_coarse + 1]),
        col (int32), count (int64), n_out, forms (as ``debug_assembly_contacts_forms``, of the segments)"""
        rowptr = np.ascontiguousarray(rowptr, np.int64)
        col, count = np.ascontiguousarray(col, np.int32), np.ascontiguousarray(count, np.int64)
        m = np.ascontiguousarray(coarse_of_unit, np.int32)
        if rowptr.ndim != 1 or rowptr.size < 1 or col.shape != count.shape or col.ndim != 1 or m.shape != (rowptr.size - 1,) or col.size != int(rowptr[-1]):
            raise HipError("debug_zoom_coarsen: rowptr [U + 1], col and count [rowptr[U]], coarse_of_unit [U]")
        no, o = C.c_int64(), np.zeros(8, np.int64)
        _ck(lib().ig_debug_zoom_coarsen(self._h, _p(rowptr), _p(col), _p(count), rowptr.size - 1, _p(m), int(n_coarse), C.byref(no), _p(o)))
        out = dict(n_out=int(no.value), rowptr=np.zeros(int(n_coarse) + 1, np.int64), col=np.zeros(no.value, np.int32), count=np.zeros(no.value, np.int64),
                   forms=dict(short=(int(o[0]), int(o[1])), lds=(int(o[2]), int(o[3])), long=(int(o[4]), int(o[5])), runs=int(o[6]), longest=int(o[7])))
        _ck(lib().ig_debug_zoom_fetch(self._h, _p(out["rowptr"]), out["rowptr"].size, _p(out["col"]), _p(out["count"]), out["n_out"]))
        return out

    def debug_zoom_time(self, n=1, coarse_of_unit=None, n_coarse=None):
        """the coarsening of the built snapshot (``coarse_of_unit`` None: two units to one) n times with hipEvents around each pass;
        the snapshot stays -> (ms [n, 6]: ``ZOOM_PASSES``, checksum of the last repeat's result)"""
        ms = np.zeros((int(n), len(ZOOM_PASSES)), np.float32)
        ck = C.c_int64()
        t = None if coarse_of_unit is None else self._unit_table(coarse_of_unit, n_coarse, "debug_zoom_time: coarse map")
        _ck(lib().ig_debug_zoom_time(self._h, _p(t), 0 if t is None else t.size, 0 if t is None else int(n_coarse), int(n), _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- the layers the reports share, over caller data (tests/test_hip_rows_direct.py)
    def debug_scan64(self, words_2d, n, sentinel=0xA5A5A5A5A5A5A5A5):
        """the reports' 64-bit scan over the first ``n`` words of every row of ``words_2d`` (uint64 [n_arrays, stride]) ->
        (out uint64 [n_arrays, stride]: the inclusive prefix sums modulo 2^64, ``sentinel`` where nothing was written; the input as the
        device holds it behind the scan)"""
        words = np.ascontiguousarray(words_2d, np.uint64)
        if words.ndim != 2:
            raise HipError("debug_scan64: the words are an array of [n_arrays, stride]")
        after = words.copy()
        out = np.full(words.shape, sentinel, np.uint64)
        _ck(lib().ig_debug_scan64(self._h, _p(after), int(n), words.shape[0], words.shape[1], _p(out)))
        return out, after

    def debug_rows_build(self, lo, word, n_rows, reduce=False, combine=True):
        """the reports' row builder over caller data: entry k goes to row ``lo[k]`` (negative: no entry) as ``word[k]`` = column << 32 |
        count -> dict: n_entries, n_out, forms (as ``debug_assembly_contacts_forms``), rowptr (int64 [n_rows + 1]) and ``word``
        (uint64 [n_out], sorted inside every row) or, reduced, ``col`` (int32 [n_out]) and ``count`` (int64 [n_out])"""
        lo = np.ascontiguousarray(lo, np.int32)
        word = np.ascontiguousarray(word, np.uint64)
        if lo.ndim != 1 or lo.shape != word.shape:
            raise HipError("debug_rows_build: lo and word are vectors of one length")
        ne, no = C.c_int64(), C.c_int64()
        o = np.zeros(8, np.int64)
        _ck(lib().ig_debug_rows_build(self._h, _p(lo), _p(word), lo.size, int(n_rows), int(bool(reduce)),
                                      int(bool(combine)), C.byref(ne), C.byref(no), _p(o)))
        out = dict(n_entries=int(ne.value), n_out=int(no.value), rowptr=np.zeros(int(n_rows) + 1, np.int64),
                   forms=dict(short=(int(o[0]), int(o[1])), lds=(int(o[2]), int(o[3])), long=(int(o[4]), int(o[5])), runs=int(o[6]), longest=int(o[7])))
        if reduce:
            out["col"], out["count"] = np.zeros(out["n_out"], np.int32), np.zeros(out["n_out"], np.int64)
        else:
            out["word"] = np.zeros(out["n_out"], np.uint64)
        _ck(lib().ig_debug_rows_fetch(self._h, _p(out["rowptr"]), out["rowptr"].size, _p(out.get("word")), _p(out.get("col")), _p(out.get("count")),
                                      out["n_out"]))
        return out

    def debug_wave_runs(self, keys, values, n_dest, wide=False):
        """the combining idiom of the passes over the contacts over caller data (tests/test_hip_wave_runs.py): entry k adds
        ``values[k]`` to ``out[keys[k]]`` (a negative key: no entry), a run of a wave's lanes with an equal key through one atomic
        -> (out int64 [n_dest], the atomics issued).  ``wide``: the sums inside the wave in 64 bits, else in 32"""
        keys = np.ascontiguousarray(keys, np.int32)
        values = np.ascontiguousarray(values, np.int64)
        if keys.ndim != 1 or keys.shape != values.shape:
            raise HipError("debug_wave_runs: keys and values are vectors of one length")
        out, n_at = np.zeros(max(int(n_dest), 0), np.int64), C.c_int64()
        _ck(lib().ig_debug_wave_runs(self._h, _p(keys), _p(values), keys.size, int(n_dest), int(bool(wide)), _p(out), C.byref(n_at)))
        return out, int(n_at.value)

    # ---- join support: which scaffold ends the contacts would link (the rule: join_support.py)
    def join_support(self, window, model=True):
        """builds the links between the ends of the placed linear contigs inside ``window`` positions as a snapshot on the device
        -> dict: window, model, rowptr (int64 [2 K + 1]), first_position, n_positions (int32 [K]: per contig), n_links and the int64
        scalars of ``join_support.SCALARS``; the links come through ``join_support_fetch``"""
        from .join_support import SCALARS

        ne, nl = C.c_int64(), C.c_int64()
        sc = np.zeros(8, np.int64)
        _ck(lib().ig_join_support_build(self._h, int(window), int(bool(model)), C.byref(ne), C.byref(nl), _p(sc)))
        K = ne.value // 2
        rowptr = np.zeros(ne.value + 1, np.int64)
        _ck(lib().ig_join_support_rows(self._h, _p(rowptr), rowptr.size))
        first, n = np.zeros(K, np.int32), np.zeros(K, np.int32)
        _ck(lib().ig_join_support_ends(self._h, _p(first), _p(n), K))
        out = dict(window=int(window), model=bool(model), rowptr=rowptr, first_position=first, n_positions=n)
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def join_support_fetch(self, first, n, model=True):
        """links first .. first + n - 1 of the built result -> (col int32 [n], observed, pairs, expected_q int64 [n]; the last two
        None with ``model=False``: a result built without the model has none)"""
        n = int(n)
        col, obs = np.zeros(max(n, 0), np.int32), np.zeros(max(n, 0), np.int64)
        prs = np.zeros(max(n, 0), np.int64) if model else None
        exq = np.zeros(max(n, 0), np.int64) if model else None
        _ck(lib().ig_join_support_fetch(self._h, int(first), n, _p(col), _p(obs), _p(prs), _p(exq)))
        return col, obs, prs, exq

    def join_support_release(self):
        _ck(lib().ig_join_support_release(self._h))

    def debug_join_support_combine(self, combine=True):
        """the two passes over the contacts of the join support: one atomic per run of a wave's lanes with the same row (True) or
        one per emission (False, the yardstick); None: the form the library ships"""
        _ck(lib().ig_debug_join_support_combine(self._h, -1 if combine is None else int(bool(combine))))

    def debug_join_support_forms(self):
        """the last join support build's work lists, as ``debug_assembly_contacts_forms``"""
        o = np.zeros(8, np.int64)
        _ck(lib().ig_debug_join_support_forms(self._h, _p(o)))
        return dict(short=(int(o[0]), int(o[1])), lds=(int(o[2]), int(o[3])), long=(int(o[4]), int(o[5])), runs=int(o[6]), longest=int(o[7]))

    def debug_join_support_time(self, window, n=1):
        """the build n times with hipEvents around each pass -> (ms [n, 9]: ``JOIN_SUPPORT_PASSES``, checksum of the observed part
        of the last result)"""
        ms = np.zeros((int(n), len(JOIN_SUPPORT_PASSES)), np.float32)
        ck = C.c_int64()
        _ck(lib().ig_debug_join_support_time(self._h, int(window), int(n), _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- orientation support: which segments the contacts would reverse (the rule: orientation_support.py)
    @staticmethod
    def _segments(first, last):
        f, l = np.asarray(first), np.asarray(last)
        if f.ndim != 1 or f.shape != l.shape or not (np.issubdtype(f.dtype, np.integer) and np.issubdtype(l.dtype, np.integer)):
            raise HipError("orientation_support: segment list: first and last are integer vectors of one length")
        if f.size and (min(f.min(), l.min()) < -2 ** 31 or max(f.max(), l.max()) >= 2 ** 31):
            raise HipError("orientation_support: segment list out of range")
        return np.ascontiguousarray(f, np.int32), np.ascontiguousarray(l, np.int32)

    def orientation_support(self, window, first, last, model=True):
        """the contacts between the arms and the flanks of the segments [first[k], last[k]] of positions, and what the model expects
        of the pairs that keep and that would flip each -> dict: window, n_placed, n_seg, first, last, geometry (int32 [n_seg, 4]:
        status, arm, left_flank, right_flank), observed (int64 [n_seg, 4]: LL, LR, RL, RR), expected_q (int64 [n_seg, 2]: keep,
        flip; None with ``model=False``) and the int64 scalars of ``orientation_support.SCALARS``"""
        from .orientation_support import SCALARS

        f, l = self._segments(first, last)
        n_seg = int(f.size)
        geo = np.zeros((n_seg, 4), np.int32)
        obs = np.zeros((n_seg, 4), np.int64)
        exq = np.zeros((n_seg, 2), np.int64) if model else None
        sc = np.zeros(8, np.int64)
        n = C.c_int32()
        _ck(lib().ig_orientation_support(self._h, int(window), int(bool(model)), n_seg, _p(f), _p(l), _p(geo), _p(obs), _p(exq), _p(sc), C.byref(n)))
        out = dict(window=int(window), n_placed=n.value, n_seg=n_seg, first=f.astype(np.int64), last=l.astype(np.int64), geometry=geo, observed=obs, expected_q=exq)
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def debug_orientation_support_time(self, window, first, last, which="observed", form=None, n=1):
        """one pass of the orientation support n times with hipEvents around each -> (ms [n], checksum of what the last pass wrote).
        ``which``: "observed" (``form``: "atomic", the yardstick, or "combined") or "model" ("default", "wave", "workgroup")"""
        forms = ORIENTATION_SUPPORT_FORMS[which]
        f, l = self._segments(first, last)
        ms = np.zeros(int(n), np.float32)
        ck = C.c_int64()
        _ck(lib().ig_debug_orientation_support_time(self._h, int(window), int(f.size), _p(f), _p(l), ("observed", "model").index(which),
                                                    forms.index(forms[0] if form is None else form), int(n), _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- gap support: the distance the contacts put across each join (the rule: gap_support.py)
    @staticmethod
    def _junctions_and_gaps(junctions, gaps_kb):
        j, g = np.asarray(junctions), np.asarray(gaps_kb)
        if j.ndim != 1 or not np.issubdtype(j.dtype, np.integer):
            raise HipError("gap_support: junction list: one integer vector")
        if j.size and (j.min() < -2 ** 31 or j.max() >= 2 ** 31):
            raise HipError("gap_support: junction list out of range")
        if g.ndim != 1:
            raise HipError("gap_support: gaps: one vector")
        return np.ascontiguousarray(j, np.int32), np.ascontiguousarray(g, np.float32)

    def gap_support(self, window, junctions, gaps_kb, model=True):
        """per listed junction the contacts that span it inside ``window`` positions and the two halves of the Poisson
        log-likelihood under every gap of ``gaps_kb`` -> dict: window, n_junctions, junction, gaps_kb, status (int32 [n_j]), geometry
        (int32 [n_j, 4]: contig, left, right, 0), observed, pairs (int64 [n_j]), log_q, expected_q (int64 [n_j, K]; expected_q None
        with ``model=False``) and the int64 scalars of ``gap_support.SCALARS``"""
        from .gap_support import SCALARS

        j, g = self._junctions_and_gaps(junctions, gaps_kb)
        n_j, K = int(j.size), int(g.size)
        status = np.zeros(max(n_j, 1), np.int32)
        geo = np.zeros((max(n_j, 1), 4), np.int32)
        obs, prs = np.zeros(max(n_j, 1), np.int64), np.zeros(max(n_j, 1), np.int64)
        lgq = np.zeros((max(n_j, 1), max(K, 1)), np.int64)
        exq = np.zeros((max(n_j, 1), max(K, 1)), np.int64) if model else None
        sc = np.zeros(8, np.int64)
        _ck(lib().ig_gap_support(self._h, int(window), int(bool(model)), n_j, _p(j), K, _p(g), _p(status), _p(geo),
                                 _p(obs), _p(prs), _p(lgq), _p(exq), _p(sc)))
        out = dict(window=int(window), n_junctions=n_j, junction=j.astype(np.int64), gaps_kb=g, status=status, geometry=geo, observed=obs, pairs=prs, log_q=lgq,
                   expected_q=exq)
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def debug_gap_support_time(self, window, junctions, gaps_kb, which="observed", n=1):
        """one pass of the gap support n times with hipEvents around each -> (ms [n], checksum of what the last pass wrote).
        ``which``: one of ``GAP_SUPPORT_PASSES`` -- "observed", or the model pass as shipped ("model"), with a wave per junction
        ("model_wave") or a workgroup per judged junction ("model_workgroup")"""
        j, g = self._junctions_and_gaps(junctions, gaps_kb)
        ms = np.zeros(int(n), np.float32)
        ck = C.c_int64()
        _ck(lib().ig_debug_gap_support_time(self._h, int(window), int(j.size), _p(j), int(g.size), _p(g),
                                            GAP_SUPPORT_PASSES.index(which), int(n), _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- placement support: where the contacts say each bin belongs (the rule: placement_support.py)
    def placement_support(self, window, min_hosts=None):
        """every placed bin of a linear contig against every other site of the genome inside ``window`` positions (``min_hosts``:
        the fewest positions a site's window must hold, default the window) -> dict: window, min_hosts, the per-bin arrays of
        ``placement_support.ARRAYS`` (int32 / int64 [N]) and the int64 scalars of ``placement_support.SCALARS``.  Nothing stays on
        the device."""
        from .placement_support import INT_ARRAYS, LONG_ARRAYS, SCALARS

        window = int(window)
        min_hosts = window if min_hosts is None else int(min_hosts)
        out = dict(window=window, min_hosts=min_hosts)
        out.update((k, np.zeros(max(self.N, 1), np.int32)) for k in INT_ARRAYS)
        out.update((k, np.zeros(max(self.N, 1), np.int64)) for k in LONG_ARRAYS)
        sc = np.zeros(7, np.int64)
        _ck(lib().ig_placement_support(self._h, window, min_hosts, *[_p(out[k]) for k in INT_ARRAYS + LONG_ARRAYS], _p(sc)))
        for k in INT_ARRAYS + LONG_ARRAYS:
            out[k] = out[k][:self.N]
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def debug_placement_support_form(self, form="default"):
        """the scan of the placement support: ``"thread"`` (a thread per row, the yardstick), ``"wave"`` (a wave per row) or
        ``"default"`` (the form the library ships: by the row's length)"""
        _ck(lib().ig_debug_placement_support_form(self._h, PLACEMENT_SUPPORT_FORMS.index(form)))

    def debug_placement_support_forms(self):
        """the last placement support call's work lists, as ``debug_assembly_contacts_forms``"""
        o = np.zeros(8, np.int64)
        _ck(lib().ig_debug_placement_support_forms(self._h, _p(o)))
        return dict(short=(int(o[0]), int(o[1])), lds=(int(o[2]), int(o[3])), long=(int(o[4]), int(o[5])), runs=int(o[6]), longest=int(o[7]))

    def debug_placement_support_time(self, window, min_hosts=None, n=1):
        """the call n times with hipEvents around each pass -> (ms [n, 10]: ``PLACEMENT_SUPPORT_PASSES``, checksum of the arrays of
        the last call)"""
        ms = np.zeros((int(n), len(PLACEMENT_SUPPORT_PASSES)), np.float32)
        ck = C.c_int64()
        _ck(lib().ig_debug_placement_support_time(self._h, int(window), int(window) if min_hosts is None else int(min_hosts), int(n),
                                                  _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- segment placement support: where the contacts say a run of bins belongs, and which way round (the rule: segment_placement.py)
    @staticmethod
    def _placement_segments(first, last):
        f, l = np.asarray(first), np.asarray(last)
        if f.ndim != 1 or f.shape != l.shape or not (np.issubdtype(f.dtype, np.integer) and np.issubdtype(l.dtype, np.integer)):
            raise HipError("segment_placement: segment list: first and last are integer vectors of one length")
        if f.size and (min(f.min(), l.min()) < -2 ** 31 or max(f.max(), l.max()) >= 2 ** 31):
            raise HipError("segment_placement: segment list out of range")
        return np.ascontiguousarray(f, np.int32), np.ascontiguousarray(l, np.int32)

    def segment_placement(self, window, first, last, min_hosts=None):
        """every segment [first[i], last[i]] of positions of a linear contig against every other site of the genome inside ``window``
        positions, the segment itself taken out of the order, and the four sums by arm and part of the window at its home, its best
        site and the runner-up -> dict: window, min_hosts, n_seg, first, last, the per-segment arrays of ``segment_placement.ARRAYS``
        (int32 / int64 [n_seg]), ``quadrants`` (int64 [n_seg, 3, 4]) and the int64 scalars of ``segment_placement.SCALARS``.
        Nothing stays on the device."""
        from .segment_placement import INT_ARRAYS, LONG_ARRAYS, SCALARS

        window = int(window)
        min_hosts = window if min_hosts is None else int(min_hosts)
        f, l = self._placement_segments(first, last)
        n_seg = int(f.size)
        ints = np.zeros((len(INT_ARRAYS), n_seg), np.int32)
        longs = np.zeros((len(LONG_ARRAYS), n_seg), np.int64)
        quad = np.zeros((n_seg, 3, 4), np.int64)
        sc = np.zeros(len(SCALARS), np.int64)
        _ck(lib().ig_segment_placement(self._h, window, min_hosts, n_seg, _p(f), _p(l), _p(ints), _p(longs), _p(quad), _p(sc)))
        out = dict(window=window, min_hosts=min_hosts, n_seg=n_seg, first=f.astype(np.int64), last=l.astype(np.int64), quadrants=quad)
        out.update((k, ints[i].copy()) for i, k in enumerate(INT_ARRAYS))
        out.update((k, longs[i].copy()) for i, k in enumerate(LONG_ARRAYS))
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def debug_segment_placement_time(self, window, first, last, min_hosts=None, n=1):
        """the call n times with hipEvents around each pass -> (ms [n, 11]: ``SEGMENT_PLACEMENT_PASSES``, checksum of every output word
        of the last call)"""
        f, l = self._placement_segments(first, last)
        ms = np.zeros((int(n), len(SEGMENT_PLACEMENT_PASSES)), np.float32)
        ck = C.c_int64()
        _ck(lib().ig_debug_segment_placement_time(self._h, int(window), int(window) if min_hosts is None else int(min_hosts), int(f.size),
                                                  _p(f), _p(l), int(n), _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- segment edits: the moves the block-level reports propose, scored exactly and applied (the rule: rearrange.py)
    @staticmethod
    def _edits(edits):
        e = np.asarray(edits)
        if e.size and (e.ndim not in (1, 2) or e.shape[-1] != 5 or not np.issubdtype(e.dtype, np.integer)):
            raise HipError("segment edits: an integer array [n, 5] of (first_bin, last_bin, anchor, side, flip)")
        return np.ascontiguousarray(e, np.int32).reshape(-1, 5)

    def edit_score(self, edits, form=0):
        """the exact sums of the genome every edit would leave (``ig_edit_score``) -> (status int32 [n], limbs int64 [n, 5] in the order
        of ``full_likelihood``'s, nz f64 [n], z f64 [n]).  ``form``: 0 the delta form, 1 the whole form (the from-scratch passes on every
        edited genome); both give the same limbs.  Changes nothing a move reads."""
        e = self._edits(edits)
        n = int(e.shape[0])
        status, limbs = np.zeros(n, np.int32), np.zeros((n, 5), np.int64)
        nz, z = np.zeros(n, np.float64), np.zeros(n, np.float64)
        _ck(lib().ig_edit_score(self._h, n, _p(e), int(form), _p(status), _p(limbs), _p(nz), _p(z)))
        return status, limbs, nz, z

    def edit_state(self, edit):
        """tests: the state one edit would leave, with the internal contig ids -> (soa17 int32 [17, N], status); nothing is committed"""
        e = self._edits(edit)
        if e.shape[0] != 1:
            raise HipError("edit_state: one edit")
        out = np.zeros((17, self.N), np.int32)
        status = C.c_int32()
        _ck(lib().ig_edit_state(self._h, _p(e), _p(out), C.byref(status)))
        return out, int(status.value)

    def edit_apply(self, edit):
        """commits one edit (``ig_edit_apply``) -> (status, limbs int64 [5]: the maintained sums behind the call).  A status other
        than 0 leaves everything as it was."""
        e = self._edits(edit)
        if e.shape[0] != 1:
            raise HipError("edit_apply: one edit")
        limbs = np.zeros(5, np.int64)
        status = C.c_int32()
        _ck(lib().ig_edit_apply(self._h, _p(e), C.byref(status), _p(limbs)))
        return int(status.value), limbs

    def debug_edit_time(self, edits, form=0, n=1):
        """``edit_score`` n times with hipEvents around each pass -> (ms [n, 6]: ``EDIT_PASSES``, checksum of the statuses and limbs of
        the last call: the two forms agree on it)"""
        e = self._edits(edits)
        ms = np.zeros((int(n), len(EDIT_PASSES)), np.float32)
        ck = C.c_int64()
        _ck(lib().ig_debug_edit_time(self._h, int(e.shape[0]), _p(e), int(form), int(n), _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- cut and join scores: the closed part of the likelihood change of every cut and every link (the rule: cut_join.py)
    def cut_scores(self):
        """``ig_cut_scores`` -> dict: valid (bool [N]: a cut in front of the bin exists), contacts (int64 [N]), limbs (int64 [N, 5]: the
        delta limbs), delta (f64 [N]); zeros where no cut exists.  Changes nothing a move reads."""
        n = self.N
        valid, contacts = np.zeros(n, np.int32), np.zeros(n, np.int64)
        limbs, delta = np.zeros((n, 5), np.int64), np.zeros(n, np.float64)
        _ck(lib().ig_cut_scores(self._h, _p(valid), _p(contacts), _p(limbs), _p(delta)))
        return dict(valid=valid != 0, contacts=contacts, limbs=limbs, delta=delta)

    def join_scores(self):
        """``ig_join_scores_build`` / ``_fetch`` / ``_release`` -> dict: K, n_pairs; per linear contig (ascending internal id)
        head_bin, tail_bin, n_sub, length_bp (int32 [K]); CSR rowptr (int64 [K + 1]), col (int32, b > a ascending); per pair contacts
        (int64), nz (int64 [n_pairs, 4, 2], link 2 sa + sb, side 0 the head), z (int64 [n_pairs, 2]), dni (int64), delta (f64 [n_pairs, 4])"""
        nk, npair = C.c_int64(), C.c_int64()
        _ck(lib().ig_join_scores_build(self._h, C.byref(nk), C.byref(npair)))
        K, P = int(nk.value), int(npair.value)
        out = dict(K=K, n_pairs=P, rowptr=np.zeros(K + 1, np.int64), col=np.zeros(P, np.int32), contacts=np.zeros(P, np.int64),
                   nz=np.zeros((P, 4, 2), np.int64), z=np.zeros((P, 2), np.int64), dni=np.zeros(P, np.int64), delta=np.zeros((P, 4), np.float64))
        for k in CONTIG_ARRAYS:
            out[k] = np.zeros(K, np.int32)
        try:
            _ck(lib().ig_join_scores_fetch(self._h, *[_p(out[k]) for k in CONTIG_ARRAYS + ("rowptr", "col", "contacts", "nz", "z", "dni", "delta")]))
        finally:
            _ck(lib().ig_join_scores_release(self._h))
        return out

    def debug_contact_terms(self, s, d, trans, count):
        """tests: eval_q on the device for the inputs of ``contact_terms_host`` (``ig_debug_contact_terms``) -> int64 of the shape of ``s``"""
        sep = np.ascontiguousarray(s, np.float32)
        dd, tt, cc = (np.ascontiguousarray(np.broadcast_to(np.asarray(a), sep.shape), np.int32) for a in (d, trans, count))
        q = np.zeros(sep.shape, np.int64)
        _ck(lib().ig_debug_contact_terms(self._h, _p(sep), _p(dd), _p(tt), _p(cc), sep.size, _p(q)))
        return q

    def debug_cut_join_form(self, form=-1):
        """tests: the form of the join pass: -1 by the number of pairs, 0 accumulators in LDS, 1 atomics per run of a wave"""
        _ck(lib().ig_debug_cut_join_form(self._h, int(form)))

    def debug_join_scores_forms(self):
        """the LIFT_C_* words of the pairs' rows of the last finished ``join_scores`` build (the handle keeps them behind the release)"""
        out = np.zeros(8, np.int64)
        _ck(lib().ig_debug_join_scores_forms(self._h, _p(out)))
        return out

    def debug_cut_join_time(self, what="cuts", n=1):
        """``cut_scores`` (what = "cuts") or the build of ``join_scores`` ("joins") n times with hipEvents around each pass ->
        (ms [n, 12]: ``CUT_JOIN_PASSES``, checksum of the integer words of the last result: the forms agree on it)"""
        ms = np.zeros((int(n), len(CUT_JOIN_PASSES)), np.float32)
        ck = C.c_int64()
        _ck(lib().ig_debug_cut_join_time(self._h, ("cuts", "joins").index(what), int(n), _p(ms), C.byref(ck)))
        return ms, int(ck.value)

    # ---- balancing the contact map of the current genome (the rule: balance.py)
    def balance_build(self, level="bin", max_side=2048, ignore_diags=2):
        """builds the rows the balancing iterates over -- both entries (u, v), (v, u) of every kept contact, sorted, equal columns
        summed -- as a snapshot on the device -> dict: level, rowptr (int64 [n_units + 1]), nnz and total (int64 [n_units]) and the
        int64 scalars of ``balance.SCALARS``; the entries come through ``balance_fetch``"""
        from .balance import LEVELS, SCALARS

        lv = LEVELS.index(level) if level in LEVELS else int(level)
        nu, ne = C.c_int64(), C.c_int64()
        sc = np.zeros(8, np.int64)
        _ck(lib().ig_balance_build(self._h, lv, int(max_side), int(ignore_diags), C.byref(nu), C.byref(ne), _p(sc)))
        U = int(nu.value)
        rowptr, nnz, total = np.zeros(U + 1, np.int64), np.zeros(U, np.int64), np.zeros(U, np.int64)
        _ck(lib().ig_balance_rows(self._h, _p(rowptr), _p(nnz), _p(total), rowptr.size))
        out = dict(level=level, rowptr=rowptr, nnz=nnz, total=total)
        out.update((k, int(v)) for k, v in zip(SCALARS, sc))
        return out

    def balance_fetch(self, first, n):
        """entries first .. first + n - 1 of the built rows -> (col int32 [n], count int64 [n])"""
        n = int(n)
        col, cnt = np.zeros(max(n, 0), np.int32), np.zeros(max(n, 0), np.int64)
        _ck(lib().ig_balance_fetch(self._h, int(first), n, _p(col), _p(cnt)))
        return col, cnt

    def balance_run(self, b0, tol=1e-5, max_iters=200):
        """the iterations of the rule over the built rows from ``b0`` (f64 per unit, 0.0 where masked) -> dict: b, marg_final (f64
        per unit), variance (f64 [n_iters]), n_iters, converged"""
        b0 = np.ascontiguousarray(b0, np.float64)
        max_iters = int(max_iters)
        b, marg = np.zeros(b0.size, np.float64), np.zeros(b0.size, np.float64)
        var = np.zeros(max(max_iters, 1), np.float64)
        n, conv = C.c_int32(), C.c_int32()
        _ck(lib().ig_balance_run(self._h, _p(b0), float(tol), max_iters, _p(b), _p(marg), _p(var), C.byref(n), C.byref(conv)))
        return dict(b=b, marg_final=marg, variance=var[:n.value].copy(), n_iters=int(n.value), converged=bool(conv.value))

    def balance_release(self):
        _ck(lib().ig_balance_release(self._h))

    def debug_balance_form(self, form="default"):
        """the marginals kernel: ``"wave"`` (a wave per row, the yardstick), ``"packed"`` (four rows of at most 16 entries share a
        wave) or ``"default"`` (the form the library ships)"""
        _ck(lib().ig_debug_balance_form(self._h, BALANCE_FORMS.index(form)))

    def debug_balance_group(self, group=0):
        """the iterations ``balance_run`` enqueues between two looks at the device's done flag (0: the default)"""
        _ck(lib().ig_debug_balance_group(self._h, int(group)))

    def debug_lane_sums(self, values, rowptr):
        """the ordered sum (``balance.lane_sum``) of every row of caller data on the device, in the handle's form -> f64 [n_rows]"""
        values = np.ascontiguousarray(values, np.float64)
        rowptr = np.ascontiguousarray(rowptr, np.int64)
        if rowptr.size < 2 or rowptr[-1] != values.size:
            raise HipError("debug_lane_sums: rowptr has n_rows + 1 >= 2 words and ends at the number of values")
        out = np.zeros(rowptr.size - 1, np.float64)
        _ck(lib().ig_debug_lane_sums(self._h, _p(values), _p(rowptr), rowptr.size - 1, _p(out)))
        return out

    def debug_balance_time(self, what="marginals", n=1):
        """over the built rows, from b = 1: ``"marginals"`` (the kernel alone) or ``"iteration"`` n times, event-timed -> ms [n]"""
        ms = np.zeros(int(n), np.float32)
        _ck(lib().ig_debug_balance_time(self._h, ("marginals", "iteration").index(what), int(n), _p(ms)))
        return ms

    def debug_balance_build_time(self, level="bin", max_side=2048, ignore_diags=2, n=1):
        """the build n times with hipEvents around each pass -> ms [n, 8]: ``BALANCE_BUILD_PASSES``; the last build's rows stay"""
        from .balance import LEVELS

        ms = np.zeros((int(n), len(BALANCE_BUILD_PASSES)), np.float32)
        _ck(lib().ig_debug_balance_build_time(self._h, LEVELS.index(level), int(max_side), int(ignore_diags), int(n), _p(ms)))
        return ms

    # ---- the balancing's rows from a built map (the rule: balance.entries_of_rows)
    @staticmethod
    def _snapshot_mode(mode, group, who):
        from .balance import MODES

        if mode not in MODES:
            raise HipError("%s: mode is one of %r (got %r)" % (who, MODES, mode))
        g = None if group is None else as_int32_exact(group, who + ": group")
        return MODES.index(mode), g

    def _snapshot_rows(self, nu, ne, sc):
        from .balance import SNAPSHOT_SCALARS

        U = int(nu.value)
        rowptr, nnz, total = np.zeros(U + 1, np.int64), np.zeros(U, np.int64), np.zeros(U, np.int64)
        _ck(lib().ig_balance_rows(self._h, _p(rowptr), _p(nnz), _p(total), rowptr.size))
        out = dict(level="units", rowptr=rowptr, nnz=nnz, total=total, n_entries=int(ne.value))
        out.update((k, int(v)) for k, v in zip(SNAPSHOT_SCALARS, sc))
        return out

    def balance_build_snapshot(self, ignore_diags=2, mode="all", group=None):
        """the balancing's rows from the snapshot on the device (``assembly_contacts("bin")``, ``assembly_contacts_units``,
        ``assembly_contacts_coarsen`` or ``pairs_pixels`` left it there), which stays as it is.  ``mode`` "cis" / "trans" with ``group``
        (int per unit: its scaffold) keeps the entries inside / between groups.  -> dict: rowptr (int64 [n_units + 1]), nnz and
        total (int64 [n_units]), n_entries and the int64 scalars of ``balance.SNAPSHOT_SCALARS``; the entries come through
        ``balance_fetch``, the iterations through ``balance_run``"""
        m, g = self._snapshot_mode(mode, group, "balance_build_snapshot")
        nu, ne, sc = C.c_int64(), C.c_int64(), np.zeros(8, np.int64)
        _ck(lib().ig_balance_build_snapshot(self._h, int(ignore_diags), m, _p(g), 0 if g is None else g.size, C.byref(nu), C.byref(ne), _p(sc)))
        return self._snapshot_rows(nu, ne, sc)

    def debug_balance_snapshot(self, rowptr, col, count, ignore_diags=2, mode="all", group=None):
        """``balance_build_snapshot`` over caller CSR data (upper triangular) on a bare handle (tests/test_hip_balance_snapshot.py): the
        data becomes the handle's snapshot, which ``assembly_contacts_fetch`` and ``assembly_contacts_coarsen`` then see -> the same
        dict"""
        rowptr = np.ascontiguousarray(rowptr, np.int64)
        col, count = np.ascontiguousarray(col, np.int32), np.ascontiguousarray(count, np.int64)
        if rowptr.ndim != 1 or rowptr.size < 1 or col.shape != count.shape or col.ndim != 1 or col.size != int(rowptr[-1]):
            raise HipError("debug_balance_snapshot: rowptr [U + 1], col and count [rowptr[U]]")
        m, g = self._snapshot_mode(mode, group, "debug_balance_snapshot")
        nu, ne, sc = C.c_int64(), C.c_int64(), np.zeros(8, np.int64)
        _ck(lib().ig_debug_balance_snapshot(self._h, _p(rowptr), _p(col), _p(count), rowptr.size - 1, int(ignore_diags), m, _p(g),
                                            0 if g is None else g.size, C.byref(nu), C.byref(ne), _p(sc)))
        return self._snapshot_rows(nu, ne, sc)

    def debug_balance_snapshot_time(self, n=1):
        """the build from the resident snapshot n times with hipEvents around each pass -> ms [n, 7]: ``BALANCE_SNAPSHOT_PASSES``; the
        snapshot stays, and so do the last build's rows"""
        ms = np.zeros((int(n), len(BALANCE_SNAPSHOT_PASSES)), np.float32)
        _ck(lib().ig_debug_balance_snapshot_time(self._h, int(n), _p(ms)))
        return ms

    # ---- bookkeeping
    def renumber_contigs(self):
        n = C.c_int32()
        m = C.c_float()
        mx = C.c_int32()
        _ck(lib().ig_renumber_contigs(self._h, C.byref(n), C.byref(m), C.byref(mx)))
        return n.value, np.float32(m.value), mx.value

    def bomb(self, shuffle):
        s = np.ascontiguousarray(shuffle, np.int32)
        _ck(lib().ig_bomb(self._h, _p(s)))

    def genome_distance(self):
        d = C.c_double()
        _ck(lib().ig_genome_distance(self._h, C.byref(d)))
        return d.value

    def valid_insert(self):
        out = np.zeros(12, np.int32)
        _ck(lib().ig_get_valid_insert(self._h, _p(out)))
        return out

    def sync(self):
        _ck(lib().ig_sync(self._h))

    def set_stream(self, hip_stream_ptr):
        _ck(lib().ig_set_stream(self._h, hip_stream_ptr))

    # ---- timing
    def reset_timers(self, enable=True):
        _ck(lib().ig_reset_timers(self._h, int(enable)))

    def set_timer_sampling(self, every):
        _ck(lib().ig_set_timer_sampling(self._h, int(every)))

    def kernel_time_ms(self, name):
        avg = C.c_double()
        n = C.c_int64()
        _ck(lib().ig_kernel_time_ms(self._h, name.encode(), C.byref(avg), C.byref(n)))
        return avg.value, n.value

    # ---- multi-GPU two-phase move
    def set_shard(self, rank, world):
        _ck(lib().ig_set_shard(self._h, rank, world))

    def partials(self):
        return lib().ig_partials_device_ptr(self._h), lib().ig_partials_count(self._h)

    def step_begin(self, frag_a, cands):
        c = np.ascontiguousarray(cands, np.int32)
        _ck(lib().ig_step_begin(self._h, int(frag_a), _p(c), c.size))

    def step_finish(self, n_cands, want_scores=False):
        res = MoveResult()
        sc = np.zeros(n_cands * N_TMP_STRUCT, np.float64) if want_scores else None
        _ck(lib().ig_step_finish(self._h, C.byref(res), _p(sc)))
        return res, sc

    # ---- debug
    def debug_eval_terms(self, s, s_tot, ob):
        s = np.ascontiguousarray(s, np.float32)
        st = np.ascontiguousarray(s_tot, np.float32)
        ob = np.ascontiguousarray(ob, np.int32)
        n = s.size
        ex = np.zeros(n, np.float32)
        exc = np.zeros(n, np.float32)
        term = np.zeros(n, np.float64)
        q = np.zeros(n, np.int64)
        _ck(lib().ig_debug_eval_terms(self._h, _p(s), _p(st), _p(ob), n, _p(ex), _p(exc), _p(term), _p(q)))
        return ex, exc, term, q

    def debug_candidate_state(self, cand, slot):
        out = np.zeros((17, self.N), np.int32)
        _ck(lib().ig_debug_candidate_state(self._h, cand, slot, _p(out)))
        return out

    def debug_last_sums(self, n_cands):
        T = N_TMP_STRUCT
        a = {k: np.zeros(n_cands * T, np.int64) for k in ("nz_hi", "nz_lo", "z_hi", "z_lo", "n_intra")}
        ext_hi = np.zeros(n_cands, np.int64)
        ext_lo = np.zeros(n_cands, np.int64)
        n_slice = np.zeros(n_cands, np.int64)
        n_uniq = np.zeros(n_cands, np.int32)
        uniq = np.zeros(n_cands * T, np.int32)
        _ck(lib().ig_debug_last_sums(self._h, _p(a["nz_hi"]), _p(a["nz_lo"]), _p(a["z_hi"]), _p(a["z_lo"]), _p(a["n_intra"]),
                                     _p(ext_hi), _p(ext_lo), _p(n_slice), _p(n_uniq), _p(uniq)))
        a.update(ext_hi=ext_hi, ext_lo=ext_lo, n_slice=n_slice, n_uniq=n_uniq, uniq=uniq.reshape(n_cands, T))
        return a

    def debug_transcendental_error(self):
        o = np.zeros(2, np.float64)
        _ck(lib().ig_debug_transcendental_error(self._h, _p(o)))
        return float(o[0]), float(o[1])

    def debug_screen_stats(self):
        """(largest used fraction of a bound, largest bound) under IG_SCREEN_VERIFY=1; (columns screened, columns scored exactly,
        terms screened, terms scored exactly)"""
        o = np.zeros(6, np.float64)
        _ck(lib().ig_debug_screen_stats(self._h, _p(o)))
        return float(o[0]), float(o[1]), int(o[2]), int(o[3]), int(o[4]), int(o[5])

    def debug_globals(self):
        sums = np.zeros(5, np.int64)
        ints = np.zeros(6, np.int32)
        _ck(lib().ig_debug_globals(self._h, _p(sums), _p(ints)))
        return sums, ints

    def debug_dbg(self, clear=False):
        """Glob.dbg (what raised a device-side consistency failure; in a tuning build a kernel's tick counters)"""
        o = np.zeros(8, np.int32)
        _ck(lib().ig_debug_dbg(self._h, _p(o), int(bool(clear))))
        return o

    def debug_pz_table(self, which=0):
        """the P_z table set_params built for parameter set ``which``: pz[d] for every rank distance d below its length"""
        out = np.zeros(4096, np.float32)
        n = C.c_int32()
        _ck(lib().ig_debug_pz_table(self._h, int(which), _p(out), out.size, C.byref(n)))
        assert 0 <= n.value <= out.size, n.value
        return out[: n.value].copy()

    def debug_tables(self):
        M = self.M
        d = np.zeros(M, np.float32)
        c = np.zeros(M, np.int32)
        st = np.zeros(M, np.float32)
        p = np.zeros(M, np.int32)
        ln = np.zeros(M, np.int32)
        _ck(lib().ig_debug_tables(self._h, _p(d), _p(c), _p(st), _p(p), _p(ln)))
        return d, c, st, p, ln
