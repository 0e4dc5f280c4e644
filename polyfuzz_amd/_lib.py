"""ctypes binding of libpolyfuzz_hip.so (the C ABI of include/polyfuzz_hip.h).

No torch, no fallback: if the library is missing or no gfx950 device is visible
the calls raise -- the host layer never computes similarities itself.
"""
import ctypes
import os
import threading

import numpy as np

from . import _build

c_i32, c_i64, c_f32, c_f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double
c_vp = ctypes.c_void_p
P = ctypes.POINTER


class PfzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libpolyfuzz_hip error {code}: {msg}")
        self.code = code


class PfzUnsupported(PfzError, NotImplementedError):
    pass


class PfzNoDevice(PfzError):
    pass


class TfidfParams(ctypes.Structure):
    _fields_ = [("ngram_lo", c_i32), ("ngram_hi", c_i32), ("clean", c_i32), ("remove_space_ngrams", c_i32)]


# every symbol include/polyfuzz_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "pfz_version": (ctypes.c_int, []),
    "pfz_last_error": (ctypes.c_char_p, []),
    "pfz_device_count": (ctypes.c_int, []),
    "pfz_ctx_create": (ctypes.c_int, [ctypes.c_int, P(c_vp)]),
    "pfz_ctx_destroy": (None, [c_vp]),
    "pfz_ctx_sync": (ctypes.c_int, [c_vp]),
    "pfz_ctx_info": (ctypes.c_int, [c_vp, ctypes.c_char_p, P(c_i32), P(c_i64)]),
    "pfz_pool_stats": (ctypes.c_int, [c_vp, P(c_i64), P(c_i64)]),
    "pfz_pool_fill": (ctypes.c_int, [c_vp, c_i32]),
    "pfz_event_record": (ctypes.c_int, [c_vp, c_i32]),
    "pfz_event_elapsed_ms": (ctypes.c_int, [c_vp, c_i32, c_i32, P(c_f32)]),
    "pfz_prof_enable": (ctypes.c_int, [c_vp, c_i32]),
    "pfz_prof_reset": (ctypes.c_int, [c_vp]),
    "pfz_prof_get": (ctypes.c_int, [c_vp, ctypes.c_char_p, P(c_f64), P(c_i64)]),
    "pfz_csr_upload": (ctypes.c_int, [c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, P(c_vp)]),
    "pfz_csr_shape": (ctypes.c_int, [c_vp, P(c_i64), P(c_i64), P(c_i64)]),
    "pfz_csr_download": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pfz_csr_free": (None, [c_vp]),
    "pfz_index_build": (ctypes.c_int, [c_vp, c_vp, P(c_vp)]),
    "pfz_index_free": (None, [c_vp]),
    "pfz_index_info": (ctypes.c_int, [c_vp, P(c_i64), P(c_i64), P(c_i64), P(c_i64), P(c_i64), P(c_i64)]),
    "pfz_index_pieces": (ctypes.c_int, [c_vp, P(c_i64), P(c_i64)]),
    "pfz_index_symmetric_launches": (ctypes.c_int, [c_vp, P(c_i64), P(c_i64)]),
    "pfz_index_symmetric_census": (ctypes.c_int, [c_vp, P(c_i64), P(c_i64)]),
    "pfz_index_symmetric_ok": (ctypes.c_int, [c_vp, c_vp, c_i32, c_i32, P(c_i32)]),
    "pfz_comm_cossim_topn_symmetric": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, ctypes.c_float, c_vp]),
    "pfz_comm_symmetric_ok": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, P(c_i32)]),
    "pfz_rccl_versions": (ctypes.c_int, [P(c_i32), P(c_i32)]),
    "pfz_topn_alloc": (ctypes.c_int, [c_vp, c_i64, c_i32, P(c_vp)]),
    "pfz_topn_free": (None, [c_vp]),
    "pfz_topn_download": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "pfz_topn_clear": (ctypes.c_int, [c_vp, c_vp]),
    "pfz_topn_download_rows_after": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_i32, c_vp, c_vp]),
    "pfz_topn_rows_begin": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_i32, c_i32]),
    "pfz_topn_rows_finish": (ctypes.c_int, [c_vp, c_i32, P(c_vp), P(c_vp)]),
    "pfz_cossim_topn_ranges": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, ctypes.c_float, c_i32, c_i32, P(c_i64), c_i32, c_vp, P(c_vp), P(c_vp)]),
    "pfz_event_wait": (ctypes.c_int, [c_vp, c_i32]),
    "pfz_stage_reserve": (ctypes.c_int, [c_vp, c_i64, P(c_vp)]),
    "pfz_topn_upload": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "pfz_topn_device_ptrs": (ctypes.c_int, [c_vp, P(c_vp), P(c_vp), P(c_i64), P(c_i32)]),
    "pfz_cossim_topn": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_f32, c_i32, c_i64, c_vp]),
    "pfz_cossim_topn_rows": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i32, c_f32, c_i32, c_i64, c_vp]),
    "pfz_cossim_topn_host": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                            c_i32, c_f32, c_i32, c_vp, c_vp]),
    "pfz_strings_upload": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, P(c_vp)]),
    "pfz_strings_free": (None, [c_vp]),
    "pfz_tfidf_fit": (ctypes.c_int, [c_vp, P(TfidfParams), c_vp, c_vp, P(c_vp)]),
    "pfz_tfidf_free": (None, [c_vp]),
    "pfz_tfidf_info": (ctypes.c_int, [c_vp, P(c_i64), P(c_i64), P(c_i32)]),
    "pfz_tfidf_export": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pfz_tfidf_import": (ctypes.c_int, [c_vp, P(TfidfParams), c_i64, c_i64, c_vp, c_vp, P(c_vp)]),
    "pfz_tfidf_transform": (ctypes.c_int, [c_vp, c_vp, c_vp, P(c_vp)]),
    "pfz_indel_argmax": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp]),
    "pfz_indel_matrix_host": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp]),
    "pfz_indel_plan_info": (ctypes.c_int, [c_vp, c_vp, P(c_i64), P(c_i64), P(c_i64)]),
    "pfz_indel_argmax_dev": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_vp]),
    "pfz_indel_topn": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i32, c_vp, c_vp]),
    "pfz_jaro_argmax": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_vp, c_vp]),
    "pfz_jaro_argmax_dev": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_vp]),
    "pfz_jaro_matrix_host": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_i64, c_i64, c_vp]),
    "pfz_jaro_join": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_f64, c_i64, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_jaro_components": (ctypes.c_int, [c_vp, c_vp, c_i32, c_f64, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_jaro_topn": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_i32, c_f64, c_vp, c_vp, c_vp]),
    "pfz_lev_argmax": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_vp, c_vp]),
    "pfz_lev_argmax_dev": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_vp]),
    "pfz_lev_topn": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_i32, c_vp, c_vp]),
    "pfz_lev_matrix_host": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_i64, c_i64, c_vp]),
    "pfz_lev_join": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_f64, c_i64, c_vp, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_lev_components": (ctypes.c_int, [c_vp, c_vp, c_i32, c_f64, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_indel_join": (ctypes.c_int, [c_vp, c_vp, c_vp, c_f64, c_i64, c_vp, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_indel_components": (ctypes.c_int, [c_vp, c_vp, c_f64, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_pairs_rescore_topn": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "pfz_pairs_join": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i32, c_f64, c_i64, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_pairs_components": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_f64, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_cossim_join_dev": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_f64, c_i64, P(c_vp), c_vp]),
    "pfz_pairs_free": (None, [c_vp]),
    "pfz_pairs_count": (ctypes.c_int, [c_vp, P(c_i64)]),
    "pfz_pairs_shape": (ctypes.c_int, [c_vp, P(c_i64), P(c_i64), P(c_i32)]),
    "pfz_pairs_download": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pfz_pairs_join_keys": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i32, c_f64, c_i64, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_pairs_components_keys": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_f64, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_fuzz_extract_one": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_vp, c_vp]),
    "pfz_fuzz_extract_one_dev": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_vp, c_vp]),
    "pfz_fuzz_plan_info": (ctypes.c_int, [c_vp, c_vp, P(c_i64), P(c_i64), P(c_i64), P(c_i64)]),
    "pfz_fuzz_join": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_f64, c_i64, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_fuzz_components": (ctypes.c_int, [c_vp, c_vp, c_i32, c_f64, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_fuzz_topn": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i64, c_i32, c_f64, c_vp, c_vp, c_vp]),
    "pfz_dense_cossim_topn_host": (ctypes.c_int, [c_vp, c_vp, c_i64, c_vp, c_i64, c_i64, c_i32, c_f32, c_i32,
                                                  c_vp, c_vp]),
    "pfz_dense_dot_topn_host": (ctypes.c_int, [c_vp, c_vp, c_i64, c_vp, c_i64, c_i64, c_i32, c_f32, c_i32,
                                               c_vp, c_vp]),
    "pfz_dense_upload": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_i32, P(c_vp)]),
    "pfz_dense_upload16": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_i32, c_i32, c_i32, P(c_vp)]),
    "pfz_dense_upload8": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_i32, c_i32, P(c_vp)]),
    "pfz_dense_upload1": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_i32, c_i32, P(c_vp)]),
    "pfz_dense_dtype": (ctypes.c_int, [c_vp, P(c_i32)]),
    "pfz_dense_shape": (ctypes.c_int, [c_vp, P(c_i64), P(c_i64)]),
    "pfz_dense_free": (None, [c_vp]),
    "pfz_dense_topn": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_f32, c_i32, c_i64, c_vp]),
    "pfz_dense_rescore_topn": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i32, c_f32, c_vp]),
    "pfz_dense_rescore_topn_mixed": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i32, c_f32, c_vp]),
    "pfz_dense_join": (ctypes.c_int, [c_vp, c_vp, c_vp, c_f64, c_i64, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_dense_components": (ctypes.c_int, [c_vp, c_vp, c_f64, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_dense_derive16": (ctypes.c_int, [c_vp, c_vp, c_i32, P(c_vp)]),
    "pfz_dense_search_margin": (ctypes.c_int, [c_i32, c_i64, P(c_f64)]),
    "pfz_hamming_join": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_hamming_components": (ctypes.c_int, [c_vp, c_vp, c_i64, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_hamming_max_distance": (ctypes.c_int, [c_i64, c_f64, P(c_i64)]),
    "pfz_hamming_join_indexed": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i64, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_hamming_components_indexed": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i32, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_hamming_index_plan": (ctypes.c_int, [c_i64, c_i64, c_vp]),
    "pfz_simhash": (ctypes.c_int, [c_vp, c_vp, P(TfidfParams), c_i32, P(c_vp), c_vp, c_vp, c_vp]),
    "pfz_dense_join16": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_f64, c_i64, c_i64, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_dense_components16": (ctypes.c_int, [c_vp, c_vp, c_vp, c_f64, c_i64, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_cossim_join": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_f64, c_i64, c_vp, c_vp, c_vp, P(c_i64), c_vp]),
    "pfz_cossim_components": (ctypes.c_int, [c_vp, c_vp, c_vp, c_f64, c_vp, P(c_i64), P(c_i64), c_vp]),
    "pfz_pr_curve_host": (ctypes.c_int, [c_vp, c_vp, c_i64, c_vp, c_i32, c_vp, c_vp]),
    "pfz_linkage_top1": (ctypes.c_int, [c_vp, c_vp, c_f64, c_vp, c_vp, c_vp]),
    "pfz_comm_unique_id": (ctypes.c_int, [c_vp]),
    "pfz_comm_init": (ctypes.c_int, [c_vp, c_vp, c_i32, c_i32, P(c_vp)]),
    "pfz_comm_destroy": (None, [c_vp]),
    "pfz_comm_group_create": (ctypes.c_int, [c_i32, P(c_vp)]),
    "pfz_comm_group_destroy": (None, [c_vp]),
    "pfz_comm_init_local": (ctypes.c_int, [c_vp, c_vp, c_i32, P(c_vp)]),
    "pfz_comm_allgather_topn": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "pfz_comm_merge_to_shards": (ctypes.c_int, [c_vp, c_vp, c_i64, c_vp]),
    "pfz_comm_barrier": (ctypes.c_int, [c_vp]),
    "pfz_comm_info": (ctypes.c_int, [c_vp, P(c_i32), P(c_i32)]),
    "pfz_tfidf_fit_sharded": (ctypes.c_int, [c_vp, c_vp, P(TfidfParams), c_vp, c_vp, P(c_vp)]),
}

_lib = None
_lock = threading.Lock()


def lib_path():
    # POLYFUZZ_HIP_LIB: another build of the same sources (tuning experiments: tools/build_variant.sh)
    return os.environ.get("POLYFUZZ_HIP_LIB") or _build.LIB_PATH


def load():
    """Load libpolyfuzz_hip.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc, gfx950).  polyfuzz_amd has no CPU fallback.")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(rc):
    if rc == 0:
        return
    msg = load().pfz_last_error().decode("utf-8", "replace")
    if rc == -4:
        raise PfzUnsupported(rc, msg)
    if rc == -2:
        raise PfzNoDevice(rc, msg)
    raise PfzError(rc, msg)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_vp)


def device_count():
    return int(load().pfz_device_count())


class Context:
    """One HIP device + stream.  `Context.default()` is a per-process singleton on
    device POLYFUZZ_HIP_DEVICE (or LOCAL_RANK, or 0)."""
    _default = None

    def __init__(self, device=None):
        if device is None:
            device = int(os.environ.get("POLYFUZZ_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        self.lib = load()
        h = c_vp()
        check(self.lib.pfz_ctx_create(int(device), ctypes.byref(h)))
        self.h = h
        self.device = int(device)

    @classmethod
    def default(cls):
        if cls._default is None:
            cls._default = cls()
        return cls._default

    def close(self):
        if getattr(self, "h", None):
            self.lib.pfz_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.lib.pfz_ctx_sync(self.h))

    def info(self):
        name = ctypes.create_string_buffer(256)
        ncu, mem = c_i32(), c_i64()
        check(self.lib.pfz_ctx_info(self.h, name, ctypes.byref(ncu), ctypes.byref(mem)))
        return {"name": name.value.decode(), "n_cu": ncu.value, "hbm_bytes": mem.value}

    def pool_stats(self):
        """(live_bytes, cached_bytes) of the context's caching device allocator"""
        live, cached = c_i64(), c_i64()
        check(self.lib.pfz_pool_stats(self.h, ctypes.byref(live), ctypes.byref(cached)))
        return live.value, cached.value

    # pfz_pool_fill's modes and the 64-bit little-endian word each writes over every block the allocator hands out
    POOL_FILL_OFF, POOL_FILL_ZERO, POOL_FILL_ONE64, POOL_FILL_ONE32 = 0, 1, 2, 3
    POOL_FILL_WORDS = {POOL_FILL_ZERO: 0x0000000000000000, POOL_FILL_ONE64: 0x0000000000000001,
                       POOL_FILL_ONE32: 0x0000000100000001}

    def pool_fill(self, mode):
        """diagnostic: fill every device block handed out from now on with the mode's word (0: off, the allocator does not clear).
        A result that differs between two modes read memory nobody wrote (pfz_pool_fill; float accumulators are its blind spot)"""
        check(self.lib.pfz_pool_fill(self.h, int(mode)))

    # timers ---------------------------------------------------------------
    def event_record(self, slot):
        check(self.lib.pfz_event_record(self.h, slot))

    def event_wait(self, slot):
        """block until event slot `slot` has fired (pfz_event_wait)"""
        check(self.lib.pfz_event_wait(self.h, slot))

    def event_wait_fn(self):
        """(address of pfz_event_wait, the context's handle as an integer): what a native consumer needs to wait for event slots
        itself, without Python in between (_pack.fill_ranges)"""
        return ctypes.cast(self.lib.pfz_event_wait, ctypes.c_void_p).value, self.h.value if hasattr(self.h, "value") else int(self.h)

    def event_elapsed_ms(self, a, b):
        ms = c_f32()
        check(self.lib.pfz_event_elapsed_ms(self.h, a, b, ctypes.byref(ms)))
        return float(ms.value)

    def prof_enable(self, on=True):
        """on: False / True (every profiled kernel) / 2 (the dominant kernels only: least overhead)"""
        check(self.lib.pfz_prof_enable(self.h, int(on)))

    def prof_reset(self):
        check(self.lib.pfz_prof_reset(self.h))

    def prof_get(self, name):
        ms, n = c_f64(), c_i64()
        check(self.lib.pfz_prof_get(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)


class _Handle:
    _free = None

    def __init__(self, ctx, h):
        self.ctx = ctx
        self.h = h

    def free(self):
        if getattr(self, "h", None) and self.ctx.h:
            getattr(self.ctx.lib, self._free)(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceCSR(_Handle):
    _free = "pfz_csr_free"

    @classmethod
    def upload(cls, ctx, indptr, indices, data, n_cols):
        indptr = np.ascontiguousarray(indptr, np.int64)
        indices = np.ascontiguousarray(indices, np.int32)
        data = np.ascontiguousarray(data, np.float32)
        h = c_vp()
        check(ctx.lib.pfz_csr_upload(ctx.h, len(indptr) - 1, int(n_cols), _ptr(indptr), _ptr(indices), _ptr(data),
                                     ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_scipy(cls, ctx, m):
        m = m.tocsr()
        if not m.has_sorted_indices:
            m = m.sorted_indices()
        return cls.upload(ctx, m.indptr, m.indices, m.data, m.shape[1])

    @property
    def shape(self):
        r, c, z = c_i64(), c_i64(), c_i64()
        check(self.ctx.lib.pfz_csr_shape(self.h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(z)))
        return r.value, c.value, z.value

    @property
    def n_rows(self):
        """rows alone: known when the matrix is enqueued -- `shape` also asks for the count of non-zeros, which waits for the
        kernels that produce it (a transform's count travels to the host behind its last kernel)"""
        r = c_i64()
        check(self.ctx.lib.pfz_csr_shape(self.h, ctypes.byref(r), None, None))
        return r.value

    def download(self):
        n_rows, n_cols, nnz = self.shape
        indptr = np.empty(n_rows + 1, np.int64)
        indices = np.empty(nnz, np.int32)
        data = np.empty(nnz, np.float32)
        check(self.ctx.lib.pfz_csr_download(self.ctx.h, self.h, _ptr(indptr), _ptr(indices), _ptr(data)))
        return indptr, indices, data, n_cols


class DeviceIndex(_Handle):
    _free = "pfz_index_free"

    @classmethod
    def build(cls, ctx, to_csr):
        h = c_vp()
        check(ctx.lib.pfz_index_build(ctx.h, to_csr.h, ctypes.byref(h)))
        return cls(ctx, h)

    def info(self):
        v = [c_i64() for _ in range(6)]
        check(self.ctx.lib.pfz_index_info(self.h, *[ctypes.byref(x) for x in v]))
        keys = ("n_rows", "n_cols", "nnz", "block_cols", "n_blocks", "table_bytes")
        out = dict(zip(keys, (x.value for x in v)))
        npc, per = c_i64(), c_i64()
        check(self.ctx.lib.pfz_index_pieces(self.h, ctypes.byref(npc), ctypes.byref(per)))
        out.update(n_pieces=npc.value, piece_postings=per.value)
        return out

    def symmetric_launches(self):
        """(launches, from-rows) of this index that K3 served in its symmetric self-match form (k3_symmetric.hip)"""
        a, b = c_i64(), c_i64()
        check(self.ctx.lib.pfz_index_symmetric_launches(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def symmetric_ok(self, csr, ntop, n_parts=1):
        """may a self-match of `csr` (the matrix this index was built from) run in K3's symmetric form, cut over n_parts GPUs?"""
        yes = c_i32()
        check(self.ctx.lib.pfz_index_symmetric_ok(self.h, csr.h, int(ntop), int(n_parts), ctypes.byref(yes)))
        return bool(yes.value)

    def symmetric_census(self):
        """(magnet rows, rows recomputed row-major) of the last symmetric launch on this index (k3_symmetric.hip)"""
        a, b = c_i64(), c_i64()
        check(self.ctx.lib.pfz_index_symmetric_census(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


class DeviceTopN(_Handle):
    _free = "pfz_topn_free"

    @classmethod
    def alloc(cls, ctx, n_rows, ntop):
        h = c_vp()
        check(ctx.lib.pfz_topn_alloc(ctx.h, int(n_rows), int(ntop), ctypes.byref(h)))
        t = cls(ctx, h)
        t.n_rows, t.ntop = int(n_rows), int(ntop)
        return t

    def download(self):
        idx = np.empty((self.n_rows, self.ntop), np.int32)
        val = np.empty((self.n_rows, self.ntop), np.float32)
        check(self.ctx.lib.pfz_topn_download(self.ctx.h, self.h, _ptr(idx), _ptr(val)))
        return idx, val

    def clear(self):
        check(self.ctx.lib.pfz_topn_clear(self.ctx.h, self.h))

    def download_rows_after(self, begin, end, event_slot):
        """Rows [begin, end) as soon as the context's event `event_slot` has fired (side stream; later work keeps running)."""
        idx = np.empty((end - begin, self.ntop), np.int32)
        val = np.empty((end - begin, self.ntop), np.float32)
        check(self.ctx.lib.pfz_topn_download_rows_after(self.ctx.h, self.h, int(begin), int(end), int(event_slot), _ptr(idx),
                                                        _ptr(val)))
        return idx, val

    def rows_begin(self, begin, end, event_slot, half):
        """enqueue the download of rows [begin, end) behind the context's event `event_slot` into pinned staging half 0 / 1"""
        check(self.ctx.lib.pfz_topn_rows_begin(self.ctx.h, self.h, int(begin), int(end), int(event_slot), int(half)))

    def rows_finish(self, half):
        """wait for the download begun on `half`: (address of int32 idx[rows][ntop], address of fp32 val[rows][ntop]) in PINNED
        memory of the context, valid until the next rows_begin on that half"""
        a, b = c_vp(), c_vp()
        check(self.ctx.lib.pfz_topn_rows_finish(self.ctx.h, int(half), ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    @classmethod
    def from_host(cls, ctx, idx, val):
        idx = np.ascontiguousarray(idx, np.int32)
        val = np.ascontiguousarray(val, np.float32)
        if idx.ndim == 1:
            idx, val = idx[:, None], val[:, None]
        t = cls.alloc(ctx, idx.shape[0], idx.shape[1])
        check(ctx.lib.pfz_topn_upload(ctx.h, t.h, _ptr(idx), _ptr(val)))
        return t

    def upload(self, idx, val):
        """overwrite the whole buffer with host arrays of its shape"""
        idx = np.ascontiguousarray(idx, np.int32).reshape(self.n_rows, self.ntop)
        val = np.ascontiguousarray(val, np.float32).reshape(self.n_rows, self.ntop)
        check(self.ctx.lib.pfz_topn_upload(self.ctx.h, self.h, _ptr(idx), _ptr(val)))

    def device_ptrs(self):
        pi, pv = c_vp(), c_vp()
        check(self.ctx.lib.pfz_topn_device_ptrs(self.h, ctypes.byref(pi), ctypes.byref(pv), None, None))
        return pi.value, pv.value


def cossim_topn(ctx, index, from_csr, ntop, lower_bound, exclude_diag=False, diag_offset=0, out=None, rows=None):
    """Enqueue K3 (for from-rows `rows` = (begin, end) only, if given); returns the (device-resident) DeviceTopN."""
    if out is None:
        out = DeviceTopN.alloc(ctx, from_csr.n_rows, ntop)      # (not .shape: that would wait for the transform)
    if rows is None:
        check(ctx.lib.pfz_cossim_topn(ctx.h, index.h, from_csr.h, int(ntop), float(lower_bound),
                                      int(bool(exclude_diag)), int(diag_offset), out.h))
    else:
        check(ctx.lib.pfz_cossim_topn_rows(ctx.h, index.h, from_csr.h, int(rows[0]), int(rows[1]), int(ntop),
                                           float(lower_bound), int(bool(exclude_diag)), int(diag_offset), out.h))
    return out


def cossim_topn_ranges(ctx, index, from_csr, ntop, lower_bound, exclude_diag, range_ends, first_event, out=None, mirror=False):
    """Enqueue the whole match with its results handed on in ascending row ranges (pfz_cossim_topn_ranges): range i ends at
    range_ends[i], the context's event first_event + i fires when its rows are final.  Returns the DeviceTopN -- with mirror=True:
    (DeviceTopN, idx address, val address), the addresses of int32 idx[n][ntop] / fp32 val[n][ntop] in pinned HOST memory that
    the device fills beside the result (rows of range i valid after ctx.event_wait(first_event + i)), or (DeviceTopN, None,
    None) where the job does not run in the form that writes one."""
    if out is None:
        out = DeviceTopN.alloc(ctx, from_csr.n_rows, ntop)
    ends = (c_i64 * len(range_ends))(*[int(e) for e in range_ends])
    hi, hv = c_vp(), c_vp()
    check(ctx.lib.pfz_cossim_topn_ranges(ctx.h, index.h, from_csr.h, int(ntop), float(lower_bound), int(bool(exclude_diag)),
                                         len(range_ends), ends, int(first_event), out.h,
                                         ctypes.byref(hi) if mirror else None, ctypes.byref(hv) if mirror else None))
    return (out, hi.value, hv.value) if mirror else out


def cossim_topn_host(ctx, from_csr3, to_csr3, n_cols, ntop, lower_bound, exclude_diag=False):
    """One-shot: (indptr, indices, data) host triples in, (idx, val) host arrays out."""
    fp, fi, fv = from_csr3
    tp, ti, tv = to_csr3
    fp = np.ascontiguousarray(fp, np.int64)
    fi = np.ascontiguousarray(fi, np.int32)
    fv = np.ascontiguousarray(fv, np.float32)
    tp = np.ascontiguousarray(tp, np.int64)
    ti = np.ascontiguousarray(ti, np.int32)
    tv = np.ascontiguousarray(tv, np.float32)
    n_from, n_to = len(fp) - 1, len(tp) - 1
    idx = np.empty((n_from, ntop), np.int32)
    val = np.empty((n_from, ntop), np.float32)
    check(ctx.lib.pfz_cossim_topn_host(ctx.h, n_from, n_to, int(n_cols), _ptr(fp), _ptr(fi), _ptr(fv),
                                       _ptr(tp), _ptr(ti), _ptr(tv), int(ntop), float(lower_bound),
                                       int(bool(exclude_diag)), _ptr(idx), _ptr(val)))
    return idx, val


# ---- strings / vectoriser -------------------------------------------------------

try:  # CPython helper built by _build.build_host_helpers(); same result as the Python code below
    from . import _pack
except ImportError:  # pragma: no cover - not built
    _pack = None


def usable_cpus():
    """CPUs this process may really use: its affinity mask, capped by the cgroup's CPU quota where there is one (the MI355X boxes
    show 256 CPUs and grant 16 CPUs' worth of time)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, int(quota) // int(period))
    except (OSError, ValueError):
        pass
    return max(1, n)


def host_threads():
    """Host threads of the two big host-side walks of a match -- the string packer (pack_into / pack) and the frame's gathers
    (_pack.fill_ranges) -- the calling thread included.  PFZ_HOST_THREADS overrides (1 = everything on the calling thread); by
    default eight -- a CCD of the MI355X host -- where the process may use twice that many CPUs, half its CPUs below that.  The helpers run on the cores that share the calling
    thread's L3 and nowhere else (_pack.c: the crew; PFZ_HOST_PIN=0 lets the scheduler place them -- measured 4 x slower on the
    two-socket MI355X host); a host that does not tell its cache topology gets none.
    Measured there (tools/r6_match_ab.py, one box): TFIDF(top_n=5).match(100 000 names) 3.31 ms on the calling thread alone,
    3.20 / 3.02 / 2.82 / 2.79 with crews of 2 / 4 / 6 / 8."""
    env = os.environ.get("PFZ_HOST_THREADS")
    return max(1, min(16, int(env))) if env else max(1, min(8, usable_cpus() // 2))


_PACK_THREADS = _PACK_INTO_THREADS = host_threads()       # (the general packer's walks / pack_into's: separate names for the A/B tools)


def pack_strings(strings, objects=None):
    """list[str] -> (code units ndarray, offsets int64[n+1], char_width).

    1-byte code units (Latin-1) when every code point is <= 0xFF, UTF-32 otherwise.
    objects: a fresh np.empty(len(strings), object) array that is to become the From column of the result frame -- filled
    in the same walk over the strings (slot i = strings[i])."""
    if _pack is not None and isinstance(strings, (list, tuple)):
        if objects is not None:
            raw, off, width = _pack.pack(strings, _PACK_THREADS, objects.ctypes.data)
        else:
            raw, off, width = _pack.pack(strings, _PACK_THREADS)
        return np.frombuffer(raw, np.uint8 if width == 1 else np.uint32), np.frombuffer(off, np.int64), width
    if objects is not None:
        objects[:] = strings
    return _pack_strings_py(strings)


def _pack_strings_py(strings):
    n = len(strings)
    lens = np.fromiter(map(len, strings), np.int64, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    joined = "".join(strings)
    try:
        raw = joined.encode("latin-1")
        chars = np.frombuffer(raw, np.uint8)
        width = 1
    except UnicodeEncodeError:
        raw = joined.encode("utf-32-le", "surrogatepass")
        chars = np.frombuffer(raw, np.uint32)
        width = 4
    if len(chars) != off[-1]:
        raise ValueError("string packing length mismatch")
    return chars, off, width


class DeviceStrings(_Handle):
    _free = "pfz_strings_free"

    @classmethod
    def upload(cls, ctx, strings):
        if len(strings) >= 1024:          # (1-byte strings: packed straight into the pinned staging buffer)
            direct = cls.upload_direct(ctx, strings)
            if direct is not None:
                return direct
        return cls.upload_packed(ctx, *pack_strings(strings))

    @classmethod
    def upload_direct(cls, ctx, strings, objects=None):
        """A list of 1-byte (Latin-1) str packed STRAIGHT into the context's pinned staging buffer and uploaded from there (no
        bytes object, no copy into the staging buffer: 3 MB of host copies less in front of the device's first kernel for 100 000
        names).  objects: see pack_strings.  Returns None -- nothing changed -- when the list is not of that kind (wide or
        non-str items, too big for the staging buffer, no C helper): the caller takes pack_strings + upload_packed."""
        if _pack is None or not hasattr(_pack, "pack_into") or not isinstance(strings, (list, tuple)):
            return None
        n = len(strings)
        off_bytes = (8 * (n + 1) + 255) & ~255
        cap = off_bytes + 48 * n + 65536
        host = c_vp()
        check(ctx.lib.pfz_stage_reserve(ctx.h, cap, ctypes.byref(host)))
        if not host.value:
            return None
        n_chars = _pack.pack_into(strings, objects.ctypes.data if objects is not None else 0, host.value, off_bytes, cap, _PACK_INTO_THREADS)
        if n_chars is None:
            return None
        h = c_vp()
        check(ctx.lib.pfz_strings_upload(ctx.h, c_vp(host.value + off_bytes), c_vp(host.value), n, 1, ctypes.byref(h)))
        s = cls(ctx, h)
        s.n = n
        s.char_width = 1
        return s

    @classmethod
    def upload_packed(cls, ctx, chars, off, width):
        """Upload the result of pack_strings()."""
        n = len(off) - 1
        h = c_vp()
        check(ctx.lib.pfz_strings_upload(ctx.h, _ptr(chars) if len(chars) else None, _ptr(off), n, width,
                                         ctypes.byref(h)))
        s = cls(ctx, h)
        s.n = n
        s.char_width = width
        return s


class DeviceTfidf(_Handle):
    _free = "pfz_tfidf_free"

    @classmethod
    def fit(cls, ctx, params, docs_a, docs_b=None):
        h = c_vp()
        rc = ctx.lib.pfz_tfidf_fit(ctx.h, ctypes.byref(params), docs_a.h if docs_a is not None else None,
                                   docs_b.h if docs_b is not None else None, ctypes.byref(h))
        if rc == -1 and b"empty vocabulary" in ctx.lib.pfz_last_error():
            raise ValueError("empty vocabulary; perhaps the documents only contain stop words")
        check(rc)
        v = cls(ctx, h)
        v.params = params
        return v

    @classmethod
    def from_state(cls, ctx, params, ngrams, idf, n_docs):
        ngrams = np.ascontiguousarray(ngrams, np.uint32)
        idf = np.ascontiguousarray(idf, np.float64)
        h = c_vp()
        check(ctx.lib.pfz_tfidf_import(ctx.h, ctypes.byref(params), len(idf), int(n_docs), _ptr(ngrams), _ptr(idf),
                                       ctypes.byref(h)))
        v = cls(ctx, h)
        v.params = params
        return v

    def info(self):
        vs, nd, cb = c_i64(), c_i64(), c_i32()
        check(self.ctx.lib.pfz_tfidf_info(self.h, ctypes.byref(vs), ctypes.byref(nd), ctypes.byref(cb)))
        return {"vocab": vs.value, "n_docs": nd.value, "code_bits": cb.value}

    def export(self):
        """-> (ngrams uint32[vocab, ngram_hi], idf float64[vocab], df int64[vocab])"""
        i = self.info()
        hi = self.params.ngram_hi
        ngrams = np.empty((i["vocab"], hi), np.uint32)
        idf = np.empty(i["vocab"], np.float64)
        df = np.empty(i["vocab"], np.int64)
        check(self.ctx.lib.pfz_tfidf_export(self.ctx.h, self.h, _ptr(ngrams), _ptr(idf), _ptr(df)))
        return ngrams, idf, df

    def transform(self, docs):
        h = c_vp()
        check(self.ctx.lib.pfz_tfidf_transform(self.ctx.h, self.h, docs.h, ctypes.byref(h)))
        return DeviceCSR(self.ctx, h)


# ---- edit distance / dense ---------------------------------------------------------

def indel_argmax(ctx, from_dev, to_dev, skip_idx=None, begin=0, end=None):
    """K4: (first arg-max index int32[n], ratio float64[n]) of from-rows [begin, end)."""
    end = from_dev.n if end is None else end
    n = end - begin
    idx = np.empty(n, np.int32)
    score = np.empty(n, np.float64)
    if skip_idx is not None:
        skip_idx = np.ascontiguousarray(skip_idx, np.int32)
        if len(skip_idx) != from_dev.n:
            raise ValueError("skip_idx must have one entry per from-string")
    check(ctx.lib.pfz_indel_argmax(ctx.h, from_dev.h, to_dev.h, _ptr(skip_idx), int(begin), int(end),
                                   _ptr(idx), _ptr(score)))
    return idx, score


def indel_topn(ctx, from_dev, to_dev, ntop, skip_idx=None, begin=0, end=None):
    """K4: the ntop best choices of from-rows [begin, end) -- (index int32[n, ntop], ratio float64[n, ntop]) in the order
    (ratio descending, to-index ascending); -1 / 0.0 beyond the choices a row has.  ntop <= 64 (PfzUnsupported beyond)."""
    end = from_dev.n if end is None else end
    n = end - begin
    idx = np.empty((n, max(int(ntop), 0)), np.int32)           # (ntop < 1 is the library's to refuse)
    score = np.empty((n, max(int(ntop), 0)), np.float64)
    skip_idx = _skip_array(skip_idx, from_dev.n)
    check(ctx.lib.pfz_indel_topn(ctx.h, from_dev.h, to_dev.h, _ptr(skip_idx), int(begin), int(end), int(ntop), _ptr(idx), _ptr(score)))
    return idx, score


def indel_plan_info(ctx, to_dev):
    """Build (once) and describe K4's cached to-side plan of a DeviceStrings handle."""
    v = [c_i64() for _ in range(3)]
    check(ctx.lib.pfz_indel_plan_info(ctx.h, to_dev.h, *[ctypes.byref(x) for x in v]))
    return {"n_symbols": v[0].value, "n_groups": v[1].value, "char_steps": v[2].value}


FUZZ_SCORERS = {"WRatio": 0, "partial_ratio": 1, "token_set_ratio": 2, "token_ratio": 3, "partial_token_sort_ratio": 4,
                "partial_token_set_ratio": 5, "partial_token_ratio": 6}


def _skip_array(skip_idx, n):
    if skip_idx is None:
        return None
    skip_idx = np.ascontiguousarray(skip_idx, np.int32)
    if len(skip_idx) != n:
        raise ValueError("skip_idx must have one entry per from-string")
    return skip_idx


def _as_device_strings(ctx, strings):
    return strings if isinstance(strings, DeviceStrings) else DeviceStrings.upload(ctx, strings)


def fuzz_extract_one(ctx, from_list, to_list, scorer, skip_idx=None, begin=0, end=None):
    """K7: process.extractOne(from_string, to_list, scorer=fuzz.<scorer>) for every from-string of rows [begin, end) --
    (index of the first best choice int32[n] (-1: none), its score float64[n] on rapidfuzz's 0..100 scale).
    from_list / to_list: lists of str (uploaded here) or resident DeviceStrings -- the token forms of a list and the
    plan of a to-list are built on the device on first use and stay cached on the handle; every pair is bounded, the
    promising ones scored, on the device."""
    same = to_list is from_list
    f_dev = _as_device_strings(ctx, from_list)
    t_dev = f_dev if same else _as_device_strings(ctx, to_list)
    end = f_dev.n if end is None else end
    n = end - begin
    idx = np.empty(n, np.int32)
    score = np.empty(n, np.float64)
    skip_idx = _skip_array(skip_idx, f_dev.n)
    check(ctx.lib.pfz_fuzz_extract_one(ctx.h, f_dev.h, t_dev.h, FUZZ_SCORERS[scorer], _ptr(skip_idx), int(begin), int(end),
                                       _ptr(idx), _ptr(score)))
    return idx, score


def fuzz_extract_one_dev(ctx, from_dev, to_dev, scorer, out, skip_idx=None, begin=0, end=None, counters=False):
    """K7 with the (index, float64 score) rows left in the 2-column DeviceTopN `out` (see best_from_topn); returns the work
    counters {bounded, scored, word_steps} when asked (that waits for the kernel)."""
    end = from_dev.n if end is None else end
    skip_idx = _skip_array(skip_idx, from_dev.n)
    work = np.zeros(4, np.uint64) if counters else None
    check(ctx.lib.pfz_fuzz_extract_one_dev(ctx.h, from_dev.h, to_dev.h, FUZZ_SCORERS[scorer], _ptr(skip_idx), int(begin), int(end),
                                           out.h, _ptr(work)))
    if counters:
        return {"pairs_bounded": int(work[0]), "pairs_scored": int(work[1]), "word_steps_scored": int(work[2])}
    return None


def indel_argmax_dev(ctx, from_dev, to_dev, out, skip_idx=None, begin=0, end=None):
    """K4 with the (first arg-max, float64 ratio) rows left in the 2-column DeviceTopN `out` (see best_from_topn)."""
    end = from_dev.n if end is None else end
    skip_idx = _skip_array(skip_idx, from_dev.n)
    check(ctx.lib.pfz_indel_argmax_dev(ctx.h, from_dev.h, to_dev.h, _ptr(skip_idx), int(begin), int(end), out.h))


def best_from_topn(idx2, val2):
    """(index int32[n], score float64[n]) out of the downloaded arrays of a 2-column result buffer: column 0 of idx, the
    two fp32 value lanes of a row read as one float64"""
    return idx2[:, 0].copy(), np.ascontiguousarray(val2).view(np.float64).reshape(-1)


def fuzz_plan_info(ctx, to_dev):
    """Build (once) and describe K7's cached plan of a DeviceStrings handle used as a to-list."""
    v = [c_i64() for _ in range(4)]
    check(ctx.lib.pfz_fuzz_plan_info(ctx.h, to_dev.h, *[ctypes.byref(x) for x in v]))
    return {"n_symbols": v[0].value, "n_groups": v[1].value, "n_tokens": v[2].value, "n_general_strings": v[3].value}


def indel_matrix(ctx, from_dev, to_dev, begin=0, end=None):
    end = from_dev.n if end is None else end
    out = np.empty((end - begin, to_dev.n), np.float64)
    check(ctx.lib.pfz_indel_matrix_host(ctx.h, from_dev.h, to_dev.h, int(begin), int(end), _ptr(out)))
    return out


# K8: jellyfish.jaro_similarity / jaro_winkler_similarity (default arguments), float64 on the 0..1 scale.  PARITY UNPINNED:
# jellyfish is not importable where this was built; the definition is restated in include/polyfuzz_hip.h.
JARO_SCORERS = {"jaro": 0, "jaro_winkler": 1}


def jaro_argmax(ctx, from_dev, to_dev, scorer, skip_idx=None, begin=0, end=None):
    """K8: (first arg-max index int32[n], score float64[n]) of from-rows [begin, end)."""
    end = from_dev.n if end is None else end
    n = end - begin
    idx = np.empty(n, np.int32)
    score = np.empty(n, np.float64)
    skip_idx = _skip_array(skip_idx, from_dev.n)
    check(ctx.lib.pfz_jaro_argmax(ctx.h, from_dev.h, to_dev.h, JARO_SCORERS[scorer], _ptr(skip_idx), int(begin), int(end),
                                  _ptr(idx), _ptr(score)))
    return idx, score


def jaro_argmax_dev(ctx, from_dev, to_dev, scorer, out, skip_idx=None, begin=0, end=None):
    """K8 with the (first arg-max, float64 score) rows left in the 2-column DeviceTopN `out` (see best_from_topn)."""
    end = from_dev.n if end is None else end
    skip_idx = _skip_array(skip_idx, from_dev.n)
    check(ctx.lib.pfz_jaro_argmax_dev(ctx.h, from_dev.h, to_dev.h, JARO_SCORERS[scorer], _ptr(skip_idx), int(begin), int(end), out.h))


def jaro_matrix(ctx, from_dev, to_dev, scorer, begin=0, end=None):
    """K8: every score of from-rows [begin, end) x all to-strings, float64 [end - begin, n_to] (the test entry)."""
    end = from_dev.n if end is None else end
    out = np.empty((end - begin, to_dev.n), np.float64)
    check(ctx.lib.pfz_jaro_matrix_host(ctx.h, from_dev.h, to_dev.h, JARO_SCORERS[scorer], int(begin), int(end), _ptr(out)))
    return out


# K9: rapidfuzz's Levenshtein.normalized_similarity / OSA.normalized_similarity (default arguments), float64 on the 0..1 scale.
# PARITY UNPINNED: rapidfuzz is not importable where this was built; the definition is restated in include/polyfuzz_hip.h.
LEV_SCORERS = {"levenshtein": 0, "osa": 1}


def lev_argmax(ctx, from_dev, to_dev, scorer, skip_idx=None, begin=0, end=None):
    """K9: (first arg-max index int32[n], similarity float64[n]) of from-rows [begin, end)."""
    end = from_dev.n if end is None else end
    n = end - begin
    idx = np.empty(n, np.int32)
    score = np.empty(n, np.float64)
    skip_idx = _skip_array(skip_idx, from_dev.n)
    check(ctx.lib.pfz_lev_argmax(ctx.h, from_dev.h, to_dev.h, LEV_SCORERS[scorer], _ptr(skip_idx), int(begin), int(end),
                                 _ptr(idx), _ptr(score)))
    return idx, score


def lev_argmax_dev(ctx, from_dev, to_dev, scorer, out, skip_idx=None, begin=0, end=None):
    """K9 with the (first arg-max, float64 similarity) rows left in the 2-column DeviceTopN `out` (see best_from_topn)."""
    end = from_dev.n if end is None else end
    skip_idx = _skip_array(skip_idx, from_dev.n)
    check(ctx.lib.pfz_lev_argmax_dev(ctx.h, from_dev.h, to_dev.h, LEV_SCORERS[scorer], _ptr(skip_idx), int(begin), int(end), out.h))


def lev_topn(ctx, from_dev, to_dev, scorer, ntop, skip_idx=None, begin=0, end=None):
    """K9: the ntop best choices of from-rows [begin, end) -- (index int32[n, ntop], similarity float64[n, ntop]) in the order
    (similarity descending, to-index ascending); -1 / 0.0 beyond the choices a row has.  ntop <= 64 (PfzUnsupported beyond)."""
    end = from_dev.n if end is None else end
    n = end - begin
    idx = np.empty((n, max(int(ntop), 0)), np.int32)           # (ntop < 1 is the library's to refuse)
    score = np.empty((n, max(int(ntop), 0)), np.float64)
    skip_idx = _skip_array(skip_idx, from_dev.n)
    check(ctx.lib.pfz_lev_topn(ctx.h, from_dev.h, to_dev.h, LEV_SCORERS[scorer], _ptr(skip_idx), int(begin), int(end), int(ntop),
                               _ptr(idx), _ptr(score)))
    return idx, score


def lev_matrix(ctx, from_dev, to_dev, scorer, begin=0, end=None):
    """K9: every DISTANCE of from-rows [begin, end) x all to-strings, int32 [end - begin, n_to] (the test entry)."""
    end = from_dev.n if end is None else end
    out = np.empty((end - begin, to_dev.n), np.int32)
    check(ctx.lib.pfz_lev_matrix_host(ctx.h, from_dev.h, to_dev.h, LEV_SCORERS[scorer], int(begin), int(end), _ptr(out)))
    return out


LEV_JOIN_COUNTERS = ("pairs_in_window", "pairs_finished", "steps")


def _join_call(n_from, capacity, dtypes, counter_names, counters, call):
    """The capacity protocol of every threshold join: buffers for `capacity` hits (None: a modest guess, four per from-row),
    call(cap, row_ptr, per-hit arrays, total, work) -> the ctypes call's status, ONE repeat with room for the exact total when it
    exceeds cap.  Returns (row_ptr, copies of the per-hit arrays cut to the total, total, dict of the counters or None)."""
    work = np.zeros(len(counter_names), np.int64) if counters else None
    total = c_i64(0)
    cap = max(4096, 4 * int(n_from)) if capacity is None else int(capacity)
    for repeat in (False, True):
        row_ptr = np.empty(n_from + 1, np.int64)
        hits = [np.empty(cap, dt) for dt in dtypes]
        check(call(cap, _ptr(row_ptr), [_ptr(a) for a in hits], ctypes.byref(total), _ptr(work)))
        if total.value <= cap:
            break
        if repeat:                                # (the second call had room for the exact total)
            raise AssertionError(f"the repeated call reports {total.value} hits, the first reported {cap}")
        cap = total.value
    n = total.value
    return row_ptr, tuple(a[:n].copy() for a in hits), n, dict(zip(counter_names, work.tolist())) if counters else None


def _components_call(n, counter_names, counters, call):
    """A components entry: call(label, pairs, components, work) -> the ctypes call's status; (label int32[n], pairs, components),
    and with counters the dict of them appended"""
    work = np.zeros(len(counter_names), np.int64) if counters else None
    label = np.empty(n, np.int32)
    pairs, components = c_i64(0), c_i64(0)
    check(call(_ptr(label), ctypes.byref(pairs), ctypes.byref(components), _ptr(work)))
    out = (label, pairs.value, components.value)
    return out + (dict(zip(counter_names, work.tolist())),) if counters else out


def lev_join(ctx, from_dev, to_dev, scorer, min_similarity, capacity=None, counters=False):
    """K11: every pair with similarity >= min_similarity (float64 against float64, equal is a hit) as CSR over the from-rows --
    (row_ptr int64[n + 1], to-index int32[hits] ascending within a row, distance int32[hits], similarity float64[hits]).
    to_dev None (or from_dev itself): the self-join, every unordered pair once as (i, j), i < j.  capacity: the hits the first call's
    buffers have room for (None: a modest guess, four per from-string); when the exact total the call returns exceeds it the
    call is repeated ONCE with room for that total, never more often.  counters=True appends a dict of LEV_JOIN_COUNTERS (the
    last call's)."""
    to_h = None if to_dev is None else to_dev.h
    row_ptr, hits, _, work = _join_call(
        from_dev.n, capacity, (np.int32, np.int32, np.float64), LEV_JOIN_COUNTERS, counters,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_lev_join(ctx.h, from_dev.h, to_h, LEV_SCORERS[scorer], float(min_similarity), cap,
                                                              ptr, *hit, total, wk))
    return (row_ptr,) + hits + ((work,) if counters else ())


def lev_components(ctx, dev, scorer, min_similarity, counters=False):
    """K12: the connected components of "similarity >= min_similarity" over the list `dev` (the pairs of lev_join's self-join,
    united on the device, never stored) -- (label int32[n], pairs, components): label[i] is the smallest position in i's
    component, pairs the number of hits (lev_join's total), components the number of components, singletons included.
    counters=True appends a dict of LEV_JOIN_COUNTERS (the walk is lev_join's: so are the values)."""
    return _components_call(dev.n, LEV_JOIN_COUNTERS, counters, lambda label, pairs, components, wk: ctx.lib.pfz_lev_components(
        ctx.h, dev.h, LEV_SCORERS[scorer], float(min_similarity), label, pairs, components, wk))


# K13: rapidfuzz.distance.Indel.normalized_similarity (K4's metric on the 0..1 scale), the definition of include/polyfuzz_hip.h

def indel_similarity(lcs, total_len):
    """1.0 - (S - 2 lcs) / S in float64 (one division, one subtraction), 1.0 where S = |a| + |b| is 0; arrays broadcast"""
    lcs, s = np.asarray(lcs, np.int64), np.asarray(total_len, np.int64)
    pos = s > 0
    return np.where(pos, 1.0 - (s - 2 * lcs).astype(np.float64) / np.where(pos, s, 1).astype(np.float64), 1.0)


def indel_lcs_of_ratio(ratio, total_len):
    """The integer LCS behind K4's float64 ratio (0..100) of pairs whose two lengths sum to total_len: the integer near
    ratio * S / 200 (or one beside it) whose (1.0 - (S - 2 lcs) / S) * 100.0 reproduces the ratio's bits.  Raises ValueError
    where no such integer exists -- then the ratio is not K4's for these lengths.  Vectorised; no per-character work."""
    ratio, s = np.asarray(ratio, np.float64), np.asarray(total_len, np.int64)
    ratio, s = np.broadcast_arrays(ratio, s)
    guess = np.rint(ratio * s / 200.0).astype(np.int64)
    lcs = np.full(ratio.shape, -1, np.int64)
    for cand in (guess, guess - 1, guess + 1):
        cand = np.clip(cand, 0, s // 2)
        ok = (lcs < 0) & (indel_similarity(cand, s) * 100.0 == ratio)
        lcs[ok] = cand[ok]
    if (lcs < 0).any():
        bad = int(np.flatnonzero((lcs < 0).reshape(-1))[0])
        raise ValueError(f"ratio {ratio.reshape(-1)[bad]!r} is no Indel ratio of two strings of {int(s.reshape(-1)[bad])} characters in all")
    return lcs


def indel_join(ctx, from_dev, to_dev, min_similarity, capacity=None, counters=False):
    """K13: lev_join's twin under the Indel similarity (rapidfuzz.distance.Indel.normalized_similarity): every pair with
    similarity >= min_similarity as CSR over the from-rows -- (row_ptr int64[n + 1], to-index int32[hits] ascending within a
    row, Indel distance |a| + |b| - 2 lcs int32[hits], similarity float64[hits]).  to_dev None (or from_dev itself): the
    self-join, i < j.  capacity and the ONE repeat as in lev_join; counters=True appends a dict of LEV_JOIN_COUNTERS."""
    to_h = None if to_dev is None else to_dev.h
    row_ptr, hits, _, work = _join_call(
        from_dev.n, capacity, (np.int32, np.int32, np.float64), LEV_JOIN_COUNTERS, counters,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_indel_join(ctx.h, from_dev.h, to_h, float(min_similarity), cap, ptr, *hit, total, wk))
    return (row_ptr,) + hits + ((work,) if counters else ())


def indel_components(ctx, dev, min_similarity, counters=False):
    """K13: lev_components's twin under the Indel similarity -- (label int32[n], pairs, components), the pairs of indel_join's
    self-join united on the device, never stored.  counters=True appends a dict of LEV_JOIN_COUNTERS."""
    return _components_call(dev.n, LEV_JOIN_COUNTERS, counters, lambda label, pairs, components, wk: ctx.lib.pfz_indel_components(
        ctx.h, dev.h, float(min_similarity), label, pairs, components, wk))


# scorer of K10 -> PFZ_PAIR_* (include/polyfuzz_hip.h)
PAIR_SCORERS = {"ratio": 0, "levenshtein": 1, "osa": 2, "jaro": 3, "jaro_winkler": 4}
PAIR_MAX_CANDIDATES = 1024             # candidates per from-row pfz_pairs_rescore_topn ranks
PAIR_MAX_TOP_N = 64                    # one list entry per lane of a wave (csrc/topn_wave.h)


def pairs_rescore_topn(ctx, from_dev, to_dev, candidates, scorer, ntop):
    """K10: the candidates of every from-string -- row i of the DeviceTopN `candidates`: indices into to_dev, anything outside
    [0, n_to) skipped -- scored under `scorer` (a PAIR_SCORERS name, or its id) and re-ranked: (index int32[n, ntop], score
    float64[n, ntop]) in the order (score descending, to-index ascending); -1 / 0.0 beyond the candidates a row has.  The table
    stays on the device.  ntop <= 64 and <= 1024 candidates per row (PfzUnsupported beyond)."""
    n = from_dev.n
    idx = np.empty((n, max(int(ntop), 0)), np.int32)           # (ntop < 1 is the library's to refuse)
    score = np.empty((n, max(int(ntop), 0)), np.float64)
    sid = PAIR_SCORERS[scorer] if isinstance(scorer, str) else int(scorer)
    check(ctx.lib.pfz_pairs_rescore_topn(ctx.h, from_dev.h, to_dev.h, candidates.h, sid, int(ntop), _ptr(idx), _ptr(score)))
    return idx, score


# K16: the scorers of K10 that live on 0..1 (ratio, on 0..100, has no threshold form), and pfz_pairs_join's out_counters, in order
PAIR_JOIN_SCORERS = {"levenshtein": 1, "osa": 2, "jaro": 3, "jaro_winkler": 4}
PAIR_JOIN_COUNTERS = ("candidates", "scored", "pairs")


def pairs_join(ctx, from_dev, to_dev, candidates, scorer, min_similarity, capacity=None, counters=False):
    """K16: the candidate pairs of the DeviceTopN `candidates` (K10's input: row i holds indices into to_dev, anything outside
    [0, n_to) skipped, an index listed twice counted once) whose score under `scorer` (a PAIR_JOIN_SCORERS name, or a PFZ_PAIR_*
    id) is >= min_similarity (float64 against float64, equal is a hit), as CSR over the from-rows -- (row_ptr int64[n + 1],
    to-index int32[hits] ascending within a row, similarity float64[hits]).  to_dev None (or from_dev itself): the self-join over
    the symmetrised table, every unordered pair {i, j} with j in row i or i in row j once, as (min, max), scored with the lower
    position as the from-string; a row's own index is skipped.  capacity and the ONE repeat as in lev_join.  counters=True appends
    a dict of PAIR_JOIN_COUNTERS (the last call's): table cells that are a candidate pair, distinct pairs scored, hits."""
    t = check_min_similarity(min_similarity)
    sid = PAIR_JOIN_SCORERS[scorer] if isinstance(scorer, str) else int(scorer)
    to_h = None if to_dev is None else to_dev.h
    row_ptr, hits, _, work = _join_call(
        from_dev.n, capacity, (np.int32, np.float64), PAIR_JOIN_COUNTERS, counters,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_pairs_join(ctx.h, from_dev.h, to_h, candidates.h, sid, t, cap, ptr, *hit, total, wk))
    return (row_ptr,) + hits + ((work,) if counters else ())


def pairs_components(ctx, dev, candidates, scorer, min_similarity, counters=False):
    """K16: the connected components of the graph whose edges are the hits of pairs_join's self-join over `dev` and `candidates`,
    united on the device, never stored -- (label int32[n], pairs, components): label[i] is the smallest position in i's component,
    pairs the number of hits (pairs_join's total), components the number of components, singletons included.  counters=True
    appends a dict of PAIR_JOIN_COUNTERS."""
    t = check_min_similarity(min_similarity)
    sid = PAIR_JOIN_SCORERS[scorer] if isinstance(scorer, str) else int(scorer)
    return _components_call(dev.n, PAIR_JOIN_COUNTERS, counters, lambda label, pairs, components, wk: ctx.lib.pfz_pairs_components(
        ctx.h, dev.h, candidates.h, sid, t, label, pairs, components, wk))


# compute_dtype of the dense path -> PFZ_DENSE_* (include/polyfuzz_hip.h)
DENSE_DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2}
_DENSE_SRC_SAME, _DENSE_SRC_F32 = 0, 1
# every operand type of the dense path: what the two public keywords, `compute_dtype` and `precision`, choose between
OPERAND_TYPES = ("float32", "float16", "bfloat16", "int8")


def check_compute_dtype(compute_dtype):
    """None / "float32": fp32 operands and the fp32 matrix cores (the default: scores of the vectors as given to 1e-5).
    "float16" / "bfloat16": the vectors are kept as 16-bit values and multiplied on the 16-bit matrix cores (16 x the fp32
    rate, half the memory) with fp32 accumulation.  The similarity is then that of the 16-BIT vectors, exact to fp32
    accuracy for vectors that are 16-bit to begin with; float32 vectors are rounded first, which moves every element by
    about 1e-3 (float16) or 1e-2 (bfloat16) relative and the scores with them -- that is why the keyword is opt-in."""
    name = "float32" if compute_dtype is None else compute_dtype
    if not isinstance(name, str) or name not in DENSE_DTYPES:
        raise ValueError(f"compute_dtype must be None or one of {sorted(DENSE_DTYPES)}, got {compute_dtype!r}")
    return name


def dense_cossim_topn_host(ctx, from_vec, to_vec, ntop, lower_bound, exclude_diag=False, normalize=True, compute_dtype=None):
    """normalize=False: raw dot products (the reference's "sparse" back-end on dense input).
    compute_dtype: see check_compute_dtype -- with "float16" / "bfloat16" the scores are those of the 16-bit vectors
    (float32 input is rounded: about 1e-3 / 1e-2 relative per element), so it is opt-in; None / "float32" is the fp32 path."""
    operand = check_compute_dtype(compute_dtype)
    if operand != "float32":
        return _dense_topn_host(ctx, from_vec, to_vec, ntop, lower_bound, exclude_diag, normalize, operand)
    a = np.ascontiguousarray(from_vec, np.float32)
    b = np.ascontiguousarray(to_vec, np.float32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"dense cosine needs two 2-D arrays with equal width, got {a.shape} and {b.shape}")
    idx = np.empty((a.shape[0], ntop), np.int32)
    val = np.empty((a.shape[0], ntop), np.float32)
    fn = ctx.lib.pfz_dense_cossim_topn_host if normalize else ctx.lib.pfz_dense_dot_topn_host
    check(fn(ctx.h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], a.shape[1], int(ntop), float(lower_bound),
             int(bool(exclude_diag)), _ptr(idx), _ptr(val)))
    return idx, val


def check_precision(precision):
    """The `precision` of the dense path, named after sentence-transformers' keyword: None (the operands `compute_dtype`
    selects) or "int8": the vectors are kept as signed 8-bit values and multiplied on the integer matrix cores with int32
    accumulation, which is exact -- the similarity is that of the INT8 vectors to fp32 rounding.  An np.int8 matrix is taken
    as it is; float vectors are quantised per row (DeviceDense.upload_int8), which moves the cosines by a few 1e-3
    (DESIGN.md section 4 has the measured figure): that is why it is opt-in.  Anything else raises ValueError."""
    if precision is None or (isinstance(precision, str) and precision == "int8"):
        return precision
    raise ValueError(f'precision must be None or "int8", got {precision!r}')


def operand_type(compute_dtype=None, precision=None):
    """The one of OPERAND_TYPES the two keywords name together; ValueError when either is invalid or both name a type."""
    name = check_compute_dtype(compute_dtype)
    if check_precision(precision) is None:
        return name
    if name != "float32":
        raise ValueError(f'precision="int8" and compute_dtype={compute_dtype!r} name two operand types: '
                         'leave compute_dtype at None')
    return "int8"


def _dense_topn_host(ctx, from_vec, to_vec, ntop, lower_bound, exclude_diag, normalize, operand, multiplier=None, rescore_to=None):
    """The one-shots' common body: upload both sides as `operand` (one of OPERAND_TYPES, or BINARY through its own door; one
    handle when to_vec is from_vec), run K5 -- with a `multiplier` rescored against float32 uploads of the same arrays, or with
    `rescore_to` ("int8" / BINARY) the float32 from-side against the to-side in that form, which is `operand`'s handle when the
    two are equal: no float32 to-side is made -- and download (idx, val)."""
    same = to_vec is from_vec
    def upload(c, v, nrm, form=operand):
        return DeviceDense.upload_bits(c, v, nrm) if form == BINARY else DeviceDense.upload_as(c, v, form, nrm)
    a = upload(ctx, from_vec, normalize)
    b = a if same else upload(ctx, to_vec, normalize)
    if a.dim != b.dim:
        raise ValueError(f"dense cosine needs two 2-D arrays with equal width, got {(a.n, a.dim)} and {(b.n, b.dim)}"
                         + (BITS_WIDTH_HINT if operand == BINARY else ""))
    if multiplier is None:
        return dense_topn(ctx, a, b, ntop, lower_bound, exclude_diag).download()
    a_x = DeviceDense.upload_as(ctx, from_vec, "float32", normalize)
    if rescore_to is not None:
        b_x = b if rescore_to == operand else upload(ctx, to_vec, normalize, rescore_to)
    else:
        b_x = a_x if same else DeviceDense.upload_as(ctx, to_vec, "float32", normalize)
    return dense_topn_rescored(ctx, a, b, a_x, b_x, ntop, lower_bound, multiplier, exclude_diag).download()


def dense_int8_topn_host(ctx, from_vec, to_vec, ntop, lower_bound, exclude_diag=False, normalize=True):
    """dense_cossim_topn_host on int8 operands (DeviceDense.upload_int8): np.int8 arrays as they are, float arrays quantised
    per row.  normalize=False: raw dot products -- of the integers as given, or of the dequantised rows."""
    return _dense_topn_host(ctx, from_vec, to_vec, ntop, lower_bound, exclude_diag, normalize, "int8")


def dense_hamming_topn_host(ctx, from_vec, to_vec, ntop, lower_bound, exclude_diag=False, normalize=True):
    """dense_cossim_topn_host on 1-bit operands (DeviceDense.upload_bits): np.uint8 / np.int8 packed rows, or float arrays
    packed on the device.  The score of a pair with h differing bits of d is the cosine of the +-1 vectors, float32(d - 2 h) /
    float32(d); normalize=False: their dot product d - 2 h."""
    return _dense_topn_host(ctx, from_vec, to_vec, ntop, lower_bound, exclude_diag, normalize, BINARY)


# ---- 1-bit operands: a door of their own (`precision`, `compute_dtype` and OPERAND_TYPES do not know them) -----------------
BINARY = "binary"                              # DeviceDense.dtype of a bit handle
BINARY_FORMS = ("binary", "ubinary")           # sentence-transformers' two spellings of packed sign bits: one device path
BITS_WIDTH_HINT = (" (packed rows count 8 bits per byte: float vectors whose width is not a multiple of 8 cannot be paired "
                   "with rows packed on the host -- pack both sides the same way)")


def check_binary(value):
    """`Embeddings.binary`: None (the dense operands of `compute_dtype` / `precision`) or "binary" / "ubinary", the names
    sentence-transformers gives packed sign bits (np.packbits(x > 0), as uint8 = "ubinary" or shifted by -128 as int8 =
    "binary").  Both select the same device path -- what is uploaded decides how it is read (DeviceDense.upload_bits).
    Anything else raises ValueError."""
    if value is None or (isinstance(value, str) and value in BINARY_FORMS):
        return value
    raise ValueError(f"binary must be None or one of {BINARY_FORMS}, got {value!r}")


def ubinary_rows(vec):
    """Packed rows as the device holds them: np.uint8 ("ubinary") as they are; np.int8 ("binary" = ubinary - 128) is the
    same bytes with bit 7 flipped."""
    vec = np.ascontiguousarray(vec)
    if vec.dtype == np.uint8:
        return vec
    if vec.dtype == np.int8:
        return vec.view(np.uint8) ^ np.uint8(0x80)
    raise ValueError(f"packed binary rows are a uint8 or an int8 array, got {vec.dtype}")


# operand type -> (the numpy dtype that is uploaded as it is -- any other float array goes up as float32 and is converted on
# the device; None: everything is widened to float32 --, what the refusal of any other dtype says, the C entry point and its
# arguments between `normalize` and the handle)
_OPERANDS = {
    "float32": (None, None, "pfz_dense_upload", lambda source: ()),
    "float16": (np.float16, "compute_dtype='float16' takes a float array",
                "pfz_dense_upload16", lambda source: (DENSE_DTYPES["float16"], source)),
    "bfloat16": (np.uint16, "compute_dtype='bfloat16' takes a float array or raw bfloat16 bits as uint16",
                 "pfz_dense_upload16", lambda source: (DENSE_DTYPES["bfloat16"], source)),
    "int8": (np.int8, "int8 precision takes an int8 or a float array", "pfz_dense_upload8", lambda source: (source,)),
}


class DeviceDense(_Handle):
    """Device-resident row-major matrix (fp32, float16 / bfloat16 or int8 values, or packed bits) + the per-row factors (K5
    operand)."""
    _free = "pfz_dense_free"

    @classmethod
    def upload_as(cls, ctx, vec, operand, normalize=True):
        """The one upload: `vec` as `operand`, one of OPERAND_TYPES (see upload and upload_int8 for what each takes)."""
        if not isinstance(operand, str) or operand not in _OPERANDS:
            raise ValueError(f"operand must be one of {OPERAND_TYPES}, got {operand!r}")
        as_given, takes, entry, extra = _OPERANDS[operand]
        vec = np.asarray(vec)
        if vec.ndim != 2:
            raise ValueError(f"dense vectors must be a 2-D array, got shape {vec.shape}")
        given = as_given is not None and vec.dtype == as_given
        if takes is not None and not given and vec.dtype.kind != "f":
            raise ValueError(f"{takes}, got {vec.dtype}"
                             + (" (unsigned values are not supported: shifting them by 128 changes the cosine)"
                                if operand == "int8" and vec.dtype == np.uint8 else ""))
        a = np.ascontiguousarray(vec) if given else np.ascontiguousarray(vec, np.float32)
        h = c_vp()
        check(getattr(ctx.lib, entry)(ctx.h, _ptr(a) if a.size else None, a.shape[0], max(a.shape[1], 1), int(bool(normalize)),
                                      *extra(_DENSE_SRC_SAME if given else _DENSE_SRC_F32), ctypes.byref(h)))
        m = cls(ctx, h)
        m.n, m.dim, m.normalize, m.dtype = a.shape[0], a.shape[1], bool(normalize), operand
        return m

    @classmethod
    def upload(cls, ctx, vec, normalize=True, compute_dtype=None):
        """compute_dtype None / "float32": widened to fp32 whatever `vec` holds (also a float16 array).
        "float16": a np.float16 array is uploaded as it is, any other float array as fp32 and rounded (to nearest even) on
        the device.  "bfloat16": a np.uint16 array is taken as raw bfloat16 bits (numpy has no such dtype), a float array is
        rounded on the device.  The similarity is then that of the 16-bit vectors: rounding float32 vectors changes the
        scores by about 1e-3 (float16) or 1e-2 (bfloat16) relative per element, which is why this is opt-in."""
        return cls.upload_as(ctx, vec, check_compute_dtype(compute_dtype), normalize)

    def derive16(self, dtype):
        """The search copy of an fp32 handle uploaded with normalize=True, made on the device (K22): row values
        round16(x[k] * (1 / ||row||)), to nearest even, as "float16" or "bfloat16" -- every value in [-1, 1].  The vectors are
        uploaded once; the copy is a 16-bit operand like any other."""
        if dtype not in ("float16", "bfloat16"):
            raise ValueError(f"the search types are 'float16' and 'bfloat16', got {dtype!r}")
        _dense_join_operand(self, "the vectors")
        h = c_vp()
        check(self.ctx.lib.pfz_dense_derive16(self.ctx.h, self.h, DENSE_DTYPES[dtype], ctypes.byref(h)))
        m = type(self)(self.ctx, h)
        m.n, m.dim, m.normalize, m.dtype = self.n, self.dim, True, dtype
        return m

    @classmethod
    def upload_bits(cls, ctx, vec, normalize=True):
        """1-bit rows (K5's Hamming tile program).  An np.uint8 array [n, B] is "ubinary": d = 8 B bits in np.packbits order,
        uploaded as it is.  An np.int8 array is "binary" (ubinary - 128) and brought to that form first (ubinary_rows): on
        the device the two are one.  A float array [n, dim] goes up as float32 and is packed on the device, d = dim, bit =
        x > 0 (NaN and +-0 give 0): the bytes of np.packbits(x > 0, axis=1).  The score of two rows with h differing bits
        is float32(d - 2 h) / float32(d), or with normalize=False d - 2 h; d < 2**24.  Other dtypes and arrays that are not
        2-D raise ValueError.  The handle has dtype "binary" and dim = d."""
        vec = np.asarray(vec)
        if vec.ndim != 2:
            raise ValueError(f"dense vectors must be a 2-D array, got shape {vec.shape}")
        if vec.dtype in (np.uint8, np.int8):
            a, bits, source = ubinary_rows(vec), 8 * vec.shape[1], _DENSE_SRC_SAME
        elif vec.dtype.kind == "f":
            a, bits, source = np.ascontiguousarray(vec, np.float32), vec.shape[1], _DENSE_SRC_F32
        else:
            raise ValueError(f"binary vectors are packed uint8 / int8 rows or a float array, got {vec.dtype}")
        h = c_vp()
        check(ctx.lib.pfz_dense_upload1(ctx.h, _ptr(a) if a.size else None, a.shape[0], max(bits, 1), int(bool(normalize)),
                                        source, ctypes.byref(h)))
        m = cls(ctx, h)
        m.n, m.dim, m.normalize, m.dtype = a.shape[0], bits, bool(normalize), BINARY
        return m

    @classmethod
    def upload_int8(cls, ctx, vec, normalize=True):
        """An np.int8 array is uploaded as it is.  A float array goes up as fp32 and is quantised on the device, symmetric
        per row: q = rint((x / max|x|) * 127), row scale max|x| / 127 (zero rows stay zero; non-finite values are outside the
        contract).  The scores are the cosines of the int8 rows -- the cosine does not depend on a row's scale --, or with
        normalize=False the dot products: of the integers as given, or of the dequantised rows q * scale.
        Widths up to 131071 (an int32 dot product of int8 rows).  Any other dtype raises ValueError, uint8 among them: the
        integer matrix cores are signed, and shifting by 128 changes the cosine."""
        return cls.upload_as(ctx, vec, "int8", normalize)


def dense_topn(ctx, from_dev, to_dev, ntop, lower_bound, exclude_diag=False, diag_offset=0, out=None):
    """Enqueue K5 on resident operands; returns the (device-resident) DeviceTopN."""
    if out is None:
        out = DeviceTopN.alloc(ctx, from_dev.n, ntop)
    check(ctx.lib.pfz_dense_topn(ctx.h, from_dev.h, to_dev.h, int(ntop), float(lower_bound), int(bool(exclude_diag)),
                                 int(diag_offset), out.h))
    return out


# ---- K14: the cosine threshold join and its components ---------------------------------------------------------------

DENSE_JOIN_COUNTERS = ("tiles", "hit_corners")      # pfz_dense_join's out_counters, in order


def dense_threshold32(t):
    """The smallest float32 >= t (a float64): a float32 score s satisfies float64(s) >= t exactly when s >= this value --
    the comparison K14 makes on the device.  Pure numpy."""
    t = np.float64(t)
    r = np.float32(t)                              # (to nearest: at most one step below t)
    return np.nextafter(r, np.float32(np.inf)) if np.float64(r) < t else r


def _dense_join_operand(dev, what):
    if dev.dtype != "float32" or not dev.normalize:
        raise ValueError(f"{what} are {dev.dtype} vectors uploaded with normalize={dev.normalize}: the cosine threshold kernels "
                         "take fp32 operands uploaded with normalize=True (DeviceDense.upload)")


def dense_join(ctx, from_dev, to_dev, min_similarity, capacity=None, counters=False):
    """K14: every pair of rows whose cosine -- dense_topn's float32, bit for bit -- is >= min_similarity (as float64: equal is a
    hit), as CSR over the from-rows: (row_ptr int64[n + 1], to-index int32[hits] ascending within a row, similarity
    float32[hits], counts).  to_dev None (or from_dev itself): the self-join, every unordered pair once as (i, j), i < j, only
    the tiles on or above the diagonal computed.  fp32 operands uploaded with normalize=True only.  capacity: the hits the first
    call's buffers have room for (None: a modest guess, four per from-row); when the exact total the call returns exceeds it
    the call is repeated ONCE with room for that total, never more often.  counts: {"pairs": hits}, with counters=True also
    DENSE_JOIN_COUNTERS (the last call's)."""
    _dense_join_operand(from_dev, "the from-vectors")
    if to_dev is not None:
        _dense_join_operand(to_dev, "the to-vectors")
    to_h = None if to_dev is None else to_dev.h
    row_ptr, hits, n, work = _join_call(
        from_dev.n, capacity, (np.int32, np.float32), DENSE_JOIN_COUNTERS, counters,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_dense_join(ctx.h, from_dev.h, to_h, float(min_similarity), cap, ptr, *hit, total, wk))
    return (row_ptr,) + hits + ({"pairs": n, **(work or {})},)


def dense_components(ctx, dev, min_similarity, counters=False):
    """K14: the connected components of "cosine >= min_similarity" over the rows of `dev` (the pairs of dense_join's self-join,
    united on the device, never stored) -- (label int32[n], pairs, components): label[i] is the smallest position in i's
    component, pairs the number of hits (dense_join's total), components the number of components, singletons included.
    counters=True appends a dict of DENSE_JOIN_COUNTERS."""
    _dense_join_operand(dev, "the vectors")
    return _components_call(dev.n, DENSE_JOIN_COUNTERS, counters, lambda label, pairs, components, wk: ctx.lib.pfz_dense_components(
        ctx.h, dev.h, float(min_similarity), label, pairs, components, wk))


# ---- K23: all pairs of binary codes within a Hamming distance, and their components ------------------------------------

HAMMING_JOIN_COUNTERS = ("tiles", "hit_waves")      # pfz_hamming_join's out_counters, in order


def _hamming_join_operand(dev, what):
    if dev.dtype != BINARY:
        raise ValueError(f"{what} are {dev.dtype} vectors: the Hamming threshold kernels take binary operands only "
                         "(DeviceDense.upload_bits)")


def hamming_max_distance(dim_bits, min_similarity):
    """The largest h in [0, dim_bits] for which the score of two codes that differ in h bits --
    float32(dim_bits - 2 h) / float32(dim_bits), what dense_topn reports for normalised bit handles -- is >= min_similarity as
    float64 (equal is kept); -1 if there is none.  The library evaluates the rule itself (no closed form).  Its own host
    function: no device is touched.  dim_bits in [1, 2**24), min_similarity a number in [0, 1]: ValueError otherwise."""
    if isinstance(dim_bits, bool) or not isinstance(dim_bits, (int, np.integer)) or not 1 <= int(dim_bits) < 1 << 24:
        raise ValueError(f"dim_bits must be an integer in [1, 2**24), not {dim_bits!r}")
    h = c_i64(0)
    check(load().pfz_hamming_max_distance(int(dim_bits), check_min_similarity(min_similarity), ctypes.byref(h)))
    return h.value


def hamming_similarity(dist, dim_bits):
    """The float32 scores of Hamming distances at dim_bits bits: (float32(d) - 2 dist) / float32(d), one IEEE division -- the bits
    of k5_hamming_panel's scores (d < 2**24: numerator and denominator are exact).  Pure numpy."""
    d = np.float32(dim_bits)
    return ((d - np.float32(2) * np.asarray(dist).astype(np.float32)) / d).astype(np.float32)


def hamming_join(ctx, from_dev, to_dev, max_distance, capacity=None, counters=False):
    """K23: every pair of rows of two bit handles of equal width that differ in at most max_distance bits, as CSR over the
    from-rows: (row_ptr int64[n + 1], to-index int32[hits] ascending within a row, distance int32[hits], counts).  to_dev None
    (or from_dev itself): the self-join, every unordered pair once as (i, j), i < j, only the tiles on or above the diagonal
    computed.  Exact: the comparison is made on the integer bit counts.  capacity and the ONE repeat as dense_join.  counts:
    {"pairs": hits}, with counters=True also HAMMING_JOIN_COUNTERS (the last call's)."""
    _hamming_join_operand(from_dev, "the from-codes")
    if to_dev is not None:
        _hamming_join_operand(to_dev, "the to-codes")
    to_h = None if to_dev is None else to_dev.h
    row_ptr, hits, n, work = _join_call(
        from_dev.n, capacity, (np.int32, np.int32), HAMMING_JOIN_COUNTERS, counters,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_hamming_join(ctx.h, from_dev.h, to_h, int(max_distance), cap, ptr, *hit, total, wk))
    return (row_ptr,) + hits + ({"pairs": n, **(work or {})},)


def hamming_components(ctx, dev, max_distance, counters=False):
    """K23: the connected components of "at most max_distance differing bits" over the rows of the bit handle `dev` (the pairs of
    hamming_join's self-join, united on the device, never stored) -- (label int32[n], pairs, components) as dense_components.
    counters=True appends a dict of HAMMING_JOIN_COUNTERS."""
    _hamming_join_operand(dev, "the codes")
    return _components_call(dev.n, HAMMING_JOIN_COUNTERS, counters, lambda label, pairs, components, wk: ctx.lib.pfz_hamming_components(
        ctx.h, dev.h, int(max_distance), label, pairs, components, wk))


# ---- K24: the same two results through a block index, for small distances ------------------------------------------------

HAMMING_INDEX_COUNTERS = ("blocks", "min_block_bits", "checks", "items", "route")      # the indexed entries' out_counters, in order
HAMMING_INDEX_BLOCKS, HAMMING_INDEX_AUTO = 1, 2      # PFZ_HAMMING_INDEX_*


def hamming_index_plan(dim_bits, max_distance):
    """The block index of codes of dim_bits bits at max_distance (csrc/k24_core.h): {"blocks": m = max_distance + 1,
    "min_block_bits", "max_block_bits", "ratio": R, the measured cost of one indexed check in tile pairs (auto runs the index iff
    checks * R <= all pairs)}.  The library's own host function: no device is touched.  ValueError: dim_bits outside [1, 2**24) or
    max_distance outside [0, dim_bits]; PfzUnsupported: no index -- more blocks than bits, or more than 256 (the message says)."""
    if isinstance(dim_bits, bool) or not isinstance(dim_bits, (int, np.integer)) or not 1 <= int(dim_bits) < 1 << 24:
        raise ValueError(f"dim_bits must be an integer in [1, 2**24), not {dim_bits!r}")
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, np.integer)) or not 0 <= int(max_distance) <= int(dim_bits):
        raise ValueError(f"max_distance must be an integer in [0, {dim_bits}], not {max_distance!r}")
    out = np.zeros(4, np.int64)
    check(load().pfz_hamming_index_plan(int(dim_bits), int(max_distance), _ptr(out)))
    return dict(zip(("blocks", "min_block_bits", "max_block_bits", "ratio"), out.tolist()))


def hamming_join_indexed(ctx, from_dev, to_dev, max_distance, auto=False, capacity=None, counters=False):
    """K24: hamming_join's result, bit for bit, through the block index -- only pairs that share the bits of one of
    max_distance + 1 blocks have their distance computed.  auto=False: the index runs, or PfzUnsupported names the limit that
    keeps it from running (hamming_index_plan; 2**24 rows); auto=True: the index runs iff it is cheaper by the library's measured
    rule, otherwise K23's tiles run inside the call.  Returns what hamming_join returns; counts: {"pairs": hits}, with
    counters=True also HAMMING_INDEX_COUNTERS (the last call's; "route": 1 = the index, 0 = the tiles)."""
    _hamming_join_operand(from_dev, "the from-codes")
    if to_dev is not None:
        _hamming_join_operand(to_dev, "the to-codes")
    to_h = None if to_dev is None else to_dev.h
    mode = HAMMING_INDEX_AUTO if auto else HAMMING_INDEX_BLOCKS
    row_ptr, hits, n, work = _join_call(
        from_dev.n, capacity, (np.int32, np.int32), HAMMING_INDEX_COUNTERS, counters,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_hamming_join_indexed(ctx.h, from_dev.h, to_h, int(max_distance), mode, cap, ptr, *hit,
                                                                          total, wk))
    return (row_ptr,) + hits + ({"pairs": n, **(work or {})},)


def hamming_components_indexed(ctx, dev, max_distance, auto=False, counters=False):
    """K24: hamming_components' result through the block index -- (label int32[n], pairs, components); auto as
    hamming_join_indexed.  counters=True appends a dict of HAMMING_INDEX_COUNTERS."""
    _hamming_join_operand(dev, "the codes")
    mode = HAMMING_INDEX_AUTO if auto else HAMMING_INDEX_BLOCKS
    return _components_call(dev.n, HAMMING_INDEX_COUNTERS, counters, lambda label, pairs, components, wk:
                            ctx.lib.pfz_hamming_components_indexed(ctx.h, dev.h, int(max_distance), mode, label, pairs, components, wk))


# ---- K25: SimHash fingerprints of a resident string list, as a bit handle -------------------------------------------------

SIMHASH_MIN_BITS, SIMHASH_MAX_BITS, SIMHASH_MAX_GRAM = 64, 1024, 8      # kK25MinBits, kK25MaxBits, kK25MaxGram of csrc/k25_core.h


def check_simhash_bits(bits):
    """bits as an int: a multiple of 64 in [64, 1024] (ValueError otherwise)"""
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not SIMHASH_MIN_BITS <= int(bits) <= SIMHASH_MAX_BITS \
            or int(bits) % 64:
        raise ValueError(f"bits must be a multiple of 64 in [{SIMHASH_MIN_BITS}, {SIMHASH_MAX_BITS}], not {bits!r}")
    return int(bits)


def check_simhash_grams(n_gram_range):
    """(lo, hi) as ints with 1 <= lo <= hi <= 8 (ValueError otherwise)"""
    try:
        lo, hi = n_gram_range
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (lo, hi)) and 1 <= lo <= hi <= SIMHASH_MAX_GRAM
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"n_gram_range must be (lo, hi) with 1 <= lo <= hi <= {SIMHASH_MAX_GRAM}, not {n_gram_range!r}")
    return int(lo), int(hi)


def simhash(ctx, dev_strings, params, bits, want_bytes=False):
    """K25: the SimHash fingerprints of a resident string list (csrc/k25_core.h is the rule; `params` a TfidfParams: TFIDF's
    analyzer) -> (DeviceDense, row, windows[, bytes]).  The handle holds the strings that have a window, in list order, as a bit
    operand (dtype "binary", dim = bits, normalize=True: what DeviceDense.upload_bits makes of such rows) for hamming_join /
    hamming_components / their indexed forms / dense_topn.  row int32[n]: a string's row in the handle, -1 = no window; windows
    int32[n]; want_bytes: uint8[n, bits / 8], every string's fingerprint (zeros where it has no window), np.packbits order."""
    bits = check_simhash_bits(bits)
    check_simhash_grams((params.ngram_lo, params.ngram_hi))
    if params.clean and dev_strings.char_width != 1:
        raise ValueError("clean on 4-byte code units: strings with code points > 0xFF are cleaned on the host")
    n = dev_strings.n
    row, windows = np.empty(n, np.int32), np.empty(n, np.int32)
    out = np.empty((n, bits // 8), np.uint8) if want_bytes else None
    h = c_vp()
    check(ctx.lib.pfz_simhash(ctx.h, dev_strings.h, ctypes.byref(params), bits, ctypes.byref(h), _ptr(row), _ptr(windows),
                              None if out is None else _ptr(out)))
    m = DeviceDense(ctx, h)
    m.n, m.dim, m.normalize, m.dtype = int((row >= 0).sum()), bits, True, BINARY
    return (m, row, windows, out) if want_bytes else (m, row, windows)


# ---- K22: the same two entries searched on the 16-bit matrix cores, scored exactly on the fp32 vectors -------------------

DENSE_JOIN16_COUNTERS = ("tiles", "hit_corners", "candidates")      # pfz_dense_join16's out_counters, in order


def dense_search_margin(dtype, ld):
    """eps of K22's search for `dtype` ("float16" / "bfloat16") and the padded width ld: how far the float32 score of two search
    copies may lie below the exact cosine -- 2 asin(u + 2^-24 + sqrt(ld) 2^-25) + (ld + 8) 2^-23, u = 2^-11 / 2^-8 (the header
    derives the first term and names the assumption behind the second).  The library's own host function: no device is touched."""
    if dtype not in ("float16", "bfloat16"):
        raise ValueError(f"the search types are 'float16' and 'bfloat16', got {dtype!r}")
    eps = c_f64(0.0)
    check(load().pfz_dense_search_margin(DENSE_DTYPES[dtype], int(ld), ctypes.byref(eps)))
    return eps.value


def dense_search_threshold32(t, eps):
    """The largest float32 <= t - eps: what K22's search compares the 16-bit scores with.  Pure numpy."""
    d = np.float64(t) - np.float64(eps)
    r = np.float32(d)                              # (to nearest: at most one step above d)
    return np.nextafter(r, np.float32(-np.inf)) if np.float64(r) > d else r


def _search16_operand(dev, what):
    if dev.dtype not in ("float16", "bfloat16") or not dev.normalize:
        raise ValueError(f"{what} are {dev.dtype} vectors uploaded with normalize={dev.normalize}: the 16-bit search takes "
                         "float16 / bfloat16 operands made with normalize=True (DeviceDense.derive16)")


def dense_join16(ctx, from16, to16, from_exact, to_exact, min_similarity, capacity=None, counters=False, cand_capacity=None):
    """K22: dense_join's result -- (row_ptr, to-index, similarity float32, counts) -- found on the 16-bit matrix cores.  from16 /
    to16: the search copies (DeviceDense.derive16) of the fp32 handles from_exact / to_exact; to16 and to_exact None: the
    self-join.  Every pair whose exact score -- dense_rescore's float32: a float64 sum rounded once -- is >= min_similarity;
    similarity is that score.  cand_capacity: the candidate keys the library's buffer has room for (None: it chooses); a search
    that finds more is repeated once with room for all.  capacity as dense_join, on the final hits.  counts: {"pairs": hits,
    "candidates": ...}, with counters=True all of DENSE_JOIN16_COUNTERS (the tiles and corners of both searches when it was
    repeated).  from_exact None: the plain 16-bit join -- the similarity is dense_topn's float32 on the 16-bit handles, bit for
    bit, and there is no second stage."""
    _search16_operand(from16, "the from-vectors")
    if to16 is not None:
        _search16_operand(to16, "the to-vectors")
    for dev, what in ((from_exact, "the exact from-vectors"), (to_exact, "the exact to-vectors")):
        if dev is not None:
            _dense_join_operand(dev, what)
    h = [None if d is None else d.h for d in (to16, from_exact, to_exact)]
    row_ptr, hits, n, work = _join_call(
        from16.n, capacity, (np.int32, np.float32), DENSE_JOIN16_COUNTERS, True,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_dense_join16(ctx.h, from16.h, h[0], h[1], h[2], float(min_similarity), cap,
                                                                  int(cand_capacity or 0), ptr, *hit, total, wk))
    return (row_ptr,) + hits + ({"pairs": n, **(work if counters else {"candidates": work["candidates"]})},)


def dense_components16(ctx, dev16, dev_exact, min_similarity, counters=False, cand_capacity=None):
    """K22: dense_components' result -- (label int32[n], pairs, components) -- over the pairs of dense_join16's self-join: the
    candidates of the 16-bit search, scored exactly and united where they hit; none is stored, but the candidate keys are:
    device memory is O(candidates).  counters=True appends a dict of DENSE_JOIN16_COUNTERS."""
    _search16_operand(dev16, "the vectors")
    _dense_join_operand(dev_exact, "the exact vectors")
    return _components_call(dev16.n, DENSE_JOIN16_COUNTERS, counters, lambda label, pairs, components, wk: ctx.lib.pfz_dense_components16(
        ctx.h, dev16.h, dev_exact.h, float(min_similarity), int(cand_capacity or 0), label, pairs, components, wk))


# ---- K18: the threshold join of K7's scorers and its components ---------------------------------------------------------

FUZZ_JOIN_COUNTERS = ("bounded", "scored", "steps")      # pfz_fuzz_join's out_counters, in order


def fuzz_join(ctx, from_dev, to_dev, scorer, score_cutoff, capacity=None, counters=False):
    """K18: every pair whose `scorer` score -- fuzz_extract_one's float64 on rapidfuzz's 0..100 scale, bit for bit -- is
    >= score_cutoff (float64 against float64: equal is a hit), as CSR over the from-rows: (row_ptr int64[n + 1], to-index
    int32[hits] ascending within a row, score float64[hits]).  scorer: a name of FUZZ_SCORERS.  to_dev None (or from_dev itself):
    the self-join, every pair i < j once as row i, to-index j.  capacity: the hits the first call's buffers have room for (None:
    a modest guess, four per from-string); when the exact total the call returns exceeds it the call is repeated ONCE with room
    for that total, never more often.  counters=True appends a dict of FUZZ_JOIN_COUNTERS (the last call's)."""
    to_h = None if to_dev is None else to_dev.h
    row_ptr, hits, _, work = _join_call(
        from_dev.n, capacity, (np.int32, np.float64), FUZZ_JOIN_COUNTERS, counters,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_fuzz_join(ctx.h, from_dev.h, to_h, FUZZ_SCORERS[scorer], float(score_cutoff), cap, ptr,
                                                               *hit, total, wk))
    return (row_ptr,) + hits + ((work,) if counters else ())


def fuzz_components(ctx, dev, scorer, score_cutoff, counters=False):
    """K18: the connected components of "score >= score_cutoff" over the list `dev` (the pairs of fuzz_join's self-join, united
    on the device, never stored) -- (label int32[n], pairs, components): label[i] is the smallest position in i's component,
    pairs the number of hits (fuzz_join's total), components the number of components, singletons included.  counters=True
    appends a dict of FUZZ_JOIN_COUNTERS."""
    return _components_call(dev.n, FUZZ_JOIN_COUNTERS, counters, lambda label, pairs, components, wk: ctx.lib.pfz_fuzz_components(
        ctx.h, dev.h, FUZZ_SCORERS[scorer], float(score_cutoff), label, pairs, components, wk))


def fuzz_topn(ctx, from_dev, to_dev, scorer, ntop, skip_idx=None, score_cutoff=0.0, begin=0, end=None, counters=False):
    """K19: the ntop best choices of from-rows [begin, end) under the K7 scorer `scorer` (a name of FUZZ_SCORERS) --
    rapidfuzz.process.extract(..., limit=ntop, score_cutoff=score_cutoff): (index int32[n, ntop], score float64[n, ntop]) in the
    order (score descending, to-index ascending) over the choices not left out (skip_idx: fuzz_extract_one's codes) whose score --
    fuzz_extract_one's float64 on the 0..100 scale, bit for bit -- is >= score_cutoff (equal is kept); -1 / 0.0 beyond the choices a
    row has.  Column 0 at score_cutoff 0 is fuzz_extract_one's answer.  ntop <= 64 (PfzUnsupported beyond).  counters=True
    appends a dict of FUZZ_JOIN_COUNTERS."""
    end = from_dev.n if end is None else end
    n = end - begin
    idx = np.empty((n, max(int(ntop), 0)), np.int32)           # (ntop < 1 is the library's to refuse)
    score = np.empty((n, max(int(ntop), 0)), np.float64)
    skip_idx = _skip_array(skip_idx, from_dev.n)
    work = np.zeros(len(FUZZ_JOIN_COUNTERS), np.uint64) if counters else None
    check(ctx.lib.pfz_fuzz_topn(ctx.h, from_dev.h, to_dev.h, FUZZ_SCORERS[scorer], _ptr(skip_idx), int(begin), int(end), int(ntop),
                                float(score_cutoff), _ptr(idx), _ptr(score), _ptr(work)))
    return (idx, score, dict(zip(FUZZ_JOIN_COUNTERS, (int(w) for w in work)))) if counters else (idx, score)


# ---- K20: the threshold join of K8's scorers and its components ----------------------------------------------------------

JARO_JOIN_COUNTERS = ("pairs_in_window", "pairs_alive_after_sweep1", "pairs_scored", "steps")      # pfz_jaro_join's out_counters, in order


def jaro_join(ctx, from_dev, to_dev, scorer, min_similarity, capacity=None, counters=False):
    """K20: every pair whose `scorer` score (a name of JARO_SCORERS) -- jaro_matrix's float64, bit for bit -- is >= min_similarity
    (float64 against float64: equal is a hit), as CSR over the from-rows: (row_ptr int64[n + 1], to-index int32[hits] ascending
    within a row, score float64[hits]).  to_dev None (or from_dev itself): the self-join, every unordered pair once as (i, j),
    i < j.  capacity and the ONE repeat as in lev_join; counters=True appends a dict of JARO_JOIN_COUNTERS (the last call's)."""
    to_h = None if to_dev is None else to_dev.h
    row_ptr, hits, _, work = _join_call(
        from_dev.n, capacity, (np.int32, np.float64), JARO_JOIN_COUNTERS, counters,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_jaro_join(ctx.h, from_dev.h, to_h, JARO_SCORERS[scorer], float(min_similarity), cap, ptr,
                                                               *hit, total, wk))
    return (row_ptr,) + hits + ((work,) if counters else ())


def jaro_components(ctx, dev, scorer, min_similarity, counters=False):
    """K20: the connected components of "score >= min_similarity" over the list `dev` (the pairs of jaro_join's self-join, united
    on the device, never stored) -- (label int32[n], pairs, components): label[i] is the smallest position in i's component,
    pairs the number of hits (jaro_join's total), components the number of components, singletons included.  counters=True
    appends a dict of JARO_JOIN_COUNTERS."""
    return _components_call(dev.n, JARO_JOIN_COUNTERS, counters, lambda label, pairs, components, wk: ctx.lib.pfz_jaro_components(
        ctx.h, dev.h, JARO_SCORERS[scorer], float(min_similarity), label, pairs, components, wk))


# ---- K21: the n best choices under K8's scorers ----------------------------------------------------------------------------

JARO_TOPN_COUNTERS = ("pairs_walked", "pairs_alive_after_sweep1", "pairs_scored", "steps")      # pfz_jaro_topn's out_counters, in order


def jaro_topn(ctx, from_dev, to_dev, scorer, ntop, skip_idx=None, score_cutoff=0.0, begin=0, end=None, counters=False):
    """K21: the ntop best choices of from-rows [begin, end) under the K8 scorer `scorer` (a name of JARO_SCORERS) --
    rapidfuzz.process.extract(..., limit=ntop, score_cutoff=score_cutoff): (index int32[n, ntop], score float64[n, ntop]) in the
    order (score descending, to-index ascending) over the choices not left out (skip_idx: jaro_argmax's codes) whose score --
    jaro_matrix's float64 on the 0..1 scale, bit for bit -- is >= score_cutoff (equal is kept); -1 / 0.0 beyond the choices a row
    has.  Column 0 at score_cutoff 0 is jaro_argmax's answer.  ntop <= 64 (PfzUnsupported beyond).  counters=True appends a dict
    of JARO_TOPN_COUNTERS."""
    end = from_dev.n if end is None else end
    n = end - begin
    idx = np.empty((n, max(int(ntop), 0)), np.int32)           # (ntop < 1 is the library's to refuse)
    score = np.empty((n, max(int(ntop), 0)), np.float64)
    skip_idx = _skip_array(skip_idx, from_dev.n)
    work = np.zeros(len(JARO_TOPN_COUNTERS), np.uint64) if counters else None
    check(ctx.lib.pfz_jaro_topn(ctx.h, from_dev.h, to_dev.h, JARO_SCORERS[scorer], _ptr(skip_idx), int(begin), int(end), int(ntop),
                                float(score_cutoff), _ptr(idx), _ptr(score), _ptr(work)))
    return (idx, score, dict(zip(JARO_TOPN_COUNTERS, (int(w) for w in work)))) if counters else (idx, score)


# ---- K15: the sparse-cosine threshold join and its components --------------------------------------------------------

SPARSE_JOIN_COUNTERS = ("visits", "skipped", "hit_steps")      # pfz_cossim_join's out_counters, in order


def check_min_similarity(min_similarity):
    """a join's threshold: a real number in [0, 1] (ValueError otherwise; NaN compares false) -> float"""
    if (isinstance(min_similarity, bool) or not isinstance(min_similarity, (int, float, np.integer, np.floating))
            or not 0.0 <= float(min_similarity) <= 1.0):
        raise ValueError(f"min_similarity must be a number in [0, 1], not {min_similarity!r}")
    return float(min_similarity)


def sparse_join(ctx, index, from_dev, min_similarity, self_join=False, capacity=None, counters=False):
    """K15: every pair (row of the DeviceCSR from_dev, row of the DeviceIndex index) whose sparse cosine -- cossim_topn's float32,
    bit for bit -- is >= min_similarity (as float64: equal is a hit; a pair without a common column never is), as CSR over the
    from-rows: (row_ptr int64[n + 1], to-index int32[hits] ascending within a row, similarity float32[hits], counts).
    self_join: from_dev is the matrix the index was built from, and every unordered pair comes once as (i, j), i < j.  capacity:
    the hits the first call's buffers have room for (None: a modest guess, four per from-row); when the exact total the call
    returns exceeds it the call is repeated ONCE with room for that total, never more often.  counts: {"pairs": hits}, with
    counters=True also SPARSE_JOIN_COUNTERS (the last call's)."""
    t = check_min_similarity(min_similarity)
    row_ptr, hits, n, work = _join_call(
        from_dev.n_rows, capacity, (np.int32, np.float32), SPARSE_JOIN_COUNTERS, counters,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_cossim_join(ctx.h, index.h, from_dev.h, int(bool(self_join)), t, cap, ptr, *hit, total,
                                                                 wk))
    return (row_ptr,) + hits + ({"pairs": n, **(work or {})},)


def sparse_components(ctx, index, dev, min_similarity, counters=False):
    """K15: the connected components of "sparse cosine >= min_similarity" over the rows of `dev`, the matrix `index` was built
    from (the pairs of sparse_join's self-join, united on the device, never stored) -- (label int32[n], pairs, components):
    label[i] is the smallest position in i's component, pairs the number of hits (sparse_join's total), components the number
    of components, singletons included.  counters=True appends a dict of SPARSE_JOIN_COUNTERS."""
    t = check_min_similarity(min_similarity)
    return _components_call(dev.n_rows, SPARSE_JOIN_COUNTERS, counters, lambda label, pairs, components, wk: ctx.lib.pfz_cossim_components(
        ctx.h, index.h, dev.h, t, label, pairs, components, wk))


# ---- K17: a sparse-cosine threshold join left on the device, and K16 over its keys -----------------------------------

PAIR_SLICE = 64                        # kPairSlice of csrc/k17_core.h: partners per work item of the key entries
PAIR_KEYS_COUNTERS = ("candidates", "scored", "pairs", "items")      # pfz_pairs_join_keys' out_counters, in order


class DevicePairs(_Handle):
    """A threshold join's pairs in HBM (pfz_pairs): n sorted keys row << 32 | col with their float32 scores, over n_from x n_to
    positions; self_join: one list, every unordered pair once with row < col."""
    _free = "pfz_pairs_free"

    def __init__(self, ctx, h):
        super().__init__(ctx, h)
        n, n_from, n_to, self_join = c_i64(0), c_i64(0), c_i64(0), c_i32(0)
        check(ctx.lib.pfz_pairs_count(h, ctypes.byref(n)))
        check(ctx.lib.pfz_pairs_shape(h, ctypes.byref(n_from), ctypes.byref(n_to), ctypes.byref(self_join)))
        self.n, self.n_from, self.n_to, self.self_join = n.value, n_from.value, n_to.value, bool(self_join.value)

    def download(self):
        """(row_ptr int64[n_from + 1], to-index int32[n], similarity float32[n]): sparse_join's first three, byte for byte"""
        row_ptr = np.empty(self.n_from + 1, np.int64)
        idx, sim = np.empty(self.n, np.int32), np.empty(self.n, np.float32)
        check(self.ctx.lib.pfz_pairs_download(self.ctx.h, self.h, _ptr(row_ptr), _ptr(idx), _ptr(sim)))
        return row_ptr, idx, sim


def sparse_join_dev(ctx, index, from_dev, min_similarity, self_join=False, capacity_hint=None, counters=False):
    """K15 with its result left on the device: the pairs sparse_join(ctx, index, from_dev, min_similarity, self_join) reports, as
    a DevicePairs.  capacity_hint: the hits the first launch has room for (None: the library's default, max(4096, 4 per
    from-row)); a larger total costs exactly one repeat inside the call.  counters=True: (pairs, dict of SPARSE_JOIN_COUNTERS)."""
    t = check_min_similarity(min_similarity)
    hint = 0 if capacity_hint is None else int(capacity_hint)
    if hint < 0:
        raise ValueError(f"capacity_hint must be >= 0, not {capacity_hint!r}")
    work = np.zeros(3, np.int64) if counters else None
    h = c_vp()
    check(ctx.lib.pfz_cossim_join_dev(ctx.h, index.h, from_dev.h, int(bool(self_join)), t, hint, ctypes.byref(h), _ptr(work)))
    pairs = DevicePairs(ctx, h)
    return (pairs, dict(zip(SPARSE_JOIN_COUNTERS, work.tolist()))) if counters else pairs


def pairs_join_keys(ctx, from_dev, to_dev, pairs, scorer, min_similarity, capacity=None, counters=False):
    """K17: pairs_join with the DevicePairs `pairs` in place of the table -- the candidate pairs are exactly its keys (a self-join's:
    to_dev None or from_dev itself, every pair once with row < col, the lower position the from-string).  Score, hit rule, CSR,
    capacity and the ONE repeat as pairs_join.  counters=True appends a dict of PAIR_KEYS_COUNTERS: the keys, the distinct pairs
    scored (== the keys), the hits, the (row, slice) work items of at most PAIR_SLICE partners the kernels were dealt."""
    t = check_min_similarity(min_similarity)
    sid = PAIR_JOIN_SCORERS[scorer] if isinstance(scorer, str) else int(scorer)
    to_h = None if to_dev is None else to_dev.h
    row_ptr, hits, _, work = _join_call(
        from_dev.n, capacity, (np.int32, np.float64), PAIR_KEYS_COUNTERS, counters,
        lambda cap, ptr, hit, total, wk: ctx.lib.pfz_pairs_join_keys(ctx.h, from_dev.h, to_h, pairs.h, sid, t, cap, ptr, *hit, total, wk))
    return (row_ptr,) + hits + ((work,) if counters else ())


def pairs_components_keys(ctx, dev, pairs, scorer, min_similarity, counters=False):
    """K17: pairs_components with the self-join DevicePairs `pairs` in place of the table -- (label int32[n], pairs, components).
    counters=True appends a dict of PAIR_KEYS_COUNTERS."""
    t = check_min_similarity(min_similarity)
    sid = PAIR_JOIN_SCORERS[scorer] if isinstance(scorer, str) else int(scorer)
    return _components_call(dev.n, PAIR_KEYS_COUNTERS, counters, lambda label, pairs_out, components, wk: ctx.lib.pfz_pairs_components_keys(
        ctx.h, dev.h, pairs.h, sid, t, label, pairs_out, components, wk))


# ---- exact rescoring of a 16-bit / int8 top-n (k5_rescore_topn) ------------------------------------------------------

RESCORE_MAX_CANDIDATES = 1024          # candidates per from-row pfz_dense_rescore_topn ranks in one pass


def check_rescore_multiplier(value):
    """The oversampling factor of a rescored search: None (no rescoring) or an int >= 1.  The coarse search on the 16-bit /
    int8 operands keeps top_n x value candidates per row, which are then scored against the float32 vectors.  bool, floats,
    0 and negative values raise ValueError."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError(f"rescore_multiplier must be None or an int >= 1, got {value!r}")
    return int(value)


def rescore_candidates(ntop, multiplier, n_to, exclude_diag=False):
    """Candidates per row of a rescored search: min(ntop x multiplier, the to-rows there are -- one less in a self-match),
    at least ntop.  More than RESCORE_MAX_CANDIDATES raise ValueError."""
    multiplier = check_rescore_multiplier(multiplier)
    if multiplier is None:
        raise ValueError("a rescored search needs a rescore_multiplier (an int >= 1)")
    m = max(int(ntop), min(int(ntop) * multiplier, int(n_to) - (1 if exclude_diag else 0)))
    if m > RESCORE_MAX_CANDIDATES:
        raise ValueError(f"top_n={int(ntop)} with rescore_multiplier={multiplier} asks for {m} candidates per row; the "
                         f"rescoring kernel takes at most {RESCORE_MAX_CANDIDATES}")
    return m


def dense_rescore(ctx, from_exact, to_exact, candidates, ntop, lower_bound, out=None):
    """Enqueue pfz_dense_rescore_topn: the columns in the idx half of the DeviceTopN `candidates` (-1: none), scored against
    the float32 operands in float64 and rounded once; the ntop best with a score > max(lower_bound, 0) by (score descending,
    column ascending).  Returns the (device-resident) DeviceTopN."""
    if out is None:
        out = DeviceTopN.alloc(ctx, from_exact.n, ntop)
    check(ctx.lib.pfz_dense_rescore_topn(ctx.h, from_exact.h, to_exact.h, candidates.h, int(ntop), float(lower_bound), out.h))
    return out


MIXED_RESCORE_TO = ("int8", BINARY)     # the to-operands pfz_dense_rescore_topn_mixed scores float32 from-vectors against


def dense_rescore_mixed(ctx, from_exact, to_coarse, candidates, ntop, lower_bound, out=None):
    """Enqueue pfz_dense_rescore_topn_mixed: dense_rescore with the float32 from-operand against an int8 or 1-bit to-operand
    itself (k5_mixed_rescore) -- the cosine (normalize=False: the dot product) of the float vector and the int8 vector, or of
    the float vector and the +-1 vector the bits stand for; float64 sums, rounded once.  No float32 to-side is needed.
    Returns the (device-resident) DeviceTopN."""
    if out is None:
        out = DeviceTopN.alloc(ctx, from_exact.n, ntop)
    check(ctx.lib.pfz_dense_rescore_topn_mixed(ctx.h, from_exact.h, to_coarse.h, candidates.h, int(ntop), float(lower_bound), out.h))
    return out


def dense_topn_rescored(ctx, from_coarse, to_coarse, from_exact, to_exact, ntop, lower_bound, multiplier, exclude_diag=False,
                        diag_offset=0, out=None, candidates=None):
    """K5 on the 16-bit / int8 / 1-bit operands for rescore_candidates(ntop, multiplier, ...) candidates per row -- with lower bound
    0: the user's bound belongs to the exact score, not to the rounded one --, then dense_rescore of those candidates against
    the float32 operands of the same vectors with the user's bound.  The scores are the fp32 path's; the columns are the
    fp32 top-n wherever that lies within the candidates.  `candidates`: a DeviceTopN of that many columns to reuse.
    A `to_exact` of dtype "int8" or "binary" -- to_coarse itself, or an int8 handle beside a 1-bit to_coarse -- is scored by
    dense_rescore_mixed instead: from_exact stays float32, the scores are those of the float from-vectors and the QUANTISED
    to-vectors, and the columns are the fp32 top-n only as far as that to-side ranks them so."""
    m = rescore_candidates(ntop, multiplier, to_coarse.n, exclude_diag)          # (raises before anything is enqueued)
    if (from_coarse.n, to_coarse.n, from_coarse.dim) != (from_exact.n, to_exact.n, from_exact.dim):
        raise ValueError(f"the coarse operands {(from_coarse.n, to_coarse.n, from_coarse.dim)} and the exact ones "
                         f"{(from_exact.n, to_exact.n, from_exact.dim)} are not the same vectors")
    if candidates is None:
        candidates = DeviceTopN.alloc(ctx, from_coarse.n, m)
    elif candidates.ntop != m:
        raise ValueError(f"the candidate buffer has {candidates.ntop} columns, this search needs {m}")
    dense_topn(ctx, from_coarse, to_coarse, m, 0.0, exclude_diag, diag_offset, out=candidates)
    rescore = dense_rescore_mixed if getattr(to_exact, "dtype", None) in MIXED_RESCORE_TO else dense_rescore
    return rescore(ctx, from_exact, to_exact, candidates, ntop, lower_bound, out=out)


RESCORE_COARSE = ("int8", "float16", "bfloat16", BINARY)


# (coarse, rescore_to) of a search whose to-side is never float32: equal forms share one handle
MIXED_RESCORE_PAIRS = (("int8", "int8"), (BINARY, BINARY), (BINARY, "int8"))


def check_rescore_to(value):
    """`rescore_to` of the doors above the C ABI: None (rescoring reads the float32 to-side) or "int8" / "binary" / "ubinary":
    the float32 from-vectors are rescored against the to-side in that form and no float32 to-side is kept.  Returns None, "int8"
    or BINARY ("ubinary" is the same device form); anything else raises ValueError."""
    if value is None:
        return None
    if isinstance(value, str) and (value == "int8" or value in BINARY_FORMS):
        return BINARY if value in BINARY_FORMS else value
    raise ValueError(f'rescore_to must be None, "int8" or one of {BINARY_FORMS}, got {value!r}')


def check_mixed_pair(coarse, rescore_to):
    """ValueError unless (coarse operand type, checked rescore_to) is one of MIXED_RESCORE_PAIRS."""
    if (coarse, rescore_to) not in MIXED_RESCORE_PAIRS:
        raise ValueError(f"rescore_to={rescore_to!r} cannot follow a {coarse} search: the pairs are "
                         + ", ".join(f"{c} -> {r}" for c, r in MIXED_RESCORE_PAIRS))


def dense_rescored_topn_host(ctx, from_vec, to_vec, ntop, lower_bound, coarse, multiplier, exclude_diag=False, normalize=True,
                             rescore_to=None):
    """One-shot dense_topn_rescored on float arrays: both are uploaded twice, as `coarse` ("int8", "float16", "bfloat16", or
    "binary": sign bits packed on the device, a Hamming search) operands and as float32 ones; (idx, val) host arrays out.
    rescore_to "int8" / "binary" (MIXED_RESCORE_PAIRS: int8 after int8, binary or int8 after binary): the to-side goes up as
    `coarse` and in that form -- once when the two are equal -- and never as float32; the float32 from-vectors are scored against
    it (dense_rescore_mixed).  to_vec is then a float array, or an array already in the `rescore_to` form, which must also be
    `coarse`: np.int8 for "int8", packed np.uint8 / np.int8 rows for "binary"."""
    if not isinstance(coarse, str) or coarse not in RESCORE_COARSE:
        raise ValueError(f"coarse must be one of {RESCORE_COARSE}, got {coarse!r}")
    check_rescore_multiplier(multiplier)
    rescore_to = check_rescore_to(rescore_to)
    same = to_vec is from_vec
    from_vec, to_vec = np.asarray(from_vec), np.asarray(to_vec)
    given = False          # to_vec is already in the rescore_to form
    if rescore_to is not None:
        check_mixed_pair(coarse, rescore_to)
        given = to_vec.ndim == 2 and to_vec.dtype in ((np.int8,) if rescore_to == "int8" else (np.uint8, np.int8))
        if given and coarse != rescore_to:
            raise ValueError(f"a {to_vec.dtype} to-side is given in the {rescore_to} form: the search needs coarse={rescore_to!r}, "
                             f"got {coarse!r} (pass float vectors to have both forms made on the device)")
    for v in (from_vec,) if given else (from_vec, to_vec):
        if v.ndim != 2 or v.dtype.kind != "f" or v.dtype.itemsize < 4:
            raise ValueError(f"a rescored search takes 2-D float32 / float64 arrays, got {v.dtype} of shape {v.shape}")
    width = 8 * to_vec.shape[1] if given and rescore_to == BINARY else to_vec.shape[1]
    if from_vec.shape[1] != width:
        raise ValueError(f"dense cosine needs two 2-D arrays with equal width, got {from_vec.shape} and {(to_vec.shape[0], width)}"
                         + (BITS_WIDTH_HINT if given and rescore_to == BINARY else ""))
    rescore_candidates(ntop, multiplier, to_vec.shape[0], exclude_diag)          # (raises before anything is uploaded)
    return _dense_topn_host(ctx, from_vec, from_vec if same else to_vec, ntop, lower_bound, exclude_diag, normalize, coarse, multiplier,
                            rescore_to)


def pr_curve(ctx, sims, thresholds):
    """K6: (count of sims >= p_k int64[k], sum of those sims float64[k]) for ascending thresholds p_k."""
    sims = np.ascontiguousarray(sims, np.float64)
    thresholds = np.ascontiguousarray(thresholds, np.float64)
    count = np.empty(len(thresholds), np.int64)
    ssum = np.empty(len(thresholds), np.float64)
    check(ctx.lib.pfz_pr_curve_host(ctx.h, _ptr(sims) if len(sims) else None, len(sims), _ptr(thresholds),
                                    len(thresholds), _ptr(count), _ptr(ssum)))
    return count, ssum


def linkage_top1(ctx, result, min_similarity):
    """K6: (cluster int32[n], key int32[n], info) of the reference's single_linkage on a self-match top-1 result."""
    cluster = np.empty(result.n_rows, np.int32)
    key = np.empty(result.n_rows, np.int32)
    info = np.zeros(3, np.int32)
    check(ctx.lib.pfz_linkage_top1(ctx.h, result.h, float(min_similarity), _ptr(cluster), _ptr(key), _ptr(info)))
    return cluster, key, {"first_row": int(info[0]), "rounds": int(info[1]), "clusters": int(info[2])}


# ---- multi-GPU (one process per GPU, RCCL) -------------------------------------------

class _LocalGroup:
    def __init__(self, h):
        self.h = h

    def __del__(self):
        try:
            if self.h:
                load().pfz_comm_group_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Comm(_Handle):
    """RCCL communicator bound to a Context.  Bootstrap: rank 0 creates the 128-byte
    unique id, the launcher broadcasts it (torch.distributed / MPI / file)."""
    _free = "pfz_comm_destroy"

    @staticmethod
    def unique_id():
        buf = (ctypes.c_uint8 * 128)()
        check(load().pfz_comm_unique_id(ctypes.cast(buf, c_vp)))
        return bytes(buf)

    @classmethod
    def init(cls, ctx, uid, rank, world):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        h = c_vp()
        check(ctx.lib.pfz_comm_init(ctx.h, ctypes.cast(buf, c_vp), int(rank), int(world), ctypes.byref(h)))
        c = cls(ctx, h)
        c.rank, c.world = int(rank), int(world)
        return c

    @classmethod
    def local_group(cls, contexts):
        """One communicator per context, all in THIS process (contexts on different GPUs or on the same one):
        host rendezvous + device-to-device copies instead of RCCL.  Each rank must be driven by its own host
        thread (the collectives block until every rank has arrived)."""
        world = len(contexts)
        g = c_vp()
        check(load().pfz_comm_group_create(world, ctypes.byref(g)))
        group = _LocalGroup(g)
        comms = []
        for rank, ctx in enumerate(contexts):
            h = c_vp()
            check(ctx.lib.pfz_comm_init_local(ctx.h, g, rank, ctypes.byref(h)))
            c = cls(ctx, h)
            c.rank, c.world, c._group = rank, world, group     # keeps the group alive
            comms.append(c)
        return comms

    @classmethod
    def from_torch_distributed(cls, ctx, dist):
        """Bootstrap through an initialised torch.distributed process group (rendezvous only)."""
        rank, world = dist.get_rank(), dist.get_world_size()
        box = [cls.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        return cls.init(ctx, box[0], rank, world)

    def barrier(self):
        check(self.ctx.lib.pfz_comm_barrier(self.h))

    def merge_to_shards(self, local, to_offset, out=None):
        """All-gather the ranks' per-to-shard candidates and keep, on every rank, the global top-n."""
        if out is None:
            out = DeviceTopN.alloc(self.ctx, local.n_rows, local.ntop)
        check(self.ctx.lib.pfz_comm_merge_to_shards(self.h, local.h, int(to_offset), out.h))
        return out

    def symmetric_ok(self, index, csr, ntop):
        """COLLECTIVE (every rank calls it): do all ranks agree that this self-match takes K3's symmetric form, and has every rank
        the session buffers for it?  (pfz_comm_symmetric_ok)"""
        yes = c_i32(0)
        check(self.ctx.lib.pfz_comm_symmetric_ok(self.h, index.h, csr.h, int(ntop), ctypes.byref(yes)))
        return bool(yes.value)

    def cossim_topn_symmetric(self, index, csr, ntop, lower_bound, out=None):
        """the self-match of the whole (replicated) list, cut over the ranks in K3's symmetric form: the FULL result on every rank"""
        if out is None:
            out = DeviceTopN.alloc(self.ctx, csr.n_rows, ntop)
        check(self.ctx.lib.pfz_comm_cossim_topn_symmetric(self.h, index.h, csr.h, int(ntop), float(lower_bound), out.h))
        return out

    def allgather_topn(self, local, out=None):
        if out is None:
            out = DeviceTopN.alloc(self.ctx, local.n_rows * self.world, local.ntop)
        check(self.ctx.lib.pfz_comm_allgather_topn(self.h, local.h, out.h))
        return out


def rccl_versions():
    """{'header': NCCL_VERSION_CODE the library was compiled against, 'runtime': ncclGetVersion() of the librccl this process
    resolved, 'path': that library's file (from /proc/self/maps)}"""
    lib = load()
    h, r = c_i32(0), c_i32(0)
    check(lib.pfz_rccl_versions(ctypes.byref(h), ctypes.byref(r)))
    path = None
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "librccl" in line:
                    path = line.split()[-1]
                    break
    except OSError:
        pass
    return {"header": h.value, "runtime": r.value, "path": path}


def tfidf_fit_sharded(ctx, comm, params, replicated, local_shard):
    h = c_vp()
    rc = ctx.lib.pfz_tfidf_fit_sharded(ctx.h, comm.h, ctypes.byref(params),
                                       replicated.h if replicated is not None else None,
                                       local_shard.h if local_shard is not None else None, ctypes.byref(h))
    if rc == -1 and b"empty vocabulary" in ctx.lib.pfz_last_error():
        raise ValueError("empty vocabulary; perhaps the documents only contain stop words")
    check(rc)
    v = DeviceTfidf(ctx, h)
    v.params = params
    return v
