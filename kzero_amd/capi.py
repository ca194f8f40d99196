"""ctypes binding of the C ABI in include/kz_hip.h (libkzhip.so).

This is exactly what a foreign host binds; the Rust equivalent is shown in INTEGRATION.md.  There is no fallback:
if the library is missing or a call fails, this module raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KZ_LIB_PATH") or os.path.join(_HERE, "libkzhip.so")

KZ_DTYPE_F32 = 0
KZ_DTYPE_F16 = 1
KZ_DTYPE_F32_SPLIT16 = 2
KZ_DTYPE_BF16 = 3  # f32 tensors, the tower in bf16 (f32 range at the f16 rate, 8 significant bits)
KZ_DTYPE_INT8 = 4  # f16 tensors, the tower's block convolutions on the i8 matrix cores: a calibrated model only (Model.quantize_int8)
KZ_DTYPE_INT8_ANY = 8  # dtype 5's plan wherever it has one; elsewhere (Go 19x19, 13x13, 9x9 at 256, other widths up to 512) "board_conv_i8", one int8 launch per layer; 6 and 7 stay unknown
KZ_DTYPE_INT8_HEADS = 5  # dtype 4's tower with the conv policy heads, the scalar head and the decode inside its launch where it can carry them; elsewhere dtype 4's plan
KZ_ENGINE_SLOTS = 4
# per-board status bits (kz_engine_wait_decoded_status / kz_engine_eval_packed_decoded_status)
KZ_BOARD_OK = 0
KZ_BOARD_BAD_DECODE = 1
KZ_BOARD_NONFINITE = 2
KZ_BOARD_FELL_BACK = 4

POLICY_KINDS = {0: "ataxx_conv", 1: "conv", 2: "attention", 3: "dense"}


class KzError(RuntimeError):
    pass


class PathPlan(C.Structure):
    _fields_ = [("tower_path", C.c_char * 48), ("launches_per_batch", C.c_int32), ("reserved", C.c_int32 * 3)]


class ModelInfo(C.Structure):
    _fields_ = [
        ("input_channels", C.c_int32), ("board_h", C.c_int32), ("board_w", C.c_int32),
        ("input_scalar_channels", C.c_int32), ("input_bool_channels", C.c_int32), ("policy_len", C.c_int32),
        ("tower_depth", C.c_int32), ("tower_channels", C.c_int32), ("policy_kind", C.c_int32),
        ("bits_bytes", C.c_int32), ("param_count", C.c_int64), ("flops_per_eval", C.c_double),
    ]


class AuditStats(C.Structure):
    """kz_audit_stats: what the shadow audit has accumulated (kz_engine_audit_stats)."""
    _fields_ = [
        ("batches", C.c_int64), ("boards", C.c_int64), ("moves", C.c_int64), ("skipped", C.c_int64),
        ("max_abs_value", C.c_float * 5), ("max_abs_prob", C.c_float),
        ("sum_sq_value", C.c_double * 5), ("sum_sq_prob", C.c_double),
    ]


class AuditResult:
    """The eight fields of kz_audit_stats as Python numbers (the per-column ones as float32 / float64 arrays of 5: value, win,
    draw, loss, moves_left), and the root mean squares derived from them."""

    def __init__(self, raw: AuditStats):
        self.batches, self.boards, self.moves, self.skipped = int(raw.batches), int(raw.boards), int(raw.moves), int(raw.skipped)
        self.max_abs_value = np.array(raw.max_abs_value[:], np.float32)
        self.max_abs_prob = np.float32(raw.max_abs_prob)
        self.sum_sq_value = np.array(raw.sum_sq_value[:], np.float64)
        self.sum_sq_prob = float(raw.sum_sq_prob)

    @property
    def rms_prob(self) -> float:
        return float(np.sqrt(self.sum_sq_prob / self.moves)) if self.moves else 0.0

    @property
    def rms_value(self) -> np.ndarray:
        return np.sqrt(self.sum_sq_value / self.boards) if self.boards else np.zeros(5)

    def __repr__(self):
        return (f"AuditResult(batches={self.batches}, boards={self.boards}, moves={self.moves}, skipped={self.skipped}, "
                f"max_abs_value={self.max_abs_value.tolist()}, max_abs_prob={float(self.max_abs_prob)}, "
                f"rms_value={self.rms_value.tolist()}, rms_prob={self.rms_prob})")


class SiteError(C.Structure):
    """kz_site_error (include/kz_hip.h): one range site of kz_model_error_profile, 48 bytes."""
    _fields_ = [("max_abs_err", C.c_double), ("sum_sq_err", C.c_double), ("sum_sq_ref", C.c_double), ("max_abs_ref", C.c_double),
                ("count", C.c_uint64), ("nonfinite", C.c_uint64)]


# the same record as a numpy dtype, with the site's name in front (Model.error_profile)
SITE_ERROR_DTYPE = np.dtype([("max_abs_err", np.float64), ("sum_sq_err", np.float64), ("sum_sq_ref", np.float64),
                             ("max_abs_ref", np.float64), ("count", np.uint64), ("nonfinite", np.uint64)])
assert C.sizeof(SiteError) == SITE_ERROR_DTYPE.itemsize == 48


class Int8SiteError(C.Structure):
    """kz_int8_site_error (include/kz_hip.h): one range site of kz_model_int8_error_profile, 120 bytes."""
    _fields_ = [("image", SiteError), ("stream", SiteError), ("at_clamp", C.c_uint64), ("ref_beyond", C.c_uint64),
                ("exponent", C.c_int32), ("reserved", C.c_int32)]


# the same record as a numpy dtype (Model.int8_error_profile puts the site's name in front)
INT8_SITE_ERROR_DTYPE = np.dtype([("image", SITE_ERROR_DTYPE), ("stream", SITE_ERROR_DTYPE), ("at_clamp", np.uint64),
                                  ("ref_beyond", np.uint64), ("exponent", np.int32), ("reserved", np.int32)])
assert C.sizeof(Int8SiteError) == INT8_SITE_ERROR_DTYPE.itemsize == 120


# name -> (restype, argtypes); every symbol include/kz_hip.h declares
SIGNATURES = {
    "kz_last_error": (C.c_char_p, []),
    "kz_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "kz_device_pci_bus_id": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    "kz_model_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "kz_model_load_memory": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "kz_model_load_onnx": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "kz_model_load_onnx_memory": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "kz_model_free": (None, [C.c_void_p]),
    "kz_model_get_info": (C.c_int, [C.c_void_p, C.POINTER(ModelInfo)]),
    "kz_engine_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "kz_engine_destroy": (None, [C.c_void_p]),
    "kz_model_supports_dtype": (C.c_int, [C.c_void_p, C.c_int]),
    "kz_model_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "kz_model_launch_geometry": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kz_model_stream_shift": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "kz_model_quantize_int8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "kz_model_int8_site_exponents": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kz_model_range_sites": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "kz_model_range_site_name": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]),
    "kz_model_range_profile": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "kz_model_range_profile_fast": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p]),
    "kz_model_range_profile_fast_path": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "kz_model_range_histogram": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "kz_model_range_histogram_fast": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "kz_model_tower_taps_path": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "kz_model_tower_taps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p]),
    "kz_model_error_profile": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                         C.c_void_p]),
    "kz_model_int8_taps_path": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "kz_model_int8_taps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p, C.c_void_p]),
    "kz_model_int8_error_profile": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                              C.c_void_p]),
    "kz_engine_max_batch": (C.c_int, [C.c_void_p]),
    "kz_engine_eval_dense": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "kz_engine_eval_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p]),
    "kz_engine_eval_packed_decoded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "kz_engine_submit_packed": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]),
    "kz_engine_wait": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "kz_engine_wait_view": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "kz_engine_submit_packed_decoded": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_void_p]),
    "kz_engine_wait_decoded": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "kz_engine_set_symmetries": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "kz_engine_eval_packed_decoded_sym": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kz_engine_submit_packed_decoded_sym": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "kz_engine_eval_packed_decoded_avg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "kz_engine_submit_packed_decoded_avg": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_void_p]),
    "kz_engine_wait_decoded_status": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_void_p)]),
    "kz_engine_eval_packed_decoded_status": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kz_engine_set_range_fallback": (C.c_int, [C.c_void_p, C.c_int]),
    "kz_engine_set_audit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "kz_engine_audit_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "kz_engine_enqueue_packed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_void_p]),
    "kz_engine_enqueue_dense_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "kz_engine_synchronize": (C.c_int, [C.c_void_p]),
    "kz_device_malloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]),
    "kz_device_free": (C.c_int, [C.c_int, C.c_void_p]),
    "kz_memcpy_h2d": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "kz_memcpy_d2h": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "kz_device_synchronize": (C.c_int, [C.c_int]),
    "kz_engine_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "kz_engine_kernel_time": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "kz_engine_tower_path": (C.c_char_p, [C.c_void_p]),
    "kz_engine_launch_geometry": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kz_engine_read_activation": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]),
}

_lib = None


def load():
    """Loads libkzhip.so.  Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise KzError(f"{LIB_PATH} is missing: build it with kzero_amd/csrc/build.sh "
                          f"(or __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            if "KZ_LIB_PATH" in os.environ and not hasattr(lib, name):
                continue  # (an older build named explicitly for a same-box A/B: its missing entry points fail when called)
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise KzError(load().kz_last_error().decode())


def device_count() -> int:
    n = C.c_int()
    check(load().kz_device_count(C.byref(n)))
    return n.value


def device_pci_bus_id(device: int) -> str:
    buf = C.create_string_buffer(64)
    check(load().kz_device_pci_bus_id(device, buf, len(buf)))
    return buf.value.decode()


F16_MAX = 65504.0


def shift_for(max_abs: float, headroom_bits: int = 2) -> int:
    """The k of kz_model_stream_shift for a stream whose shifted sites reach max_abs (include/kz_hip.h):
    k = max(0, ceil(log2(max_abs / 65504)) + headroom_bits).  Exact: frexp, no floating-point logarithm."""
    max_abs = float(max_abs)
    if not np.isfinite(max_abs) or max_abs < 0:
        raise KzError(f"shift_for: max_abs must be finite and non-negative, got {max_abs}")
    if max_abs == 0.0:  # (log2(0) = -inf)
        return 0
    mant, exp = np.frexp(max_abs / F16_MAX)  # max_abs / 65504 = mant * 2^exp, mant in [0.5, 1)
    ceil_log2 = int(exp) - 1 if mant == 0.5 else int(exp)
    return max(0, ceil_log2 + int(headroom_bits))


KZ_RANGE_BINS = 96  # include/kz_hip.h: bin 0 +-0, bin 95 inf / NaN, bin b in 1 .. 94 the binade E = b - 51 (the ends clamped)
SHIFT_REPORT_FIELDS = ("total", "zero", "nonfinite", "f16_over", "f16_top", "f16_subnormal", "f16_flushed", "split_lo_subnormal",
                       "clamped_low", "clamped_high")


def shift_report(hist: np.ndarray, k: int) -> dict:
    """What a stream shift of k does to the stored values a range histogram counted (Model.range_histogram; hist
    [n_sites, 96]): per site E' = E - k on the shifted sites and E' = E on the last one, and the counts — uint64 [n_sites] each —
      total, zero, nonfinite                  all elements; +-0; inf or NaN
      f16_over, f16_top                       E' >= 16: beyond f16; E' = 15: the binade that holds 65504 .. 65536
      f16_subnormal, f16_flushed              -25 <= E' <= -15; E' < -25: rounds to zero or to the smallest subnormal
      split_lo_subnormal                      E' <= -3: the lo half of a split16 pair is subnormal or gone
      clamped_low, clamped_high               the two end bins (E <= -50, E >= 43) as they are: for every k in [-24, 24] they lie
                                              in f16_flushed (and split_lo_subnormal) and in f16_over, so nothing is guessed
    Pure integer arithmetic: the library reports, the caller decides, as for shift_for."""
    hist = np.asarray(hist)
    if hist.ndim != 2 or hist.shape[1] != KZ_RANGE_BINS or hist.shape[0] < 1:
        raise KzError(f"shift_report: hist must be [n_sites, {KZ_RANGE_BINS}], got {hist.shape}")
    k = int(k)
    if not -24 <= k <= 24:
        raise KzError(f"shift_report: k = {k} out of range [-24, 24]")
    hist = hist.astype(np.uint64)
    n = hist.shape[0]
    out = {name: np.zeros(n, np.uint64) for name in SHIFT_REPORT_FIELDS}
    for site in range(n):
        row = [int(v) for v in hist[site]]
        shift = k if site < n - 1 else 0  # (the last site is behind the final BatchNorm: a shift does not move it)
        r = dict.fromkeys(SHIFT_REPORT_FIELDS, 0)
        r["total"], r["zero"], r["nonfinite"] = sum(row), row[0], row[KZ_RANGE_BINS - 1]
        r["clamped_low"], r["clamped_high"] = row[1], row[KZ_RANGE_BINS - 2]
        for b in range(1, KZ_RANGE_BINS - 1):
            e = b - 51 - shift  # (bin 1: at most this; bin 94: at least this — the classes below hold for both)
            r["f16_over"] += row[b] if e >= 16 else 0
            r["f16_top"] += row[b] if e == 15 else 0
            r["f16_subnormal"] += row[b] if -25 <= e <= -15 else 0
            r["f16_flushed"] += row[b] if e < -25 else 0
            r["split_lo_subnormal"] += row[b] if e <= -3 else 0
        for name in SHIFT_REPORT_FIELDS:
            out[name][site] = r[name]
    return out


class Model:
    """`Arc<Graph>`: immutable, shareable across engines, threads and devices."""

    def __init__(self, blob: bytes = None, path: str = None, onnx_scalar_channels: int = None):
        """blob/path: a KZMODEL1 container or an ONNX file; onnx_scalar_channels: for ONNX, how many input planes are
        broadcast scalars (the mapper's input_scalar_count) — needed for the packed-input entry points."""
        self._h = C.c_void_p()
        if onnx_scalar_channels is not None:
            if blob is not None:
                check(load().kz_model_load_onnx_memory(blob, len(blob), onnx_scalar_channels, C.byref(self._h)))
            else:
                check(load().kz_model_load_onnx(path.encode(), onnx_scalar_channels, C.byref(self._h)))
        elif blob is not None:
            check(load().kz_model_load_memory(blob, len(blob), C.byref(self._h)))
        else:
            check(load().kz_model_load(path.encode(), C.byref(self._h)))
        info = ModelInfo()
        check(load().kz_model_get_info(self._h, C.byref(info)))
        self.info = info

    def plan(self, max_batch: int, dtype: int):
        """(tower path, launches per batch) kz_engine_create would choose — host logic, no GPU needed."""
        out = PathPlan()
        check(load().kz_model_plan(self._h, max_batch, dtype, C.byref(out)))
        return out.tower_path.decode(), out.launches_per_batch

    def launch_geometry(self, max_batch: int, dtype: int, batch: int):
        """(workgroups, boards per workgroup) an engine of (max_batch, dtype) reports for `batch` — host logic, no GPU needed."""
        wgs, per = C.c_int(0), C.c_int(0)
        check(load().kz_model_launch_geometry(self._h, max_batch, dtype, batch, C.byref(wgs), C.byref(per)))
        return wgs.value, per.value

    def supports_dtype(self, dtype: int) -> bool:
        return load().kz_model_supports_dtype(self._h, dtype) == 1

    @classmethod
    def _adopt(cls, handle):
        self = cls.__new__(cls)
        self._h = handle
        self.info = ModelInfo()
        check(load().kz_model_get_info(self._h, C.byref(self.info)))
        return self

    def stream_shift(self, k: int) -> "Model":
        """The same function with a residual stream 2^-k times as large (kz_model_stream_shift): a new Model."""
        out = C.c_void_p()
        check(load().kz_model_stream_shift(self._h, int(k), C.byref(out)))
        return Model._adopt(out)

    def quantize_int8(self, site_max) -> "Model":
        """The same network with an int8 calibration beside it (kz_model_quantize_int8): a new Model, the only kind an engine of
        KZ_DTYPE_INT8 takes.  site_max: max |x| per range site, in range_sites' order (range_profile_fast's, times any headroom);
        the last entry is accepted and ignored."""
        site_max = np.ascontiguousarray(site_max, dtype=np.float32)
        out = C.c_void_p()
        check(load().kz_model_quantize_int8(self._h, site_max.ctypes.data, int(site_max.size), C.byref(out)))
        return Model._adopt(out)

    def int8_site_exponents(self) -> np.ndarray:
        """e_s = ceil(log2(site_max[s] / 127)) of every quantised range site — all but the last — of a calibrated model
        (kz_model_int8_site_exponents): int32 [n_sites - 1]."""
        exp = np.zeros(max(2 * self.info.tower_depth, 1), np.int32)
        check(load().kz_model_int8_site_exponents(self._h, exp.ctypes.data))
        return exp[:2 * self.info.tower_depth]

    def range_sites(self):
        """The names of the range profile's sites, in order (kz_model_range_sites / kz_model_range_site_name)."""
        n = C.c_int()
        check(load().kz_model_range_sites(self._h, C.byref(n)))
        names = []
        for site in range(n.value):
            buf = C.create_string_buffer(32)
            check(load().kz_model_range_site_name(self._h, site, buf, len(buf)))
            names.append(buf.value.decode())
        return names

    def range_profile(self, device: int, bits: np.ndarray, scalars_in: np.ndarray):
        """max |x| of every stored tower tensor on these boards, in exact f32 on the GPU (kz_model_range_profile):
        (site_max float32 [n_sites], board_max float32 [batch] over the sites a shift moves)."""
        return self._range_profile("kz_model_range_profile", device, bits, scalars_in)

    def range_profile_fast(self, device: int, bits: np.ndarray, scalars_in: np.ndarray):
        """The same profile inside the one-launch exact-f32 tower where that kernel takes the network — tens of thousands of
        boards per second — and exactly range_profile elsewhere (kz_model_range_profile_fast)."""
        return self._range_profile("kz_model_range_profile_fast", device, bits, scalars_in)

    def range_profile_fast_path(self) -> str:
        """Where range_profile_fast runs: "tower_resident_f32" or "conv_igemm_f32" — host logic, no GPU needed."""
        buf = C.create_string_buffer(32)
        check(load().kz_model_range_profile_fast_path(self._h, buf, len(buf)))
        return buf.value.decode()

    def range_histogram(self, device: int, bits: np.ndarray, scalars_in: np.ndarray, fast: bool = True) -> np.ndarray:
        """How many stored values of every site lie in each binade on these boards, counted in exact f32 on the GPU: uint64
        [n_sites, 96], every row summing to batch * h * w * tower_channels (kz_model_range_histogram_fast: inside the one-launch
        tower where range_profile_fast_path says so; fast=False: kz_model_range_histogram, per layer).  shift_report reads it."""
        n = C.c_int()
        check(load().kz_model_range_sites(self._h, C.byref(n)))
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        hist = np.zeros((n.value, KZ_RANGE_BINS), np.uint64)
        entry = load().kz_model_range_histogram_fast if fast else load().kz_model_range_histogram
        check(entry(self._h, device, bits.ctypes.data, bits.shape[1] if bits.ndim == 2 else 0, scalars_in.ctypes.data,
                    bits.shape[0], hist.ctypes.data))
        return hist

    def tower_taps_path(self, max_batch: int, dtype: int) -> str:
        """The kernel a tap call runs: plan(max_batch, dtype)'s tower without "+heads" (kz_model_tower_taps_path) — host logic,
        no GPU needed; fails where the taps fail."""
        buf = C.create_string_buffer(64)
        check(load().kz_model_tower_taps_path(self._h, max_batch, dtype, buf, len(buf)))
        return buf.value.decode()

    def tower_taps(self, device: int, max_batch: int, dtype: int, bits: np.ndarray, scalars_in: np.ndarray, site_first: int = 0,
                   n_sites: int = None, out: np.ndarray = None) -> dict:
        """What the one-launch tower of an engine of (max_batch, dtype) stores at the range sites [site_first, site_first +
        n_sites) on these boards, as the kernel rounds it (kz_model_tower_taps): {site name: float32 [batch, C, H, W]}.
        out: a float32 array of [n_sites, batch, C, H, W] elements to fill instead of a new one (the dict's arrays are views)."""
        if n_sites is None:
            n_sites = len(self.range_sites()) - site_first
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        batch = bits.shape[0]
        shape = (max(n_sites, 0), batch, self.info.tower_channels, self.info.board_h, self.info.board_w)
        if out is None:
            out = np.zeros(shape, np.float32)
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.size < int(np.prod(shape)):
            raise KzError(f"tower_taps: out must be a C-contiguous float32 array of at least {int(np.prod(shape))} elements")
        check(load().kz_model_tower_taps(self._h, device, max_batch, dtype, bits.ctypes.data, bits.shape[1] if bits.ndim == 2 else 0,
                                         scalars_in.ctypes.data, batch, site_first, n_sites, out.ctypes.data))
        names = self.range_sites()
        view = out.reshape(-1)[:int(np.prod(shape))].reshape(shape)
        return {names[site_first + i]: view[i] for i in range(n_sites)}

    def error_profile(self, device: int, max_batch: int, dtype: int, bits: np.ndarray, scalars_in: np.ndarray) -> np.ndarray:
        """Per range site, how far that tower's stored tensors are from exact f32 on these boards, reduced on the GPU
        (kz_model_error_profile): a structured array [n_sites] with the fields site (the name), max_abs_err, sum_sq_err,
        sum_sq_ref, max_abs_ref, count, nonfinite.  rms error relative to the reference's rms: sqrt(sum_sq_err / sum_sq_ref)."""
        try:
            names = self.range_sites()
        except KzError:
            names = [""]  # (a network without range sites: the call below says so in its own name)
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        raw = np.zeros(len(names), SITE_ERROR_DTYPE)
        check(load().kz_model_error_profile(self._h, device, max_batch, dtype, bits.ctypes.data, bits.shape[1] if bits.ndim == 2 else 0,
                                            scalars_in.ctypes.data, bits.shape[0], raw.ctypes.data))
        out = np.zeros(len(names), np.dtype([("site", "U24")] + SITE_ERROR_DTYPE.descr))
        out["site"] = names
        for f in SITE_ERROR_DTYPE.names:
            out[f] = raw[f]
        return out

    def int8_taps_path(self, max_batch: int, dtype: int) -> str:
        """The kernel an int8 tap call runs, "tower_resident_i8" or "board_conv_i8", never with "+heads"
        (kz_model_int8_taps_path) — host logic, no GPU needed; fails where the int8 taps fail."""
        buf = C.create_string_buffer(64)
        check(load().kz_model_int8_taps_path(self._h, max_batch, dtype, buf, len(buf)))
        return buf.value.decode()

    def int8_taps(self, device: int, max_batch: int, dtype: int, bits: np.ndarray, scalars_in: np.ndarray, site_first: int = 0,
                  n_sites: int = None) -> tuple:
        """What the int8 tower of an engine of (max_batch, dtype) stores at the range sites [site_first, site_first + n_sites)
        on these boards (kz_model_int8_taps): ({site name: int8 [batch, C, H, W]}, {site name: float32 [batch, C, H, W]}) —
        the image's q (0 at the last site, which has none; -128 where no lane wrote) and the f16 stream value stored beside it
        (the tower output at the last site; NaN at a mid site, which has none)."""
        if n_sites is None:
            n_sites = len(self.range_sites()) - site_first
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        batch = bits.shape[0]
        shape = (max(n_sites, 0), batch, self.info.tower_channels, self.info.board_h, self.info.board_w)
        image, stream = np.zeros(shape, np.int8), np.zeros(shape, np.float32)
        check(load().kz_model_int8_taps(self._h, device, max_batch, dtype, bits.ctypes.data, bits.shape[1] if bits.ndim == 2 else 0,
                                        scalars_in.ctypes.data, batch, site_first, n_sites, image.ctypes.data, stream.ctypes.data))
        names = self.range_sites()
        return ({names[site_first + i]: image[i] for i in range(n_sites)}, {names[site_first + i]: stream[i] for i in range(n_sites)})

    def int8_error_profile(self, device: int, max_batch: int, dtype: int, bits: np.ndarray, scalars_in: np.ndarray) -> np.ndarray:
        """Per range site, how far that int8 tower's stored images (q * 2^e_s) and f16 stream values are from exact f32 on these
        boards, and how many elements sit at the clamp, reduced on the GPU (kz_model_int8_error_profile): a structured array
        [n_sites] with the fields site (the name), image and stream (error_profile's six fields each), at_clamp, ref_beyond,
        exponent, reserved."""
        try:
            names = self.range_sites()
        except KzError:
            names = [""]  # (a network without range sites: the call below says so in its own name)
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        raw = np.zeros(len(names), INT8_SITE_ERROR_DTYPE)
        check(load().kz_model_int8_error_profile(self._h, device, max_batch, dtype, bits.ctypes.data, bits.shape[1] if bits.ndim == 2 else 0,
                                                 scalars_in.ctypes.data, bits.shape[0], raw.ctypes.data))
        out = np.zeros(len(names), np.dtype([("site", "U24")] + INT8_SITE_ERROR_DTYPE.descr))
        out["site"] = names
        for f in INT8_SITE_ERROR_DTYPE.names:
            out[f] = raw[f]
        return out

    def _range_profile(self, entry: str, device: int, bits: np.ndarray, scalars_in: np.ndarray):
        n = C.c_int()
        check(load().kz_model_range_sites(self._h, C.byref(n)))
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        batch = bits.shape[0]
        site_max = np.zeros(n.value, np.float32)
        board_max = np.zeros(max(batch, 1), np.float32)
        check(getattr(load(), entry)(self._h, device, bits.ctypes.data, bits.shape[1] if bits.ndim == 2 else 0,
                                     scalars_in.ctypes.data, batch, site_max.ctypes.data, board_max.ctypes.data))
        return site_max, board_max[:batch]

    def close(self):
        if self._h:
            load().kz_model_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def calibrate_int8(model: Model, device: int, bits: np.ndarray, scalars_in: np.ndarray, headroom: float = 1.0) -> Model:
    """`model` calibrated for KZ_DTYPE_INT8 on these positions: range_profile_fast, then quantize_int8 with site_max x headroom.
    headroom 1 fits the profiled positions exactly; positions not yet seen can be larger, and what exceeds +-127 steps saturates."""
    site_max, _ = model.range_profile_fast(device, bits, scalars_in)
    return model.quantize_int8(site_max.astype(np.float64) * float(headroom))


def auto_stream_shift(model: Model, device: int, bits: np.ndarray, scalars_in: np.ndarray, headroom_bits: int = 2):
    """The shift `model` needs on these sampled positions (HipModel::auto_stream_shift of the C++ mirror): range_profile_fast,
    m = the largest board_max, k = shift_for(m, headroom_bits).  Returns (model.stream_shift(k) — or `model` itself for
    k == 0 —, k, m, boards).  No boards: k = 0 and boards = 0, nothing is measured.  m = +inf raises: a network that overflows
    f32 is not a shift's business."""
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    boards = int(bits.shape[0]) if bits.ndim == 2 else 0
    if boards == 0:
        return model, 0, 0.0, 0
    _, board_max = model.range_profile_fast(device, bits, scalars_in)
    m = float(board_max.max())
    if not np.isfinite(m):
        raise KzError(f"auto_stream_shift: the residual stream is not finite in exact f32 on the {boards} sampled boards: "
                      f"no shift brings such a network into range")
    k = shift_for(m, headroom_bits)
    return (model.stream_shift(k) if k else model), k, m, boards


class DeviceBuffer:
    def __init__(self, device: int, nbytes: int):
        self.device, self.nbytes = device, nbytes
        self.ptr = C.c_void_p()
        check(load().kz_device_malloc(device, nbytes, C.byref(self.ptr)))

    @classmethod
    def from_host(cls, device: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        buf = cls(device, arr.nbytes)
        if arr.nbytes:
            check(load().kz_memcpy_h2d(device, buf.ptr, arr.ctypes.data, arr.nbytes))
        return buf

    def to_host(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        if out.nbytes:
            check(load().kz_memcpy_d2h(self.device, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            load().kz_device_free(self.device, self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    """One per executor thread, like `CudaNetwork` (rust/kz-core/src/network/cudnn.rs:18-43)."""

    def __init__(self, model: Model, device: int, max_batch: int, dtype: int):
        self.model, self.device, self.dtype = model, device, dtype
        self._h = C.c_void_p()
        check(load().kz_engine_create(model._h, device, max_batch, dtype, C.byref(self._h)))
        self.max_batch = load().kz_engine_max_batch(self._h)

    @property
    def tower_path(self) -> str:
        return load().kz_engine_tower_path(self._h).decode()

    def launch_geometry(self, batch: int):
        """(workgroups per launch, boards per workgroup) of the path's dominant launch at `batch`."""
        wgs, per = C.c_int(), C.c_int()
        check(load().kz_engine_launch_geometry(self._h, batch, C.byref(wgs), C.byref(per)))
        return wgs.value, per.value

    def eval_dense(self, x: np.ndarray):
        info = self.model.info
        x = np.ascontiguousarray(x, dtype=np.float32)
        batch = x.shape[0]
        scalars = np.empty((batch, 5), np.float32)
        policy = np.empty((batch, info.policy_len), np.float32)
        check(load().kz_engine_eval_dense(self._h, x.ctypes.data, batch, scalars.ctypes.data, policy.ctypes.data))
        return scalars, policy

    def eval_packed(self, bits: np.ndarray, scalars_in: np.ndarray):
        info = self.model.info
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        batch = bits.shape[0]
        scalars = np.empty((batch, 5), np.float32)
        policy = np.empty((batch, info.policy_len), np.float32)
        stride = bits.shape[1] if bits.ndim == 2 else 0
        check(load().kz_engine_eval_packed(self._h, bits.ctypes.data, stride, scalars_in.ctypes.data, batch,
                                           scalars.ctypes.data, policy.ctypes.data))
        return scalars, policy

    def set_symmetries(self, square_src: np.ndarray, policy_map: np.ndarray):
        """The board symmetries as tables (kz_engine_set_symmetries): square_src [n_sym, h*w], policy_map [n_sym, policy_len]."""
        square_src = np.ascontiguousarray(square_src, dtype=np.int32)
        policy_map = np.ascontiguousarray(policy_map, dtype=np.int32)
        info = self.model.info
        if square_src.ndim != 2 or policy_map.ndim != 2 or square_src.shape[0] != policy_map.shape[0] or \
                square_src.shape[1] != info.board_h * info.board_w or policy_map.shape[1] != info.policy_len:
            raise KzError(f"set_symmetries: tables of shape {square_src.shape} and {policy_map.shape}, expected "
                          f"[n_sym, {info.board_h * info.board_w}] and [n_sym, {info.policy_len}]")
        check(load().kz_engine_set_symmetries(self._h, square_src.shape[0], square_src.ctypes.data, policy_map.ctypes.data))

    @staticmethod
    def _sym_ids(sym, batch: int) -> np.ndarray:
        sym = np.ascontiguousarray(sym, dtype=np.uint8)
        if sym.shape != (batch,):
            raise KzError(f"sym: one id per board expected ({batch}), got shape {sym.shape}")
        return sym

    def eval_packed_decoded(self, bits: np.ndarray, scalars_in: np.ndarray, move_lists, sym=None):
        """decode_output on the GPU: returns (values [batch,5], [probs per board]).  sym: one symmetry id per board
        (set_symmetries): the boards go through the network mapped, the probabilities come back for the listed moves."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        batch = bits.shape[0]
        offsets = np.zeros(batch + 1, np.int64)
        offsets[1:] = np.cumsum([len(m) for m in move_lists])
        idx = np.ascontiguousarray(np.concatenate([np.asarray(m, np.int32) for m in move_lists] + [np.zeros(0, np.int32)]),
                                   dtype=np.int32)
        values = np.empty((batch, 5), np.float32)
        probs = np.empty(max(len(idx), 1), np.float32)
        if sym is not None:
            sym = self._sym_ids(sym, batch)
            check(load().kz_engine_eval_packed_decoded_sym(self._h, bits.ctypes.data, bits.shape[1] if bits.ndim == 2 else 0,
                                                           scalars_in.ctypes.data, batch, sym.ctypes.data, offsets.ctypes.data,
                                                           idx.ctypes.data, values.ctypes.data, probs.ctypes.data))
            return values, [probs[offsets[i]:offsets[i + 1]].copy() for i in range(batch)]
        check(load().kz_engine_eval_packed_decoded(self._h, bits.ctypes.data, bits.shape[1] if bits.ndim == 2 else 0,
                                                   scalars_in.ctypes.data, batch, offsets.ctypes.data, idx.ctypes.data,
                                                   values.ctypes.data, probs.ctypes.data))
        return values, [probs[offsets[i]:offsets[i + 1]].copy() for i in range(batch)]

    def submit_packed(self, slot: int, bits: np.ndarray, scalars_in: np.ndarray):
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        check(load().kz_engine_submit_packed(self._h, slot, bits.ctypes.data, bits.shape[1], scalars_in.ctypes.data,
                                             bits.shape[0]))
        return bits.shape[0]

    def wait(self, slot: int, batch: int):
        scalars = np.empty((batch, 5), np.float32)
        policy = np.empty((batch, self.model.info.policy_len), np.float32)
        check(load().kz_engine_wait(self._h, slot, scalars.ctypes.data, policy.ctypes.data))
        return scalars, policy

    def submit_packed_decoded(self, slot: int, bits: np.ndarray, scalars_in: np.ndarray, move_lists, sym=None):
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        offsets = np.zeros(len(move_lists) + 1, np.int64)
        offsets[1:] = np.cumsum([len(m) for m in move_lists])
        idx = np.ascontiguousarray(np.concatenate([np.asarray(m, np.int32) for m in move_lists]) if offsets[-1] else
                                   np.zeros(0, np.int32))
        if sym is not None:
            sym = self._sym_ids(sym, bits.shape[0])
            check(load().kz_engine_submit_packed_decoded_sym(self._h, slot, bits.ctypes.data, bits.shape[1],
                                                             scalars_in.ctypes.data, bits.shape[0], sym.ctypes.data,
                                                             offsets.ctypes.data, idx.ctypes.data))
            return offsets
        check(load().kz_engine_submit_packed_decoded(self._h, slot, bits.ctypes.data, bits.shape[1],
                                                     scalars_in.ctypes.data, bits.shape[0], offsets.ctypes.data,
                                                     idx.ctypes.data))
        return offsets

    @staticmethod
    def _csr(move_lists):
        offsets = np.zeros(len(move_lists) + 1, np.int64)
        offsets[1:] = np.cumsum([len(m) for m in move_lists])
        idx = np.ascontiguousarray(np.concatenate([np.asarray(m, np.int32) for m in move_lists] + [np.zeros(0, np.int32)]),
                                   dtype=np.int32)
        return offsets, idx

    def eval_packed_decoded_avg(self, bits: np.ndarray, scalars_in: np.ndarray, move_lists):
        """Every board under every symmetry of set_symmetries, averaged on the GPU (kz_engine_eval_packed_decoded_avg): the
        original boards and move lists once per board in, (values [batch,5], [probs per board]) out; at most
        max_batch // n_sym boards."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        batch = bits.shape[0]
        offsets, idx = self._csr(move_lists)
        values = np.empty((batch, 5), np.float32)
        probs = np.empty(max(len(idx), 1), np.float32)
        check(load().kz_engine_eval_packed_decoded_avg(self._h, bits.ctypes.data, bits.shape[1] if bits.ndim == 2 else 0,
                                                       scalars_in.ctypes.data, batch, offsets.ctypes.data, idx.ctypes.data,
                                                       values.ctypes.data, probs.ctypes.data))
        return values, [probs[offsets[i]:offsets[i + 1]].copy() for i in range(batch)]

    def submit_packed_decoded_avg(self, slot: int, bits: np.ndarray, scalars_in: np.ndarray, move_lists):
        """The asynchronous half (kz_engine_submit_packed_decoded_avg); wait_decoded(slot, the returned offsets) waits."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        offsets, idx = self._csr(move_lists)
        check(load().kz_engine_submit_packed_decoded_avg(self._h, slot, bits.ctypes.data, bits.shape[1], scalars_in.ctypes.data,
                                                         bits.shape[0], offsets.ctypes.data, idx.ctypes.data))
        return offsets

    def submit_packed_decoded_avg_csr(self, slot: int, bits: np.ndarray, scalars_in: np.ndarray, offsets: np.ndarray, idx: np.ndarray):
        """The same with the CSR move lists already built: what a timed loop calls."""
        check(load().kz_engine_submit_packed_decoded_avg(self._h, slot, bits.ctypes.data, bits.shape[1], scalars_in.ctypes.data,
                                                         bits.shape[0], offsets.ctypes.data, idx.ctypes.data))

    def submit_packed_decoded_csr(self, slot: int, bits: np.ndarray, scalars_in: np.ndarray, offsets: np.ndarray, idx: np.ndarray,
                                  sym: np.ndarray = None):
        """The same with the CSR move lists already built (contiguous uint8 / float32 / int64 / int32 arrays; sym: uint8): what
        a timed loop calls."""
        if sym is not None:
            check(load().kz_engine_submit_packed_decoded_sym(self._h, slot, bits.ctypes.data, bits.shape[1], scalars_in.ctypes.data,
                                                             bits.shape[0], sym.ctypes.data, offsets.ctypes.data, idx.ctypes.data))
            return
        check(load().kz_engine_submit_packed_decoded(self._h, slot, bits.ctypes.data, bits.shape[1], scalars_in.ctypes.data,
                                                     bits.shape[0], offsets.ctypes.data, idx.ctypes.data))

    def wait_decoded_view(self, slot: int):
        """kz_engine_wait_decoded without copies: the two pointers into the slot's pinned staging."""
        pv, pp = C.c_void_p(), C.c_void_p()
        check(load().kz_engine_wait_decoded(self._h, slot, C.byref(pv), C.byref(pp)))
        return pv.value, pp.value

    def wait_decoded(self, slot: int, offsets: np.ndarray):
        """values [batch,5] and one probability array per board: copies of the slot's pinned staging."""
        pv, pp = C.c_void_p(), C.c_void_p()
        check(load().kz_engine_wait_decoded(self._h, slot, C.byref(pv), C.byref(pp)))
        batch, total = len(offsets) - 1, int(offsets[-1])
        values = np.ctypeslib.as_array(C.cast(pv, C.POINTER(C.c_float)), shape=(batch, 5)).copy() if batch else np.empty((0, 5), np.float32)
        probs = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_float)), shape=(total,)).copy() if total else np.zeros(0, np.float32)
        return values, [probs[offsets[i]:offsets[i + 1]] for i in range(batch)]

    def wait_decoded_status(self, slot: int, offsets: np.ndarray):
        """wait_decoded that does not fail for an error inside the batch (kz_engine_wait_decoded_status): values [batch,5],
        one probability array per board and status uint8 [batch] (KZ_BOARD_* bits), copies of the slot's staging."""
        pv, pp, ps = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(load().kz_engine_wait_decoded_status(self._h, slot, C.byref(pv), C.byref(pp), C.byref(ps)))
        batch, total = len(offsets) - 1, int(offsets[-1])
        values = np.ctypeslib.as_array(C.cast(pv, C.POINTER(C.c_float)), shape=(batch, 5)).copy() if batch else np.empty((0, 5), np.float32)
        probs = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_float)), shape=(total,)).copy() if total else np.zeros(0, np.float32)
        status = np.ctypeslib.as_array(C.cast(ps, C.POINTER(C.c_uint8)), shape=(batch,)).copy() if batch else np.zeros(0, np.uint8)
        return values, [probs[offsets[i]:offsets[i + 1]] for i in range(batch)], status

    def eval_packed_decoded_status(self, bits: np.ndarray, scalars_in: np.ndarray, move_lists, sym=None):
        """eval_packed_decoded with the per-board status instead of a failing call (kz_engine_eval_packed_decoded_status):
        returns (values [batch,5], [probs per board], status uint8 [batch])."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        scalars_in = np.ascontiguousarray(scalars_in, dtype=np.float32)
        batch = bits.shape[0]
        offsets, idx = self._csr(move_lists)
        values = np.empty((batch, 5), np.float32)
        probs = np.empty(max(len(idx), 1), np.float32)
        status = np.zeros(max(batch, 1), np.uint8)
        sym = self._sym_ids(sym, batch) if sym is not None else None
        check(load().kz_engine_eval_packed_decoded_status(self._h, bits.ctypes.data, bits.shape[1] if bits.ndim == 2 else 0,
                                                          scalars_in.ctypes.data, batch, sym.ctypes.data if sym is not None else None,
                                                          offsets.ctypes.data, idx.ctypes.data, values.ctypes.data, probs.ctypes.data,
                                                          status.ctypes.data))
        return values, [probs[offsets[i]:offsets[i + 1]].copy() for i in range(batch)], status[:batch]

    def set_range_fallback(self, dtype: int):
        """KZ_DTYPE_F32: the calls that return a batch re-evaluate its out-of-range boards in exact f32 inside the engine
        (kz_engine_set_range_fallback); -1: off (the default)."""
        check(load().kz_engine_set_range_fallback(self._h, dtype))

    def set_audit(self, dtype: int, period: int = 1, boards: int = 16):
        """KZ_DTYPE_F32 / KZ_DTYPE_F32_SPLIT16: the first `boards` boards of every `period`-th decoded submit also run on a
        sibling engine of that dtype and the deviation is accumulated (kz_engine_set_audit); -1: off (the default)."""
        check(load().kz_engine_set_audit(self._h, dtype, period, boards))

    def audit_stats(self, reset: bool = False) -> AuditResult:
        """What the audit has accumulated (kz_engine_audit_stats); reset: zero it afterwards."""
        raw = AuditStats()
        check(load().kz_engine_audit_stats(self._h, C.byref(raw), int(reset)))
        return AuditResult(raw)

    def wait_view(self, slot: int, batch: int):
        """Zero-copy wait: arrays over the slot's pinned staging, valid until the next submit on that slot."""
        ps, pp = C.c_void_p(), C.c_void_p()
        check(load().kz_engine_wait_view(self._h, slot, C.byref(ps), C.byref(pp)))
        if batch == 0:
            return np.empty((0, 5), np.float32), np.empty((0, self.model.info.policy_len), np.float32)
        plen = self.model.info.policy_len
        scalars = np.ctypeslib.as_array(C.cast(ps, C.POINTER(C.c_float)), shape=(batch, 5))
        policy = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_float)), shape=(batch, plen))
        return scalars, policy

    def enqueue_packed_device(self, d_bits: DeviceBuffer, stride: int, d_scalars: DeviceBuffer, batch: int,
                              d_scalars_out: DeviceBuffer, d_policy_out: DeviceBuffer):
        check(load().kz_engine_enqueue_packed_device(self._h, d_bits.ptr, stride, d_scalars.ptr, batch,
                                                     d_scalars_out.ptr, d_policy_out.ptr))

    def enqueue_dense_device(self, d_input: DeviceBuffer, batch: int, d_scalars_out: DeviceBuffer,
                             d_policy_out: DeviceBuffer):
        check(load().kz_engine_enqueue_dense_device(self._h, d_input.ptr, batch, d_scalars_out.ptr, d_policy_out.ptr))

    def synchronize(self):
        check(load().kz_engine_synchronize(self._h))

    def set_profiling(self, on: bool):
        check(load().kz_engine_set_profiling(self._h, int(on)))

    def kernel_time(self, prefix: str):
        total, n = C.c_double(), C.c_int64()
        check(load().kz_engine_kernel_time(self._h, prefix.encode(), C.byref(total), C.byref(n)))
        return total.value, n.value

    def read_activation(self, name: str, batch: int) -> np.ndarray:
        info = self.model.info
        out = np.empty((batch, info.tower_channels, info.board_h, info.board_w), np.float32)
        check(load().kz_engine_read_activation(self._h, name.encode(), batch, out.ctypes.data))
        return out

    def close(self):
        if self._h:
            load().kz_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
