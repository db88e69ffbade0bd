"""msm_amd — Python host binding of libmsm (MI355X Edwards-BLS12 MSM).

Mirrors the reference's public surface (src/submission/submission.ts:25-157):

    compute_msm(base_affine_points, scalars, window_size=None) -> (x, y)

with the same input shapes (BigIntPoint-like dicts / tuples, or U32ArrayPoint-like wire words),
the same output ({x, y} as ints, identity = (0, 1)), and the reference's helper entry points
(split_dynamic, point_add_affine, get_best_window_size).  All compute runs in libmsm's HIP
kernels; there is no CPU fallback: if the shared library or a gfx950 device is missing, calls
raise MsmError.
"""
from __future__ import annotations

import atexit
import ctypes
import os
from typing import Iterable, Optional, Sequence, Tuple, Union

import numpy as np

__all__ = [
    "MsmError", "MsmOpts", "load", "compute_msm", "compute_msm_wire", "compute_msm_device",
    "compute_msm_partial", "compute_msm_device_partial", "compute_msm_many_device", "compute_msm_many_device_partial",
    "compute_msm_shared_device", "compute_msm_many", "compute_msm_shared", "compute_msm_cpu", "MSM_FLAG_SERIAL",
    "combine_partials", "combine_partials_many", "point_add_affine",
    "split_dynamic", "get_best_window_size", "set_profiling", "last_profile", "device_count", "device_ordinals",
    "MSM_FLAG_DEVICES", "MSM_FLAG_WINDOWS", "MSM_FLAG_HALF_WINDOWS", "MSM_FLAG_SCALAR_BITS", "MSM_MAX_DEVICES",
    "window_count",
    "lib_path", "points_to_wire", "scalars_to_wire", "wire_to_int", "P", "Bases", "BasesInfo",
    "MsmOptsTyped", "MSM_FLAG_SCALAR_TYPE", "SCALAR_TYPES", "scalars_to_native",
    "MSM_FLAG_SCALAR_FIELD", "WIDE_TYPES", "FR_MODULUS", "scalars_to_wide",
    "FR_FORMS", "fr_combine", "fr_fold", "fr_mul", "fr_convert", "fr_powers", "fr_dot", "fr_to_ints",
    "fr_inverse", "fr_cumprod", "fr_cumsum", "fr_tensor", "MSM_FR_SCAN_SUM", "MSM_FR_SCAN_EXCLUSIVE",
]

P = 8444461749428370424248824938781546531375899335154063827935233455917409239041

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSM_AMD_LIB selects an alternative in-tree build (kernel A/B experiments); default libmsm.so
_LIB = os.environ.get("MSM_AMD_LIB") or os.path.join(_HERE, "_lib", "libmsm.so")


class MsmError(RuntimeError):
    def __init__(self, code: int, where: str = ""):
        self.code = code
        msg = _strerror(code)
        super().__init__(f"libmsm error {code} ({msg}){' in ' + where if where else ''}")


class MsmOpts(ctypes.Structure):
    """include/msm.h msm_opts: the original four fields, then the device list (read by libmsm only
    when flags has MSM_FLAG_DEVICES), the scalar width (MSM_FLAG_SCALAR_BITS), then the window range
    (MSM_FLAG_WINDOWS)."""
    _fields_ = [("window_bits", ctypes.c_uint32), ("run_length", ctypes.c_uint32),
                ("device", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("devices", ctypes.POINTER(ctypes.c_int32)), ("n_devices", ctypes.c_uint32),
                ("scalar_bits", ctypes.c_uint32), ("window_lo", ctypes.c_uint32), ("window_hi", ctypes.c_uint32)]


class MsmOptsTyped(MsmOpts):
    """include/msm.h msm_opts_typed: a msm_opts followed by scalar_type (MSM_SCALAR_*), read by libmsm
    only when flags has MSM_FLAG_SCALAR_TYPE, and scalar_field (MSM_FIELD_*), read only when flags has
    MSM_FLAG_SCALAR_FIELD -- the shorter MsmOpts keeps its 40 bytes."""
    _fields_ = [("scalar_type", ctypes.c_uint32), ("scalar_field", ctypes.c_uint32)]


class MsmProfile(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in (
        "prepare_points", "recode_count", "coarse_scan", "coarse_scatter", "fine_sort", "accumulate",
        "fixup", "bucket_reduce_1", "bucket_reduce_2", "readback", "device_total", "host_tail")] + [
        ("entries", ctypes.c_uint64), ("window_bits", ctypes.c_uint32), ("windows", ctypes.c_uint32),
        ("run_length", ctypes.c_uint32), ("chunk_len", ctypes.c_uint32),
        ("accumulate_sum", ctypes.c_double), ("device_total_sum", ctypes.c_double), ("profiled", ctypes.c_uint32),
        ("msms_per_launch", ctypes.c_uint32), ("accumulate_union_sum", ctypes.c_double)]

class BasesInfo(ctypes.Structure):
    """include/msm.h msm_bases_info_t."""
    _fields_ = [("n", ctypes.c_uint64), ("levels", ctypes.c_uint32), ("window_bits", ctypes.c_uint32),
                ("chunk_bits", ctypes.c_uint32), ("windows", ctypes.c_uint32), ("device", ctypes.c_int32),
                ("reserved", ctypes.c_uint32), ("bytes", ctypes.c_uint64)]


class FixedInfo(ctypes.Structure):
    """include/msm.h msm_fixed_info_t."""
    _fields_ = [("bases", ctypes.c_uint32), ("window_bits", ctypes.c_uint32), ("scalar_bits", ctypes.c_uint32),
                ("windows", ctypes.c_uint32), ("records", ctypes.c_uint64), ("bytes", ctypes.c_uint64),
                ("device", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class GuardHit(ctypes.Structure):
    """csrc/host_guard.h GuardHit: one finding of msm_test_guard_check."""
    _fields_ = [("buffer", ctypes.c_uint32), ("device", ctypes.c_int32), ("slot", ctypes.c_int32),
                ("side", ctypes.c_uint32), ("first", ctypes.c_int64), ("last", ctypes.c_int64),
                ("count", ctypes.c_uint64)]


class Subset(ctypes.Structure):
    """include/msm.h msm_subset_t."""
    _fields_ = [("first", ctypes.c_uint64), ("m", ctypes.c_uint64), ("indices", ctypes.c_void_p)]


class Combine(ctypes.Structure):
    """include/msm.h msm_combine_t."""
    _fields_ = [("b_bases", ctypes.c_void_p), ("a", Subset), ("b", Subset), ("a_scalars", ctypes.c_void_p),
                ("b_scalars", ctypes.c_void_p), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class FrCombine(ctypes.Structure):
    """include/msm.h msm_fr_combine_t."""
    _fields_ = [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("x", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("flags", ctypes.c_uint32), ("in_form", ctypes.c_uint32), ("out_form", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


MSM_FR_SUB = 1  # out_i = x_i a_i - y_i b_i (include/msm.h)
MSM_FR_X_BROADCAST = 2  # x holds one element, used for every i
MSM_FR_Y_BROADCAST = 4  # likewise y
MSM_FR_SCAN_SUM = 1  # msm_fr_scan*: the running sum instead of the running product
MSM_FR_SCAN_EXCLUSIVE = 2  # out_i over j < i instead of j <= i
FR_FORMS = {"wire": 0, "fr_mont": 1}  # MSM_FR_WIRE, MSM_FR_MONT: the names scalar_type uses
MSM_COMBINE_SUB = 1  # R_i = a_i A_i - b_i B_i (include/msm.h)
MSM_COMBINE_A_BROADCAST = 2  # a_scalars holds one scalar, used for every i
MSM_COMBINE_B_BROADCAST = 4  # likewise b_scalars
MSM_FLAG_SERIAL = 1  # pipelined entries: one launch in flight at a time
MSM_FLAG_DEVICES = 2  # msm_opts carries a device list (include/msm.h)
MSM_FLAG_WINDOWS = 4  # msm_opts carries a window range
MSM_FLAG_HALF_WINDOWS = 8  # with MSM_FLAG_WINDOWS: the range counts half windows
MSM_FLAG_SCALAR_BITS = 16  # msm_opts carries the scalars' width (narrow scalars, Bases.compute* only)
MSM_FLAG_SCALAR_TYPE = 32  # the options are a MsmOptsTyped: native integer scalars (Bases.compute* only)
MSM_FLAG_SCALAR_FIELD = 64  # MsmOptsTyped.scalar_field is set: wide native scalars (Bases.compute* only)
MSM_MAX_DEVICES = 16
# include/msm.h MSM_SCALAR_*: name -> (value, numpy dtype of the array, element bits e)
SCALAR_TYPES = {
    "bit": (1, np.dtype(np.uint8), 1),  # np.packbits(..., bitorder="little")
    "u8": (2, np.dtype(np.uint8), 8), "u16": (3, np.dtype(np.uint16), 16), "u32": (4, np.dtype(np.uint32), 32),
    "u64": (5, np.dtype(np.uint64), 64), "i8": (6, np.dtype(np.int8), 8), "i16": (7, np.dtype(np.int16), 16),
    "i32": (8, np.dtype(np.int32), 32), "i64": (9, np.dtype(np.int64), 64),
}
# include/msm.h MSM_FIELD_*: name -> (value, element bits e).  Little-endian elements of e / 8 bytes: 128-bit
# integers, 256-bit integers (arkworks BigInt<4>) and Fr of ark-ed-on-bls12-377 in Montgomery form.
WIDE_TYPES = {"u128": (1, 128), "i128": (2, 128), "u256": (3, 256), "fr_mont": (4, 256)}
# r, the order of the curve's prime subgroup: the modulus of the scalar field Fr (251 bits)
FR_MODULUS = 0x04aad957a68b2955982d1347970dec005293a3afc43c8afeb95aee9ac33fd9ff
MSM_STREAM_NULL = 1  # hip_stream value: order after the null (legacy default) stream


_lib: Optional[ctypes.CDLL] = None


def lib_path() -> str:
    return _LIB


def load() -> ctypes.CDLL:
    """Load libmsm.so (built in-tree by `make -C webgpu-msm_amd`).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise MsmError(-6, f"libmsm.so not built at {_LIB} (run __graft_entry__.build())")
    # One HIP runtime per process: torch ships its own libamdhip64 (soname libamdhip64.so.7) that
    # its libraries NEED by the unversioned name.  Loading torch first lets libmsm bind to that
    # same runtime by soname; loading libmsm first would pull /opt/rocm's copy and torch would
    # then initialise a second runtime that sees no devices.
    # (MSM_AMD_NO_TORCH=1 skips this: libmsm then runs on /opt/rocm's runtime, as the Node addon and
    # C callers do -- for comparing the two runtimes)
    if not os.environ.get("MSM_AMD_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = ctypes.CDLL(_LIB)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    vp = ctypes.c_void_p
    sz = ctypes.c_size_t
    optp = ctypes.POINTER(MsmOpts)
    sig = {
        "msm_init": ([], ctypes.c_int),
        "msm_shutdown": ([], None),
        "msm_device_count": ([], ctypes.c_int),
        "msm_device_ordinal": ([ctypes.c_int], ctypes.c_int),
        "msm_strerror": ([ctypes.c_int], ctypes.c_char_p),
        "msm_best_window": ([sz], ctypes.c_uint32),
        "msm_compute": ([vp, vp, sz, optp, u32p], ctypes.c_int),
        "msm_compute_partial": ([vp, vp, sz, optp, u32p], ctypes.c_int),
        "msm_compute_device": ([vp, vp, sz, optp, vp, u32p], ctypes.c_int),
        "msm_compute_device_partial": ([vp, vp, sz, optp, vp, u32p], ctypes.c_int),
        "msm_compute_batch_device": ([vp, vp, sz, sz, optp, vp, u32p], ctypes.c_int),
        "msm_compute_many_device": ([vp, vp, sz, sz, optp, vp, u32p], ctypes.c_int),
        "msm_compute_many_device_partial": ([vp, vp, sz, sz, optp, vp, u32p], ctypes.c_int),
        "msm_compute_shared_device": ([vp, vp, sz, sz, optp, vp, u32p], ctypes.c_int),
        "msm_compute_many": ([vp, vp, sz, sz, optp, u32p], ctypes.c_int),
        "msm_compute_shared": ([vp, vp, sz, sz, optp, u32p], ctypes.c_int),
        "msm_compute_cpu": ([vp, vp, sz, ctypes.c_uint32, ctypes.c_int, u32p], ctypes.c_int),
        "msm_compute_cocompute": ([vp, vp, sz, optp, ctypes.c_double, ctypes.c_int, u32p], ctypes.c_int),
        "msm_combine_partials": ([vp, sz, u32p], ctypes.c_int),
        "msm_combine_partials_many": ([vp, sz, sz, u32p], ctypes.c_int),
        "msm_point_add_affine": ([u32p, u32p, u32p], ctypes.c_int),
        "msm_split": ([ctypes.c_uint32, vp, sz, u32p], ctypes.c_int),
        "msm_split_windows": ([ctypes.c_uint32], ctypes.c_uint32),
        "msm_window_count": ([ctypes.c_uint32], ctypes.c_uint32),
        "msm_set_profiling": ([ctypes.c_int], ctypes.c_int),
        "msm_gen_points": ([u32p, ctypes.c_uint64, ctypes.c_uint64, sz, u32p], ctypes.c_int),
        "msm_gen_scalars": ([ctypes.c_uint64, sz, u32p], ctypes.c_int),
        "msm_last_profile": ([ctypes.POINTER(MsmProfile)], ctypes.c_int),
        "msm_bases_create": ([vp, sz, optp, ctypes.c_uint32, ctypes.POINTER(vp)], ctypes.c_int),
        "msm_bases_create_device": ([vp, sz, optp, ctypes.c_uint32, vp, ctypes.POINTER(vp)], ctypes.c_int),
        "msm_bases_create_compressed": ([vp, sz, ctypes.c_uint32, optp, ctypes.c_uint32, ctypes.POINTER(vp)], ctypes.c_int),
        "msm_bases_create_compressed_device": ([vp, sz, ctypes.c_uint32, optp, ctypes.c_uint32, vp, ctypes.POINTER(vp)],
                                               ctypes.c_int),
        "msm_decompress_points": ([vp, sz, ctypes.c_uint32, optp, vp], ctypes.c_int),
        "msm_decompress_points_device": ([vp, sz, ctypes.c_uint32, optp, vp, vp], ctypes.c_int),
        "msm_compress_points": ([vp, sz, ctypes.c_uint32, vp], ctypes.c_int),
        "msm_test_decompress_constants": ([u32p], ctypes.c_int),
        "msm_bases_destroy": ([vp], ctypes.c_int),
        "msm_bases_info": ([vp, ctypes.POINTER(BasesInfo)], ctypes.c_int),
        "msm_bases_compute": ([vp, vp, optp, u32p], ctypes.c_int),
        "msm_bases_compute_device": ([vp, vp, optp, vp, u32p], ctypes.c_int),
        "msm_bases_compute_many": ([vp, vp, sz, optp, u32p], ctypes.c_int),
        "msm_bases_compute_many_device": ([vp, vp, sz, optp, vp, u32p], ctypes.c_int),
        "msm_bases_compute_subset": ([vp, ctypes.POINTER(Subset), vp, optp, u32p], ctypes.c_int),
        "msm_bases_compute_subset_device": ([vp, ctypes.POINTER(Subset), vp, optp, vp, u32p], ctypes.c_int),
        "msm_bases_compute_subset_many": ([vp, ctypes.POINTER(Subset), vp, sz, optp, u32p], ctypes.c_int),
        "msm_bases_compute_subset_many_device": ([vp, ctypes.POINTER(Subset), vp, sz, optp, vp, u32p], ctypes.c_int),
        "msm_bases_scale": ([vp, ctypes.POINTER(Subset), vp, optp, vp], ctypes.c_int),
        "msm_bases_scale_device": ([vp, ctypes.POINTER(Subset), vp, optp, vp, vp], ctypes.c_int),
        "msm_bases_scale_create": ([vp, ctypes.POINTER(Subset), vp, optp, ctypes.c_uint32, ctypes.POINTER(vp)],
                                   ctypes.c_int),
        "msm_bases_scale_create_device": ([vp, ctypes.POINTER(Subset), vp, optp, ctypes.c_uint32, vp,
                                           ctypes.POINTER(vp)], ctypes.c_int),
        "msm_test_scale_digits": ([vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p], ctypes.c_int),
        "msm_bases_combine": ([vp, ctypes.POINTER(Combine), optp, vp], ctypes.c_int),
        "msm_bases_combine_device": ([vp, ctypes.POINTER(Combine), optp, vp, vp], ctypes.c_int),
        "msm_bases_combine_create": ([vp, ctypes.POINTER(Combine), optp, ctypes.c_uint32, ctypes.POINTER(vp)],
                                     ctypes.c_int),
        "msm_bases_combine_create_device": ([vp, ctypes.POINTER(Combine), optp, ctypes.c_uint32, vp,
                                             ctypes.POINTER(vp)], ctypes.c_int),
        "msm_test_combine_digits": ([vp, vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p], ctypes.c_int),
        "msm_fixed_create": ([vp, ctypes.POINTER(Subset), ctypes.c_uint32, ctypes.c_uint32, optp, ctypes.POINTER(vp)],
                             ctypes.c_int),
        "msm_fixed_create_vector": ([vp, ctypes.POINTER(Subset), ctypes.c_uint32, ctypes.c_uint32, optp,
                                     ctypes.POINTER(vp)], ctypes.c_int),
        "msm_test_vector_plan": ([ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                  u32p], ctypes.c_int),
        "msm_test_vector_slab": ([ctypes.c_uint64], None),
        "msm_test_vector_group": ([ctypes.c_uint32], None),
        "msm_fixed_destroy": ([vp], ctypes.c_int),
        "msm_fixed_info": ([vp, ctypes.POINTER(FixedInfo)], ctypes.c_int),
        "msm_fixed_mul": ([vp, vp, sz, optp, vp], ctypes.c_int),
        "msm_fixed_mul_device": ([vp, vp, sz, optp, vp, vp], ctypes.c_int),
        "msm_fixed_mul_create": ([vp, vp, sz, optp, ctypes.c_uint32, ctypes.POINTER(vp)], ctypes.c_int),
        "msm_fixed_mul_create_device": ([vp, vp, sz, optp, ctypes.c_uint32, vp, ctypes.POINTER(vp)], ctypes.c_int),
        "msm_fr_combine": ([ctypes.POINTER(FrCombine), sz, optp, vp], ctypes.c_int),
        "msm_fr_combine_device": ([ctypes.POINTER(FrCombine), sz, optp, vp, vp], ctypes.c_int),
        "msm_fr_powers": ([vp, vp, sz, ctypes.c_uint32, optp, vp], ctypes.c_int),
        "msm_fr_powers_device": ([vp, vp, sz, ctypes.c_uint32, optp, vp, vp], ctypes.c_int),
        "msm_fr_dot": ([vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, optp, u32p], ctypes.c_int),
        "msm_fr_dot_device": ([vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, optp, vp, u32p], ctypes.c_int),
        "msm_test_fr_op": ([ctypes.c_uint32, vp, vp, vp, sz], ctypes.c_int),
        "msm_fr_inverse": ([vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, optp, vp], ctypes.c_int),
        "msm_fr_inverse_device": ([vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, optp, vp, vp], ctypes.c_int),
        "msm_fr_scan": ([vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, optp, vp], ctypes.c_int),
        "msm_fr_scan_device": ([vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, optp, vp, vp],
                               ctypes.c_int),
        "msm_fr_tensor": ([vp, vp, ctypes.c_uint32, vp, ctypes.c_uint32, optp, vp], ctypes.c_int),
        "msm_fr_tensor_device": ([vp, vp, ctypes.c_uint32, vp, ctypes.c_uint32, optp, vp, vp], ctypes.c_int),
        "msm_test_fr_inv": ([vp, vp, sz], ctypes.c_int),
        "msm_test_fr_scan_constants": ([u32p], ctypes.c_int),
        "msm_test_fr_scan_plan": ([sz, ctypes.c_uint32, u32p], ctypes.c_int),
        "msm_test_fr_scan_device": ([vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp],
                                    ctypes.c_int),
        "msm_test_fr_inverse_device": ([vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp], ctypes.c_int),
        "msm_test_fixed_digits": ([vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                   ctypes.POINTER(ctypes.c_int32), u32p, u32p], ctypes.c_int),
        "msm_test_fixed_plan": ([ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p], ctypes.c_int),
        "msm_test_fixed_bases": ([vp, ctypes.POINTER(vp)], ctypes.c_int),
        "msm_test_fixed_proj": ([u32p, sz], ctypes.c_int),
        "msm_test_host_field": ([ctypes.c_uint32, vp, vp, vp, sz], ctypes.c_int),
        "msm_test_subset_plan": ([sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                  u32p], ctypes.c_int),
        "msm_test_bases_plan": ([sz, ctypes.c_uint32, ctypes.c_uint32, u32p], ctypes.c_int),
        "msm_test_narrow_plan": ([sz, ctypes.c_uint32, ctypes.c_uint32, u32p], ctypes.c_int),
        "msm_test_native_plan": ([sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p], ctypes.c_int),
        "msm_test_wide_plan": ([sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p], ctypes.c_int),
        "msm_test_fr_from_mont": ([u32p, sz, u32p, ctypes.c_void_p], ctypes.c_int),
        "msm_test_dense_plan": ([sz, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, u32p],
                                ctypes.c_int),
        "msm_test_dense_segments": ([vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p], ctypes.c_int),
        "msm_test_acc_state": ([u32p, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, sz, vp], ctypes.c_int),
        "msm_test_red_state": ([u32p, vp, sz, vp, vp, vp, sz, vp, vp, sz, vp], ctypes.c_int),
        "msm_test_red_map": ([sz, ctypes.c_uint32, optp, ctypes.c_uint32, u32p, vp, sz, vp, sz], ctypes.c_int),
        "msm_test_red_map_term": ([ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p, vp, sz], ctypes.c_int),
        "msm_test_tail_plan": ([sz, optp, ctypes.c_uint32, vp, ctypes.c_int, u32p, u32p], ctypes.c_int),
        "msm_test_bases_records": ([vp, ctypes.c_uint32, u32p], ctypes.c_int),
        "msm_test_split_scalars": ([vp, sz, ctypes.c_uint32, ctypes.c_uint32, u32p], ctypes.c_int),
        "msm_test_field_op": ([ctypes.c_uint32, vp, vp, u32p, sz], ctypes.c_int),
        "msm_test_point_op": ([ctypes.c_uint32, vp, vp, u32p, sz], ctypes.c_int),
        "msm_test_wide_masks": ([u32p], ctypes.c_int),
        "msm_test_limb_op": ([ctypes.c_uint32, vp, vp, vp, u32p, sz], ctypes.c_int),
        "msm_test_records": ([ctypes.c_uint32, vp, sz, u32p, u32p, vp, vp, u32p, sz], ctypes.c_int),
        "msm_test_shard_range": ([sz, sz, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)], ctypes.c_int),
        "msm_test_sharded": ([ctypes.c_int, vp, vp, sz, optp, ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32, vp,
                              u32p], ctypes.c_int),
        "msm_test_tail": ([sz, vp, ctypes.c_int, u32p, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
        "msm_test_tail_words": ([sz], sz),
        "msm_test_plan": ([sz, ctypes.c_uint32, ctypes.c_int, optp, u32p], ctypes.c_int),
        "msm_test_pack": ([vp, sz, ctypes.c_uint32, vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
                          ctypes.c_int),
        "msm_test_tail_batch": ([sz, ctypes.c_uint32, vp, ctypes.c_int, u32p, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
        "msm_test_peer_state": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
        "msm_test_host_timing": ([ctypes.c_int, sz, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
        "msm_test_pools": ([ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        "msm_test_guard_name": ([ctypes.c_uint32], ctypes.c_char_p),
        "msm_test_guard": ([ctypes.c_int], ctypes.c_int),
        "msm_test_guard_release": ([ctypes.c_int], ctypes.c_int),
        "msm_test_guard_check": ([ctypes.c_int, ctypes.POINTER(GuardHit), sz, ctypes.POINTER(sz)], ctypes.c_int),
        "msm_test_guard_plant": ([ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int], ctypes.c_int),
        "msm_test_guard_fill": ([ctypes.c_uint32], ctypes.c_int),
        "msm_test_guard_poison": ([ctypes.c_int], ctypes.c_int),
        "msm_test_guard_peek": ([ctypes.c_int, ctypes.c_int, ctypes.c_uint32, sz, sz, u32p], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        if name.startswith(("msm_test_", "msm_bases_", "msm_decompress_", "msm_compress_", "msm_fr_")) and not hasattr(L, name):
            continue  # a test hook or the handle API an older library variant (MSM_AMD_LIB A/B builds) predates
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    # Explicit teardown at interpreter exit (registered after torch's import, so it runs before
    # torch's own exit handlers): the library's streams, buffers and parked pool threads are released
    # and joined while the HIP runtime is still whole, not left to the shared objects' finalizers.
    atexit.register(_shutdown_at_exit)
    return L


def _shutdown_at_exit() -> None:
    if _lib is not None:
        _lib.msm_shutdown()


def _strerror(code: int) -> str:
    try:
        return load().msm_strerror(code).decode()
    except Exception:  # library itself missing
        return "libmsm unavailable"


def _check(rc: int, where: str) -> None:
    if rc != 0:
        raise MsmError(rc, where)


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


def _out(n: int) -> Tuple[np.ndarray, ctypes.POINTER(ctypes.c_uint32)]:
    o = np.zeros(n, dtype=np.uint32)
    return o, o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _opts(window_size: Optional[int], run_length: Optional[int] = None, device: int = -1, flags: int = 0,
          devices: Optional[Sequence[int]] = None, windows: Optional[Tuple[int, int]] = None,
          scalar_bits: Optional[int] = None, scalar_type=None):
    """A msm_opts by reference.  `devices` (a list of HIP ordinals) runs the call on several
    devices (MSM_FLAG_DEVICES); the array is kept alive by the returned object.  `windows` =
    (lo, hi) restricts the MSM to those signed-digit windows (MSM_FLAG_WINDOWS; needs an explicit
    window_size); (lo, hi, 2) counts the range in half windows (MSM_FLAG_HALF_WINDOWS: half window
    2w is window w's lower-half buckets, 2w + 1 its upper half).  `scalar_bits` = b declares narrow
    scalars of ceil(b / 32) words (MSM_FLAG_SCALAR_BITS; the Bases.compute* calls only).
    `scalar_type` (a SCALAR_TYPES name, or a raw MSM_SCALAR_* value) declares native integer scalars
    (MSM_FLAG_SCALAR_TYPE; the same calls only): the options are then a MsmOptsTyped.  A WIDE_TYPES
    name declares wide scalars instead (MSM_FLAG_SCALAR_FIELD, MsmOptsTyped.scalar_field)."""
    if scalar_type is None:
        o = MsmOpts(int(window_size or 0), int(run_length or 0), int(device), int(flags))
    elif isinstance(scalar_type, str) and scalar_type in WIDE_TYPES:
        o = MsmOptsTyped(int(window_size or 0), int(run_length or 0), int(device), int(flags) | MSM_FLAG_SCALAR_FIELD)
        o.scalar_field = WIDE_TYPES[scalar_type][0]
    else:
        o = MsmOptsTyped(int(window_size or 0), int(run_length or 0), int(device), int(flags) | MSM_FLAG_SCALAR_TYPE)
        o.scalar_type = SCALAR_TYPES[scalar_type][0] if isinstance(scalar_type, str) else int(scalar_type)
    if scalar_bits is not None:
        if not 0 <= int(scalar_bits) < 1 << 32:
            raise ValueError("scalar_bits out of range")
        o.scalar_bits = int(scalar_bits)
        o.flags |= MSM_FLAG_SCALAR_BITS
    if windows is not None:
        o.window_lo, o.window_hi = int(windows[0]), int(windows[1])
        o.flags |= MSM_FLAG_WINDOWS
        if len(windows) > 2:
            if int(windows[2]) not in (1, 2):
                raise ValueError(f"window range unit 1/{windows[2]}: only whole (1) or half (2) windows")
            if int(windows[2]) == 2:
                o.flags |= MSM_FLAG_HALF_WINDOWS
    if devices is not None:
        arr = (ctypes.c_int32 * max(len(devices), 1))(*[int(d) for d in devices])
        o.devices = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32))
        o.n_devices = len(devices)
        o.flags |= MSM_FLAG_DEVICES
        o._keep = arr
    return ctypes.byref(o)


def wire_to_int(words: Iterable[int]) -> int:
    v = 0
    for w in words:
        v = (v << 32) | int(w)
    return v


def _int_be_words(v: int) -> bytes:
    if v < 0 or v >= 1 << 256:
        raise ValueError("value does not fit 256 bits")
    return int(v).to_bytes(32, "big")


def points_to_wire(points) -> np.ndarray:
    """BigIntPoint[] ({x,y,t,z} ints or (x,y,t,z) tuples) or U32ArrayPoint[] -> wire [n, 32] u32.

    Same layout as submission.ts:35-86 / convert_worker.ts:8-57: x|y|t|z, each 8 BE words.
    A numpy array of shape [n, 32] is taken as already-marshalled wire data.
    """
    if isinstance(points, np.ndarray):
        return _u32(points).reshape(-1, 32)
    pts = list(points)
    if not pts:
        return np.zeros((0, 32), dtype=np.uint32)
    first = pts[0]
    keys = ("x", "y", "t", "z")
    if isinstance(first, dict):
        get = lambda p, k: p[k]  # noqa: E731
    elif hasattr(first, "x"):
        get = lambda p, k: getattr(p, k)  # noqa: E731
    else:
        get = lambda p, k: p[keys.index(k)]  # noqa: E731
    sample = get(first, "x")
    if isinstance(sample, (int, np.integer)):
        buf = b"".join(_int_be_words(int(get(p, k))) for p in pts for k in keys)
        return np.frombuffer(buf, dtype=">u4").astype(np.uint32).reshape(-1, 32)
    out = np.empty((len(pts), 32), dtype=np.uint32)
    for i, p in enumerate(pts):  # U32ArrayPoint: four BE u32[8]
        for j, k in enumerate(keys):
            out[i, 8 * j: 8 * j + 8] = np.asarray(get(p, k), dtype=np.uint32)
    return out


# Compressed point forms (include/msm.h MSM_POINTS_X_*): 8 BE words per point, x alone ("subgroup": y is
# the root whose point is in the prime-order subgroup, Aleo's form) or x with y's sign in bit 255 ("ysign").
POINT_FORMS = {"subgroup": 1, "ysign": 2}


def _point_form(form) -> int:
    if isinstance(form, str):
        if form not in POINT_FORMS:
            raise ValueError(f"unknown point form {form!r}: one of {sorted(POINT_FORMS)}")
        return POINT_FORMS[form]
    return int(form)


def xs_to_wire(xs, form="subgroup", signs=None) -> np.ndarray:
    """x-coordinates -> compressed points [n, 8] u32.  Python ints are packed as 8 BE words; for
    form="ysign" `signs` gives each point's flag (y > p - y) and is set here, in bit 255 -- an x with
    that bit already set does not fit the field and is passed through for the library to refuse.  An
    [n, 8] uint32 array is taken as already marshalled (msm_compress_points' output, flags included);
    `signs` must then be None."""
    if isinstance(xs, np.ndarray) and xs.dtype != object:
        if signs is not None:
            raise ValueError("signs are for integer x-coordinates; a word array carries its own flags")
        return np.ascontiguousarray(_u32(xs).reshape(-1, 8))
    vals = [int(v) for v in xs]
    if signs is not None:
        if _point_form(form) != POINT_FORMS["ysign"]:
            raise ValueError('signs need form="ysign"')
        flags = [bool(f) for f in signs]
        if len(flags) != len(vals):
            raise ValueError("signs and xs differ in length")
        for v in vals:
            if v >> 255:
                raise ValueError("x does not leave bit 255 free for the sign")
        vals = [v | (int(f) << 255) for v, f in zip(vals, flags)]
    if not vals:
        return np.zeros((0, 8), dtype=np.uint32)
    buf = b"".join(_int_be_words(v) for v in vals)
    return np.frombuffer(buf, dtype=">u4").astype(np.uint32).reshape(-1, 8)


def decompress_points(xs, form="subgroup", signs=None, device: int = -1) -> np.ndarray:
    """Compressed points (anything xs_to_wire takes) -> wire points [n, 32], y recovered on the device
    (msm_decompress_points).  MsmError -3 for an x out of range, -4 for an x of no such point."""
    w = xs_to_wire(xs, form, signs)
    out = np.zeros((w.shape[0], 32), dtype=np.uint32)
    _check(load().msm_decompress_points(_ptr(w), w.shape[0], _point_form(form), _opts(None, None, device), _ptr(out)),
           "msm_decompress_points")
    return out


def decompress_points_device(d_xs, n: int, d_points, form="subgroup", device: int = -1, stream: int = 0) -> None:
    """The same between device buffers (torch tensors or raw pointers, 16-byte aligned): n x 8 words in,
    n x 32 words out; complete on return."""
    _check(load().msm_decompress_points_device(_dev_ptr(d_xs), n, _point_form(form), _opts(None, None, device),
                                               _stream(stream, d_xs, d_points), _dev_ptr(d_points)),
           "msm_decompress_points_device")


def compress_points(points, form="subgroup") -> np.ndarray:
    """Affine points -> compressed points [n, 8] (msm_compress_points, host only): wire points [n, 32]
    with z = 1, [n, 16] x|y words, or (x, y) integer pairs.  Subgroup membership is not tested."""
    if isinstance(points, np.ndarray) and points.dtype != object:
        a = _u32(points)
        if a.ndim != 2 or a.shape[1] not in (16, 32):
            raise ValueError("points: [n, 32] wire words or [n, 16] x|y words")
        if a.shape[1] == 32:
            z = a[:, 24:32]
            if a.shape[0] and not (np.all(z[:, :7] == 0) and np.all(z[:, 7] == 1)):
                raise ValueError("compress_points takes affine points (z = 1)")
        xy = np.ascontiguousarray(a[:, :16])
    else:
        pts = [(int(p[0]), int(p[1])) for p in points]
        buf = b"".join(_int_be_words(x) + _int_be_words(y) for x, y in pts)
        xy = np.frombuffer(buf, dtype=">u4").astype(np.uint32).reshape(-1, 16)
    out = np.zeros((xy.shape[0], 8), dtype=np.uint32)
    _check(load().msm_compress_points(_ptr(xy), xy.shape[0], _point_form(form), _ptr(out)), "msm_compress_points")
    return out


def _scalar_words(scalar_bits: Optional[int]) -> int:
    """u32 words per wire scalar: 8, or ceil(b / 32) for narrow scalars of b bits (0 for a width
    outside 1..256: arrays then go to the library as they are, and it reports the width)."""
    if scalar_bits is None:
        return 8
    return (int(scalar_bits) + 31) // 32 if 1 <= int(scalar_bits) <= 256 else 0


def scalars_to_wire(scalars, scalar_bits: Optional[int] = None) -> np.ndarray:
    """bigint[] or Uint32Array[] (BE u32[8]) -> [n, 8] u32.  With `scalar_bits` = b the narrow
    format of the Bases.compute* calls: [n, ceil(b / 32)] u32, big-endian words; a value >= 2^b
    raises ValueError."""
    words = _scalar_words(scalar_bits)
    if isinstance(scalars, np.ndarray):
        return _u32(scalars).reshape(-1, words) if words else np.atleast_2d(_u32(scalars))
    if not words:
        raise ValueError("scalar_bits must be 1..256")
    sc = list(scalars)
    if not sc:
        return np.zeros((0, words), dtype=np.uint32)
    if isinstance(sc[0], (int, np.integer)):
        if scalar_bits is None:
            buf = b"".join(_int_be_words(int(s)) for s in sc)
        else:
            if any(int(s) < 0 or int(s) >> int(scalar_bits) for s in sc):
                raise ValueError(f"a scalar does not fit {int(scalar_bits)} bits")
            buf = b"".join(int(s).to_bytes(4 * words, "big") for s in sc)
        return np.frombuffer(buf, dtype=">u4").astype(np.uint32).reshape(-1, words)
    return np.stack([np.asarray(s, dtype=np.uint32).reshape(words) for s in sc])


def scalars_to_native(values, scalar_type: str) -> np.ndarray:
    """Python ints -> the array a Bases.compute*(scalar_type=...) call takes: the type's numpy dtype, or
    for "bit" the little-order bitmap np.packbits(bits, bitorder="little").  A value the type cannot
    hold raises ValueError."""
    if scalar_type not in SCALAR_TYPES:
        raise ValueError(f"unknown scalar type {scalar_type!r}")
    _, dt, e = SCALAR_TYPES[scalar_type]
    vals = [int(v) for v in values]
    lo, hi = (-(1 << (e - 1)), 1 << (e - 1)) if scalar_type[0] == "i" else (0, 1 << e)
    if any(not lo <= v < hi for v in vals):
        raise ValueError(f"a scalar does not fit {scalar_type}")
    if scalar_type == "bit":
        return np.packbits(np.array(vals, dtype=np.uint8), bitorder="little")
    return np.array(vals, dtype=dt).reshape(-1)


def scalars_to_wide(values, scalar_type: str) -> np.ndarray:
    """Python ints -> the array a Bases.compute*(scalar_type=<a WIDE_TYPES name>) call takes: uint64
    [n, e / 64], little-endian limbs (least significant first).  "i128" takes negative values (two's
    complement); "fr_mont" takes v < r and encodes the Montgomery form v 2^256 mod r, the memory of an
    arkworks Fr.  A value the type cannot hold raises ValueError."""
    if scalar_type not in WIDE_TYPES:
        raise ValueError(f"unknown wide scalar type {scalar_type!r}")
    e = WIDE_TYPES[scalar_type][1]
    vals = [int(v) for v in values]
    lo, hi = (-(1 << 127), 1 << 127) if scalar_type == "i128" else (0, FR_MODULUS if scalar_type == "fr_mont" else 1 << e)
    if any(not lo <= v < hi for v in vals):
        raise ValueError(f"a scalar does not fit {scalar_type}")
    if scalar_type == "fr_mont":
        vals = [(v << 256) % FR_MODULUS for v in vals]
    buf = b"".join((v & ((1 << e) - 1)).to_bytes(e // 8, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").astype(np.uint64).reshape(-1, e // 64)


class WideArrayError(TypeError, ValueError):
    """An array that a wide scalar type does not take.  A TypeError; also a ValueError, which is what these
    type names raised with any array while they were unknown."""


def _wide_check(arr, name: str, where: str = "") -> None:
    """The arrays a wide type takes: C-contiguous [n, e / 64] 64-bit, [n, e / 32] uint32 or [n, e / 8] uint8
    (numpy: uint64 / uint32 / uint8; torch: int64 / uint8).  TypeError for anything else."""
    e = WIDE_TYPES[name][1]
    dt = str(getattr(arr, "dtype", None))
    size = {"uint64": 8, "uint32": 4, "uint8": 1, "torch.int64": 8, "torch.uint8": 1}.get(dt)
    shape = tuple(getattr(arr, "shape", ()))
    if size is None or len(shape) != 2 or shape[1] * size * 8 != e:
        raise WideArrayError(f"scalar_type {name!r} takes [n, {e // 64}] 64-bit, [n, {e // 32}] uint32 or [n, {e // 8}] uint8 "
                        f"arrays, not {dt} {shape}{where}")
    contiguous = arr.flags["C_CONTIGUOUS"] if isinstance(arr, np.ndarray) else arr.is_contiguous()
    if not contiguous:
        raise WideArrayError(f"scalar_type {name!r} takes C-contiguous arrays{where}")


def _wide_device(t, name) -> None:
    """A device vector of a wide type: a tensor is checked as _wide_check does and must be on a device; a
    raw device pointer is taken as it is."""
    if name in WIDE_TYPES and not isinstance(t, int):
        if isinstance(t, np.ndarray) or not getattr(t, "is_cuda", False):
            raise WideArrayError(f"scalar_type {name!r}: the device entries take a device tensor or a raw pointer")
        _wide_check(t, name)


_TORCH_NATIVE = {"torch.bool": "bool", "torch.uint8": "u8", "torch.int8": "i8", "torch.int16": "i16",
                 "torch.int32": "i32", "torch.int64": "i64", "torch.uint16": "u16", "torch.uint32": "u32",
                 "torch.uint64": "u64"}


def _native_type(scalars, scalar_type, scalar_bits):
    """Resolve `scalar_type` for one array (or the first of a list): "native" becomes the name of the
    numpy or torch dtype -- bool is "u8" with scalar_bits = 1 unless a width is given.  Returns
    (name or None, scalar_bits)."""
    if scalar_type is None:
        return None, scalar_bits
    if scalar_type != "native":
        if scalar_type in WIDE_TYPES:  # ("native" never infers one: a [n, 4] uint64 array is ambiguous)
            if scalars is not None and not isinstance(scalars, (int, list, tuple)):
                _wide_check(scalars, scalar_type)
            return scalar_type, scalar_bits
        if scalar_type not in SCALAR_TYPES:
            raise ValueError(f"unknown scalar type {scalar_type!r}")
        return scalar_type, scalar_bits
    dt = getattr(scalars, "dtype", None)
    if isinstance(dt, np.dtype):
        name = "bool" if dt == np.bool_ else next((k for k, (_, d, _) in SCALAR_TYPES.items()
                                                    if k != "bit" and d == dt), None)
    else:
        name = _TORCH_NATIVE.get(str(dt))
    if name is None:
        raise TypeError(f"no native scalar type for dtype {dt!r}")
    if name == "bool":
        return "u8", 1 if scalar_bits is None else scalar_bits
    return name, scalar_bits


def _native_host(scalars, name: str) -> np.ndarray:
    """A host vector of a native type as a flat contiguous numpy array of the type's dtype: typed
    arrays (and CPU torch tensors) pass through uncopied when contiguous; ints are packed.
    A wide type's vector stays [n, k] (its first dimension counts the scalars) and is copied only where
    its memory is not 8-byte aligned."""
    if name in WIDE_TYPES:
        if hasattr(scalars, "numpy") and not isinstance(scalars, np.ndarray):
            _wide_check(scalars, name)
            scalars = scalars.numpy()  # a CPU tensor: shares its memory (torch has no uint64: int64 limbs)
            scalars = scalars.view(np.uint64) if scalars.dtype == np.int64 else scalars
        if not isinstance(scalars, np.ndarray):
            return scalars_to_wide(scalars, name)
        _wide_check(scalars, name)
        if scalars.ctypes.data & 7:
            buf = np.empty(scalars.nbytes // 8, dtype=np.uint64)
            buf.view(np.uint8)[:] = scalars.reshape(-1).view(np.uint8)
            scalars = buf.view(scalars.dtype).reshape(scalars.shape)
        return scalars
    dt = SCALAR_TYPES[name][1]
    if hasattr(scalars, "numpy") and not isinstance(scalars, np.ndarray):
        scalars = scalars.numpy()  # a CPU tensor: shares its memory
    if isinstance(scalars, np.ndarray):
        if scalars.dtype == np.bool_ and dt == np.uint8:
            scalars = scalars.view(np.uint8)
        if scalars.dtype != dt:
            raise TypeError(f"scalar_type {name!r} takes {dt} arrays, not {scalars.dtype}")
        return np.ascontiguousarray(scalars).reshape(-1)
    return scalars_to_native(scalars, name)


def _native_len(arr: np.ndarray, name: str, m: Optional[int]) -> int:
    """Scalars a host vector holds: its elements, or for a bitmap `m` (at most 8 per byte)."""
    if name != "bit":
        return arr.shape[0]
    if m is None:
        raise ValueError("a bit vector's length is not its byte count: pass m")
    if (int(m) + 7) // 8 > arr.shape[0]:
        raise ValueError("fewer bits than m")
    return int(m)


def _xy(o: np.ndarray) -> Tuple[int, int]:
    return wire_to_int(o[:8]), wire_to_int(o[8:16])


def get_best_window_size(n: int) -> int:
    """getBestWindowSize (submission.ts:18-23), retuned for the signed-digit GPU pipeline."""
    return int(load().msm_best_window(n))


def compute_msm_wire(points_wire: np.ndarray, scalars_wire: np.ndarray, window_size: Optional[int] = None,
                     run_length: Optional[int] = None, device: int = -1,
                     devices: Optional[Sequence[int]] = None, cpu_work_ratio: float = 0.0,
                     cpu_threads: int = 0) -> Tuple[int, int]:
    """msm_compute on host wire arrays; `devices` shards the points over those HIP ordinals.
    cpu_work_ratio > 0 is the reference's CPU/GPU co-compute (?cpuWorkRatio, submission.ts:94-154):
    the first floor(ratio n) points on the host Pippenger (cpu_threads threads, 0 = all) beside the
    GPU share, joined with one EC add (msm_compute_cocompute)."""
    L = load()
    pts = _u32(points_wire).reshape(-1, 32)
    sc = _u32(scalars_wire).reshape(-1, 8)
    n = min(pts.shape[0], sc.shape[0])  # the oracle zips to the shorter length
    pts, sc = np.ascontiguousarray(pts[:n]), np.ascontiguousarray(sc[:n])
    o, op = _out(16)
    opts = _opts(window_size, run_length, device, devices=devices)
    if cpu_work_ratio:
        _check(L.msm_compute_cocompute(_ptr(pts), _ptr(sc), n, opts, float(cpu_work_ratio), int(cpu_threads), op),
               "msm_compute_cocompute")
    else:
        _check(L.msm_compute(_ptr(pts), _ptr(sc), n, opts, op), "msm_compute")
    return _xy(o)


def compute_msm(base_affine_points, scalars, window_size: Optional[int] = None,
                run_length: Optional[int] = None, device: int = -1,
                devices: Optional[Sequence[int]] = None, cpu_work_ratio: float = 0.0) -> Tuple[int, int]:
    """compute_msm (submission.ts:25-157): MSM of BigIntPoint[]/U32ArrayPoint[] with bigint[]/Uint32Array[];
    cpu_work_ratio as the reference's ?cpuWorkRatio (compute_msm_wire)."""
    return compute_msm_wire(points_to_wire(base_affine_points), scalars_to_wire(scalars), window_size,
                            run_length, device, devices, cpu_work_ratio)


def compute_msm_partial(points_wire: np.ndarray, scalars_wire: np.ndarray, window_size: Optional[int] = None,
                        device: int = -1, devices: Optional[Sequence[int]] = None,
                        windows: Optional[Tuple[int, int]] = None) -> np.ndarray:
    L = load()
    pts = _u32(points_wire).reshape(-1, 32)
    sc = _u32(scalars_wire).reshape(-1, 8)
    n = min(pts.shape[0], sc.shape[0])
    pts, sc = np.ascontiguousarray(pts[:n]), np.ascontiguousarray(sc[:n])
    o, op = _out(32)
    _check(L.msm_compute_partial(_ptr(pts), _ptr(sc), n,
                                 _opts(window_size, None, device, devices=devices, windows=windows), op),
           "msm_compute_partial")
    return o


def launch_plan(n: int, nm: int = 1, pipelined: bool = False, window_size: Optional[int] = None,
                run_length: Optional[int] = None, windows: Optional[Tuple[int, int]] = None) -> dict:
    """The launch plan libmsm builds for n points and nm MSMs per launch (msm_test_plan; default
    device shape): window width c, windows per MSM in the launch, run length K, reduction chunk L,
    coarse bins per window and the skew floor of K.  No GPU needed."""
    out = np.zeros(7, np.uint32)
    _check(load().msm_test_plan(n, nm, int(pipelined), _opts(window_size, run_length, windows=windows),
                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), "msm_test_plan")
    return dict(zip(("c", "windows", "run_length", "chunk_len", "msms_per_launch", "coarse_bins", "skew_floor"),
                    (int(v) for v in out)))


def pack_points(points_wire, xyz: bool = False) -> Tuple[np.ndarray, bool, bool]:
    """The packed uploads' host packing (msm_test_pack): wire records -> x|y (or x|y|z) words,
    whether every z is 1, whether some t >= p.  No GPU needed."""
    pts = np.ascontiguousarray(_u32(points_wire).reshape(-1, 32))
    n = pts.shape[0]
    w = 24 if xyz else 16
    out = np.zeros((n, w), np.uint32)
    z1, tb = ctypes.c_int(0), ctypes.c_int(0)
    _check(load().msm_test_pack(_ptr(pts), n, 2 if xyz else 1, _ptr(out), ctypes.byref(z1), ctypes.byref(tb)),
           "msm_test_pack")
    return out, bool(z1.value), bool(tb.value)


def window_count(window_size: int) -> int:
    """Signed-digit windows of an MSM at window width c, overflow window included
    (msm_window_count): the index space of the `windows=(lo, hi)` ranges."""
    return int(load().msm_window_count(int(window_size)))


def _dev_ptr(t) -> int:
    return int(t.data_ptr()) if hasattr(t, "data_ptr") else int(t)


def _stream(stream: Optional[int], *tensors) -> Optional[int]:
    """The stream libmsm orders its work after: the caller's, or -- when any input is a torch
    tensor -- torch's current stream on that tensor's device (so inputs written by kernels just
    enqueued there are complete before libmsm reads them).  Raw device pointers with no stream
    leave the ordering to the caller (None)."""
    if stream:
        return stream
    for t in tensors:
        if hasattr(t, "is_cuda") and t.is_cuda:
            import torch

            return torch.cuda.current_stream(t.device).cuda_stream or MSM_STREAM_NULL
    return None


def _first(xs):
    return xs[0] if len(xs) else None


def compute_msm_device(d_points, d_scalars, n: int, window_size: Optional[int] = None,
                       run_length: Optional[int] = None, device: int = -1, stream: int = 0,
                       devices: Optional[Sequence[int]] = None) -> Tuple[int, int]:
    """Inputs already in HBM (torch tensors or raw device pointers, wire layout).  With `devices`
    the listed devices other than the inputs' own copy their shard over xGMI and reduce it."""
    L = load()
    o, op = _out(16)
    _check(L.msm_compute_device(_dev_ptr(d_points), _dev_ptr(d_scalars), n,
                                _opts(window_size, run_length, device, devices=devices),
                                _stream(stream, d_points, d_scalars), op), "msm_compute_device")
    return _xy(o)


def compute_msm_device_partial(d_points, d_scalars, n: int, window_size: Optional[int] = None,
                               device: int = -1, stream: int = 0,
                               devices: Optional[Sequence[int]] = None,
                               windows: Optional[Tuple[int, int]] = None) -> np.ndarray:
    L = load()
    o, op = _out(32)
    _check(L.msm_compute_device_partial(_dev_ptr(d_points), _dev_ptr(d_scalars), n,
                                        _opts(window_size, None, device, devices=devices, windows=windows),
                                        _stream(stream, d_points, d_scalars), op), "msm_compute_device_partial")
    return o


def compute_msm_batch_device(d_points, d_scalars, n: int, count: int, window_size: Optional[int] = None,
                             device: int = -1, stream: int = 0) -> np.ndarray:
    L = load()
    o, op = _out(16 * count)
    _check(L.msm_compute_batch_device(_dev_ptr(d_points), _dev_ptr(d_scalars), n, count,
                                      _opts(window_size, None, device), _stream(stream, d_points, d_scalars), op),
           "msm_compute_batch_device")
    return o.reshape(count, 16)


def compute_msm_many_device(points_list, scalars_list, n: int, window_size: Optional[int] = None,
                            run_length: Optional[int] = None, device: int = -1, stream: int = 0,
                            flags: int = 0) -> np.ndarray:
    """len(points_list) independent n-point MSMs on device-resident inputs (torch tensors or raw
    device pointers), pipelined inside libmsm: the device runs MSM b+1 while the host finishes
    MSM b.  Returns [count][16] BE words (x | y)."""
    L = load()
    count = len(points_list)
    if len(scalars_list) != count:
        raise ValueError("points_list and scalars_list differ in length")
    pp = (ctypes.c_void_p * max(count, 1))(*[_dev_ptr(t) for t in points_list])
    ss = (ctypes.c_void_p * max(count, 1))(*[_dev_ptr(t) for t in scalars_list])
    o, op = _out(16 * max(count, 1))
    _check(L.msm_compute_many_device(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(ss, ctypes.c_void_p), n, count,
                                     _opts(window_size, run_length, device, flags),
                                     _stream(stream, _first(points_list), _first(scalars_list)), op),
           "msm_compute_many_device")
    return o[:16 * count].reshape(count, 16)


def compute_msm_shared_device(d_points, scalars_list, n: int, window_size: Optional[int] = None,
                              run_length: Optional[int] = None, device: int = -1, stream: int = 0,
                              flags: int = 0) -> np.ndarray:
    """Prover batch: len(scalars_list) MSMs over ONE device-resident base vector (prepared once
    per call).  Returns [count][16] BE words."""
    L = load()
    count = len(scalars_list)
    ss = (ctypes.c_void_p * max(count, 1))(*[_dev_ptr(t) for t in scalars_list])
    o, op = _out(16 * max(count, 1))
    _check(L.msm_compute_shared_device(_dev_ptr(d_points), ctypes.cast(ss, ctypes.c_void_p), n, count,
                                       _opts(window_size, run_length, device, flags),
                                       _stream(stream, d_points, _first(scalars_list)), op),
           "msm_compute_shared_device")
    return o[:16 * count].reshape(count, 16)


def _host_list(arrs, words: int):
    keep = [np.ascontiguousarray(_u32(a).reshape(-1, words) if words else np.atleast_2d(_u32(a))) for a in arrs]
    ptrs = (ctypes.c_void_p * max(len(keep), 1))(*[a.ctypes.data for a in keep])
    return keep, ptrs


def _native_list(arrs, name: str):
    keep = [_native_host(a, name) for a in arrs]
    ptrs = (ctypes.c_void_p * max(len(keep), 1))(*[a.ctypes.data for a in keep])
    return keep, ptrs


class Bases:
    """A base vector prepared once and kept on one device (include/msm.h msm_bases_*): every
    compute call then brings scalars only.  `levels` > 1 also keeps the shifted copies
    2^(j S) P_i, and every MSM runs folded over 1/levels of the windows (0 = the library's choice).

        with Bases.from_wire(points) as bases:
            x, y = bases.compute(scalars)

    A coordinate >= p or a z = 0 point fails the constructor (MsmError -3 / -4), never a compute
    call.  Use after close() -- or after the library shut down -- raises MsmError(-1)."""

    def __init__(self, handle: int):
        self._h = handle

    @classmethod
    def from_wire(cls, points, levels: int = 0, window_size: Optional[int] = None, device: int = -1) -> "Bases":
        """Host points (wire [n, 32] words, or anything points_to_wire takes)."""
        pts = np.ascontiguousarray(points_to_wire(points))
        h = ctypes.c_void_p()
        _check(load().msm_bases_create(_ptr(pts), pts.shape[0], _opts(window_size, None, device), int(levels),
                                       ctypes.byref(h)), "msm_bases_create")
        return cls(h.value or 0)

    @classmethod
    def from_device(cls, d_points, n: int, levels: int = 0, window_size: Optional[int] = None, device: int = -1,
                    stream: int = 0) -> "Bases":
        """Points already in HBM (a torch tensor or a raw device pointer, wire layout)."""
        h = ctypes.c_void_p()
        _check(load().msm_bases_create_device(_dev_ptr(d_points), n, _opts(window_size, None, device), int(levels),
                                              _stream(stream, d_points), ctypes.byref(h)), "msm_bases_create_device")
        return cls(h.value or 0)

    @classmethod
    def from_x(cls, xs, form="subgroup", signs=None, levels: int = 0, window_size: Optional[int] = None,
               device: int = -1) -> "Bases":
        """Host compressed points (anything xs_to_wire takes): 32 bytes per point go up, y is recovered
        on the device, and the handle is the one from_wire makes from the same points.  An x of no
        point of the form fails here (MsmError -4), as does one out of range (-3)."""
        w = xs_to_wire(xs, form, signs)
        h = ctypes.c_void_p()
        _check(load().msm_bases_create_compressed(_ptr(w), w.shape[0], _point_form(form),
                                                  _opts(window_size, None, device), int(levels), ctypes.byref(h)),
               "msm_bases_create_compressed")
        return cls(h.value or 0)

    @classmethod
    def from_x_device(cls, d_xs, n: int, form="subgroup", levels: int = 0, window_size: Optional[int] = None,
                      device: int = -1, stream: int = 0) -> "Bases":
        """Compressed points already in HBM (a torch tensor or a raw device pointer, 16-byte aligned)."""
        h = ctypes.c_void_p()
        _check(load().msm_bases_create_compressed_device(_dev_ptr(d_xs), n, _point_form(form),
                                                         _opts(window_size, None, device), int(levels),
                                                         _stream(stream, d_xs), ctypes.byref(h)),
               "msm_bases_create_compressed_device")
        return cls(h.value or 0)

    @property
    def info(self) -> dict:
        inf = BasesInfo()
        _check(load().msm_bases_info(self._h or None, ctypes.byref(inf)), "msm_bases_info")
        return {name: int(getattr(inf, name)) for name, _ in BasesInfo._fields_ if name != "reserved"}

    # Every compute call takes `scalar_bits` = b (include/msm.h MSM_FLAG_SCALAR_BITS): the scalars are
    # then narrow -- [n, ceil(b / 32)] words each, big-endian words, below 2^b (scalars_to_wire(...,
    # scalar_bits=b) packs ints) -- and the MSM runs the windows of a b-bit scalar only.
    # And `scalar_type` (include/msm.h MSM_FLAG_SCALAR_TYPE): None (the word formats above), a
    # SCALAR_TYPES name -- the vector is then a flat array of that integer type, negative values
    # included, or for "bit" a little-order bitmap -- or "native", the type of the array's own numpy /
    # torch dtype (bool: "u8" with scalar_bits = 1).  scalar_bits then bounds the magnitude, |v| < 2^b.
    # A WIDE_TYPES name (include/msm.h MSM_FLAG_SCALAR_FIELD) takes little-endian 128- / 256-bit elements:
    # [n, e / 64] uint64 (torch: int64), [n, e / 32] uint32 or [n, e / 8] uint8, C-contiguous; "fr_mont" is
    # Fr in Montgomery form (scalars_to_wide packs ints).  "native" never infers a wide type.

    def compute(self, scalars, window_size: Optional[int] = None, run_length: Optional[int] = None,
                scalar_bits: Optional[int] = None, scalar_type=None) -> Tuple[int, int]:
        """One MSM of host scalars ([n, 8] wire words, or anything scalars_to_wire takes)."""
        n = self.info["n"]
        ty, scalar_bits = _native_type(scalars, scalar_type, scalar_bits)
        if ty:
            sc = _native_host(scalars, ty)
            short = _native_len(sc, ty, n) < n
        else:
            sc = np.ascontiguousarray(scalars_to_wire(scalars, scalar_bits))
            short = sc.shape[0] < n
        if short:
            raise ValueError("fewer scalars than the handle has points")
        o, op = _out(16)
        _check(load().msm_bases_compute(self._h, _ptr(sc),
                                        _opts(window_size, run_length, scalar_bits=scalar_bits, scalar_type=ty), op),
               "msm_bases_compute")
        return _xy(o)

    def compute_device(self, d_scalars, window_size: Optional[int] = None, run_length: Optional[int] = None,
                       stream: int = 0, scalar_bits: Optional[int] = None, scalar_type=None) -> Tuple[int, int]:
        """One MSM of device-resident scalars (a torch tensor or a raw device pointer, n x 8 words)."""
        ty, scalar_bits = _native_type(d_scalars, scalar_type, scalar_bits)
        _wide_device(d_scalars, ty)
        o, op = _out(16)
        _check(load().msm_bases_compute_device(self._h or None, _dev_ptr(d_scalars),
                                               _opts(window_size, run_length, scalar_bits=scalar_bits,
                                                     scalar_type=ty),
                                               _stream(stream, d_scalars), op), "msm_bases_compute_device")
        return _xy(o)

    def compute_many(self, scalars_list, window_size: Optional[int] = None, run_length: Optional[int] = None,
                     flags: int = 0, scalar_bits: Optional[int] = None, scalar_type=None) -> np.ndarray:
        """len(scalars_list) pipelined MSMs of host scalar vectors.  [count][16] BE words."""
        n = self.info["n"]
        ty, scalar_bits = _native_type(_first(scalars_list), scalar_type, scalar_bits)
        if ty:
            ks, ss = _native_list(scalars_list, ty)
            short = any(_native_len(b, ty, n) < n for b in ks)
        else:
            ks, ss = _host_list(scalars_list, _scalar_words(scalar_bits))
            short = any(b.shape[0] < n for b in ks)
        if short:
            raise ValueError("fewer scalars than the handle has points")
        count = len(ks)
        o, op = _out(16 * max(count, 1))
        _check(load().msm_bases_compute_many(self._h, ctypes.cast(ss, ctypes.c_void_p), count,
                                             _opts(window_size, run_length, -1, flags, scalar_bits=scalar_bits,
                                                   scalar_type=ty), op),
               "msm_bases_compute_many")
        return o[:16 * count].reshape(count, 16)

    def compute_many_device(self, scalars_list, window_size: Optional[int] = None, run_length: Optional[int] = None,
                            flags: int = 0, stream: int = 0, scalar_bits: Optional[int] = None,
                            scalar_type=None) -> np.ndarray:
        """The same with device-resident scalar vectors."""
        count = len(scalars_list)
        ty, scalar_bits = _native_type(_first(scalars_list), scalar_type, scalar_bits)
        for t in scalars_list:
            _wide_device(t, ty)
        ss = (ctypes.c_void_p * max(count, 1))(*[_dev_ptr(t) for t in scalars_list])
        o, op = _out(16 * max(count, 1))
        _check(load().msm_bases_compute_many_device(self._h or None, ctypes.cast(ss, ctypes.c_void_p), count,
                                                    _opts(window_size, run_length, -1, flags, scalar_bits=scalar_bits,
                                                          scalar_type=ty),
                                                    _stream(stream, _first(scalars_list)), op),
               "msm_bases_compute_many_device")
        return o[:16 * count].reshape(count, 16)

    # ---- subsets of the bases (include/msm.h msm_bases_compute_subset*) ----
    # Range form: bases [first, first + m).  Indexed form: bases indices[i] (uint32, each < n,
    # repeats allowed; `first` must stay 0).  m is the length of the scalar vector(s).

    @staticmethod
    def _subset(first: int, m: int, index_ptrs: Optional[Sequence[int]]):
        """A msm_subset_t by reference; the pointer array is kept alive by the returned object."""
        sub = Subset(int(first), int(m), None)
        if index_ptrs is not None:
            arr = (ctypes.c_void_p * max(len(index_ptrs), 1))(*index_ptrs)
            sub.indices = ctypes.cast(arr, ctypes.c_void_p)
            sub._keep = arr
        return sub

    @staticmethod
    def _host_indices(indices, m: int, count: int):
        """Host index vectors of `count` MSMs (one array: shared by all) as uint32 arrays of m."""
        if indices is None:
            return None, None
        vecs = list(indices) if isinstance(indices, (list, tuple)) else [indices] * count
        if len(vecs) != count:
            raise ValueError("one index vector per scalar vector")
        keep, seen = [], {}
        for v in vecs:  # a vector given again keeps one copy, and so one pointer
            if id(v) not in seen:
                seen[id(v)] = np.ascontiguousarray(np.asarray(v).astype(np.uint32, copy=False).reshape(-1))
            keep.append(seen[id(v)])
        if any(a.shape[0] != m for a in keep):
            raise ValueError("an index vector's length differs from the scalar vector's")
        return keep, [a.ctypes.data for a in keep]

    @staticmethod
    def _device_indices(indices, count: int):
        if indices is None:
            return None
        vecs = list(indices) if isinstance(indices, (list, tuple)) else [indices] * count
        if len(vecs) != count:
            raise ValueError("one index vector per scalar vector")
        for t in vecs:
            if hasattr(t, "dtype") and hasattr(t, "element_size") and t.element_size() != 4:
                raise ValueError("device indices must be a 32-bit integer tensor")
        return [_dev_ptr(t) for t in vecs]

    def compute_subset(self, scalars, first: int = 0, indices=None, window_size: Optional[int] = None,
                       run_length: Optional[int] = None, scalar_bits: Optional[int] = None, scalar_type=None,
                       m: Optional[int] = None) -> Tuple[int, int]:
        """One MSM of the m = len(scalars) host scalars over bases [first, first + m), or over
        bases indices[0..m) (a uint32 array).  A "bit" vector's m is given (or is len(indices))."""
        ty, scalar_bits = _native_type(scalars, scalar_type, scalar_bits)
        if ty:
            sc = _native_host(scalars, ty)
            m = _native_len(sc, ty, len(indices) if m is None and indices is not None else m)
        else:
            sc = np.ascontiguousarray(scalars_to_wire(scalars, scalar_bits))
            m = sc.shape[0]
        keep, ptrs = self._host_indices(indices, m, 1)
        sub = self._subset(first, m, ptrs)
        o, op = _out(16)
        _check(load().msm_bases_compute_subset(self._h or None, ctypes.byref(sub), _ptr(sc),
                                               _opts(window_size, run_length, scalar_bits=scalar_bits,
                                                     scalar_type=ty), op),
               "msm_bases_compute_subset")
        return _xy(o)

    def compute_subset_device(self, d_scalars, first: int = 0, indices=None, m: Optional[int] = None,
                              window_size: Optional[int] = None, run_length: Optional[int] = None,
                              stream: int = 0, scalar_bits: Optional[int] = None,
                              scalar_type=None) -> Tuple[int, int]:
        """The same with device-resident scalars (a torch tensor [m, 8], or a raw device pointer with
        `m`) and, in indexed form, a device-resident int32/uint32 index tensor (or pointer)."""
        ty, scalar_bits = _native_type(d_scalars, scalar_type, scalar_bits)
        _wide_device(d_scalars, ty)
        if ty == "bit" and m is None:
            raise ValueError("a bit vector's length is not its byte count: pass m")
        m = len(d_scalars) if m is None else int(m)
        sub = self._subset(first, m, self._device_indices(indices, 1))
        o, op = _out(16)
        _check(load().msm_bases_compute_subset_device(self._h or None, ctypes.byref(sub), _dev_ptr(d_scalars),
                                                      _opts(window_size, run_length, scalar_bits=scalar_bits,
                                                            scalar_type=ty),
                                                      _stream(stream, d_scalars, indices), op),
               "msm_bases_compute_subset_device")
        return _xy(o)

    def compute_subset_many(self, scalars_list, first: int = 0, indices=None, window_size: Optional[int] = None,
                            run_length: Optional[int] = None, flags: int = 0,
                            scalar_bits: Optional[int] = None, scalar_type=None,
                            m: Optional[int] = None) -> np.ndarray:
        """len(scalars_list) pipelined MSMs of host scalar vectors of one length m, over one range
        or over each MSM's own index vector (`indices`: a list of arrays, or one array for all).
        [count][16] BE words.  "bit" vectors need `m`."""
        ty, scalar_bits = _native_type(_first(scalars_list), scalar_type, scalar_bits)
        if ty:
            ks, ss = _native_list(scalars_list, ty)
            lens = [_native_len(b, ty, m) for b in ks]
        else:
            ks, ss = _host_list(scalars_list, _scalar_words(scalar_bits))
            lens = [b.shape[0] for b in ks]
        count = len(ks)
        m = lens[0] if count else 0
        if any(k != m for k in lens):
            raise ValueError("the scalar vectors of one call share their length")
        keep, ptrs = self._host_indices(indices, m, count)
        sub = self._subset(first, m, ptrs)
        o, op = _out(16 * max(count, 1))
        _check(load().msm_bases_compute_subset_many(self._h or None, ctypes.byref(sub), ctypes.cast(ss, ctypes.c_void_p),
                                                    count,
                                                    _opts(window_size, run_length, -1, flags, scalar_bits=scalar_bits,
                                                          scalar_type=ty),
                                                    op),
               "msm_bases_compute_subset_many")
        return o[:16 * count].reshape(count, 16)

    def compute_subset_many_device(self, scalars_list, first: int = 0, indices=None, m: Optional[int] = None,
                                   window_size: Optional[int] = None, run_length: Optional[int] = None,
                                   flags: int = 0, stream: int = 0, scalar_bits: Optional[int] = None,
                                   scalar_type=None) -> np.ndarray:
        """The same with device-resident scalar (and index) vectors."""
        count = len(scalars_list)
        ty, scalar_bits = _native_type(_first(scalars_list), scalar_type, scalar_bits)
        for t in scalars_list:
            _wide_device(t, ty)
        if ty == "bit" and m is None:
            raise ValueError("a bit vector's length is not its byte count: pass m")
        if m is None:
            m = len(scalars_list[0]) if count else 0
        ss = (ctypes.c_void_p * max(count, 1))(*[_dev_ptr(t) for t in scalars_list])
        sub = self._subset(first, m, self._device_indices(indices, count))
        tensors = list(scalars_list[:1]) + (list(indices[:1]) if isinstance(indices, (list, tuple)) else [indices])
        o, op = _out(16 * max(count, 1))
        _check(load().msm_bases_compute_subset_many_device(self._h or None, ctypes.byref(sub),
                                                           ctypes.cast(ss, ctypes.c_void_p), count,
                                                           _opts(window_size, run_length, -1, flags,
                                                                 scalar_bits=scalar_bits, scalar_type=ty),
                                                           _stream(stream, *tensors), op),
               "msm_bases_compute_subset_many_device")
        return o[:16 * count].reshape(count, 16)

    # ---- per-point scalar multiples (include/msm.h msm_bases_scale*) ----
    # Q_i = s_i * P_i over all the bases, the range [first, first + m) or bases indices[i] (repeats
    # allowed: zeros give the fixed-base batch s_i * P_0).  Scalars are wire words, or narrow ones with
    # `scalar_bits`; the integer is not reduced mod r.

    def _scale_subset(self, m: int, first: int, indices, host: bool):
        """The msm_subset_t of a scale call by reference (None: all the bases), and what it keeps alive."""
        if indices is None and not first and m == self.info["n"]:
            return None, None
        if indices is None:
            return ctypes.byref(self._subset(first, m, None)), None
        if host:
            keep, ptrs = self._host_indices(indices, m, 1)
        else:
            keep, ptrs = indices, self._device_indices(indices, 1)
        sub = self._subset(first, m, ptrs)
        return ctypes.byref(sub), (keep, sub)

    def scale(self, scalars, first: int = 0, indices=None, scalar_bits: Optional[int] = None) -> np.ndarray:
        """s_i * P_i for host scalars: wire records [m, 32] (x | y | t | z = 1, canonical)."""
        sc = np.ascontiguousarray(scalars_to_wire(scalars, scalar_bits))
        m = sc.shape[0]
        sub, keep = self._scale_subset(m, first, indices, True)
        out = np.zeros((m, 32), dtype=np.uint32)
        _check(load().msm_bases_scale(self._h or None, sub, _ptr(sc), _opts(None, scalar_bits=scalar_bits), _ptr(out)),
               "msm_bases_scale")
        return out

    def scale_device(self, d_scalars, d_out, m: Optional[int] = None, first: int = 0, indices=None,
                     scalar_bits: Optional[int] = None, stream: int = 0) -> None:
        """The same between device buffers (torch tensors, or raw pointers with `m`): d_out takes m x 32
        words (16-byte aligned, not overlapping the scalars); complete on return."""
        m = len(d_scalars) if m is None else int(m)
        sub, keep = self._scale_subset(m, first, indices, False)
        _check(load().msm_bases_scale_device(self._h or None, sub, _dev_ptr(d_scalars),
                                             _opts(None, scalar_bits=scalar_bits),
                                             _stream(stream, d_scalars, indices, d_out), _dev_ptr(d_out)),
               "msm_bases_scale_device")

    def scaled(self, scalars, first: int = 0, indices=None, scalar_bits: Optional[int] = None, levels: int = 0,
               window_size: Optional[int] = None) -> "Bases":
        """A new handle of the points s_i * P_i, which never leave the device: the handle
        Bases.from_wire(self.scale(...)) makes."""
        sc = np.ascontiguousarray(scalars_to_wire(scalars, scalar_bits))
        sub, keep = self._scale_subset(sc.shape[0], first, indices, True)
        h = ctypes.c_void_p()
        _check(load().msm_bases_scale_create(self._h or None, sub, _ptr(sc),
                                             _opts(window_size, scalar_bits=scalar_bits), int(levels),
                                             ctypes.byref(h)), "msm_bases_scale_create")
        return Bases(h.value or 0)

    def scaled_device(self, d_scalars, m: Optional[int] = None, first: int = 0, indices=None,
                      scalar_bits: Optional[int] = None, levels: int = 0, window_size: Optional[int] = None,
                      stream: int = 0) -> "Bases":
        """The same with device-resident scalars (and indices)."""
        m = len(d_scalars) if m is None else int(m)
        sub, keep = self._scale_subset(m, first, indices, False)
        h = ctypes.c_void_p()
        _check(load().msm_bases_scale_create_device(self._h or None, sub, _dev_ptr(d_scalars),
                                                    _opts(window_size, scalar_bits=scalar_bits), int(levels),
                                                    _stream(stream, d_scalars, indices), ctypes.byref(h)),
               "msm_bases_scale_create_device")
        return Bases(h.value or 0)

    # ---- pairwise combinations (include/msm.h msm_bases_combine*) ----
    # R_i = a_i * A_i +- b_i * B_i: the A_i are this handle's bases [a_first, a_first + m) or a_indices[i],
    # the B_i those of `other` (None: this handle again) at b_first or b_indices.  `a` and `b`: None (the
    # scalar 1), one int (the same scalar for every i), or m scalars as scalars_to_wire takes them; the
    # device calls take tensors, one row with a_broadcast / b_broadcast.  `sub` subtracts the B term.

    def _combine_args(self, other, a, b, a_first, b_first, a_indices, b_indices, m, sub, scalar_bits, host,
                      a_broadcast=False, b_broadcast=False):
        """The msm_combine_t of a call, what it keeps alive, and m."""
        oth = self if other is None else other
        flags = MSM_COMBINE_SUB if sub else 0
        sides = []
        for sc, bc, flag in ((a, a_broadcast, MSM_COMBINE_A_BROADCAST), (b, b_broadcast, MSM_COMBINE_B_BROADCAST)):
            if host and isinstance(sc, (int, np.integer)):
                sc, bc = [int(sc)], True
            if host and sc is not None:
                sc = np.ascontiguousarray(scalars_to_wire(sc, scalar_bits))
            if bc:
                flags |= flag
            sides.append((sc, bc))
        if m is None:
            lens = [len(sc) for sc, bc in sides if sc is not None and not bc]
            lens += [len(ix) for ix in (a_indices, b_indices) if ix is not None]
            m = lens[0] if lens else min(self.info["n"] - int(a_first), oth.info["n"] - int(b_first))
        m = int(m)
        for sc, bc in sides:
            if host and sc is not None and sc.shape[0] != (1 if bc else m):
                raise ValueError("a scalar array's length differs from m")
        keep, subs = [sides], []
        for first, indices in ((a_first, a_indices), (b_first, b_indices)):
            if indices is None:
                ptrs = None
            elif host:
                k, ptrs = self._host_indices(indices, m, 1)
                keep.append(k)
            else:
                ptrs = self._device_indices(indices, 1)
            subs.append(self._subset(first, m, ptrs))
        ptr = (lambda x: None if x is None else _ptr(x)) if host else (lambda x: None if x is None else _dev_ptr(x))
        cb = Combine(None if other is None else (other._h or None), subs[0], subs[1], ptr(sides[0][0]), ptr(sides[1][0]),
                     flags, 0)
        keep.append(subs)
        return cb, keep, m

    def combine(self, other=None, a=None, b=None, a_first: int = 0, b_first: int = 0, a_indices=None, b_indices=None,
                m: Optional[int] = None, sub: bool = False, scalar_bits: Optional[int] = None) -> np.ndarray:
        """a_i * A_i +- b_i * B_i for host scalars (and indices): wire records [m, 32] (x | y | t | z = 1,
        canonical)."""
        cb, keep, m = self._combine_args(other, a, b, a_first, b_first, a_indices, b_indices, m, sub, scalar_bits, True)
        out = np.zeros((m, 32), dtype=np.uint32)
        _check(load().msm_bases_combine(self._h or None, ctypes.byref(cb), _opts(None, scalar_bits=scalar_bits),
                                        _ptr(out)), "msm_bases_combine")
        return out

    def combine_device(self, d_out, other=None, a=None, b=None, a_first: int = 0, b_first: int = 0, a_indices=None,
                       b_indices=None, m: Optional[int] = None, sub: bool = False, scalar_bits: Optional[int] = None,
                       a_broadcast: bool = False, b_broadcast: bool = False, stream: int = 0) -> None:
        """The same between device buffers (torch tensors, or raw pointers with `m`): d_out takes m x 32
        words (16-byte aligned, overlapping no input); complete on return."""
        cb, keep, m = self._combine_args(other, a, b, a_first, b_first, a_indices, b_indices, m, sub, scalar_bits, False,
                                         a_broadcast, b_broadcast)
        _check(load().msm_bases_combine_device(self._h or None, ctypes.byref(cb), _opts(None, scalar_bits=scalar_bits),
                                               _stream(stream, a, b, a_indices, b_indices, d_out), _dev_ptr(d_out)),
               "msm_bases_combine_device")

    def combined(self, other=None, a=None, b=None, a_first: int = 0, b_first: int = 0, a_indices=None, b_indices=None,
                 m: Optional[int] = None, sub: bool = False, scalar_bits: Optional[int] = None, levels: int = 0,
                 window_size: Optional[int] = None) -> "Bases":
        """A new handle of the points a_i * A_i +- b_i * B_i, which never leave the device: the handle
        Bases.from_wire(self.combine(...)) makes."""
        cb, keep, m = self._combine_args(other, a, b, a_first, b_first, a_indices, b_indices, m, sub, scalar_bits, True)
        h = ctypes.c_void_p()
        _check(load().msm_bases_combine_create(self._h or None, ctypes.byref(cb),
                                               _opts(window_size, scalar_bits=scalar_bits), int(levels),
                                               ctypes.byref(h)), "msm_bases_combine_create")
        return Bases(h.value or 0)

    def combined_device(self, other=None, a=None, b=None, a_first: int = 0, b_first: int = 0, a_indices=None,
                        b_indices=None, m: Optional[int] = None, sub: bool = False, scalar_bits: Optional[int] = None,
                        a_broadcast: bool = False, b_broadcast: bool = False, levels: int = 0,
                        window_size: Optional[int] = None, stream: int = 0) -> "Bases":
        """The same with device-resident scalars (and indices)."""
        cb, keep, m = self._combine_args(other, a, b, a_first, b_first, a_indices, b_indices, m, sub, scalar_bits, False,
                                         a_broadcast, b_broadcast)
        h = ctypes.c_void_p()
        _check(load().msm_bases_combine_create_device(self._h or None, ctypes.byref(cb),
                                                      _opts(window_size, scalar_bits=scalar_bits), int(levels),
                                                      _stream(stream, a, b, a_indices, b_indices), ctypes.byref(h)),
               "msm_bases_combine_create_device")
        return Bases(h.value or 0)

    def fold(self, x, x_inv=None, levels: int = 0, window_size: Optional[int] = None) -> "Bases":
        """One folding step of an inner-product argument's generators, for an even n: the handle of
        x_inv * P_i + x * P_(i + n/2), i < n/2 (x_inv None: P_i + x * P_(i + n/2)), both scalars broadcast."""
        n = self.info["n"]
        if n % 2:
            raise ValueError("fold needs an even number of bases")
        return self.combined(a=None if x_inv is None else int(x_inv), b=int(x), b_first=n // 2, m=n // 2, levels=levels,
                             window_size=window_size)

    def points(self, first: int = 0, m: Optional[int] = None, indices=None) -> np.ndarray:
        """The wire records [m, 32] of the handle's own points (all, a range or an index list): scale by
        ones at scalar_bits = 1.  A handle made from x-coordinates has no other copy of its y."""
        if m is None:
            m = len(indices) if indices is not None else self.info["n"] - int(first)
        return self.scale(np.ones((max(int(m), 0), 1), dtype=np.uint32), first, indices, scalar_bits=1)

    def fixed_table(self, indices=None, first: Optional[int] = None, count: Optional[int] = None,
                    window_bits: int = 0, scalar_bits: int = 0) -> "FixedBase":
        """A fixed-base table (include/msm.h msm_fixed_create) of k <= 8 of the handle's bases: all of
        them, the range [first, first + count), or `indices` (repeats allowed).  window_bits 0 is the
        library's choice, scalar_bits 0 means 256.  The table keeps its own records: the handle may be
        closed at once."""
        return self._table("msm_fixed_create", indices, first, count, window_bits, scalar_bits)

    def vector_table(self, indices=None, first: Optional[int] = None, count: Optional[int] = None,
                     window_bits: int = 0, scalar_bits: int = 0) -> "FixedBase":
        """The same table over up to 4096 of the handle's bases (include/msm.h msm_fixed_create_vector),
        for many rows over the same generators: the row commitments of a matrix, batches of Pedersen
        vector commitments.  window_bits 0 keeps the table small (at most 64 MiB where a width allows)."""
        return self._table("msm_fixed_create_vector", indices, first, count, window_bits, scalar_bits)

    def _table(self, entry: str, indices, first, count, window_bits: int, scalar_bits: int) -> "FixedBase":
        if indices is not None:
            keep = np.ascontiguousarray(np.asarray(indices).astype(np.uint32, copy=False).reshape(-1))
            sub = ctypes.byref(self._subset(0, keep.shape[0], [keep.ctypes.data]))
        elif first is not None or count is not None:
            f = int(first or 0)
            sub = ctypes.byref(self._subset(f, self.info["n"] - f if count is None else int(count), None))
        else:
            sub = None
        h = ctypes.c_void_p()
        _check(getattr(load(), entry)(self._h or None, sub, int(window_bits), int(scalar_bits), None, ctypes.byref(h)),
               entry)
        return FixedBase(h.value or 0)

    def close(self) -> None:
        """Free the records.  Closing twice is harmless."""
        h, self._h = self._h, 0
        if h and _lib is not None:
            _lib.msm_bases_destroy(h)  # -1 when msm_shutdown already freed it

    def __enter__(self) -> "Bases":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter teardown: the module's globals may be gone
            pass


class FixedBase:
    """A fixed-base table of k bases B_0 .. B_(k-1) (include/msm.h msm_fixed_*), made by
    Bases.fixed_table (k <= 8) or Bases.vector_table (k <= 4096): every call computes Q_i = sum_j s_ij * B_j for m rows of k scalars, one mixed
    addition per window and base.

        with bases.fixed_table(indices=[0]) as g:
            keys = g.mul(secrets)                      # wire records [m, 32]

    Scalars are wire words [m, k, 8] (or [m * k, 8], row i's k scalars together), or narrow ones with
    `scalar_bits` no wider than the table's; Python ints are taken in the same order.  The integer is
    not reduced mod r.  Use after close() -- or after the library shut down -- raises MsmError(-1)."""

    def __init__(self, handle: int):
        self._h = handle

    @property
    def info(self) -> dict:
        inf = FixedInfo()
        _check(load().msm_fixed_info(self._h or None, ctypes.byref(inf)), "msm_fixed_info")
        return {name: int(getattr(inf, name)) for name, _ in FixedInfo._fields_ if name != "reserved"}

    def _rows(self, scalars, scalar_bits: Optional[int]) -> Tuple[np.ndarray, int]:
        """Host scalars as [m * k, sw] words, and m."""
        if not isinstance(scalars, np.ndarray):
            scalars = list(scalars)
            if scalars and isinstance(scalars[0], (list, tuple)):
                scalars = [s for row in scalars for s in row]
        sc = np.ascontiguousarray(scalars_to_wire(scalars, scalar_bits))
        k = self.info["bases"]
        if sc.shape[0] % k:
            raise ValueError(f"{sc.shape[0]} scalars are no whole rows of {k}")
        return sc, sc.shape[0] // k

    def mul(self, scalars, scalar_bits: Optional[int] = None) -> np.ndarray:
        """sum_j s_ij * B_j for host scalars: wire records [m, 32] (x | y | t | z = 1, canonical)."""
        sc, m = self._rows(scalars, scalar_bits)
        out = np.zeros((m, 32), dtype=np.uint32)
        _check(load().msm_fixed_mul(self._h or None, _ptr(sc), m, _opts(None, scalar_bits=scalar_bits), _ptr(out)),
               "msm_fixed_mul")
        return out

    def mul_device(self, d_scalars, d_out, m: Optional[int] = None, scalar_bits: Optional[int] = None,
                   stream: int = 0) -> None:
        """The same between device buffers (torch tensors, or raw pointers with `m`): d_scalars holds
        m rows of k scalars, d_out takes m x 32 words (16-byte aligned, not overlapping the scalars);
        complete on return."""
        m = len(d_out) if m is None else int(m)
        _check(load().msm_fixed_mul_device(self._h or None, _dev_ptr(d_scalars), m,
                                           _opts(None, scalar_bits=scalar_bits), _stream(stream, d_scalars, d_out),
                                           _dev_ptr(d_out)), "msm_fixed_mul_device")

    def mul_bases(self, scalars, scalar_bits: Optional[int] = None, levels: int = 0,
                  window_size: Optional[int] = None) -> Bases:
        """A new handle of the m points, which never leave the device: the handle
        Bases.from_wire(self.mul(...)) makes."""
        sc, m = self._rows(scalars, scalar_bits)
        h = ctypes.c_void_p()
        _check(load().msm_fixed_mul_create(self._h or None, _ptr(sc), m, _opts(window_size, scalar_bits=scalar_bits),
                                           int(levels), ctypes.byref(h)), "msm_fixed_mul_create")
        return Bases(h.value or 0)

    def mul_bases_device(self, d_scalars, m: int, scalar_bits: Optional[int] = None, levels: int = 0,
                         window_size: Optional[int] = None, stream: int = 0) -> Bases:
        """The same with device-resident scalars (m rows of k)."""
        h = ctypes.c_void_p()
        _check(load().msm_fixed_mul_create_device(self._h or None, _dev_ptr(d_scalars), int(m),
                                                  _opts(window_size, scalar_bits=scalar_bits), int(levels),
                                                  _stream(stream, d_scalars), ctypes.byref(h)),
               "msm_fixed_mul_create_device")
        return Bases(h.value or 0)

    def _records_handle(self) -> Bases:
        """The table's records copied into a handle of their own (msm_test_fixed_bases)."""
        h = ctypes.c_void_p()
        _check(load().msm_test_fixed_bases(self._h or None, ctypes.byref(h)), "msm_test_fixed_bases")
        return Bases(h.value or 0)

    def points(self) -> np.ndarray:
        """The table's points as wire records [records, 32]: entry (j, win, d), d = 1 .. 2^(w-1), at
        (j * windows + win) * 2^(w-1) + d - 1 holds d * 2^(w * win) * B_j."""
        with self._records_handle() as b:
            return b.points()

    def close(self) -> None:
        """Free the table.  Closing twice is harmless."""
        h, self._h = self._h, 0
        if h and _lib is not None:
            _lib.msm_fixed_destroy(h)  # -1 when msm_shutdown already freed it

    def __enter__(self) -> "FixedBase":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter teardown: the module's globals may be gone
            pass


# ---- scalar-field vectors (include/msm.h msm_fr_*) ----
# Arithmetic mod r = FR_MODULUS on vectors of 32-byte elements, in one of two forms: "wire" ([n, 8] u32,
# big-endian words: what scalars_to_wire makes and every *_device entry reads; any integer < 2^256 on
# input, canonical on output) and "fr_mont" ([n, 4] u64 or [n, 8] u32, little-endian: what
# scalars_to_wide(.., "fr_mont") makes, the memory of an arkworks Fr).  numpy arrays (and lists of ints) go
# to the host entries and come back as numpy [n, 8] uint32; torch device tensors go to the device entries
# and come back as tensors, into `out` if given (which may be the first or the second operand itself).
# Arithmetic mod r is meaningful only for bases in the prime-order subgroup (the curve has cofactor 4).

def _fr_form(form) -> int:
    if form not in FR_FORMS:
        raise ValueError(f"unknown Fr form {form!r}: one of {sorted(FR_FORMS)}")
    return FR_FORMS[form]


def _fr_on_device(v) -> bool:
    return bool(getattr(v, "is_cuda", False))


def _fr_rows(v) -> int:
    """The 32-byte elements a device tensor holds."""
    if not v.is_contiguous():
        raise ValueError("Fr vectors must be contiguous")
    nbytes = v.numel() * v.element_size()
    if nbytes % 32:
        raise ValueError("an Fr vector holds 32 bytes per element")
    return nbytes // 32


def _fr_host(v, form: str) -> np.ndarray:
    """A host vector as C-contiguous [n, 8] uint32 in `form`: an array as it is ([n, 4] uint64 for "fr_mont"),
    ints encoded (reduced mod r for "fr_mont")."""
    if isinstance(v, np.ndarray):
        if v.dtype == np.uint64 and form == "fr_mont":
            v = np.ascontiguousarray(v).view(np.uint32)
        return np.ascontiguousarray(v, dtype=np.uint32).reshape(-1, 8)
    v = list(v)
    if v and not isinstance(v[0], (int, np.integer)):  # a list of elements, 8 words each
        return np.ascontiguousarray(np.stack([np.asarray(s, dtype=np.uint32).reshape(8) for s in v]))
    vals = [int(s) for s in v]
    if form == "fr_mont":
        return scalars_to_wide([s % FR_MODULUS for s in vals], "fr_mont").view(np.uint32).reshape(-1, 8)
    return np.ascontiguousarray(scalars_to_wire(vals)).reshape(-1, 8)


def fr_to_ints(v, form: str = "wire") -> list:
    """The residues mod r of a host vector in `form` (a tensor is copied down first)."""
    _fr_form(form)
    if hasattr(v, "cpu"):
        v = v.cpu().contiguous().numpy().view(np.uint32)
    rows = _fr_host(v, form)
    if form == "wire":
        return [wire_to_int(row) % FR_MODULUS for row in rows]
    r_inv = pow(1 << 256, -1, FR_MODULUS)
    return [int.from_bytes(row.astype("<u4").tobytes(), "little") * r_inv % FR_MODULUS for row in rows]


def _fr_operand(v, form: str, like, m: int, broadcast: bool):
    """One operand of a combine call beside `like`, the first: (what to keep alive, pointer, rows, broadcast)."""
    if v is None:
        return None, None, 0, False
    if _fr_on_device(like):
        if isinstance(v, (int, np.integer)):
            import torch

            v = torch.from_numpy(_fr_host([int(v)], form).view(np.int32)).to(like.device)
        elif not _fr_on_device(v):
            raise TypeError("device and host Fr vectors in one call")
        rows = _fr_rows(v)
        ptr = _dev_ptr(v)
    else:
        if _fr_on_device(v):
            raise TypeError("device and host Fr vectors in one call")
        v = _fr_host([int(v)] if isinstance(v, (int, np.integer)) else v, form)
        rows = v.shape[0]
        ptr = _ptr(v)
    broadcast = broadcast or (rows == 1 and m != 1)
    if rows != (1 if broadcast else m):
        raise ValueError("an Fr operand's length differs from the first operand's")
    return v, ptr, rows, broadcast


def fr_combine(a, b=None, x=None, y=None, sub: bool = False, form: str = "wire", out_form: Optional[str] = None,
               out=None, x_broadcast: bool = False, y_broadcast: bool = False, device: int = -1, stream: int = 0):
    """out_i = x_i * a_i +- y_i * b_i mod r.  b None: no second term.  x and y: None (1), one int or a
    one-row vector (the same multiplier for every i), or a vector as long as a.  `form` is the form of
    every operand, `out_form` (None: the same) that of the result."""
    out_form = form if out_form is None else out_form
    fi, fo = _fr_form(form), _fr_form(out_form)
    dev = _fr_on_device(a)
    if not dev:
        a = _fr_host(a, form)
    m = _fr_rows(a) if dev else a.shape[0]
    kb, pb, rb, _ = _fr_operand(b, form, a, m, False)
    if b is not None and rb != m:
        raise ValueError("an Fr operand's length differs from the first operand's")
    kx, px, _, bx = _fr_operand(x, form, a, m, x_broadcast)
    ky, py, _, by = _fr_operand(y, form, a, m, y_broadcast)
    flags = (MSM_FR_SUB if sub else 0) | (MSM_FR_X_BROADCAST if bx else 0) | (MSM_FR_Y_BROADCAST if by else 0)
    if dev:
        if out is None:
            import torch

            out = torch.empty_like(a) if fi == fo else torch.empty((m, 8), dtype=torch.int32, device=a.device)
        elif not _fr_on_device(out) or _fr_rows(out) != m:
            raise ValueError("out must be a device tensor of the first operand's length")
        cb = FrCombine(_dev_ptr(a) if m else None, pb, px, py, flags, fi, fo, 0)
        _check(load().msm_fr_combine_device(ctypes.byref(cb), m, _opts(None, device=a.device.index),
                                            _stream(stream, a, kb, kx, ky, out), _dev_ptr(out)),
               "msm_fr_combine_device")
        return out
    if out is not None:
        raise ValueError("out= is for device tensors")
    res = np.zeros((m, 8), dtype=np.uint32)
    cb = FrCombine(_ptr(a), pb, px, py, flags, fi, fo, 0)
    _check(load().msm_fr_combine(ctypes.byref(cb), m, _opts(None, device=device), _ptr(res)), "msm_fr_combine")
    return res


def fr_fold(a, x, x_inv=None, form: str = "wire", out_form: Optional[str] = None, out=None, device: int = -1,
            stream: int = 0):
    """One folding step of an inner-product argument's witness, for an even n: a'_i = x * a_i + x_inv *
    a_(i + n/2), i < n/2 (x_inv None: x * a_i + a_(i + n/2)) -- the scalars that go with Bases.fold(x, x_inv).
    `out` may be the low half itself (a[:n // 2] of a device tensor)."""
    if not _fr_on_device(a):
        a = _fr_host(a, form)
    n = _fr_rows(a) if _fr_on_device(a) else a.shape[0]
    if n % 2:
        raise ValueError("fold needs an even number of elements")
    rows = a.reshape(n, -1)
    return fr_combine(rows[:n // 2], rows[n // 2:], x=x, y=x_inv, form=form, out_form=out_form, out=out, x_broadcast=True,
                      y_broadcast=x_inv is not None, device=device, stream=stream)


def fr_mul(a, x, form: str = "wire", out_form: Optional[str] = None, out=None, device: int = -1, stream: int = 0):
    """x_i * a_i mod r: a Hadamard product for a vector x, a scaling for one int or a one-row x."""
    return fr_combine(a, x=x, form=form, out_form=out_form, out=out, device=device, stream=stream)


def fr_convert(a, form: str, out_form: str, out=None, device: int = -1, stream: int = 0):
    """`a` in the other form: "fr_mont" to "wire" is the route from arkworks Fr memory to the scalars the
    scale, fixed-base and combine entries read; "wire" to "wire" reduces 256-bit integers mod r."""
    return fr_combine(a, form=form, out_form=out_form, out=out, device=device, stream=stream)


def fr_powers(g: int, n: int, first: Optional[int] = None, out_form: str = "wire", out=None,
              device: Optional[int] = None, stream: int = 0):
    """first * g^i mod r for i < n (first None: 1).  A numpy [n, 8] uint32 from the host entry; with `device`
    (a HIP ordinal) or a device tensor `out`, a device tensor from the device entry, which never leaves it:
    table.mul_bases_device(fr_powers(tau, n, device=0), n) is an SRS."""
    fo = _fr_form(out_form)
    n = int(n)
    gw = scalars_to_wire([int(g) % (1 << 256)])
    cw = None if first is None else scalars_to_wire([int(first) % (1 << 256)])
    cp = None if cw is None else _ptr(cw)
    if out is None and device is None:
        res = np.zeros((n, 8), dtype=np.uint32)
        _check(load().msm_fr_powers(_ptr(gw), cp, n, fo, _opts(None), _ptr(res)), "msm_fr_powers")
        return res
    if out is None:
        import torch

        out = torch.empty((n, 8), dtype=torch.int32, device=f"cuda:{int(device)}")
    elif not _fr_on_device(out) or _fr_rows(out) != n:
        raise ValueError("out must be a device tensor of n elements")
    _check(load().msm_fr_powers_device(_ptr(gw), cp, n, fo, _opts(None, device=out.device.index),
                                       _stream(stream, out), _dev_ptr(out)), "msm_fr_powers_device")
    return out


def fr_dot(a, b=None, form: str = "wire", out_form: Optional[str] = None, device: int = -1, stream: int = 0) -> np.ndarray:
    """sum_i a_i * b_i mod r (b None: sum_i a_i) as one element in `out_form` (None: `form`): a numpy [8]
    uint32 on the host, whichever entry computed it (fr_to_ints([result], out_form)[0] is its residue)."""
    out_form = form if out_form is None else out_form
    fi, fo = _fr_form(form), _fr_form(out_form)
    res = np.zeros(8, dtype=np.uint32)
    rp = res.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    if _fr_on_device(a):
        n = _fr_rows(a)
        if b is not None and (not _fr_on_device(b) or _fr_rows(b) != n):
            raise ValueError("b must be a device tensor as long as a")
        _check(load().msm_fr_dot_device(_dev_ptr(a) if n else None, None if b is None else _dev_ptr(b), n, fi, fo,
                                        _opts(None, device=a.device.index), _stream(stream, a, b), rp),
               "msm_fr_dot_device")
        return res
    a = _fr_host(a, form)
    if b is not None:
        b = _fr_host(b, form)
        if b.shape[0] != a.shape[0]:
            raise ValueError("b must be as long as a")
    _check(load().msm_fr_dot(_ptr(a), None if b is None else _ptr(b), a.shape[0], fi, fo, _opts(None, device=device), rp),
           "msm_fr_dot")
    return res


def _fr_word(c: Optional[int]):
    """One int as the 8 wire words the entries take for `c` (None: NULL, the factor 1)."""
    return None if c is None else scalars_to_wire([int(c) % (1 << 256)])


def _fr_unary(host_name: str, dev_name: str, a, cw, extra: tuple, form: str, out_form: Optional[str], out, device: int,
              stream: int, grid_cap: Optional[int] = None):
    """The calling convention of msm_fr_inverse* and msm_fr_scan* (`extra`: the words between m and the
    forms): numpy in, numpy out through the host entry; a device tensor in, a device tensor out -- `out`
    if given, which may be `a` itself -- through the device entry, or its test hook with `grid_cap`."""
    out_form = form if out_form is None else out_form
    fi, fo = _fr_form(form), _fr_form(out_form)
    cp = None if cw is None else _ptr(cw)
    L = load()
    if _fr_on_device(a):
        m = _fr_rows(a)
        if out is None:
            import torch

            out = torch.empty_like(a) if fi == fo else torch.empty((m, 8), dtype=torch.int32, device=a.device)
        elif not _fr_on_device(out) or _fr_rows(out) != m:
            raise ValueError("out must be a device tensor of the operand's length")
        pa = _dev_ptr(a) if m else None
        if grid_cap is not None:
            _check(getattr(L, "msm_test_" + dev_name[4:])(pa, cp, m, *extra, fi, fo, int(grid_cap), _dev_ptr(out)),
                   "msm_test_" + dev_name[4:])
        else:
            _check(getattr(L, dev_name)(pa, cp, m, *extra, fi, fo, _opts(None, device=a.device.index), _stream(stream, a, out),
                                        _dev_ptr(out)), dev_name)
        return out
    if out is not None or grid_cap is not None:
        raise ValueError("out= is for device tensors")
    a = _fr_host(a, form)
    res = np.zeros((a.shape[0], 8), dtype=np.uint32)
    _check(getattr(L, host_name)(_ptr(a), cp, a.shape[0], *extra, fi, fo, _opts(None, device=device), _ptr(res)), host_name)
    return res


def fr_inverse(a, scale: Optional[int] = None, form: str = "wire", out_form: Optional[str] = None, out=None,
               device: int = -1, stream: int = 0):
    """scale * a_i^-1 mod r (scale None: 1), and 0 where a_i is 0 mod r -- arkworks' batch_inversion_and_mul.
    `out` may be the device tensor `a` itself."""
    return _fr_unary("msm_fr_inverse", "msm_fr_inverse_device", a, _fr_word(scale), (), form, out_form, out, device, stream)


def fr_cumprod(a, first: Optional[int] = None, exclusive: bool = False, form: str = "wire", out_form: Optional[str] = None,
               out=None, device: int = -1, stream: int = 0):
    """The running product first * a_0 * .. * a_i (first None: 1); exclusive: first * a_0 * .. * a_(i-1), which
    starts at `first`.  `out` may be the device tensor `a` itself."""
    return _fr_unary("msm_fr_scan", "msm_fr_scan_device", a, _fr_word(first), (MSM_FR_SCAN_EXCLUSIVE if exclusive else 0,),
                     form, out_form, out, device, stream)


def fr_cumsum(a, exclusive: bool = False, form: str = "wire", out_form: Optional[str] = None, out=None, device: int = -1,
              stream: int = 0):
    """The running sum a_0 + .. + a_i; exclusive: a_0 + .. + a_(i-1), which starts at 0."""
    return _fr_unary("msm_fr_scan", "msm_fr_scan_device", a, None,
                     (MSM_FR_SCAN_SUM | (MSM_FR_SCAN_EXCLUSIVE if exclusive else 0),), form, out_form, out, device, stream)


def fr_tensor(pairs, first: Optional[int] = None, out_form: str = "wire", out=None, device: Optional[int] = None,
              stream: int = 0):
    """first * prod_j (bit_j(i) ? hi_j : lo_j) mod r for i < 2^k, from k pairs (lo_j, hi_j) of ints, pair j on
    bit j of the index (first None: 1).  A numpy [2^k, 8] uint32 from the host entry; with `device` (a HIP
    ordinal) or a device tensor `out`, a device tensor from the device entry, as fr_powers."""
    fo = _fr_form(out_form)
    pairs = [(int(lo) % (1 << 256), int(hi) % (1 << 256)) for lo, hi in pairs]
    k = len(pairs)
    if k > 31:
        raise MsmError(-1, "msm_fr_tensor")
    n = 1 << k
    lo = scalars_to_wire([p[0] for p in pairs] or [0])
    hi = scalars_to_wire([p[1] for p in pairs] or [0])
    cw = _fr_word(first)
    cp = None if cw is None else _ptr(cw)
    if out is None and device is None:
        res = np.zeros((n, 8), dtype=np.uint32)
        _check(load().msm_fr_tensor(_ptr(lo), _ptr(hi), k, cp, fo, _opts(None), _ptr(res)), "msm_fr_tensor")
        return res
    if out is None:
        import torch

        out = torch.empty((n, 8), dtype=torch.int32, device=f"cuda:{int(device)}")
    elif not _fr_on_device(out) or _fr_rows(out) != n:
        raise ValueError("out must be a device tensor of 2^k elements")
    _check(load().msm_fr_tensor_device(_ptr(lo), _ptr(hi), k, cp, fo, _opts(None, device=out.device.index),
                                       _stream(stream, out), _dev_ptr(out)), "msm_fr_tensor_device")
    return out


def compute_msm_many(points_list, scalars_list, n: int, window_size: Optional[int] = None,
                     run_length: Optional[int] = None, device: int = -1, flags: int = 0,
                     devices: Optional[Sequence[int]] = None) -> np.ndarray:
    """len(points_list) independent n-point MSMs of HOST arrays (wire [n, 32] / [n, 8] each),
    uploaded into libmsm's in-flight launch slots while the others compute.  [count][16]."""
    L = load()
    count = len(points_list)
    if len(scalars_list) != count:
        raise ValueError("points_list and scalars_list differ in length")
    kp, pp = _host_list(points_list, 32)
    ks, ss = _host_list(scalars_list, 8)
    for a, b in zip(kp, ks):
        if a.shape[0] < n or b.shape[0] < n:
            raise ValueError("an input holds fewer than n points/scalars")
    o, op = _out(16 * max(count, 1))
    _check(L.msm_compute_many(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(ss, ctypes.c_void_p), n, count,
                              _opts(window_size, run_length, device, flags, devices), op), "msm_compute_many")
    return o[:16 * count].reshape(count, 16)


def compute_msm_shared(points_wire, scalars_list, n: Optional[int] = None, window_size: Optional[int] = None,
                       run_length: Optional[int] = None, device: int = -1, flags: int = 0,
                       devices: Optional[Sequence[int]] = None) -> np.ndarray:
    """Prover batch of HOST arrays: one base vector [n, 32], len(scalars_list) scalar vectors
    [n, 8]; the base vector is uploaded and prepared once.  [count][16]."""
    L = load()
    pts = np.ascontiguousarray(_u32(points_wire).reshape(-1, 32))
    n = pts.shape[0] if n is None else n
    ks, ss = _host_list(scalars_list, 8)
    if pts.shape[0] < n or any(b.shape[0] < n for b in ks):
        raise ValueError("an input holds fewer than n points/scalars")
    count = len(ks)
    o, op = _out(16 * max(count, 1))
    _check(L.msm_compute_shared(_ptr(pts), ctypes.cast(ss, ctypes.c_void_p), n, count,
                                _opts(window_size, run_length, device, flags, devices), op), "msm_compute_shared")
    return o[:16 * count].reshape(count, 16)


def compute_msm_cpu(points_wire, scalars_wire, window_size: Optional[int] = None,
                    threads: int = 0) -> Tuple[int, int]:
    """The reference's CPU-only path (cpuWorkRatio = 1, msm_end_to_end lib.rs:106-121) as
    libmsm's own multithreaded host Pippenger (msm_compute_cpu).  Explicit; never a fallback."""
    L = load()
    pts = _u32(points_wire).reshape(-1, 32)
    sc = _u32(scalars_wire).reshape(-1, 8)
    n = min(pts.shape[0], sc.shape[0])
    pts, sc = np.ascontiguousarray(pts[:n]), np.ascontiguousarray(sc[:n])
    o, op = _out(16)
    _check(L.msm_compute_cpu(_ptr(pts), _ptr(sc), n, int(window_size or 0), int(threads), op), "msm_compute_cpu")
    return _xy(o)


def compute_msm_many_device_partial(points_list, scalars_list, n: int, window_size: Optional[int] = None,
                                    run_length: Optional[int] = None, device: int = -1,
                                    stream: int = 0, flags: int = 0,
                                    windows: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """compute_msm_many_device, each result as a projective X|Y|T|Z partial: [count][32] BE words."""
    L = load()
    count = len(points_list)
    if len(scalars_list) != count:
        raise ValueError("points_list and scalars_list differ in length")
    pp = (ctypes.c_void_p * max(count, 1))(*[_dev_ptr(t) for t in points_list])
    ss = (ctypes.c_void_p * max(count, 1))(*[_dev_ptr(t) for t in scalars_list])
    o, op = _out(32 * max(count, 1))
    _check(L.msm_compute_many_device_partial(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(ss, ctypes.c_void_p), n,
                                             count, _opts(window_size, run_length, device, flags, windows=windows),
                                             _stream(stream, _first(points_list), _first(scalars_list)), op),
           "msm_compute_many_device_partial")
    return o[:32 * count].reshape(count, 32)


def combine_partials(partials: np.ndarray) -> Tuple[int, int]:
    L = load()
    p = _u32(partials).reshape(-1, 32)
    o, op = _out(16)
    _check(L.msm_combine_partials(_ptr(p), p.shape[0], op), "msm_combine_partials")
    return _xy(o)


def combine_partials_many(parts: np.ndarray):
    """parts [world, K, 32] (an all_gather of K partials per rank) -> the K joined affine results."""
    L = load()
    p = np.ascontiguousarray(_u32(parts))
    world, count = p.shape[0], p.shape[1]
    o, op = _out(16 * max(count, 1))
    _check(L.msm_combine_partials_many(_ptr(p.reshape(-1)), world, count, op), "msm_combine_partials_many")
    return [_xy(o[16 * k: 16 * k + 16]) for k in range(count)]


def point_add_affine(a: Tuple[int, int], b: Tuple[int, int]) -> Tuple[int, int]:
    """point_add_affine (lib.rs:240-253)."""
    L = load()
    aw = np.frombuffer(_int_be_words(a[0]) + _int_be_words(a[1]), dtype=">u4").astype(np.uint32)
    bw = np.frombuffer(_int_be_words(b[0]) + _int_be_words(b[1]), dtype=">u4").astype(np.uint32)
    o, op = _out(16)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    _check(L.msm_point_add_affine(aw.ctypes.data_as(u32p), bw.ctypes.data_as(u32p), op), "msm_point_add_affine")
    return _xy(o)


def split_dynamic(window_size: int, scalars_wire: np.ndarray) -> np.ndarray:
    """split_dynamic (lib.rs:196-202): [n_windows * n] u32, window 0 most significant."""
    L = load()
    sc = _u32(scalars_wire).reshape(-1, 8)
    nw = L.msm_split_windows(window_size)
    o, op = _out(max(nw * sc.shape[0], 1))
    _check(L.msm_split(window_size, _ptr(sc), sc.shape[0], op), "msm_split")
    return o[: nw * sc.shape[0]]


BENCH_G = (2796670805570508460920584878396618987767121022598342527208237783066948667246,
           8134280397689638111748378379571739274369602049665521098046934931245960532166)
XORSHIFT_SEED = 0x9E3779B97F4A7C15


def gen_points(n: int, k0: int = 1, step: int = 1, base: Tuple[int, int] = BENCH_G) -> np.ndarray:
    """Wire points [n, 32]: (k0 + i*step) * base (the benchmark page's fixed base, AllBenchmarks.tsx:111-119)."""
    L = load()
    g = np.frombuffer(_int_be_words(base[0]) + _int_be_words(base[1]), dtype=">u4").astype(np.uint32)
    o, op = _out(max(n, 1) * 32)
    _check(L.msm_gen_points(g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), k0, step, n, op), "msm_gen_points")
    return o[: n * 32].reshape(n, 32)


def gen_scalars(n: int, seed: int = XORSHIFT_SEED) -> np.ndarray:
    """Scalars [n, 8] BE: xorshift64(13,7,17), 4 words each (first most significant), mod p."""
    L = load()
    o, op = _out(max(n, 1) * 8)
    _check(L.msm_gen_scalars(seed, n, op), "msm_gen_scalars")
    return o[: n * 8].reshape(n, 8)


def set_profiling(enable=True) -> None:
    """0/False: off.  1/True: hipEvents between every phase (eager launches).  2: k_accumulate and
    the device total only, keeping the captured-graph replay (what bench.py times)."""
    mode = int(enable) if not isinstance(enable, bool) else (1 if enable else 0)
    _check(load().msm_set_profiling(mode), "msm_set_profiling")


def last_profile() -> dict:
    prof = MsmProfile()
    _check(load().msm_last_profile(ctypes.byref(prof)), "msm_last_profile")
    return {name: getattr(prof, name) for name, _ in MsmProfile._fields_}


def device_count() -> int:
    return int(load().msm_device_count())


def device_ordinals() -> list:
    """HIP ordinals of the visible gfx950 devices (msm_device_ordinal)."""
    L = load()
    return [int(L.msm_device_ordinal(i)) for i in range(int(L.msm_device_count()))]


def _test_field_op(op: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Device field op on canonical little-endian word arrays [n, 8] (test hook)."""
    L = load()
    a = _u32(a).reshape(-1, 8)
    b = _u32(b).reshape(-1, 8)
    o, op_ = _out(a.size)
    _check(L.msm_test_field_op(op, _ptr(a), _ptr(b), op_, a.shape[0]), "msm_test_field_op")
    return o.reshape(-1, 8)


def _test_point_op(op: int, p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """Device point op on affine LE word arrays [n, 16] -> projective std LE words [n, 32] (test hook)."""
    L = load()
    p = _u32(p).reshape(-1, 16)
    q = _u32(q).reshape(-1, 16)
    o, op_ = _out(p.shape[0] * 32)
    _check(L.msm_test_point_op(op, _ptr(p), _ptr(q), op_, p.shape[0]), "msm_test_point_op")
    return o.reshape(-1, 32)


# Raw-limb test hooks (csrc/msm_kernels.hip LimbOp): name -> (op, words of a, of b, of the output)
# per element.  Limbs go in and come out as they are, neither converted nor reduced.
_LIMB_OPS = {name: (i, wa, wb, wo) for i, (name, wa, wb, wo) in enumerate((
    ("mul_all", 9, 9, 9), ("mul_gh", 9, 9, 9), ("mul_eh", 9, 9, 9), ("mul_ef", 9, 9, 9), ("mul_gheh", 9, 9, 9),
    ("mul_sd_u", 9, 9, 9), ("mul_sd_s", 9, 9, 9), ("mul_2d", 9, 0, 9), ("mul_d", 9, 0, 9), ("sub", 9, 9, 9),
    ("neg", 9, 0, 9), ("add_n", 9, 9, 9), ("dbl_n", 9, 0, 9), ("to_std", 9, 0, 9), ("to_host_mont", 9, 0, 9),
    ("inv", 9, 0, 9), ("from_words", 8, 0, 9), ("to_words", 9, 0, 8), ("words_lt_p", 8, 0, 1),
    ("pt_add", 36, 36, 36), ("pt_dbl", 36, 0, 36), ("pt_madd", 36, 27, 36), ("pt_add_quad", 36, 36, 36),
    ("sqr", 9, 0, 9), ("std_neg", 9, 0, 9), ("is_one", 9, 0, 1), ("sqrt_ts", 9, 0, 9),
    ("from_record", 32, 0, 36), ("mul_order", 36, 0, 36), ("shift_lane", 32, 1, 32)))}


def _test_wide_masks() -> Tuple[int, int, int, int]:
    """The (WIDE_ALL, WIDE_GH, WIDE_EH, WIDE_EF) reduction masks the loaded library was built with
    (fp29.cuh; all zero in an MSM_NARROW_DIGITS build).  No GPU needed."""
    o, op_ = _out(4)
    _check(load().msm_test_wide_masks(op_), "msm_test_wide_masks")
    return tuple(int(x) for x in o)


def _test_decompress_constants() -> dict:
    """k_decompress_x's constants as the library holds them (tests/test_sqrt_model.py recomputes them)."""
    o, op = _out(28)
    _check(load().msm_test_decompress_constants(op), "msm_test_decompress_constants")
    le = lambda w: sum(int(v) << (32 * i) for i, v in enumerate(w))  # noqa: E731
    return {"two_adicity": int(o[0]), "exp_words": int(o[1]), "order_bits": int(o[2]), "exp": le(o[3:11]),
            "order": le(o[11:19]), "omega_mont_limbs": [int(v) for v in o[19:28]]}


def _test_scale_digits(value: int, scalar_bits: int) -> list:
    """The scale ladder's windows of one `scalar_bits`-bit value, least significant first, by the
    kernel's own digit function run on the host (msm_test_scale_digits); their number is the ladder's
    trip count.  Needs no device."""
    sc = scalars_to_wire([int(value)], scalar_bits)
    digits = np.zeros(256, dtype=np.uint32)
    count = ctypes.c_uint32()
    _check(load().msm_test_scale_digits(_ptr(sc), sc.shape[1], int(scalar_bits),
                                        digits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(count)),
           "msm_test_scale_digits")
    return [int(d) for d in digits[:count.value]]


def _test_combine_digits(a: int, b: int, scalar_bits: int) -> list:
    """The joint ladder's digits of the `scalar_bits`-bit values a and b, least significant first (bit j of
    a + 2 * bit j of b), by the kernel's own digit function run on the host (msm_test_combine_digits);
    their number is the ladder's trip count.  Needs no device."""
    sa, sb = scalars_to_wire([int(a)], scalar_bits), scalars_to_wire([int(b)], scalar_bits)
    digits = np.zeros(256, dtype=np.uint32)
    count = ctypes.c_uint32()
    _check(load().msm_test_combine_digits(_ptr(sa), _ptr(sb), sa.shape[1], int(scalar_bits),
                                          digits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(count)),
           "msm_test_combine_digits")
    return [int(d) for d in digits[:count.value]]


def _test_fixed_digits(value: int, scalar_bits: int, window_bits: int) -> Tuple[list, int]:
    """The fixed-base evaluation's signed digits of one `scalar_bits`-bit value for windows of
    `window_bits` bits, least significant first, by the kernel's own digit function run on the host
    (msm_test_fixed_digits), and the carry out of the top window.  Needs no device."""
    sc = scalars_to_wire([int(value)], scalar_bits)
    digits = np.zeros(257, dtype=np.int32)
    count, carry = ctypes.c_uint32(), ctypes.c_uint32()
    _check(load().msm_test_fixed_digits(_ptr(sc), sc.shape[1], int(scalar_bits), int(window_bits),
                                        digits.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(count),
                                        ctypes.byref(carry)), "msm_test_fixed_digits")
    return [int(d) for d in digits[:count.value]], int(carry.value)


def _test_fixed_plan(bases: int, window_bits: int = 0, scalar_bits: int = 0) -> dict:
    """The shape msm_fixed_create gives a table (msm_test_fixed_plan): window and scalar widths, windows
    per base, records and bytes.  The creation's refusals apply (MsmError -1).  Needs no device."""
    o, op_ = _out(7)
    _check(load().msm_test_fixed_plan(int(bases), int(window_bits), int(scalar_bits), op_), "msm_test_fixed_plan")
    return {"window_bits": int(o[0]), "scalar_bits": int(o[1]), "windows": int(o[2]),
            "records": int(o[3]) | int(o[4]) << 32, "bytes": int(o[5]) | int(o[6]) << 32}


def _test_vector_plan(bases: int, window_bits: int = 0, scalar_bits: int = 0, m: int = 0, sw: int = 8) -> dict:
    """The shape msm_fixed_create_vector gives a table (msm_test_vector_plan), as _test_fixed_plan's, and
    with m > 0 how a call of m rows of sw-word scalars on it is cut: bases per part G, parts P, the
    fold's passes, a slab's rows and the partial buffer's bytes.  Needs no device."""
    o, op_ = _out(14)
    _check(load().msm_test_vector_plan(int(bases), int(window_bits), int(scalar_bits), int(m), int(sw), op_),
           "msm_test_vector_plan")
    plan = {"window_bits": int(o[0]), "scalar_bits": int(o[1]), "windows": int(o[2]),
            "records": int(o[3]) | int(o[4]) << 32, "bytes": int(o[5]) | int(o[6]) << 32}
    if m:
        plan.update(G=int(o[7]), P=int(o[8]), passes=int(o[9]), slab_rows=int(o[10]) | int(o[11]) << 32,
                    part_bytes=int(o[12]) | int(o[13]) << 32)
    return plan


def _test_vector_slab(max_bytes: int = 0) -> None:
    """Caps the partial buffer of the vector tables' calls that follow (msm_test_vector_slab), so that a
    small call runs as several slabs of rows; 0 restores the library's 256 MiB."""
    load().msm_test_vector_slab(int(max_bytes))


def _test_vector_group(g: int = 0) -> None:
    """Makes every vector-table call that follows take `g` bases per part (msm_test_vector_group; clipped
    to what the scalars' width allows); 0 restores the library's rule."""
    load().msm_test_vector_group(int(g))


# msm_test_host_field's ops (csrc/host_test_hooks.h): name -> (op, takes b, works on points)
_HOST_FIELD_OPS = {name: (i, two, pt) for i, (name, two, pt) in enumerate((
    ("mul", True, False), ("mul_n3", True, False), ("mul_n4", True, False), ("add", True, False), ("sub", True, False),
    ("inv", False, False), ("from_std", False, False), ("to_std", False, False), ("div2k_1", False, False),
    ("div2k_32", False, False), ("div2k_63", False, False), ("pt_add", True, True), ("pt_add_no_t", True, True),
    ("pt_dbl", False, True), ("pt_dbl_n1", False, True), ("pt_dbl_n2", False, True), ("pt_dbl_n5", False, True)))}


def _test_host_field(name: str, a, b=None) -> list:
    """hostfield.h's function `name` (_HOST_FIELD_OPS) on raw representatives below p: Python ints, the
    integer an Fq's four limbs hold (msm_test_host_field); points are (X, Y, T, Z) tuples of them.
    Returns ints, or tuples of four.  Needs no device."""
    op, two, pt = _HOST_FIELD_OPS[name]
    w = 4 if pt else 1

    def pack(vals):
        flat = [c for v in vals for c in v] if pt else list(vals)
        return np.array([(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for v in flat for k in range(4)], dtype=np.uint64)

    av = pack(a)
    n = av.size // (4 * w)
    bv = pack(b) if two else None
    if two and bv.size != av.size:
        raise ValueError("a and b differ in length")
    out = np.zeros(av.size, dtype=np.uint64)
    _check(load().msm_test_host_field(op, av.ctypes.data, bv.ctypes.data if two else None, out.ctypes.data, n),
           "msm_test_host_field")
    vals = [sum(int(x) << (64 * k) for k, x in enumerate(out[4 * i: 4 * i + 4])) for i in range(n * w)]
    return [tuple(vals[4 * i: 4 * i + 4]) for i in range(n)] if pt else vals


def _test_fixed_proj(m: int) -> np.ndarray:
    """What the last fixed-base evaluation of m points on the default device left in its slot
    (msm_test_fixed_proj; nothing is launched): [ceil(m / 64) * 64, 27] limbs X | Y | Z per lane,
    the lanes past m included."""
    nblk = (int(m) + 63) // 64
    o, op_ = _out(nblk * 27 * 64)
    _check(load().msm_test_fixed_proj(op_, int(m)), "msm_test_fixed_proj")
    return np.ascontiguousarray(o.reshape(nblk, 27, 64).transpose(0, 2, 1)).reshape(nblk * 64, 27)


def _test_limb_op(name: str, a, b=None, neg=None) -> np.ndarray:
    """Device op `name` (_LIMB_OPS) on raw u32 limb arrays: a [n, wa], b [n, wb] for the two-operand
    ops (shift_lane: the doublings of each record, at most 255), neg [n] negate flags for pt_madd
    -> [n, wo] (test hook)."""
    op, wa, wb, wo = _LIMB_OPS[name]
    a = _u32(a).reshape(-1, wa)
    n = a.shape[0]
    b = _u32(b).reshape(n, wb) if wb else None
    neg = _u32(neg).reshape(n) if name == "pt_madd" else None
    o, op_ = _out(n * wo)
    _check(load().msm_test_limb_op(op, _ptr(a), _ptr(b) if wb else None, _ptr(neg) if neg is not None else None,
                                   op_, n), "msm_test_limb_op")
    return o.reshape(n, wo)


def _test_records(fmt: int, points, entries=(), acc=None) -> Tuple[np.ndarray, int, np.ndarray]:
    """k_prepare_points on `points` (BE words; fmt 0: 32-word wire records x|y|t|z, 1: x|y, 2: x|y|z)
    -> (records [n, 32], device error word, sums [m, 36]): the sums are acc[j] + the record of
    entries[j] (index << 1 | sign) through load_pre_signed and pt_madd on raw limbs (test hook)."""
    w = {0: 32, 1: 16, 2: 24}[fmt]
    pts = _u32(points).reshape(-1, w)
    n = pts.shape[0]
    ents = _u32(entries).reshape(-1)
    m = ents.shape[0]
    accs = _u32(acc if m else []).reshape(m, 36)
    rec, rec_ = _out(n * 32)
    err, err_ = _out(1)
    o, op_ = _out(max(m, 1) * 36)
    _check(load().msm_test_records(fmt, _ptr(pts), n, rec_, err_, _ptr(ents), _ptr(accs), op_, m), "msm_test_records")
    return rec.reshape(n, 32), int(err[0]), o.reshape(-1, 36)[:m]


def _test_bases_plan(n: int, levels: int, window_size: int = 0) -> dict:
    """The fold geometry of a `levels`-level handle (msm_test_bases_plan): window width c, windows
    per folded MSM, chunk bits S, points of the folded problem.  No GPU needed."""
    o, op_ = _out(4)
    _check(load().msm_test_bases_plan(n, levels, window_size, op_), "msm_test_bases_plan")
    return dict(zip(("c", "windows", "chunk_bits", "points"), (int(v) for v in o)))


def _test_narrow_plan(n: int, scalar_bits: int, window_size: int = 0) -> dict:
    """The geometry of a narrow-scalar launch (msm_test_narrow_plan; no GPU needed): the widest
    window c, the windows W', the base width q, the nhi windows of q + 1 bits, the words per scalar
    and the packed flag.  254 bits and more report the plain launch's (8 words, overflow window
    included in `windows`)."""
    out = np.zeros(6, np.uint32)
    _check(load().msm_test_narrow_plan(n, int(scalar_bits), int(window_size),
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), "msm_test_narrow_plan")
    return dict(zip(("c", "windows", "q", "nhi", "words", "packed"), (int(v) for v in out)))


def _test_wide_plan(n: int, scalar_type, scalar_bits: int, window_size: int = 0) -> dict:
    """The plan of a wide-type launch (msm_test_wide_plan; no GPU needed): _test_narrow_plan's fields for
    scalar_bits, plus vector_bytes and region_bytes.  `scalar_type` is a WIDE_TYPES name or a raw
    MSM_FIELD_* value."""
    out = np.zeros(8, dtype=np.uint32)
    ty = WIDE_TYPES[scalar_type][0] if isinstance(scalar_type, str) else int(scalar_type)
    _check(load().msm_test_wide_plan(n, ty, int(scalar_bits), int(window_size),
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), "msm_test_wide_plan")
    return dict(zip(("c", "windows", "q", "nhi", "words", "packed", "vector_bytes", "region_bytes"),
                    (int(v) for v in out)))


def _test_fr_from_mont(values) -> Tuple[list, list]:
    """csrc/fr.cuh on the host (msm_test_fr_from_mont; no GPU needed): for every 256-bit int a, whether a < r
    and a 2^-256 mod r.  Returns (decoded ints, canonical flags)."""
    vals = [int(v) for v in values]
    buf = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u4").astype(np.uint32)
    out = np.zeros_like(buf)
    ok = np.zeros(len(vals), dtype=np.uint8)
    _check(load().msm_test_fr_from_mont(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(vals),
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                        ok.ctypes.data_as(ctypes.c_void_p)), "msm_test_fr_from_mont")
    raw = out.astype("<u4").tobytes()
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(vals))], [bool(x) for x in ok]


_FR_OPS = {"mont_mul": 0, "add": 1, "sub": 2, "to_mont": 3, "round_trip": 4}


def _test_fr_op(name: str, a, b=None) -> list:
    """csrc/fr.cuh's arithmetic on the host (msm_test_fr_op; no GPU needed), on 256-bit ints: "mont_mul" a b
    2^-256 mod r (b < r), "add" and "sub" (a, b < r), "to_mont" a 2^256 mod r, "round_trip" fr_from_mont of it."""
    av = [int(v) for v in a]
    bv = [0] * len(av) if b is None else [int(v) for v in b]
    pack = lambda vals: np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u4").astype(np.uint32)
    pa, pb = pack(av), pack(bv)
    out = np.zeros_like(pa)
    _check(load().msm_test_fr_op(_FR_OPS[name], _ptr(pa), _ptr(pb), _ptr(out), len(av)), "msm_test_fr_op")
    raw = out.astype("<u4").tobytes()
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(av))]


def _test_fr_constants() -> dict:
    """fr.cuh's R^k mod r for k = 0..3 as ints, and the Fr kernels' shape: workgroup size, k_fr_dot_partial's
    and k_fr_combine's grid caps, k_fr_powers' elements per lane."""
    out = np.zeros(36, dtype=np.uint32)
    _check(load().msm_test_fr_op(5, None, None, _ptr(out), 0), "msm_test_fr_op")
    raw = out[:32].astype("<u4").tobytes()
    return {"r_powers": [int.from_bytes(raw[32 * k: 32 * k + 32], "little") for k in range(4)],
            "threads": int(out[32]), "dot_cap": int(out[33]), "combine_cap": int(out[34]), "pow_steps": int(out[35])}


def _test_fr_inv(values) -> list:
    """csrc/fr.cuh's fr_inv on the host (msm_test_fr_inv; no GPU needed): for every a < r in Montgomery form,
    a^-1 in Montgomery form, 0 for 0.  MsmError -1 for a value at or above r."""
    vals = [int(v) for v in values]
    buf = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u4").astype(np.uint32)
    out = np.zeros(max(len(vals), 1) * 8, dtype=np.uint32)
    _check(load().msm_test_fr_inv(_ptr(buf) if len(vals) else None, _ptr(out), len(vals)), "msm_test_fr_inv")
    raw = out.astype("<u4").tobytes()
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(vals))]


def _test_fr_scan_constants() -> dict:
    """The shape of k_fr_inverse, k_fr_scan_* and k_fr_tensor (msm_test_fr_scan_constants; no GPU needed):
    elements per lane and per tile, the most spans of a scan, k_fr_inverse's grid cap, the squarings and
    products of one fr_inv, the largest k of a tensor product."""
    out = np.zeros(8, dtype=np.uint32)
    _check(load().msm_test_fr_scan_constants(out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))),
           "msm_test_fr_scan_constants")
    keys = ("e", "tile", "scan_cap", "inverse_cap", "inv_squarings", "inv_products", "tensor_max_k")
    return {k: int(v) for k, v in zip(keys, out)}


def _test_fr_scan_plan(m: int, grid_cap: int) -> dict:
    """The launch plan of a scan of m elements over at most grid_cap spans, as msm_fr_scan* makes it
    (msm_test_fr_scan_plan; no GPU needed)."""
    if not (0 <= int(m) < (1 << 64) and 0 <= int(grid_cap) < (1 << 32)):
        raise MsmError(-1, "msm_test_fr_scan_plan")
    out = np.zeros(4, dtype=np.uint32)
    _check(load().msm_test_fr_scan_plan(int(m), int(grid_cap), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))),
           "msm_test_fr_scan_plan")
    return {"e": int(out[0]), "tile": int(out[1]), "grid": int(out[2]), "tiles_per_span": int(out[3])}


def _test_fr_inverse_device(a, grid_cap: int, scale: Optional[int] = None, form: str = "wire",
                            out_form: Optional[str] = None, out=None):
    """fr_inverse of a device tensor with at most grid_cap workgroups (msm_test_fr_inverse_device)."""
    return _fr_unary("msm_fr_inverse", "msm_fr_inverse_device", a, _fr_word(scale), (), form, out_form, out, -1, 0,
                     grid_cap=grid_cap)


def _test_fr_scan_device(a, grid_cap: int, first: Optional[int] = None, sum: bool = False, exclusive: bool = False,
                         form: str = "wire", out_form: Optional[str] = None, out=None):
    """fr_cumprod / fr_cumsum of a device tensor over at most grid_cap spans (msm_test_fr_scan_device)."""
    flags = (MSM_FR_SCAN_SUM if sum else 0) | (MSM_FR_SCAN_EXCLUSIVE if exclusive else 0)
    return _fr_unary("msm_fr_scan", "msm_fr_scan_device", a, _fr_word(first), (flags,), form, out_form, out, -1, 0,
                     grid_cap=grid_cap)


def _test_native_plan(n: int, scalar_type, scalar_bits: int, window_size: int = 0) -> dict:
    """The plan of a native-type launch (msm_test_native_plan; no GPU needed): _test_narrow_plan's
    fields for scalar_bits, then the bytes of one vector and of its region in a launch's upload buffer."""
    out = np.zeros(8, dtype=np.uint32)
    ty = SCALAR_TYPES[scalar_type][0] if isinstance(scalar_type, str) else int(scalar_type)
    _check(load().msm_test_native_plan(n, ty, int(scalar_bits), int(window_size),
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), "msm_test_native_plan")
    return dict(zip(("c", "windows", "q", "nhi", "words", "packed", "vector_bytes", "region_bytes"),
                    (int(v) for v in out)))


def _test_dense_plan(n: int, nm: int = 1, pipelined: bool = False, scalar_bits: int = 8, window_size: int = 0) -> dict:
    """The dense-bucket part of a narrow launch's plan (msm_test_dense_plan; no GPU needed): whether
    the launch takes the dense accumulation, the entries per unit lane E, the keys W * B, the unit
    kernel's grid bound and the run length K, for the default device shape (256 CUs, 4 waves per
    SIMD).  E and the bound are 0 for a launch that is not dense."""
    o, op_ = _out(5)
    _check(load().msm_test_dense_plan(n, int(nm), 1 if pipelined else 0, int(scalar_bits), int(window_size), op_),
           "msm_test_dense_plan")
    return dict(zip(("dense", "E", "nkeys", "units", "K"), (int(v) for v in o)))


def _test_dense_segments(bucket_start, S: int) -> Tuple[np.ndarray, np.ndarray]:
    """k_dense_segments alone on the device (test hook): bucket_start [nkeys + 1] (non-decreasing)
    and the segment length S -> (seg_base [nkeys + 1], unit_key [bucket_start[-1] // S + nkeys]);
    unit_key's words past the live units come back as 0xffffffff."""
    bs = np.ascontiguousarray(_u32(bucket_start).reshape(-1))
    nkeys = bs.shape[0] - 1
    if nkeys < 1:
        raise ValueError("bucket_start holds nkeys + 1 words")
    seg, seg_ = _out(nkeys + 1)
    unit, unit_ = _out(int(bs[-1]) // int(S) + nkeys)
    _check(load().msm_test_dense_segments(_ptr(bs), nkeys, int(S), seg_, unit_), "msm_test_dense_segments")
    return seg, unit


def _test_acc_state(keys=(), workgroups=()) -> dict:
    """What the last lone MSM of the default device left in its slot's workspace (msm_test_acc_state, test
    hook; tests/test_gpu_acc_chains.py): M, K, nkeys, runs, workgroups, second_pass, c; bucket_start
    [nkeys + 1], run_key [runs], sorted_entry [M], cross_key and lead_open [workgroups], the skewed
    workgroups (sorted), and the affine (x, y) of buckets[key] for `keys` and of lead_val[wg] for
    `workgroups`, as dicts."""
    L = load()
    info, info_ = _out(8)
    _check(L.msm_test_acc_state(info_, None, None, None, None, None, None, None, 0, None, None, 0, None),
           "msm_test_acc_state")
    M, K, nkeys, runs, nwg, nskew, second, c = (int(v) for v in info)
    ks = np.ascontiguousarray(_u32(list(keys)).reshape(-1))
    ws = np.ascontiguousarray(_u32(list(workgroups)).reshape(-1))
    bs, rk, se = np.zeros(nkeys + 1, np.uint32), np.zeros(max(runs, 1), np.uint32), np.zeros(max(M, 1), np.uint32)
    ck, lo = np.zeros(max(nwg, 1), np.uint32), np.zeros(max(nwg, 1), np.uint32)
    sk = np.zeros(max(nskew, 1), np.uint32)
    kxy, wxy = np.zeros((max(len(ks), 1), 16), np.uint32), np.zeros((max(len(ws), 1), 16), np.uint32)
    _check(L.msm_test_acc_state(info_, _ptr(bs), _ptr(rk), _ptr(se), _ptr(ck), _ptr(lo), _ptr(sk), _ptr(ks), len(ks),
                                _ptr(kxy), _ptr(ws), len(ws), _ptr(wxy)), "msm_test_acc_state")
    if [int(v) for v in info] != [M, K, nkeys, runs, nwg, nskew, second, c]:
        raise RuntimeError("msm_test_acc_state: the slot changed between the two reads")
    return {"M": M, "K": K, "nkeys": nkeys, "runs": runs, "workgroups": nwg, "second_pass": bool(second), "c": c,
            "bucket_start": bs, "run_key": rk[:runs], "sorted_entry": se[:M], "cross_key": ck[:nwg],
            "lead_open": lo[:nwg], "skewed": sorted(int(v) for v in sk[:nskew]),
            "buckets": {int(k): _xy(kxy[i]) for i, k in enumerate(ks)},
            "lead_val": {int(g): _xy(wxy[i]) for i, g in enumerate(ws)}}


RED_PATHS = ("groups+terms", "reduce_2", "fold")  # msm_test_red_state's second-stage path, by value


def _test_red_state(chunks=(), group_points=(), terms=()) -> dict:
    """What the bucket reduction of the last lone MSM of the default device left in its slot
    (msm_test_red_state, test hook; tests/test_gpu_red_state.py): chunk length L, nchunks, ngroups, nv,
    nterms, windows W, buckets B, the second-stage path (a RED_PATHS name), pairs, RG_OUT, c and the set of
    empty windows; and the affine (x, y) of red_U / red_T for `chunks` [(w, c)], of red_G for
    `group_points` [(w, g, idx)] and of the window terms for `terms` [(w, t)], as dicts."""
    L = load()
    info, info_ = _out(16)
    _check(L.msm_test_red_state(info_, None, 0, None, None, None, 0, None, None, 0, None), "msm_test_red_state")
    keys = ("L", "nchunks", "ngroups", "nv", "nterms", "W", "B", "path", "pairs", "rg_out", "c")
    st = dict(zip(keys, (int(v) for v in info[:11])))
    st["empty"] = {w for w in range(st["W"]) if (int(info[11 + w // 32]) >> (w % 32)) & 1}
    st["path"], st["pairs"] = RED_PATHS[st["path"]], bool(st["pairs"])
    chunks, group_points, terms = list(chunks), list(group_points), list(terms)
    ci = np.ascontiguousarray(_u32([w * st["nchunks"] + c for w, c in chunks]).reshape(-1))
    gi = np.ascontiguousarray(_u32([(w * st["ngroups"] + g) * st["rg_out"] + i for w, g, i in group_points]).reshape(-1))
    ti = np.ascontiguousarray(_u32([w * st["nterms"] + t for w, t in terms]).reshape(-1))
    u, t, g, tx = (np.zeros((max(len(a), 1), 16), np.uint32) for a in (ci, ci, gi, ti))
    before = info.copy()
    _check(L.msm_test_red_state(info_, _ptr(ci), len(ci), _ptr(u), _ptr(t), _ptr(gi), len(gi), _ptr(g), _ptr(ti), len(ti),
                                _ptr(tx)), "msm_test_red_state")
    if not np.array_equal(before, info):
        raise RuntimeError("msm_test_red_state: the slot changed between the two reads")
    st["U"] = {k: _xy(u[i]) for i, k in enumerate(chunks)}
    st["T"] = {k: _xy(t[i]) for i, k in enumerate(chunks)}
    st["G"] = {k: _xy(g[i]) for i, k in enumerate(group_points)}
    st["terms"] = {k: _xy(tx[i]) for i, k in enumerate(terms)}
    return st


def _test_red_map(n: int, nm: int = 1, chunk_len: int = 0, window_size: Optional[int] = None,
                  windows: Optional[Tuple[int, int]] = None, scalar_bits: Optional[int] = None, extra: int = 0) -> dict:
    """The first reduction stage's grid maps on the host (msm_test_red_map: the kernels' own red1_lane and
    red1_group) for the plan of nm MSMs of n points: L, nchunks, ngroups, W, Wr, B, Wm, w0, `lanes`
    [W nchunks + extra][2] = (window, chunk) and `groups` [W ngroups + extra][3] = (window, group, live),
    0xffffffff where the map says false.  chunk_len = 0 takes the plan's own.  No GPU needed."""
    L = load()
    info, info_ = _out(8)
    o = _opts(window_size, windows=windows, scalar_bits=scalar_bits)
    _check(L.msm_test_red_map(n, nm, o, chunk_len, info_, None, 0, None, 0), "msm_test_red_map")
    d = dict(zip(("L", "nchunks", "ngroups", "W", "Wr", "B", "Wm", "w0"), (int(v) for v in info)))
    lanes = np.zeros((d["W"] * d["nchunks"] + extra, 2), np.uint32)
    groups = np.zeros((d["W"] * d["ngroups"] + extra, 3), np.uint32)
    _check(L.msm_test_red_map(n, nm, o, chunk_len, info_, _ptr(lanes), len(lanes), _ptr(groups), len(groups)),
           "msm_test_red_map")
    d["lanes"], d["groups"] = lanes, groups
    return d


def _test_red_map_term(nv: int, ngroups: int, term: int) -> dict:
    """k_red2_terms' map on the host (msm_test_red_map_term): red2_term's idx, g0, g1, kbit, npts, bitsel
    and `groups` = red2_term_group(j) for j < npts.  No GPU needed."""
    o, o_ = _out(6)
    _check(load().msm_test_red_map_term(nv, ngroups, term, o_, None, 0), "msm_test_red_map_term")
    g = np.zeros(max(int(o[4]), 1), np.uint32)
    _check(load().msm_test_red_map_term(nv, ngroups, term, o_, _ptr(g), int(o[4])), "msm_test_red_map_term")
    d = dict(zip(("idx", "g0", "g1", "kbit", "npts", "bitsel"), (int(v) for v in o)))
    d["groups"] = [int(v) for v in g[:d["npts"]]]
    return d


def _test_tail_plan(n: int, terms=None, helpers: int = 0, chunk_len: int = 0, window_size: Optional[int] = None,
                    windows: Optional[Tuple[int, int]] = None):
    """The host tail on caller-given window terms for a plan of the caller's (msm_test_tail_plan):
    without `terms` the plan's {windows, nterms, nv, L, w0, Wm}; with them ([windows nterms, 32] host
    Montgomery words) the tail's affine (x, y).  No GPU needed."""
    info, info_ = _out(6)
    o = _opts(window_size, windows=windows)
    if terms is None:
        _check(load().msm_test_tail_plan(n, o, chunk_len, None, 0, info_, None), "msm_test_tail_plan")
        return dict(zip(("windows", "nterms", "nv", "L", "w0", "Wm"), (int(v) for v in info)))
    t = np.ascontiguousarray(_u32(terms).reshape(-1))
    _check(load().msm_test_tail_plan(n, o, chunk_len, None, 0, info_, None), "msm_test_tail_plan")
    if t.size != int(info[0]) * int(info[1]) * 32:
        raise ValueError("terms: windows * nterms * 32 words")
    out, out_ = _out(16)
    _check(load().msm_test_tail_plan(n, o, chunk_len, _ptr(t), int(helpers), info_, out_), "msm_test_tail_plan")
    return _xy(out)


def _test_subset_plan(n_handle: int, levels: int, window_size: int, first: int, m: int, indexed: bool) -> dict:
    """The launch plan of one subset MSM of m terms on a handle of n_handle points (msm_test_subset_plan):
    the terms the plan counts (d.n), whether its entries carry their fine key (packed), the record
    stride, the fine bits fb, and the scatter variant (0 plain, 1 range, 2 indexed).  Applies the
    argument rules that need no device (MsmError -1).  No device needed."""
    o, op_ = _out(5)
    _check(load().msm_test_subset_plan(n_handle, levels, window_size, first, m, 1 if indexed else 0, op_),
           "msm_test_subset_plan")
    return {"n": int(o[0]), "packed": int(o[1]), "stride": int(o[2]), "fb": int(o[3]), "sub": int(o[4])}


def _test_bases_records(bases: "Bases", level: int) -> np.ndarray:
    """The records of one level of a handle, [n, 32] words (test hook)."""
    n = bases.info["n"]
    o, op_ = _out(max(n, 1) * 32)
    _check(load().msm_test_bases_records(bases._h or None, level, op_), "msm_test_bases_records")
    return o[: n * 32].reshape(n, 32)


def _test_split_scalars(scalars, levels: int, chunk_bits: int) -> np.ndarray:
    """k_split_scalars on wire scalars [n, 8] -> [levels * n, 8] virtual scalars (test hook)."""
    sc = np.ascontiguousarray(_u32(scalars).reshape(-1, 8))
    o, op_ = _out(levels * sc.shape[0] * 8)
    _check(load().msm_test_split_scalars(_ptr(sc), sc.shape[0], levels, chunk_bits, op_), "msm_test_split_scalars")
    return o.reshape(-1, 8)


def _test_sharded(mode: int, points, scalars, n: int, devices: Sequence[int], window_size: Optional[int] = None,
                  stream: int = 0) -> Tuple[int, int]:
    """Test hook: the device-list shard/join paths with a list that may repeat a device (mode 0:
    host wire arrays as msm_compute, 1: device-resident inputs as msm_compute_device)."""
    L = load()
    arr = (ctypes.c_int32 * len(devices))(*devices)
    o, op = _out(16)
    if mode == 0:
        pts = np.ascontiguousarray(_u32(points).reshape(-1, 32)[:n])
        sc = np.ascontiguousarray(_u32(scalars).reshape(-1, 8)[:n])
        pp, sp, st = _ptr(pts), _ptr(sc), None
    else:
        pp, sp, st = _dev_ptr(points), _dev_ptr(scalars), _stream(stream, points, scalars)
    _check(L.msm_test_sharded(mode, pp, sp, n, _opts(window_size), arr, len(devices), st, op), "msm_test_sharded")
    return _xy(o)


# ---- guarded workspaces (csrc/host_ctx.h g_guard, csrc/host_guard.h; tests/test_gpu_guard.py) ----
_GUARD_SIDES = ("front", "back", "zero")


def _test_guard_names() -> list:
    """The buffer names of the guard reports, by index (msm_test_guard_name).  No GPU needed."""
    L, names = load(), []
    while True:
        s = L.msm_test_guard_name(len(names))
        if s is None:
            return names
        names.append(s.decode())


def _test_guard(on: bool) -> bool:
    """Switch the guarded-allocation mode (msm_test_guard); returns the previous state.  MsmError -1
    while the library holds an allocation made in the other mode: run msm_shutdown first."""
    rc = load().msm_test_guard(1 if on else 0)
    _check(min(rc, 0), "msm_test_guard")
    return bool(rc)


def _test_guard_release(device: int = -1) -> None:
    """Free the workspaces of the device's context (every context for -1), keeping handles: the next
    call allocates each buffer at exactly its own plan's size (msm_test_guard_release)."""
    _check(load().msm_test_guard_release(int(device)), "msm_test_guard_release")


def _test_guard_check(device: int = -1) -> list:
    """Touched guard bands and broken zero invariants (msm_test_guard_check), each a dict: buffer
    name, device, slot (-1: not a slot's), side ("front" / "back" / "zero"), first and last offset in
    bytes -- a front guard's from the payload's start (negative), a back guard's from its end, a zero
    invariant's word from the payload's start -- and the count (bytes; words for "zero").  What is
    reported is repaired, so the next check is clean."""
    L, names = load(), _test_guard_names()
    cap = 64
    while True:
        rep, cnt = (GuardHit * cap)(), ctypes.c_size_t(0)
        _check(L.msm_test_guard_check(int(device), rep, cap, ctypes.byref(cnt)), "msm_test_guard_check")
        if cnt.value > cap:  # (the first cap were repaired already: they are in `rep`, the rest come again)
            raise RuntimeError(f"{cnt.value} guard findings, more than {cap}: {_guard_dicts(rep, cap, names)}")
        return _guard_dicts(rep, cnt.value, names)


def _guard_dicts(rep, k: int, names: list) -> list:
    return [{"buffer": names[h.buffer] if h.buffer < len(names) else int(h.buffer), "device": int(h.device),
             "slot": int(h.slot), "side": _GUARD_SIDES[h.side], "first": int(h.first), "last": int(h.last),
             "count": int(h.count)} for h in rep[:k]]


def _test_guard_plant(buffer: str, where: int, slot: int = 0, device: int = -1) -> None:
    """Self-test of the check (msm_test_guard_plant): one byte written with hipMemset into `buffer` of
    `slot` -- where 0: first byte of the back guard, 1: its last byte, 2: last byte of the front guard,
    3: the second payload word."""
    _check(load().msm_test_guard_plant(int(device), int(slot), _test_guard_names().index(buffer), int(where)),
           "msm_test_guard_plant")


def _test_guard_fill(word: int) -> int:
    """Set the 32-bit word guarded allocations write over their payload (msm_test_guard_fill) and return
    the previous one.  0 is the default; MsmError -1 for a word above 3.  It changes allocations made
    after the call, and nothing while the guard mode is off.  No GPU needed."""
    if not 0 <= int(word) < (1 << 32):
        raise MsmError(-1, "msm_test_guard_fill")
    rc = load().msm_test_guard_fill(int(word))
    _check(min(rc, 0), "msm_test_guard_fill")
    return int(rc)


def _test_guard_poison(device: int = -1) -> None:
    """Overwrite, at quiescence, the payload of every guarded workspace buffer, h_out and context buffer
    with the current fill word (msm_test_guard_poison): nothing is freed, no graph dropped.  The five
    regions the kernels keep all-zero and the handles' records are left as they are."""
    _check(load().msm_test_guard_poison(int(device)), "msm_test_guard_poison")


def _test_guard_peek(buffer, first_word: int, words: int, slot: int = 0, device: int = -1) -> np.ndarray:
    """`words` payload words of `buffer` (a name of _test_guard_names, or an index) from `first_word` on,
    as uint32 (msm_test_guard_peek); nothing is launched.  MsmError -1 for a range outside the payload,
    a buffer that is not allocated or not a slot's or the context's, and a process without a context."""
    if isinstance(buffer, str):
        names = _test_guard_names()
        buffer = names.index(buffer) if buffer in names else len(names)
    if not (0 <= int(buffer) < (1 << 32) and 0 <= int(first_word) < (1 << 62) and 0 <= int(words) < (1 << 40)):
        raise MsmError(-1, "msm_test_guard_peek")
    out = np.zeros(max(int(words), 1), dtype=np.uint32)
    _check(load().msm_test_guard_peek(int(device), int(slot), int(buffer), int(first_word), int(words),
                                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), "msm_test_guard_peek")
    return out[:int(words)]
