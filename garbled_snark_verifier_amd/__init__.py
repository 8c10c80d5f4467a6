"""MI355X-native garbling / evaluation engine for the streaming Free-XOR / half-gates gate loop of
BitVM/garbled-snark-verifier.

This module is the thin Python host layer over the C ABI in ``include/gsv_engine.h``
(``libgsv_engine.so``: hand-written HIP kernels for gfx950 + C++ host runtime).  It mirrors the
reference's entry points for the hot path

    CircuitBuilder::streaming_garbling    src/circuit/mod.rs:180-203   ->  CircuitBuilder.streaming_garbling
    CircuitBuilder::streaming_evaluation  src/circuit/mod.rs:225-249   ->  CircuitBuilder.streaming_evaluation
    AESAccumulatingHash                   src/ciphertext_hasher.rs     ->  StreamingResult.ciphertext_hash

There is no CPU fallback: every garble/evaluate call runs on a HIP device or raises ``GsvError``.
"""
import atexit
import collections
import ctypes as C
import os
import sys
import weakref

import numpy as np

from . import build as _build

__all__ = ["GsvError", "lib", "Program", "Engine", "Session", "CircuitBuilder", "StreamingResult", "labels_from_seed", "GATE_NAMES", "cbcmac", "cbcmac_many",
           "write_gc_file", "read_gc_file", "gc_file_name", "blake3", "blake3_file", "blake3_streams", "Blake3",
           "CiphertextMismatch", "outboard_file_name", "blake3_outboard_root", "blake3_file_outboard", "blake3_files", "blake3_outboard_size", "SinkCommit",
           "checkpoint_file_name", "cbcmac_checkpoints_size", "cbcmac_file_checkpoints", "cbcmac_file_check", "cbcmac_files", "cbcmac_streams_check"]

GATE_NAMES = ["And", "Nand", "Nimp", "Imp", "Ncimp", "Cimp", "Nor", "Or", "Xor", "Xnor", "Not"]
_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


class GsvError(RuntimeError):
    pass


class CiphertextMismatch(GsvError):
    """GSV_ERR_MISMATCH: a received ciphertext stream differs from its BLAKE3 outboard or commitment.  `instance` is the instance of
    the session (blake3_files: the index into `paths`), `group` the group of 2^k chunks (the tail behind the last complete group
    counts as the group after it) and `first_record` the first record the differing value covers; `group` and `first_record` are
    None when the outboard or the last chunk did not match the commitment before the pass.  `resume_call` (Session.evaluate_calls with
    restartable=True): the call the session was rolled back to and the repeat starts at — Session.resume_info() adds the record —
    or None when nothing can be resumed."""

    def __init__(self, message, instance=None, group=None, first_record=None, resume_call=None):
        super().__init__(message)
        self.instance, self.group, self.first_record, self.resume_call = instance, group, first_record, resume_call


# Device objects are released in dependency order BEFORE the interpreter tears down: a session collected during interpreter
# shutdown would call into a HIP runtime that has already destroyed its own state (observed: std::bad_variant_access inside hipFree).
_live = {"session": weakref.WeakSet(), "plan": weakref.WeakSet(), "program": weakref.WeakSet(), "engine": weakref.WeakSet()}


class _gc_paused:
    """Cyclic garbage collection paused for the duration of a streaming call.  A streaming pass runs Python on OTHER threads (the sink /
    source callbacks) and, in ring mode, its device calls wait for the host's progress.  If the collector fires on such a thread and
    finalizes a forgotten Session / Plan / Program, `gsv_*_destroy` -> hipFree synchronises the WHOLE device: it waits for the running
    window, which waits for the host's stream position, which waits for the callback that is stuck in hipFree — until the device's
    watchdog ends the pass after GSV_DEP_WAIT_SECONDS with GSV_ERR_DEVICE (seen once in round 5's full GPU suite).
    Since round 6 the engine itself defers every release requested while a streaming pass is in flight (engine.cpp, ReleaseGate;
    include/gsv_engine.h "Deferred release"), so a destroy from a callback is harmless whoever issues it; the pause stays as a second
    layer (it also keeps collector pauses out of the callbacks, which sit on the drain's critical path)."""

    _lock = __import__("threading").Lock()
    _depth = 0
    _was_enabled = False

    def __enter__(self):
        import gc
        with _gc_paused._lock:
            if _gc_paused._depth == 0:
                _gc_paused._was_enabled = gc.isenabled()
                gc.disable()
            _gc_paused._depth += 1

    def __exit__(self, *exc):
        import gc
        with _gc_paused._lock:
            _gc_paused._depth -= 1
            if _gc_paused._depth == 0 and _gc_paused._was_enabled:
                gc.enable()
        return False


@atexit.register
def _close_everything():
    for kind in ("session", "plan", "program", "engine"):
        for obj in list(_live[kind]):
            try:
                obj.close()
            except Exception:
                pass


class _ProgramInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_inputs", "n_outputs", "n_gates", "n_ciphertexts", "n_dead")] + [("gate_count", C.c_uint64 * 11)] + [
        (n, C.c_uint64) for n in ("n_steps", "and_depth", "n_and_steps", "max_step_width", "n_slots", "peak_live", "device_bytes", "n_lds_slots",
                                 "reads_lds", "reads_hbm", "writes_lds", "writes_hbm", "n_fused_free", "and_terms")]


class _PlanSessionOpts(C.Structure):
    _fields_ = [("retain_stream", C.c_int), ("max_concurrent_calls", C.c_uint32), ("window_ct_records", C.c_uint64), ("max_scratch_slots", C.c_uint64),
                ("max_window_calls", C.c_uint32), ("drain_segment_records", C.c_uint32)]


_SCHED_FIELDS = ["n_calls", "n_windows", "n_dependencies", "max_width", "scratch_slots", "wire_file_slots", "window_ct_records", "critical_steps", "total_steps",
                 "n_segments", "segment_ct_records", "ct_ring_records"]


class _PlanScheduleInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in _SCHED_FIELDS]


class _CompileOpts(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("struct_size", "window_div", "keep_trace", "background", "consume_recorder", "reserved")] + [("for_plan", C.c_void_p)]


class _PlanRecorderOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("window_div", C.c_uint32), ("plan_file", C.c_char_p)]


class _Gate(C.Structure):
    _fields_ = [("wire_a", C.c_uint64), ("wire_b", C.c_uint64), ("wire_c", C.c_uint64), ("gate_type", C.c_uint8), ("pad", C.c_uint8 * 7)]


EXPORTS = [
    "gsv_last_error", "gsv_recorder_create", "gsv_recorder_destroy", "gsv_recorder_allocate_wire", "gsv_recorder_declare_input",
    "gsv_recorder_push_gates", "gsv_recorder_declare_outputs", "gsv_recorder_record_circuit", "gsv_recorder_counts", "gsv_program_compile", "gsv_program_destroy",
    "gsv_program_get_info", "gsv_engine_create", "gsv_engine_destroy", "gsv_deferred_release_count", "gsv_session_fallback_count", "gsv_plan_build_file_pair", "gsv_plan_build_file_div", "gsv_plan_from_circuit_div", "gsv_plan_call_record_form", "gsv_labels_from_seed", "gsv_session_create", "gsv_session_destroy",
    "gsv_session_set_garble_inputs", "gsv_session_garble", "gsv_session_set_evaluate_inputs", "gsv_session_upload_ciphertexts",
    "gsv_session_evaluate", "gsv_session_set_hasher", "gsv_session_sync", "gsv_session_last_kernel_ms", "gsv_session_read_outputs", "gsv_session_read_ciphertexts",
    "gsv_session_ciphertext_hash", "gsv_cbcmac_update", "gsv_cbcmac_update_many", "gsv_commit_labels",
    "gsv_plan_from_circuit", "gsv_plan_io", "gsv_plan_recorder_create", "gsv_plan_recorder_destroy", "gsv_plan_recorder_allocate_wire",
    "gsv_plan_recorder_declare_input", "gsv_plan_recorder_push_gates", "gsv_plan_recorder_call", "gsv_plan_recorder_finish", "gsv_plan_create", "gsv_plan_destroy", "gsv_plan_add_call", "gsv_plan_finish", "gsv_plan_counts", "gsv_session_create_plan", "gsv_session_create_plan_ex",
    "gsv_session_garble_streaming", "gsv_session_garble_streaming_calls", "gsv_plan_call_info", "gsv_plan_image_bytes", "gsv_plan_wire_file", "gsv_plan_save", "gsv_plan_load", "gsv_plan_build_file", "gsv_cbcmac_chains_per_step", "gsv_session_evaluate_streaming", "gsv_session_instances_per_workgroup", "gsv_session_enable_step_clock", "gsv_session_read_step_clock", "gsv_program_step_stats",
    "gsv_session_create_plan_opts", "gsv_session_plan_schedule_info", "gsv_session_plan_window", "gsv_session_set_unchecked_slices",
    "gsv_session_garble_streaming_sink", "gsv_session_garble_evaluate", "gsv_session_evaluate_streaming_indexed", "gsv_session_evaluate_streaming_source",
    "gsv_recorder_allocate_wires", "gsv_plan_recorder_allocate_wires", "gsv_program_compile_opts", "gsv_program_wait", "gsv_plan_recorder_create_opts", "gsv_session_set_drain_instances",
    "gsv_session_garble_streaming_commit", "gsv_blake3_create", "gsv_blake3_destroy", "gsv_blake3_update", "gsv_blake3_absorb_subtree", "gsv_blake3_finalize", "gsv_blake3_file",
    "gsv_engine_blake3_streams", "gsv_engine_blake3_streams_seconds",
    "gsv_session_evaluate_streaming_commit", "gsv_session_evaluate_streaming_source_commit", "gsv_session_ciphertext_blake3",
    "gsv_blake3_outboard_root", "gsv_blake3_file_outboard", "gsv_session_garble_streaming_commit_outboard", "gsv_engine_blake3_files",
    "gsv_session_evaluate_streaming_verified", "gsv_session_mismatch_info", "gsv_session_windows_launched",
    "gsv_blake3_outboard_size", "gsv_session_garble_streaming_sink_commit", "gsv_session_evaluate_streaming_source_verified",
    "gsv_session_evaluate_streaming_calls", "gsv_session_evaluate_streaming_source_calls", "gsv_session_evaluate_resume_info",
    "gsv_cbcmac_checkpoints_size", "gsv_cbcmac_file_checkpoints", "gsv_cbcmac_file_check", "gsv_engine_cbcmac_streams_check", "gsv_engine_cbcmac_streams_check_seconds",
    "gsv_engine_cbcmac_files", "gsv_session_garble_streaming_checkpoints", "gsv_session_garble_streaming_check",
    "gsv_session_evaluate_streaming_mac_calls", "gsv_session_evaluate_streaming_source_mac_calls", "gsv_session_ciphertext_cbcmac_check",
]

# CiphertextHandler / CiphertextSource as host callbacks (include/gsv_engine.h: gsv_ct_sink_fn, gsv_ct_source_fn)
CT_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64)
CT_SOURCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64)
# an instance's BLAKE3 outboard as it is produced (gsv_outboard_sink_fn): (user, instance, byte_offset, bytes, n_bytes)
OUTBOARD_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64)
# what Session.garble_to_sink returns with a commitment: lists with one entry per drained instance, or None (see there)
SinkCommit = collections.namedtuple("SinkCommit", "cbcmac blake3 outboards last_chunks")


def lib():
    """Loads (building in-tree if needed) libgsv_engine.so.  Raises if the library cannot be built/loaded."""
    global _lib
    if _lib is None:
        so = _build.build()
        L = C.CDLL(so)
        u8p, vp = C.POINTER(C.c_uint8), C.c_void_p
        L.gsv_last_error.restype = C.c_char_p
        L.gsv_recorder_create.argtypes = [C.POINTER(vp)]
        L.gsv_recorder_destroy.argtypes = [vp]
        L.gsv_recorder_destroy.restype = None
        L.gsv_recorder_allocate_wire.argtypes = [vp, C.c_uint16, C.POINTER(C.c_uint64)]
        L.gsv_recorder_declare_input.argtypes = [vp, C.c_uint64]
        L.gsv_recorder_push_gates.argtypes = [vp, C.POINTER(_Gate), C.c_size_t]
        L.gsv_recorder_declare_outputs.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t]
        L.gsv_recorder_record_circuit.argtypes = [vp, C.c_char_p]
        L.gsv_recorder_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_program_compile.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(vp)]
        L.gsv_program_compile_opts.argtypes = [vp, vp, C.POINTER(vp)]  # (opts: any structure laid out as gsv_compile_opts)
        L.gsv_program_destroy.argtypes = [vp]
        L.gsv_program_destroy.restype = None
        L.gsv_program_get_info.argtypes = [vp, C.POINTER(_ProgramInfo)]
        L.gsv_engine_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.gsv_engine_destroy.argtypes = [vp]
        L.gsv_engine_destroy.restype = None
        L.gsv_session_fallback_count.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.gsv_plan_call_record_form.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint32)]
        L.gsv_plan_build_file_pair.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32]
        L.gsv_deferred_release_count.argtypes = []
        L.gsv_deferred_release_count.restype = C.c_uint64
        L.gsv_labels_from_seed.argtypes = [C.c_uint64, C.c_size_t, u8p, u8p, u8p, u8p]
        L.gsv_session_create.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.c_uint64, C.POINTER(vp)]
        L.gsv_session_destroy.argtypes = [vp]
        L.gsv_session_destroy.restype = None
        L.gsv_session_set_garble_inputs.argtypes = [vp, u8p, u8p, u8p]
        L.gsv_session_garble.argtypes = [vp, C.c_uint64]
        L.gsv_session_set_evaluate_inputs.argtypes = [vp, u8p, u8p, u8p]
        L.gsv_session_upload_ciphertexts.argtypes = [vp, C.c_size_t, u8p, C.c_uint64]
        L.gsv_session_evaluate.argtypes = [vp, C.c_uint64]
        L.gsv_session_set_hasher.argtypes = [vp, C.c_int]
        L.gsv_session_sync.argtypes = [vp]
        L.gsv_session_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gsv_session_read_outputs.argtypes = [vp, u8p, u8p]
        L.gsv_session_read_ciphertexts.argtypes = [vp, C.c_size_t, C.c_uint64, C.c_uint64, u8p]
        L.gsv_session_ciphertext_hash.argtypes = [vp, C.c_size_t, u8p]
        L.gsv_cbcmac_update.argtypes = [u8p, u8p, C.c_uint64]
        L.gsv_commit_labels.argtypes = [u8p, C.c_uint64, u8p]
        L.gsv_cbcmac_update_many.argtypes = [u8p, C.POINTER(C.c_void_p), C.c_size_t, C.c_uint64]
        L.gsv_plan_from_circuit.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp)]
        L.gsv_plan_from_circuit_div.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(vp)]
        L.gsv_plan_io.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_plan_recorder_create.argtypes = [C.POINTER(vp)]
        L.gsv_plan_recorder_create_opts.argtypes = [vp, C.POINTER(vp)]  # (opts: any structure laid out as gsv_plan_recorder_opts)
        L.gsv_plan_recorder_destroy.argtypes = [vp]
        L.gsv_plan_recorder_destroy.restype = None
        L.gsv_plan_recorder_allocate_wire.argtypes = [vp, C.c_uint16, C.POINTER(C.c_uint64)]
        L.gsv_plan_recorder_declare_input.argtypes = [vp, C.c_uint64]
        L.gsv_plan_recorder_push_gates.argtypes = [vp, C.POINTER(_Gate), C.c_size_t]
        L.gsv_plan_recorder_call.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_plan_recorder_finish.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(vp)]
        L.gsv_plan_create.argtypes = [C.POINTER(vp)]
        L.gsv_plan_destroy.argtypes = [vp]
        L.gsv_plan_destroy.restype = None
        L.gsv_plan_add_call.argtypes = [vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.gsv_plan_finish.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.c_size_t]
        L.gsv_plan_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_session_create_plan.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
        L.gsv_session_create_plan_ex.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(vp)]
        L.gsv_session_evaluate_streaming.argtypes = [vp, C.c_uint64, C.c_char_p, C.c_uint64, u8p]
        L.gsv_session_garble_streaming.argtypes = [vp, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, u8p]
        L.gsv_session_garble_streaming_calls.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, u8p]
        L.gsv_plan_call_info.argtypes = [vp, C.c_uint64] + [C.POINTER(C.c_uint64)] * 5
        L.gsv_plan_image_bytes.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_plan_wire_file.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_plan_save.argtypes = [vp, C.c_char_p]
        L.gsv_plan_load.argtypes = [C.c_char_p, vp, C.POINTER(vp)]
        L.gsv_plan_build_file.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
        L.gsv_plan_build_file_div.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32]
        L.gsv_session_instances_per_workgroup.argtypes = [vp, C.POINTER(C.c_int)]
        L.gsv_session_enable_step_clock.argtypes = [vp]
        L.gsv_session_read_step_clock.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.gsv_program_step_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.gsv_session_create_plan_opts.argtypes = [vp, vp, C.c_size_t, C.POINTER(_PlanSessionOpts), C.POINTER(vp)]
        L.gsv_session_plan_schedule_info.argtypes = [vp, C.POINTER(_PlanScheduleInfo)]
        L.gsv_session_plan_window.argtypes = [vp, C.c_uint64] + [C.POINTER(C.c_uint64)] * 3
        L.gsv_session_set_unchecked_slices.argtypes = [vp, C.c_int]
        L.gsv_session_set_drain_instances.argtypes = [vp, C.c_size_t]
        L.gsv_session_garble_streaming_sink.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, CT_SINK_FN, vp, C.c_int, u8p]
        L.gsv_session_garble_evaluate.argtypes = [vp, vp, C.c_uint64, C.c_int, u8p]
        L.gsv_session_evaluate_streaming_indexed.argtypes = [vp, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64), u8p]
        L.gsv_session_evaluate_streaming_source.argtypes = [vp, C.c_uint64, CT_SOURCE_FN, vp, u8p]
        L.gsv_session_garble_streaming_commit.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, u8p, u8p]
        L.gsv_blake3_create.argtypes = [C.POINTER(vp)]
        L.gsv_blake3_destroy.argtypes = [vp]
        L.gsv_blake3_destroy.restype = None
        L.gsv_blake3_update.argtypes = [vp, u8p, C.c_uint64]
        L.gsv_blake3_absorb_subtree.argtypes = [vp, u8p, C.c_uint32]
        L.gsv_blake3_finalize.argtypes = [vp, u8p]
        L.gsv_blake3_file.argtypes = [C.c_char_p, u8p]
        L.gsv_engine_blake3_streams.argtypes = [vp, u8p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64, u8p]
        L.gsv_engine_blake3_streams_seconds.argtypes = [vp, C.POINTER(C.c_double)]
        L.gsv_session_evaluate_streaming_commit.argtypes = [vp, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, u8p, u8p]
        L.gsv_session_evaluate_streaming_source_commit.argtypes = [vp, C.c_uint64, CT_SOURCE_FN, vp, u8p, u8p]
        L.gsv_session_ciphertext_blake3.argtypes = [vp, u8p]
        L.gsv_blake3_outboard_root.argtypes = [u8p, C.c_uint64, u8p, C.c_uint64, u8p]
        L.gsv_blake3_file_outboard.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, u8p]
        L.gsv_session_garble_streaming_commit_outboard.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, u8p, u8p, C.c_char_p]
        L.gsv_engine_blake3_files.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(C.c_char_p), u8p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_session_evaluate_streaming_verified.argtypes = [vp, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_char_p, u8p, C.c_uint64, u8p, u8p]
        L.gsv_session_mismatch_info.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 3
        L.gsv_session_windows_launched.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.gsv_blake3_outboard_size.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_session_garble_streaming_sink_commit.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, CT_SINK_FN, vp, C.c_int, u8p, u8p, OUTBOARD_SINK_FN, vp, u8p]
        L.gsv_session_evaluate_streaming_source_verified.argtypes = [vp, C.c_uint64, CT_SOURCE_FN, vp, C.POINTER(u8p), C.POINTER(C.c_uint64), u8p, u8p, C.c_uint64, u8p, u8p]
        L.gsv_session_evaluate_streaming_calls.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_char_p, u8p, C.c_uint64, u8p, u8p]
        L.gsv_session_evaluate_streaming_source_calls.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, CT_SOURCE_FN, vp, C.POINTER(u8p), C.POINTER(C.c_uint64), u8p, u8p, C.c_uint64, u8p, u8p]
        L.gsv_session_evaluate_resume_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_cbcmac_checkpoints_size.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
        L.gsv_cbcmac_file_checkpoints.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, u8p]
        L.gsv_cbcmac_file_check.argtypes = [C.c_char_p, C.c_char_p, C.c_int, u8p, C.POINTER(C.c_uint64)]
        L.gsv_engine_cbcmac_streams_check.argtypes = [vp, u8p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_engine_cbcmac_streams_check_seconds.argtypes = [vp, C.POINTER(C.c_double)]
        L.gsv_engine_cbcmac_files.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(C.c_char_p), u8p, u8p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsv_session_garble_streaming_checkpoints.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, u8p, C.c_char_p]
        L.gsv_session_garble_streaming_check.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, u8p, u8p]
        L.gsv_session_evaluate_streaming_mac_calls.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_char_p, u8p, u8p]
        L.gsv_session_evaluate_streaming_source_mac_calls.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, CT_SOURCE_FN, vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint64), u8p, u8p]
        L.gsv_session_ciphertext_cbcmac_check.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, u8p, u8p]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise GsvError("gsv status %d: %s" % (rc, lib().gsv_last_error().decode(errors="replace")))


def _chk_mismatch(rc, place, resume=None):
    """_chk, but GSV_ERR_MISMATCH raises CiphertextMismatch at place() = (instance, group[, first_record]); resume() -> its resume_call."""
    if rc == 5:
        message = "gsv status 5: %s" % lib().gsv_last_error().decode(errors="replace")
        raise CiphertextMismatch(message, *place(), **({"resume_call": resume()} if resume else {}))
    _chk(rc)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None


def _rows(a, n=None):
    """The first n (default: all) rows of a 2-D uint8 array as a list of bytes; None stays None."""
    return None if a is None else [bytes(r) for r in a[:n]]


def _pack_expected(expected, n):
    """The commitments a verified evaluation trusts, one per instance -> (one uint8 array, bytes per commitment)."""
    exp = [bytes(e) for e in expected]
    if len(exp) != n or len(set(len(e) for e in exp)) != 1 or len(exp[0]) not in (16, 32):
        raise ValueError("expected: one commitment of 16 or of 32 bytes per instance")
    return np.frombuffer(b"".join(exp), np.uint8), len(exp[0])


def _u8(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a if shape is None else a.reshape(shape)


def labels_from_seed(seed, n_inputs):
    """(delta, false_label0, true_label0, input_label0[n_inputs,16]) as GarbleMode::new draws them
    (src/circuit/modes/garble_mode.rs:80-97,116-118)."""
    d, f, t = (np.zeros(16, np.uint8) for _ in range(3))
    inp = np.zeros((n_inputs, 16), np.uint8)
    _chk(lib().gsv_labels_from_seed(seed, n_inputs, _p(d), _p(f), _p(t), _p(inp)))
    return d, f, t, inp


def cbcmac(cts, state=None):
    """AESAccumulatingHash over 16-byte records (src/ciphertext_hasher.rs:23-29)."""
    st = np.zeros(16, np.uint8) if state is None else _u8(state).copy()
    a = _u8(cts).reshape(-1)
    _chk(lib().gsv_cbcmac_update(_p(st), _p(a) if a.size else None, a.size // 16))
    return st.tobytes()


def cbcmac_many(streams, states=None):
    """AESAccumulatingHash of several equally long streams at once (gsv_cbcmac_update_many: four chains side by side per step)."""
    arrs = [_u8(a).reshape(-1) for a in streams]
    n = arrs[0].size // 16
    assert all(a.size == n * 16 for a in arrs)
    st = np.zeros((len(arrs), 16), np.uint8) if states is None else _u8(states, (len(arrs), 16)).copy()
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    _chk(lib().gsv_cbcmac_update_many(_p(st), ptrs, len(arrs), n))
    return [bytes(st[i]) for i in range(len(arrs))]


class Blake3:
    """The host's incremental BLAKE3 (plain hash mode, 32-byte digest): update(bytes) any number of times, digest().  absorb_subtree(cv, k)
    takes the next 2^k chunks as the chaining value of their subtree — how a stream hashed on the device is finished."""

    def __init__(self):
        self.h = C.c_void_p()
        _chk(lib().gsv_blake3_create(C.byref(self.h)))

    def update(self, data):
        a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else _u8(data).reshape(-1)
        _chk(lib().gsv_blake3_update(self.h, _p(a) if a.size else None, a.size))
        return self

    def absorb_subtree(self, chaining_value, log2_chunks):
        _chk(lib().gsv_blake3_absorb_subtree(self.h, _p(np.frombuffer(bytes(chaining_value), np.uint8)), int(log2_chunks)))
        return self

    def digest(self):
        out = np.zeros(32, np.uint8)
        _chk(lib().gsv_blake3_finalize(self.h, _p(out)))
        return out.tobytes()

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.gsv_blake3_destroy(self.h)
            self.h = None


def blake3(data):
    """BLAKE3 (plain hash mode, 32 bytes) of a byte string / uint8 array: the commitment of a ciphertext stream given as gc-file bytes."""
    return Blake3().update(data).digest()


def blake3_file(path):
    """BLAKE3 of a file's bytes (a gc_<i>.bin: what the evaluator compares with the garbler's BLAKE3 commitment)."""
    out = np.zeros(32, np.uint8)
    _chk(lib().gsv_blake3_file(os.fsencode(path), _p(out)))
    return out.tobytes()


def outboard_file_name(index):
    """The BLAKE3 outboard of gc_<index>.bin, beside it (include/gsv_engine.h, "BLAKE3 outboards")."""
    return "gc_%d.b3o" % index


def blake3_outboard_root(outboard, last_chunk):
    """The root an outboard (bytes) folds to with the stream's last chunk (bytes: what lies behind the last whole KiB-chunk boundary
    in front of the end, 16 .. 1024 bytes; empty for the empty stream).  A malformed outboard raises GsvError (GSV_ERR_INVALID)."""
    ob = np.frombuffer(bytes(outboard), np.uint8)
    last = np.frombuffer(bytes(last_chunk), np.uint8)
    out = np.zeros(32, np.uint8)
    _chk(lib().gsv_blake3_outboard_root(_p(ob) if ob.size else _p(np.zeros(1, np.uint8)), ob.size, _p(last) if last.size else None, last.size, _p(out)))
    return out.tobytes()


def blake3_outboard_size(n_records, k):
    """(outboard_bytes, last_chunk_bytes) of a stream of n_records records in groups of 2^k chunks (k <= 20): how many bytes an
    outboard callback will receive per instance, and how many bytes of a last_chunks entry are the last chunk."""
    a, b = C.c_uint64(), C.c_uint64()
    _chk(lib().gsv_blake3_outboard_size(int(n_records), int(k), C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def blake3_file_outboard(path, k, outboard_path=None):
    """Writes the outboard of the file at `path` for groups of 2^k chunks to `outboard_path` (None: nowhere), on the host; returns
    the file's BLAKE3 digest."""
    out = np.zeros(32, np.uint8)
    _chk(lib().gsv_blake3_file_outboard(os.fsencode(path), int(k), os.fsencode(outboard_path) if outboard_path is not None else None, _p(out)))
    return out.tobytes()


def blake3_files(engine, paths, outboards=None):
    """BLAKE3 of equally long files on the device, read in bounded segments (GSV_DRAIN_SEGMENT_RECORDS records per file) without
    evaluating them: a list of 32-byte digests.  With `outboards` (one path per file) every group of 2^k chunks is compared with
    the file's outboard as it is hashed; the first difference raises CiphertextMismatch(instance = index into paths, group)."""
    n = len(paths)
    arr = (C.c_char_p * max(1, n))(*[os.fsencode(q) for q in paths])
    obs = None
    if outboards is not None:
        assert len(outboards) == n
        obs = (C.c_char_p * max(1, n))(*[os.fsencode(q) for q in outboards])
    out = np.zeros((max(1, n), 32), np.uint8)
    bad_file, bad_group = C.c_uint64(), C.c_uint64()
    rc = lib().gsv_engine_blake3_files(engine.h, arr, n, obs, _p(out), C.byref(bad_file), C.byref(bad_group))
    _chk_mismatch(rc, lambda: (int(bad_file.value), int(bad_group.value)))
    return _rows(out, n)


def blake3_streams(engine, array, segments, with_seconds=False):
    """BLAKE3 of n equally long streams on the device: `array` is [n_streams, records, 16] uint8, `segments` the record counts in which
    the streams are fed to the drain's chunk / reduce / carry kernels (they add up to `records`).  Returns n_streams 32-byte digests;
    with_seconds=True: (digests, device seconds from the first hash kernel to the last)."""
    a = _u8(array)
    assert a.ndim == 3 and a.shape[2] == 16, a.shape
    seg = (C.c_uint64 * max(1, len(segments)))(*[int(x) for x in segments])
    out = np.zeros((a.shape[0], 32), np.uint8)
    _chk(lib().gsv_engine_blake3_streams(engine.h, _p(a) if a.size else None, a.shape[0], a.shape[1], seg, len(segments), _p(out)))
    digests = _rows(out)
    if not with_seconds:
        return digests
    s = C.c_double()
    _chk(lib().gsv_engine_blake3_streams_seconds(engine.h, C.byref(s)))
    return digests, s.value


_MAC_GROUP_DEFAULT = 0xFFFFFFFF  # GSV_MAC_GROUP_DEFAULT: the knob GSV_MAC_GROUP_LOG2
_NO_PLACE = (1 << 64) - 1


def checkpoint_file_name(index):
    """The CBC-MAC checkpoints of gc_<index>.bin, beside it (include/gsv_engine.h, "CBC-MAC checkpoints")."""
    return "gc_%d.mck" % index


def cbcmac_checkpoints_size(n_records, k=None):
    """Bytes of the checkpoint file of a stream of n_records records with a chain state every 2^k records (k <= 30; None:
    GSV_MAC_GROUP_LOG2)."""
    a = C.c_uint64()
    _chk(lib().gsv_cbcmac_checkpoints_size(int(n_records), _MAC_GROUP_DEFAULT if k is None else int(k), C.byref(a)))
    return int(a.value)


def cbcmac_file_checkpoints(path, k=None, out_path=None):
    """Writes the checkpoints of the file at `path` — its CBC-MAC chain state after every 2^k records (None: GSV_MAC_GROUP_LOG2) — to
    `out_path` (None: nowhere), on the host; returns the file's CBC-MAC."""
    out = np.zeros(16, np.uint8)
    _chk(lib().gsv_cbcmac_file_checkpoints(os.fsencode(path), _MAC_GROUP_DEFAULT if k is None else int(k), os.fsencode(out_path) if out_path is not None else None, _p(out)))
    return out.tobytes()


def cbcmac_file_check(path, checkpoints, threads=0):
    """The file at `path` against its checkpoint file, on the host, groups in parallel over `threads` threads: (CBC-MAC, None) when
    every group holds — the CBC-MAC is then the checkpoint file's last state — else (None, the lowest group that does not).  A
    malformed checkpoint file, or one for another file length, raises GsvError (GSV_ERR_INVALID)."""
    out = np.zeros(16, np.uint8)
    bad = C.c_uint64()
    rc = lib().gsv_cbcmac_file_check(os.fsencode(path), os.fsencode(checkpoints), int(threads), _p(out), C.byref(bad))
    if rc == 5:
        return None, int(bad.value)
    _chk(rc)
    return out.tobytes(), None


def cbcmac_files(engine, paths, checkpoints, expected=None):
    """CBC-MAC commitments of equally long files verified on the device against their checkpoint files (one path per file), read in
    bounded segments (GSV_DRAIN_SEGMENT_RECORDS records per file) without evaluating them: a list of 16-byte CBC-MACs.  expected: one
    trusted 16-byte commitment per file, compared with the checkpoint file's last state before anything is uploaded.  The first
    difference — the lowest group, then the lowest file — raises CiphertextMismatch(instance = index into paths, group, first_record);
    group and first_record are None when a last state did not match `expected`."""
    n = len(paths)
    assert len(checkpoints) == n
    arr = (C.c_char_p * max(1, n))(*[os.fsencode(q) for q in paths])
    cks = (C.c_char_p * max(1, n))(*[os.fsencode(q) for q in checkpoints])
    exp = None
    if expected is not None:
        exp = np.frombuffer(b"".join(bytes(e) for e in expected), np.uint8)
        if exp.size != 16 * n:
            raise ValueError("expected: one 16-byte commitment per file")
    out = np.zeros((max(1, n), 16), np.uint8)
    bad_file, bad_group = C.c_uint64(), C.c_uint64()
    rc = lib().gsv_engine_cbcmac_files(engine.h, arr, n, cks, _p(exp), _p(out), C.byref(bad_file), C.byref(bad_group))

    def place():
        if bad_group.value == _NO_PLACE:
            return int(bad_file.value), None, None
        k = int.from_bytes(open(checkpoints[int(bad_file.value)], "rb").read(16)[12:16], "little")
        return int(bad_file.value), int(bad_group.value), int(bad_group.value) << k
    _chk_mismatch(rc, place)
    return _rows(out, n)


def cbcmac_streams_check(engine, array, segments, checkpoints, with_seconds=False):
    """The device check alone: `array` is [n_streams, records, 16] uint8, `segments` the record counts in which the streams are fed to
    the check kernel (they add up to `records`), `checkpoints` one checkpoint file's bytes per stream.  Returns None when every group
    of every stream holds, else (stream, group) of the lowest group that does not (then the lowest stream); with_seconds=True:
    (that, device seconds)."""
    a = _u8(array)
    assert a.ndim == 3 and a.shape[2] == 16, a.shape
    cks = [bytes(c) for c in checkpoints]
    assert len(cks) == a.shape[0] and len(set(len(c) for c in cks)) == 1
    ck = np.frombuffer(b"".join(cks), np.uint8)
    seg = (C.c_uint64 * max(1, len(segments)))(*[int(x) for x in segments])
    bad_stream, bad_group = C.c_uint64(), C.c_uint64()
    rc = lib().gsv_engine_cbcmac_streams_check(engine.h, _p(a) if a.size else None, a.shape[0], a.shape[1], seg, len(segments), _p(ck), len(cks[0]), C.byref(bad_stream), C.byref(bad_group))
    if rc != 5:
        _chk(rc)
    found = (int(bad_stream.value), int(bad_group.value)) if rc == 5 else None
    if not with_seconds:
        return found
    s = C.c_double()
    _chk(lib().gsv_engine_cbcmac_streams_check_seconds(engine.h, C.byref(s)))
    return found, s.value


def cbcmac_chains_per_step():
    """How many chains one host thread advances side by side (16 with VAES + AVX-512, 4 with AES-NI)."""
    return int(lib().gsv_cbcmac_chains_per_step())


class Program:
    """A recorded circuit compiled to device steps (gsv_recorder + gsv_program)."""

    def __init__(self, handle):
        self.h = handle
        _live["program"].add(self)
        info = _ProgramInfo()
        _chk(lib().gsv_program_get_info(self.h, C.byref(info)))
        self.info = {n: (list(getattr(info, n)) if n == "gate_count" else int(getattr(info, n))) for n, _ in _ProgramInfo._fields_}

    def step_stats(self):
        """Diagnostics: per step [and_cnt, xor_cnt, lds_reads, hbm_reads, lds_writes, hbm_writes]."""
        out = np.zeros((self.info["n_steps"], 6), np.uint32)
        _chk(lib().gsv_program_step_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    @classmethod
    def from_circuit(cls, spec, chain_feedback=False):
        """Record one of the built-in restated circuits through the two-pass credit driver and compile it.
        chain_feedback: output i is copied to input i after every replay (component chains)."""
        L = lib()
        r = C.c_void_p()
        _chk(L.gsv_recorder_create(C.byref(r)))
        try:
            _chk(L.gsv_recorder_record_circuit(r, spec.encode()))
            return cls._compile(r, chain_feedback)
        finally:
            L.gsv_recorder_destroy(r)

    @classmethod
    def from_gates(cls, n_inputs, gates, outputs, credits=None, feedback=None, for_plan=None, window_div=None):
        """Record an explicit gate list through the CircuitMode-shaped recorder API.
        gates: iterable of (gate_type, a, b, c) with wire ids: 0/1 constants, inputs 2..2+n_inputs-1, further
        wires in first-write order; c == None marks a dead gate (UNREACHABLE).
        feedback: [(output index, input index)] copied after every replay (gsv_program_compile's feedback lists; the sources may be
        the destinations of other pairs).  for_plan: the PlanRecorder the program is a unit of — it is compiled once, for the
        recorder's window_div (gsv_program_compile_opts), and cannot have feedback.  window_div = 2 | 4: ONE image for half / a quarter
        of the LDS label window, the trace is not kept (no variant is compiled when a session asks for another layout)."""
        L = lib()
        r = C.c_void_p()
        _chk(L.gsv_recorder_create(C.byref(r)))
        try:
            known = set()
            for _ in range(n_inputs):
                w = C.c_uint64()
                _chk(L.gsv_recorder_allocate_wire(r, 1, C.byref(w)))
                _chk(L.gsv_recorder_declare_input(r, w.value))
                known.add(w.value)
            arr = (_Gate * max(1, len(gates)))()
            for i, (t, a, b, c) in enumerate(gates):
                if c is not None and c not in known and c >= 2:
                    w = C.c_uint64()
                    _chk(L.gsv_recorder_allocate_wire(r, 1, C.byref(w)))
                    if w.value != c:
                        raise GsvError("from_gates: wires must be numbered in first-write order (expected %d, got %d)" % (w.value, c))
                    known.add(c)
                arr[i].wire_a, arr[i].wire_b, arr[i].gate_type = a, b, t
                arr[i].wire_c = 0xFFFFFFFFFFFFFFFF if c is None else c
            _chk(L.gsv_recorder_push_gates(r, arr, len(gates)))
            outs = (C.c_uint64 * max(1, len(outputs)))(*outputs)
            _chk(L.gsv_recorder_declare_outputs(r, outs, len(outputs)))
            if for_plan is not None or window_div is not None:
                if feedback:
                    raise ValueError("feedback lists go through gsv_program_compile: not with for_plan / window_div")
                h = C.c_void_p()
                o = _CompileOpts(struct_size=C.sizeof(_CompileOpts), window_div=int(window_div or 0), for_plan=for_plan.h if for_plan is not None else None)
                _chk(L.gsv_program_compile_opts(r, C.byref(o), C.byref(h)))
                return cls(h)
            if feedback:
                h = C.c_void_p()
                src = (C.c_uint32 * len(feedback))(*[int(a) for a, _ in feedback])
                dst = (C.c_uint32 * len(feedback))(*[int(b) for _, b in feedback])
                _chk(L.gsv_program_compile(r, src, dst, len(feedback), C.byref(h)))
                return cls(h)
            return cls._compile(r, False)
        finally:
            L.gsv_recorder_destroy(r)

    @classmethod
    def _compile(cls, r, chain_feedback):
        L = lib()
        h = C.c_void_p()
        if chain_feedback:
            no = C.c_uint64()
            _chk(L.gsv_recorder_counts(r, None, C.byref(no), None))
            n_out = no.value
            idx = (C.c_uint32 * n_out)(*range(n_out))
            _chk(L.gsv_program_compile(r, idx, idx, n_out, C.byref(h)))
        else:
            _chk(L.gsv_program_compile(r, None, None, 0, C.byref(h)))
        return cls(h)

    def close(self):
        if getattr(self, "h", None) is not None and _lib is not None and not sys.is_finalizing():
            _lib.gsv_program_destroy(self.h)
        self.h = None

    __del__ = close


class Engine:
    """One GPU (gsv_engine).  Creation fails loudly when no HIP device is present."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _chk(lib().gsv_engine_create(device, C.byref(self.h)))
        self.device = device
        _live["engine"].add(self)

    def close(self):
        # sessions (and plans loaded straight into this device) use the engine's stream and device: they go first, whoever still holds them
        # (a session kept alive by a reference cycle and collected after the engine was closed ran gsv_session_destroy on a freed engine)
        if getattr(self, "h", None) is not None and self.h:
            for kind in ("session", "plan"):
                for s in list(_live[kind]):
                    if getattr(s, "engine", None) is self:
                        s.close()
        if getattr(self, "h", None) is not None and _lib is not None and self.h and not sys.is_finalizing():
            _lib.gsv_engine_destroy(self.h)
        self.h = None

    __del__ = close


class Plan:
    """A sequence of calls to compiled programs over one wire file (gsv_plan): component-level programs."""

    def __init__(self):
        self.h = C.c_void_p()
        _chk(lib().gsv_plan_create(C.byref(self.h)))
        _live["plan"].add(self)
        self.programs = []  # keep the programs alive
        self.n_inputs = self.n_outputs = 0

    @classmethod
    def from_circuit(cls, spec, units, half_window=False, window_div=None):
        """Record a built-in circuit with the named components (list of names such as "fq12::mul_montgomery") as calls.
        window_div = 2 | 4 (half_window=True is window_div=2): compile every program once, for half / a quarter of the LDS label
        window; the one image then serves every layout of up to that many instances per workgroup and the recorded traces are not
        kept — a third less host memory and one compilation for plans with hundreds of programs."""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        self.programs = []
        _live["plan"].add(self)
        div = int(window_div) if window_div else (2 if half_window else 1)
        if div not in (1, 2, 4):
            raise ValueError("window_div must be 1, 2 or 4")
        _chk(lib().gsv_plan_from_circuit_div(spec.encode(), ",".join(units).encode(), div if div > 1 else 0, C.byref(self.h)))  # 0: as GSV_PLAN_WINDOW_DIV / GSV_PLAN_HALF_WINDOW say
        self._read_info()
        return self

    @staticmethod
    def build_file(spec, units, path, window_div=4):
        """Build the plan of a built-in circuit straight into the plan file `path` (gsv_plan_build_file_div): every program is written
        by the worker that compiled it and dropped from memory.  Load it with Plan.load(path, engine)."""
        if int(window_div) not in (1, 2, 4):
            raise ValueError("window_div must be 1, 2 or 4 (one image per program; 1 = full LDS window, one instance per workgroup only)")
        _chk(lib().gsv_plan_build_file_div(spec.encode(), ",".join(units).encode(), os.fsencode(path), int(window_div)))

    @staticmethod
    def build_file_pair(spec, units_a, path_a, window_div_a, path_b, window_div_b, units_b=None):
        """Two plan files from ONE build (gsv_plan_build_file_pair): the units both plans share are recorded once and compiled for both
        shares of the LDS window (units_b None: the same units).  Each file equals what build_file writes for its units and window_div."""
        _chk(lib().gsv_plan_build_file_pair(spec.encode(), ",".join(units_a).encode(), os.fsencode(path_a), int(window_div_a),
                                            ",".join(units_b).encode() if units_b is not None else None, os.fsencode(path_b), int(window_div_b)))

    def _read_info(self):
        g, c, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _chk(lib().gsv_plan_counts(self.h, C.byref(g), C.byref(c), C.byref(k)))
        n_in, n_out = C.c_uint64(), C.c_uint64()
        _chk(lib().gsv_plan_io(self.h, C.byref(n_in), C.byref(n_out)))
        self.n_inputs, self.n_outputs = n_in.value, n_out.value
        self.info = {"n_inputs": n_in.value, "n_outputs": n_out.value, "n_gates": g.value, "n_ciphertexts": c.value, "n_calls": k.value, "n_steps": 0}

    def save(self, path):
        """Write the finished plan (compiled programs + calls) to `path` (gsv_plan_save)."""
        _chk(lib().gsv_plan_save(self.h, os.fsencode(path)))

    @classmethod
    def load(cls, path, engine=None):
        """Read a plan file.  With `engine` the program records go straight into that GPU's memory and the host keeps
        only metadata (the ranks of a node share the file through the page cache); without, a complete host copy."""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        self.programs = []
        _live["plan"].add(self)
        self.engine = engine  # a device-resident plan must not outlive its engine
        _chk(lib().gsv_plan_load(os.fsencode(path), engine.h if engine is not None else None, C.byref(self.h)))
        self._read_info()
        return self

    def image_bytes(self):
        """(bytes of compiled program records, number of distinct programs)."""
        b, n = C.c_uint64(), C.c_uint64()
        _chk(lib().gsv_plan_image_bytes(self.h, C.byref(b), C.byref(n)))
        return b.value, n.value

    def wire_file(self):
        """(global wire slots, largest program's own slots): a session's wire file is their sum x 16 bytes per instance."""
        g, m = C.c_uint64(), C.c_uint64()
        _chk(lib().gsv_plan_wire_file(self.h, C.byref(g), C.byref(m)))
        return g.value, m.value

    def call_info(self):
        """Per call: [gate offset, gates, ciphertext offset, ciphertexts, device steps] as a uint64 array [n_calls, 5]."""
        n = self.info["n_calls"]
        out = np.zeros((n, 5), np.uint64)
        v = [C.c_uint64() for _ in range(5)]
        for k in range(n):
            _chk(lib().gsv_plan_call_info(self.h, k, *[C.byref(x) for x in v]))
            out[k] = [x.value for x in v]
        return out

    def call_record_forms(self):
        """Per call: wires per AND input of its program's records (2 or 4); a window with a four-wire program runs the FW kernel."""
        v = C.c_uint32()
        out = []
        for k in range(self.info["n_calls"]):
            _chk(lib().gsv_plan_call_record_form(self.h, k, C.byref(v)))
            out.append(int(v.value))
        return out

    def add_call(self, program, in_globals, out_globals):
        a = np.ascontiguousarray(in_globals, np.uint32)
        b = np.ascontiguousarray(out_globals, np.uint32)
        assert a.size == program.info["n_inputs"] and b.size == program.info["n_outputs"]
        _chk(lib().gsv_plan_add_call(self.h, program.h, a.ctypes.data_as(C.POINTER(C.c_uint32)), b.ctypes.data_as(C.POINTER(C.c_uint32))))
        self.programs.append(program)

    def finish(self, n_inputs, output_globals):
        o = np.ascontiguousarray(output_globals, np.uint32)
        _chk(lib().gsv_plan_finish(self.h, n_inputs, o.ctypes.data_as(C.POINTER(C.c_uint32)), o.size))
        self.n_inputs, self.n_outputs = n_inputs, int(o.size)
        g, c, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _chk(lib().gsv_plan_counts(self.h, C.byref(g), C.byref(c), C.byref(k)))
        self.info = {"n_inputs": n_inputs, "n_outputs": int(o.size), "n_gates": g.value, "n_ciphertexts": c.value, "n_calls": k.value, "n_steps": 0}

    def close(self):
        if getattr(self, "h", None) and _lib is not None and not sys.is_finalizing():
            _lib.gsv_plan_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlanRecorder:
    """The plan builder driven gate by gate through the C ABI (gsv_plan_recorder_*): what a host with its own two-pass
    driver uses.  Wires: 0 / 1 constants, further ids handed out by allocate_wire."""

    def __init__(self, window_div=None):
        """window_div = 2 | 4 (gsv_plan_recorder_create_opts): the glue programs, and every unit compiled with
        Program.from_gates(for_plan=this recorder), exist as ONE image for half / a quarter of the LDS label window that serves every
        layout of up to that many instances per workgroup; no other variant is compiled later."""
        self.h = C.c_void_p()
        if window_div is None:
            _chk(lib().gsv_plan_recorder_create(C.byref(self.h)))
        else:
            if int(window_div) not in (1, 2, 4):
                raise ValueError("window_div must be 1, 2 or 4")
            o = _PlanRecorderOpts(C.sizeof(_PlanRecorderOpts), int(window_div), None)
            _chk(lib().gsv_plan_recorder_create_opts(C.byref(o), C.byref(self.h)))
        self.programs = []
        self.n_inputs = 0

    def allocate_wire(self, credits=1):
        w = C.c_uint64()
        _chk(lib().gsv_plan_recorder_allocate_wire(self.h, credits, C.byref(w)))
        return w.value

    def input_wire(self):
        w = self.allocate_wire(1)
        _chk(lib().gsv_plan_recorder_declare_input(self.h, w))
        self.n_inputs += 1
        return w

    def push_gates(self, gates):
        """gates: list of (gate_type, a, b, c); c == None marks a dead gate."""
        arr = (_Gate * max(1, len(gates)))()
        for i, (t, a, b, c) in enumerate(gates):
            arr[i].wire_a, arr[i].wire_b, arr[i].gate_type = a, b, t
            arr[i].wire_c = 0xFFFFFFFFFFFFFFFF if c is None else c
        _chk(lib().gsv_plan_recorder_push_gates(self.h, arr, len(gates)))

    def call(self, program, in_wires):
        self.programs.append(program)
        a = (C.c_uint64 * max(1, len(in_wires)))(*in_wires)
        n_out = program.info["n_outputs"]
        o = (C.c_uint64 * max(1, n_out))()
        assert len(in_wires) == program.info["n_inputs"]
        _chk(lib().gsv_plan_recorder_call(self.h, program.h, a, o))
        return list(o[:n_out])

    def finish(self, output_wires):
        plan = Plan.__new__(Plan)
        plan.h = C.c_void_p()
        _live["plan"].add(plan)
        plan.programs = list(self.programs)
        o = (C.c_uint64 * max(1, len(output_wires)))(*output_wires)
        _chk(lib().gsv_plan_recorder_finish(self.h, o, len(output_wires), C.byref(plan.h)))
        g, c, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _chk(lib().gsv_plan_counts(plan.h, C.byref(g), C.byref(c), C.byref(k)))
        plan.n_inputs, plan.n_outputs = self.n_inputs, len(output_wires)
        plan.info = {"n_inputs": self.n_inputs, "n_outputs": len(output_wires), "n_gates": g.value, "n_ciphertexts": c.value, "n_calls": k.value, "n_steps": 0}
        return plan

    def close(self):
        if self.h:
            lib().gsv_plan_recorder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_commitment(commitment, discard, outboard_dir=None):
    if commitment not in ("cbcmac", "blake3", "both"):
        raise ValueError("commitment must be 'cbcmac', 'blake3' or 'both'")
    if discard and commitment != "cbcmac":
        raise ValueError("discard=True drops the ciphertexts: it cannot be combined with commitment=%r" % commitment)
    if outboard_dir is not None and commitment == "cbcmac":
        raise ValueError("outboard_dir needs commitment='blake3' or 'both': an outboard holds the values of the BLAKE3 commitment")


class Session:
    """A batch of instances on one program (gsv_session) or, with a Plan, on a sequence of component programs."""

    def __init__(self, engine, program, n_instances=1, replays=1, ct_capacity_replays=None, retain_stream=True, concurrent_calls=0, window_ct_records=0,
                 max_scratch_slots=0, max_window_calls=0, drain_segment_records=0):
        """Plan sessions: retain_stream = True (the whole stream stays on the device), False (one window of it) or "ring" (GSV_STREAM_RING:
        the whole pass as one launch over a ciphertext ring); concurrent_calls = how many independent calls of the plan may run side by
        side (0: as many as give every CU a workgroup, 1: sequential); window_ct_records / max_scratch_slots / max_window_calls: see gsv_plan_session_opts (0 = automatic)."""
        self.engine, self.program = engine, program
        self.n, self.replays = n_instances, replays
        self.ct_cap = replays if ct_capacity_replays is None else ct_capacity_replays
        self.h = C.c_void_p()
        if isinstance(program, Plan):
            assert replays == 1
            if retain_stream == "ring" or (retain_stream is not True and retain_stream is not False and retain_stream == 2):
                rs = 2  # GSV_STREAM_RING
            elif retain_stream in (True, False, 0, 1):
                rs = int(bool(retain_stream))
            else:
                raise ValueError("retain_stream must be True, False, 0, 1, 2 or \"ring\"")
            o = _PlanSessionOpts(rs, int(concurrent_calls), int(window_ct_records), int(max_scratch_slots), int(max_window_calls), int(drain_segment_records))
            _chk(lib().gsv_session_create_plan_opts(engine.h, program.h, n_instances, C.byref(o), C.byref(self.h)))
        else:
            _chk(lib().gsv_session_create(engine.h, program.h, n_instances, replays, self.ct_cap, C.byref(self.h)))
        self.n_in, self.n_out = program.info["n_inputs"], program.info["n_outputs"]
        _live["session"].add(self)

    def set_garble_inputs(self, delta, const_label0, input_label0):
        d = _u8(delta, (self.n, 16))
        c = _u8(const_label0, (self.n, 32))
        i = _u8(input_label0, (self.n, self.n_in * 16))
        _chk(lib().gsv_session_set_garble_inputs(self.h, _p(d), _p(c), _p(i) if self.n_in else None))

    def garble(self, gate_id_base=0):
        _chk(lib().gsv_session_garble(self.h, gate_id_base))

    def _garble_commit(self, commitment, gate_id_base, first_call, n_calls, directory, first_index, threads, outboard_dir=None):
        """commitment "blake3" | "both" (gsv_session_garble_streaming_commit): BLAKE3 digests are computed on the device and reported by the
        call that ends the pass (None before); "both" returns (CBC-MACs, digests)."""
        if commitment not in ("blake3", "both"):
            raise ValueError("commitment must be 'cbcmac', 'blake3' or 'both'")
        n = getattr(self, "n_drain", self.n)
        macs = np.zeros((self.n, 16), np.uint8) if commitment == "both" else None
        dig = np.zeros((n, 32), np.uint8)
        with _gc_paused():
            _chk(lib().gsv_session_garble_streaming_commit_outboard(self.h, gate_id_base, first_call, n_calls, directory.encode() if directory else None, first_index, threads, _p(macs), _p(dig),
                                                                    os.fsencode(outboard_dir) if outboard_dir is not None else None))
        digests = _rows(dig) if self._ends_pass(first_call, n_calls) else None  # (else the engine leaves `dig` alone)
        return (_rows(macs), digests) if commitment == "both" else digests

    def _ends_pass(self, first_call, n_calls):
        """Does the slice [first_call, first_call + n_calls) of a streaming garble (0, 0: all of it) end its pass?"""
        return (first_call == 0 and n_calls == 0) or not isinstance(self.program, Plan) or first_call + n_calls == self.schedule_info()["n_calls"]

    def _garble_checkpoints(self, gate_id_base, first_call, n_calls, directory, first_index, threads, checkpoint_dir):
        out = np.zeros((self.n, 16), np.uint8)
        with _gc_paused():
            _chk(lib().gsv_session_garble_streaming_checkpoints(self.h, gate_id_base, first_call, n_calls, directory.encode() if directory else None, first_index, threads, _p(out),
                                                                os.fsencode(checkpoint_dir)))
        return _rows(out)

    def garble_check(self, checkpoint_dir, first_index=0, indexes=None, first_call=0, n_calls=0, expected=None, gate_id_base=0):
        """Garble and verify the streams against the CBC-MAC checkpoint files <checkpoint_dir>/gc_<index>.mck (index = indexes[i], or
        first_index + i) on the device: nothing is drained and no host MAC worker runs.  Plan sessions may run it in slices (first_call,
        n_calls; 0, 0: the whole pass), every slice of a pass with the same check.  expected: one trusted 16-byte commitment per
        instance, compared with the files' last states before anything is launched.  Returns the verified CBC-MACs from the call that
        ends the pass (None before); a stream that differs raises CiphertextMismatch(instance, group, first_record)."""
        n = getattr(self, "n_drain", self.n)
        idx_p = None
        if indexes is not None:
            idx = np.ascontiguousarray(indexes, np.uint64)
            assert idx.size == n
            idx_p = idx.ctypes.data_as(C.POINTER(C.c_uint64))
        exp = None
        if expected is not None:
            exp = np.frombuffer(b"".join(bytes(e) for e in expected), np.uint8)
            if exp.size != 16 * n:
                raise ValueError("expected: one 16-byte commitment per instance")
        out = np.zeros((n, 16), np.uint8)
        with _gc_paused():
            rc = lib().gsv_session_garble_streaming_check(self.h, gate_id_base, first_call, n_calls, os.fsencode(checkpoint_dir), idx_p, first_index, _p(exp), _p(out))
        _chk_mismatch(rc, self.mismatch_info)
        return _rows(out) if self._ends_pass(first_call, n_calls) else None

    def garble_streaming(self, gate_id_base=0, directory=None, first_index=0, threads=0, discard=False, commitment="cbcmac", outboard_dir=None, checkpoint_dir=None):
        """Garble all replays while the host drains the stream segment by segment: returns the per-instance ciphertext
        hashes (CBC-MAC, gate order) and, with `directory`, writes gc_<first_index+i>.bin files.  discard=True: garble
        only, the ciphertexts are dropped.  commitment="blake3": 32-byte BLAKE3 digests of the streams instead, computed on the
        device (nothing of the stream is copied out unless `directory` is given); "both": (CBC-MACs, BLAKE3 digests).
        outboard_dir (with "blake3" / "both"): the BLAKE3 outboards gc_<first_index+i>.b3o are written there.
        checkpoint_dir (with "cbcmac"): the CBC-MAC checkpoint files gc_<first_index+i>.mck are written there (k = GSV_MAC_GROUP_LOG2)."""
        _check_commitment(commitment, discard, outboard_dir)
        if checkpoint_dir is not None:
            if commitment != "cbcmac" or discard:
                raise ValueError("checkpoint_dir needs commitment='cbcmac' and discard=False: the files hold the states of the CBC-MAC")
            return self._garble_checkpoints(gate_id_base, 0, 0, directory, first_index, threads, checkpoint_dir)
        if commitment != "cbcmac":
            return self._garble_commit(commitment, gate_id_base, 0, 0, directory, first_index, threads, outboard_dir)
        if discard:
            directory, first_index, threads = None, 0, 0
        out = None if discard else np.zeros((self.n, 16), np.uint8)
        with _gc_paused():
            _chk(lib().gsv_session_garble_streaming(self.h, gate_id_base, directory.encode() if directory else None, first_index, threads, _p(out)))
        return _rows(out)

    def garble_calls(self, first_call, n_calls, gate_id_base=0, directory=None, first_index=0, threads=0, discard=False, commitment="cbcmac", outboard_dir=None, checkpoint_dir=None):
        """Plan sessions: garble calls [first_call, first_call + n_calls) only (a slice of the plan).  Wires, gate ids and the
        CBC-MAC states continue from the previous slice; first_call == 0 starts a new pass.  Returns the MAC states after the
        slice (the commitments once the last slice has run), or None with discard=True.  commitment="blake3" / "both" as for
        garble_streaming: the BLAKE3 state chains from slice to slice too, the digests are None until the slice that ends the pass.
        outboard_dir as for garble_streaming, in every slice of the pass: the first slice truncates the outboards, later ones append;
        checkpoint_dir likewise."""
        _check_commitment(commitment, discard, outboard_dir)
        if checkpoint_dir is not None:
            if commitment != "cbcmac" or discard:
                raise ValueError("checkpoint_dir needs commitment='cbcmac' and discard=False: the files hold the states of the CBC-MAC")
            if first_call == 0 and n_calls == 0:
                raise ValueError("an empty slice")  # (0, 0 means the whole pass to the C entry point)
            return self._garble_checkpoints(gate_id_base, first_call, n_calls, directory, first_index, threads, checkpoint_dir)
        if commitment != "cbcmac":
            if first_call == 0 and n_calls == 0:
                raise ValueError("an empty slice")  # (0, 0 means the whole pass to the C entry point)
            return self._garble_commit(commitment, gate_id_base, first_call, n_calls, directory, first_index, threads, outboard_dir)
        if discard:
            directory, first_index, threads = None, 0, 0
        out = None if discard else np.zeros((self.n, 16), np.uint8)
        with _gc_paused():
            _chk(lib().gsv_session_garble_streaming_calls(self.h, gate_id_base, first_call, n_calls, directory.encode() if directory else None, first_index, threads, _p(out)))
        return _rows(out)

    def garble_to_sink(self, handler, gate_id_base=0, first_call=0, n_calls=0, threads=0, with_hashes=False, commitment=None, outboards=False):
        """Garble with every ciphertext handed to `handler(instance, first_record, records)` — the generic CiphertextHandler
        (circuit/mod.rs:140-178): `records` is an [n,16] uint8 array in gate order, valid during the call only; the runs of one
        instance arrive in stream order.  Exceptions raised by the handler abort the pass.  Returns the CBC-MACs with
        with_hashes=True.
        commitment="cbcmac" | "blake3" | "both" (gsv_session_garble_streaming_sink_commit) returns a SinkCommit(cbcmac, blake3,
        outboards, last_chunks) instead, one entry per drained instance: `cbcmac` the MAC states after this call (None with
        "blake3"); `blake3` the 32-byte digests, computed on the device, and `last_chunks` the streams' last chunks as bytes — both
        None with "cbcmac", and None until the slice that ends the pass; `outboards` (outboards=True, with "blake3" / "both") the
        BLAKE3 outboards as bytes, accumulated on the session from slice to slice and returned by the slice that ends the pass,
        None before.  `handler` may then be None: with "blake3" nothing of the stream is copied to the host."""
        if commitment is None:
            if outboards:
                raise ValueError("outboards=True needs commitment='blake3' or 'both': an outboard holds the values of the BLAKE3 commitment")
            if handler is None:
                raise ValueError("a handler, a commitment, or both")
        elif commitment not in ("cbcmac", "blake3", "both"):
            raise ValueError("commitment must be None, 'cbcmac', 'blake3' or 'both'")
        elif outboards and commitment == "cbcmac":
            raise ValueError("outboards=True needs commitment='blake3' or 'both': an outboard holds the values of the BLAKE3 commitment")
        failure = []

        def _cb(_user, inst, first, ptr, n):
            try:
                handler(int(inst), int(first), np.ctypeslib.as_array(ptr, shape=(int(n), 16)))
                return 0
            except BaseException as e:  # noqa: BLE001 - must not unwind through the C frames
                failure.append(e)
                return 1

        cb = CT_SINK_FN(_cb) if handler is not None else CT_SINK_FN()
        if commitment is None:
            out = np.zeros((self.n, 16), np.uint8) if with_hashes else None
            with _gc_paused():
                rc = lib().gsv_session_garble_streaming_sink(self.h, gate_id_base, first_call, n_calls, cb, None, threads, _p(out))
            if failure:
                raise failure[0]
            _chk(rc)
            return _rows(out)
        n = getattr(self, "n_drain", self.n)
        ends_pass = self._ends_pass(first_call, n_calls)  # (else the engine leaves the digests alone)
        b3 = commitment != "cbcmac"
        macs = np.zeros((n, 16), np.uint8) if commitment != "blake3" else None
        dig = np.zeros((n, 32), np.uint8) if b3 else None
        last = np.zeros((n, 1024), np.uint8) if b3 else None
        if outboards and first_call == 0:
            self._sink_outboards = [bytearray() for _ in range(n)]  # a slice that starts at call 0 starts every outboard again
        acc = getattr(self, "_sink_outboards", None)

        def _ob(_user, inst, offset, ptr, n_bytes):
            try:
                buf = acc[int(inst)]
                if int(offset) != len(buf):
                    raise GsvError("outboard of instance %d: bytes at offset %d, %d were expected" % (inst, offset, len(buf)))
                buf += C.string_at(ptr, int(n_bytes))
                return 0
            except BaseException as e:  # noqa: BLE001
                failure.append(e)
                return 1

        if outboards and (acc is None or len(acc) != n):
            raise GsvError("this slice continues a pass whose earlier slices collected no outboards for these instances")
        ob_cb = OUTBOARD_SINK_FN(_ob) if outboards else OUTBOARD_SINK_FN()
        with _gc_paused():
            rc = lib().gsv_session_garble_streaming_sink_commit(self.h, gate_id_base, first_call, n_calls, cb, None, threads, _p(macs), _p(dig), ob_cb, None, _p(last))
        if failure:
            raise failure[0]
        _chk(rc)
        if b3 and ends_pass:
            total = self.program.info["n_ciphertexts"] * (1 if isinstance(self.program, Plan) else self.replays)
            last_bytes = blake3_outboard_size(total, 0)[1]
        return SinkCommit(_rows(macs),
                          _rows(dig) if b3 and ends_pass else None,
                          [bytes(x) for x in acc] if outboards and ends_pass else None,
                          _rows(last[:, :last_bytes]) if b3 and ends_pass else None)

    def garble_evaluate(self, evaluator, gate_id_base=0, threads=0, with_hashes=False):
        """Garble this (plan, retain_stream=False) session while `evaluator` — a session of the same plan and options with its inputs
        set — evaluates every window straight from this session's device block (gsv_session_garble_evaluate)."""
        out = np.zeros((self.n, 16), np.uint8) if with_hashes else None
        with _gc_paused():
            _chk(lib().gsv_session_garble_evaluate(self.h, evaluator.h, gate_id_base, threads, _p(out)))
        return _rows(out)

    def _evaluate_commit(self, commitment, call):
        """The streaming evaluators' commitments: `call(macs, digests)` runs the C entry point with the arrays this commitment asks for
        (None for the other); returns the MACs, the 32-byte BLAKE3 digests (computed on the device), or (MACs, digests) for "both"."""
        macs = np.zeros((self.n, 16), np.uint8) if commitment != "blake3" else None
        dig = np.zeros((self.n, 32), np.uint8) if commitment != "cbcmac" else None
        call(macs, dig)
        m, d = _rows(macs), _rows(dig)
        return (m, d) if commitment == "both" else m if d is None else d

    def _pack_mac_expected(self, expected):
        """The CBC-MAC commitments a checkpoint-verified pass trusts, one of 16 bytes per instance -> one uint8 array; None stays None."""
        if expected is None:
            return None
        exp = np.frombuffer(b"".join(bytes(e) for e in expected), np.uint8)
        if len(expected) != self.n or exp.size != 16 * self.n:
            raise ValueError("expected: one 16-byte commitment per instance")
        return exp

    def _evaluate_mac_files(self, gate_id_base, first_call, n_calls, restartable, directory, idx_p, first_index, checkpoint_dir, expected):
        """gsv_session_evaluate_streaming_mac_calls: gc files verified against the checkpoint files of checkpoint_dir while they are
        evaluated.  Returns the verified CBC-MACs from the slice that ends the pass, None before."""
        exp = self._pack_mac_expected(expected)
        out = np.zeros((self.n, 16), np.uint8)
        with _gc_paused():
            rc = lib().gsv_session_evaluate_streaming_mac_calls(self.h, gate_id_base, first_call, n_calls, int(bool(restartable)), os.fsencode(directory), idx_p, first_index,
                                                                os.fsencode(checkpoint_dir), _p(exp), _p(out))
        _chk_mismatch(rc, self.mismatch_info, self._resume_call)
        return _rows(out) if self._ends_pass(first_call, n_calls) else None

    def _evaluate_mac_source(self, gate_id_base, first_call, n_calls, restartable, source, checkpoints, expected):
        """gsv_session_evaluate_streaming_source_mac_calls: `checkpoints` holds one bytes object per instance, byte for byte a gc_<i>.mck."""
        cks = [np.frombuffer(bytes(c), np.uint8) for c in checkpoints]
        if len(cks) != self.n:
            raise ValueError("checkpoints: one per instance")
        exp = self._pack_mac_expected(expected)
        nothing = np.zeros(1, np.uint8)
        ck_p = (C.POINTER(C.c_uint8) * self.n)(*[_p(c) if c.size else _p(nothing) for c in cks])
        ck_n = (C.c_uint64 * self.n)(*[c.size for c in cks])
        cb, failure = self._source_callback(source)
        out = np.zeros((self.n, 16), np.uint8)
        with _gc_paused():
            rc = lib().gsv_session_evaluate_streaming_source_mac_calls(self.h, gate_id_base, first_call, n_calls, int(bool(restartable)), cb, None, ck_p, ck_n, _p(exp), _p(out))
        if failure:
            raise failure[0]
        _chk_mismatch(rc, self.mismatch_info, self._resume_call)
        return _rows(out) if self._ends_pass(first_call, n_calls) else None

    def _evaluate_files(self, commitment, gate_id_base, directory, idx_p, first_index, outboard_dir, expected, checkpoint_dir=None):
        """evaluate_streaming / evaluate_streaming_indexed (idx_p: the index list, or None for first_index + i); with outboard_dir or
        expected gsv_session_evaluate_streaming_verified, where GSV_ERR_MISMATCH raises CiphertextMismatch with the place; with
        checkpoint_dir gsv_session_evaluate_streaming_mac_calls over the whole pass."""
        if checkpoint_dir is not None:
            if commitment != "cbcmac" or outboard_dir is not None:
                raise ValueError("checkpoint_dir needs commitment='cbcmac' and no outboard_dir: the files hold the states of the CBC-MAC")
            return self._evaluate_mac_files(gate_id_base, 0, 0, False, directory, idx_p, first_index, checkpoint_dir, expected)
        verified = outboard_dir is not None or expected is not None
        if verified:
            if commitment == "cbcmac":
                raise ValueError("outboard_dir / expected need commitment='blake3' or 'both'")
            if outboard_dir is None or expected is None:
                raise ValueError("verified streaming takes outboard_dir and expected together")
            exp_a, exp_len = _pack_expected(expected, self.n)

        def call(macs, dig):
            with _gc_paused():
                if verified:
                    rc = lib().gsv_session_evaluate_streaming_verified(self.h, gate_id_base, os.fsencode(directory), idx_p, first_index, os.fsencode(outboard_dir), _p(exp_a), exp_len, _p(macs), _p(dig))
                elif dig is not None:
                    rc = lib().gsv_session_evaluate_streaming_commit(self.h, gate_id_base, directory.encode(), idx_p, first_index, _p(macs), _p(dig))
                elif idx_p is not None:
                    rc = lib().gsv_session_evaluate_streaming_indexed(self.h, gate_id_base, directory.encode(), idx_p, _p(macs))
                else:
                    rc = lib().gsv_session_evaluate_streaming(self.h, gate_id_base, directory.encode(), first_index, _p(macs))
            _chk_mismatch(rc, self.mismatch_info)

        return self._evaluate_commit(commitment, call)

    def mismatch_info(self):
        """(instance, group, first_record) of the mismatch the last verified pass ended with; group and first_record are None when
        the outboard or the last chunk did not match the commitment before the pass."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _chk(lib().gsv_session_mismatch_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        unknown = (1 << 64) - 1
        return int(a.value), None if b.value == unknown else int(b.value), None if c.value == unknown else int(c.value)

    def evaluate_streaming_indexed(self, directory, indexes, gate_id_base=0, commitment="cbcmac", outboard_dir=None, expected=None, checkpoint_dir=None):
        """Evaluate with instance i reading gc_<indexes[i]>.bin: the finalized instances of a cut-and-choose run in one session.
        commitment, outboard_dir, checkpoint_dir and expected as for evaluate_streaming."""
        _check_commitment(commitment, False)
        idx = np.ascontiguousarray(indexes, np.uint64)
        assert idx.size == self.n
        idx_p = idx.ctypes.data_as(C.POINTER(C.c_uint64))
        return self._evaluate_files(commitment, gate_id_base, directory, idx_p, 0, outboard_dir, expected, checkpoint_dir)

    def evaluate_from_source(self, source, gate_id_base=0, commitment="cbcmac", outboards=None, expected=None, last_chunks=None, checkpoints=None):
        """Evaluate with the ciphertexts pulled from `source(instance, first_record, n) -> [n,16] uint8` (None / short = exhausted):
        the generic CiphertextSource (ciphertext_source.rs:14-34).  Returns the CBC-MACs of what was read; commitment as for
        evaluate_streaming.
        Verified (gsv_session_evaluate_streaming_source_verified, with "blake3" / "both"): `outboards` (one bytes object per instance)
        and `expected` (the commitments, 32 bytes each or the first 16) together.  With `last_chunks` (the streams' last chunks as
        bytes, as garble_to_sink returns them) the outboards are checked against the commitments before `source` is called at all;
        without, they are checked for form only and the commitments are compared at the end of the pass — until then the outboards
        are unauthenticated.  Either way the pass stops at the first group that differs from its outboard: CiphertextMismatch names
        (instance, group, first_record), and read_outputs then fails.
        Verified against CBC-MAC checkpoints (gsv_session_evaluate_streaming_source_mac_calls, with "cbcmac"): `checkpoints`, one bytes
        object per instance (byte for byte a gc_<i>.mck), with an optional `expected` of 16-byte commitments; malformed checkpoints are
        refused before `source` is called at all.  Returns the verified CBC-MACs."""
        _check_commitment(commitment, False)
        if checkpoints is not None:
            if commitment != "cbcmac" or outboards is not None or last_chunks is not None:
                raise ValueError("checkpoints need commitment='cbcmac' and neither outboards nor last_chunks: they hold the states of the CBC-MAC")
            return self._evaluate_mac_source(gate_id_base, 0, 0, False, source, checkpoints, expected)
        ob_p, ob_n, last_a, exp_a, exp_len = self._pack_outboards(commitment, outboards, expected, last_chunks)
        cb, failure = self._source_callback(source)

        def call(macs, dig):
            with _gc_paused():
                if ob_p is not None:
                    rc = lib().gsv_session_evaluate_streaming_source_verified(self.h, gate_id_base, cb, None, ob_p, ob_n, _p(last_a), _p(exp_a), exp_len, _p(macs), _p(dig))
                elif dig is None:
                    rc = lib().gsv_session_evaluate_streaming_source(self.h, gate_id_base, cb, None, _p(macs))
                else:
                    rc = lib().gsv_session_evaluate_streaming_source_commit(self.h, gate_id_base, cb, None, _p(macs), _p(dig))
            if failure:
                raise failure[0]
            _chk_mismatch(rc, self.mismatch_info)

        return self._evaluate_commit(commitment, call)

    def _pack_outboards(self, commitment, outboards, expected, last_chunks):
        """The arguments of a verified evaluation from a source -> (outboard pointers, their lengths, last chunks [n,1024] or None,
        commitments, bytes per commitment); five times None when none of them is given (unverified)."""
        if outboards is None and expected is None and last_chunks is None:
            return None, None, None, None, 0
        if commitment == "cbcmac":
            raise ValueError("outboards / expected / last_chunks need commitment='blake3' or 'both'")
        if outboards is None or expected is None:
            raise ValueError("verified evaluation takes outboards and expected together")
        obs = [np.frombuffer(bytes(o), np.uint8) for o in outboards]
        if len(obs) != self.n:
            raise ValueError("outboards: one per instance")
        exp_a, exp_len = _pack_expected(expected, self.n)
        last_a = None
        if last_chunks is not None:
            lc = [bytes(x) for x in last_chunks]
            if len(lc) != self.n or any(len(x) > 1024 for x in lc):
                raise ValueError("last_chunks: one per instance, at most 1024 bytes each")
            last_a = np.zeros((self.n, 1024), np.uint8)
            for i, x in enumerate(lc):
                last_a[i, :len(x)] = np.frombuffer(x, np.uint8)
        nothing = np.zeros(1, np.uint8)
        ob_p = (C.POINTER(C.c_uint8) * self.n)(*[_p(o) if o.size else _p(nothing) for o in obs])
        ob_p._keep = (obs, nothing)  # the arrays the pointers point into
        ob_n = (C.c_uint64 * self.n)(*[o.size for o in obs])
        return ob_p, ob_n, last_a, exp_a, exp_len

    @staticmethod
    def _source_callback(source):
        """`source(instance, first_record, n) -> [n,16] uint8` as a gsv_ct_source_fn, and the list an exception it raises is kept in."""
        failure = []

        def _cb(_user, inst, first, ptr, n):
            try:
                a = source(int(inst), int(first), int(n))
                if a is None:
                    return 1
                a = _u8(a).reshape(-1)
                if a.size != int(n) * 16:
                    return 1
                C.memmove(ptr, a.ctypes.data, a.size)
                return 0
            except BaseException as e:  # noqa: BLE001
                failure.append(e)
                return 2

        return CT_SOURCE_FN(_cb), failure

    def evaluate_calls(self, first_call, n_calls, directory=None, indexes=None, first_index=0, source=None, gate_id_base=0, commitment="cbcmac", outboard_dir=None, outboards=None,
                       expected=None, last_chunks=None, restartable=False, checkpoint_dir=None, checkpoints=None):
        """Plan sessions: evaluate calls [first_call, first_call + n_calls) only, whole windows of the schedule (windows()), from gc files
        (`directory`, with `indexes` or `first_index`) or from `source` — evaluate_streaming / evaluate_streaming_indexed /
        evaluate_from_source in slices (gsv_session_evaluate_streaming_calls / _source_calls).  The wire file, gate ids, the stream
        position, the MAC states, the BLAKE3 state and the outboard comparison continue from the previous evaluate slice; first_call == 0
        starts a new pass, every slice asks for the same commitment and verification as the first, and read_outputs succeeds after the
        slice that ends the pass.  Returns what the whole-pass method returns, the MACs being the states after the slice and the BLAKE3
        digests None until the slice that ends the pass.  Verified: outboard_dir + expected (files), or outboards + expected
        [+ last_chunks] (source), in every slice.
        restartable=True keeps a restart point in front of the slice: when the slice fails with a CiphertextMismatch that has a place
        or because a file or the source ran dry, the session is rolled back — resume_info() says to which call and from which record
        the ciphertexts are needed again (CiphertextMismatch.resume_call is that call) — and the repaired slice is simply repeated.
        Verified against CBC-MAC checkpoints, with commitment="cbcmac": checkpoint_dir (files) or checkpoints (source; one bytes object
        per instance), with an optional `expected` of 16-byte commitments, in every slice.  Then the verified CBC-MACs come back from
        the slice that ends the pass, None before."""
        _check_commitment(commitment, False)
        if (directory is None) == (source is None):
            raise ValueError("a directory of gc files or a source")
        if first_call == 0 and n_calls == 0:
            raise ValueError("an empty slice")  # (0, 0 means the whole pass to the C entry points)
        if checkpoint_dir is not None or checkpoints is not None:
            if commitment != "cbcmac" or outboard_dir is not None or outboards is not None or last_chunks is not None:
                raise ValueError("checkpoint_dir / checkpoints need commitment='cbcmac' and no outboards: they hold the states of the CBC-MAC")
            if (checkpoint_dir is not None) != (directory is not None) or (checkpoints is not None) != (source is not None):
                raise ValueError("checkpoint_dir belongs to gc files, checkpoints to a source")
            if source is not None:
                if indexes is not None:
                    raise ValueError("indexes belong to gc files")
                return self._evaluate_mac_source(gate_id_base, first_call, n_calls, restartable, source, checkpoints, expected)
            idx_p = None
            if indexes is not None:
                idx = np.ascontiguousarray(indexes, np.uint64)
                assert idx.size == self.n
                idx_p = idx.ctypes.data_as(C.POINTER(C.c_uint64))
            return self._evaluate_mac_files(gate_id_base, first_call, n_calls, restartable, directory, idx_p, first_index, checkpoint_dir, expected)
        macs = np.zeros((self.n, 16), np.uint8) if commitment != "blake3" else None
        dig = np.zeros((self.n, 32), np.uint8) if commitment != "cbcmac" else None
        failure = []
        if source is not None:
            if outboard_dir is not None or indexes is not None:
                raise ValueError("outboard_dir / indexes belong to gc files: a source takes outboards")
            ob_p, ob_n, last_a, exp_a, exp_len = self._pack_outboards(commitment, outboards, expected, last_chunks)
            cb, failure = self._source_callback(source)
            with _gc_paused():
                rc = lib().gsv_session_evaluate_streaming_source_calls(self.h, gate_id_base, first_call, n_calls, int(bool(restartable)), cb, None, ob_p, ob_n, _p(last_a), _p(exp_a), exp_len,
                                                                       _p(macs), _p(dig))
        else:
            if outboards is not None or last_chunks is not None:
                raise ValueError("outboards / last_chunks belong to a source: gc files take outboard_dir")
            exp_a, exp_len = None, 0
            if outboard_dir is not None or expected is not None:
                if commitment == "cbcmac":
                    raise ValueError("outboard_dir / expected need commitment='blake3' or 'both'")
                if outboard_dir is None or expected is None:
                    raise ValueError("verified streaming takes outboard_dir and expected together")
                exp_a, exp_len = _pack_expected(expected, self.n)
            idx_p = None
            if indexes is not None:
                idx = np.ascontiguousarray(indexes, np.uint64)
                assert idx.size == self.n
                idx_p = idx.ctypes.data_as(C.POINTER(C.c_uint64))
            with _gc_paused():
                rc = lib().gsv_session_evaluate_streaming_calls(self.h, gate_id_base, first_call, n_calls, int(bool(restartable)), os.fsencode(directory), idx_p, first_index,
                                                                os.fsencode(outboard_dir) if outboard_dir is not None else None, _p(exp_a), exp_len, _p(macs), _p(dig))
        if failure:
            raise failure[0]
        _chk_mismatch(rc, self.mismatch_info, self._resume_call)
        m, d = _rows(macs), _rows(dig) if self._ends_pass(first_call, n_calls) else None  # (else the engine leaves `dig` alone)
        return (m, d) if commitment == "both" else m if commitment == "cbcmac" else d

    def resume_info(self):
        """(next_call, next_record) after a restartable evaluate_calls slice failed and the session was rolled back: the call to repeat
        from and the first record of every instance's stream that is needed again.  (0, 0): no restart point reaches back far enough,
        the pass starts again from set_evaluate_inputs.  Raises GsvError when nothing can be resumed."""
        a, b = C.c_uint64(), C.c_uint64()
        _chk(lib().gsv_session_evaluate_resume_info(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def _resume_call(self):
        try:
            return self.resume_info()[0]
        except GsvError:
            return None

    def schedule_info(self):
        """Plan sessions: the call-level schedule this session executes (windows, batches of calls side by side, wire-file layout,
        depth in device steps)."""
        i = _PlanScheduleInfo()
        _chk(lib().gsv_session_plan_schedule_info(self.h, C.byref(i)))
        n = C.c_uint64()
        _chk(lib().gsv_session_windows_launched(self.h, C.byref(n)))
        return dict({k: int(getattr(i, k)) for k in _SCHED_FIELDS}, windows_launched=int(n.value))  # (windows the session's last pass launched)

    def fallback_count(self):
        """How often this plan session has fallen back to the safe schedule (one call per launch) after a dependency wait gave up."""
        n = C.c_uint64()
        _chk(lib().gsv_session_fallback_count(self.h, C.byref(n)))
        return int(n.value)

    def windows(self):
        """[(first_call, n_calls, max_width)] of the schedule: slices handed to garble_calls start and end on these boundaries."""
        out = []
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        for w in range(self.schedule_info()["n_windows"]):
            _chk(lib().gsv_session_plan_window(self.h, w, C.byref(a), C.byref(b), C.byref(c)))
            out.append((a.value, b.value, c.value))
        return out

    def set_drain_instances(self, n):
        """The streaming calls garble every instance but only the first `n` instances' ciphertext streams leave the device (0 = all):
        their hashes / gc files / sink runs are what the calls then return (a checked SAMPLE of a full-GPU batch)."""
        _chk(lib().gsv_session_set_drain_instances(self.h, int(n)))
        self.n_drain = int(n) or self.n

    def set_unchecked_slices(self, on=True):
        """Timing harnesses only: allow garble_calls slices that do not continue the previous one (stale wires, meaningless MACs)."""
        _chk(lib().gsv_session_set_unchecked_slices(self.h, int(bool(on))))

    def evaluate_streaming(self, directory, first_index=0, gate_id_base=0, commitment="cbcmac", outboard_dir=None, expected=None, checkpoint_dir=None):
        """Evaluate with the ciphertexts read from gc_<first_index+i>.bin segment by segment; returns the files' CBC-MACs.
        commitment="blake3": the files' 32-byte BLAKE3 digests instead, computed on the device from the uploaded segments (no MAC
        worker runs); "both": (CBC-MACs, BLAKE3 digests).  Comparing them with the garbler's commitments is the caller's part —
        unless outboard_dir and expected are given (verified streaming, with "blake3" / "both"): `expected` holds the commitment of
        every instance (32 bytes, or the first 16), the outboards gc_<index>.b3o in outboard_dir are checked against them before
        anything is uploaded, and the pass stops at the first group of 2^k chunks that differs from its outboard: CiphertextMismatch
        names (instance, group), and read_outputs then fails.
        checkpoint_dir (with "cbcmac"; gsv_session_evaluate_streaming_mac_calls): the files are verified against the CBC-MAC checkpoint
        files gc_<index>.mck of that directory on the device while they are evaluated, and no host MAC worker runs.  With `expected`
        (16-byte commitments) the files' last states are compared before anything is uploaded.  Returns the verified CBC-MACs; a group
        of 2^k records that does not hold raises CiphertextMismatch(instance, group, first_record) at the launch that would read it."""
        _check_commitment(commitment, False)
        return self._evaluate_files(commitment, gate_id_base, directory, None, first_index, outboard_dir, expected, checkpoint_dir)

    def set_evaluate_inputs(self, const_active, input_active, input_bits):
        c = _u8(const_active, (self.n, 32))
        a = _u8(input_active, (self.n, self.n_in * 16))
        b = _u8(input_bits, (self.n, self.n_in))
        _chk(lib().gsv_session_set_evaluate_inputs(self.h, _p(c), _p(a) if self.n_in else None, _p(b) if self.n_in else None))

    def upload_ciphertexts(self, instance, cts):
        a = _u8(cts).reshape(-1)
        _chk(lib().gsv_session_upload_ciphertexts(self.h, instance, _p(a) if a.size else None, a.size // 16))

    def evaluate(self, gate_id_base=0):
        _chk(lib().gsv_session_evaluate(self.h, gate_id_base))

    def set_hasher(self, kind):
        """'aes' (AesNiHasher, default) or 'blake3' (Blake3Hasher)."""
        _chk(lib().gsv_session_set_hasher(self.h, {"aes": 0, "blake3": 1}[kind]))

    def sync(self):
        _chk(lib().gsv_session_sync(self.h))

    @property
    def instances_per_workgroup(self):
        n = C.c_int()
        _chk(lib().gsv_session_instances_per_workgroup(self.h, C.byref(n)))
        return n.value

    def enable_step_clock(self):
        """Diagnostics: instance 0 stamps a 100 MHz clock at every step of a launch's last replay."""
        _chk(lib().gsv_session_enable_step_clock(self.h))

    def read_step_clock(self):
        out = np.zeros(self.program.info["n_steps"] + 1, np.uint64)
        _chk(lib().gsv_session_read_step_clock(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def last_kernel_ms(self):
        ms = C.c_double()
        _chk(lib().gsv_session_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def read_outputs(self, with_bits=False):
        lab = np.zeros((self.n, self.n_out, 16), np.uint8)
        bits = np.zeros((self.n, self.n_out), np.uint8) if with_bits else None
        _chk(lib().gsv_session_read_outputs(self.h, _p(lab), _p(bits)))
        return (lab, bits) if with_bits else lab

    def read_ciphertexts(self, instance, first=0, n=None):
        if n is None:
            n = self.ct_cap * self.program.info["n_ciphertexts"] - first
        out = np.zeros((n, 16), np.uint8)
        _chk(lib().gsv_session_read_ciphertexts(self.h, instance, first, n, _p(out) if n else None))
        return out

    def ciphertext_hash(self, instance):
        h = np.zeros(16, np.uint8)
        _chk(lib().gsv_session_ciphertext_hash(self.h, instance, _p(h)))
        return h.tobytes()

    def ciphertext_cbcmac_check(self, checkpoint_dir, first_index=0, indexes=None, expected=None):
        """Verify every instance's resident stream (after garble(), or after upload_ciphertexts of every instance) against the CBC-MAC
        checkpoint files <checkpoint_dir>/gc_<index>.mck (index = indexes[i], or first_index + i) on the device, where it lies.
        expected: one trusted 16-byte commitment per instance, compared with the files' last states first.  Returns the verified
        CBC-MACs — what ciphertext_hash(i) folds on the host —; a stream that differs raises CiphertextMismatch(instance, group,
        first_record).  Sessions that retain the whole stream only."""
        idx_p = None
        if indexes is not None:
            idx = np.ascontiguousarray(indexes, np.uint64)
            assert idx.size == self.n
            idx_p = idx.ctypes.data_as(C.POINTER(C.c_uint64))
        exp = self._pack_mac_expected(expected)
        out = np.zeros((self.n, 16), np.uint8)
        rc = lib().gsv_session_ciphertext_cbcmac_check(self.h, os.fsencode(checkpoint_dir), idx_p, first_index, _p(exp), _p(out))
        _chk_mismatch(rc, self.mismatch_info)
        return _rows(out)

    def ciphertext_blake3(self, with_seconds=False):
        """BLAKE3 of every instance's resident stream in gate order (after garble(), or after upload_ciphertexts of every instance),
        hashed on the device where it lies: a list of 32-byte digests.  Sessions that retain the whole stream only.
        with_seconds=True: (digests, device seconds from the first hash kernel to the last)."""
        out = np.zeros((self.n, 32), np.uint8)
        _chk(lib().gsv_session_ciphertext_blake3(self.h, _p(out)))
        digests = [bytes(out[i]) for i in range(self.n)]
        if not with_seconds:
            return digests
        s = C.c_double()
        _chk(lib().gsv_engine_blake3_streams_seconds(self.engine.h, C.byref(s)))
        return digests, s.value

    def close(self):
        if getattr(self, "h", None) is not None and _lib is not None and self.h and not sys.is_finalizing():
            _lib.gsv_session_destroy(self.h)
        self.h = None

    __del__ = close


class StreamingResult:
    """Fields of the reference's StreamingResult that exist for this path (src/circuit/mod.rs:81-107)."""
    pass


class CircuitBuilder:
    """Host-side mirror of the reference's CircuitBuilder entry points for the garble/evaluate path."""

    @staticmethod
    def streaming_garbling(circuit, seeds, engine=None, program=None, replays=1, keep_ciphertexts=True, hasher="aes"):
        """Garble `circuit` once per seed (one instance per seed, all on `engine`'s GPU).
        Mirrors CircuitBuilder::streaming_garbling(inputs, cap, seed, AESAccumulatingHash, f) per instance
        (src/circuit/mod.rs:185-203): labels from the seed's ChaCha stream, ciphertext hash = CBC-MAC."""
        seeds = [seeds] if np.isscalar(seeds) else list(seeds)
        engine = engine or Engine(0)
        program = program or Program.from_circuit(circuit)
        n_in = program.info["n_inputs"]
        B = len(seeds)
        delta = np.zeros((B, 16), np.uint8)
        consts = np.zeros((B, 2, 16), np.uint8)
        inputs = np.zeros((B, n_in, 16), np.uint8)
        for i, s in enumerate(seeds):
            delta[i], consts[i, 0], consts[i, 1], inputs[i] = labels_from_seed(s, n_in)
        sess = Session(engine, program, B, replays)
        sess.set_hasher(hasher)
        sess.set_garble_inputs(delta, consts, inputs)
        sess.garble(0)
        sess.sync()
        r = StreamingResult()
        r.session, r.program = sess, program
        r.delta, r.false_label0, r.true_label0, r.input_label0 = delta, consts[:, 0], consts[:, 1], inputs
        r.output_label0 = sess.read_outputs()
        r.kernel_ms = sess.last_kernel_ms()
        r.n_ciphertexts = program.info["n_ciphertexts"] * replays
        r.gate_count = [g * replays for g in program.info["gate_count"]]
        r.ciphertext_hash = [sess.ciphertext_hash(i) for i in range(B)]
        r.ciphertexts = [sess.read_ciphertexts(i) for i in range(B)] if keep_ciphertexts else None
        return r

    @staticmethod
    def streaming_evaluation(circuit, true_active, false_active, input_active, input_bits, ciphertexts, engine=None, program=None, replays=1,
                             hasher="aes"):
        """Evaluate instances from their ciphertext streams (src/circuit/mod.rs:225-249).  Arrays carry a
        leading instance dimension; `ciphertexts` is a list of [n,16] uint8 arrays (gc_{i}.bin bytes)."""
        engine = engine or Engine(0)
        program = program or Program.from_circuit(circuit)
        ta, fa = _u8(true_active).reshape(-1, 16), _u8(false_active).reshape(-1, 16)
        B = ta.shape[0]
        consts = np.stack([fa, ta], axis=1)
        sess = Session(engine, program, B, replays)
        sess.set_hasher(hasher)
        sess.set_evaluate_inputs(consts, input_active, input_bits)
        for i in range(B):
            sess.upload_ciphertexts(i, ciphertexts[i])
        sess.evaluate(0)
        sess.sync()
        r = StreamingResult()
        r.session, r.program = sess, program
        r.output_active, r.output_bits = sess.read_outputs(with_bits=True)
        r.kernel_ms = sess.last_kernel_ms()
        r.ciphertext_hash = [sess.ciphertext_hash(i) for i in range(B)]
        return r


# ---- ciphertext files: the reference's gc_{index}.bin format ---------------------------------------------------
# src/cut_and_choose/ciphertext_repository.rs:29,94-106,157 writes, and FileSource (src/circuit/ciphertext_source.rs:36-107)
# reads, a bare concatenation of 16-byte S::to_bytes() records in gate order, no header.  FileSource CBC-MACs what it
# reads, so evaluation re-derives the commitment; read_gc_file returns the same pair.
def gc_file_name(index):
    return "gc_%d.bin" % index


def write_gc_file(path, ciphertexts):
    """Writes a ciphertext stream ([n,16] uint8) as gc_{i}.bin bytes and returns its AESAccumulatingHash."""
    a = _u8(ciphertexts).reshape(-1, 16)
    with open(path, "wb") as f:
        f.write(a.tobytes())
    return cbcmac(a)


def read_gc_file(path):
    """Returns ([n,16] uint8 ciphertexts, AESAccumulatingHash) of a gc_{i}.bin file; rejects a trailing partial record."""
    data = np.fromfile(path, dtype=np.uint8)
    if data.size % 16:
        raise GsvError("%s: length %d is not a multiple of 16-byte ciphertext records" % (path, data.size))
    cts = data.reshape(-1, 16)
    return cts, cbcmac(cts)
