"""Writes tests/golden/blake3_known_answers.json: BLAKE3 digests (plain hash mode, 32 bytes) of bytes(i % 251 for i in range(n)) — the
input rule of the official test_vectors.json — for the lengths tests/test_blake3_commit.py uses.  The digests are RECORDED RESULTS of an
implementation that is neither the engine's nor tests/b3_ref.py: LLVM's copy of the official C code, which the ROCm toolchain's
libclang-cpp.so exports as llvm_blake3_hasher_{init,update,finalize} (called through ctypes with a 4 KiB state buffer).

    python tests/golden/make_blake3_golden.py
"""
import ctypes as C
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5120, 6144, 7168, 8192, 8193, 16384, 31744, 102400]


def llvm_blake3():
    """hash(bytes) -> 32 bytes through LLVM's BLAKE3, or None where the library (or its symbols) cannot be loaded."""
    path = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "lib", "libclang-cpp.so")
    try:
        L = C.CDLL(path)
        init, update, final = L.llvm_blake3_hasher_init, L.llvm_blake3_hasher_update, L.llvm_blake3_hasher_finalize
    except (OSError, AttributeError):
        return None
    init.argtypes = [C.c_void_p]
    update.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    final.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    for f in (init, update, final):
        f.restype = None

    def h(data):
        state = C.create_string_buffer(4096)
        out = C.create_string_buffer(32)
        init(state)
        update(state, bytes(data), len(data))
        final(state, out, 32)
        return out.raw
    return h


def pattern(n):
    return bytes(i % 251 for i in range(n))


if __name__ == "__main__":
    h = llvm_blake3()
    assert h is not None, "LLVM's BLAKE3 is not available here"
    doc = {"source": "llvm_blake3_hasher_* of the ROCm toolchain's libclang-cpp.so (LLVM's copy of the official BLAKE3 C code)",
           "input": "bytes(i % 251 for i in range(n))", "digests": {str(n): h(pattern(n)).hex() for n in LENGTHS}}
    with open(os.path.join(HERE, "blake3_known_answers.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
