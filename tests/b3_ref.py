"""BLAKE3 (plain hash mode, 32-byte output) in pure Python, written from the specification's definition of the tree: the input is split
recursively — the left subtree takes the largest power-of-two number of chunks that leaves at least one byte for the right one — with no
incremental state, no chaining-value stack and no lazy merging.  It shares nothing with the engine's host_crypto.hpp; the engine's host
hasher and its device kernels are tested against it.

blake3(data)                  the digest
chunk_cv(chunk, counter)      chaining value of one chunk (<= 1024 bytes) as a NON-root node
subtree_cv(data, chunk0)      chaining value of a whole subtree as a NON-root node: data = a power-of-two number of full chunks, the
                              first of which is chunk number chunk0 of its stream
"""
import struct

IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
CHUNK_START, CHUNK_END, PARENT, ROOT = 1, 2, 4, 8
PERMUTATION = (2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)
M32 = 0xFFFFFFFF


def _g(v, a, b, c, d, x, y):
    v[a] = (v[a] + v[b] + x) & M32
    t = v[d] ^ v[a]
    v[d] = (t >> 16) | (t << 16) & M32
    v[c] = (v[c] + v[d]) & M32
    t = v[b] ^ v[c]
    v[b] = (t >> 12) | (t << 20) & M32
    v[a] = (v[a] + v[b] + y) & M32
    t = v[d] ^ v[a]
    v[d] = (t >> 8) | (t << 24) & M32
    v[c] = (v[c] + v[d]) & M32
    t = v[b] ^ v[c]
    v[b] = (t >> 7) | (t << 25) & M32


def compress(cv, block, counter, block_len, flags):
    """The eight-word chaining value (truncated output) of one compression; block: 64 bytes."""
    m = list(struct.unpack("<16I", block))
    v = list(cv) + list(IV[:4]) + [counter & M32, (counter >> 32) & M32, block_len, flags]
    for r in range(7):
        _g(v, 0, 4, 8, 12, m[0], m[1])
        _g(v, 1, 5, 9, 13, m[2], m[3])
        _g(v, 2, 6, 10, 14, m[4], m[5])
        _g(v, 3, 7, 11, 15, m[6], m[7])
        _g(v, 0, 5, 10, 15, m[8], m[9])
        _g(v, 1, 6, 11, 12, m[10], m[11])
        _g(v, 2, 7, 8, 13, m[12], m[13])
        _g(v, 3, 4, 9, 14, m[14], m[15])
        m = [m[i] for i in PERMUTATION]
    return tuple(v[i] ^ v[i + 8] for i in range(8))


def _chunk(chunk, counter, root):
    assert len(chunk) <= 1024
    blocks = [chunk[i:i + 64] for i in range(0, len(chunk), 64)] or [b""]
    cv = IV
    for i, b in enumerate(blocks):
        flags = (CHUNK_START if i == 0 else 0) | (CHUNK_END if i == len(blocks) - 1 else 0)
        if root and i == len(blocks) - 1:
            flags |= ROOT
        cv = compress(cv, b.ljust(64, b"\0"), counter, len(b), flags)
    return cv


def _node(data, chunk0, root):
    if len(data) <= 1024:
        return _chunk(data, chunk0, root)
    left_chunks = 1
    while left_chunks * 2 * 1024 < len(data):
        left_chunks *= 2
    left = _node(data[:left_chunks * 1024], chunk0, False)
    right = _node(data[left_chunks * 1024:], chunk0 + left_chunks, False)
    return compress(IV, struct.pack("<16I", *(left + right)), 0, 64, PARENT | (ROOT if root else 0))


def blake3(data):
    return struct.pack("<8I", *_node(bytes(data), 0, True))


def chunk_cv(chunk, counter):
    return struct.pack("<8I", *_chunk(bytes(chunk), counter, False))


def subtree_cv(data, chunk0):
    data = bytes(data)
    n = len(data) // 1024
    assert n * 1024 == len(data) and n >= 1 and n & (n - 1) == 0 and chunk0 % n == 0
    return struct.pack("<8I", *_node(data, chunk0, False))
