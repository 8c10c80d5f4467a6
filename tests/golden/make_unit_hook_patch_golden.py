"""Writes tests/golden/unit_hook_patch_golden.json: for every hunk of bindings/rust/streaming_mode_unit_hook.patch the sha256 of the lines
of the reference's file that the hunk replaces (old_start .. old_start + old_len - 1), and each file's line count.  Hashes and numbers
only: tests/test_rust_shim.py checks with them that the patch applies to the reference without the reference at hand.

  python tests/golden/make_unit_hook_patch_golden.py <checkout of BitVM/garbled-snark-verifier v0.4.0>"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_rust_shim import patch_hunks  # noqa: E402

ref = sys.argv[1]
files = {}
for f, hunks in patch_hunks().items():
    lines = open(os.path.join(ref, f)).read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    files[f] = {"n_lines": len(lines), "hunks": [{"old_start": s, "old_len": n, "sha256": hashlib.sha256("\n".join(lines[s - 1:s - 1 + n]).encode()).hexdigest()} for s, n, _, _ in hunks]}
json.dump({"patch": "bindings/rust/streaming_mode_unit_hook.patch", "reference": "BitVM/garbled-snark-verifier v0.4.0", "files": files}, open(os.path.join(HERE, "unit_hook_patch_golden.json"), "w"), indent=1)
