"""Cut-and-choose instance sharding across GPUs (one process per GPU, torch.distributed).

The path partitions into independent units: instance i — own seed, own delta, labels and
ciphertext stream — goes to rank i mod world (reference: `seeds.par_iter()` over a pinned rayon pool,
src/cut_and_choose/garbler.rs:206-234).  Nothing is exchanged while garbling; the single collective is an
all-gather of fixed-size commit records at the end (GarbledInstanceCommit, garbler.rs:61-99), which is
latency-bound (tens of KB per instance) so ring-vs-direct over xGMI is irrelevant.

Commit record (bytes), one per instance — the fields of GarbledInstanceCommit in declaration order behind the
instance index:
    index u64 LE | ciphertext_commit 16 | input_labels_commit: n_in x {commit(label0), commit(label1)} |
    per output wire {commit(label1), commit(label0)} (output_label1_commit, output_label0_commit) |
    true_constant_commit = commit(true.label1) | false_constant_commit = commit(false.label0)
with commit = AesLabelCommitHasher = AES_K(label) (cut_and_choose/mod.rs:41-48).  Only the constants' SEMANTIC labels are
committed (true.select(true), false.select(false), garbler.rs:94-97): AES_K has a public key and is invertible, so publishing
both labels of one wire would reveal delta.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import lib as _lib  # noqa: F401  (host AES for label commits lives behind the C ABI)


def u64_stream_from_labels(labels, total):
    """The first `total` values of `rng.next_u64()` given the first ceil(total / 2) values of `rng.gen::<u128>()` as 16-byte big-endian
    labels (S::to_bytes): rand 0.8.5 draws a u128 as next_u64() | next_u64() << 64 — the first call is the LOW half."""
    out = []
    for lab in np.asarray(labels, np.uint8).reshape(-1, 16):
        b = bytes(lab)
        out += [int.from_bytes(b[8:16], "big"), int.from_bytes(b[0:8], "big")]
    return np.array(out[:total], dtype=np.uint64)


def instance_seeds(master_seed, total, rng="chacha"):
    """`total` u64 seeds drawn up front by the garbler, as the reference draws them: `rng.gen::<u64>()` per instance on the caller's RNG
    (cut_and_choose/garbler.rs:201-203), which the reference's own test seeds as `ChaCha20Rng::seed_from_u64(1234)`
    (cut_and_choose/tests.rs:102).  The ChaCha stream is the product's own (gsv_labels_from_seed: the generator behind
    GarbleMode::new); tests compare it with the oracle's independent restatement.  rng="numpy" keeps the pre-round-5 PCG64 draw for
    callers that stored such seeds."""
    if rng == "numpy":
        g = np.random.Generator(np.random.PCG64(master_seed))
        return g.integers(0, 2**63, size=total, dtype=np.uint64)
    if rng != "chacha":
        raise ValueError("rng must be \"chacha\" or \"numpy\"")
    from . import labels_from_seed
    n128 = (int(total) + 1) // 2
    d, f, t, inp = labels_from_seed(int(master_seed), max(0, n128 - 3))
    labels = np.concatenate([np.stack([d, f, t]), np.asarray(inp, np.uint8).reshape(-1, 16)])[:n128]
    return u64_stream_from_labels(labels, int(total))


def shard_instances(total, rank, world):
    return list(range(rank, total, world))


def record_len(n_outputs, n_inputs=0):
    return 8 + 16 + 32 * n_inputs + 32 * n_outputs + 32


def record_fields(rec, n_outputs, n_inputs):
    """Views into one record: (index, ct_hash, input_commits[n_in,2,16], output_commits[n_out,2,16] = (label1, label0),
    true_constant_commit, false_constant_commit)."""
    rec = np.asarray(rec, np.uint8)
    assert rec.shape[-1] == record_len(n_outputs, n_inputs)
    o = 24
    inp = rec[o:o + 32 * n_inputs].reshape(n_inputs, 2, 16); o += 32 * n_inputs
    out = rec[o:o + 32 * n_outputs].reshape(n_outputs, 2, 16); o += 32 * n_outputs
    return int.from_bytes(bytes(rec[:8]), "little"), rec[8:24], inp, out, rec[o:o + 16], rec[o + 16:o + 32]


def commit_labels(labels):
    """AesLabelCommitHasher over an [n,16] array of labels."""
    from . import _chk, _p, lib
    labels = np.ascontiguousarray(labels, np.uint8).reshape(-1, 16)
    out = np.zeros_like(labels)
    _chk(lib().gsv_commit_labels(_p(labels), labels.shape[0], _p(out)))
    return out


def commit_record(index, ct_hash, output_label0, delta, false_label0, true_label0, input_label0=None):
    """GarbledInstanceCommit::new (garbler.rs:85-99).  `input_label0`: [n_in,16] label0 of the circuit's input wires in
    EncodeInput order (GarbledInstance.input_wire_values); label1 = label0 ^ delta."""
    out0 = np.ascontiguousarray(output_label0, np.uint8).reshape(-1, 16)
    delta = np.ascontiguousarray(delta, np.uint8).reshape(16)
    in0 = np.zeros((0, 16), np.uint8) if input_label0 is None else np.ascontiguousarray(input_label0, np.uint8).reshape(-1, 16)
    labels = np.concatenate([
        np.stack([in0, in0 ^ delta[None, :]], axis=1).reshape(-1, 16),    # per input: label0, label1
        np.stack([out0 ^ delta[None, :], out0], axis=1).reshape(-1, 16),  # per output: label1, label0
        (np.asarray(true_label0, np.uint8) ^ delta)[None, :],             # true.select(true)
        np.asarray(false_label0, np.uint8)[None, :],                      # false.select(false)
    ])
    rec = np.zeros(record_len(out0.shape[0], in0.shape[0]), np.uint8)
    rec[:8] = np.frombuffer(int(index).to_bytes(8, "little"), np.uint8)
    rec[8:24] = np.frombuffer(bytes(ct_hash), np.uint8)
    rec[24:] = commit_labels(labels).reshape(-1)
    return rec


def all_gather_records(local, total, rank, world, device=None):
    """All ranks end up with the [total, record_len] table ordered by instance index.  One all_gather
    (RCCL over xGMI when the backend is nccl; gloo in the CPU tests)."""
    if world == 1:
        out = local
    else:
        per = -(-total // world)
        rec_len = local.shape[1]
        dev = device or ("cuda" if dist.get_backend() == "nccl" else "cpu")
        buf = torch.zeros((per, rec_len), dtype=torch.uint8, device=dev)
        buf[: local.shape[0]] = local.to(dev)
        gathered = [torch.zeros_like(buf) for _ in range(world)]
        dist.all_gather(gathered, buf)
        rows = []
        for r in range(world):
            n_r = len(shard_instances(total, r, world))
            rows.append(gathered[r][:n_r].cpu())
        out = torch.cat(rows)
    # order by the instance index stored in the first 8 bytes
    a = out.cpu().numpy()
    idx = a[:, :8].copy().view("<u8").reshape(-1)
    return out.cpu()[torch.from_numpy(np.argsort(idx, kind="stable"))]


def _check_commitment(commitment):
    if commitment not in ("cbcmac", "blake3"):
        raise ValueError("commitment must be 'cbcmac' or 'blake3'")


def garble_and_commit(circuit, seeds, indexes, engine=None, program=None, replays=1, gc_dir=None, session_kw=None, threads=0, commitment="cbcmac", outboard_dir=None, checkpoint_dir=None,
                      check_dir=None):
    """Garbler::create + commit (garbler.rs:191-257) for the given (index, seed) pairs in ONE session: returns the
    [len(seeds), record_len] commit records; with gc_dir the ciphertext streams go to gc_<index>.bin
    (ciphertext_repository.rs:94-127).  Indexes must be consecutive when gc_dir is used.  `program` may be a Plan (the
    verifier): the stream is then drained window by window of the session's schedule.  commitment="blake3": the record's 16-byte
    ciphertext hash is the truncated BLAKE3 digest of the stream, computed on the device (Blake3Hasher truncates the same way);
    outboard_dir then receives the streams' BLAKE3 outboards gc_<index>.b3o (consecutive indexes, as for gc_dir).
    checkpoint_dir (commitment="cbcmac"): the streams' CBC-MAC checkpoint files gc_<index>.mck are written there (consecutive indexes).
    check_dir (commitment="cbcmac", no gc_dir): the streams are not drained but verified on the device against the checkpoint files
    gc_<index>.mck of that directory (Session.garble_check; any indexes); a stream that differs raises CiphertextMismatch with the
    position in `seeds` as its instance."""
    from . import Engine, Plan, Program, Session, labels_from_seed
    _check_commitment(commitment)
    if outboard_dir is not None and commitment != "blake3":
        raise ValueError("outboard_dir needs commitment='blake3'")
    if (checkpoint_dir is not None or check_dir is not None) and commitment != "cbcmac":
        raise ValueError("checkpoint_dir / check_dir need commitment='cbcmac'")
    if check_dir is not None and (gc_dir is not None or checkpoint_dir is not None):
        raise ValueError("check_dir verifies the streams where they are garbled: nothing is written")
    engine = engine or Engine(0)
    program = program or Program.from_circuit(circuit, chain_feedback=replays > 1)
    n_in = program.info["n_inputs"]
    B = len(seeds)
    delta = np.zeros((B, 16), np.uint8); consts = np.zeros((B, 2, 16), np.uint8); inputs = np.zeros((B, n_in, 16), np.uint8)
    for i, s in enumerate(seeds):
        delta[i], consts[i, 0], consts[i, 1], inputs[i] = labels_from_seed(int(s), n_in)
    if isinstance(program, Plan):
        sess = Session(engine, program, B, retain_stream=False, **(session_kw or {}))
    else:
        sess = Session(engine, program, B, replays, min(replays, 2) if replays > 1 else 1)
    sess.set_garble_inputs(delta, consts, inputs)
    if gc_dir is not None or outboard_dir is not None or checkpoint_dir is not None:
        assert list(indexes) == list(range(indexes[0], indexes[0] + B)), "gc files are numbered first_index + i"
    kw = {"outboard_dir": outboard_dir} if outboard_dir is not None else {}
    if checkpoint_dir is not None:
        kw["checkpoint_dir"] = checkpoint_dir
    if check_dir is not None:
        try:
            hashes = sess.garble_check(check_dir, indexes=[int(i) for i in indexes])
        except Exception:
            sess.close()
            raise
    else:
        hashes = sess.garble_streaming(directory=gc_dir, first_index=int(indexes[0]) if B else 0, threads=threads, commitment=commitment, **kw)  # threads: host MAC workers (0 = the engine's default)
    if commitment == "blake3":
        hashes = [d[:16] for d in hashes]
    outs = sess.read_outputs()
    recs = np.stack([commit_record(indexes[i], hashes[i], outs[i], delta[i], consts[i, 0], consts[i, 1], inputs[i]) for i in range(B)])
    sess.close()
    return recs


def cut_and_choose_commit(circuit, master_seed, total, rank, world, engine=None, program=None, garble=None, device=None, session_kw=None, threads=0, commitment="cbcmac"):
    """BASELINE config 5 / `Garbler::create` -> `commit` (garbler.rs:191-257) across ranks: `total` seeds are drawn from one master
    seed (:201-203), instance i goes to rank i mod world (the reference: one instance per pinned core, mod.rs:131-186), every rank
    garbles its instances WITH the ciphertext commitment (AESAccumulatingHash over the whole stream, :219-222) and builds their
    GarbledInstanceCommit records, and ONE all-gather leaves every rank with the [total, record_len] table ordered by instance
    index.  Nothing else is exchanged.  `garble(circuit, seeds, indexes) -> records` replaces the GPU garbler in the CPU tests.
    `threads`: host MAC workers of this rank's drain — the ranks of a node share the host's cores (bench.mac_threads_for_rank).
    commitment="blake3": the records carry the truncated BLAKE3 digest of the stream instead of the CBC-MAC; a `garble` stand-in is
    then called as garble(circuit, seeds, indexes, commitment="blake3").  Returns (table as a uint8 numpy array, seeds)."""
    _check_commitment(commitment)
    seeds = instance_seeds(master_seed, total)
    mine = shard_instances(total, rank, world)
    if garble is None:
        garble = lambda c, sd, idx, **kw: garble_and_commit(c, sd, idx, engine=engine, program=program, session_kw=session_kw, threads=threads, **kw)  # noqa: E731
    n_out, n_in = (program.info["n_outputs"], program.info["n_inputs"]) if program is not None else (None, None)
    if mine:
        kw = {} if commitment == "cbcmac" else {"commitment": commitment}
        local = np.ascontiguousarray(garble(circuit, [int(seeds[i]) for i in mine], mine, **kw), np.uint8)
    else:
        if n_out is None:
            raise ValueError("a rank without instances needs `program` to size its (empty) share of the gather")
        local = np.zeros((0, record_len(n_out, n_in)), np.uint8)
    table = all_gather_records(torch.from_numpy(local), total, rank, world, device=device)
    return table.numpy(), seeds


def _outboard_header(ob):
    """(k, n_records) of an outboard's 24-byte header (include/gsv_engine.h, "BLAKE3 outboards"), or None."""
    if len(ob) < 24 or ob[:8] != b"GSVB3OB\n" or int.from_bytes(ob[8:12], "little") != 1:
        return None
    return int.from_bytes(ob[12:16], "little"), int.from_bytes(ob[16:24], "little")


def _last_chunk(path):
    """The bytes of a gc file behind its last whole-KiB boundary in front of the end: what no outboard represents."""
    import os
    size = os.path.getsize(path)
    start = (max(1, -(-size // 1024)) - 1) * 1024
    with open(path, "rb") as f:
        f.seek(start)
        return f.read()


def _host_file_check(path, outboard_path):
    """blake3_file with an outboard, on the host: (digest, None) when the file matches its outboard, (digest, group) with the first
    group of 2^k chunks that differs (the tail behind the last complete group counts as the group after it)."""
    import os
    import tempfile
    from . import GsvError, blake3_file_outboard
    want = open(outboard_path, "rb").read()
    head = _outboard_header(want)
    if head is None or head[0] > 20:
        raise GsvError("%s is not an outboard" % outboard_path)
    k = head[0]
    with tempfile.TemporaryDirectory() as td:
        mine = os.path.join(td, "file.b3o")
        digest = blake3_file_outboard(path, k, mine)
        got = open(mine, "rb").read()
    if got == want:
        return digest, None
    if got[:24] != want[:24] or len(got) != len(want):
        raise GsvError("%s is not the outboard of a file of this length" % outboard_path)
    n_groups = (max(1, -(-head[1] // 64)) - 1) >> k
    v = next(j for j in range((len(got) - 24) // 32) if got[24 + 32 * j:56 + 32 * j] != want[24 + 32 * j:56 + 32 * j])
    return digest, min(v, n_groups)


def _device_file_hashes(engine, paths, outboards):
    """blake3_files over the received files of the finalized instances: {position: 16-byte hash | "message"}.  A file that differs from
    its outboard is named and the rest is hashed again without it; a file the device call cannot take (another length than the
    others, an outboard that is none) goes through the host."""
    from . import CiphertextMismatch, GsvError, blake3_file, blake3_files
    out, todo = {}, list(range(len(paths)))
    while todo:
        try:
            got = blake3_files(engine, [paths[j] for j in todo], None if outboards is None else [outboards[j] for j in todo])
            out.update({j: d[:16] for j, d in zip(todo, got)})
            break
        except CiphertextMismatch as e:
            out[todo.pop(e.instance)] = "ciphertext corrupted (group %d)" % e.group
        except GsvError:
            for j in todo:
                try:
                    if outboards is None:
                        out[j] = blake3_file(paths[j])[:16]
                    else:
                        d, group = _host_file_check(paths[j], outboards[j])
                        out[j] = d[:16] if group is None else "ciphertext corrupted (group %d)" % group
                except Exception as e:  # noqa: BLE001
                    out[j] = "failed to get ciphertext source: %s" % e
            break
    return out


def _mac_file_hashes(engine, paths, checkpoints):
    """The finalized instances' files against their CBC-MAC checkpoint files: {position: 16-byte hash | "message"}.  With an engine on
    the device (cbcmac_files) — a file that differs is named and the rest is checked again without it, and files the device call cannot
    take together (another length or k than the others, a checkpoint file that is none) go through the host checker one by one."""
    from . import CiphertextMismatch, GsvError, cbcmac_file_check, cbcmac_files

    def host(j):
        try:
            h, group = cbcmac_file_check(paths[j], checkpoints[j])
            return h if group is None else "ciphertext corrupted (group %d)" % group
        except Exception as e:  # noqa: BLE001
            return "failed to get ciphertext source: %s" % e
    out, todo = {}, list(range(len(paths))) if engine is not None else []
    while todo:
        try:
            got = cbcmac_files(engine, [paths[j] for j in todo], [checkpoints[j] for j in todo])
            out.update(dict(zip(todo, got)))
            break
        except CiphertextMismatch as e:
            out[todo.pop(e.instance)] = "ciphertext corrupted (group %d)" % e.group
        except GsvError:
            break
    for j in range(len(paths)):
        if j not in out:
            out[j] = host(j)
    return out


def run_regarbling(commits, to_finalize, seeds, circuit, gc_dir, engine=None, program=None, replays=1, commitment="cbcmac", outboard_dir=None, checkpoint_dir=None):
    """Evaluator::run_regarbling (cut_and_choose/evaluator.rs:83-181).  `commits`: [total, record_len] table of the
    garbler's commit records; `to_finalize`: indexes kept for evaluation; `seeds`: {index: seed} of the OPENED instances.
      * finalized index: its gc_<index>.bin is streamed through the CBC-MAC and compared with the committed ciphertext
        hash ("ciphertext corrupted" otherwise);
      * opened index: the circuit is garbled again from the revealed seed — all opened instances in one GPU launch —
        and the whole commit record must match ("regarbling failed"); a missing seed is an error ("failed to find seed").
    commitment="blake3": the committed hash is the truncated BLAKE3 digest — the file is hashed with blake3_file, the re-garbling
    commits the same way.  With an `engine` the finalized instances' files are hashed on the device instead (blake3_files: read in
    bounded segments, never evaluated); outboard_dir (the outboards gc_<index>.b3o the garbler sent) makes either path compare every
    group of 2^k chunks with the file's outboard, and a file that differs is reported as "ciphertext corrupted (group g)" — the part
    to fetch again.
    checkpoint_dir (commitment="cbcmac"): the garbler's CBC-MAC checkpoint files gc_<index>.mck lie there.  A finalized file that has
    one is verified group by group against it — on the device with an `engine` (cbcmac_files), else by the host checker
    (cbcmac_file_check) — its last state is what is compared with the committed hash, and a file that differs is reported as
    "ciphertext corrupted (group g)".  Opened instances that have one are re-garbled and verified on the device without their
    ciphertexts leaving it (Session.garble_check); the record compare is unchanged.  Instances without a checkpoint file take the
    paths above.  Returns (ok, errors) with errors = {index: message}; the reference returns Err(()) as soon as any instance fails."""
    import os
    from . import CiphertextMismatch, blake3_file, checkpoint_file_name, gc_file_name, outboard_file_name, read_gc_file
    _check_commitment(commitment)
    if outboard_dir is not None and commitment != "blake3":
        raise ValueError("outboard_dir needs commitment='blake3'")
    if checkpoint_dir is not None and commitment != "cbcmac":
        raise ValueError("checkpoint_dir needs commitment='cbcmac'")

    def has_checkpoints(i):
        return checkpoint_dir is not None and os.path.exists(os.path.join(checkpoint_dir, checkpoint_file_name(i)))
    commits = np.asarray(commits, np.uint8)
    errors = {}
    fin = set(int(i) for i in to_finalize)
    device = {}
    if commitment == "blake3" and engine is not None:
        there = [i for i in sorted(fin) if os.path.exists(os.path.join(gc_dir, gc_file_name(i))) and (outboard_dir is None or os.path.exists(os.path.join(outboard_dir, outboard_file_name(i))))]
        got = _device_file_hashes(engine, [os.path.join(gc_dir, gc_file_name(i)) for i in there],
                                  None if outboard_dir is None else [os.path.join(outboard_dir, outboard_file_name(i)) for i in there])
        device = {i: got[j] for j, i in enumerate(there)}
    if checkpoint_dir is not None:
        there = [i for i in sorted(fin) if os.path.exists(os.path.join(gc_dir, gc_file_name(i))) and has_checkpoints(i)]
        got = _mac_file_hashes(engine, [os.path.join(gc_dir, gc_file_name(i)) for i in there], [os.path.join(checkpoint_dir, checkpoint_file_name(i)) for i in there])
        device = {i: got[j] for j, i in enumerate(there)}
    for index in sorted(fin):
        path = os.path.join(gc_dir, gc_file_name(index))
        try:
            if index in device:
                h = device[index]
            elif commitment == "blake3" and outboard_dir is not None:
                h, group = _host_file_check(path, os.path.join(outboard_dir, outboard_file_name(index)))
                h = h[:16] if group is None else "ciphertext corrupted (group %d)" % group
            else:
                h = blake3_file(path)[:16] if commitment == "blake3" else read_gc_file(path)[1]
        except Exception as e:  # FileSource::from_path failing (ciphertext_source.rs:36-60)
            errors[index] = "failed to get ciphertext source: %s" % e
            continue
        if isinstance(h, str):
            errors[index] = h
        elif bytes(h) != bytes(commits[index, 8:24]):
            errors[index] = "ciphertext corrupted"
    opened = [i for i in range(commits.shape[0]) if i not in fin]
    missing = [i for i in opened if i not in seeds]
    for i in missing:
        errors[i] = "failed to find seed"
    todo = [i for i in opened if i in seeds and not has_checkpoints(i)]
    if todo:
        recs = garble_and_commit(circuit, [seeds[i] for i in todo], todo, engine=engine, program=program, replays=replays, commitment=commitment)
        for k, i in enumerate(todo):
            if not (recs[k] == commits[i]).all():
                errors[i] = "regarbling failed"
    # ... and the opened instances whose checkpoint files are there: verified where they are garbled.  A stream that differs from its
    # checkpoints cannot give the committed hash; it is named, and the others are garbled again without it.
    todo = [i for i in opened if i in seeds and has_checkpoints(i)]
    while todo:
        try:
            recs = garble_and_commit(circuit, [seeds[i] for i in todo], todo, engine=engine, program=program, replays=replays, check_dir=checkpoint_dir)
        except CiphertextMismatch as e:
            errors[todo.pop(e.instance)] = "regarbling failed"
            continue
        for k, i in enumerate(todo):
            if not (recs[k] == commits[i]).all():
                errors[i] = "regarbling failed"
        break
    return (not errors), errors


class ConsistencyError(Exception):
    """cut_and_choose/evaluator.rs ConsistencyError: `kind` is the variant name, `index` the instance."""

    def __init__(self, kind, index, **details):
        super().__init__("%s (instance %d)%s" % (kind, index, (" " + repr(details)) if details else ""))
        self.kind, self.index, self.details = kind, index, details


def _last_checkpoint(path, n_records):
    """The commitment a CBC-MAC checkpoint file claims for a stream of n_records records: its last state, sixteen zero bytes for the
    empty stream.  The file is not read whole (2^-k of the stream: large at small k): its byte length comes from the engine
    (cbcmac_checkpoints_size, the one place that knows the format) for the k the header names, and the last 16 bytes are read."""
    import os
    from . import cbcmac_checkpoints_size
    with open(path, "rb") as f:
        head = f.read(24)
        size = os.fstat(f.fileno()).st_size
        if len(head) < 24 or head[:8] != b"GSVMACK\n" or int.from_bytes(head[8:12], "little") != 1:
            raise ValueError("%s is not a version 1 checkpoint file" % path)
        k, n = int.from_bytes(head[12:16], "little"), int.from_bytes(head[16:24], "little")
        if n != n_records:
            raise ValueError("%s holds the checkpoints of a stream of %d records, the stream here holds %d" % (path, n, n_records))
        if k > 30 or size != cbcmac_checkpoints_size(n, k):
            raise ValueError("%s: k = %d and n_records = %d do not make %d bytes" % (path, k, n, size))
        if n == 0:
            return bytes(16)
        f.seek(size - 16)
        return f.read(16)


def _gpu_evaluate_batch(circuit, engine, program, gc_dir, commitment="cbcmac", outboard_dir=None, checkpoint_dir=None):
    """Default evaluation backend of evaluate_from: EvaluateMode over FileSources on the GPU, ALL finalized instances in one session —
    one launch per window of the stream for the whole batch (gsv_session_evaluate_streaming_indexed).  The reference evaluates the
    cases side by side on a rayon pool (`into_par_iter`, cut_and_choose/evaluator.rs:354-475); a one-instance session per case would
    use one CU of 256 and pay a session per case.  The files' CBC-MACs (the CiphertextMismatch check) are folded while reading, instance i on
    worker i mod T of the engine's pool, beside the uploads (engine.cpp, evaluate_streaming_impl).  commitment="blake3": the hash of a
    case is the first 16 bytes of its file's BLAKE3 digest instead, computed on the device from the uploaded segments (no MAC worker).
    outboard_dir: verified streaming — `run` then takes expected= (the committed 16-byte hashes) and raises CiphertextMismatch, with the
    position in the batch as its instance, at the first group that differs from its outboard.  checkpoint_dir (commitment="cbcmac"):
    the same against the CBC-MAC checkpoint files gc_<i>.mck of that directory, on the device and without MAC workers."""
    from . import Engine, Plan, Program, Session
    _check_commitment(commitment)
    eng = engine or Engine(0)
    prog = program or Program.from_circuit(circuit)

    def run(indexes, true_active, false_active, input_active, input_bits, expected=None):
        B = len(indexes)
        sess = Session(eng, prog, B, retain_stream=False) if isinstance(prog, Plan) else Session(eng, prog, B)
        try:
            consts = np.stack([np.asarray(false_active, np.uint8).reshape(B, 16), np.asarray(true_active, np.uint8).reshape(B, 16)], axis=1)
            sess.set_evaluate_inputs(consts, np.asarray(input_active, np.uint8).reshape(B, -1, 16), np.asarray(input_bits, np.uint8).reshape(B, -1))
            kw = {"outboard_dir": outboard_dir, "expected": expected} if outboard_dir is not None else {}
            if checkpoint_dir is not None:
                kw = {"checkpoint_dir": checkpoint_dir, "expected": expected}
            hashes = [h[:16] for h in sess.evaluate_streaming_indexed(gc_dir, [int(i) for i in indexes], commitment=commitment, **kw)]
            labels, bits = sess.read_outputs(with_bits=True)
            return [(labels[k], bits[k], hashes[k]) for k in range(B)]
        finally:
            sess.close()
    return run


def evaluate_from(commits, cases, circuit, gc_dir, n_outputs, engine=None, program=None, evaluate=None, evaluate_batch=None, commitment="cbcmac", outboard_dir=None, checkpoint_dir=None):
    """Evaluator::evaluate_from (cut_and_choose/evaluator.rs:338-476): evaluate the finalized instances from their gc_<i>.bin and
    check everything the evaluator was handed against the garbler's commit record BEFORE trusting the result.
    `cases`: list of dicts {index, true_constant_wire[16], false_constant_wire[16], input_active[n_in,16], input_bits[n_in]}
    (EvaluatorCaseInput).  Raises ConsistencyError with the reference's variants — TrueConstantMismatch,
    FalseConstantMismatch, MissingCiphertextHash, InputLabelsCountMismatch, InputLabelsMismatch, CiphertextMismatch,
    OutputLabelMismatch — and returns [(index, output_active[n_out,16], output_bits[n_out])].

    The cases are evaluated TOGETHER (the reference: `into_par_iter`): the checks that need no evaluation run for every case first,
    then one batch evaluates every case in front of the first failing one, then the remaining checks run case by case — so the error
    raised is the one a case-by-case run in list order would raise (per case the reference's order of checks, evaluator.rs:371-465).
    `evaluate_batch(indexes, true[B,16], false[B,16], input_active[B,n_in,16], input_bits[B,n_in]) -> [(output_active, output_bits,
    ciphertext_hash)]` defaults to the GPU evaluator; `evaluate(index, true, false, input_active, input_bits) -> (..)` is the
    case-by-case form tests without a GPU pass (the CPU oracle's).
    commitment="blake3": the table was written with commitment="blake3" (garble_and_commit), the record's hash field is the first 16
    bytes of BLAKE3(gc_<i>.bin), and the default GPU evaluator returns that of the file it read; the stand-ins keep their signature
    and return whatever hash they choose.
    outboard_dir (with commitment="blake3"): the garbler's BLAKE3 outboards gc_<i>.b3o lie there and the evaluation is VERIFIED — each
    outboard, folded with the last chunk of its file, must give the committed hash before anything is evaluated, and the default GPU
    evaluator stops at the first group of 2^k chunks that differs from its outboard (Session.evaluate_streaming_indexed(outboard_dir=,
    expected=)).  Either is ConsistencyError("CiphertextMismatch", index) with the group in its message; the checks of the cases in
    front of that one which need no evaluation still come first.  With a stand-in the up-front check runs here on the host, and the
    stand-in may raise CiphertextMismatch itself (a batch stand-in: with the position in the batch as its instance).
    checkpoint_dir (with commitment="cbcmac"): the garbler's CBC-MAC checkpoint files gc_<i>.mck lie there and the evaluation is
    VERIFIED in the same way against them — each file's last state must be the committed hash before anything is evaluated, and the
    default GPU evaluator stops at the first group of 2^k records that does not arrive at its claimed state
    (Session.evaluate_streaming_indexed(checkpoint_dir=, expected=)), with no MAC worker on the host.  The errors, their order and
    the stand-ins' part are those of outboard_dir."""
    import os
    from . import CiphertextMismatch, blake3_outboard_root, checkpoint_file_name, gc_file_name, outboard_file_name
    _check_commitment(commitment)
    if outboard_dir is not None and commitment != "blake3":
        raise ValueError("outboard_dir needs commitment='blake3'")
    if checkpoint_dir is not None and commitment != "cbcmac":
        raise ValueError("checkpoint_dir needs commitment='cbcmac'")
    commits = np.asarray(commits, np.uint8)
    gpu_default = evaluate_batch is None and evaluate is None
    if evaluate_batch is None:
        if evaluate is not None:
            def evaluate_batch(idx, t, f, a, b):
                out = []
                for k in range(len(idx)):
                    try:
                        out.append(evaluate(idx[k], t[k], f[k], a[k], b[k]))
                    except CiphertextMismatch as e:
                        raise CiphertextMismatch(str(e), k, e.group, e.first_record)
                return out
        else:
            evaluate_batch = _gpu_evaluate_batch(circuit, engine, program, gc_dir, commitment, outboard_dir, checkpoint_dir)
    n_in_committed = (commits.shape[1] - record_len(n_outputs, 0)) // 32
    parsed, first_error = [], None
    for case in cases:
        index = int(case["index"])
        t_act = np.asarray(case["true_constant_wire"], np.uint8).reshape(16)
        f_act = np.asarray(case["false_constant_wire"], np.uint8).reshape(16)
        in_act = np.asarray(case["input_active"], np.uint8).reshape(-1, 16)
        in_bits = np.asarray(case["input_bits"], np.uint8).reshape(-1)
        _, ct_commit, in_commits, out_commits, true_commit, false_commit = record_fields(commits[index], n_outputs, n_in_committed)
        got = commit_labels(np.stack([t_act, f_act]))
        if bytes(got[0]) != bytes(true_commit):
            first_error = ConsistencyError("TrueConstantMismatch", index, expected=bytes(true_commit), actual=bytes(got[0]))
        elif bytes(got[1]) != bytes(false_commit):
            first_error = ConsistencyError("FalseConstantMismatch", index, expected=bytes(false_commit), actual=bytes(got[1]))
        elif not os.path.exists(os.path.join(gc_dir, gc_file_name(index))):
            first_error = ConsistencyError("MissingCiphertextHash", index)
        elif in_act.shape[0] != n_in_committed or in_bits.shape[0] != n_in_committed:
            # (the reference counts after evaluating; a batch cannot hold a ragged case, and no other check can fire first)
            first_error = ConsistencyError("InputLabelsCountMismatch", index, expected=n_in_committed, actual=in_act.shape[0])
        if first_error is not None:
            break
        parsed.append((index, t_act, f_act, in_act, in_bits, ct_commit, in_commits, out_commits))
    results = []

    def check_input_labels(index, in_act, in_bits, in_commits):
        actual = commit_labels(in_act)
        expected = in_commits[np.arange(n_in_committed), in_bits.astype(np.int64) & 1]  # commit_for_value(value)
        bad = np.nonzero((actual != expected).any(axis=1))[0]
        if bad.size:
            k = int(bad[0])
            raise ConsistencyError("InputLabelsMismatch", index, label_index=k, expected=bytes(expected[k]), actual=bytes(actual[k]))

    def ciphertext_mismatch(pos, **details):
        """a verified evaluation found case `pos` of the batch bad: the cases in front of it first get the check that needs no evaluation"""
        for c in parsed[:pos + 1]:
            check_input_labels(c[0], c[3], c[4], c[6])
        return ConsistencyError("CiphertextMismatch", parsed[pos][0], **details)

    if parsed and outboard_dir is not None and not gpu_default:
        for pos, c in enumerate(parsed):  # (the default GPU evaluator makes this check itself, before it uploads anything)
            try:
                root = blake3_outboard_root(open(os.path.join(outboard_dir, outboard_file_name(c[0])), "rb").read(), _last_chunk(os.path.join(gc_dir, gc_file_name(c[0]))))
            except Exception as e:  # noqa: BLE001 - no outboard, or a malformed one
                raise ciphertext_mismatch(pos, outboard=str(e))
            if root[:16] != bytes(c[5]):
                raise ciphertext_mismatch(pos, outboard="outboard or last chunk does not match the commitment")
    if parsed and checkpoint_dir is not None and not gpu_default:
        for pos, c in enumerate(parsed):  # (likewise: each file's last state against the record's hash)
            try:
                claimed = _last_checkpoint(os.path.join(checkpoint_dir, checkpoint_file_name(c[0])), os.path.getsize(os.path.join(gc_dir, gc_file_name(c[0]))) // 16)
            except Exception as e:  # noqa: BLE001 - no checkpoint file, or a malformed one
                raise ciphertext_mismatch(pos, checkpoints=str(e))
            if claimed != bytes(c[5]):
                raise ciphertext_mismatch(pos, checkpoints="the last checkpoint does not match the commitment")
    if parsed:
        kw = {"expected": [bytes(c[5]) for c in parsed]} if gpu_default and (outboard_dir is not None or checkpoint_dir is not None) else {}
        try:
            evaluated = evaluate_batch([c[0] for c in parsed], np.stack([c[1] for c in parsed]), np.stack([c[2] for c in parsed]),
                                       np.stack([c[3] for c in parsed]), np.stack([c[4] for c in parsed]), **kw)
        except CiphertextMismatch as e:
            raise ciphertext_mismatch(e.instance, group=e.group, first_record=e.first_record, message=str(e))
        for (index, _t, _f, in_act, in_bits, ct_commit, in_commits, out_commits), (out_act, out_bits, file_hash) in zip(parsed, evaluated):
            check_input_labels(index, in_act, in_bits, in_commits)
            if bytes(file_hash) != bytes(ct_commit):
                raise ConsistencyError("CiphertextMismatch", index, expected=bytes(ct_commit), actual=bytes(file_hash))
            out_act = np.asarray(out_act, np.uint8).reshape(-1, 16)
            out_bits = np.asarray(out_bits, np.uint8).reshape(-1)
            oh = commit_labels(out_act)
            exp_out = out_commits[np.arange(n_outputs), 1 - (out_bits.astype(np.int64) & 1)]  # value 1 -> label1 commit (stored first)
            if (oh != exp_out).any():
                raise ConsistencyError("OutputLabelMismatch", index)
            results.append((index, out_act, out_bits))
    if first_error is not None:
        raise first_error
    return results
