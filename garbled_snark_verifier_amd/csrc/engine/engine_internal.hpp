// Types and helpers shared by the parts of the host runtime (engine.cpp is ONE translation unit; its parts are the engine_*.ipp files,
// included in order inside its extern "C" block): error reporting, device allocation, the deferred-release gate, and the objects behind the
// opaque handles of include/gsv_engine.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/gsv_engine.h"
#include "../gadgets/circuits.hpp"
#include "drain_pipeline.hpp"
#include "hip_owned.hpp"
#include "host_crypto.hpp"
#include "kernel_api.h"
#include "knobs.hpp"
#include "mac_checkpoints.hpp"
#include "plan_builder.hpp"
#include "plan_layout.hpp"
#include "schedule.hpp"
#include "program.hpp"
#include "upload_pipeline.hpp"

using namespace gsv;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define GSV_TRY try {
#define GSV_CATCH                                                                 \
  }                                                                               \
  catch (const std::exception& e) { return fail(GSV_ERR_CIRCUIT, e.what()); }     \
  catch (...) { return fail(GSV_ERR_CIRCUIT, "unknown exception"); }

// A failed HIP call leaves its error behind for hipGetLastError(); the kernel launchers report hipGetLastError(), so the stale
// error of e.g. an out-of-memory hipMalloc would make every later launch of the process look failed: clear it here.
#define HIPCHK(expr)                                                                                         \
  do {                                                                                                       \
    hipError_t _e = (expr);                                                                                  \
    if (_e != hipSuccess) {                                                                                  \
      (void)hipGetLastError();                                                                               \
      return fail(GSV_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));                        \
    }                                                                                                        \
  } while (0)

// Large device allocations report what was asked for and what the device had left.
static int dev_alloc(DevBuf& p, size_t bytes, const char* what) {
  hipError_t e = p.alloc(bytes ? bytes : 16);
  if (e == hipSuccess) return GSV_OK;
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  char msg[256];
  std::snprintf(msg, sizeof msg, "hipMalloc of %.2f GB for %s failed (%s): device has %.2f of %.2f GB free", double(bytes) / 1e9, what, hipGetErrorString(e), double(free_b) / 1e9,
                double(total_b) / 1e9);
  return fail(GSV_ERR_DEVICE, msg);
}
#define DEVALLOC(p, bytes, what) do { int _rc = dev_alloc((p), (bytes), (what)); if (_rc) return _rc; } while (0)
// ---- deferred release ---------------------------------------------------------------------------------------------------------------
// Releasing device memory or a stream synchronises the device.  While a streaming pass runs that is at best a stall of whoever destroys something
// and at worst a deadlock: a ring pass waits for the host's stream position, which waits for a sink / source callback — and a host that
// drops a session, plan, program or engine FROM that callback (a Rust `Drop` inside `CiphertextHandler::handle`, Python's collector on
// the callback thread: profiles/r05_debug/) would wait in the release for that very pass until the device's watchdog ends it.  The destroy
// entry points therefore never free while a streaming pass is in flight in this process: the request is queued and runs, in order, when
// the last pass in flight has synchronised (the handle is invalid for the host from the moment destroy returns, as always).  Outside a
// pass a destroy runs at once, under the gate's lock: a pass that starts meanwhile waits for it instead of being stalled by it.
namespace {
struct ReleaseGate {
  std::recursive_mutex mu;                      // recursive: a queued plan destroy runs its programs' destroys
  int active = 0;                               // streaming passes in flight (any session of this process)
  std::vector<std::function<void()>> pending;   // destroy requests that arrived meanwhile, in arrival order
  uint64_t n_deferred = 0;                      // statistics (gsv_deferred_release_count)
};
ReleaseGate& release_gate() { static ReleaseGate g; return g; }
// First local of every streaming entry point: declared before anything else so that it is destroyed LAST — a session destroyed from
// its own pass's callback is still alive while the entry point uses it.  Also reads this pass's knobs into s->pass (s may be null).
struct PassGuard {
  explicit PassGuard(gsv_session* s);  // (below gsv_session)
  ~PassGuard() {
    ReleaseGate& g = release_gate();
    std::lock_guard<std::recursive_mutex> lk(g.mu);
    if (--g.active != 0) return;
    std::vector<std::function<void()>> run;
    run.swap(g.pending);
    for (auto& f : run) f();
  }
  PassGuard(const PassGuard&) = delete;
  PassGuard& operator=(const PassGuard&) = delete;
};
void release_or_defer(std::function<void()> fn) {
  ReleaseGate& g = release_gate();
  std::lock_guard<std::recursive_mutex> lk(g.mu);
  if (g.active > 0) { g.pending.push_back(std::move(fn)); ++g.n_deferred; return; }
  fn();
}
}  // namespace

// A stream that must make progress WHILE a window runs on the engine's stream (the drain's gathers and copies, the other half of a
// garble -> evaluate pair).  The runtime multiplexes streams onto a few hardware queues per priority level, in order within a queue: a
// side stream that lands on the main stream's queue would sit behind the running window — which, with a ciphertext ring, itself waits
// for that side stream's work (observed: the ring stalls until the device watchdog fires, depending on how many streams the process
// had created before).  Streams of another priority level come from another pool of hardware queues, so these ask for the highest.
// (Not for the evaluator of a garble -> evaluate pair: two long launches on queues of DIFFERENT priority, whichever way round, took
// 46.5 s for the verifier instead of 42.9 s on equal terms — ensure_pair probes for a stream of the same priority that overlaps.)
static hipError_t create_side_stream(Stream& out, bool highest_priority) {
  int least = 0, greatest = 0;
  if (!highest_priority || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || greatest == least) return out.create(hipStreamNonBlocking);
  return out.create(hipStreamNonBlocking, greatest);
}

struct gsv_recorder {
  RecordMode mode;
  std::vector<uint32_t> inputs, outputs;  // SSA ids
  bool outputs_declared = false;
};

struct DevProgram {
  DevBuf steps, ands, xors, fb_src, fb_dst, out_slots, ct_pos;
  size_t bytes = 0;
};

// What a program was compiled from: kept so that the half-window variant (two instances per workgroup) can be
// compiled the first time a session needs it.
struct ProgramSource {
  Trace trace;
  std::vector<uint32_t> inputs, outputs;
  std::vector<std::pair<uint32_t, uint32_t>> feedback;
  CompileOptions opt;
};

struct gsv_program {
  Program prog;                    // compiled for 1/window_div of the LDS label window: serves every layout of up to window_div instances per workgroup
  std::map<uint32_t, std::unique_ptr<Program>> variants;  // instances per workgroup (2, 4) -> the program compiled for that share of the window, on demand, from `src`
  uint32_t window_div = 1;         // 1: full window (the other layouts are compiled on demand); 2 / 4: `prog` itself was compiled for half / a quarter of the
                                   // window and is the only image (GSV_PLAN_WINDOW_DIV: no second variant, no trace kept)
  bool device_only = false;        // loaded by gsv_plan_load straight into device memory: the host keeps the metadata, not the records
  uint64_t loaded_image_bytes = 0; // size of the records of a device_only program
  uint32_t image_key(uint32_t ni) const { return ni <= window_div ? 1u : ni; }  // which compiled image a layout runs
  const Program& variant(uint32_t ni) const { return ni <= window_div ? prog : *variants.at(ni); }
  std::unique_ptr<ProgramSource> src;
  std::mutex mu;
  std::map<std::pair<int, int>, std::shared_ptr<DevProgram>> dev;  // per (device, image key); sessions look at the images through plain pointers: they never keep one alive
  // gsv_program_compile_opts(background = 1): the handle exists at once, `prog` is filled by a worker of the library's compile pool.  What a
  // plan recorder needs to take a call of the program (arity, gate count) is known from the recording and kept here; everything that
  // reads `prog` goes through program_ready() first.
  uint64_t decl_inputs = 0, decl_outputs = 0, decl_gates = 0;
  bool has_feedback = false, has_decl = false;
  struct gsv_plan_recorder* for_recorder = nullptr;  // compiled with gsv_compile_opts.for_plan: registered there until either side is destroyed (g_recorder_link_mu)
  std::mutex cmu;
  std::condition_variable ccv;
  bool compiling = false;
  int compile_rc = 0;
  std::string compile_err;
  size_t image_bytes() const {
    if (device_only) return size_t(loaded_image_bytes);
    return prog.steps.size() * sizeof(StepDesc) + prog.ands.size() * sizeof(AndRec) + prog.xors.size() * sizeof(XorRec) +
           (prog.fb_src_slot.size() * 2 + prog.output_slots.size() + prog.ct_pos.size()) * sizeof(uint32_t);
  }
};

// A plan = a sequence of calls to compiled programs over ONE wire file per instance (component-level programs: the
// reference instantiates the same component shapes thousands of times, streaming_mode.rs:150-247).  Wires that cross
// calls live in a "global" region behind the programs' own slots; a call copies its inputs in, runs, copies its outputs out.
struct PlanCall {
  gsv_program* prog;
  std::vector<uint32_t> in_globals, out_globals;
  uint64_t gid_off = 0, ct_off = 0;  // gate ids / ciphertext records consumed by the calls before this one
};
struct gsv_plan {
  std::vector<gsv_program*> owned;  // programs created by gsv_plan_from_circuit (destroyed with the plan)
  std::vector<PlanCall> calls;
  uint32_t n_globals = 0, n_inputs = 0;
  std::vector<uint32_t> outputs;
  uint64_t n_gates = 0, n_ct = 0;
  bool finished = false;
  int device = -1;  // >= 0: loaded by gsv_plan_load straight into that device's memory (device_only programs): serves that device only
};

struct gsv_engine {
  int device = 0;
  Stream stream;
  DevBuf te;  // device T-tables
  double b3_streams_seconds = 0;  // last gsv_engine_blake3_streams: HIP-event time from the first hash kernel to the last (upload in front and the host's finish behind are outside)
  double mac_check_seconds = 0;   // last gsv_engine_cbcmac_streams_check: HIP-event time from the first check kernel to the last failing-group word (the upload in front is outside)
  ~gsv_engine() { (void)hipSetDevice(device); }  // ... then te, then the stream
};

struct PairState;
struct B3Stream;
struct MacCheckStream;
struct EvalCarry;
struct gsv_session {
  gsv_engine* e = nullptr;
  gsv_program* p = nullptr;
  const DevProgram* dp = nullptr;  // program sessions: the program's image on this device (owned by p->dev)
  size_t n_inst = 0;
  uint64_t replays = 1, ct_cap = 1;
  DevBuf W, VB, CT, delta, out, out_bits, in_bits, step_clock, ct_stage;
  DevBuf ct_gate;  // its bytes() is also the capacity of every buffer of ct_gate_more (ensure_ct_gate)
  Event ev0, ev1;
  int hasher = 0;  // 0 AesNiHasher, 1 Blake3Hasher (gsv_session_set_hasher: any time between passes)
  knobs::Session kn; knobs::Pass pass;  // knobs.hpp: read when the session was created / at the top of the garble or evaluate entry point that runs (PassGuard, or assigned there): per pass
  uint32_t ni = 1;  // instances per workgroup the session was laid out for (chosen at creation: program variants, schedule)
  // ... and of its LAUNCHES: gsvk_launch_batch runs BLAKE3 (one gate per lane, no multi-lane form) at one instance per workgroup whatever
  // the layout, and the hasher may change after creation.  Everything that counts workgroups or indexes by blockIdx.x asks here.
  uint32_t launch_ni() const { return hasher == 1 ? 1u : ni; }
  size_t launch_groups() const { return (n_inst + launch_ni() - 1) / launch_ni(); }  // grid.x of a launch = instance groups
  const gsv_plan* plan = nullptr;
  std::string ring_diag;  // ring mode: the longest interval between two publications of the host's position in the last pass, and where it went
  Stream aux_stream;  // gather kernels and flag polls of the drain, beside the running window
  std::vector<const DevProgram*> call_dev;  // per call of the plan: its program's image (owned by that program)
  // Call-level schedule (schedule.hpp): windows of consecutive calls; the calls of a window run as a dataflow inside ONE launch
  // (grid.y = calls), each waiting for the completion flags of the calls it depends on.  Everything of the session that depends on the
  // schedule is ONE value: the layout (plan_layout.hpp: schedule, facade, wire-file layout, the tables in stream order) and what
  // make_plan_state puts on the device for it — the tables, the completion flags [instance group][call] (compared with the launch epoch:
  // never reset) and the two mapped counters.  Built whole, then assigned: the session never holds half of one.
  struct PlanState {
    PlanLayout L;
    DevBuf d_calls, d_copy_src, d_copy_dst, d_deps, d_flags, d_error, plan_out_slots;
    MappedHost<uint32_t> done;  // per call of the plan: workgroups that have finished it in the current pass (mapped host memory, written by the device)
    MappedHost<unsigned long long> ct_pos;  // ring mode: the host's stream-position counter (page-locked, mapped into the device)
  } ps;
  const Schedule& sched() const { return ps.L.sched; }
  bool retain() const { return ps.L.retain; }              // plan sessions: whole ciphertext stream kept on the device (else one block: streaming only)
  bool ring() const { return ps.L.ring; }                  // the device block is a ring of max_block() records
  bool safe() const { return ps.L.safe; }                  // the schedule is the safe one
  uint64_t max_block() const { return ps.L.max_block; }    // ciphertext records per instance of the device block
  uint64_t max_segment() const { return ps.L.max_segment; }  // ... of a gate-order buffer
  // A fall-back to the safe schedule that failed while the session's buffers were growing leaves `ps` empty and says why here: the
  // session then refuses to stage inputs or to run (plan_session_usable)
  std::string unusable;
  uint32_t epoch = 0;
  // Safe-schedule fallback (round 6): the options the session was created with and the host's last inputs (re-staged when a pass is
  // repeated), so that a second schedule can be installed into the same session.
  gsv_plan_session_opts opts{};
  bool dep_fault = false;                    // the last pass ended with status 1 (a dependency wait gave up)
  uint64_t n_fallbacks = 0;
  std::vector<uint8_t> stash_delta, stash_consts, stash_inputs, stash_bits;
  int stash_kind = 0;                        // 0 nothing, 1 garble inputs, 2 evaluate inputs
  size_t drain_instances = 0;               // streaming calls: only the first this-many instances' streams leave the device (0 = all)
  uint64_t next_call = 0;                   // streaming slices: the call the next slice must start with
  bool unchecked_slices = false;            // benchmarks may garble slices out of order (results are then meaningless)
  const Program& prog() const { return plan ? ps.L.facade : p->variant(ni); }
  const Program& call_prog(size_t k) const { return plan->calls[k].prog->variant(ni); }
  uint32_t first_input_slot() const { return plan ? ps.L.global_base : SLOT_FIRST_INPUT; }
  bool ran = false, last_eval = false, garbled = false;
  std::vector<uint64_t> ct_uploaded;  // per instance: records supplied by gsv_session_upload_ciphertexts
  std::unique_ptr<gsv_drain> drain;    // streaming drain: copy streams, pinned buffers, per-instance MAC states (created on first use)
  PassCommit pass_commit = PassCommit::None;  // what the pass in progress carries, as its first slice asked (drain_pipeline.hpp: commit_slice_conflict)
  std::unique_ptr<B3Stream> b3;        // BLAKE3 commitments of the drained streams: device buffers and per-instance hashers, beside drain->macs (engine_blake3.ipp)
  std::unique_ptr<MacCheckStream> mac_check;  // the CBC-MAC check of a garbling pass against checkpoint files (engine_cbcmac.ipp): device buffers, carries, position — beside `b3`, chained from slice to slice
  uint32_t mck_k = 0;                  // log2 of the group size of the checkpoint files the pass in progress writes (GSV_MAC_GROUP_LOG2 when its first slice began)
  std::unique_ptr<B3Stream> b3_eval;   // ... of the streams a streaming evaluation reads (gsv_session_evaluate_streaming*_commit): apart from `b3`, which a garbling pass chains from slice to slice
  std::unique_ptr<MacCheckStream> mac_eval;  // ... and the CBC-MAC check of the streams a streaming evaluation reads, against checkpoints (gsv_session_evaluate_streaming_mac_calls): apart from `mac_check`, as b3_eval from b3
  std::unique_ptr<EvalCarry> evs;      // a streaming evaluation in slices: next call, MAC states, outboards, restart points (engine_blake3.ipp; created on first use)
  // verified streaming evaluation (gsv_session_evaluate_streaming_verified): where the last such pass found a stream that differs from its outboard
  bool mismatch = false;
  uint64_t mismatch_instance = 0, mismatch_group = 0, mismatch_record = 0;
  uint64_t windows_launched = 0;       // plan sessions: windows the last pass launched (gsv_session_windows_launched)
  std::vector<DevBuf> ct_gate_more;    // further gate-order buffers of the drain pipeline (ct_gate is the first)
  DevBuf ct_alt;                       // garble -> evaluate on the device: the second program-order ciphertext block
  std::unique_ptr<PairState> pair;     // ... and its stream / events (created on first use)
  gsv_session();   // (both in engine_drain.ipp, where PairState, B3Stream and EvalCarry are complete)
  ~gsv_session();  // selects the device and synchronises the engine's stream; the members then release what they hold
  uint64_t ct_stride() const { return plan ? (retain() ? plan->n_ct : max_block()) : ct_cap * p->prog.n_ct; }  // n_ct does not depend on the variant
};
// The one place a verified pass (evaluated against outboards, or garbled against checkpoint files) reports a differing stream at:
// what gsv_session_mismatch_info reads.  group = record = ~0: the difference has no place in the stream (a commitment before the pass).
static inline void set_mismatch(gsv_session* s, uint64_t instance, uint64_t group, uint64_t record) { s->mismatch = true; s->mismatch_instance = instance; s->mismatch_group = group; s->mismatch_record = record; }
static inline void clear_mismatch(gsv_session* s) { s->mismatch = false; }
// what stage_labels, launch and the streaming passes ask first: a session left without a schedule (gsv_session::unusable) refuses
static inline int plan_session_usable(const gsv_session* s) { return s->unusable.empty() ? GSV_OK : fail(GSV_ERR_DEVICE, s->unusable); }
// records of one instance's whole ciphertext stream: what a streaming pass drains or reads, and what a commitment covers
static inline uint64_t stream_records(const gsv_session* s) { return s->plan ? s->plan->n_ct : s->replays * s->prog().n_ct; }
PassGuard::PassGuard(gsv_session* s) { if (s) s->pass = knobs::Pass(); ReleaseGate& g = release_gate(); std::lock_guard<std::recursive_mutex> lk(g.mu); ++g.active; }

// Failure paths release whatever was allocated so far through the public destroy functions (a failed hipMalloc on a
// multi-GB session must not leave the GPU full).
struct SessionDeleter { void operator()(gsv_session* s) const { gsv_session_destroy(s); } };
struct EngineDeleter { void operator()(gsv_engine* e) const { gsv_engine_destroy(e); } };
typedef std::unique_ptr<gsv_session, SessionDeleter> SessionPtr;
typedef std::unique_ptr<gsv_engine, EngineDeleter> EnginePtr;
