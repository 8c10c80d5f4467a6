// The engine's tuning knobs: the ONE place that reads the process environment (besides the process-lifetime statics for GSV_NO_VAES,
// host_crypto.hpp, and GSV_EXP_CHUNK, gadgets/bn254_groth16.hpp).
//
// Rule: a knob is read on the thread that entered the C ABI, at the top of the public entry point that uses it — before any worker
// thread is started and outside any loop — and travels as data from there.  Never on compile-pool, warm-up-recorder, drain-worker or
// second-walker threads, never per launch, never in a polling loop.  The structs below READ THEIR KNOBS WHEN THEY ARE CONSTRUCTED: an
// entry point declares one (`const knobs::PlanBuild kn;`) or assigns a fresh one (`s->pass = knobs::Pass();`, PassGuard) and hands it on.
//
// knob                        type     default              read by                                what it affects
// -- compile knobs: knobs::compile_options(scope) -> CompileOptions (program.hpp); kept in ProgramSource::opt for variants compiled later
// GSV_FUSE                    flag     1                    program + plan scope                   fold free gates into their readers
// GSV_AND_CAP / GSV_XOR_CAP   int      0 (no cap)           program + plan scope                   most AND-family / free gates per step
// GSV_LDS_SLOTS_CAP           int      none                 program + plan scope                   upper bound on the LDS window a program may use
// GSV_AND_TERMS               0|2|4    0 (choose)           program + plan scope                   wires per AND input (record form)
// GSV_SCHED_STATS             set?     unset                program + plan scope                   print wire-file coalescing statistics per program
// GSV_LDS_LIFETIME            int      1024                 program scope                          steps a wire may live in the LDS window
// GSV_FUSE_DUP                int      2                    program scope                          readers up to which a small free gate is recomputed
// GSV_ORDER_BY_READER         flag     1                    program scope                          gate order inside a step
// GSV_HBM_ARENA               int      4                    program scope                          HBM wire file = factor x peak live wires
// GSV_LDS_SLOTS               int      LDS_WINDOW_SLOTS     program scope                          LDS window of the program (0 = every wire in HBM)
//    program scope: gsv_program_compile*, hostsim_compile.  plan scope: gsv_plan_from_circuit*, gsv_plan_build_file*,
//    gsv_plan_recorder_finish, hostsim_plan_build.
// -- plan-build knobs: a knobs::PlanBuild at gsv_plan_from_circuit*, gsv_plan_build_file*, gsv_plan_recorder_finish
// GSV_COMPILE_THREADS         int      hardware, <= 16      + gsv_program_compile* (first background compile creates the pool),
//                                                             gsv_session_create_plan* (window variants)  compile workers
// GSV_PLAN_WARMUP_THREADS     int      compile threads / 4  plan build                             warm-up recorders beside the driver (0 = none)
// GSV_PLAN_ID_SLACK           int      262144               plan build                             reuse distance of recycled global wire ids
// GSV_PLAN_DEBUG              set?     unset                plan build, schedule, pass             progress and per-program statistics on stderr
// GSV_PLAN_WINDOW_DIV         1|2|4    1                    gsv_plan_from_circuit*, _build_file*   one image per program for 1/div of the LDS window;
// GSV_PLAN_HALF_WINDOW        flag     0                      (only when window_div is passed as 0)  older spelling of GSV_PLAN_WINDOW_DIV=2
// -- session knobs: the knobs::Session a session is created with (gsv_session_create, gsv_session_create_plan*)
// GSV_INSTANCES_PER_WG        1|2|4    by instance count    session creation                       instances per workgroup
// GSV_SIDE_STREAM_PRIORITY    0?       on                   session creation                       side streams ask for the highest stream priority (off: a value that begins with 0)
// -- schedule knobs: a knobs::Sched when a plan session's schedule is installed (creation, safe-schedule fallback);
//    a non-zero gsv_plan_session_opts field wins over its knob
// GSV_PLAN_CONCURRENCY        int      CUs / workgroups     (opts.max_concurrent_calls)            calls side by side
// GSV_DRAIN_SEGMENT_RECORDS   int      by free memory       (opts.drain_segment_records)           records per drain segment
// GSV_CT_RING                 =1?      off                  (opts.retain_stream == 0)              ciphertext ring instead of a window block
// GSV_CT_RING_RECORDS         int      3 segments           ring sessions                          ring size (tests: small rings)
// GSV_VERIFY_SCHEDULE         set?     unset                also set by GSV_PLAN_DEBUG             full hazard check of the schedule
// GSV_FAULT_WITHHOLD_DEP      =1?      off                  never for the safe schedule            tests: a dependency that never completes
// -- pass knobs: a knobs::Pass at the top of every gsv_session_garble* / gsv_session_evaluate* entry point, kept in the session
//    for that pass only
// GSV_DEP_WAIT_SECONDS        seconds  60, <= 86400         pass                                   device dependency watchdog and the host's deadline
// GSV_DIAG                    int      0                    pass                                   KernelArgs::diag (diagnostic library only)
// GSV_DRAIN_DEBUG             set?     unset                pass                                   drain progress on stderr
// GSV_DRAIN_STATS             set?     unset                pass                                   where the drain's host thread waited
// GSV_DRAIN_GROUP             1|4|16   by cores / VAES      pass                                   MAC chains per drain worker
// GSV_DRAIN_CHUNK_MB          int      16                   pass                                   page-locked chunk buffers of the drain
// GSV_DRAIN_COPIES            int      3                    pass                                   copy streams of the drain
// GSV_DRAIN_DEPTH             int      by free memory       pass                                   gate-order buffers of the drain pipeline
// GSV_PAIR_CU_MASK            flag     1                    pass                                   CU-masked streams for garble || evaluate pairs
// GSV_B3_SUBTREE_LOG2         0..20    10                   pass, gsv_engine_blake3_streams,       BLAKE3 commitments: log2 of the chunks the device reduces to one value (anything else: the call is refused)
//                                                             gsv_session_ciphertext_blake3
// GSV_MAC_GROUP_LOG2          0..30    8                    every entry point that writes          CBC-MAC checkpoints: log2 of the records between two chain states, where the caller passes
//                                                             checkpoint files                       GSV_MAC_GROUP_DEFAULT (a reader takes k from the file).  Measured (tools/mac_check_rate.py):
//                                                                                                    the largest k of 8 .. 16 whose check rate over 1 GiB segments of 256 streams is within 10 % of the best
// -- a knobs::ResidentB3 at gsv_session_ciphertext_blake3 (with GSV_B3_SUBTREE_LOG2)
// GSV_B3_RESIDENT_RECORDS     int      by free memory       gsv_session_ciphertext_blake3          most records per instance one launch range of the resident hash covers
//                                                                                                    (default: the two chunk-value buffers take <= 1/10 of the free memory, <= 64 M records)
// -- a knobs::ResidentMac at gsv_session_ciphertext_cbcmac_check (k comes from the checkpoint files)
// GSV_MAC_RESIDENT_RECORDS    int      by free memory       gsv_session_ciphertext_cbcmac_check    most records per instance one launch range of the resident check covers
//                                                                                                    (default: the slices of claimed states take <= 1/10 of the free memory, <= 64 M records)
#pragma once
#include <algorithm>  // (with <initializer_list>)
#include <cstdlib>
#include <thread>
#include "program.hpp"

namespace gsv::knobs {
inline bool is_set(const char* name) { return getenv(name) != nullptr; }
inline bool read_int(const char* name, long long* v) { const char* e = getenv(name); if (e) *v = atoll(e); return e != nullptr; }
inline long long int_or(const char* name, long long dflt) { (void)read_int(name, &dflt); return dflt; }
inline bool flag(const char* name, bool dflt) { return int_or(name, dflt) != 0; }
inline unsigned long long at_least_1(const char* name) { long long v; return read_int(name, &v) ? std::max(1ll, v) : 0; }  // 0 = not set
inline long long one_of(const char* name, std::initializer_list<long long> ok, long long dflt, long long bad) { long long v; return !read_int(name, &v) ? dflt : std::find(ok.begin(), ok.end(), v) != ok.end() ? v : bad; }  // not set: dflt; set to something not in `ok`: bad
inline double positive_seconds(const char* name, double dflt, double most) { const char* e = getenv(name); char* end = nullptr; const double v = e ? std::strtod(e, &end) : 0.0; return e && end != e && v > 0 ? std::min(v, most) : dflt; }
enum class Scope { Program, Plan };
inline CompileOptions compile_options(Scope scope) {
  CompileOptions o; long long v;
  o.fuse = flag("GSV_FUSE", o.fuse);
  if (scope == Scope::Program) {
    o.lds_max_lifetime = uint32_t(int_or("GSV_LDS_LIFETIME", o.lds_max_lifetime)); o.fuse_dup_fanout = uint32_t(int_or("GSV_FUSE_DUP", o.fuse_dup_fanout));
    o.order_by_reader = flag("GSV_ORDER_BY_READER", o.order_by_reader); o.hbm_arena_factor = uint32_t(int_or("GSV_HBM_ARENA", o.hbm_arena_factor));
    if (read_int("GSV_LDS_SLOTS", &v)) o.lds_slots = std::min<uint32_t>(uint32_t(v), LDS_WINDOW_SLOTS);
  }
  o.and_cap = uint32_t(int_or("GSV_AND_CAP", o.and_cap)); o.xor_cap = uint32_t(int_or("GSV_XOR_CAP", o.xor_cap));
  if (read_int("GSV_LDS_SLOTS_CAP", &v)) o.lds_slots = std::min<uint32_t>(o.lds_slots, uint32_t(v));  // experiments: more instances per workgroup
  o.and_terms = uint32_t(one_of("GSV_AND_TERMS", {0, 2, 4}, o.and_terms, o.and_terms)); o.sched_stats = is_set("GSV_SCHED_STATS");
  return o;
}
inline size_t compile_threads() { return size_t(std::min(16ll, std::max(1ll, int_or("GSV_COMPILE_THREADS", (long long)std::thread::hardware_concurrency())))); }
inline size_t plan_id_slack() {
  const char* e = getenv("GSV_PLAN_ID_SLACK"); char* end = nullptr; const long long v = e ? std::strtoll(e, &end, 10) : 262144;
  if (e && (end == e || *end != 0 || v < 0 || v > (1ll << 28))) gsv_panic("GSV_PLAN_ID_SLACK must be an integer in [0, 2^28]");
  return size_t(v);
}
inline uint32_t b3_subtree_log2() {
  const char* e = getenv("GSV_B3_SUBTREE_LOG2"); char* end = nullptr; const long long v = e ? std::strtoll(e, &end, 10) : 10;
  return e && (end == e || *end != 0 || v < 0 || v > 20) ? ~0u : uint32_t(v);  // ~0u = set to something else: the entry point that needs it refuses (like window_div)
}
inline uint32_t mac_group_log2() {
  const char* e = getenv("GSV_MAC_GROUP_LOG2"); char* end = nullptr; const long long v = e ? std::strtoll(e, &end, 10) : 8;
  return e && (end == e || *end != 0 || v < 0 || v > 30) ? ~0u : uint32_t(v);  // ~0u = set to something else: the entry point that needs it refuses
}
struct PlanBuild {
  CompileOptions opt = compile_options(Scope::Plan);
  size_t compile_threads = knobs::compile_threads();
  size_t warmup_threads = size_t(std::max(0ll, int_or("GSV_PLAN_WARMUP_THREADS", (long long)std::max<size_t>(1, compile_threads / 4))));
  size_t id_slack = plan_id_slack();
  bool debug = is_set("GSV_PLAN_DEBUG");
  uint32_t window_div = uint32_t(one_of("GSV_PLAN_WINDOW_DIV", {1, 2, 4}, flag("GSV_PLAN_HALF_WINDOW", false) ? 2 : 1, 0));  // 0 = GSV_PLAN_WINDOW_DIV holds something else
};
struct Session {
  uint32_t instances_per_wg = uint32_t(one_of("GSV_INSTANCES_PER_WG", {1, 2, 4}, 0, 0));  // 0 = by instance count
  bool side_stream_priority = !(getenv("GSV_SIDE_STREAM_PRIORITY") && getenv("GSV_SIDE_STREAM_PRIORITY")[0] == '0');  // off only by a value that begins with 0
};
struct Sched {  // 0 = not set
  uint32_t plan_concurrency = uint32_t(at_least_1("GSV_PLAN_CONCURRENCY"));
  uint64_t drain_segment_records = at_least_1("GSV_DRAIN_SEGMENT_RECORDS"), ct_ring_records = at_least_1("GSV_CT_RING_RECORDS");
  bool ct_ring = int_or("GSV_CT_RING", 0) == 1, fault_withhold_dep = int_or("GSV_FAULT_WITHHOLD_DEP", 0) == 1, verify = is_set("GSV_PLAN_DEBUG") || is_set("GSV_VERIFY_SCHEDULE");
};
struct Pass {
  double dep_wait_seconds = positive_seconds("GSV_DEP_WAIT_SECONDS", 60.0, 86400.0);
  uint32_t diag = uint32_t(int_or("GSV_DIAG", 0));  // timing experiments (libgsv_engine_diag.so only): outputs are wrong when set
  bool drain_debug = is_set("GSV_DRAIN_DEBUG"), plan_debug = is_set("GSV_PLAN_DEBUG"), drain_stats = is_set("GSV_DRAIN_STATS"), pair_cu_mask = flag("GSV_PAIR_CU_MASK", true);
  int drain_group = int(one_of("GSV_DRAIN_GROUP", {1, 4, 16}, 0, 0)), drain_copies = int(std::max(1ll, int_or("GSV_DRAIN_COPIES", 3)));  // group 0 = by cores / VAES
  uint64_t drain_chunk_mb = uint64_t(std::max(1ll, int_or("GSV_DRAIN_CHUNK_MB", 16)));
  size_t drain_depth = size_t(at_least_1("GSV_DRAIN_DEPTH"));  // 0 = by free memory
  uint32_t b3_subtree_log2 = knobs::b3_subtree_log2();
  uint32_t mac_group_log2 = knobs::mac_group_log2();
};
struct ResidentB3 {
  uint32_t b3_subtree_log2 = knobs::b3_subtree_log2();
  uint64_t resident_records = at_least_1("GSV_B3_RESIDENT_RECORDS");  // 0 = by free memory
};
struct ResidentMac {
  uint64_t resident_records = at_least_1("GSV_MAC_RESIDENT_RECORDS");  // 0 = by free memory
};
}  // namespace gsv::knobs
