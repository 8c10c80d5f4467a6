// Host runtime + C ABI (include/gsv_engine.h) of the MI355X garbling engine: ONE translation unit: this file, the ten parts it includes and the headers they share.
// Device memory, streams and events are plain HIP runtime calls behind the owners of hip_owned.hpp; there is NO CPU execution path for
// garble/evaluate — without a HIP device gsv_engine_create fails with GSV_ERR_DEVICE.
//   hip_owned.hpp             move-only owners of device buffers, page-locked host buffers, streams and events: the only release calls
//   drain_pipeline.hpp        host side of the streaming drain, no session in sight: where a stream goes and what may be combined (DrainSink, PassCommit), gc files, MAC / copy workers, BLAKE3 absorbers (tests/drain_pipeline)
//   upload_pipeline.hpp       host side of the streaming evaluator, no session in sight: staging buffers, H2D copies, MAC pool, the gc file source (tests/upload_pipeline)
//   outboard.hpp              BLAKE3 outboards, host code only: format, host writer, loaders, and B3Check — what a receiver's streams are compared with (tests/drain_pipeline)
//   mac_checkpoints.hpp       CBC-MAC checkpoint files, host code only: format, host writer, host checker (tests/mac_checkpoints)
//   plan_layout.hpp           what a plan session derives from its schedule, host values only: the parameter policy (plan_sched_params) and the tables of the window launches (PlanLayout, build_plan_layout) (tests/plan_layout, tests/hostsim)
//   engine_internal.hpp       error reporting, device allocation, the deferred-release gate, the objects behind the opaque handles
//   engine_abi_record.ipp     gsv_recorder_*, gsv_program_*, gsv_engine_*, gsv_labels_from_seed
//   engine_session.ipp        program sessions
//   engine_plan.ipp           gsv_plan_*: built-in builder (single / dual), plan files, background compilation, plan recorder
//   engine_plan_session.ipp   plan sessions: schedule + device tables, inputs, window launches
//   engine_blake3.ipp         BLAKE3 commitments: gsv_blake3_*, the device tree hash of segmented streams, B3Receiver: its one single-threaded consumer; FilesOnDevice / StreamsOnDevice: the loops that bring n equally long streams to the device, for this part and the next
//   engine_cbcmac.ipp         CBC-MAC commitments verified against chain checkpoints (mac_checkpoints.hpp): gsv_cbcmac_file_*, MacCheckReceiver, the device check of segmented streams and of files, the check's half of a restart point
//   engine_garble_commit.ipp  GarbleCommit: the commitments of one slice of a streaming garbling pass (BLAKE3 state and absorbers, outboards, checkpoint files, the check on the device)
//   engine_drain.ipp          streaming garbler: the device side of the drain (plan windows, program rings), garble || evaluate, safe-schedule fallback
//   engine_evaluate.ipp       evaluation: the resident stream, streaming sources (plan ring, plan windows, program rings), unverified or verified against BLAKE3 outboards or CBC-MAC checkpoints
//   engine_readback.ipp       read-back, step clock and step statistics, commitments to the resident stream, CBC-MAC helpers
// (The parts share file-local helpers and are included in this order inside one extern "C" block; build.py's dependency scan covers them.)
#include "engine_internal.hpp"

extern "C" {

#include "engine_abi_record.ipp"
#include "engine_session.ipp"
#include "engine_plan.ipp"
#include "engine_plan_session.ipp"
#include "engine_blake3.ipp"
#include "engine_cbcmac.ipp"
#include "engine_garble_commit.ipp"
#include "engine_drain.ipp"
#include "engine_evaluate.ipp"
#include "engine_readback.ipp"

}  // extern "C"
