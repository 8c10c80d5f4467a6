// CBC-MAC commitments VERIFIED on the device against chain checkpoints (part of kernels.hip; DESIGN.md §3 "Commitment stage",
// include/gsv_engine.h "CBC-MAC checkpoints").
//
// commit_i = h_L with h_j = AES_K(h_{j-1} ^ ct_j), h_0 = 0 (the reference's AESAccumulatingHash): one serial chain per stream, which
// cannot be COMPUTED in parallel.  With the chain state after every 2^k records (mac_checkpoints.hpp: the checkpoint file gc_<i>.mck) it
// can be CHECKED in parallel: group g is one chain of its own that starts from the CLAIMED state g - 1, runs the group's records and must
// arrive at the claimed state g.  If every group holds, state -1 is zero and the last state is the commitment, the stream's true CBC-MAC
// is the commitment, by induction over the groups; the checkpoints themselves need no trust.
//
// A stream reaches the kernel in SEGMENTS of a gate-order buffer ([instance][record], as blake3_device.hpp).  One chain per lane: chain
// c of an instance covers the part of group (first >> k) + c that lies inside the segment.  A group that a segment boundary cuts is
// carried: the chain writes its state to the instance's 16-byte carry and chain 0 of the next segment goes on from it (two carry
// buffers, ping-pong: the lane that reads a carry and the lane that writes one are different lanes of one launch).
//
// The first part of this file — which state a chain starts from, where it ends, what it compares — is plain C++ over a table accessor
// (gate_math.hpp), so the same code runs on the host with PlainTables (tests/mac_checkpoints); the kernel and its launcher follow.
#pragma once
#include "gate_math.hpp"

namespace gsv {
namespace dev {

// Chain c of a segment: records [first, first + n) of a stream of `total` records, groups of 2^k records.
struct MacChain {
  uint64_t group;      // the group the chain belongs to
  uint64_t lo, hi;     // its records, as offsets into the segment: [lo, hi), never empty
  uint32_t start;      // where it starts from: MAC_FROM_ZERO / MAC_FROM_CARRY / MAC_FROM_STATE (the claimed state group - 1)
  bool ends_group;     // it reaches the end of its group (or of the stream): compare with the claimed state `group`; else: write the carry
};
enum : uint32_t { MAC_FROM_ZERO = 0, MAC_FROM_CARRY = 1, MAC_FROM_STATE = 2 };

// chains of a segment (n > 0): one per group the segment touches
GSV_HD uint64_t mac_chain_count(uint64_t first, uint64_t n, uint32_t k) { return ((first + n - 1) >> k) - (first >> k) + 1; }
// states the segment touches: (first >> k) - 1 .. (first + n - 1) >> k, i.e. mac_chain_count + 1 of them; slice index of state s:
GSV_HD uint64_t mac_slice_index(uint64_t first, uint32_t k, uint64_t state) { return state + 1 - (first >> k); }

GSV_HD MacChain mac_chain(uint64_t first, uint64_t n, uint32_t k, uint64_t total, uint64_t c) {
  MacChain m;
  m.group = (first >> k) + c;
  const uint64_t g_lo = m.group << k, g_end = (m.group + 1) << k;
  const uint64_t g_hi = g_end < total ? g_end : total;
  const uint64_t lo = g_lo > first ? g_lo : first, hi = g_hi < first + n ? g_hi : first + n;
  m.lo = lo - first; m.hi = hi - first;
  m.start = lo != g_lo ? MAC_FROM_CARRY : m.group == 0 ? MAC_FROM_ZERO : MAC_FROM_STATE;
  m.ends_group = hi == g_hi;
  return m;
}

// One chain, run: `rec(q)` is record q of the segment, `slice` the claimed states the segment touches (mac_slice_index; entry 0 is not
// read when the segment starts in group 0), `carry_in` / `carry_out` the instance's carries.  While one block is encrypted the next
// record's load is already in flight.  Returns true when the chain ended its group at a state that DIFFERS from the claimed one.
template <class Tab, class Rec>
GSV_HD bool mac_chain_run(const Tab& T, const MacChain& m, uint64_t first, uint32_t k, Rec rec, const Label* slice, const Label* carry_in, Label* carry_out) {
  Label st{{0, 0, 0, 0}};
  if (m.start == MAC_FROM_CARRY) st = *carry_in;
  else if (m.start == MAC_FROM_STATE) st = slice[mac_slice_index(first, k, m.group - 1)];
  Label nxt = rec(m.lo);
  for (uint64_t q = m.lo; q < m.hi; ++q) {
    const Label cur = nxt;
    if (q + 1 < m.hi) nxt = rec(q + 1);
    st = aes128_encrypt(T, lxor(st, cur));
  }
  if (!m.ends_group) { *carry_out = st; return false; }
  const Label want = slice[mac_slice_index(first, k, m.group)];
  return ((st.w[0] ^ want.w[0]) | (st.w[1] ^ want.w[1]) | (st.w[2] ^ want.w[2]) | (st.w[3] ^ want.w[3])) != 0;
}

// A stream that is RESIDENT in program order (gsv_session_ciphertext_cbcmac_check) is checked where it lies: record q of a block's
// gate-order stream is block[(q / n_ct) * n_ct + ct_pos[q % n_ct]] (kernel_api.h, gsvk_b3_chunks_indexed: n_ct records per replay, ct_pos
// the position table).  A chain asks for ascending q, so the replay it stands in is kept and the division is taken only where a
// request leaves it by more than one replay; any order of requests gives the same positions.
struct MacIndexedPos {
  const uint32_t* ct_pos;
  uint64_t n_ct, rep_base = 0;  // rep_base: first record of the replay the last request lay in
  GSV_HD MacIndexedPos(const uint32_t* ct_pos_, uint64_t n_ct_) : ct_pos(ct_pos_), n_ct(n_ct_) {}
  GSV_HD uint64_t at(uint64_t q) {
    if (q - rep_base >= n_ct) rep_base = q - rep_base - n_ct < n_ct ? rep_base + n_ct : (q / n_ct) * n_ct;
    return rep_base + ct_pos[q - rep_base];
  }
};

}  // namespace dev
}  // namespace gsv

#if defined(__HIPCC__)
namespace gsv {
namespace dev {

#define GSV_MAC_BLOCK_THREADS 256u  // two workgroups of 64 KiB tables fit a CU's 160 KiB

// grid = (ceil(n_chains / 256), instances), 256 threads, GSV_LDS_TABLE_BYTES of dynamic LDS from LDS address 0 (no static LDS).
//   seg[inst * seg_stride + q]        record q < n of the segment; `first` is the stream position of record 0, the same for all instances
//   slice[inst * slice_stride + j]    claimed state (first >> k) - 1 + j, j <= n_chains (slice_stride >= n_chains + 1)
//   carry_in / carry_out [inst]       16 bytes each
//   bad[inst]                         the lowest group of the instance whose chain did not arrive at its claimed state (all ones: none)
// Read pattern: neighbouring lanes read 2^k x 16 bytes apart, 16 bytes per trip, PLAIN loads — a lane comes back for the other seven
// records of a 128-byte line in its next trips, so the line should stay in L2 / the CU's L1 meanwhile (a non-temporal load would fetch it
// eight times).  Round keys: through the scalar cache (LdsBankedTable::rk, c_rk), 44 SGPRs live across the chain loop; LDS holds the
// bank-replicated Te0 / Te2 only.
template <class Rec>
__device__ __forceinline__ void mac_check_lane(const uint32_t* te, Rec rec, uint64_t first, uint64_t n, uint32_t k, uint64_t total, const uint4* slice_, uint64_t slice_stride, const uint4* carry_in_,
                                               uint4* carry_out_, unsigned long long* bad) {
  extern __shared__ __attribute__((aligned(16))) char s_mac_mem[];
  (void)s_mac_mem;  // the dynamic LDS block starts at LDS address 0
  // this kernel's own copy of the table fill of run_program_kernel: dword i of the table region, entry x = i / 64; first 32 dwords Te0[x], next 32 Te2[x]
  for (uint32_t i = threadIdx.x; i < GSV_LDS_TABLE_BYTES / 4; i += GSV_MAC_BLOCK_THREADS) *reinterpret_cast<lds_u32*>(uintptr_t(i * 4u)) = te[((i & 32u) ? 512u : 0u) + (i >> 6)];
  __syncthreads();
  const uint64_t c = uint64_t(blockIdx.x) * GSV_MAC_BLOCK_THREADS + threadIdx.x;
  if (c >= mac_chain_count(first, n, k)) return;
  const uint32_t inst = blockIdx.y;
  const LdsBankedTable aes{(threadIdx.x & 31u) * 4u, (cst_u32*)c_rk};
  const MacChain m = mac_chain(first, n, k, total, c);
  const Label* slice = reinterpret_cast<const Label*>(slice_ + uint64_t(inst) * slice_stride);
  const bool differs = mac_chain_run(aes, m, first, k, rec, slice, reinterpret_cast<const Label*>(carry_in_ + inst), reinterpret_cast<Label*>(carry_out_ + inst));
  if (differs) __hip_atomic_fetch_min(bad + inst, (unsigned long long)m.group, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ __launch_bounds__(GSV_MAC_BLOCK_THREADS) void cbcmac_check_kernel(const uint32_t* te, const uint4* seg_, uint64_t seg_stride, uint64_t first, uint64_t n, uint32_t k, uint64_t total,
                                                                              const uint4* slice_, uint64_t slice_stride, const uint4* carry_in_, uint4* carry_out_, unsigned long long* bad) {
  const glb_u128* seg = (const glb_u128*)(seg_) + uint64_t(blockIdx.y) * seg_stride;
  mac_check_lane(te, [seg](uint64_t q) { const u32x4 v = seg[q]; return Label{{v.x, v.y, v.z, v.w}}; }, first, n, k, total, slice_, slice_stride, carry_in_, carry_out_, bad);
}
// The same with the segment read where a resident stream lies: record q of the segment is record block_first + q of the gate-order stream
// of block[inst] (MacIndexedPos; block_stride in records), which is only read.  Read pattern: a lane walks 2^k gate positions of its
// group, at the scattered program-order addresses the position table names — a permutation of 16-byte records; plain loads, as above.
__global__ __launch_bounds__(GSV_MAC_BLOCK_THREADS) void cbcmac_check_indexed_kernel(const uint32_t* te, const uint4* block_, uint64_t block_stride, const uint32_t* ct_pos, uint64_t n_ct, uint64_t block_first,
                                                                                      uint64_t first, uint64_t n, uint32_t k, uint64_t total, const uint4* slice_, uint64_t slice_stride,
                                                                                      const uint4* carry_in_, uint4* carry_out_, unsigned long long* bad) {
  const glb_u128* block = (const glb_u128*)(block_) + uint64_t(blockIdx.y) * block_stride;
  MacIndexedPos pos(ct_pos, n_ct);
  mac_check_lane(te, [block, block_first, pos](uint64_t q) mutable { const u32x4 v = block[pos.at(block_first + q)]; return Label{{v.x, v.y, v.z, v.w}}; }, first, n, k, total, slice_, slice_stride,
                 carry_in_, carry_out_, bad);
}

}  // namespace dev
}  // namespace gsv

namespace gsv {
namespace dev {
// once per device and kernel: the tables are addressed from LDS byte 0, so there must be no static LDS in front of the dynamic block
inline int mac_kernel_ready(const void* kf, std::set<int>& done) {
  static std::mutex attr_mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return int(hipErrorInvalidDevice);
  std::lock_guard<std::mutex> lk(attr_mu);
  if (done.count(dev)) return 0;
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, kf) != hipSuccess || fa.sharedSizeBytes != 0) return int(hipErrorInvalidValue);
  const hipError_t e0 = hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, int(GSV_LDS_TABLE_BYTES));
  if (e0 != hipSuccess) return int(e0);
  done.insert(dev);
  return 0;
}
// what both launchers ask of a segment and its slice; *blocks = grid.x
inline bool mac_launch_shape(uint64_t first, uint64_t n, uint32_t k, uint64_t total, uint64_t slice_stride, uint32_t n_instances, uint32_t* blocks) {
  if (n_instances == 0 || n_instances > 65535u || k > 30u || first + n < first || first + n > total) return false;
  if (n == 0) { *blocks = 0; return true; }
  const uint64_t chains = mac_chain_count(first, n, k);
  if (chains + 1 > slice_stride || (chains + GSV_MAC_BLOCK_THREADS - 1) / GSV_MAC_BLOCK_THREADS > 0x7fffffffull) return false;
  *blocks = uint32_t((chains + GSV_MAC_BLOCK_THREADS - 1) / GSV_MAC_BLOCK_THREADS);
  return true;
}
}  // namespace dev
}  // namespace gsv

extern "C" {
// One segment of n_instances streams against its slice of claimed states (cbcmac_check_kernel).  n == 0: nothing is launched.
int gsvk_cbcmac_check(const void* te, const void* seg, uint64_t seg_stride, uint64_t first, uint64_t n, uint32_t k, uint64_t total, const void* slice, uint64_t slice_stride,
                      const void* carry_in, void* carry_out, void* bad, uint32_t n_instances, hipStream_t s) {
  uint32_t blocks = 0;
  if (!gsv::dev::mac_launch_shape(first, n, k, total, slice_stride, n_instances, &blocks) || n > seg_stride) return int(hipErrorInvalidValue);
  if (n == 0) return 0;
  static std::set<int> attr_done;
  if (const int rc = gsv::dev::mac_kernel_ready(reinterpret_cast<const void*>(gsv::dev::cbcmac_check_kernel), attr_done)) return rc;
  hipLaunchKernelGGL(gsv::dev::cbcmac_check_kernel, dim3(blocks, n_instances), dim3(GSV_MAC_BLOCK_THREADS), GSV_LDS_TABLE_BYTES, s,
                     static_cast<const uint32_t*>(te), static_cast<const uint4*>(seg), seg_stride, first, n, k, total, static_cast<const uint4*>(slice), slice_stride,
                     static_cast<const uint4*>(carry_in), static_cast<uint4*>(carry_out), static_cast<unsigned long long*>(bad));
  return int(hipGetLastError());
}
// ... of streams that lie in program order (cbcmac_check_indexed_kernel): the segment is records [block_first, block_first + n) of the
// gate-order stream of a block of block_records records, whole replays of n_ct records, inside block_stride.  What is checked here is
// the segment against the block and the block against its stride; that block + n_instances x block_stride lies inside the caller's
// buffer (a plan session passes CT + the call's offset with the stream's full stride) and that ct_pos holds n_ct positions below n_ct
// rests on the caller: the session's own tables.
int gsvk_cbcmac_check_indexed(const void* te, const void* block, uint64_t block_stride, const void* ct_pos, uint64_t n_ct, uint64_t block_records, uint64_t block_first, uint64_t first, uint64_t n,
                              uint32_t k, uint64_t total, const void* slice, uint64_t slice_stride, const void* carry_in, void* carry_out, void* bad, uint32_t n_instances, hipStream_t s) {
  uint32_t blocks = 0;
  if (!gsv::dev::mac_launch_shape(first, n, k, total, slice_stride, n_instances, &blocks)) return int(hipErrorInvalidValue);
  if (n_ct == 0 || block_records % n_ct != 0 || block_records > block_stride || block_first + n < block_first || block_first + n > block_records) return int(hipErrorInvalidValue);
  if (n == 0) return 0;
  static std::set<int> attr_done;
  if (const int rc = gsv::dev::mac_kernel_ready(reinterpret_cast<const void*>(gsv::dev::cbcmac_check_indexed_kernel), attr_done)) return rc;
  hipLaunchKernelGGL(gsv::dev::cbcmac_check_indexed_kernel, dim3(blocks, n_instances), dim3(GSV_MAC_BLOCK_THREADS), GSV_LDS_TABLE_BYTES, s,
                     static_cast<const uint32_t*>(te), static_cast<const uint4*>(block), block_stride, static_cast<const uint32_t*>(ct_pos), n_ct, block_first, first, n, k, total,
                     static_cast<const uint4*>(slice), slice_stride, static_cast<const uint4*>(carry_in), static_cast<uint4*>(carry_out), static_cast<unsigned long long*>(bad));
  return int(hipGetLastError());
}
}  // extern "C"
#endif
