// BLAKE3 tree hash of the ciphertext streams, on the device (part of kernels.hip; DESIGN.md §3 "Commitment stage").
//
// commit_i = BLAKE3(stream_i), plain hash mode.  A stream reaches these kernels in SEGMENTS of a gate-order buffer (what
// gather_segment_kernel / the plan gathers write: [instance][record], 16 bytes a record, 64 records a chunk).  The device computes
//   * the chaining value of every 1 KiB chunk but the stream's LAST one (chunk_kernel: one lane per chunk, CHUNK_START / CHUNK_END
//     only, the 64-bit counter is the chunk's index in the instance's whole stream), and
//   * for aligned groups of G = 2^k consecutive chunks that end before the last chunk, the ONE parent value of the group
//     (parent_kernel, one launch per tree level, flag PARENT; compact_kernel moves the group values out).
// ROOT is never applied here: the last chunk, and with it the decision what the root node is, belongs to the host (host_crypto.hpp,
// Blake3Host), which receives 32 bytes per group, the few chunk values behind the last complete group, and the last chunk's bytes.
// Records of a segment that do not fill a chunk (< 64) are carried to the next segment through one of two carry buffers (ping-pong:
// a launch reads one and writes the other), chunk values that do not fill a group likewise through one of two value buffers.
// Every instance has the same stream length and segmentation, so all counts are launch parameters the host computes.
// A stream that is RESIDENT in program order (gsv_session_ciphertext_blake3) is hashed where it lies: b3_chunk_indexed_kernel reads the
// records of a range through the position table instead of from a gate-order buffer; the carry, the values and the reduce are the same.
//
// Read pattern: one lane per chunk, i.e. neighbouring lanes read 1 KiB apart, four 16-byte non-temporal loads per 64-byte block.
// No LDS, no atomics, no grid-wide synchronisation: a launch boundary separates the tree levels.
#pragma once

namespace gsv {
namespace dev {

#define GSV_B3_CHUNK_START 1u
#define GSV_B3_CHUNK_END 2u
#define GSV_B3_PARENT 4u

__device__ __forceinline__ uint32_t b3t_rotr(uint32_t x, uint32_t n) { return __builtin_amdgcn_alignbit(x, x, n); }  // v_alignbit_b32

#define GSV_B3T_G(a, b, c, d, x, y)          \
  a += b + (x); d = b3t_rotr(d ^ a, 16u);    \
  c += d;       b = b3t_rotr(b ^ c, 12u);    \
  a += b + (y); d = b3t_rotr(d ^ a, 8u);     \
  c += d;       b = b3t_rotr(b ^ c, 7u);
// one round over message words in the order given: the permutation between rounds is the renaming of the arguments
#define GSV_B3T_ROUND(i0, i1, i2, i3, i4, i5, i6, i7, i8, i9, i10, i11, i12, i13, i14, i15) \
  GSV_B3T_G(v0, v4, v8, v12, m[i0], m[i1])   GSV_B3T_G(v1, v5, v9, v13, m[i2], m[i3])         \
  GSV_B3T_G(v2, v6, v10, v14, m[i4], m[i5])  GSV_B3T_G(v3, v7, v11, v15, m[i6], m[i7])        \
  GSV_B3T_G(v0, v5, v10, v15, m[i8], m[i9])  GSV_B3T_G(v1, v6, v11, v12, m[i10], m[i11])      \
  GSV_B3T_G(v2, v7, v8, v13, m[i12], m[i13]) GSV_B3T_G(v3, v4, v9, v14, m[i14], m[i15])

// cv <- the first eight words of compress(cv, m, counter, 64 bytes, flags); m is indexed by constants only (registers)
__device__ __forceinline__ void b3_compress(uint32_t (&cv)[8], const uint32_t (&m)[16], uint32_t ctr_lo, uint32_t ctr_hi, uint32_t flags) {
  uint32_t v0 = cv[0], v1 = cv[1], v2 = cv[2], v3 = cv[3], v4 = cv[4], v5 = cv[5], v6 = cv[6], v7 = cv[7];
  uint32_t v8 = 0x6A09E667u, v9 = 0xBB67AE85u, v10 = 0x3C6EF372u, v11 = 0xA54FF53Au, v12 = ctr_lo, v13 = ctr_hi, v14 = 64u, v15 = flags;
  GSV_B3T_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  GSV_B3T_ROUND(2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)
  GSV_B3T_ROUND(3, 4, 10, 12, 13, 2, 7, 14, 6, 5, 9, 0, 11, 15, 8, 1)
  GSV_B3T_ROUND(10, 7, 12, 9, 14, 3, 13, 15, 4, 0, 11, 2, 5, 8, 1, 6)
  GSV_B3T_ROUND(12, 13, 9, 11, 15, 10, 14, 8, 7, 2, 5, 3, 0, 1, 6, 4)
  GSV_B3T_ROUND(9, 14, 11, 5, 8, 12, 15, 1, 13, 3, 0, 10, 2, 6, 4, 7)
  GSV_B3T_ROUND(11, 15, 5, 0, 1, 9, 8, 6, 14, 10, 2, 12, 3, 4, 7, 13)
  cv[0] = v0 ^ v8; cv[1] = v1 ^ v9; cv[2] = v2 ^ v10; cv[3] = v3 ^ v11; cv[4] = v4 ^ v12; cv[5] = v5 ^ v13; cv[6] = v6 ^ v14; cv[7] = v7 ^ v15;
}

// Record `idx` of carry || segment for one instance (read once: non-temporal)
__device__ __forceinline__ u32x4 b3_record(const glb_u128* carry, uint32_t carry_n, const glb_u128* seg, uint64_t idx) {
  const glb_u128* p = idx < carry_n ? carry + idx : seg + (idx - carry_n);
  return __builtin_nontemporal_load(p);
}

// grid = (max(1, ceil(n_chunks / 64)), instances), 64 threads.  Lane j of the grid's x direction hashes records [64 j, 64 j + 64) of
// carry_in[inst] (carry_n records) || seg[inst] (seg_n records) as chunk number chunk0 + j of the stream and writes its chaining value
// to cv[inst][cv_off + j]; the tail_n = carry_n + seg_n - 64 n_chunks (<= 64) records behind the last chunk go to carry_out[inst].
__global__ __launch_bounds__(64) void b3_chunk_kernel(const uint4* seg_, uint64_t seg_stride, const uint4* carry_in_, uint32_t carry_n, uint4* carry_out_, uint32_t tail_n,
                                                      uint64_t chunk0, uint32_t n_chunks, uint32_t* cv_, uint64_t cv_stride, uint32_t cv_off) {
  const uint32_t inst = blockIdx.y;
  const glb_u128* seg = (const glb_u128*)(seg_) + uint64_t(inst) * seg_stride;
  const glb_u128* carry = (const glb_u128*)(carry_in_) + uint64_t(inst) * 64u;
  if (blockIdx.x == 0 && threadIdx.x < tail_n)
    ((glb_u128*)carry_out_)[uint64_t(inst) * 64u + threadIdx.x] = b3_record(carry, carry_n, seg, uint64_t(n_chunks) * 64u + threadIdx.x);
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= n_chunks) return;
  const uint64_t rec0 = uint64_t(j) * 64u, ctr = chunk0 + j;
  uint32_t cv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  u32x4 r0 = b3_record(carry, carry_n, seg, rec0), r1 = b3_record(carry, carry_n, seg, rec0 + 1), r2 = b3_record(carry, carry_n, seg, rec0 + 2), r3 = b3_record(carry, carry_n, seg, rec0 + 3);
#pragma unroll 1
  for (uint32_t b = 0; b < 16u; ++b) {
    const uint32_t m[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
    if (b < 15u) {  // the next block's records are in flight while this one is compressed
      const uint64_t q = rec0 + 4u * (b + 1u);
      r0 = b3_record(carry, carry_n, seg, q); r1 = b3_record(carry, carry_n, seg, q + 1); r2 = b3_record(carry, carry_n, seg, q + 2); r3 = b3_record(carry, carry_n, seg, q + 3);
    }
    b3_compress(cv, m, uint32_t(ctr), uint32_t(ctr >> 32), (b == 0 ? GSV_B3_CHUNK_START : 0u) | (b == 15u ? GSV_B3_CHUNK_END : 0u));
  }
  glb_u128* out = (glb_u128*)(cv_) + (uint64_t(inst) * cv_stride + cv_off + j) * 2u;
  out[0] = u32x4{cv[0], cv[1], cv[2], cv[3]};
  out[1] = u32x4{cv[4], cv[5], cv[6], cv[7]};
}

// The chunk kernel over a stream that lies in PROGRAM order (a resident ring / a plan call's block: program.hpp, ct_pos): record q of
// the block's gate-order stream is block[(q / n_ct) * n_ct + ct_pos[q % n_ct]], and the launch hashes carry_in || records
// [first, first + n) of it, n = 64 n_chunks + tail_n - carry_n.  Everything else — chunk numbers, the carry, where the values go — is
// b3_chunk_kernel's, so the reduce kernels and the host's bookkeeping (B3Stream) do not know which of the two ran.
// A cursor divides once, where it enters the block, and then steps (replay, g) with a wrap.  Read pattern: neighbouring lanes are 64
// gate positions apart at scattered program-order addresses (the read of gather_segment_kernel without its write and the second read);
// the records of a 128-byte line are read by several lanes, or by one lane in successive trips, at different times.  Plain loads (they
// may hit the CU's L1; non-temporal ones are served by L2 every time) measured 19 % faster here.
#ifndef GSV_B3_INDEXED_NT
#define GSV_B3_INDEXED_NT 0  // load flavour of the scattered record reads: plain (0) or non-temporal (1).  Measured: plain 814 GB/s, non-temporal 662-688 GB/s
#endif
struct B3IndexedCursor {
  const glb_u128* carry;
  const glb_u128* block;
  const uint32_t* ct_pos;
  uint64_t n_ct, idx, rep_base, g;  // idx: position in carry || range; (rep_base, g): where the next record of the range lies
  uint32_t carry_n;
  __device__ __forceinline__ B3IndexedCursor(const glb_u128* carry_, uint32_t carry_n_, const glb_u128* block_, const uint32_t* ct_pos_, uint64_t n_ct_, uint64_t first, uint64_t idx_)
      : carry(carry_), block(block_), ct_pos(ct_pos_), n_ct(n_ct_), idx(idx_), carry_n(carry_n_) {
    const uint64_t q = first + (idx_ > carry_n_ ? idx_ - carry_n_ : 0u);
    rep_base = (q / n_ct_) * n_ct_;
    g = q - rep_base;
  }
  __device__ __forceinline__ u32x4 next() {
    if (idx < carry_n) return __builtin_nontemporal_load(carry + idx++);
    const glb_u128* p = block + (rep_base + ct_pos[g]);
    if (++g == n_ct) { g = 0; rep_base += n_ct; }
#if GSV_B3_INDEXED_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
  }
};
// grid and outputs as b3_chunk_kernel; block_stride = records between the instances' blocks
__global__ __launch_bounds__(64) void b3_chunk_indexed_kernel(const uint4* block_, uint64_t block_stride, const uint32_t* ct_pos, uint64_t n_ct, uint64_t first, const uint4* carry_in_, uint32_t carry_n,
                                                              uint4* carry_out_, uint32_t tail_n, uint64_t chunk0, uint32_t n_chunks, uint32_t* cv_, uint64_t cv_stride, uint32_t cv_off) {
  const uint32_t inst = blockIdx.y;
  const glb_u128* block = (const glb_u128*)(block_) + uint64_t(inst) * block_stride;
  const glb_u128* carry = (const glb_u128*)(carry_in_) + uint64_t(inst) * 64u;
  if (blockIdx.x == 0 && threadIdx.x < tail_n)
    ((glb_u128*)carry_out_)[uint64_t(inst) * 64u + threadIdx.x] = B3IndexedCursor(carry, carry_n, block, ct_pos, n_ct, first, uint64_t(n_chunks) * 64u + threadIdx.x).next();
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= n_chunks) return;
  const uint64_t ctr = chunk0 + j;
  B3IndexedCursor cur(carry, carry_n, block, ct_pos, n_ct, first, uint64_t(j) * 64u);
  uint32_t cv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  u32x4 r0 = cur.next(), r1 = cur.next(), r2 = cur.next(), r3 = cur.next();
#pragma unroll 1
  for (uint32_t b = 0; b < 16u; ++b) {
    const uint32_t m[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
    if (b < 15u) { r0 = cur.next(); r1 = cur.next(); r2 = cur.next(); r3 = cur.next(); }  // the next block's records are in flight while this one is compressed
    b3_compress(cv, m, uint32_t(ctr), uint32_t(ctr >> 32), (b == 0 ? GSV_B3_CHUNK_START : 0u) | (b == 15u ? GSV_B3_CHUNK_END : 0u));
  }
  glb_u128* out = (glb_u128*)(cv_) + (uint64_t(inst) * cv_stride + cv_off + j) * 2u;
  out[0] = u32x4{cv[0], cv[1], cv[2], cv[3]};
  out[1] = u32x4{cv[4], cv[5], cv[6], cv[7]};
}

// One level of the group trees, in place: cv[inst][i * step] <- parent(cv[inst][i * step], cv[inst][i * step + step / 2]) for i < n_parents.
// A lane reads both children before it writes over the left one, and no other lane of the launch touches either.
__global__ __launch_bounds__(64) void b3_parent_kernel(uint32_t* cv_, uint64_t cv_stride, uint32_t n_parents, uint32_t step) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n_parents) return;
  glb_u128* l = (glb_u128*)(cv_) + (uint64_t(blockIdx.y) * cv_stride + uint64_t(i) * step) * 2u;
  const glb_u128* r = l + uint64_t(step / 2u) * 2u;
  const u32x4 a = l[0], b = l[1], c = r[0], d = r[1];
  const uint32_t m[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
  uint32_t cv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  b3_compress(cv, m, 0u, 0u, GSV_B3_PARENT);
  l[0] = u32x4{cv[0], cv[1], cv[2], cv[3]};
  l[1] = u32x4{cv[4], cv[5], cv[6], cv[7]};
}

// After the levels: group g's value sits at cv[inst][g * group].  red[inst][g] <- it for g < n_groups (dense: stride n_groups), and the
// n_left values behind the last complete group go to the front of the OTHER value buffer, where the next segment's chunk values join them.
__global__ __launch_bounds__(64) void b3_compact_kernel(const uint32_t* cv_, uint64_t cv_stride, uint32_t n_groups, uint32_t group, uint32_t n_left, uint32_t* red_, uint32_t* next_) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n_groups + n_left) return;
  const glb_u128* src = (const glb_u128*)(cv_) + uint64_t(blockIdx.y) * cv_stride * 2u;
  const bool grp = i < n_groups;
  src += grp ? uint64_t(i) * group * 2u : (uint64_t(n_groups) * group + (i - n_groups)) * 2u;
  glb_u128* dst = grp ? (glb_u128*)(red_) + (uint64_t(blockIdx.y) * n_groups + i) * 2u
                      : (glb_u128*)(next_) + (uint64_t(blockIdx.y) * cv_stride + (i - n_groups)) * 2u;
  dst[0] = src[0];
  dst[1] = src[1];
}

}  // namespace dev
}  // namespace gsv

extern "C" {
int gsvk_b3_chunks(const void* seg, uint64_t seg_stride, const void* carry_in, uint32_t carry_n, void* carry_out, uint32_t tail_n, uint64_t chunk0, uint32_t n_chunks,
                   void* cv, uint64_t cv_stride, uint32_t cv_off, uint32_t n_instances, hipStream_t s) {
  if (n_instances == 0 || tail_n > 64u || carry_n > 64u || uint64_t(cv_off) + n_chunks > cv_stride) return int(hipErrorInvalidValue);
  if (n_chunks == 0 && tail_n == 0) return 0;
  hipLaunchKernelGGL(gsv::dev::b3_chunk_kernel, dim3(n_chunks ? (n_chunks + 63u) / 64u : 1u, n_instances), dim3(64), 0, s, static_cast<const uint4*>(seg), seg_stride,
                     static_cast<const uint4*>(carry_in), carry_n, static_cast<uint4*>(carry_out), tail_n, chunk0, n_chunks, static_cast<uint32_t*>(cv), cv_stride, cv_off);
  return int(hipGetLastError());
}
// the same over records [first, first + n) of a program-order block's gate-order stream (b3_chunk_indexed_kernel); the caller keeps the range inside the block
int gsvk_b3_chunks_indexed(const void* block, uint64_t block_stride, const void* ct_pos, uint64_t n_ct, uint64_t first, const void* carry_in, uint32_t carry_n, void* carry_out, uint32_t tail_n,
                           uint64_t chunk0, uint32_t n_chunks, void* cv, uint64_t cv_stride, uint32_t cv_off, uint32_t n_instances, hipStream_t s) {
  if (n_instances == 0 || n_ct == 0 || tail_n > 64u || carry_n > 64u || uint64_t(cv_off) + n_chunks > cv_stride) return int(hipErrorInvalidValue);
  if (n_chunks == 0 && tail_n == 0) return 0;
  hipLaunchKernelGGL(gsv::dev::b3_chunk_indexed_kernel, dim3(n_chunks ? (n_chunks + 63u) / 64u : 1u, n_instances), dim3(64), 0, s, static_cast<const uint4*>(block), block_stride,
                     static_cast<const uint32_t*>(ct_pos), n_ct, first, static_cast<const uint4*>(carry_in), carry_n, static_cast<uint4*>(carry_out), tail_n, chunk0, n_chunks,
                     static_cast<uint32_t*>(cv), cv_stride, cv_off);
  return int(hipGetLastError());
}
// n_have values per instance in cv (stride cv_stride values): n_have / 2^k groups are reduced and written to red (dense), the rest moves to the
// front of cv_next
int gsvk_b3_reduce(void* cv, uint64_t cv_stride, uint32_t n_have, uint32_t k, void* red, void* cv_next, uint32_t n_instances, hipStream_t s) {
  if (n_instances == 0 || k > 20u || n_have > cv_stride) return int(hipErrorInvalidValue);
  const uint32_t group = 1u << k, n_groups = n_have >> k, n_left = n_have - (n_groups << k);
  for (uint32_t l = 1; l <= k && n_groups; ++l) {
    const uint32_t n_parents = n_groups << (k - l);
    hipLaunchKernelGGL(gsv::dev::b3_parent_kernel, dim3((n_parents + 63u) / 64u, n_instances), dim3(64), 0, s, static_cast<uint32_t*>(cv), cv_stride, n_parents, 1u << l);
  }
  if (n_groups + n_left)
    hipLaunchKernelGGL(gsv::dev::b3_compact_kernel, dim3((n_groups + n_left + 63u) / 64u, n_instances), dim3(64), 0, s, static_cast<const uint32_t*>(cv), cv_stride, n_groups, group, n_left,
                       static_cast<uint32_t*>(red), static_cast<uint32_t*>(cv_next));
  return int(hipGetLastError());
}
}  // extern "C"
