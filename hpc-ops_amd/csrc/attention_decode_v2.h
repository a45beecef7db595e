// Interface between the decode-attention C entries (attention_decode.hip) and the second-generation kernel
// (attention_decode_v2.hip): fp8 with per-tensor or per-token K scales and bf16, head pairs on NHD (development: HND) pages,
// four heads (development), or one (virtual) kv head per workgroup on any page layout.  Internal header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attention_decode_route.h"

namespace hpc {
namespace decode2 {

struct Args {
  const void* q;
  const void* kcache;
  const void* vcache;
  const int* block_ids;
  const int* lens;       // num_seq_kvcache [B]
  const int* task_map;   // the scheduler's task map: only header int 6 (min_process_len) is read - the plan is in-kernel
  uint16_t* y;
  float* part_o;         // [workgroups][2][2 heads][16][128]   (both: DecodeWs::part_o2 / part_lse2, attention_decode_route.h)
  float* part_lse;       // [workgroups][2][2 heads][16]
  int* arrive;           // [pairs * B] arrival counters of split requests (zero before the call, left zero)
  const float* qscale;   // [B * Sq, qscale_stride]
  const float* kscale;   // [1] or the K-scale tail rows of the cache
  const float* vscale;   // [1] or [Hkv]
  int num_batch, num_seq_q, num_head_kv, g_shift, page_shift, max_blocks;
  int ldq, ldy, qscale_stride, new_kv_included;
  // one kv head per workgroup only (mode 3): the workgroup's head index is a VIRTUAL head - slice (vh & (slices - 1)) of the
  // 1 << share_shift slices that kv head vh >> share_shift's q heads are cut into (GQA group 16 with more q rows than a form
  // holds).  num_head_kv counts virtual heads and g_shift is the slice's group then: q heads, q scales, y rows, partial slots
  // and arrival counters are addressed by vh exactly as for a real head; K / V pages, per-token K scales and per-head V
  // scales by vh >> share_shift.  0 everywhere else.
  int share_shift = 0;
  int min_range_cost;  // smallest range of the in-kernel plan, in cost units (64-token tiles + 2 per request)
  int bf16;       // 1: bf16 q / K / V (no scales; ldq and every stride in BYTES), 0: fp8 e4m3
  int ktok = 0;   // fp8: 1 = per-token K scales in the pages' tail rows (kscale + ks_* strides) and per-head V scales (quant_type 0)
  int pair_wgs[4];  // fp8, 4 head pairs: workgroups (= ranges) per pair, [0] = 0: equal shares
  int big_pct;      // > 100: ranges of the first half of the grid are this many percent of the others' length
  int dev_nomem;  // development key kDevDecodeNoKvLoads = 1: K / V loads fetch nothing (compute-only timing; results are wrong)
  int pair_xor;   // workgroups from mate_from on (the SECOND workgroup of every CU) serve head pair p ^ pair_xor: a CU's two
  int mate_from;  // workgroups stream slices of the token rows that differ in byte-address bit 9 (see the kernel); 0 = off
  int xcd_map;    // development key kDevDecodeXcdMap: eight 3-bit entries, workgroup 8 j + x serves pair (e & 3) of range 2 j + (e >> 2), e = entry x
  int dev_sleep;  // development key kDevDecodeSleep: workgroups of even head pairs sleep this many x 64 clocks per wave-iteration
  int dev_merge_dup = 0;  // development key kDevDecodeMergeDup = 1: the last arriver loads (and folds with weight zero) a duplicate for a missing second chunk
  int dev_nosnap = 0;     // development key kDevDecodeNoSnap = 1: short requests of an underloaded launch may be split (rounds 2-5)
  int dev_slice;  // development key kDevDecodeOneSlice = s + 1: every workgroup streams slice s of the token rows (timing only; results are wrong)
  long k_block_stride, k_token_stride;  // bytes
  long v_block_stride, v_token_stride;
  long ks_block_stride, ks_row_stride, ks_head_stride;  // bytes
  int hnd = 0;    // fp8: 1 = HND pages [page][head][token][128 B] (k / v_head_stride below; token strides are 128)
  long k_head_stride = 0, v_head_stride = 0;  // bytes (read by the HND form only)
  float scale_log2;
  void* prof;  // development: per-wave timing sums [workgroups][4][12] uint64 (null = off)
};

// Launches the form that `r` (generation 2) names on r.num_wg workgroups.  `a`: filled by the entry but for the members that follow
// from the grid (pair_xor ... dev_slice); a.arrive is the workspace's counter region, left zero also when the launch fails.
int launch(Args a, const DecodeRoute& r, hipStream_t stream);
#ifdef HPC_DEV
// development build: arrivals that drew a ticket ABOVE their request's chunk count since the last reset - the signature of
// an arrival counter that was not zero on entry (the zero-bytes contract of the workspace was broken: the last arriver is
// never recognised and the request's rows of y stay unwritten).  Synchronises the device.
int ticket_overruns(bool reset);
#endif

}  // namespace decode2
}  // namespace hpc
