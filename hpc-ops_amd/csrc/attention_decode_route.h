// Which decode-attention kernel form and grid runs for a call: decode_route() is the one statement of it.
// Internal header, host only, no HIP calls: a pure function of the call's shapes, the CU count and - in the development
// build - the keys that select a form or a grid (12, 14, 28, 29, 33, 54, 55, 60; read here and nowhere else).
#pragma once
#include "hpc_common.h"
#include "hpc_dev.h"

namespace hpc {
namespace decode2 {
// Arrival counters of split requests: a fixed region at the very start of a call's workspace.  It must be zero
// the first time a workspace is used (the kernels leave it zero); its place and size do not depend on the call.
constexpr int64_t kCounterBytes = 64 * 1024;
}  // namespace decode2

// Where each piece of a decode call's scratch sits, in bytes from the start of the workspace: the one statement of it
// (hpc_attention_decode_workspace_bytes sizes from it, the two generations' argument blocks are carved from it):
//   [arrival counters: kCounterBytes, zero-once, shared by the two generations - one of which runs per call]
//   [first generation: part_o [num_bins][2 slots][rows][128] f32, part_lse [num_bins][2][rows] f32 (rows = the call's q rows per kv
//    head, padded to 16), first_bin [num_head_kv * num_batch] i32 (combine-kernel form only), padded to 16 bytes]
//   [second generation: part_o [num_wg][2 slots][2 heads][16][128] f32, then part_lse [num_wg][2][2][16] f32 directly behind the
//    num_wg slots in use]
// num_wg is the second generation's grid.  Invariant: num_wg <= num_bins - decode_route() never routes a grid above the bin count
// the workspace was sized with -, so a call's total never exceeds the size at num_wg = num_bins, which is what the sizer returns.
struct DecodeWs {
  int64_t counters, part_o, part_lse, first_bin;  // first generation (counters: either)
  int64_t part_o2, part_lse2;                     // second generation
  int64_t total;
};
static inline DecodeWs decode_ws_layout(int num_bins, int num_batch, int num_head_kv, int num_seq_q, int group, int num_wg) {
  const int64_t rows = (static_cast<int64_t>(num_seq_q) * group + 15) / 16 * 16;
  const int64_t first_bin_bytes = static_cast<int64_t>(num_batch) * num_head_kv * 4;
  DecodeWs w{};
  w.counters = 0;
  w.part_o = decode2::kCounterBytes;
  w.part_lse = w.part_o + static_cast<int64_t>(num_bins) * 2 * rows * 128 * 4;
  w.first_bin = w.part_lse + static_cast<int64_t>(num_bins) * 2 * rows * 4;
  w.part_o2 = w.first_bin + (first_bin_bytes + 15) / 16 * 16;
  w.part_lse2 = w.part_o2 + static_cast<int64_t>(num_wg) * 2 * 2 * 16 * 128 * 4;
  w.total = w.part_lse2 + static_cast<int64_t>(num_wg) * 2 * 2 * 16 * 4;
  return w;
}

struct DecodeCall {  // what the call is; strides in BYTES
  bool bf16;         // else fp8 e4m3
  int quant_type;    // fp8: 1 = q per token and head, K / V per tensor; 0 = K per token (page tail rows), V per head
  bool lens_on_device;
  int num_bins, num_batch, num_seq_q, num_head_q, num_head_kv, block_size;
  int64_t k_block_stride, k_token_stride, k_head_stride;
  int64_t v_block_stride, v_token_stride, v_head_stride;
  int64_t ks_block_stride, ks_row_stride, ks_head_stride;  // per-token K scales (quant_type 0)
  int cu_count;  // <= 0 (no device): first generation
};

struct DecodeRoute {  // what runs
  int code;        // HPC_OK or the refusal; nothing below is set on a refusal
  int generation;  // 1: attention_decode.hip (a workgroup per scheduler bin), 2: attention_decode_v2.hip (in-kernel plan and merge)
  // second generation
  int mode;         // 1: a head pair per workgroup, 2: four heads (development), 3: one (virtual) kv head with up to 32 q rows
  int hnd;          // head pairs on HND pages [page][head][token][128 B] (development)
  int share_shift;  // mode 3: a kv head's 16 q heads are served as 1 << share_shift virtual heads of 8 adjacent q heads
  // first generation
  int passes;          // 2: one pass per slice of 8 adjacent q heads of a group-16 kv head, each streaming the whole cache
  int num_nb;          // 16-row q blocks per kv head (and pass): the kernel form
  int num_wg;          // either generation: grid of the main kernel
  int combine_kernel;  // first generation: split requests merged by decode_combine_kernel in a second launch (no arrival counters)
};

// Refusals come first, in the order of the C entries.  A call routes by its q rows per kv head (num_seq_q x group):
//  * <= 16: head pairs (NHD pages with adjacent kv heads contiguous - 128 B apart for fp8, 256 B for bf16 -, an even number of kv
//    heads, lengths on the device, <= 1024 requests) or the first generation's one-block form;
//  * 17 ... 32: one kv head per workgroup (any page layout and head count; fp8 on pages of 32 / 64 only) or the two-block form;
//  * 33 ... 48: bf16 only, the three-block form - 16 x 3 rows in one pass, 319 / 395 us against 365 / 503 us as two slices on the
//    C3 mix / uniform 8k at 8 kv heads (profiles/gqa_groups_decode.txt);
//  * group 16 with more rows than that (fp8 > 32, bf16 > 48) is served as two slices of 8 adjacent q heads.  num_seq_q 3, 4 (24 / 32
//    rows per slice): each slice is a virtual kv head of the one-head form - a slice's q heads, q scales and y rows are contiguous
//    at (virtual head) << 3, what that kernel computes for a real head of group 8; only K / V / scale addresses use the real
//    head.  A kv head's K / V bytes are requested once per slice; sibling slices share an XCD's L2 where the kv head count allows
//    (see the kernel): 1.40-1.58 x the time of one pass.  A call that form cannot take runs as one first-generation pass per
//    slice (2 x).  bf16 num_seq_q 5 (40 rows per slice): two passes of the three-block form, 599 / 755 us - measured against four
//    slices of 20 rows on the one-head form: 659 / 899 us.
// (static: the product and the development library may sit in one process, and each must call its own)
static inline DecodeRoute decode_route(const DecodeCall& c) {
  DecodeRoute r{};
  auto refuse = [&r](int code) { return r.code = code, r; };
  const bool ktok = !c.bf16 && c.quant_type == 0;
  if (!c.bf16 && ((c.quant_type != 0 && c.quant_type != 1) || c.num_seq_q > 4)) return refuse(HPC_ERR_UNSUPPORTED);
  if (c.block_size != 16 && c.block_size != 32 && c.block_size != 64) return refuse(HPC_ERR_UNSUPPORTED);
  if (c.num_head_kv <= 0 || c.num_head_q % c.num_head_kv || c.num_batch <= 0 || c.num_bins <= 0) return refuse(HPC_ERR_INVALID);
  const int group = c.num_head_q / c.num_head_kv;
  // powers of two up to 16: q rows are addressed by shift and mask (the prefill ops take the same set)
  if ((group != 1 && group != 2 && group != 4 && group != 8 && group != 16) || c.num_seq_q < 1 || c.num_seq_q > 5)
    return refuse(HPC_ERR_UNSUPPORTED);
  const auto mult16 = [](int64_t a, int64_t b, int64_t d) { return ((a | b | d) & 15) == 0; };  // 16-byte vector accesses
  if (!mult16(c.k_block_stride, c.k_token_stride, c.k_head_stride) || !mult16(c.v_block_stride, c.v_token_stride, c.v_head_stride))
    return refuse(HPC_ERR_UNSUPPORTED);
  if (ktok && c.block_size < 32) return refuse(HPC_ERR_UNSUPPORTED);  // scale rows hold 32 tokens

  const bool sliced = group == 16 && c.num_seq_q * group > (c.bf16 ? 48 : 32);
  const int rows = sliced ? c.num_seq_q * 8 : c.num_seq_q * group;  // per (virtual) kv head or pass
  const int64_t counters = static_cast<int64_t>(c.num_batch) * c.num_head_kv * 4;
  const auto first_generation = [&] {
    r = DecodeRoute{};
    r.generation = 1;
    r.passes = sliced ? 2 : 1;
    r.num_nb = (rows + 15) / 16;
    r.num_wg = c.num_bins;
    // development key kDevDecodeCombineKernel = 1: the round-1 form
    r.combine_kernel = counters > decode2::kCounterBytes || hpc_dev_tuning_get(kDevDecodeCombineKernel) == 1;
    return r;
  };
  // development keys: kDevDecodeFp8NoPair (either dtype) / kDevDecodeBf16NoPair = 1: first generation only; kDevDecodeQt0FirstGen = 1:
  // per-token K scales on the first generation (rounds 1-5)
  if (!c.lens_on_device || c.cu_count <= 0 || rows > 32 || hpc_dev_tuning_get(kDevDecodeFp8NoPair) == 1 ||
      (c.bf16 && hpc_dev_tuning_get(kDevDecodeBf16NoPair) == 1) || (ktok && hpc_dev_tuning_get(kDevDecodeQt0FirstGen) == 1))
    return first_generation();

  // ---- second generation: what its forms need (strides that reach the kernel as 32-bit offsets, counters that fit the region) ----
  const int heads = c.num_head_kv << (sliced ? 1 : 0);  // virtual heads
  const int head_bytes = c.bf16 ? 256 : 128;
  const bool below_4g = c.k_block_stride > 0 && c.v_block_stride > 0 && c.k_block_stride < (1ll << 32) && c.v_block_stride < (1ll << 32);
  const bool ks_below_4g = c.ks_block_stride > 0 && c.ks_block_stride < (1ll << 32) && (c.ks_row_stride % 4) == 0;
  const bool nhd = c.k_head_stride == head_bytes && c.v_head_stride == head_bytes;
  // One kv head per workgroup (mode 3): 17 ... 32 q rows per (virtual) kv head.  Measured against the two-block form
  // (profiles/round6_decode_ab.txt, call 8; C3 lengths, us): num_seq_q 3, 8 / 64 heads NHD mix 195.6 -> 163.8, uniform 8k 220 -> 196;
  // HND 193 -> 150 / 218 -> 180; num_seq_q 4: 4 / 32 heads 112 -> 87.5 / 112 -> 95, 1 / 8 heads 49.5 -> 41.4.  Development key
  // kDevDecodeSoloForm: 1 = never (rounds 1-5), 2 = also every other call that the pair form does not take (<= 16 q rows on HND pages
  // or with an odd head count) - there the first generation stays ahead (one kv head, 8 q rows: 31 against 38-40 us; HND mix 138 /
  // 139, 32 x 128 + 32 x 4k 63 against 71 us), 3 = every eligible call (A/B against the pair forms).
  const int k60 = hpc_dev_tuning_get(kDevDecodeSoloForm);
  const bool pair_case = heads % 2 == 0 && rows <= 16 && nhd && (!ktok || c.ks_head_stride == 128);
  const bool solo_ok = below_4g && (!ktok || (ks_below_4g && (c.ks_head_stride % 4) == 0)) && (c.block_size >= 32 || c.bf16) &&
                       c.k_token_stride * 32 < (1ll << 31) && c.v_token_stride * 32 < (1ll << 31) && c.num_batch <= 1024 &&
                       static_cast<int64_t>(c.num_batch) * heads * 4 <= decode2::kCounterBytes;
  if (solo_ok && (k60 == 3 || (k60 == 2 && !pair_case) || (k60 == 0 && rows > 16))) {
    r.mode = 3;
    r.share_shift = sliced ? 1 : 0;
  } else if (!sliced) {  // virtual heads exist in the one-head form only
    // fp8 with per-tensor scales on HND pages, a head's tokens contiguous: development key kDevDecodeHndPair = 1 only.  Measured
    // (profiles/round6_decode_ab.txt, call 3): against the first generation the HND form wins on length mixes (C3 mix 137.3 vs 141.2 us,
    // 32 x 128 + 32 x 4k 57.8 vs 60.6) and loses where the task map gives every workgroup one whole (request, head) and this kernel's
    // plan cuts every request in two (uniform 8k: 181.7 us = 0.74 against 164-178 us = 0.75-0.82) - and 1 KB contiguous pieces stream
    // no faster through this pipeline than the NHD form's 256-byte slices do: HND pages stay on the first generation.
    const bool hnd = !c.bf16 && !ktok && c.k_token_stride == 128 && c.v_token_stride == 128 && c.k_head_stride >= 128 * c.block_size &&
                     c.v_head_stride >= 128 * c.block_size && c.k_head_stride < (1ll << 28) && c.v_head_stride < (1ll << 28) &&
                     heads > 1 && hpc_dev_tuning_get(kDevDecodeHndPair) == 1;
    // per-token K scales: a wave-iteration's 32 tokens x 2 heads of scales must be one contiguous 256-byte piece of a page's tail row
    if (heads % 2 == 0 && rows <= 16 && (nhd || hnd) && below_4g && c.num_batch <= 1024 &&
        static_cast<int64_t>(c.num_batch) * (heads / 2) * 4 <= decode2::kCounterBytes && (!ktok || (c.ks_head_stride == 128 && ks_below_4g))) {
      // Four heads per workgroup (fp8, <= 8 q rows per kv head, a multiple of 4 kv heads): measured 3-5 % SLOWER than head pairs on the
      // graded shapes (uniform 8k 188.8 vs 183.0 us, C3 mix 145.4 vs 138.6 us, profiles/round3_decode_fp8_forms_ab.txt) - the waves
      // sit in the load issue either way.  Development key kDevDecodeQuadForm = 2 selects it (kept: tested, half the softmax work);
      // GQA groups 4 and 8 only - its column -> (head, q row) selects were written and tested for those.
      const bool quad = !c.bf16 && !ktok && !hnd && heads % 4 == 0 && (group == 4 || group == 8) && rows <= 8 &&
                        hpc_dev_tuning_get(kDevDecodeQuadForm) == 2;
      r.mode = quad ? 2 : 1;
      r.hnd = hnd;
    }
  }
  if (r.mode == 0) return first_generation();
  // two 4-wave workgroups per CU (<= 256 registers, 65 KB of LDS each), a whole number of units: a workgroup is a (token range,
  // head pair, quad or (virtual) head); the scratch is sized for num_bins workgroups
  const int unit = r.mode == 3 ? heads : heads / (r.mode == 2 ? 4 : 2);
  const int wg_dev = hpc_dev_tuning_get(kDevDecodeGrid);
  const int num_wg = wg_dev > 0 ? wg_dev : 2 * c.cu_count;
  r.num_wg = (num_wg < c.num_bins ? num_wg : c.num_bins) / unit * unit;
  if (r.num_wg <= 0) return first_generation();  // fewer bins than units
  r.generation = 2;
  return r;
}

}  // namespace hpc
