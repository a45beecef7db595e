/* hpc_amd.h — C-ABI of libhpc_amd.so, the MI355X (gfx950) drop-in for the decode-step hot path
 * of Tencent/hpc-ops.
 *
 * Every entry point replaces one `*_async` host launcher of the reference (cited per function)
 * and keeps its argument meaning: raw device pointers, int dims, int64 strides for the KV cache,
 * the stream last.  No torch types cross this boundary.
 *
 * Return convention (replaces the reference's `bool running` / cudaError_t mix,
 * src/attention/entry.cc:722, src/allreduce/entry.cc:187-189):
 *    0  launched on `stream` (asynchronous, never synchronises)
 *   -1  HPC_ERR_UNSUPPORTED  shape / tile configuration not supported
 *   -2  HPC_ERR_INVALID      bad argument (null pointer, inconsistent sizes)
 *   -3  HPC_ERR_LAUNCH       the HIP runtime refused the launch
 *   -4  HPC_ERR_TIMEOUT      (fused all-reduce only) an earlier call on this process gave up waiting
 *                            for a peer; the symmetric buffers / signal pads are in an undefined state
 * The Python shim turns every non-zero code into RuntimeError("... launch failed!").
 */
#ifndef HPC_AMD_H_
#define HPC_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* hipStream_t without dragging hip headers into FFI users. */
typedef struct ihipStream_t* hpc_stream_t;

/* ---- library identity (reference: src/C/version.cc, src/C/built_json.cu:17-43) ---------- */
const char* hpc_version(void);
const char* hpc_built_json(void);
/* Number of compute units of device `device_id` (reference get_sm_count(), src/utils/utils.cc:15-27;
 * here per device, not a device-0 cache). */
int hpc_get_cu_count(int device_id);

/* ---- RMSNorm (+fp8 quant) ------------------------------------------------------------------
 * reference: fused_rmsnorm_with_scale_async, src/normalization/fused_rmsnorm_with_scale.h:19-22
 *            kernel src/normalization/fused_rmsnorm_with_scale.cu:14-137.
 * input bf16 [batch, hidden], weight bf16 [hidden], scale f32 [1] (or [2] when is_moe).
 * output_fp8 e4m3 [batch, hidden] = y / scale[0];  is_moe: output_fp32 = y,
 * output_fp8_scale2 = y / scale[1].  hidden % 8 == 0, hidden <= 16384. */
int hpc_fused_rmsnorm_with_scale_async(const void* input, const void* weight, void* output_fp8,
                                       void* output_fp32, void* output_fp8_scale2,
                                       const void* scale, float eps, int batch_size,
                                       int hidden_state, int is_moe, hpc_stream_t stream);

/* ---- decode attention: dynamic split-KV tile scheduler ----------------------------------------
 * reference: assign_attention_decode_task_{sync,async}, src/attention/decode/decode.h:37-46,
 *            src/attention/decode/assign_task.cu:333-492, CPU entry packing src/attention/entry.cc:727-778,
 *            record/bins constants src/attention/decode/sched_task_info.h:18-36.
 * Task-map layout (int32 rows of 12) is the reference's; see hpc-ops_amd/csrc/sched_task_info.h.
 *
 * hpc_attention_decode_num_bins: number of scheduler bins (= decode workgroups) on `device_id`
 *   for num_seq_q in 1..5 (reference: kCtaPerSmMap[sm][num_seq_q-1] * get_sm_count()).
 * hpc_attention_decode_tile_n:   KV tokens per scheduling tile (64).
 * hpc_assign_attention_decode_task_rows / _sync: host scheduler. `_rows` returns the number of
 *   48-byte rows the host image needs (1 + bins*(tiles_per_bin+1) + ceil(Hkv*B*4/48)); `_sync`
 *   fills `task_map` (>= rows*12 ints) like the reference CPU entry and returns rows.
 * hpc_assign_attention_decode_task_async: device scheduler; `task_map` is the workspace of
 *   hpc.get_attention_decode_task_workspace (header ints 2..4 pre-filled by the allocator),
 *   num_seq_kvcache is a device pointer.  `num_total_ctas` is the UPPER bound the decode launch is sized for: a
 *   batch with little work is planned on fewer bins (hpc_attention_decode_effective_bins: at least 8 tiles per bin,
 *   at least 64 bins) and header int 1 of the map records the count used - consumers read it from there.  Byte-
 *   identical to the host scheduler run with that count.
 * hpc_attention_decode_effective_bins: that count from host lengths (what the CPU entry of the op passes to _sync).
 * hpc_attention_decode_task_workspace_bytes: bytes of a task-map workspace for up to max_num_batch requests of up to
 *   max_seqlen KV tokens on a device of num_cu CUs, whatever bin count (up to 4 per CU) a call plans on - the reference's
 *   sizes (hpc/attention.py:540-571).  *sched_bytes (nullable): the part the allocator records in header int 4.  < 0: error. */
int hpc_attention_decode_num_bins(int num_seq_q, int device_id);
int hpc_attention_decode_effective_bins(const int* num_seq_kvcache, int num_batch, int num_head_kv, int num_seq_q,
                                        int new_kv_included, int max_bins);
int hpc_attention_decode_tile_n(void);
int hpc_assign_attention_decode_task_rows(const int* num_seq_kvcache, int num_total_ctas,
                                          int num_batch, int num_head_kv, int num_seq_q,
                                          int new_kv_included, int min_process_len);
int64_t hpc_attention_decode_task_workspace_bytes(int num_cu, int max_num_batch, int64_t max_seqlen, int num_head_kv,
                                                  int min_process_len, int64_t* sched_bytes);
int hpc_assign_attention_decode_task_sync(const int* num_seq_kvcache, int num_total_ctas,
                                          int num_batch, int num_head_kv, int num_seq_q,
                                          int new_kv_included, int min_process_len, int* task_map,
                                          int task_map_rows);
int hpc_assign_attention_decode_task_async(int* task_map, const int* num_seq_kvcache,
                                           int num_total_ctas, int num_batch, int num_head_kv,
                                           int num_seq_q, int new_kv_included, int min_process_len,
                                           hpc_stream_t stream);

/* ---- decode attention (paged KV, D = 128, GQA group 1, 2, 4, 8 or 16) -------------------------------
 * num_head_q / num_head_kv in {1, 2, 4, 8, 16} - the groups the prefill ops take; any other ratio is HPC_ERR_UNSUPPORTED.
 * A call routes by its q rows per kv head, num_seq_q * group:
 *   <= 16     head pairs (NHD pages, even kv head count, device lengths) or the first-generation one-block form
 *             (HND pages, odd kv head count, NULL lengths): groups 1 and 2 at every num_seq_q, group 16 at num_seq_q 1;
 *   17 ... 32 one kv head per workgroup (fp8: pages of 32 / 64, device lengths) or the first generation's two-block
 *             form: group 16 at num_seq_q 2, group 8 at 3 / 4;
 *   33 ... 48 bf16 only, group 8 at num_seq_q 5 and group 16 at num_seq_q 3: the first generation's three-block form;
 *   group 16 beyond that (fp8 num_seq_q 3 / 4: 48 / 64 rows; bf16 4 / 5: 64 / 80): no wider form - the kv head's 16 q heads are
 *             served as 2 slices of 8.  At num_seq_q 3 / 4 each slice is a virtual kv head of the one-head-per-workgroup form
 *             that reads the real head's K / V: its bytes are requested twice, sibling slices run on the same XCD when the kv
 *             head count divides or is a multiple of 8, and its L2 absorbs about half of the repeat (1.4-1.6 x the time of
 *             one pass; profiles/gqa_groups_decode.txt).  Outside that form's conditions (device lengths; fp8: pages of 32 / 64;
 *             num_batch * num_head_kv * 2 <= 16384), and at bf16 num_seq_q 5 (40 rows per slice: the three-block form), the call
 *             runs as one first-generation pass per slice: 2 x the time of a pass.  No sliced call is refused.
 * hpc_attention_decode_workspace_bytes is unchanged by slicing (partial slots are per workgroup).
 * reference: attention_decode_bf16_async / attention_decode_fp8_async,
 *            src/attention/decode/decode.h:17-35 (kernels under src/attention/decode/sm90/).
 * q [B*Sq, Hq, 128] (row stride ldQ elements), kcache/vcache logical [blocks, block_size, Hkv, 128]
 * with element strides (block, token, head), block_ids int32 [B, num_seq_max_blocks],
 * y bf16 [B*Sq, Hq, 128] (row stride ldY).  `task_map_ptr` is a task map produced by the
 * scheduler above for the same num_seq_kvcache / num_seq_q / new_kv_included.  `num_bins` is the UPPER bound the
 * launch and the workspace are sized with - hpc_attention_decode_num_bins(num_seq_q, device), the value the torch
 * binding passes - NOT the map's header[1]: the scheduler plans a batch with little work on fewer bins
 * (hpc_attention_decode_effective_bins) and records the count it used in header[1] <= num_bins; the kernels read it
 * from there.  A caller that passed header[1] as num_bins would cap the head-pair kernel's grid at that count instead of
 * two workgroups per CU.
 * `workspace` holds the arrival counters of split requests and the fp32 split-KV partials:
 * hpc_attention_decode_workspace_bytes bytes.  Its first hpc_attention_decode_workspace_zero_bytes() bytes (the
 * counters: a fixed place and size whatever the shapes of the call) must be ZERO the first time the buffer is
 * used - like the reference's split_flag, which its entry allocates zeroed (src/attention/entry.cc:690-694) - and
 * every call leaves them zero again, so one buffer per stream can be reused call after call, with any sequence
 * of shapes, and inside a captured hipGraph; the rest needs no initialisation (the reference allocates
 * lse/split_out per call, src/attention/entry.cc:492-499; here it is 2 slots per workgroup instead of splitk
 * slots per request).  The zero-bytes contract applies to EVERY decode path (since round 5 the first-generation
 * kernels take their tickets there too): a counter that is not zero on entry - a caller-owned buffer that was never
 * cleared, or one left behind by a launch that faulted - means the last arriver of a split request is never
 * recognised and that request's rows of y are not written.  One buffer must not be used by two calls that may run
 * concurrently (two streams: two buffers).  The split-KV combine runs inside the launch on both kernel generations:
 * the chunk of a request that arrives LAST merges all of them (reference: static_splitk_kernels.cuh:362-377); there
 * is no second kernel.
 * num_seq_kvcache_ptr (device int32 [num_batch]) / new_kv_included as in the reference launchers (decode.h:17-35): with
 * them, NHD pages (adjacent kv heads contiguous) with an even head count and <= 16 q rows per kv head take the
 * second-generation kernel (attention_decode_v2.hip), which plans its ranges in closed form from the lengths and takes
 * from the task map only header int 6 (the scheduler call's min_process_len: the lower bound of its split granularity);
 * NULL lengths = the task map's bins drive the first-generation kernel. */
int64_t hpc_attention_decode_workspace_bytes(int num_bins, int num_batch, int num_head_kv,
                                             int num_seq_q, int heads_per_group);
int64_t hpc_attention_decode_workspace_zero_bytes(void);
/* 0 when `stream` is not being captured into a hipGraph, else the unique non-zero id of the capture (< 0: error).  A
 * host that caches the decode workspace per stream must not carry a buffer whose zero-fill was only RECORDED in one
 * capture over to another capture or to eager calls: key the cache on (stream, capture id). */
long long hpc_stream_capture_id(hpc_stream_t stream);
int hpc_attention_decode_bf16_async(void* y_ptr, void* workspace, const int* task_map_ptr,
                                    const void* q_ptr, const void* kcache_ptr,
                                    const void* vcache_ptr, const int* block_ids_ptr,
                                    const int* num_seq_kvcache_ptr, int new_kv_included, int num_bins,
                                    int num_batch, int num_seq_q, int num_head_q, int num_head_kv,
                                    int num_dim_qk, int num_dim_v, int block_size,
                                    int num_seq_max_blocks, int ldY, int ldQ,
                                    int64_t kcache_block_stride, int64_t kcache_token_stride,
                                    int64_t kcache_head_stride, int64_t vcache_block_stride,
                                    int64_t vcache_token_stride, int64_t vcache_head_stride,
                                    hpc_stream_t stream);
/* FP8 (OCP e4m3fn) variant.  q e4m3 [B*Sq, Hq, 128]; qscale f32 [B*Sq, qscale_pad_stride] (row
 * b*Sq+s, column q head); quant_type 1 (QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR): kscale f32[1],
 * vscale f32[1]; quant_type 0 (QPERTOKEN_PERHEAD_KPERTOKEN_PERHEAD_VPERHEAD): kscale_ptr = base of
 * the K-scale rows that follow the block_size token rows of every K page (row r of head h holds
 * the fp32 scales of tokens 32r..32r+31 as 128 raw bytes; byte strides given explicitly - the
 * reference reads them through a TMA view, sm90/dynamic/...qkpertoken..._dynamic.cu:84-91),
 * vscale f32[Hkv].  Numerics: P~ = e4m3(256 * 2^(s - running max)), O = sum(P~ V)/sum(p) * vscale/256.
 * num_seq_q <= 4.  block_size 16/32/64 for quant_type 1, 32/64 for quant_type 0.
 * num_seq_kvcache_ptr (device int32 [num_batch]) / new_kv_included as in the reference launcher
 * (decode.h:27-35): with them, NHD pages (adjacent kv heads 128 bytes apart), <= 16 q rows per kv head and
 * an even kv head count take the second-generation kernel (attention_decode_v2.hip: 256 contiguous bytes per
 * row and load - two heads of a token - deep prefetch, the schedule planned in-kernel from the lengths in the
 * closed form of the scheduler above: of the task map that path consumes header int 6 = the scheduler call's
 * min_process_len - a workgroup's range is never shorter than that many KV tokens - while the map's bins and
 * split decisions do not apply there; since round 6 per-token K scales on NHD pages run there too, and calls with
 * 17 ... 32 q rows per kv head - speculative steps, num_seq_q 3 / 4 at 8 q heads per kv head - run the same pipeline with ONE
 * kv head per workgroup, on NHD and HND pages, both quant types, pages of 32 / 64 tokens); with <= 16 q rows an odd kv head
 * count - incl. a single kv head - and HND pages run the first-generation kernel from the task map;
 * num_seq_kvcache_ptr may be NULL, then the task map drives the first-generation kernel as for bf16. */
int hpc_attention_decode_fp8_async(void* y_ptr, void* workspace, const int* task_map_ptr,
                                   const void* q_ptr, const void* kcache_ptr,
                                   const void* vcache_ptr, const int* block_ids_ptr,
                                   const int* num_seq_kvcache_ptr, const float* qscale_ptr,
                                   const void* kscale_ptr, const float* vscale_ptr,
                                   int new_kv_included, int quant_type, int num_bins,
                                   int num_batch, int num_seq_q, int num_head_q, int num_head_kv,
                                   int num_dim_qk, int num_dim_v, int block_size,
                                   int num_seq_max_blocks, int qscale_pad_stride, int ldY, int ldQ,
                                   int64_t kcache_block_stride, int64_t kcache_token_stride,
                                   int64_t kcache_head_stride, int64_t vcache_block_stride,
                                   int64_t vcache_token_stride, int64_t vcache_head_stride,
                                   int64_t kscale_block_stride, int64_t kscale_row_stride,
                                   int64_t kscale_head_stride, hpc_stream_t stream);

/* ---- grouped FP8 GEMM with 128-block scales -------------------------------------------------------
 * reference: group_gemm_blockwise_fp8_async, src/group_gemm/group_gemm.h:12-29
 *            (kernel src/group_gemm/kernels.cuh:532-892; scatter-A variant cp_async/group_gemm_fp8_scatter.cu).
 * Y[m, n] = bf16( sum_kb (sum_{k in kb} X[row(m),k] W[g,n,k]) * xs(m,kb) * ws[g, n/128, kb] ) for the
 * seqlens[g] rows starting at cu_seqlens[g].  x e4m3 [rows, k]; w e4m3 [G, n, k]; ws f32
 * [G, n/128, num_block_k_pad4]; y bf16 [m, n].  n, k multiples of 128.
 * row_index (nullable): x / xs row of output row m (gather-free MoE), else row(m) = m.
 * xs addressing in floats: xs[term * xscale_row_stride + kb * xscale_kb_stride] with
 *   term = row(m)                       when col_base == NULL  (row-major [rows, k/128]: strides k/128, 1)
 *   term = col_base[g]*tile_m + slot    when col_base != NULL  (reference layout [k/128, m_pad],
 *                                        col_base = cu_tiles: strides 1, m_pad).
 * cu_tiles128_ptr (nullable): exclusive scan of ceil(seqlens/128), [G+1] (hpc_moe_tiles_async with
 * tile_m = 128); when given and groups are large (> 32 rows on average) the MFMA-bound 128x128-tile
 * kernel is used instead of the weight-streaming one. */
int hpc_group_gemm_blockwise_fp8_async(void* y_ptr, const void* x_ptr, const void* w_ptr,
                                       const void* seqlens_ptr, const void* cu_seqlens_ptr,
                                       const void* xscale_ptr, const void* wscale_ptr,
                                       const void* row_index_ptr, const void* col_base_ptr,
                                       int num_group, int m, int n, int k, int num_block_k_pad4,
                                       int tile_m, int64_t xscale_row_stride,
                                       int64_t xscale_kb_stride, const void* cu_tiles128_ptr,
                                       hpc_stream_t stream);
/* 1 when a caller of the grouped GEMMs (either scale kind) that does not have cu_tiles128 should compute it for a call of m
 * rows in num_group groups - groups long enough for a tiled kernel -, 0 when the call streams either way. */
int hpc_group_gemm_scan_wanted(int num_group, int m);

/* ---- fused MoE pieces ---------------------------------------------------------------------------
 * reference: src/fuse_moe/fuse_moe.h:15-62 (count_and_gather_async / blockwise_count_and_gather_async,
 *            reduce_async, fuse_moe_blockwise_async), src/activation/activation.h:15-53.
 * hpc_moe_count_and_slot_async: seqlens[e], cu_seqlens[E+1], tiles[e] = ceil(seqlens/tile_m),
 *   cu_tiles[E+1], topk_pos[T,k] (stable arrival order, -1 for experts outside
 *   [rank_ep*E, (rank_ep+1)*E)), row_index[pos] = token.  All int32 device buffers.
 * hpc_moe_tiles_async: tiles / cu_tiles from seqlens only.
 * hpc_moe_gather_blockwise_async: x_gathered[pos] = x[token]; xscale_t[kb][cu_tiles[e]*tile_m+slot].
 * hpc_act_mul_and_blockwise_quant_async: gate_up bf16 [rows, 2*I] -> out e4m3 [rows, I],
 *   out_scale[r*scale_row_stride + jb*scale_block_stride] (r = row_to_col[row] or row); rows =
 *   min(*num_rows_ptr, max_rows) when num_rows_ptr != NULL (device int).
 * hpc_moe_reduce_async: y[t] = bf16(sum_j topk_scale[t,j]*x[topk_pos[t,j]] + shared[t]). */
int hpc_moe_count_and_slot_async(const void* topk_ids, int num_tokens, int num_topk, int num_expert,
                                 int rank_ep, int tile_m, void* seqlens, void* cu_seqlens,
                                 void* tiles, void* cu_tiles, void* topk_pos, void* row_index,
                                 hpc_stream_t stream);
int hpc_moe_tiles_async(const void* seqlens, int num_group, int tile_m, void* tiles, void* cu_tiles,
                        hpc_stream_t stream);
int hpc_moe_gather_blockwise_async(const void* x, const void* x_scale, const void* topk_ids,
                                   const void* topk_pos, const void* cu_seqlens,
                                   const void* cu_tiles, int num_tokens, int num_topk,
                                   int num_expert, int rank_ep, int hidden, int tile_m, int m_pad,
                                   void* x_gathered, void* xscale_t, hpc_stream_t stream);
int hpc_act_mul_and_blockwise_quant_async(void* out_ptr, void* out_scale_ptr, const void* gate_up_ptr,
                                          const void* num_rows_ptr, int max_rows,
                                          int intermediate_size, int64_t scale_row_stride,
                                          int64_t scale_block_stride, const void* row_to_col_ptr,
                                          hpc_stream_t stream);
int hpc_moe_reduce_async(void* y_ptr, const void* x_ptr, const void* topk_pos_ptr,
                         const void* topk_scale_ptr, const void* shared_output_ptr, int num_tokens,
                         int num_topk, int hidden_size, hpc_stream_t stream);
/* Whole blockwise pipeline (count/slot -> gate_up GEMM -> SiLU*up + quant -> down GEMM -> reduce);
 * `workspace` >= hpc_fuse_moe_blockwise_workspace_bytes(...) bytes, uninitialised.
 * intermediate_size2 = gate_up_weight.size(1) = 2*I (as in the reference entry, fuse_moe/entry.cc:520). */
int64_t hpc_fuse_moe_blockwise_workspace_bytes(int num_tokens, int num_topk, int hidden_size,
                                               int intermediate_size2, int num_expert);
int hpc_fuse_moe_blockwise_async(void* y_ptr, void* workspace, const void* x_ptr,
                                 const void* x_scale_ptr, const void* gate_up_weight_ptr,
                                 const void* gate_up_weight_scale_ptr, const void* down_weight_ptr,
                                 const void* down_weight_scale_ptr, const void* topk_ids_ptr,
                                 const void* topk_scale_ptr, const void* shared_output_ptr,
                                 int num_tokens, int hidden_size, int intermediate_size2,
                                 int num_topk, int num_expert_total, int num_expert,
                                 int gate_up_ws_pad4, int down_ws_pad4, int rank_ep,
                                 hpc_stream_t stream);

/* ---- MXFP4 weights x e4m3 activations (W4A8), decode steps (ours: no reference counterpart; csrc/group_gemm_mxfp4.hip) ----
 * The statement is tests/mxfp4_ref.py.  For the seqlens[g] output rows r starting at cu_seqlens[g], with row(r) = row_index[r] when
 * row_index is given (gather-free MoE: the token) and r otherwise:
 *   P[r, n, kb] = sum over the 128 k of block kb of x[row(r), k] * e2m1(weight[g, n, k]) * 2^(weight_scale[g, n, k / 32] - 127)
 *   tot = fmaf(P[r, n, kb], x_scale[row(r), kb], tot), kb ascending, fp32;   y[r, n] = bf16_rne(tot)
 * x e4m3 [x_rows, k] and x_scale f32 [x_rows, k / 128], both row-major (the pair hpc_blockwise_fp8_quant_async writes); weight
 * uint8 [G, n, k / 2] in checkpoint layout, two e2m1 codes per byte, even k in the low nibble; weight_scale uint8 [G, n, k / 32],
 * e8m0 (byte 255, NaN, is unspecified); y bf16 [m, n].  k % 128 == 0, n % 64 == 0, n * k / 2 and x_rows * k <= 0xfffffff0,
 * num_group <= 65535 (HPC_ERR_UNSUPPORTED otherwise, as for a pointer that is not 16-byte aligned); null pointers, sizes below
 * zero, num_group, n or k of zero and x_rows < m without a row_index are HPC_ERR_INVALID.  m == 0 launches nothing; an empty
 * group costs nothing but its workgroups' first load.  A pass over a group's weights serves 16 / 32 / 48 rows, chosen from
 * m / num_group (<= 10 / <= 22 / more); longer groups take several passes - correct at any length, meant for decode steps.
 * hpc_group_gemm_mxfp4_plan gives the rows per pass and the grid of such a call (0 where nothing is launched; any out pointer may
 * be NULL) and returns what the call would for these shapes.  Every check is made on the host before any device call. */
int hpc_group_gemm_mxfp4_plan(int num_group, int m, int x_rows, int n, int k, int* tokens_per_pass, int* grid_x, int* grid_y);
int hpc_group_gemm_mxfp4_async(void* y, const void* x, const float* x_scale, const void* weight, const void* weight_scale,
                               const int* seqlens, const int* cu_seqlens, const int* row_index /* may be NULL */, int num_group,
                               int m, int x_rows, int n, int k, hpc_stream_t stream);
/* The fused MoE on MXFP4 expert weights: hpc_fuse_moe_blockwise_async's pipeline and workspace layout with the GEMM above in both
 * places - count/slot -> gate-up GEMM (rows through row_index, scales by token) -> hpc_act_mul_and_blockwise_quant_async (e4m3 +
 * f32 128-block scales: what the second GEMM takes) -> down GEMM -> reduce.  gate_up_weight uint8 [E, 2I, H / 2] with scales
 * [E, 2I, H / 32], down_weight uint8 [E, H, I / 2] with scales [E, H, I / 32]; hidden % 128 == 0, intermediate_size2 % 256 == 0,
 * num_topk <= 128.  No host sync. */
int64_t hpc_fuse_moe_mxfp4_workspace_bytes(int num_tokens, int num_topk, int hidden_size, int intermediate_size2, int num_expert);
int hpc_fuse_moe_mxfp4_async(void* y_ptr, void* workspace, const void* x_ptr, const void* x_scale_ptr,
                             const void* gate_up_weight_ptr, const void* gate_up_weight_scale_ptr, const void* down_weight_ptr,
                             const void* down_weight_scale_ptr, const void* topk_ids_ptr, const void* topk_scale_ptr,
                             const void* shared_output_ptr, int num_tokens, int hidden_size, int intermediate_size2, int num_topk,
                             int num_expert, int rank_ep, hpc_stream_t stream);

/* Per-tensor FP8 MoE pieces (reference src/fuse_moe/fuse_moe.h:15-40 fuse_moe_async, src/group_gemm/
 * group_gemm.h group_gemm_fp8_async, src/activation/activation.h act_mul_and_quant_async /
 * scaled_fp8_quant_async, cp.async pipeline src/fuse_moe/cp_async/fuse_moe.cu:16-63):
 * Y = bf16((X W^T) * y_scale[g]); n % 64 == 0, k % 64 == 0; x_rows = rows of x (bounds the loads when
 * row_index is used).  act: out = e4m3(silu(gate) * up * scale[0]) with the bf16-rounded multiply of
 * the reference when use_bf16_mul.  The fused per-tensor pipeline uses the same workspace size as the
 * blockwise one (hpc_fuse_moe_blockwise_workspace_bytes with intermediate_size2 rounded up to 256). */
int hpc_group_gemm_pertensor_fp8_async(void* y_ptr, const void* x_ptr, const void* w_ptr,
                                       const void* seqlens_ptr, const void* cu_seqlens_ptr,
                                       const void* yscale_ptr, const void* row_index_ptr, int num_group,
                                       int m, int x_rows, int n, int k, const void* cu_tiles128_ptr,
                                       hpc_stream_t stream);
int hpc_act_mul_and_quant_async(void* out_ptr, const void* gate_up_ptr, const void* scale_ptr,
                                const void* num_rows_ptr, int max_rows, int intermediate_size,
                                int use_bf16_mul, hpc_stream_t stream);
/* out[i] = e4m3(float(in[i]) * (1.0f / scale[0])), saturating, any numel > 0 (reference scaled_fp8_quant_async,
 * src/activation/activation.h + activation.cu:461-505, entry src/activation/entry.cc:158-200).  The reference
 * overloads on the input type; here in_dtype says it: 0 = bf16, 1 = fp16, 2 = fp32. */
int hpc_scaled_fp8_quant_async(void* out_ptr, const void* in_ptr, const void* scale_ptr, int64_t numel,
                               int in_dtype, hpc_stream_t stream);
int hpc_moe_gather_rows_async(const void* x, const void* topk_pos, int num_tokens, int num_topk,
                              int hidden, void* x_gathered, hpc_stream_t stream);
int hpc_fuse_moe_pertensor_async(void* y_ptr, void* workspace, const void* x_ptr,
                                 const void* gate_up_weight_ptr, const void* down_weight_ptr,
                                 const void* gate_up_scale_ptr, const void* down_scale_ptr,
                                 const void* act_and_mul_scale_ptr, const void* topk_ids_ptr,
                                 const void* topk_scale_ptr, const void* shared_output_ptr,
                                 int num_tokens, int hidden_size, int intermediate_size2, int num_topk,
                                 int num_expert, int rank_ep, int use_bf16_mul, hpc_stream_t stream);

/* ---- RoPE + optional QK RMSNorm + paged KV-cache write (producer of the decode-attention inputs) ----
 * reference: rope_norm_store_kv_async / rope_norm_store_kv_fp8_async, src/rope/rope.cu:790-950
 *            (kernels :99, :420), entry src/rope/entry.cc:14-240.
 * qkv bf16 [rows, (Hq + 2*Hkv) * 128]; cos_sin f32 [max_pos, 128] (cos | sin halves, neox pairing);
 * num_seqlen_per_req int32 [num_req] (total length incl. the new tokens), q_index int32 [num_req+1],
 * kvcache_indices int32 [num_req, max_blocks_per_req]; caches [blocks, block_size, Hkv, 128]
 * contiguous inside a block, block stride in elements; out_k / out_v (nullable) bypass the cache
 * ([rows, Hkv, 128]).  qk_norm_policy 0 none / 1 rope then RMSNorm / 2 RMSNorm then rope (eps 1e-6,
 * f32 weights [128]).  The tail of each request's last page and (fp8) its split_k_flag row are zeroed.
 * fp8: q/k/v e4m3; quant_policy 1 = dynamic per-token per-head q scale amax/upper_max written to
 * q_scale (decode [rows, Hq]; prefill [num_req, Hq, max_seqlens_pad]), 2 = static q_scale_inv[0];
 * k, v divided by k_scale[0], v_scale[0].  head dims must be 128. */
int hpc_rope_norm_store_kv_async(void* out_q, void* kcache, void* vcache, void* out_k, void* out_v,
                                 const void* qkv, const void* cos_sin, const void* num_seqlen_per_req,
                                 const void* q_index, const void* kvcache_indices,
                                 const void* q_norm_weight, const void* k_norm_weight,
                                 int64_t kcache_block_stride, int64_t vcache_block_stride, int num_req,
                                 int max_blocks_per_req, int kv_block_size, int num_rows,
                                 int num_q_heads, int num_kv_heads, int qk_head_dim, int v_head_dim,
                                 int is_prefill, int qk_norm_policy, hpc_stream_t stream);
int hpc_rope_norm_store_kv_fp8_async(void* out_q, void* kcache, void* vcache, void* out_k, void* out_v,
                                     void* split_k_flag, void* q_scale, const void* qkv,
                                     const void* cos_sin, const void* num_seqlen_per_req,
                                     const void* q_index, const void* kvcache_indices,
                                     const void* q_norm_weight, const void* k_norm_weight,
                                     const void* k_scale, const void* v_scale, const void* q_scale_inv,
                                     float upper_max, int max_seqlens_pad, int64_t kcache_block_stride,
                                     int64_t vcache_block_stride, int num_req, int max_blocks_per_req,
                                     int kv_block_size, int num_rows, int num_q_heads, int num_kv_heads,
                                     int qk_head_dim, int v_head_dim, int is_prefill, int qk_norm_policy,
                                     int quant_policy, hpc_stream_t stream);

/* ---- router GEMM: y = x (w_high + scale * w_low)^T, bf16 operands, fp32 accumulate ----
 * reference: gemm_bf16xfp32_async, src/gemm/gemm.h:13-17 (kernel src/gemm/sm90/gemm_bf16xfp32.cu:88-410,
 * config src/gemm/sm90/entry.cc:23-84).  x [m,k] bf16, w_high / w_low [n,k] bf16, y [m,n] bf16 or fp32.
 * n % 64 == 0, k % 64 == 0.  hpc_gemm_bf16xfp32_plan(m, n, k, use_splitk, ...) gives the split count the library picks
 * (hpc_gemm_bf16xfp32_splits returns the same number) and the arrival counters that go with it; when splits > 1 the
 * caller provides splitk_y (splits*m*n fp32) and split_flag: zeroed int32 [*flag_rows, flag_ld >= *flag_ld] (*flag_ld:
 * the smallest row stride); the counters are zero again when the call retires.  The plan returns the code the launch
 * would refuse the shape with (0: none), its outputs are set either way. */
int hpc_gemm_bf16xfp32_splits(int m, int n, int k, int use_splitk);
int hpc_gemm_bf16xfp32_plan(int m, int n, int k, int use_splitk, int* splits, int* flag_rows, int* flag_ld);
int hpc_gemm_bf16xfp32_async(void* y, void* splitk_y, void* split_flag, const void* x, const void* w_high,
                             const void* w_low, int m, int n, int k, float scale, int use_fp32_output,
                             int splits, int flag_ld, hpc_stream_t stream);

/* ---- fused softmax + top-k router (the step between the router GEMM and fuse_moe*) ---------------------
 * No reference kernel exists (hpc/gemm.py:16-61 stops at the GEMM; BASELINE north_star names the op); the
 * semantics are pinned to stable PyTorch: ids = the first `topk` entries of a STABLE descending sort of the
 * fp32 logits (ties -> smaller expert id; bit-exact), p = softmax(logits) in fp32,
 * topk_scale = p[ids] (renormalize = 0) or p[ids] / sum(p[ids]) (renormalize = 1), best expert first.
 * logits f32 [num_tokens, ld_logits >= num_expert], 16-byte aligned rows; num_expert % 4 == 0, <= 1024;
 * topk <= 64.  topk_ids int32 [num_tokens, topk], topk_scale f32 [num_tokens, topk] - the tensors
 * hpc_fuse_moe_*_async take. */
int hpc_topk_router_async(int* topk_ids, float* topk_scale, const float* logits, int num_tokens, int num_expert,
                          int64_t ld_logits, int topk, int renormalize, hpc_stream_t stream);

/* ---- group-limited top-k router (DeepSeek-V3 / R1, Kimi-K2, DeepSeek-V2 routing; same place in the chain) ----
 * No reference kernel exists; the semantics are the PyTorch statement tests/grouped_router_ref.py:
 *   s = sigmoid(logits) (scoring_func 1) or softmax(logits) (0), fp32;  c = s + correction_bias (c = s when NULL);
 *   the experts form num_expert_group contiguous groups of group_size = num_expert / num_expert_group; a group's
 *   score is the sum of its two best c with a bias and its best c without; the topk_group best groups stay (ties ->
 *   smaller group id);  ids = the first `topk` entries of a STABLE descending sort of c over the experts of the
 *   groups that stay (ties -> smaller expert id), best first;  topk_scale = s[ids] - the UNBIASED scores -, divided
 *   by (their sum + 1e-20) when renormalize, times routed_scaling_factor.
 * num_expert_group == topk_group keeps every group (one group: plain top-k on c).  A NaN in a row leaves that row's
 * result unspecified, its ids still in [0, num_expert).
 * logits f32 [num_tokens, ld_logits >= num_expert], 16-byte aligned rows; correction_bias f32 [num_expert], 16-byte
 * aligned, or NULL; num_expert % 4 == 0, <= 1024; group_size % 4 == 0; topk <= 64 and <= topk_group * group_size.
 * topk_ids int32 [num_tokens, topk], topk_scale f32 [num_tokens, topk] - the tensors hpc_fuse_moe_*_async take. */
int hpc_grouped_topk_router_async(int* topk_ids, float* topk_scale, const float* logits,
                                  const float* correction_bias /* may be NULL */, int num_tokens, int num_expert,
                                  int64_t ld_logits, int topk, int num_expert_group, int topk_group,
                                  int scoring_func /* 0 softmax, 1 sigmoid */, int renormalize,
                                  float routed_scaling_factor, hpc_stream_t stream);

/* bf16 causal prefill: paged KV cache, and contiguous varlen K/V [total_seq, Hkv, 128] (row strides ldK / ldV
 * elements; every q token attends the keys of its request up to itself).
 * reference: attention_with_kvcache_prefill_bf16_async / attention_prefill_bf16_async (src/attention/prefill/prefill.h,
 * entries src/attention/entry.cc:83-150 and :15-81).  seqlens_kvcache counts the request's q tokens too. */
int hpc_attention_with_kvcache_prefill_bf16_async(
    void* y, const void* q, const void* kcache, const void* vcache, const void* cu_seqlens_q, const void* block_ids,
    const void* seqlens_kvcache, int num_batch, int max_seqlens_q, int num_dim_qk, int num_dim_v, int num_head_q,
    int num_head_kv, int block_size, int num_seq_max_blocks, int ldY, int ldQ, int64_t kcache_block_stride,
    int64_t kcache_token_stride, int64_t kcache_head_stride, int64_t vcache_block_stride,
    int64_t vcache_token_stride, int64_t vcache_head_stride, hpc_stream_t stream);
int hpc_attention_prefill_bf16_async(void* y, const void* q, const void* k, const void* v, const void* cu_seqlens_q,
                                     int num_batch, int max_seqlens_q, int num_dim_qk, int num_dim_v, int num_head_q,
                                     int num_head_kv, int ldY, int ldQ, int ldK, int ldV, hpc_stream_t stream);

/* Block-sparse form (reference attention_with_kvcache_blocksparse_prefill_fp8, src/attention/entry.cc:264-409):
 * block_mask uint8 [B, Hq, ceil(max_seqlens_q/128) = mask_tiles_m, mask_tiles_kv] over 128 (q positions of the
 * request) x 128 (kv tokens) tiles, non-zero = attend; null = dense.  128 % block_size == 0. */
int hpc_attention_with_kvcache_blocksparse_prefill_fp8_async(
    void* y, const void* q, const void* kcache, const void* vcache, const void* qscale, const void* kscale,
    const void* vscale, const void* cu_seqlens_q, const void* block_ids, const void* seqlens_kvcache,
    const void* block_mask, int mask_tiles_m, int mask_tiles_kv, int quant_type, int num_batch, int max_seqlens_q,
    int max_seqlens_q_pad, int num_dim_qk, int num_dim_v, int num_head_q, int num_head_kv, int block_size,
    int num_seq_max_blocks, int ldY, int ldQ, int64_t kcache_block_stride, int64_t kcache_token_stride,
    int64_t kcache_head_stride, int64_t vcache_block_stride, int64_t vcache_token_stride,
    int64_t vcache_head_stride, int64_t kscale_block_stride_bytes, int64_t kscale_row_stride_bytes,
    int64_t kscale_head_stride_bytes, hpc_stream_t stream);

/* Masked (DeepEP-layout) activation + quant: gate_up bf16 [num_expert * rows_per_expert, 2 I]; only the first
 * num_per_expert[e] rows of every expert are computed (others untouched).  Per-tensor form: e4m3(silu(g) u scale[0]);
 * blockwise form: per-128 scale = amax / 448 to out_scale [rows, I/128], q = e4m3(a / (scale + 1e-8)).
 * reference: masked_act_mul_and_quant_async / masked_act_mul_and_blockwise_quant_async (src/activation/activation.h,
 * entry src/activation/entry.cc:50-110). */
int hpc_masked_act_mul_and_quant_async(void* out, const void* gate_up, const void* scale, const void* num_per_expert,
                                       int num_total_tokens, int intermediate_size, int num_tokens_per_expert,
                                       hpc_stream_t stream);
int hpc_masked_act_mul_and_blockwise_quant_async(void* out, void* out_scale, const void* gate_up,
                                                 const void* num_per_expert, int num_total_tokens,
                                                 int intermediate_size, int num_tokens_per_expert,
                                                 hpc_stream_t stream);

/* ---- 128-block e4m3 activation quantisation, alone and behind residual add + RMSNorm: the producers of the
 * (x e4m3 [T, H], x_scale f32 [T, H/128]) pair hpc_fuse_moe_blockwise_async / hpc_group_gemm_blockwise_fp8_async take ----
 * No reference kernel exists; the semantics are the PyTorch statement tests/blockwise_quant_ref.py.  For a row a (values
 * taken to fp32) and each block b of 128 consecutive columns - the arithmetic of the blockwise activation above:
 *   amax = max |a[b*128 : (b+1)*128]|;  scale = amax / 448 (fp32 division) -> output_scale[t, b];
 *   q = e4m3fn(a * (1 / (scale + 1e-8f))), one fp32 multiply, round to nearest even -> output_fp8[t, b*128 ...].
 * An all-zero block gives scale 0 and q 0.  A NaN or Inf in a block leaves that block's q and scale unspecified, other
 * blocks and rows unaffected; fp32 denormal inputs are unspecified.
 *
 * hpc_blockwise_fp8_quant_async: input [num_tokens, hidden] contiguous, in_dtype 0 = bf16, 1 = fp16, 2 = fp32.
 *
 * hpc_fused_rmsnorm_blockwise_quant_async: input bf16 [num_tokens, hidden], weight bf16 [hidden].
 *   h = input, or with residual (bf16 [num_tokens, hidden], IN/OUT) h = bf16(float(input) + float(residual)), stored to
 *   residual and normed as rounded (the order of the fused all-reduce ops);
 *   y = bf16(float(h) * rsqrt(mean(float(h)^2) + eps) * float(weight)), fp32 throughout, rounded once;
 *   (output_fp8, output_scale) = the block quantisation above of the bf16-ROUNDED y, i.e. bit for bit what
 *   hpc_blockwise_fp8_quant_async gives on y;  output_normed (bf16 [num_tokens, hidden], may be NULL) = y, the input of
 *   the router GEMM.  input is never written; the buffers must not overlap.
 *
 * Both: hidden % 128 == 0, 128 <= hidden <= 16384 (-1 otherwise); num_tokens >= 0, 0 launches nothing; input, weight,
 * residual and output_normed 16-byte aligned, output_fp8 8-byte aligned (-1 otherwise); output_fp8 e4m3
 * [num_tokens, hidden], output_scale f32 [num_tokens, hidden / 128] row-major.  Every check is made on the host. */
int hpc_blockwise_fp8_quant_async(void* output_fp8, float* output_scale, const void* input, int in_dtype, int num_tokens,
                                  int hidden, hpc_stream_t stream);
int hpc_fused_rmsnorm_blockwise_quant_async(void* output_fp8, float* output_scale, void* output_normed /* may be NULL */,
                                            const void* input, const void* weight,
                                            void* residual /* in/out, may be NULL */, float eps, int num_tokens,
                                            int hidden, hpc_stream_t stream);

/* ---- dense FP8 linear with 128-block scales for decode batches (ours: no reference counterpart) ----
 * The Q/KV/O projections, dense and shared-expert MLPs and the LM head of a block-scaled FP8 model; the statement is
 * tests/linear_fp8_ref.py, in fp32 or better:
 *   y[m, n] = bf16( sum_kb x_scale[m, kb] * weight_scale[n / 128, kb] * sum_{k in block kb} float(x[m, k]) * float(weight[n, k]) )
 * x e4m3 [m, k] and x_scale f32 [m, k / 128], both row-major (the pair hpc_blockwise_fp8_quant_async writes); weight e4m3
 * [n, k] row-major; weight_scale f32 [ceil(n / 128), k / 128] with ws_row_stride >= k / 128 floats between rows; y bf16
 * [m, n].  k % 128 == 0, n % 64 == 0, 0 <= m <= 256 (prefill-sized calls: hpc_group_gemm_blockwise_fp8_async), n * k and
 * m * k <= 0xfffffff0; x and weight 16-byte, y 8-byte, workspace 16-byte aligned.  m == 0 launches nothing.
 * splits: 0 = the library chooses for the current device, 1 .. max_splits = the caller's count of K slices (every slice keeps
 * a k-block; max_splits = min(16, k / 128)).  With more than one split every slice writes an fp32 partial plane to
 * workspace ([splits, m, n], workspace_bytes >= the plan's) and the last slice to arrive at a (64-token, 64-row) tile - counted
 * on counters, int32 [plan's count], ZERO on entry and zero again on exit - sums the planes in split order: the result for
 * a given (m, n, k, splits, CU count) is bit-identical from call to call.  No workgroup waits for another.
 * hpc_gemm_blockwise_fp8_plan(m, n, k, splits_wanted, cu_count (<= 0: the current device's), ...) gives the split count such
 * a call runs with, max_splits, the workspace bytes and the counter count (both 0 without a split) and returns what the call
 * would: HPC_ERR_UNSUPPORTED for k % 128, n % 64, m > 256, operands beyond 32-bit offsets or planes beyond 0xfffffff0 bytes,
 * HPC_ERR_INVALID for negative sizes and splits beyond max_splits.  hpc_gemm_blockwise_fp8_async adds HPC_ERR_INVALID for
 * null pointers, ws_row_stride < k / 128 and a workspace that is missing or too small, HPC_ERR_UNSUPPORTED for alignment.
 * Every check is made on the host before any device call. */
int hpc_gemm_blockwise_fp8_plan(int m, int n, int k, int splits_wanted, int cu_count, int* splits, int* max_splits,
                                int64_t* workspace_bytes, int* counters);
int hpc_gemm_blockwise_fp8_async(void* y, const void* x, const float* x_scale, const void* weight, const float* weight_scale,
                                 int m, int n, int k, int64_t ws_row_stride, int splits, void* workspace,
                                 int64_t workspace_bytes, void* counters, hpc_stream_t stream);

/* ---- MLA decode attention over the paged latent KV cache, bf16 (csrc/attention_decode_mla.hip) -------------------------------
 * No reference kernel exists; the semantics are the PyTorch statement tests/mla_ref.py (weight-absorbed multi-head latent
 * attention: DeepSeek-V3 / R1, Kimi-K2).  One latent row of 576 bf16 per token (512 compressed KV + 64 RoPE) is the key of every
 * head, its first 512 columns the value.  With L_b = the tokens of request b including the num_seq_q new ones, row (b, s, h) sees
 * tokens j < L_b - num_seq_q + s + 1:
 *   z_j = softmax_scale * sum_{d < 576} q[b * num_seq_q + s, h, d] * c_b[j, d]
 *   out[b * num_seq_q + s, h, :] = bf16( sum_j softmax(z)_j * c_b[j, :512] )     lse[b * num_seq_q + s, h] = log sum_j exp(z_j)
 * q bf16 [num_batch * num_seq_q, num_head, 576] contiguous; ckv bf16, token (page, t) at ckv + page * ckv_block_stride +
 * t * ckv_token_stride elements (token stride >= 576, both strides multiples of 8, base 16-byte aligned); block_ids int32
 * [num_batch, max_blocks] (entries past a request's pages are never read); num_seq_kvcache int32 [num_batch] ON THE DEVICE:
 * the tokens before this step, or including the new ones with new_kv_included - no host decision depends on its values.
 * out bf16 [num_batch * num_seq_q, num_head, 512]; lse fp32 [num_batch * num_seq_q, num_head] or NULL.
 * num_head % 16 == 0, 16 .. 128; num_seq_q 1 .. 4; block_size 16 / 32 / 64 / 128; max_blocks * block_size <= 2^30.
 * splits: pieces every request's tokens are cut into (piece length ceil(L_b / splits) rounded up to 64 tokens, computed on the
 * device): 0 = the library chooses for the current device, 1 .. max_splits = the caller's count.  One piece writes out
 * directly; more go through `workspace` (16-byte aligned, never zeroed: pieces past a request's end are neither written nor
 * read) and a merge launch that sums the pieces in piece order - no float atomics, bit-identical from call to call.
 * hpc_attention_decode_mla_plan(num_batch, num_seq_q, num_head, splits_wanted, num_cu (<= 0: the current device's), ...) gives
 * the split count such a call runs with, max_splits and the workspace bytes (0 with one piece) and returns what the call
 * would: HPC_ERR_UNSUPPORTED for the head count and num_seq_q, HPC_ERR_INVALID for negative counts and splits beyond max_splits.
 * hpc_attention_decode_mla_bf16_async adds HPC_ERR_INVALID for null pointers (lse may be NULL), negative max_blocks or block
 * stride and a workspace that is missing or too small, HPC_ERR_UNSUPPORTED for block_size, the strides and alignment.  Every
 * check is made on the host before any device call. */
int hpc_attention_decode_mla_plan(int num_batch, int num_seq_q, int num_head, int splits_wanted, int num_cu, int* splits,
                                  int* max_splits, int64_t* workspace_bytes);
int hpc_attention_decode_mla_bf16_async(void* out, float* lse, const void* q, const void* ckv, const int* block_ids,
                                        const int* num_seq_kvcache, int num_batch, int num_seq_q, int num_head, int block_size,
                                        int max_blocks, int64_t ckv_block_stride, int64_t ckv_token_stride, float softmax_scale,
                                        int new_kv_included, int splits, void* workspace, int64_t workspace_bytes,
                                        hpc_stream_t stream);

/* ---- The FP8 latent KV cache of the MLA ops (the constants: csrc/mla_fp8_format.h) -----------------------------------------
 * One token is a row of 656 bytes: bytes 0 .. 511 hold 512 float8_e4m3fn codes (the normalised compressed KV, column d at byte
 * d), bytes 512 .. 527 four little-endian fp32 scales (scale g belongs to columns 128 g .. 128 g + 127), bytes 528 .. 655 the
 * 64 RoPE'd k_pe columns in bf16, unquantised.  Latent column d < 512 of a token is
 *   c[d] = bf16_rne( fp32(code[d]) * scale[d / 128] )          (one fp32 multiply, one round-to-nearest-even to bf16)
 * for ANY finite non-negative scales; a scale of 0 makes its group zeros; NaN codes and non-finite scales in tokens a row can
 * see are unspecified.  Token (page, t) lies at ckv + page * ckv_block_stride_bytes + t * ckv_token_stride_bytes: token stride
 * >= 656, both strides multiples of 16 bytes, base 16-byte aligned.
 *
 * hpc_attention_decode_mla_fp8_async is hpc_attention_decode_mla_bf16_async on the dequantised cache - every other argument,
 * limit, refusal, the split rule, hpc_attention_decode_mla_plan and the workspace are the bf16 call's; q, out and lse keep
 * their types.  Built from the same kernel source behind the gather, it agrees with the bf16 call on the dequantised cache bit
 * for bit.  HPC_ERR_UNSUPPORTED for a token stride < 656 or not a multiple of 16, a block stride not a multiple of 16, a
 * misaligned base. */
int hpc_attention_decode_mla_fp8_async(void* out, float* lse, const void* q, const void* ckv, const int* block_ids,
                                       const int* num_seq_kvcache, int num_batch, int num_seq_q, int num_head, int block_size,
                                       int max_blocks, int64_t ckv_block_stride_bytes, int64_t ckv_token_stride_bytes,
                                       float softmax_scale, int new_kv_included, int splits, void* workspace,
                                       int64_t workspace_bytes, hpc_stream_t stream);

/* ---- Token-sparse MLA decode attention: each q row attends to the tokens its list names (csrc/attention_decode_mla.hip) ------
 * The attention of a DeepSeek-V3.2 (DSA) decode step; the statement is tests/mla_sparse_ref.py.  indices int32
 * [num_batch * num_seq_q, topk] contiguous ON THE DEVICE: row b * num_seq_q + s lists LOGICAL token positions of request b (what
 * an indexer's top-k yields; the kernel translates pages through block_ids), shared by all heads of that q row.  With
 * vis(b, s) = L_b - num_seq_q + s + 1, entry k is valid when 0 <= idx_k < vis(b, s), idx_k / block_size < max_blocks and its
 * page id lies in [0, num_blocks); every other entry (-1 padding, any negative, a position at or past vis or beyond the table, a
 * poisoned page id) contributes nothing and causes no memory access - every address is checked against a host value.
 *   z_k = softmax_scale * sum_{d < 576} q[b * num_seq_q + s, h, d] * c_b[idx_k, d]        over valid k
 *   out[b * num_seq_q + s, h, :] = bf16( sum_k softmax(z)_k * c_b[idx_k, :512] )         lse = log sum_k exp(z_k)
 * A position listed twice counts twice; a row without a valid entry gets out = 0 and lse = -inf.  The FP8 call applies the same
 * to the dequantised cache, as hpc_attention_decode_mla_fp8_async does, and agrees with the bf16 call on it bit for bit.
 * 1 <= topk <= 65536, any value; num_blocks = pages in the cache's pool; every other argument, limit and refusal is the dense
 * call's, in its order, plus HPC_ERR_INVALID for null indices, topk <= 0 and num_blocks < 0 and HPC_ERR_UNSUPPORTED for
 * topk > 65536.  splits cuts the LIST: piece p covers slots [p * plen, min(topk, (p + 1) * plen)), plen = ceil(topk / splits)
 * rounded up to 64, a host value; pieces that would start at or past topk are not launched, and
 * hpc_attention_decode_mla_sparse_plan reports the effective count in *splits, the workspace bytes that go with it and, where
 * asked (grid and narrow may be NULL), the attention launch's workgroups and whether it takes the 16-head form.  The
 * merge sums the pieces in piece order, skipping a piece that saw no token - no float atomics, bit-identical from call to call.
 * Nothing on the host reads num_seq_kvcache, block_ids or indices. */
int hpc_attention_decode_mla_sparse_plan(int num_batch, int num_seq_q, int num_head, int topk, int splits_wanted, int num_cu,
                                         int* splits, int* max_splits, int64_t* workspace_bytes, int* grid, int* narrow);
int hpc_attention_decode_mla_sparse_bf16_async(void* out, float* lse, const void* q, const void* ckv, const int* block_ids,
                                               const int* num_seq_kvcache, const int* indices, int num_batch, int num_seq_q,
                                               int num_head, int topk, int block_size, int max_blocks, int num_blocks,
                                               int64_t ckv_block_stride, int64_t ckv_token_stride, float softmax_scale,
                                               int new_kv_included, int splits, void* workspace, int64_t workspace_bytes,
                                               hpc_stream_t stream);
int hpc_attention_decode_mla_sparse_fp8_async(void* out, float* lse, const void* q, const void* ckv, const int* block_ids,
                                              const int* num_seq_kvcache, const int* indices, int num_batch, int num_seq_q,
                                              int num_head, int topk, int block_size, int max_blocks, int num_blocks,
                                              int64_t ckv_block_stride_bytes, int64_t ckv_token_stride_bytes,
                                              float softmax_scale, int new_kv_included, int splits, void* workspace,
                                              int64_t workspace_bytes, hpc_stream_t stream);

/* ---- The DSA lightning indexer: FP8 index-key cache, MQA logits, top-k (csrc/mla_indexer.hip) --------------------------------
 * What yields the `indices` of the token-sparse attention above.  No reference kernel; the statement is
 * tests/mla_indexer_ref.py, the layout and the one route csrc/mla_indexer_route.h.
 * The index-key cache: every token has one key of 128 columns shared by all index heads, 128 float8_e4m3fn codes and one fp32
 * scale, column d = fp32(code[d]) * scale for ANY finite non-negative scale.  Page p lies at k_cache + p *
 * k_cache_block_stride_bytes: the codes of its block_size tokens first (token t at byte 128 t), then the block_size fp32 scales
 * (token t at byte 128 * block_size + 4 t).  block_size 16 / 32 / 64 / 128, block stride >= 132 * block_size and a multiple of
 * 16 bytes, base 16-byte aligned; pages are addressed through the block_ids of the latent cache.
 *
 * hpc_mla_indexer_store_k_fp8_async: row r of k (bf16 [num_rows, 128], row stride in elements, a multiple of 8, base 16-byte
 * aligned) is one new token; its request and position are those of hpc_mla_rope_norm_store_kv_async (num_seqlen_per_req,
 * q_index, block_ids ON THE DEVICE, never read by the host).  In fp32: scale = max |k[r]| / 448, code[d] = e4m3fn_sat(k[r, d] *
 * (1 / (scale + 1e-8))) - bit for bit hpc_blockwise_fp8_quant_async on the row.  Only the 128 + 4 bytes of a new token are
 * written; rows of no request, positions beyond the table and page ids outside [0, num_blocks) store nothing.
 *
 * hpc_mla_indexer_logits_fp8_async: q e4m3 [num_batch * num_seq_q, num_head, 128] contiguous, weights fp32 [num_batch *
 * num_seq_q, num_head] (the caller folds the q scales, the softmax scale and num_head^-0.5 into them; they may be negative),
 * both 16-byte aligned; num_head 16 / 32 / 64; num_seq_q 1 .. 4.  With L_b and vis(b, s) = L_b - num_seq_q + s + 1 as in the
 * sparse attention (num_seq_kvcache, new_kv_included), for 0 <= j < min(vis(b, s), max_blocks * block_size):
 *   logits[(b * num_seq_q + s) * logits_row_stride + j] = kscale_b[j] * sum_h weights[., h] * relu( sum_d q[., h, d] * kcode_b[j, d] )
 * and -inf where the page id of j lies outside [0, num_blocks) (its page is never loaded).  Columns at or past that bound are
 * NOT written.  logits fp32, row stride in floats >= max_blocks * block_size <= 2^30.  The head sum has a fixed order, there are
 * no float atomics: the same bits on every call.  Every address is checked against a host value.
 *
 * hpc_mla_indexer_topk_async: a pure selection over row r's columns [0, n_r), n_r = clamp(vis, 0, num_cols): the min(topk, n_r)
 * best positions under (logit descending, position ascending) in torch.topk's order of values (-0.0 == +0.0, NaN above +inf,
 * -inf an ordinary lowest value), written to indices int32 [num_batch * num_seq_q, topk] in ASCENDING position order, then -1.
 * With n_r <= topk the list is 0 .. n_r - 1 and no logit is read; columns at or past n_r are never read.  1 <= topk <= 65536.
 *
 * hpc_mla_indexer_topk_fp8_async: the two back to back through `workspace` (fp32 rows of logits_row_stride floats,
 * workspace_bytes >= the plan's, 4-byte aligned, never zeroed); bit-identical to the two calls.
 *
 * hpc_mla_indexer_plan(..., topk (0: a logits call), num_cu (<= 0: the current device's), ...) gives the logits launch's
 * workgroups and the tokens of a request's context each owns (a host value: 512, doubled up to 8192 while the grid is beyond 16
 * per CU), the top-k launch's workgroups, and the fused call's scratch: its row stride in floats and its bytes.  It returns what
 * the calls would for these arguments.
 * HPC_ERR_INVALID: negative counts, num_seq_q <= 0, a negative block stride, null pointers (with work), max_blocks == 0 with
 * work, a workspace that is missing or too small; HPC_ERR_UNSUPPORTED: num_seq_q > 4, num_head, block_size, topk outside
 * 1 .. 65536, the strides, alignment, sizes beyond int32 or 2^30 columns.  num_batch == 0 (store: num_rows == 0 or num_req == 0)
 * launches nothing.  Every check is made on the host before any device call; hpc_mla_indexer_*_refusal return the refusal of the
 * same call in words, or NULL for a call that is accepted: pure host functions.  Nothing on the host reads lengths or pages. */
int hpc_mla_indexer_plan(int num_batch, int num_seq_q, int num_head, int block_size, int max_blocks, int topk, int num_cu,
                         int* grid, int* chunk, int* topk_grid, int64_t* logits_row_stride, int64_t* workspace_bytes);
const char* hpc_mla_indexer_store_k_fp8_refusal(const void* k_cache, const void* k, const int* num_seqlen_per_req,
                                                const int* q_index, const int* block_ids, int num_rows, int num_req,
                                                int block_size, int max_blocks, int num_blocks,
                                                int64_t k_cache_block_stride_bytes, int64_t k_row_stride);
int hpc_mla_indexer_store_k_fp8_async(void* k_cache, const void* k, const int* num_seqlen_per_req, const int* q_index,
                                      const int* block_ids, int num_rows, int num_req, int block_size, int max_blocks,
                                      int num_blocks, int64_t k_cache_block_stride_bytes, int64_t k_row_stride,
                                      hpc_stream_t stream);
const char* hpc_mla_indexer_logits_fp8_refusal(const float* logits, const void* q, const float* weights, const void* k_cache,
                                               const int* block_ids, const int* num_seq_kvcache, int num_batch, int num_seq_q,
                                               int num_head, int block_size, int max_blocks, int num_blocks,
                                               int64_t k_cache_block_stride_bytes, int64_t logits_row_stride);
int hpc_mla_indexer_logits_fp8_async(float* logits, const void* q, const float* weights, const void* k_cache,
                                     const int* block_ids, const int* num_seq_kvcache, int num_batch, int num_seq_q, int num_head,
                                     int block_size, int max_blocks, int num_blocks, int64_t k_cache_block_stride_bytes,
                                     int64_t logits_row_stride, int new_kv_included, hpc_stream_t stream);
const char* hpc_mla_indexer_topk_refusal(const int* indices, const float* logits, const int* num_seq_kvcache, int num_batch,
                                         int num_seq_q, int64_t num_cols, int topk, int64_t logits_row_stride);
int hpc_mla_indexer_topk_async(int* indices, const float* logits, const int* num_seq_kvcache, int num_batch, int num_seq_q,
                               int64_t num_cols, int topk, int64_t logits_row_stride, int new_kv_included, hpc_stream_t stream);
const char* hpc_mla_indexer_topk_fp8_refusal(const int* indices, const void* q, const float* weights, const void* k_cache,
                                             const int* block_ids, const int* num_seq_kvcache, int num_batch, int num_seq_q,
                                             int num_head, int block_size, int max_blocks, int num_blocks,
                                             int64_t k_cache_block_stride_bytes, int topk, const void* workspace,
                                             int64_t workspace_bytes);
int hpc_mla_indexer_topk_fp8_async(int* indices, const void* q, const float* weights, const void* k_cache, const int* block_ids,
                                   const int* num_seq_kvcache, int num_batch, int num_seq_q, int num_head, int block_size,
                                   int max_blocks, int num_blocks, int64_t k_cache_block_stride_bytes, int topk,
                                   int new_kv_included, void* workspace, int64_t workspace_bytes, hpc_stream_t stream);

/* ---- DSA prefill: the indexer and the token-sparse attention over a ragged chunk (csrc/mla_indexer_prefill.hip) ---------------
 * What the calls above are for a decode step, for a prompt chunk whose requests have any number of rows.  The row rule is the
 * writers' (hpc_mla_rope_norm_store_kv_async, hpc_mla_indexer_store_k_fp8_async): row r of the chunk belongs to the last request
 * b with q_index[b] <= r, at pos = num_seqlen_per_req[b] - (q_index[b + 1] - r); num_seqlen_per_req int32 [num_req] are total
 * lengths INCLUDING the chunk's tokens, q_index int32 [num_req + 1], block_ids int32 [num_req, max_blocks], all ON THE DEVICE and
 * never read by the host.  A row at or past q_index[num_req] or with pos < 0 is a row of no request; a live row sees
 * vis(r) = min(pos + 1, max_blocks * block_size) tokens: causal inside the chunk, all of the cached context before it.  The
 * statement is the decode statement on the expanded form (every row a one-row request of length pos + 1):
 * tests/mla_indexer_prefill_ref.py.
 *
 * hpc_mla_indexer_logits_prefill_fp8_async: q e4m3 [num_rows, num_head, 128] and weights fp32 [num_rows, num_head] hold the
 * chunk's rows row_begin .. row_begin + num_rows - 1; logits row r of the CALL (row row_begin + r of the chunk) gets the formula
 * of hpc_mla_indexer_logits_fp8_async for 0 <= j < vis and, bit for bit, the values of that call on the expanded form; columns
 * at or past vis and rows of no request are NOT written; -inf where the page id lies outside [0, num_blocks).  A key tile is
 * loaded once per tile of 16 rows.
 * hpc_mla_indexer_topk_prefill_async: hpc_mla_indexer_topk_async with n_r = min(vis(row_begin + r), num_cols); a row of no
 * request gets all -1.
 * hpc_mla_indexer_topk_prefill_fp8_async: the two over slabs of scratch_rows rows (0: what fits 256 MiB of scratch) through
 * `workspace` (fp32 [slab_rows, max_blocks * block_size], never zeroed); bit-identical to the two calls over the whole chunk
 * whatever the slab.  The slab count is a host value.
 * hpc_mla_indexer_prefill_plan(..., topk (0: a logits call), scratch_rows, num_cu (<= 0: the current device's), ...) gives the
 * row tile, the logits grid of a call over num_rows rows (ceil(num_rows / tile) * chunks; 0 without requests), the chunk, the
 * slab, the slab count and the scratch's row stride and bytes; it returns what the calls would.
 * Codes as the decode calls', plus HPC_ERR_INVALID for a negative row_begin or scratch_rows.  num_rows == 0 or num_req == 0
 * launches nothing (nothing is written); a caller's slab of more than 2^40 bytes is HPC_ERR_UNSUPPORTED.  The *_refusal
 * functions are pure host functions.
 *
 * hpc_attention_prefill_mla_sparse_{bf16,fp8}_async: hpc_attention_decode_mla_sparse_{bf16,fp8}_async with q bf16
 * [num_rows, num_head, 576], indices int32 [num_rows, topk] and vis(r) from the row rule; a row of no request is an empty row
 * (out = 0, lse = -inf).  The same kernel, route (num_batch = num_rows, num_seq_q = 1: hpc_attention_decode_mla_sparse_plan
 * sizes the scratch), splits rule, limits and refusals, plus HPC_ERR_INVALID for a null q_index or a negative num_req.
 * As in the other calls of this section num_rows == 0 or num_req == 0 launches nothing and WRITES nothing: a caller of the
 * C-ABI that passes no request fills its own outputs (the torch ops do: lists of -1, out = 0, lse = -inf).  The plan's grid and
 * chunk are those of one logits launch over num_rows rows; the fused call launches the logits once per slab and each launch
 * takes its chunk from its own rows (a partial last slab may take a shorter one; no logit depends on it). */
int hpc_mla_indexer_prefill_plan(int num_rows, int num_req, int num_head, int block_size, int max_blocks, int topk,
                                 int scratch_rows, int num_cu, int* tile, int* grid, int* chunk, int* slab_rows, int* slabs,
                                 int64_t* logits_row_stride, int64_t* workspace_bytes);
const char* hpc_mla_indexer_logits_prefill_fp8_refusal(const float* logits, const void* q, const float* weights,
                                                       const void* k_cache, const int* block_ids, const int* num_seqlen_per_req,
                                                       const int* q_index, int num_rows, int num_req, int row_begin, int num_head,
                                                       int block_size, int max_blocks, int num_blocks,
                                                       int64_t k_cache_block_stride_bytes, int64_t logits_row_stride);
int hpc_mla_indexer_logits_prefill_fp8_async(float* logits, const void* q, const float* weights, const void* k_cache,
                                             const int* block_ids, const int* num_seqlen_per_req, const int* q_index, int num_rows,
                                             int num_req, int row_begin, int num_head, int block_size, int max_blocks,
                                             int num_blocks, int64_t k_cache_block_stride_bytes, int64_t logits_row_stride,
                                             hpc_stream_t stream);
const char* hpc_mla_indexer_topk_prefill_refusal(const int* indices, const float* logits, const int* num_seqlen_per_req,
                                                 const int* q_index, int num_rows, int num_req, int row_begin, int64_t num_cols,
                                                 int topk, int64_t logits_row_stride);
int hpc_mla_indexer_topk_prefill_async(int* indices, const float* logits, const int* num_seqlen_per_req, const int* q_index,
                                       int num_rows, int num_req, int row_begin, int64_t num_cols, int topk,
                                       int64_t logits_row_stride, hpc_stream_t stream);
const char* hpc_mla_indexer_topk_prefill_fp8_refusal(const int* indices, const void* q, const float* weights, const void* k_cache,
                                                     const int* block_ids, const int* num_seqlen_per_req, const int* q_index,
                                                     int num_rows, int num_req, int num_head, int block_size, int max_blocks,
                                                     int num_blocks, int64_t k_cache_block_stride_bytes, int topk, int scratch_rows,
                                                     const void* workspace, int64_t workspace_bytes);
int hpc_mla_indexer_topk_prefill_fp8_async(int* indices, const void* q, const float* weights, const void* k_cache,
                                           const int* block_ids, const int* num_seqlen_per_req, const int* q_index, int num_rows,
                                           int num_req, int num_head, int block_size, int max_blocks, int num_blocks,
                                           int64_t k_cache_block_stride_bytes, int topk, int scratch_rows, void* workspace,
                                           int64_t workspace_bytes, hpc_stream_t stream);
int hpc_attention_prefill_mla_sparse_bf16_async(void* out, float* lse, const void* q, const void* ckv, const int* block_ids,
                                                const int* num_seqlen_per_req, const int* q_index, const int* indices,
                                                int num_rows, int num_req, int num_head, int topk, int block_size, int max_blocks,
                                                int num_blocks, int64_t ckv_block_stride, int64_t ckv_token_stride,
                                                float softmax_scale, int splits, void* workspace, int64_t workspace_bytes,
                                                hpc_stream_t stream);
int hpc_attention_prefill_mla_sparse_fp8_async(void* out, float* lse, const void* q, const void* ckv, const int* block_ids,
                                               const int* num_seqlen_per_req, const int* q_index, const int* indices, int num_rows,
                                               int num_req, int num_head, int topk, int block_size, int max_blocks, int num_blocks,
                                               int64_t ckv_block_stride_bytes, int64_t ckv_token_stride_bytes, float softmax_scale,
                                               int splits, void* workspace, int64_t workspace_bytes, hpc_stream_t stream);

/* ---- The indexer's front end: key LayerNorm + RoPE + Hadamard rotation + FP8 quant + store, q likewise (csrc/mla_indexer_prep.hip)
 * What runs between a layer's wq_b / wk / weights_proj GEMMs and hpc_mla_indexer_topk_fp8_async, in one launch.  No reference
 * kernel; the statement is tests/mla_indexer_prep_ref.py, the host rule csrc/mla_indexer_route.h (mla_indexer_prep_route).
 * Row r of k (bf16 [num_rows, 128], row stride in elements) is one new token; its request and position are those of
 * hpc_mla_indexer_store_k_fp8_async.  Everything in fp32 with ONE rounding to bf16, after the rotation:
 *   n = (k[r] - mean) / sqrt(var + eps) * k_norm_weight + k_norm_bias (biased variance over the 128 columns),
 *   n[:64] = rot(n[:64], cos_sin[pos]) (rot and the table [max_pos, 64] of hpc_mla_rope_norm_store_kv_async, on the FIRST 64
 *   columns; interleaved 0 pairs i with i + 32), kr = bf16(H128(n) * rotate_scale), H128 the Walsh-Hadamard transform in
 *   Sylvester order; kr goes into the cache exactly as hpc_mla_indexer_store_k_fp8_async(kr) writes it, and to out_k (bf16
 *   [num_rows, 128] contiguous) when given.  k_cache NULL: out_k alone (block_size, the block stride, block_ids not looked at).
 * With q (bf16 [num_rows, num_head, 128], row and head strides in elements; num_head 16 / 32 / 64): qr = bf16(H128(q[r, h] with
 *   its first 64 columns turned) * rotate_scale) -> out_q_rot (bf16, contiguous, optional); its 128-block quantisation -> out_q
 *   (e4m3 codes, contiguous) and out_weights[r, h] = fp32(fp32(head_weights[r, h] * scale) * weight_scale), weight_scale =
 *   float(softmax_scale * num_head^-0.5) formed by the caller in double (head_weights fp32 or bf16 [num_rows, num_head]
 *   contiguous): the q / weights of hpc_mla_indexer_logits_fp8_async.
 *   q NULL: the key alone; num_head, head_weights, weight_scale are not looked at and the q outputs must be NULL.
 * pow2_scale != 0: both quantisers take the smallest power of two >= amax / 448 as the scale (exponent field + 1 when the mantissa
 *   is not zero, clamped to [1, 254]) and code = e4m3(x / scale), exactly.
 * Rows of no request store nothing and are zeros in every output; a page id outside [0, num_blocks) and a position beyond the
 * table store nothing; the cos_sin row is clamped to max_pos - 1; only the 128 + 4 bytes of a new token are written.
 * HPC_ERR_INVALID: negative counts, no destination for the key, q outputs or head_weights without q, q without head_weights / a
 * finite weight_scale / out_q / out_weights, null pointers with work, max_pos == 0 with work, a negative eps or block stride;
 * HPC_ERR_UNSUPPORTED: num_head, block_size, strides that are no multiple of 8 elements or too short, misaligned bases,
 * num_rows * (1 + num_head) beyond int32.  num_rows == 0 or num_req == 0 launches nothing.  hpc_mla_indexer_prep_fp8_refusal
 * returns the refusal of the same call in words, or NULL: a pure host function.  Nothing on the host reads a device value; no
 * atomics, a fixed butterfly order: the same bits on every call. */
const char* hpc_mla_indexer_prep_fp8_refusal(const void* k_cache, const void* out_k, const void* out_q, const float* out_weights,
                                             const void* out_q_rot, const void* k, const void* q, const void* head_weights,
                                             const float* k_norm_weight, const float* k_norm_bias, const float* cos_sin,
                                             const int* num_seqlen_per_req, const int* q_index, const int* block_ids,
                                             int num_rows, int num_req, int num_head, int block_size, int max_blocks,
                                             int num_blocks, int max_pos, int64_t k_cache_block_stride_bytes,
                                             int64_t k_row_stride, int64_t q_row_stride, int64_t q_head_stride,
                                             int head_weights_bf16, float weight_scale, float eps, float rotate_scale);
int hpc_mla_indexer_prep_fp8_async(void* k_cache, void* out_k, void* out_q, float* out_weights, void* out_q_rot, const void* k,
                                   const void* q, const void* head_weights, const float* k_norm_weight, const float* k_norm_bias,
                                   const float* cos_sin, const int* num_seqlen_per_req, const int* q_index, const int* block_ids,
                                   int num_rows, int num_req, int num_head, int block_size, int max_blocks, int num_blocks,
                                   int max_pos, int64_t k_cache_block_stride_bytes, int64_t k_row_stride, int64_t q_row_stride,
                                   int64_t q_head_stride, int head_weights_bf16, float weight_scale, float eps,
                                   float rotate_scale, int interleaved, int pow2_scale, hpc_stream_t stream);

/* ---- MLA latent-cache write: kv_a RMSNorm + RoPE + paged store, bf16 (csrc/mla_store.hip) ------------------------------------
 * No reference kernel exists; the semantics are the PyTorch statement tests/mla_store_ref.py.  The producer of the cache and of
 * the RoPE columns of q that hpc_attention_decode_mla_bf16_async reads.  Row r of kv_a is one new token; its request b is the
 * last one with q_index[b] <= r and its position pos = num_seqlen_per_req[b] - (q_index[b + 1] - r), as in
 * hpc_rope_norm_store_kv_async; rows at or past q_index[num_req] and rows with pos < 0 belong to no request.  In fp32 with one
 * rounding to bf16:
 *   lat[:512] = kv_a[r, :512] / sqrt(mean(kv_a[r, :512]^2) + eps) * kv_norm_weight
 *   lat[512:] = rot(kv_a[r, 512:576], cos_sin[pos])            out_q_pe[r, h, :] = rot(q_pe[r, h, :], cos_sin[pos])
 *   ckv_cache[block_ids[b, pos / block_size], pos % block_size, :576] = lat    and / or    out_ckv[r, :] = lat
 * rot turns the pair (a, b) into (a cos_i - b sin_i, b cos_i + a sin_i), cos_i = cos_sin[pos, i], sin_i = cos_sin[pos, 32 + i],
 * i < 32; the pair is elements (2i, 2i + 1) with interleaved != 0 (GPT-J style) and (i, i + 32) with 0 (neox).
 * kv_a bf16 [num_rows, 576] and out_ckv bf16 [num_rows, 576] with row strides; q_pe / out_q_pe bf16 [num_rows, num_head, 64]
 * with row and head strides (out_q_pe may be q_pe: in place), both NULL to process the latent rows only; ckv_cache as in
 * hpc_attention_decode_mla_bf16_async (token (page, t) at ckv_cache + page * ckv_block_stride + t * ckv_token_stride); one of
 * ckv_cache and out_ckv may be NULL.  All strides in elements and multiples of 8, the token stride and (with more than
 * one row) the row strides of kv_a and out_ckv >= 576, the head and row strides of q_pe and out_q_pe >= 64 (with more than one
 * head / row), the row stride of out_q_pe >= (num_head - 1) * its head stride + 64, out_q_pe either q_pe itself with q_pe's strides
 * or disjoint from it, every base 16-byte aligned.  cos_sin f32 [max_pos, 64], kv_norm_weight f32 [512], num_seqlen_per_req int32 [num_req], q_index int32
 * [num_req + 1], block_ids int32 [num_req, max_blocks], all ON THE DEVICE and never read by the host.  Only the 576 columns
 * of the new tokens' cells are written in the cache (no tail is cleared); rows of no request store nothing there and are
 * written as zeros in out_ckv and out_q_pe.  The kernel trusts no device value with an address: the table index is clamped to
 * max_pos - 1 (the result of such a row is unspecified), a token is not stored when pos / block_size >= max_blocks or when its
 * page id is outside [0, num_blocks).
 * HPC_ERR_INVALID: null pointers, neither destination, one of q_pe / out_q_pe without the other, negative counts, max_pos 0;
 * HPC_ERR_UNSUPPORTED: num_head outside 1 .. 128, block_size outside 16 / 32 / 64 / 128, the strides, alignment.  num_rows == 0
 * or num_req == 0 launches nothing.  Every check is made on the host before any device call. */
int hpc_mla_rope_norm_store_kv_async(void* ckv_cache, void* out_ckv, void* out_q_pe, const void* kv_a, const void* q_pe,
                                     const float* cos_sin, const float* kv_norm_weight, const int* num_seqlen_per_req,
                                     const int* q_index, const int* block_ids, int num_rows, int num_req, int num_head,
                                     int block_size, int max_blocks, int num_blocks, int max_pos, int64_t ckv_block_stride,
                                     int64_t ckv_token_stride, int64_t kv_a_row_stride, int64_t out_ckv_row_stride,
                                     int64_t q_pe_row_stride, int64_t q_pe_head_stride, int64_t out_q_pe_row_stride,
                                     int64_t out_q_pe_head_stride, float eps, int interleaved, hpc_stream_t stream);
/* The same into the FP8 latent cache described above: arguments, the row-to-position rule, the guards and the refusals are those
 * of hpc_mla_rope_norm_store_kv_async, except that ckv_cache holds 656-byte rows and its two strides are in BYTES (multiples of
 * 16, token stride >= 656).  With lat the bf16-rounded row the bf16 call stores, per group g of 128 columns and in fp32:
 *   scale[g] = max |lat[128 g .. 128 g + 127]| / 448        code[d] = e4m3fn_sat( lat[d] * (1 / (scale[d / 128] + 1e-8)) )
 * and bytes 528 .. 655 = lat[512:] in bf16.  Only those 656 bytes of a new token's cell are written.  out_ckv and out_q_pe stay
 * bf16 and are bit-identical to the bf16 call's. */
int hpc_mla_rope_norm_store_kv_fp8_async(void* ckv_cache, void* out_ckv, void* out_q_pe, const void* kv_a, const void* q_pe,
                                         const float* cos_sin, const float* kv_norm_weight, const int* num_seqlen_per_req,
                                         const int* q_index, const int* block_ids, int num_rows, int num_req, int num_head,
                                         int block_size, int max_blocks, int num_blocks, int max_pos,
                                         int64_t ckv_block_stride_bytes, int64_t ckv_token_stride_bytes, int64_t kv_a_row_stride,
                                         int64_t out_ckv_row_stride, int64_t q_pe_row_stride, int64_t q_pe_head_stride,
                                         int64_t out_q_pe_row_stride, int64_t out_q_pe_head_stride, float eps, int interleaved,
                                         hpc_stream_t stream);

/* ---- MLA prefill attention, non-absorbed form, bf16, with an lse output (csrc/attention_prefill_mla.hip) ----------------------
 * No reference kernel; the statement is tests/mla_prefill_ref.py.  Request b has Sq = cu_seqlens_q[b + 1] - cu_seqlens_q[b] q rows
 * and Lk = cu_seqlens_k[b + 1] - cu_seqlens_k[b] keys (cu_seqlens_k NULL: the cu_seqlens_q array).  Row s sees keys
 * j <= Lk - Sq + s with causal != 0 (bottom-right aligned) and every j < Lk with causal == 0:
 *   z_j = softmax_scale * (q[s, h, :128] . k_nope[j, h] + q[s, h, 128:] . k_pe[j])
 *   out[s, h, :] = bf16( softmax(z) @ v[:, h] )          lse[s, h] = log sum_j exp(z_j)         (fp32, natural log)
 * A row that sees no key (Lk == 0, or Lk - Sq + s < 0) writes zeros and -inf.  q bf16 [Tq, num_head, 192] (columns 128..191 with
 * RoPE applied), k_nope / v bf16 [Tk, num_head, 128], k_pe bf16 [Tk, 64] (one head shared by all), each with row (and head)
 * strides in elements; out bf16 [Tq, num_head, 128] and lse fp32 [Tq, num_head] contiguous, lse may be NULL.  cu_seqlens_* int32
 * [num_batch + 1] ON THE DEVICE: only max_seqlens_q (the grid) is read on the host, max_seqlens_k (-1: not given) is checked for
 * being there.  Reads are bounded by the rows of the request that exist; no float atomics, bit-identical from call to call.
 * Refusals, in this order: HPC_ERR_INVALID for a null out, q, k_nope, k_pe, v or cu_seqlens_q; HPC_ERR_UNSUPPORTED for a base that
 * is not 16-byte aligned or a stride that is no multiple of 8; HPC_ERR_UNSUPPORTED for a q stride under 192, a k_nope / v stride
 * under 128, a k_pe row stride under 64; HPC_ERR_INVALID for cu_seqlens_k with max_seqlens_k < 0; HPC_ERR_INVALID for a negative
 * num_batch or max_seqlens_q, num_head <= 0 or a softmax_scale that is not positive and finite; HPC_ERR_UNSUPPORTED for num_head
 * or num_batch beyond 65535 or a row stride beyond 2^25.  num_batch == 0 or max_seqlens_q == 0 launches nothing.  Every check is
 * made on the host before any device call (csrc/attention_prefill_mla_route.h). */
int hpc_attention_prefill_mla_bf16_async(void* out, float* lse, const void* q, const void* k_nope, const void* k_pe, const void* v,
                                         const int* cu_seqlens_q, const int* cu_seqlens_k, int num_batch, int num_head,
                                         int max_seqlens_q, int max_seqlens_k, int64_t q_row_stride, int64_t q_head_stride,
                                         int64_t k_row_stride, int64_t k_head_stride, int64_t k_pe_row_stride, int64_t v_row_stride,
                                         int64_t v_head_stride, float softmax_scale, int causal, hpc_stream_t stream);

/* ---- merge of two attention states by their log-sum-exps (csrc/merge_attn_states.hip) ------------------------------------------
 * No reference kernel; the statement is tests/mla_prefill_ref.py.  In fp32 with one rounding to bf16, per (row, head):
 *   m = max(la, lb)   wa = exp(la - m)   wb = exp(lb - m)   out = (wa a + wb b) / (wa + wb)   lse = m + log(wa + wb)
 * a side whose lse is -inf passes the other through bit for bit; both -inf: zeros and -inf.  out / out_a / out_b bf16
 * [num_rows, num_head, dim] with row and head strides in elements (multiples of 8, >= dim), dim % 8 == 0, dim <= 512; the lse
 * arrays fp32 [num_rows, num_head] contiguous.  out may be out_a (same base and strides) and lse may be lse_a: in place; any
 * other overlap of an output with an input is HPC_ERR_UNSUPPORTED, like dim, alignment and the strides; null pointers and
 * negative counts are HPC_ERR_INVALID.  num_rows == 0 or num_head == 0 launches nothing. */
int hpc_merge_attn_states_async(void* out, float* lse, const void* out_a, const float* lse_a, const void* out_b, const float* lse_b,
                                int64_t num_rows, int num_head, int dim, int64_t out_row_stride, int64_t out_head_stride,
                                int64_t a_row_stride, int64_t a_head_stride, int64_t b_row_stride, int64_t b_head_stride,
                                hpc_stream_t stream);

/* ---- MLA latent-cache gather: paged latent cache -> contiguous bf16 rows (csrc/mla_gather.hip) -----------------------------------
 * No reference kernel; the statement is tests/mla_gather_ref.py, without a float in it.  The step between the cache and the kv_b
 * projection of a chunked-prefill context pass.  Request b owns output rows cu_seqlens[b] <= r < cu_seqlens[b + 1]; row r is the
 * token at pos = seq_starts[b] + (r - cu_seqlens[b]) (seq_starts NULL: zeros):
 *   out[r, :576] = ckv_cache[block_ids[b, pos / block_size], pos % block_size, :576]                       the bits, untouched
 * out bf16 [num_rows, 576] with a row stride in elements (a multiple of 8, >= 576 with more than one row), ckv_cache as in
 * hpc_attention_decode_mla_bf16_async (token (page, t) at ckv_cache + page * ckv_block_stride + t * ckv_token_stride, strides in
 * elements and multiples of 8, token stride >= 576), every base 16-byte aligned.  block_ids int32 [num_req, max_blocks],
 * cu_seqlens int32 [num_req + 1], seq_starts int32 [num_req], all ON THE DEVICE and never read by the host: num_rows is the
 * host's bound on r.  Rows of no request (r < cu_seqlens[0], r >= cu_seqlens[num_req], or outside the range of the request a
 * cu_seqlens that does not ascend leads to) are not written, nor are the bytes between 576 columns and the row stride.  A row
 * of a request whose token cannot be fetched - pos < 0, pos / block_size >= max_blocks, a page id outside [0, num_blocks) - is
 * written as 576 zeros.  The kernel trusts no device value with an address; cache offsets are 64-bit.
 * HPC_ERR_INVALID: negative counts, and with num_rows > 0 and num_req > 0 a null out, ckv_cache, block_ids or cu_seqlens;
 * HPC_ERR_UNSUPPORTED: block_size outside 16 / 32 / 64 / 128, the strides, alignment, num_rows beyond INT32_MAX - 32, strides
 * whose offsets would leave 2^60 bytes.  num_rows == 0 or num_req == 0 launches nothing.  Every check is made on the host
 * before any device call. */
int hpc_mla_gather_ckv_async(void* out, const void* ckv_cache, const int* block_ids, const int* cu_seqlens, const int* seq_starts,
                             int num_rows, int num_req, int block_size, int max_blocks, int num_blocks, int64_t ckv_block_stride,
                             int64_t ckv_token_stride, int64_t out_row_stride, hpc_stream_t stream);
/* The same from the FP8 latent cache described above: ckv_cache holds 656-byte rows and its two strides are in BYTES (multiples
 * of 16, token stride >= 656); everything else, the guards and the refusals are those of hpc_mla_gather_ckv_async.  A fetched
 * row is dequantised as hpc_attention_decode_mla_fp8_async does it, one fp32 multiply and one rounding:
 *   out[r, d] = bf16_rne( fp32(code[d]) * scale[d / 128] ), d < 512        out[r, 512:] = bytes 528 .. 655, untouched */
int hpc_mla_gather_ckv_fp8_async(void* out, const void* ckv_cache, const int* block_ids, const int* cu_seqlens,
                                 const int* seq_starts, int num_rows, int num_req, int block_size, int max_blocks, int num_blocks,
                                 int64_t ckv_block_stride_bytes, int64_t ckv_token_stride_bytes, int64_t out_row_stride,
                                 hpc_stream_t stream);

/* ---- MLA absorb matmuls: W_UK into q, W_UV out of the latent attention output (csrc/mla_absorb.hip) -----------------------------
 * No reference kernel; the statements are tests/mla_absorb_ref.py.  bf16 operands, fp32 accumulation, one rounding:
 *   absorb_q     out[t, h, c] = bf16( sum_{d < 128} q_nope[t, h, d] * w_uk[h, d, c] ),  c < 512
 *   unabsorb_o   o[t, h * 128 + v] = bf16( sum_{c < 512} o_lat[t, h, c] * w_uv[h, v, c] ),  v < 128
 * q_nope [T, H, 128], o_lat [T, H, 512] and absorb_q's out [T, H, 512]: last dim contiguous, row and head strides in elements,
 * multiples of 8 (views such as q[..., :128] of [T, H, 192] and q_abs[..., :512] of [T, H, 576]: the columns outside are
 * neither read nor written).  w_uk / w_uv [H, 128, 512]: last dim contiguous, head and row strides multiples of 8, row
 * stride >= 512 - the two halves of kv_b.view(H, 256, 512).  Every base 16-byte aligned.  unabsorb_o's out: quant == 0: bf16
 * [T, H * 128] with a row stride >= H * 128, a multiple of 8; quant != 0: e4m3fn codes [T, H * 128] and out_scale f32 [T, H],
 * both contiguous (out_row_stride == H * 128), the rule of hpc_blockwise_fp8_quant_async per (token, head) on the bf16-rounded
 * o: scale = amax / 448, code = e4m3fn(o * (1 / (scale + 1e-8))) - bit for bit that op on the quant == 0 output.
 * 1 <= H <= 128; num_tokens == 0 launches nothing; offsets are 64-bit.  No workspace, no atomics: the same bits on every call.
 * Every check is made on the host before any device call (csrc/mla_absorb_route.h).  HPC_ERR_INVALID: a negative
 * num_tokens, null pointers (num_tokens > 0), out_scale without quant; HPC_ERR_UNSUPPORTED: H, the strides, alignment, an
 * output that shares bytes with an input.  hpc_mla_*_refusal return the refusal of the same call in words, one message per
 * rule, or NULL for a call that is accepted: pure host functions. */
const char* hpc_mla_absorb_q_refusal(const void* out, const void* q_nope, const void* w_uk, int64_t num_tokens, int num_head,
                                     int64_t q_row_stride, int64_t q_head_stride, int64_t w_head_stride, int64_t w_row_stride,
                                     int64_t out_row_stride, int64_t out_head_stride);
int hpc_mla_absorb_q_async(void* out, const void* q_nope, const void* w_uk, int64_t num_tokens, int num_head,
                           int64_t q_row_stride, int64_t q_head_stride, int64_t w_head_stride, int64_t w_row_stride,
                           int64_t out_row_stride, int64_t out_head_stride, hpc_stream_t stream);
const char* hpc_mla_unabsorb_o_refusal(const void* out, const float* out_scale, const void* o_lat, const void* w_uv,
                                       int64_t num_tokens, int num_head, int64_t o_row_stride, int64_t o_head_stride,
                                       int64_t w_head_stride, int64_t w_row_stride, int64_t out_row_stride, int quant);
int hpc_mla_unabsorb_o_async(void* out, float* out_scale, const void* o_lat, const void* w_uv, int64_t num_tokens, int num_head,
                             int64_t o_row_stride, int64_t o_head_stride, int64_t w_head_stride, int64_t w_row_stride,
                             int64_t out_row_stride, int quant, hpc_stream_t stream);

/* x_scale [rows, n = K/128] -> transposed, tile-padded, compact [n, m] layout that
 * hpc_group_gemm_blockwise_fp8_async reads (DeepEP-format inputs).
 * reference: reformat_x_scale_async, src/group_gemm/group_gemm.h:27-29 (entry src/group_gemm/entry.cc:170-222). */
int hpc_reformat_x_scale_async(void* output, const void* x_scale, const void* seqlens, const void* cu_seqlens,
                               int num_group, int m, int n, int tilem, hpc_stream_t stream);

/* ---- paged-KV causal prefill attention, FP8 ----
 * reference: attention_with_kvcache_prefill_{qpertoken_perhead_kvpertensor,qkpertoken_perhead_vperhead}_fp8_async
 *            (src/attention/prefill/prefill.h, entry src/attention/entry.cc:152-262).
 * q e4m3 [total_q, Hq, 128]; caches as in hpc_attention_decode_fp8_async (strides in elements); qscale f32
 * [B, Hq, max_seqlens_q_pad]; cu_seqlens_q int32 [B+1]; seqlens_kvcache int32 [B] = cached tokens INCLUDING
 * the request's q tokens (q row s attends keys j <= L_b - Sq_b + s); y bf16 [total_q, Hq, 128].
 * quant_type 1: kscale/vscale f32 [1]; 0: kscale = K-scale tail rows of the cache (strides in bytes),
 * vscale f32 [Hkv].  head dims 128, page size 16/32/64, Hq/Hkv in {1,2,4,8,16}. */
int hpc_attention_with_kvcache_prefill_fp8_async(
    void* y, const void* q, const void* kcache, const void* vcache, const void* qscale, const void* kscale,
    const void* vscale, const void* cu_seqlens_q, const void* block_ids, const void* seqlens_kvcache,
    int quant_type, int num_batch, int max_seqlens_q, int max_seqlens_q_pad, int num_dim_qk, int num_dim_v,
    int num_head_q, int num_head_kv, int block_size, int num_seq_max_blocks, int ldY, int ldQ,
    int64_t kcache_block_stride, int64_t kcache_token_stride, int64_t kcache_head_stride,
    int64_t vcache_block_stride, int64_t vcache_token_stride, int64_t vcache_head_stride,
    int64_t kscale_block_stride_bytes, int64_t kscale_row_stride_bytes, int64_t kscale_head_stride_bytes,
    hpc_stream_t stream);

/* ---- Stem block-sparse mask generation (feeds hpc_attention_with_kvcache_blocksparse_prefill_fp8) ----------------
 * Stem block S = 128 tokens, stride R = 16 (16 groups of 8 tokens g, g+16, ..., g+112 per block), head dim 128; only
 * these are supported (-1 otherwise).  Kb_r / Qb_r = ceil(len_r / 128); every output element is written, padding
 * blocks as zeros (kflat, qflat, vbias, mask) or -inf (logits).
 *
 * hpc_stem_oam_prep_paged_kv_async
 *   reference: stem_oam_prep_paged_kv_qpertoken_perhead_kvpertensor_dim128_async (quant_type 1) and
 *   stem_oam_prep_paged_kv_qkpertoken_perhead_vperhead_dim128_async (quant_type 0),
 *   src/stem/stem_oam_prep_paged_kv_dim128.h (entry src/stem/entry.cc:19-110).
 *   kcache / vcache e4m3 [pages, block_size = 32 | 64, Hkv, 128] (strides in elements), kv_indices int32
 *   [B, num_seq_max_blocks], kv_seq_lens int32 [B].  kflat bf16 [B, Hkv, max_num_stem_blocks, 2048]: group g of block
 *   b = sum of kscale_t * K[t] at columns (15 - g) * 128 (reversed group order); v_norm f32 scratch
 *   [B, Hkv, max_num_stem_blocks * 8]: max row norm of vscale * V per 16-token window; vbias f32
 *   [B, Hkv, max_num_stem_blocks] from the per-(request, head) mean / sample std of log(v_norm + 1e-6).
 *   quant_type 1: kscale / vscale f32 [1]; 0: kscale f32 per token at [page, row / 32, head, row % 32] (strides in
 *   f32 elements), vscale f32 [Hkv]. */
int hpc_stem_oam_prep_paged_kv_async(
    void* kflat, void* vbias, void* v_norm, const void* kcache, const void* vcache, const void* kscale,
    const void* vscale, const void* kv_indices, const void* kv_seq_lens, int quant_type, int num_batch, int num_dim_qk,
    int num_dim_v, int num_head_kv, int block_size, int num_seq_max_blocks, int stem_block_size, int stem_stride,
    int max_num_stem_blocks, float lambda_mag, int64_t kcache_block_stride, int64_t kcache_token_stride,
    int64_t kcache_head_stride, int64_t vcache_block_stride, int64_t vcache_token_stride, int64_t vcache_head_stride,
    int64_t kscale_block_stride, int64_t kscale_row_stride, int64_t kscale_head_stride, hpc_stream_t stream);
/* reference: stem_oam_prep_varlen_q_dim128_async, src/stem/stem_oam_prep_varlen_q_dim128.h (entry :114-155).
 * q_fp8 e4m3 [total_q, Hq, 128] (row stride ldQ bytes), qscale f32 [B, Hq, >= max q_len] (strides in elements),
 * cu_seqlens_q int32 [B + 1].  qflat bf16 [B, Hq, max_num_q_blocks, 2048], group g at columns g * 128. */
int hpc_stem_oam_prep_varlen_q_async(void* qflat, const void* q_fp8, const void* qscale, const void* q_seq_lens,
                                     const void* cu_seqlens_q, int num_batch, int num_head_q, int num_dim_qk,
                                     int stem_block_size, int stem_stride, int max_num_q_blocks, int64_t ldQ,
                                     int64_t qscale_batch_stride, int64_t qscale_head_stride, hpc_stream_t stream);
/* reference: stem_oam_gemm_dim128_async, src/stem/stem_oam_gemm_dim128.h (entry :157-222).
 * qflat / kflat / vbias contiguous as produced above; block_logits bf16 [B, Hq, max_num_qb, max_num_kb] =
 * qflat . kflat^T / 64 + vbias[h_q / (Hq / Hkv)], -inf where qb >= Qb_r, kb >= Kb_r or (causal) qb + off < kb with
 * off = (kv_len - q_len + 127) / 128. */
int hpc_stem_oam_gemm_async(void* block_logits, const void* qflat, const void* kflat, const void* vbias,
                            const void* q_seq_lens, const void* kv_seq_lens, int num_batch, int num_head_q,
                            int num_head_kv, int max_num_qb, int max_num_kb, int stem_block_size, int stem_stride,
                            int causal, hpc_stream_t stream);
/* reference: stem_tpd_async, src/stem/stem_tpd.h (entry :224-266).  block_logits bf16 contiguous
 * [B, H, max_Qb, max_Kb <= 32768]; mask uint8 of the same shape: per row < Qb_r the columns < Kb_r whose order key is
 * at or above the exact top-`budget` threshold, plus the first initial_blocks, the window_size blocks ending at the
 * diagonal min(row + off, Kb_r - 1) and the diagonal; 0 elsewhere. */
int hpc_stem_tpd_async(void* mask, const void* block_logits, const void* q_seq_lens, const void* kv_seq_lens,
                       const void* num_prompt_tokens, int num_batch, int num_heads, int max_Qb, int max_Kb,
                       int block_size, float alpha, int initial_blocks, int window_size, float k_block_num_rate_medium,
                       int k_block_num_bias_medium, float k_block_num_rate_large, int k_block_num_bias_large,
                       hpc_stream_t stream);

/* ---- fused sampler (end of the decode step) ----
 * reference: fused_sampler_async / fused_sampler_temperature_async, src/sampler/sampler.h:17-45
 *            (kernels src/sampler/fused_sampler.cu, fused_sampler_temperature.cu; entry src/sampler/entry.cc).
 * logits [B, V] fp32 (dtype 0) or bf16 (1), inner stride 1, row stride in elements; V % 8 == 0, V < 2^20.
 * Pipeline: repetition penalty (bit mask rows selected by slot_id) -> temperature -> [softmax over V,
 * policy 1] -> top-k (k <= max_topk in {32, 64}; 0 / out of range = max_topk) -> [softmax over the top-k,
 * policy 2] -> top-p -> Gumbel-max (gumbel_noise [B, V] fp32, or Philox noise from rng_seed when null) ->
 * token_ids int32 [B] and the sampled token's bit OR-ed into its penalty row.  Ties resolve towards the
 * smaller token id.  workspace: hpc_fused_sampler_workspace_bytes (full sampler) or
 * batch_size * hpc_sampler_segments(V) * 8 bytes (temperature path). */
int hpc_sampler_segments(int vocab_size);
int64_t hpc_fused_sampler_workspace_bytes(int batch_size, int vocab_size, int max_topk);
int hpc_fused_sampler_async(void* token_ids, void* workspace, const void* logits, int logits_dtype,
                            void* penalty_mask, int64_t penalty_mask_row_bytes, const void* slot_id,
                            const void* repetition_penalty, float repetition_penalty_val,
                            const void* temperature, float temperature_val, int softmax_policy,
                            const void* topk, int topk_int_bytes, int topk_val, const void* topp,
                            float topp_val, const void* gumbel_noise, int batch_size, int vocab_size,
                            int64_t logits_row_stride, int max_topk, uint64_t rng_seed, hpc_stream_t stream);
int hpc_fused_sampler_temperature_async(void* token_ids, void* workspace, const void* logits,
                                        int logits_dtype, int64_t logits_row_stride, const void* temperature,
                                        float temperature_val, const void* gumbel_noise,
                                        const void* draft_token_ids, int batch_size, int vocab_size,
                                        uint64_t rng_seed, hpc_stream_t stream);

/* ---- draft-token verification at the end of a speculative (MTP) decode step (ours: no reference counterpart) ----
 * Rejection sampling of num_draft = K draft tokens per request against the target model's logits, with a draft that
 * puts probability 1 on its token.  logits [batch_size * (K + 1), V] as for the sampler above (dtype 0 fp32 / 1 bf16,
 * inner stride 1, row stride >= V in elements, V % 8 == 0, V < 2^20, never written); row b * (K + 1) + j is position j
 * of request b.  draft_token_ids int64 [batch_size, K], 0 <= K <= 15 (may be NULL when K == 0): the first entry < 0 or
 * >= V ends the request's drafts, n_b = number of leading valid entries; logits rows past n_b are not read.
 * temperature f32 [batch_size] or NULL (then temperature_val); T = 0 is greedy for that request.
 * For j < n_b, d = draft[b][j], x = fp32 row b * (K + 1) + j:
 *   T > 0: accept iff uniform[b][j] < softmax(x / T)[d];   T == 0: accept iff d == argmax(x), ties -> smaller id.
 * First rejection at j: out[b][j] = argmax(x / T + gumbel) with entry d at -inf (T == 0: argmax(x)) - the token
 *   hpc_fused_sampler_temperature_async gives that row with draft d -, num_accepted[b] = j.
 * All n_b accepted: out[b][n_b] = argmax(x / T + gumbel) of row b * (K + 1) + n_b, no mask; num_accepted[b] = n_b.
 * out[b][:num_accepted[b]] are the accepted drafts, entries after the sampled one are -1.
 * uniform_samples f32 [batch_size, K] in [0, 1) and gumbel_noise f32 [batch_size * (K + 1), V]: both or neither
 * (uniform_samples is not looked at when K == 0); with
 * neither both are drawn from Philox keyed by rng_seed (> 0) at the sampler's launch offset, the uniform at a counter
 * no Gumbel draw takes.  output_token_ids int32 [batch_size, K + 1], num_accepted int32 [batch_size].
 * workspace: hpc_speculative_verify_workspace_bytes.  batch_size * (K + 1) <= 65535.  Every check runs on the host before
 * the batch_size == 0 return and before any launch: HPC_ERR_INVALID for null pointers, negative sizes, K < 0, a row
 * stride below V, one noise tensor without the other and rng_seed == 0 without noise; HPC_ERR_UNSUPPORTED for K > 15,
 * V % 8 != 0, V >= 2^20 and more than 65535 rows. */
int64_t hpc_speculative_verify_workspace_bytes(int batch_size, int num_draft, int vocab_size);
int hpc_speculative_verify_async(void* output_token_ids, void* num_accepted, void* workspace, const void* logits,
                                 int logits_dtype, int64_t logits_row_stride, const void* draft_token_ids,
                                 const void* temperature, float temperature_val, const void* uniform_samples,
                                 const void* gumbel_noise, int batch_size, int num_draft, int vocab_size,
                                 uint64_t rng_seed, hpc_stream_t stream);

/* ---- log-probability, rank and top-N of a given token per logits row (ours: no reference counterpart) ----
 * What a completion API's logprobs / top_logprobs, an RL rollout and prompt_logprobs need of the logits a step ends in,
 * in one pass.  logits [rows, V] as for the sampler above (dtype 0 fp32 / 1 bf16, inner stride 1, row stride >= V in
 * elements, V % 8 == 0, V < 2^20, never written).  token_ids [rows] of token_id_bytes = 4 (int32) or 8 (int64): the
 * token a sampler or the verification emitted for that row, or a prompt token.  An entry < 0 or >= V marks a dead row
 * (the -1 entries of a speculative step): its logits are not read, its outputs are 0.0, 0, -1 ..., 0.0 ....
 * temperature f32 [temperature_count] or NULL (then temperature_val >= 0): row r uses entry
 * r / (rows / temperature_count), so a count of rows is a value per row and a count of batch_size the per-request tensor
 * hpc_speculative_verify_async takes.  With x the fp32 row: y = x / T (an fp32 division) when T > 0, y = x when T == 0;
 * negative or NaN T is unspecified.
 *   token_logprobs f32 [rows]           y[t] - logsumexp(y)
 *   token_ranks    i32 [rows]           1 + #{i : x[i] > x[t] or (x[i] == x[t] and i < t)}: the order of the raw logits
 *                                       as floats, -0.0 == +0.0, ties to the smaller id (a stable descending sort); it
 *                                       does not depend on T
 *   top_ids        i32 [rows, num_top]  the first num_top ids of that order
 *   top_logprobs   f32 [rows, num_top]  y[id] - logsumexp(y) of those ids
 * Where rank <= num_top, top_ids[r][rank - 1] is the token and top_logprobs[r][rank - 1] has the bits of
 * token_logprobs[r].  -inf logits are ordinary (they add nothing and rank last; such a token has logprob -inf); a row
 * with a NaN, a +inf or a maximum of -inf is unspecified.  0 <= num_top <= 32, num_top <= V; top_ids and top_logprobs
 * may be NULL when num_top == 0.  workspace: hpc_token_logprobs_workspace_bytes.  Any number of rows: one launch pair
 * per 65535.  Every check runs on the host before the rows == 0 return and before any launch: HPC_ERR_INVALID for null
 * pointers, negative sizes, a dtype other than 0 / 1, a row stride below V, token_id_bytes other than 4 / 8, a
 * temperature_count < 1 or one that does not divide rows, a negative temperature_val without a tensor;
 * HPC_ERR_UNSUPPORTED for V % 8 != 0, V >= 2^20, num_top > 32 and num_top > V. */
int64_t hpc_token_logprobs_workspace_bytes(int rows, int num_top, int vocab_size);
int hpc_token_logprobs_async(void* token_logprobs, void* token_ranks, void* top_ids, void* top_logprobs, void* workspace,
                             const void* logits, int logits_dtype, int64_t logits_row_stride, const void* token_ids,
                             int token_id_bytes /* 4 or 8 */, const void* temperature /* may be NULL */,
                             int temperature_count, float temperature_val, int rows, int num_top, int vocab_size,
                             hpc_stream_t stream);

/* ---- communicator: socket rendezvous + symmetric device buffers (HIP IPC over xGMI) ---------------
 * reference: src/communicator/{communicator,channel,listener,connector,protocol}.cc (rank-0 star over
 *            an abstract unix socket "unix://name" / bare name, or "tcp://ip:port"),
 *            multicast_communicator.cc:21-153 (CreateTensorSync), entry.cc:18-90 (torch class).
 * hpc_comm_create returns a handle > 0 (negative = error); device_id < 0 = no HIP device (host-only
 * rendezvous, used by the CPU tests).  hpc_comm_create_tensor_sync is collective: allocates nbytes of
 * uncached device memory on every rank, exchanges IPC handles, ptrs_out[r] = rank r's buffer mapped
 * in this process (there is no multicast object on xGMI).  hpc_comm_lookup_peers translates an
 * address inside a local symmetric buffer into the same offset of every rank's buffer (returns the
 * world size or -1); hpc_comm_region_bytes_left returns the bytes from `ptr` to the end of the local
 * symmetric buffer that contains it (-1 if none) - the entries use it to learn a signal pad's capacity. */
int hpc_comm_create(int rank, int world_size, int device_id, const char* name);
int hpc_comm_destroy(int handle);
int hpc_comm_barrier(int handle);
int hpc_comm_allgather(int handle, const void* in, int64_t nbytes, void* out);
int hpc_comm_info(int handle, int* rank, int* world_size, int* device_id);
int hpc_comm_create_tensor_sync(int handle, int64_t nbytes, void** ptrs_out);
int hpc_comm_lookup_peers(const void* ptr, void** peer_ptrs, int* rank_out);
int64_t hpc_comm_region_bytes_left(const void* ptr);

/* ---- fused AllReduce + residual + RMSNorm (bf16) over peer memory ------------------------------------
 * reference: fuse_allreduce_rmsnorm_high_throughput_async, src/allreduce/
 *            fuse_allreduce_rmsnorm_high_throughput.h:11-17 (kernel .cu:15-99), and
 *            fuse_allreduce_rmsnorm_low_latency_async, fuse_allreduce_rmsnorm_low_latency.h:29-49,503-504.
 * R = bf16(sum_r x_r + residual); out = bf16(float(R) * rsqrt(mean(R^2) + eps) * w).
 * High throughput: this rank owns `num_rows` token rows (slices may differ between ranks); peer_x_ptrs[p] /
 *   peer_out_ptrs[p] address those rows inside rank p's symmetric input / output buffers,
 *   peer_signal_ptrs[p] rank p's signal pad of `signal_pad_words` zero-initialised uint32 (block b uses
 *   words [b * stride, b * stride + world_size), stride = hpc_fuse_allreduce_rmsnorm_high_throughput_signal_stride(
 *   world_size, grid, signal_pad_words): the blocks' flag groups are spread over the whole pad in 64-byte units - packed
 *   together they sit behind one channel of the uncached memory and every barrier access serialises there).
 *   The barriers pair block b of every rank, so the grid is a
 *   function of rank-invariant inputs only: hpc_fuse_allreduce_rmsnorm_high_throughput_grid(world_size,
 *   num_max_blocks, signal_pad_words) = min(max(num_max_blocks, 512), signal_pad_words / world_size); all
 *   ranks must pass the same num_max_blocks and pad size.  -2 when the pad cannot hold one block.
 *   hidden <= 16384, world_size <= 8.  (The reference supports H in {4096,5120,7168}.)
 * Low latency (Lamport, token t owned by rank t % world_size): data_buffer_ptrs_dev = device int64
 *   table of the ranks' workspace bases, workspace = 3 slots x 2 stages, pre-filled with 0x80000000
 *   words by the caller, buffer_flags_dev = 9 x uint32 {cur, dirty, bytes per slot, 0, bytes to clear
 *   x4, arrive} advanced on the device.
 * Every spin on a peer is bounded (~seconds).  A spin that gives up bumps a counter in pinned host memory:
 *   hpc_allreduce_timeouts reads it without synchronising any stream (0 in a healthy run), and from then on
 *   both entries return HPC_ERR_TIMEOUT instead of launching - after a lost peer the Lamport slots / signal
 *   pads hold leftovers, so the handles must be re-created; hpc_allreduce_reset_timeouts re-arms the entries. */
int hpc_fuse_allreduce_rmsnorm_high_throughput_grid(int world_size, int num_max_blocks, int signal_pad_words);
int hpc_fuse_allreduce_rmsnorm_high_throughput_signal_stride(int world_size, int grid, int signal_pad_words);
int hpc_fuse_allreduce_rmsnorm_high_throughput_async(
    const void* const* peer_x_ptrs, void* const* peer_out_ptrs, void* const* peer_signal_ptrs,
    const void* residual_ptr, void* out_residual_ptr, const void* weight_ptr, float rms_norm_eps,
    int num_rows, int hidden_size, int rank, int world_size, int num_max_blocks, int signal_pad_words,
    hpc_stream_t stream);
int hpc_fuse_allreduce_rmsnorm_low_latency_async(
    void* output_ptr, void* residual_out_ptr, const void* input_ptr, const void* data_buffer_ptrs_dev,
    void* local_workspace_ptr, void* buffer_flags_dev, const void* residual_in_ptr,
    const void* weight_ptr, float rms_norm_eps, int num_tokens, int hidden_size, int rank,
    int world_size, int64_t workspace_bytes, hpc_stream_t stream);
/* The same entry with the two mode flags of the reference op (src/allreduce/entry.cc:84: `rmsnorm_fusion`, `use_two_shot`):
 *   rmsnorm_fusion = 0: output = the reduced rows (bf16), no residual / norm (residual and weight pointers may be null);
 *   use_two_shot   = 0: the one-shot Lamport form - every rank pushes its rows to every rank and reduces them itself (the
 *   reference accepts the flag and runs its two-shot kernel either way; results here are bit-identical between the forms).
 *   One-shot workspace: 3 x num_tokens x world_size x hidden x 2 bytes (-2 when workspace_bytes is smaller). */
int hpc_allreduce_low_latency_async(
    void* output_ptr, void* residual_out_ptr, const void* input_ptr, const void* data_buffer_ptrs_dev,
    void* local_workspace_ptr, void* buffer_flags_dev, const void* residual_in_ptr,
    const void* weight_ptr, float rms_norm_eps, int num_tokens, int hidden_size, int rank,
    int world_size, int64_t workspace_bytes, int rmsnorm_fusion, int use_two_shot, hpc_stream_t stream);
int hpc_allreduce_timeouts(void);
int hpc_allreduce_reset_timeouts(void);

#ifdef __cplusplus
}
#endif
#endif /* HPC_AMD_H_ */
