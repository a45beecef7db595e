// Shared argument block of the grouped FP8 GEMM kernels: the streaming form and the entry points that fill the block
// (group_gemm_blockwise.hip), the 128 x 128 and 256 x 128 tiled forms (group_gemm_tiled.hip, group_gemm_tiled256.hip) and
// the 256 x 256 tile kernel (group_gemm_p8.hip); and what these files call of one another.
#pragma once
#include <stdint.h>

namespace hpc {
namespace ggemm {

struct Args {
  const uint8_t* x;       // [rows, K] e4m3
  const uint8_t* w;       // [G, N, K] e4m3
  const float* xs;        // activation scales, see xs_row_stride / xs_kb_stride
  const float* ws;        // [G, N/128, ws_ld]
  uint16_t* y;            // [M, N] bf16
  const int* seqlens;     // [G]
  const int* cu_seqlens;  // [G]   first row of group g in y (and in x when row_index == null)
  const int* row_index;   // null, or [M] -> row of x / xs for output row m (gather-free MoE)
  const int* col_base;    // null, or [G] (cu_tiles): transposed xs, column = col_base[g]*tile_m + slot
  int N, K, KB, tile_m;
  int ws_group_stride, ws_ntile_stride, ws_kb_stride;  // floats; per-tensor scales: (1, 0, 0)
  int has_xs;                                           // 0: no activation scales (factor 1)
  unsigned x_bytes;                                     // bytes of x (bounds the activation loads)
  long xs_row_stride, xs_kb_stride;                     // in floats
  // fused SiLU(gate) * up + 128-block quantisation in the epilogue of the gate-up GEMM (256 x 256 tile kernel only;
  // N = 2 * inter, a tile = 128 gate rows + the 128 up rows of the same columns): act_out e4m3 [M, inter],
  // act_scale f32 [M, inter / 128]; y is not written
  uint8_t* act_out = nullptr;
  float* act_scale = nullptr;
  // per-tensor form of the same epilogue (act_scale == nullptr): out = e4m3(silu(gate) * up * act_mul_scale[0]), with
  // the bf16-rounded multiply of the reference when use_bf16_mul (reference src/activation/activation.cu:19-75)
  const float* act_mul_scale = nullptr;
  int use_bf16_mul = 0;
  int no_half_tile = 0;  // development (key kDevP8NoHalfTile): 1 = the 256 x 256 kernel runs its full body only, 2 = no tail body (<= 64 rows)
  int nt_single = 1;     // 256 x 256 kernel, tail body: non-temporal weight loads for a group's ONLY (<= 64-row) token tile
  int tail_regs = 0;     // development (key kDevP8TailRegs): 1 = the register-streamed tail body instead of the LDS-ring one
  int item_scan_old = 0; // development (key kDevP8ItemScanOld): 1 = the item lookup's scans / lane reads through ds_bpermute (rounds 2-5) instead of DPP + v_readlane
  int ext_rows = 0;      // 256 x 256 kernel: 1 = a group's short tail rides along with its full tiles (group_gemm_p8.hip::locate_item)
  int item_order = 0;    // 256 x 256 kernel: 0 = tail tiles in place, 1 = full tiles first, tail tiles last (group_gemm_p8.hip::locate_item)
  void* prof = nullptr;  // development: s_memtime log of the 256 x 256 kernel's section boundaries (hpc_dev_p8_prof_buffer)
};

}  // namespace ggemm
}  // namespace hpc

namespace hpc { struct GgemmRoute; }  // group_gemm_route.h
// The launchers of the three tile kernels: each launches what `r` names.  `cu_tiles` = exclusive scan of ceil(seqlens / 128).
int hpc_ggemm_launch_tiled(const hpc::ggemm::Args& a, const hpc::GgemmRoute& r, const int* cu_tiles, int num_group,
                           hipStream_t stream);
int hpc_ggemm_launch_tiled256(const hpc::ggemm::Args& a, const hpc::GgemmRoute& r, const int* cu_tiles, int num_group,
                              hipStream_t stream);
int hpc_ggemm_launch_p8(const hpc::ggemm::Args& a, const hpc::GgemmRoute& r, const int* cu_tiles, int num_group,
                        hipStream_t stream);

// Gate-up GEMM of a fused MoE (group_gemm_blockwise.hip): the arguments of hpc_group_gemm_{blockwise,pertensor}_fp8_async with
// n = 2 * inter, plus the epilogue's outputs (Args::act_out ...).  *fused = GgemmRoute::act: 1 they are written, 0 y is, as by the plain entry.
int hpc_group_gemm_blockwise_fp8_act(void* y_ptr, void* act_out, void* act_scale, const void* x_ptr, const void* w_ptr,
                                     const void* seqlens_ptr, const void* cu_seqlens_ptr, const void* xscale_ptr,
                                     const void* wscale_ptr, const void* row_index_ptr, const void* col_base_ptr, int num_group,
                                     int m, int n, int k, int num_block_k_pad4, int tile_m, int64_t xscale_row_stride,
                                     int64_t xscale_kb_stride, const void* cu_tiles128_ptr, hipStream_t stream, int* fused);
int hpc_group_gemm_pertensor_fp8_act(void* y_ptr, void* act_out, const void* act_mul_scale_ptr, int use_bf16_mul,
                                     const void* x_ptr, const void* w_ptr, const void* seqlens_ptr, const void* cu_seqlens_ptr,
                                     const void* yscale_ptr, const void* row_index_ptr, int num_group, int m, int x_rows, int n,
                                     int k, const void* cu_tiles128_ptr, hipStream_t stream, int* fused);
