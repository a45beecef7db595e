// The two absorb matmuls of an MLA decode step, bf16, gfx950: W_UK into q in front of the decode attention and W_UV out of
// its latent output, the second with the 128-block e4m3 quantisation of the output projection's input in its epilogue.
//
//   absorb_q     out[t, h, c] = bf16( sum_{d < 128} q_nope[t, h, d] * w_uk[h, d, c] )          c < 512
//   unabsorb_o   o[t, h, v]   = bf16( sum_{c < 512} o_lat[t, h, c] * w_uv[h, v, c] )           v < 128
//                quant: scale[t, h] = amax_v |o| / 448, codes = e4m3( o * (1 / (scale + 1e-8)) )   (act_quant.h, on the bf16 o)
//
// Ours only (no reference kernel): semantics = the PyTorch statements tests/mla_absorb_ref.py.  fp32 accumulation in
// v_mfma_f32_16x16x32_bf16, one rounding.  Grid, tile and refusals: mla_absorb_route.h.  No split-K, no atomics, no workspace.
//
// Both products are computed TRANSPOSED - weight as the A operand (M), tokens as B (N) - so that a token sits on a lane
// (column l & 15 of the accumulator) and four consecutive output columns in its registers: 8-byte pieces (unabsorb_o stores
// them as they are, absorb_q gathers them into 16-byte stores), and for the quantiser an abs-max that is in-lane plus two
// cross-lane steps (row4_max) per wave.
//
// absorb_q.  Workgroup = (head, slice of 128 latent columns, tile of 64 or 256 tokens).  The reduction index d is the ROW of
// w_uk, so the A operand needs w_uk transposed: the slice's [128 d][128 c] block is copied as it lies into an LDS image (rows of
// 288 bytes: the 8 rows x 32 bytes a 32-lane half takes in a transposing read touch every bank once) and read ONCE through
// ds_read_b64_tr_b16, by every wave: 8 column blocks x 4 k-steps of fragments = 128 VGPRs.  From there the waves are on their
// own - wave w takes the token blocks w, w + 4, ... of the tile, no workgroup barrier - with the next block's q in flight
// while this one is multiplied.  The transposing read hands lane group g the rows 4 g .. 4 g + 3 of two 16-row blocks, so
// k-slot j of group g is d = 32 ks + 16 (j >> 2) + 4 g + (j & 3); the q fragment is loaded from global memory in that order
// (two 8-byte loads per k-step), the same permutation on both sides.  The accumulators hold 4 columns x 8 blocks of a token:
// they go through 4 KiB of the wave's own LDS (the image's bytes, free by then) so that a token's 256 bytes leave in 16-byte
// stores, 16 lanes to a row.
//
// unabsorb_o.  Workgroup = (head, tile of 64 tokens).  Both operands are contiguous along the reduction: fragments are 16-byte
// global loads, no LDS in front of the MFMA.  The four waves cut K = 512 in four (wave w: c in [128 w, 128 w + 128)); each holds
// the head's 128 x 128 weight block as 8 row blocks x 4 k-steps = 128 VGPRs for all token blocks of the tile.  Per token
// block the four partial accumulators meet in LDS and wave w sums rows 32 w .. 32 w + 31 in wave order ((p0 + p1) + p2) + p3 -
// a fixed order, the same in both modes -, rounds to bf16 and either stores, or quantises: the wave's abs-max, the four
// waves' through LDS, the scale and the codes from the ROUNDED values - what blockwise_quant_kernel computes from the stored bf16.
//
// A token row past T is clamped to T - 1 for the loads and not stored; every lane runs every MFMA and LDS read (EXEC all ones).
#include "act_quant.h"
#include "hpc_common.h"
#include "mla_absorb_route.h"
#include "../../include/hpc_amd.h"

namespace hpc {
namespace mla_absorb {

constexpr int kPitch = 288;                               // bytes of an LDS row of the w_uk image (256 of data)
constexpr int kImageBytes = kMlaAbsorbNope * kPitch;      // 36,864
constexpr int kKStepsQ = kMlaAbsorbNope / 32;             // 4
constexpr int kTokBlocks = kMlaAbsorbTokTile / 16;        // 4: unabsorb_o's token blocks per workgroup
constexpr int kColBlocksQ = kMlaAbsorbSlice / 16;         // 8 column blocks of a slice
constexpr int kOutPitch = 272;                            // bytes of a token's row in a wave's output scratch (256 of data)
static_assert(4 * 16 * kOutPitch <= kImageBytes && kOutPitch % 16 == 0, "the four waves' output scratch overlays the image");
static_assert(kPitch % 16 == 0 && (kPitch / 4) % 64 == 8, "a 32-lane half's 8 rows x 8 dwords cover the 64 banks once");

struct Args {
  const uint8_t* x;  // q_nope / o_lat
  const uint8_t* w;
  uint8_t* out;
  float* out_scale;
  int64_t x_rs, x_hs, w_hs, w_rs, out_rs, out_hs;  // BYTES
  int64_t num_tokens;
  int num_head, per_head, tok_tile;
};

// workgroup id -> head (dealt to one XCD) and piece of the head; false: no such head
__device__ __forceinline__ bool place(const Args& a, int& head, int& piece) {
  const int id = blockIdx.x, xcd = id % kMlaAbsorbXcds, k = id / kMlaAbsorbXcds;
  head = k / a.per_head * kMlaAbsorbXcds + xcd;
  piece = k % a.per_head;
  return head < a.num_head;
}

__device__ __forceinline__ u32x2 lds_tr(const uint8_t* p) {
  const v4i16 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      reinterpret_cast<lds_v4i16*>(static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_u8*)p))));
  return __builtin_bit_cast(u32x2, v);
}

__global__ __launch_bounds__(kMlaAbsorbThreads) void mla_absorb_q_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[kImageBytes];
  int head, piece;
  if (!place(a, head, piece)) return;  // the whole workgroup
  const int slice = piece % kMlaAbsorbSlices, tile = piece / kMlaAbsorbSlices;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c16 = lane & 15, g = lane >> 4;
  const int64_t t_tile = static_cast<int64_t>(tile) * a.tok_tile;
  const int64_t t_end = t_tile + a.tok_tile < a.num_tokens ? t_tile + a.tok_tile : a.num_tokens;

  // the q fragment of a 16-token block: k-slot j of lane group g is d = 32 ks + 16 (j >> 2) + 4 g + (j & 3)
  const uint8_t* qbase = a.x + head * a.x_hs + (4 * g) * 2;
  auto load_q = [&](int64_t t0, bf16x8(&qf)[kKStepsQ]) {
    const int64_t t = t0 + c16;
    const uint8_t* qrow = qbase + (t < a.num_tokens ? t : a.num_tokens - 1) * a.x_rs;
#pragma unroll
    for (int ks = 0; ks < kKStepsQ; ++ks) {
      const u32x2 lo = *reinterpret_cast<const u32x2*>(qrow + (32 * ks) * 2);
      const u32x2 hi = *reinterpret_cast<const u32x2*>(qrow + (32 * ks + 16) * 2);
      qf[ks] = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
    }
  };
  int64_t t0 = t_tile + 16 * wv;  // this wave's token blocks: t0, t0 + 64, ...
  bf16x8 qf[kKStepsQ], qn[kKStepsQ];
  if (t0 < t_end) load_q(t0, qf);  // in flight while the weights are staged

  // ---- the slice's [128 d][128 c] block of w_uk, as it lies: 2,048 chunks of 16 bytes, 8 per thread ----
  {
    const uint8_t* src = a.w + head * a.w_hs + slice * (kMlaAbsorbSlice * 2);
    u32x4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = i * kMlaAbsorbThreads + tid, row = idx >> 4, ch = idx & 15;
      v[i] = ld16(src + row * a.w_rs + ch * 16);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = i * kMlaAbsorbThreads + tid, row = idx >> 4, ch = idx & 15;
      *reinterpret_cast<u32x4*>(s_img + row * kPitch + ch * 16) = v[i];
    }
  }
  __syncthreads();

  // ---- A fragments: (w_uk slice)^T, all 8 column blocks x 4 k-steps, read once for every token block of the wave ----
  bf16x8 wf[kColBlocksQ][kKStepsQ];
  {
    const uint8_t* base = s_img + (4 * g + (c16 >> 2)) * kPitch + (c16 & 3) * 8;
#pragma unroll
    for (int cb = 0; cb < kColBlocksQ; ++cb)
#pragma unroll
      for (int ks = 0; ks < kKStepsQ; ++ks) {
        const u32x2 lo = lds_tr(base + (32 * ks) * kPitch + cb * 32);
        const u32x2 hi = lds_tr(base + (32 * ks + 16) * kPitch + cb * 32);
        wf[cb][ks] = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
      }
  }
  __syncthreads();  // the image is read: its bytes become the waves' output scratch; no workgroup barrier from here on

  uint8_t* scr = s_img + wv * (16 * kOutPitch);  // this wave's [16 tokens][128 columns] bf16
  uint8_t* obase = a.out + head * a.out_hs + slice * (kMlaAbsorbSlice * 2) + (lane & 15) * 16;
  while (t0 < t_end) {  // wave-uniform
    const int64_t t_next = t0 + 64;
    const bool more = t_next < t_end;
    if (more) load_q(t_next, qn);
    // lane (c16, g): token c16, columns 16 cb + 4 g + 0..3
#pragma unroll
    for (int cb = 0; cb < kColBlocksQ; ++cb) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < kKStepsQ; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cb][ks], qf[ks], acc, 0, 0, 0);
      *reinterpret_cast<u32x2*>(scr + c16 * kOutPitch + (16 * cb + 4 * g) * 2) =
          u32x2{pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3])};
    }
    // through the wave's scratch (LDS operations of one wave complete in order): a token's 256 bytes leave in 16-byte stores
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int tok = 4 * i + g;
      const u32x4 v = *reinterpret_cast<const u32x4*>(scr + tok * kOutPitch + (lane & 15) * 16);
      if (t0 + tok < a.num_tokens) st16(obase + (t0 + tok) * a.out_rs, v);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (!more) break;
#pragma unroll
    for (int ks = 0; ks < kKStepsQ; ++ks) qf[ks] = qn[ks];
    t0 = t_next;
  }
}

constexpr int kRowBlocks = kMlaAbsorbNope / 16;        // 8 blocks of 16 weight rows (v)
constexpr int kKStepsO = kMlaAbsorbLatent / 32 / 4;    // 4 k-steps per wave: a quarter of K

template <bool kQuant>
__global__ __launch_bounds__(kMlaAbsorbThreads) void mla_unabsorb_o_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) f32x4 s_part[4][kRowBlocks][64];  // [wave][row block][lane]: 32 KiB
  __shared__ float s_amax[4][16];
  int head, tile;
  if (!place(a, head, tile)) return;  // the whole workgroup
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c16 = lane & 15, g = lane >> 4;
  const int k0 = (128 * wv + 8 * g) * 2;  // byte offset along the reduction of this lane's k-slots in k-step 0

  // ---- A fragments: rows 16 vb + c16 of the head's w_uv, this wave's quarter of K ----
  bf16x8 wf[kRowBlocks][kKStepsO];
  {
    const uint8_t* wrow = a.w + head * a.w_hs + c16 * a.w_rs + k0;
#pragma unroll
    for (int vb = 0; vb < kRowBlocks; ++vb)
#pragma unroll
      for (int ks = 0; ks < kKStepsO; ++ks) wf[vb][ks] = *reinterpret_cast<const bf16x8*>(wrow + vb * 16 * a.w_rs + ks * 64);
  }

  const int64_t t_tile = static_cast<int64_t>(tile) * kMlaAbsorbTokTile;
#pragma unroll 1
  for (int tb = 0; tb < kTokBlocks; ++tb) {
    const int64_t t0 = t_tile + 16 * tb;
    if (t0 >= a.num_tokens) break;  // the whole workgroup: the barriers below stay matched
    const int64_t t = t0 + c16;
    const bool valid = t < a.num_tokens;
    const uint8_t* xrow = a.x + (valid ? t : a.num_tokens - 1) * a.x_rs + head * a.x_hs + k0;
    bf16x8 xf[kKStepsO];
#pragma unroll
    for (int ks = 0; ks < kKStepsO; ++ks) xf[ks] = *reinterpret_cast<const bf16x8*>(xrow + ks * 64);
#pragma unroll
    for (int vb = 0; vb < kRowBlocks; ++vb) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < kKStepsO; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[vb][ks], xf[ks], acc, 0, 0, 0);
      s_part[wv][vb][lane] = acc;
    }
    __syncthreads();

    // ---- wave w finishes row blocks 2 w, 2 w + 1: lane (c16, g) holds token c16, v = 16 vb + 4 g + 0..3 ----
    uint32_t ow[2][2];
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int vb = 2 * wv + j;
      const f32x4 r = ((s_part[0][vb][lane] + s_part[1][vb][lane]) + s_part[2][vb][lane]) + s_part[3][vb][lane];
      ow[j][0] = pack_bf16x2(r[0], r[1]);
      ow[j][1] = pack_bf16x2(r[2], r[3]);
    }
    if constexpr (!kQuant) {
      if (valid) {
        uint8_t* orow = a.out + t * a.out_rs + (head * kMlaAbsorbNope + 32 * wv + 4 * g) * 2;
#pragma unroll
        for (int j = 0; j < 2; ++j) *reinterpret_cast<u32x2*>(orow + j * 32) = u32x2{ow[j][0], ow[j][1]};
      }
    } else {
      float f[2][4];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bf16x4_to_f32(ow[j][0], ow[j][1], f[j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) amax = fmaxf(amax, fabsf(f[j][i]));
      }
      amax = row4_max(amax);  // over the four lane groups: the wave's 32 values of token c16
      if (g == 0) s_amax[wv][c16] = amax;
      __syncthreads();
      amax = fmaxf(fmaxf(s_amax[0][c16], s_amax[1][c16]), fmaxf(s_amax[2][c16], s_amax[3][c16]));
      const float scale = e4m3_block_scale(amax);
      const float inv = e4m3_block_inv(scale);
      if (valid) {
        uint8_t* orow = a.out + t * a.out_rs + head * kMlaAbsorbNope + 32 * wv + 4 * g;
#pragma unroll
        for (int j = 0; j < 2; ++j)
          *reinterpret_cast<uint32_t*>(orow + j * 16) = quant_4xe4m3(f[j][0] * inv, f[j][1] * inv, f[j][2] * inv, f[j][3] * inv);
        if (wv == 0 && g == 0) a.out_scale[t * a.num_head + head] = scale;
      }
    }
    __syncthreads();  // s_part and s_amax are written again by the next token block
  }
}

}  // namespace mla_absorb
}  // namespace hpc

namespace {
hpc::MlaAbsorbCall make_call(const void* out, const void* out_scale, const void* x, const void* w, int64_t num_tokens, int num_head,
                             int64_t x_rs, int64_t x_hs, int64_t w_hs, int64_t w_rs, int64_t out_rs, int64_t out_hs, int quant) {
  hpc::MlaAbsorbCall c{};
  c.out = reinterpret_cast<uintptr_t>(out);
  c.out_scale = reinterpret_cast<uintptr_t>(out_scale);
  c.x = reinterpret_cast<uintptr_t>(x);
  c.w = reinterpret_cast<uintptr_t>(w);
  c.num_tokens = num_tokens;
  c.num_head = num_head;
  c.x_row_stride = x_rs, c.x_head_stride = x_hs, c.w_head_stride = w_hs, c.w_row_stride = w_rs;
  c.out_row_stride = out_rs, c.out_head_stride = out_hs;
  c.quant = quant;
  return c;
}

hpc::mla_absorb::Args make_args(const hpc::MlaAbsorbCall& c, const hpc::MlaAbsorbRoute& r, int out_elem) {
  hpc::mla_absorb::Args a{};
  a.x = reinterpret_cast<const uint8_t*>(c.x);
  a.w = reinterpret_cast<const uint8_t*>(c.w);
  a.out = reinterpret_cast<uint8_t*>(c.out);
  a.out_scale = reinterpret_cast<float*>(c.out_scale);
  a.x_rs = 2 * c.x_row_stride, a.x_hs = 2 * c.x_head_stride, a.w_hs = 2 * c.w_head_stride, a.w_rs = 2 * c.w_row_stride;
  a.out_rs = out_elem * c.out_row_stride, a.out_hs = out_elem * c.out_head_stride;
  a.num_tokens = c.num_tokens;
  a.num_head = c.num_head;
  a.per_head = r.per_head;
  a.tok_tile = r.tok_tile;
  return a;
}
}  // namespace

extern "C" const char* hpc_mla_absorb_q_refusal(const void* out, const void* q_nope, const void* w_uk, int64_t num_tokens,
                                                int num_head, int64_t q_row_stride, int64_t q_head_stride, int64_t w_head_stride,
                                                int64_t w_row_stride, int64_t out_row_stride, int64_t out_head_stride) {
  return hpc::mla_absorb_q_route(make_call(out, nullptr, q_nope, w_uk, num_tokens, num_head, q_row_stride, q_head_stride,
                                           w_head_stride, w_row_stride, out_row_stride, out_head_stride, 0)).why;
}

extern "C" int hpc_mla_absorb_q_async(void* out, const void* q_nope, const void* w_uk, int64_t num_tokens, int num_head,
                                      int64_t q_row_stride, int64_t q_head_stride, int64_t w_head_stride, int64_t w_row_stride,
                                      int64_t out_row_stride, int64_t out_head_stride, hipStream_t stream) {
  const hpc::MlaAbsorbCall c = make_call(out, nullptr, q_nope, w_uk, num_tokens, num_head, q_row_stride, q_head_stride, w_head_stride,
                                         w_row_stride, out_row_stride, out_head_stride, 0);
  const hpc::MlaAbsorbRoute r = hpc::mla_absorb_q_route(c);  // every check on the host, before any device call
  if (r.code != HPC_OK) return r.code;
  if (r.empty) return HPC_OK;
  hpc::mla_absorb::mla_absorb_q_kernel<<<static_cast<unsigned>(r.grid), r.threads, 0, stream>>>(make_args(c, r, 2));
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

extern "C" const char* hpc_mla_unabsorb_o_refusal(const void* out, const float* out_scale, const void* o_lat, const void* w_uv,
                                                  int64_t num_tokens, int num_head, int64_t o_row_stride, int64_t o_head_stride,
                                                  int64_t w_head_stride, int64_t w_row_stride, int64_t out_row_stride, int quant) {
  return hpc::mla_unabsorb_o_route(make_call(out, out_scale, o_lat, w_uv, num_tokens, num_head, o_row_stride, o_head_stride,
                                             w_head_stride, w_row_stride, out_row_stride, 0, quant)).why;
}

extern "C" int hpc_mla_unabsorb_o_async(void* out, float* out_scale, const void* o_lat, const void* w_uv, int64_t num_tokens,
                                        int num_head, int64_t o_row_stride, int64_t o_head_stride, int64_t w_head_stride,
                                        int64_t w_row_stride, int64_t out_row_stride, int quant, hipStream_t stream) {
  const hpc::MlaAbsorbCall c = make_call(out, out_scale, o_lat, w_uv, num_tokens, num_head, o_row_stride, o_head_stride, w_head_stride,
                                         w_row_stride, out_row_stride, 0, quant);
  const hpc::MlaAbsorbRoute r = hpc::mla_unabsorb_o_route(c);
  if (r.code != HPC_OK) return r.code;
  if (r.empty) return HPC_OK;
  const unsigned grid = static_cast<unsigned>(r.grid);
  if (quant)
    hpc::mla_absorb::mla_unabsorb_o_kernel<true><<<grid, r.threads, 0, stream>>>(make_args(c, r, 1));
  else
    hpc::mla_absorb::mla_unabsorb_o_kernel<false><<<grid, r.threads, 0, stream>>>(make_args(c, r, 2));
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
