// Operand-layout probe for v_mfma_scale_f32_16x16x128_f8f6f4 with an FP4 (e2m1) A operand, an e4m3 B operand and a register scale
// on A - the instruction form of csrc/group_gemm_mxfp4.hip (development tool; its result is quoted in DESIGN.md).  One wave runs
// single MFMAs into a zero accumulator on planted operands: one non-zero FP4 code, one non-zero e4m3 byte, one scale byte other
// than 127, and reports
//   1. for every (lane, nibble) of A which (row, k) it is, found against a B operand packed by the expected layout;
//   2. for every (lane, byte) of B which (column, k) it is, found against an A operand packed by the expected layout;
//   3. for every lane's scale byte the set of (row, k) of A it multiplies;
//   4. which byte of the scale register each op_sel value picks;
//   5. the value of each of the 16 e2m1 codes in either nibble.
// Expected (and what the kernel relies on): lane l holds row / column l % 16.  FP4: the 32 consecutive k of group l / 16 - register j
// of the first four holds k = 32 (l / 16) + 8 j ... + 7, low nibble first.  e4m3: the 16 consecutive k of group l / 16 and the 16 that
// lie 64 further on - registers 0 ... 3 hold k = 16 (l / 16) ... + 15, registers 4 ... 7 k = 64 + 16 (l / 16) ... + 15, low byte first (the
// "chunks g and g + 4 of a 128-byte row" of the FP8 kernels).  The lane's scale multiplies exactly its own 32 FP4 values; op_sel s
// picks byte s.  Only the RELATION between the two operands' k and the reach of a scale can be observed; the FP4 side is
// taken as the one that is consecutive.
// Every kernel sums its MFMA results into a per-lane value that is stored unconditionally: an MFMA whose only use sits in a
// lane-dependent branch is sunk into that branch by hipcc and then runs under a partial EXEC mask, on operand registers the
// other lanes never wrote (the first version of this probe read NaN that way).
//   hipcc --offload-arch=gfx950 -O2 tools/probes/probe_mfma_fp4.hip -o tools/probes/bin/probe_mfma_fp4 && tools/probes/bin/probe_mfma_fp4
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kOne8 = 0x38;  // e4m3 1.0
constexpr int kOne4 = 0x2;   // e2m1 1.0

template <int kOpSel>
__device__ __forceinline__ f32x4 mfma(i32x8 a, i32x8 b, int scale_a) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, f32x4{0.f, 0.f, 0.f, 0.f}, /*cbsz: A fp4*/ 4, /*blgp: B e4m3*/ 0,
                                                          kOpSel, scale_a, 0, 0x7f7f7f7f);
}
// the expected packing of one element
__device__ __forceinline__ i32x8 a_single(int lane, int row, int k, int code) {
  i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
  if (lane == row + 16 * (k / 32)) a[(k % 32) / 8] = code << (4 * (k % 8));
  return a;
}
__device__ __forceinline__ i32x8 b_single(int lane, int col, int k, int byte) {
  i32x8 b = {0, 0, 0, 0, 0, 0, 0, 0};
  if (lane == col + 16 * ((k % 64) / 16)) b[4 * (k / 64) + (k % 16) / 4] = byte << (8 * (k % 4));
  return b;
}
// D[row][col]: col = lane & 15, row = 4 (lane >> 4) + register.  Every non-zero entry is reported: (row, col, value) of the last one
// and how many there were.
__device__ __forceinline__ void report(f32x4 d, int lane, int* where, float* value, int* count) {
  for (int i = 0; i < 4; ++i)
    if (d[i] != 0.f) {
      *where = ((4 * (lane >> 4) + i) << 8) | (lane & 15);
      *value = d[i];
      atomicAdd(count, 1);
    }
}

// out[(lane, pos)] for 64 x 32 positions: where = (row << 8 | col), k, value, count of non-zero outputs over all 128 k
__global__ void discover_kernel(int which, int* where, int* kk, float* value, int* count, float* sink) {
  const int lane = threadIdx.x;
  float keep = 0.f;
  for (int l = 0; l < 64; ++l)
    for (int j = 0; j < 32; ++j)
      for (int k0 = 0; k0 < 128; ++k0) {
        i32x8 a, b;
        if (which == 0) {  // one FP4 nibble of A planted by position, B by the expected layout at (col 0, k0)
          a = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
          if (lane == l) a[j / 8] = kOne4 << (4 * (j % 8));
          b = b_single(lane, 0, k0, kOne8);
        } else {  // one e4m3 byte of B planted by position, A by the expected layout at (row 0, k0)
          b = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
          if (lane == l) b[j / 4] = kOne8 << (8 * (j % 4));
          a = a_single(lane, 0, k0, kOne4);
        }
        const f32x4 d = mfma<0>(a, b, 0x7f7f7f7f);
        keep += d[0] + d[1] + d[2] + d[3];
        int w = -1;
        float v = 0.f;
        report(d, lane, &w, &v, &count[l * 32 + j]);
        if (w >= 0) {
          where[l * 32 + j] = w;
          kk[l * 32 + j] = k0;
          value[l * 32 + j] = v;
        }
      }
  sink[lane] = keep;
}

// covered[ls][row * 128 + k] = D[row][0] for A = 1.0 at (row, k) alone, B = 1.0 everywhere, lane ls's scale byte 128 (x 2), others 127
__global__ void scale_kernel(float* covered, float* sink) {
  const int lane = threadIdx.x;
  float keep = 0.f;
  i32x8 b;
  for (int i = 0; i < 8; ++i) b[i] = kOne8 * 0x01010101;
  for (int ls = 0; ls < 64; ++ls)
    for (int row = 0; row < 16; ++row)
      for (int k0 = 0; k0 < 128; ++k0) {
        const f32x4 d = mfma<0>(a_single(lane, row, k0, kOne4), b, lane == ls ? 0x7f7f7f80 : 0x7f7f7f7f);
        keep += d[0] + d[1] + d[2] + d[3];
        if ((lane & 15) == 0 && (lane >> 4) == row / 4) covered[(ls * 16 + row) * 128 + k0] = d[row % 4];
      }
  sink[lane] = keep;
}

// opsel[(s * 4 + byte) * 64 + lane] = the lane's D register 0 (lane 0: D[0][0]) for A = 1.0 at (0, 0), B = 1.0, every lane's scale 127
// in all bytes but `byte` = 128, op_sel = s.  Every lane stores.
template <int kS>
__device__ void opsel_one(float* out, int lane) {
  i32x8 b;
  for (int i = 0; i < 8; ++i) b[i] = kOne8 * 0x01010101;
  for (int byte = 0; byte < 4; ++byte) {
    const int sc = 0x7f7f7f7f + (1 << (8 * byte));
    const f32x4 d = mfma<kS>(a_single(lane, 0, 0, kOne4), b, sc);
    out[(kS * 4 + byte) * 64 + lane] = d[0];
  }
}
__global__ void opsel_kernel(float* out, float* codes) {
  const int lane = threadIdx.x;
  opsel_one<0>(out, lane);
  opsel_one<1>(out, lane);
  opsel_one<2>(out, lane);
  opsel_one<3>(out, lane);
  // the 16 codes, in the low nibble (k = 0) and the high nibble (k = 1) of the first byte
  for (int c = 0; c < 16; ++c)
    for (int k0 = 0; k0 < 2; ++k0) {
      const f32x4 d = mfma<0>(a_single(lane, 0, k0, c), b_single(lane, 0, k0, kOne8), 0x7f7f7f7f);
      codes[(c * 2 + k0) * 64 + lane] = d[0];
    }
}

#define CK(x)                                                          \
  do {                                                                 \
    if ((x) != hipSuccess) {                                           \
      printf("HIP error at line %d\n", __LINE__);                      \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  int *where, *kk, *count;
  float *value, *covered, *small;
  CK(hipMalloc(&where, 2048 * 4));
  CK(hipMalloc(&kk, 2048 * 4));
  CK(hipMalloc(&count, 2048 * 4));
  CK(hipMalloc(&value, 2048 * 4));
  CK(hipMalloc(&covered, 64 * 16 * 128 * 4));
  CK(hipMalloc(&small, 48 * 64 * 4));
  float* sink;
  CK(hipMalloc(&sink, 64 * 4));
  std::vector<int> hw(2048), hk(2048), hc(2048);
  std::vector<float> hv(2048);
  int bad_total = 0;
  for (int which = 0; which < 2; ++which) {
    CK(hipMemset(where, 0xff, 2048 * 4));
    CK(hipMemset(kk, 0xff, 2048 * 4));
    CK(hipMemset(count, 0, 2048 * 4));
    discover_kernel<<<1, 64>>>(which, where, kk, value, count, sink);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(hw.data(), where, 2048 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hk.data(), kk, 2048 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hc.data(), count, 2048 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hv.data(), value, 2048 * 4, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 32; ++j) {
        const int i = l * 32 + j;
        // A: D[row][0], so `where` = row << 8; B: D[0][col], so `where` = col
        const int idx = which == 0 ? hw[i] >> 8 : hw[i] & 255, other = which == 0 ? hw[i] & 255 : hw[i] >> 8;
        const int want_k = which == 0 ? 32 * (l / 16) + j : 16 * (l / 16) + j % 16 + 64 * (j / 16);
        const bool ok = hc[i] == 1 && idx == l % 16 && other == 0 && hk[i] == want_k && hv[i] == 1.f;
        if (!ok && bad++ < 16)
          printf("  %s lane %2d pos %2d: %d non-zero outputs, last at %s %d k %d value %g\n", which == 0 ? "A" : "B", l, j, hc[i],
                 which == 0 ? "row" : "col", idx, hk[i], hv[i]);
      }
    printf("%s operand (%s): lane l, position j (%s) is %s l %% 16, k = %s: %d of 2048 positions differ\n",
           which == 0 ? "A" : "B", which == 0 ? "e2m1, 4 registers" : "e4m3, 8 registers",
           which == 0 ? "nibble j % 8 of register j / 8" : "byte j % 4 of register j / 4", which == 0 ? "row" : "column",
           which == 0 ? "32 (l / 16) + j" : "16 (l / 16) + j % 16 + 64 (j / 16)", bad);
    for (int l = 0; l < 64; l += 21)
      printf("  lane %2d: position 0 -> (%d, k %d), position 9 -> (%d, k %d), position 31 -> (%d, k %d)\n", l,
             which == 0 ? hw[l * 32] >> 8 : hw[l * 32] & 255, hk[l * 32], which == 0 ? hw[l * 32 + 9] >> 8 : hw[l * 32 + 9] & 255,
             hk[l * 32 + 9], which == 0 ? hw[l * 32 + 31] >> 8 : hw[l * 32 + 31] & 255, hk[l * 32 + 31]);
    bad_total += bad;
  }
  scale_kernel<<<1, 64>>>(covered, sink);
  CK(hipDeviceSynchronize());
  std::vector<float> cov(64 * 16 * 128);
  CK(hipMemcpy(cov.data(), covered, cov.size() * 4, hipMemcpyDeviceToHost));
  int bad = 0;
  for (int ls = 0; ls < 64; ++ls) {
    int n2 = 0, kmin = 999, kmax = -1, rmin = 99, rmax = -1, other = 0;
    for (int row = 0; row < 16; ++row)
      for (int k = 0; k < 128; ++k) {
        const float v = cov[(ls * 16 + row) * 128 + k];
        if (v == 2.f) {
          ++n2;
          kmin = k < kmin ? k : kmin;
          kmax = k > kmax ? k : kmax;
          rmin = row < rmin ? row : rmin;
          rmax = row > rmax ? row : rmax;
        } else if (v != 1.f) {
          ++other;
        }
      }
    const bool ok = n2 == 32 && other == 0 && rmin == ls % 16 && rmax == ls % 16 && kmin == 32 * (ls / 16) && kmax == kmin + 31;
    if (!ok || ls % 21 == 0)
      printf("  scale of lane %2d multiplies %d values: rows %d..%d, k %d..%d (%d outputs neither 1 nor 2)%s\n", ls, n2, rmin, rmax, kmin,
             kmax, other, ok ? "" : "  <-- not the lane's own 32");
    bad += !ok;
  }
  printf("A scale: the byte of lane l multiplies row l %% 16, k = 32 (l / 16) ... + 31 and nothing else: %d of 64 lanes differ\n", bad);
  bad_total += bad;
  opsel_kernel<<<1, 64>>>(small, small + 16 * 64);
  CK(hipDeviceSynchronize());
  std::vector<float> all(48 * 64);
  CK(hipMemcpy(all.data(), small, all.size() * 4, hipMemcpyDeviceToHost));
  float hs[48];
  for (int i = 0; i < 48; ++i) hs[i] = all[i * 64];  // lane 0
  for (int s = 0; s < 4; ++s) {
    printf("  op_sel %d: output with byte 0 / 1 / 2 / 3 of the scale register = 128:  %g %g %g %g\n", s, hs[s * 4], hs[s * 4 + 1],
           hs[s * 4 + 2], hs[s * 4 + 3]);
    for (int b = 0; b < 4; ++b) bad_total += hs[s * 4 + b] != (b == s ? 2.f : 1.f);
  }
  static const float e2m1[16] = {0.f, .5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f, -0.f, -.5f, -1.f, -1.5f, -2.f, -3.f, -4.f, -6.f};
  printf("  e2m1 codes 0..15, low nibble:");
  for (int c = 0; c < 16; ++c) printf(" %g", hs[16 + 2 * c]);
  printf("\n  e2m1 codes 0..15, high nibble:");
  for (int c = 0; c < 16; ++c) printf(" %g", hs[16 + 2 * c + 1]);
  printf("\n");
  for (int c = 0; c < 32; ++c) bad_total += hs[16 + c] != e2m1[c / 2];
  printf("%s\n", bad_total == 0 ? "RESULT: the expected layout holds in every respect" : "RESULT: the expected layout does NOT hold");
  return bad_total == 0 ? 0 : 2;
}
