"""Test helpers; `allclose` has the contract of reference tests/utils.py:176-189
(dtype/device/shape asserts + torch.allclose in fp32, worst offenders printed on failure)."""
import math

import pytest
import torch


def allclose(ref_tensor, real_tensor, atol=1e-8, rtol=1e-5):
    assert ref_tensor.dtype == real_tensor.dtype, (ref_tensor.dtype, real_tensor.dtype)
    assert ref_tensor.device == real_tensor.device, (ref_tensor.device, real_tensor.device)
    assert ref_tensor.shape == real_tensor.shape, (ref_tensor.shape, real_tensor.shape)
    a, b = ref_tensor.to(torch.float32), real_tensor.to(torch.float32)
    ok = torch.allclose(a, b, atol=atol, rtol=rtol)
    if not ok:
        err = (a - b).abs()
        bad = err > (atol + rtol * a.abs())
        flat = torch.where(bad.reshape(-1))[0]
        top = torch.topk(err.reshape(-1), min(10, err.numel())).indices
        print(f"\nallclose FAILED: {int(bad.sum())}/{a.numel()} elements out of tolerance "
              f"(atol={atol}, rtol={rtol}); max abs err {float(err.max()):.6g}")
        for i in top.tolist():
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), a.shape))
            print(f"  {idx}: ref={float(a.reshape(-1)[i]):.6g} real={float(b.reshape(-1)[i]):.6g}")
        if flat.numel():
            pass
    return ok


# Floor of the per-row scale in attn_close: a row whose largest |ref| is below it is measured against the floor, so
# all-zero reference rows cannot divide by zero.  Far below the smallest row scale of any decode generator here
# (near-uniform attention over 64k tokens of randn V: max |y| ~ 1e-3) and above bf16's subnormals.
ATTN_FLOOR = 1e-5


def attn_rel_err(ref, real, num_seq_q=1, floor=ATTN_FLOOR):
    """Per (request, q row, q head): max_d |real - ref| / max(max_d |ref|, floor), as float32 [B, Sq, Hq].  NaN and inf
    in `real` count as an infinite error."""
    assert ref.shape == real.shape, (ref.shape, real.shape)
    hq, d = ref.shape[-2], ref.shape[-1]
    a = ref.float().reshape(-1, num_seq_q, hq, d)
    b = real.float().reshape(-1, num_seq_q, hq, d).to(a.device)
    err = (b - a).abs().amax(-1).nan_to_num(nan=float("inf"))
    return err / a.abs().amax(-1).clamp_min(floor)


def attn_close(ref, real, tau, num_seq_q=1, floor=ATTN_FLOOR, label=""):
    """Scale-aware decode-attention bar: every (request, q row, q head) of `real` must sit within tau of its own row's
    scale (attn_rel_err).  An absolute atol on outputs of |y| ~ 0.01 accepts an all-zero answer; this one does not.
    On failure the worst rows are printed: request, row, head, relative error, max |ref|."""
    rel = attn_rel_err(ref, real, num_seq_q, floor)
    ok = bool((rel <= tau).all())
    if not ok:
        scale = ref.float().reshape(rel.shape + (-1,)).abs().amax(-1)
        bad = int((rel > tau).sum())
        print(f"\nattn_close FAILED {label}: {bad}/{rel.numel()} (request, row, head) out of tau={tau:.4g}; "
              f"worst {float(rel.max()):.4g}")
        for i in torch.topk(rel.reshape(-1), min(10, rel.numel())).indices.tolist():
            b, s, h = (int(v) for v in torch.unravel_index(torch.tensor(i), rel.shape))
            print(f"  request {b} row {s} head {h}: err {float(rel[b, s, h]):.4g} x scale, max|ref| {float(scale[b, s, h]):.4g}")
    return ok


# fp32 slack of the rope + KV store bar (rope_excess / rope_close), as a fraction of the head's largest |value|.
# Measured, not chosen: see rope_excess.
ROPE_SLACK = 2.0 ** -20


def _floor_log2(x, lowest):
    """floor(log2 |x|) of a float64 tensor, exactly (frexp: |x| = m * 2^e with m in [0.5, 1)), not below `lowest`."""
    a = x.double().abs()
    e = torch.frexp(a)[1].long() - 1
    return torch.where(a == 0, torch.full_like(e, lowest), e).clamp_min(lowest)


def ulp_bf16(x):
    """Spacing of bf16 at |x| (float64 tensor): 2^(floor(log2 |x|) - 7), the smallest normal's below it."""
    return torch.exp2((_floor_log2(x, -126) - 7).double())


def ulp_e4m3(x):
    """Spacing of e4m3 at |x|: 2^(floor(log2 |x|) - 3), and the subnormal step 2^-9 below 2^-6."""
    return torch.exp2((_floor_log2(x, -6) - 3).double())


def rope_excess(ref64, got, mult=None):
    """What a rope output misses the exact result by, beyond one rounding: per (row, head) of [rows, H, 128]
        max_d (|got - t| - 0.5 ulp(t)) / max_d |t|
    with t = ref64 and bf16's ulp for a bf16 output (mult None), and t = clamp(ref64 * mult, -448, 448) and e4m3's ulp for
    an e4m3 output written as x * mult (mult: the fp32 multiplier the kernel uses, a scalar or [rows, H]).  NaN in `got`
    counts as an infinite excess.  The kernel computes in fp32 and rounds once, so its excess is fp32 noise; the bar is
    excess <= ROPE_SLACK.

    Where ROPE_SLACK comes from: the fp32 oracle (oracle/rope.py rms_norm / rotary_neox in fp32, one rounding) against the
    float64 statement (rope_norm_ref64) on 4096 rows x 16 heads, norm policies 0 / 1 / 2, inputs of scale 1 and 1e-3,
    has a worst excess of about 1e-7 of the head maximum: 0.7e-7 ... 1.4e-7 for bf16 depending on the seed, up to 1.0e-7
    for e4m3 with the dynamic scale's reciprocal, 1.4e-8 with a fixed multiplier of order 1 (tests/test_rope_bar.py
    measures it again on its own inputs and prints it).  ROPE_SLACK = 2^-20 = 9.5e-7 is the 1.4e-7 with a margin of about
    8 x (raised, it may reach 2^-18 at most: beyond that is a finding about the kernel), for what a correct
    kernel may do differently: the order of the sum of squares, the hardware reciprocal square root, the reciprocal of
    the scale, fused multiply-adds in the rotation."""
    assert ref64.dtype == torch.float64 and ref64.shape == got.shape, (ref64.dtype, ref64.shape, got.shape)
    if mult is None:
        t, ulp = ref64, ulp_bf16(ref64)
    else:
        m = torch.as_tensor(mult, dtype=torch.float32).double()
        t = (ref64 * (m.reshape(-1)[0] if m.numel() == 1 else m.unsqueeze(-1))).clamp(-448.0, 448.0)
        ulp = ulp_e4m3(t)
    over = ((got.float().double() - t).abs() - 0.5 * ulp).nan_to_num(nan=float("inf")).amax(-1)
    return over / t.abs().amax(-1).clamp_min(1e-300)


def rope_close(ref64, got, mult=None, slack=ROPE_SLACK, label=""):
    """The rope bar: every (row, head) of `got` within half an ulp of the exact result plus `slack` x the head's largest
    |value| (rope_excess).  Prints the worst excess in units of the slack; on failure the worst elements too: row, head,
    element, value, reference."""
    ex = rope_excess(ref64, got, mult)
    worst = float(ex.max()) if ex.numel() else float("-inf")
    ok = bool((ex <= slack).all())
    print(f"rope_close {label}: worst excess {worst:.3g} of the head maximum = {worst / slack:.3g} x slack"
          + ("" if ok else f"  FAILED: {int((ex > slack).sum())}/{ex.numel()} (row, head) over"))
    if not ok:
        m = None if mult is None else torch.as_tensor(mult, dtype=torch.float32).double()
        for i in torch.topk(ex.reshape(-1), min(10, ex.numel())).indices.tolist():
            r, h = (int(v) for v in torch.unravel_index(torch.tensor(i), ex.shape))
            t = ref64[r, h] if m is None else (ref64[r, h] * (m.reshape(-1)[0] if m.numel() == 1 else m[r, h])).clamp(-448.0, 448.0)
            d = int((got[r, h].float().double() - t).abs().nan_to_num(nan=float("inf")).argmax())
            print(f"  row {r} head {h} element {d}: got {float(got[r, h, d]):.9g} ref {float(t[d]):.9g} "
                  f"(excess {float(ex[r, h]):.3g}, head max {float(t.abs().max()):.4g})")
    return ok


NORM_SLACK = 2.0 ** -19
"""fp32 slack of the RMSNorm quantiser's bar (quant_close in tests/test_normalization_bar.py), relative to each element.

Measured: the fp32 oracle (oracle/normalization.py::rmsnorm_fp32, then `* (1 / scale)` in fp32) against the float64
statement (tests/quant_ref.py::rmsnorm_ref64) on every input of tests/test_normalization_bar.py (15 hidden sizes x 1 / 3 /
5 / 9 rows, both scale pairs) has a worst quant_excess of 2.22e-7 on the fp32 output and 8.8e-8 on the e4m3 outputs
(test_fp32_oracle_passes_and_its_excess prints them again and holds the constant to them).  8 x 2.22e-7 = 1.78e-6, and the
next power of two at or above that is 2^-19 = 1.91e-6.  The margin is for what a correct kernel may do differently from the oracle: another order
of the sum of squares, the hardware reciprocal square root, `1.0f / scale` and a multiply where the oracle multiplies
the same reciprocal, and its two fp32 multiplies.  Cap: 2^-18; a kernel that needs more is a finding."""

ACT_SLACK = 2.0 ** -19
"""fp32 slack of the activation quantisers' bar (tests/test_act_quant_bar.py), relative to each element.

Measured: a CPU model of the device formula g / (1 + __expf(-g)) in fp32 (tests/quant_ref.py::silu_device_model: the
exponential evaluated in float64, rounded to fp32 and moved by +1 / 0 / -1 fp32 ulp - the microarchitecture guide states
no accuracy for the hardware exponential, so +-1 ulp is used - then the add, the divide, `* u` and `* scale` each
rounded to fp32) against the float64 silu(g) * u * scale over the test's random gates (|g| <= 8) has a worst
quant_excess of 2.75e-7 on the fp32 value in front of the cast (no half-ulp term: the model's fp32 error itself) and of
1.1e-8 on its e4m3 codes (positive only on the few elements an fp32 error carries over an e4m3 tie, so it falls with the
element count; the larger figure counts).  test_device_model_passes_and_its_excess prints both again and holds the
constant to them.  4 x 2.75e-7 = 1.1e-6, rounded up to a power of two: 2^-19 = 1.91e-6.  Cap: 2^-16; a kernel that
needs more is a finding."""


def quant_excess(t64, got, ulp):
    """What a quantiser's output misses its float64 target by, beyond one rounding, per element and relative to it:
        (|got - t| - 0.5 ulp(t)) / max(|t|, tiny)
    t64: the target, already multiplied by the scale and clamped to +-448 for e4m3.  ulp: ulp_e4m3 or ulp_bf16, or None
    for an fp32 output (no half-ulp term: the slack alone is the bar).  A NaN in `got` where t is finite is an infinite
    excess; where t is NaN `got` must be NaN (for e4m3: the byte 0x7f) and the excess is then 0.  Zeros compare by value,
    so -0 meets a target of +0."""
    assert t64.dtype == torch.float64 and t64.shape == got.shape, (t64.dtype, t64.shape, got.shape)
    g = got.float().double()
    half = 0.5 * ulp(t64) if ulp is not None else torch.zeros_like(t64)
    ex = ((g - t64).abs() - half) / t64.abs().clamp_min(1e-300)
    ex = torch.where(g.isnan(), torch.full_like(ex, float("inf")), ex)
    nan_ok = g.isnan() & (got.view(torch.uint8) == 0x7F if got.dtype == torch.float8_e4m3fn else True)
    return torch.where(t64.isnan(), torch.where(nan_ok, 0.0, float("inf")).to(ex.dtype), ex)


def quant_close(t64, got, ulp, slack, label=""):
    """The quantisers' bar: every element of `got` within half an ulp of its float64 target plus `slack` x |target|
    (quant_excess).  Prints the worst excess in units of the slack; on failure the ten worst elements too."""
    ex = quant_excess(t64, got, ulp)
    worst = float(ex.max()) if ex.numel() else float("-inf")
    ok = bool((ex <= slack).all())
    print(f"quant_close {label}: worst excess {worst:.3g} = {worst / slack:.3g} x slack"
          + ("" if ok else f"  FAILED: {int((ex > slack).sum())}/{ex.numel()} elements over"))
    if not ok:
        for i in torch.topk(ex.reshape(-1), min(10, ex.numel())).indices.tolist():
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ex.shape))
            print(f"  {idx}: got {float(got.reshape(-1)[i].float()):.9g} target {float(t64.reshape(-1)[i]):.9g} "
                  f"excess {float(ex.reshape(-1)[i]):.3g}")
    return ok


def to_cpu(*ts):
    return [t.cpu() if t is not None else None for t in ts]


def moe_allclose(ref, real, rtol=0.01, atol=0.01, max_literal_outliers=0.005, max_rel_rms=5e-3, max_abs_frac=0.02):
    """Tolerance of the fused-MoE parity checks at hidden sizes beyond the reference test's (512).

    The reference bar is rtol = atol = 0.01 at hidden 512 / ffn <= 512 (tests/test_fuse_moe_blockwise.py:268,350),
    where outputs are O(1).  With the same generator at hidden 4096 / ffn 11008 every expert contribution is
    O(10-30) and is rounded to bf16 (ulp 0.06-0.25) after each GEMM; a bf16 rounding of a gate_up element that
    flips with the fp32 summation order can move one e4m3 code of the quantised activation (a 6 % step of that
    element), so a small fraction of the outputs differs by a few bf16 ulps whatever the kernel does.  The bar:
      * at least 1 - max_literal_outliers (99.5 %) of the elements meet the reference's literal (0.01, 0.01);
      * the relative RMS error of every row is <= max_rel_rms;
      * no element is off by more than max_abs_frac of the largest |ref| (a wrong expert / scale / row is O(1))."""
    a, b = ref.float(), real.float()
    err = (a - b).abs()
    literal_miss = float((err > atol + rtol * a.abs()).float().mean())
    rel_rms = float((err.pow(2).mean(-1).sqrt() / a.pow(2).mean(-1).sqrt().clamp_min(1e-3)).max())
    worst = float(err.max() / a.abs().max().clamp_min(1e-3))
    ok = literal_miss <= max_literal_outliers and rel_rms <= max_rel_rms and worst <= max_abs_frac
    if not ok:
        print(f"\nmoe_allclose FAILED: max abs err {float(err.max()):.4g} ({worst:.4g} of max |ref|), worst row relative "
              f"rms {rel_rms:.4g}, fraction outside the literal (0.01, 0.01) bar {literal_miss:.5f}")
    return ok


def dev_set(key, value):
    """Set a development register (csrc/hpc_dev.h).  They exist only in the development build of the library
    (`HPC_AMD_DEV=1` -> hpc/libhpc_amd_dev.so); the product has none, so against the product a non-zero value SKIPS
    the test case - tests/test_dev_build.py re-runs every test marked `dev` in a subprocess with HPC_AMD_DEV=1 - and
    a zero (= the shipped configuration) is a no-op."""
    import hpc

    if hpc._C.DEV_BUILD:
        assert hpc._C.lib.hpc_dev_tuning_set(key, value) == 0
    elif value != 0:
        pytest.skip("pins a kernel variant through a development register: runs against the development build "
                    "(tests/test_dev_build.py)")


# Rows per expert that put one group through every site of the 256 x 256 grouped GEMM's fused activation epilogue
# (n = 2 * inter = 512, k = hidden = 512, 231 rows per group on average: csrc/group_gemm_route.h picks that kernel with the
# epilogue; csrc/group_gemm_p8.hip, locate_item and the dispatch in gemm_fp8_p8_kernel, pick the body):
#   265  one full tile that carries the 9 rows behind it as its ride-along block (9 <= 16 per full tile)
#   40   the tail body, as the group's only tile
#   100  the half-tile body (65 ... 128 rows)
#   456  a full tile, then a 200-row last tile on the full body
#   296  a full tile, then a 40-row tail body that is not the group's only tile (40 > 16: no ride-along)
EPILOGUE_SITE_ROWS = [265, 40, 100, 456, 296]


def topk1_ids_with_rows(rows):
    """topk_ids [sum(rows), 1], constructed: expert e receives exactly rows[e] tokens, its tokens spread over the batch by
    a fixed stride that is coprime with the token count."""
    n = sum(rows)
    stride = next(s for s in range(n // 3, n) if math.gcd(s, n) == 1)
    ids = torch.repeat_interleave(torch.arange(len(rows), dtype=torch.int32), torch.tensor(rows))
    out = torch.empty(n, dtype=torch.int32)
    out[(torch.arange(n) * stride) % n] = ids
    assert torch.bincount(out.long(), minlength=len(rows)).tolist() == list(rows)
    return out.view(n, 1)
