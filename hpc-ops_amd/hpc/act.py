"""hpc.act — activation + quant surface used by the fused MoE (reference hpc/act.py:7-114), including the
masked (DeepEP-layout) variants, and the 128-block quantiser of its input (blockwise_fp8_quant, ours)."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _C  # noqa: F401  (loads the libraries that register torch.ops.hpc.*)


def act_mul_and_quant(gate_up: Tensor, scale: Tensor, use_bf16_mul: bool = True,
                      output: Tensor = None) -> Tensor:
    """e4m3( silu(gate_up[:, :C]) * gate_up[:, C:] * scale[0] ) for bf16 gate_up [N, 2C]; with
    use_bf16_mul the product is rounded through bf16 like the reference kernel."""
    return torch.ops.hpc.act_mul_and_quant(gate_up, scale, use_bf16_mul, output)


def scaled_fp8_quant(input: Tensor, scale: Tensor, output: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Quantise a float32 / float16 / bfloat16 tensor to e4m3 with one per-tensor scale: output = e4m3(input *
    (1 / scale[0])), saturating; returns (output, scale) like the reference (hpc/act.py:108-114,
    src/activation/activation.cu:461-505)."""
    return torch.ops.hpc.scaled_fp8_quant(input, scale, output)


def masked_act_mul_and_quant(gate_up: Tensor, scale: Tensor, num_per_expert: Tensor,
                             output: Optional[Tensor] = None) -> Tensor:
    """DeepEP layout: gate_up bf16 [num_expert * padded_tokens, 2C], only the first num_per_expert[e] rows of
    expert e are valid: e4m3(silu(gate) * up * scale[0]) for those rows, the others are left untouched
    (reference hpc/act.py:37-67)."""
    return torch.ops.hpc.masked_act_mul_and_quant(gate_up, scale, num_per_expert, output)


def masked_act_mul_and_blockwise_quant(gate_up: Tensor, num_per_expert: Tensor, output: Optional[Tensor] = None,
                                       output_scale: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """DeepEP layout, 128-block quantisation: a = silu(gate) * up, scale = amax_128(|a|) / 448 -> float32
    [N, C/128], q = e4m3(a / (scale + 1e-8)) -> [N, C]; valid rows only (reference hpc/act.py:70-105)."""
    return torch.ops.hpc.masked_act_mul_and_blockwise_quant(gate_up, num_per_expert, output, output_scale)


def blockwise_fp8_quant(input: Tensor, output: Optional[Tensor] = None,
                        output_scale: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """128-block e4m3 quantisation of hidden states: returns (q float8_e4m3fn [T, H], scale float32 [T, H/128]), the
    (x, x_scale) pair fuse_moe_blockwise* and group_gemm_blockwise_fp8 take - e.g. of the bf16 output of
    fuse_allreduce_rmsnorm_*.  No reference counterpart (torch.ops.hpc_quant.blockwise_fp8_quant); semantics = PyTorch,
    in fp32, per row and block b of 128 consecutive columns - the rule of the MoE's own activation quantiser:
        amax = max |a[b*128:(b+1)*128]|;  scale = amax / 448;  q = e4m3fn(a * (1 / (scale + 1e-8)))
    An all-zero block gives scale 0 and q 0; a NaN or Inf leaves its own block unspecified, fp32 denormals too.

    input: bfloat16, float16 or float32 [T, H], contiguous, H % 128 == 0, 128 <= H <= 16384.  output / output_scale, when
    given, are written and returned as the same objects (nothing is allocated: the call captures into a hipGraph).
    T == 0 returns empty tensors without a launch."""
    q, scale = torch.ops.hpc_quant.blockwise_fp8_quant(input, output, output_scale)
    return (q if output is None else output), (scale if output_scale is None else output_scale)


@torch.library.register_fake("hpc_quant::blockwise_fp8_quant")
def _blockwise_fp8_quant_fake(input, output=None, output_scale=None):
    t, h = input.shape
    out = output if output is not None else torch.empty((t, h), dtype=torch.float8_e4m3fn, device=input.device)
    osc = output_scale if output_scale is not None else torch.empty((t, h // 128), dtype=torch.float32, device=input.device)
    return out, osc


@torch.library.register_fake("hpc::masked_act_mul_and_quant")
def _masked_act_mul_and_quant_fake(input, scale, num_per_expert, output=None):
    if output is not None:
        return output
    return torch.empty(tuple(input.shape[:-1]) + (input.shape[-1] // 2,), dtype=torch.float8_e4m3fn, device=input.device)


@torch.library.register_fake("hpc::masked_act_mul_and_blockwise_quant")
def _masked_act_mul_and_blockwise_quant_fake(input, num_per_expert, output=None, output_scale=None):
    n, c = input.shape[0], input.shape[1] // 2
    out = output if output is not None else torch.empty((n, c), dtype=torch.float8_e4m3fn, device=input.device)
    osc = output_scale if output_scale is not None else torch.empty((n, c // 128), dtype=torch.float32,
                                                                    device=input.device)
    return out, osc


@torch.library.register_fake("hpc::act_mul_and_quant")
def _act_mul_and_quant_fake(input, scale, use_bf16_mul, output):
    if output is not None:
        return output
    return torch.empty(tuple(input.shape[:-1]) + (input.shape[-1] // 2,), dtype=torch.float8_e4m3fn, device=input.device)


@torch.library.register_fake("hpc::scaled_fp8_quant")
def _scaled_fp8_quant_fake(input, scale, output):
    out = output if output is not None else torch.empty_like(input, dtype=torch.float8_e4m3fn)
    sc = scale if scale is not None else torch.empty((1,), dtype=torch.float32, device=input.device)
    return out, sc
