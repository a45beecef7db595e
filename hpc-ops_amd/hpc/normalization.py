"""hpc.normalization — fused RMSNorm + FP8 quantisation (public surface of reference hpc/normalization.py:6-53), and the
form with one scale per 128 columns in front of the blockwise fused MoE (fused_rmsnorm_blockwise_quant, ours)."""
from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from . import _C  # noqa: F401  (loads the libraries that register torch.ops.hpc.*)

_F8 = torch.float8_e4m3fn


def fused_rmsnorm_with_scale(a: Tensor, weight: Tensor, eps: float = torch.finfo(torch.float32).eps,
                             scale: Tensor = torch.tensor([1], dtype=torch.float32),
                             is_moe: bool = False) -> Union[Tensor, Tuple[Tensor]]:
    """y = a * rsqrt(mean(a^2) + eps) * weight, quantised to float8_e4m3fn as y / scale[0].

    a: bfloat16 [rows, hidden] (hidden % 8 == 0, <= 16384; the reference instantiates 320 / 4096 / 5120 only);
    weight: bfloat16 [hidden] or [1, hidden]; scale: float32 [1] ([2] with is_moe; moved to a's device).
    Returns the fp8 tensor, or with is_moe the triple (y in fp32, y / scale[0] in fp8, y / scale[1] in fp8).
    """
    dev_scale = scale if scale.device == a.device else scale.to(a.device)
    q0, y32, q1 = torch.ops.hpc.fused_rmsnorm_with_scale(a, weight, dev_scale, eps, is_moe)
    if is_moe:
        return y32, q0, q1
    return q0


@torch.library.register_fake("hpc::fused_rmsnorm_with_scale")
def fused_rmsnorm_with_scale_fake(a, weight, scale, eps, is_moe):
    # schema order (input, weight, scale, eps, is_moe) - the reference's fake swaps eps / scale
    # (hpc/normalization.py:44-53); the op always has three outputs
    return (torch.empty_like(a, dtype=_F8), torch.empty_like(a, dtype=torch.float32), torch.empty_like(a, dtype=_F8))


def fused_rmsnorm_blockwise_quant(a: Tensor, weight: Tensor, eps: float = 1e-6, residual: Optional[Tensor] = None,
                                  return_normed: bool = False, output: Optional[Tensor] = None,
                                  output_scale: Optional[Tensor] = None,
                                  output_normed: Optional[Tensor] = None) -> Tuple[Tensor, ...]:
    """Residual add + RMSNorm + 128-block e4m3 quantisation in one kernel: returns (q float8_e4m3fn [T, H], scale float32
    [T, H/128]) - the (x, x_scale) pair fuse_moe_blockwise* takes - or (q, scale, y) with return_normed, y the bfloat16
    [T, H] normed rows the router GEMM (gemm_bf16xfp32) consumes.  No reference counterpart
    (torch.ops.hpc_quant.fused_rmsnorm_blockwise_quant); semantics = PyTorch:
        h = a, or with residual h = bf16(a.float() + residual.float()), stored to residual IN PLACE and normed as rounded
            (the order of fuse_allreduce_rmsnorm_*)
        y = bf16(h.float() * rsqrt(mean(h.float()^2) + eps) * weight.float())     fp32 throughout, rounded once
        q, scale = blockwise_fp8_quant(y)                                          of the bf16-ROUNDED y, bit for bit
    so this op and "norm to bf16, then blockwise_fp8_quant" hand the MoE identically quantised rows.

    a: bfloat16 [T, H], contiguous, H % 128 == 0, 128 <= H <= 16384, never written; weight: bfloat16 [H] or [1, H];
    residual: bfloat16 [T, H].  output / output_scale / output_normed (the last with return_normed only), when given, are
    written and returned as the same objects; with all of them given nothing is allocated and the call captures into a
    hipGraph.  The buffers must not overlap.  T == 0 returns empty tensors without a launch."""
    q, scale, y = torch.ops.hpc_quant.fused_rmsnorm_blockwise_quant(a, weight, eps, residual, return_normed, output,
                                                                    output_scale, output_normed)
    q = q if output is None else output
    scale = scale if output_scale is None else output_scale
    if return_normed:
        return q, scale, (y if output_normed is None else output_normed)
    return q, scale


@torch.library.register_fake("hpc_quant::fused_rmsnorm_blockwise_quant")
def _fused_rmsnorm_blockwise_quant_fake(a, weight, eps, residual, return_normed, output=None, output_scale=None,
                                        output_normed=None):
    # the op always has three outputs: the third is an empty [0] tensor without return_normed
    t, h = a.shape
    q = output if output is not None else torch.empty((t, h), dtype=_F8, device=a.device)
    sc = output_scale if output_scale is not None else torch.empty((t, h // 128), dtype=torch.float32, device=a.device)
    if not return_normed:
        y = torch.empty((0,), dtype=a.dtype, device=a.device)
    else:
        y = output_normed if output_normed is not None else torch.empty_like(a)
    return q, sc, y
