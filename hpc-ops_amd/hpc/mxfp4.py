"""hpc.mxfp4 — OCP MXFP4 expert weights (W4A8) for decode steps: the grouped GEMM and the fused MoE on it.

Weights are e2m1 codes, two per byte with the even k in the low nibble, with one e8m0 scale byte per 32 values - checkpoint
layout, read as it is.  Activations are e4m3 with float32 scales per 128 values, the pair `hpc.blockwise_fp8_quant` writes.
The ops live in torch.ops.hpc_mxfp4 (torch.ops.hpc carries the reference's surface only); the statement of their arithmetic is
tests/mxfp4_ref.py.  Meant for decode-sized groups: correct at any group length, but longer groups only take more passes over
the weights (no tile kernel).
"""
import torch
from torch import Tensor

from . import _C  # noqa: F401  (loads the libraries that register torch.ops.hpc_mxfp4.*)

_PACKED = tuple(getattr(torch, n) for n in ("float4_e2m1fn_x2", "float8_e8m0fnu") if hasattr(torch, n))


def _u8(t: Tensor) -> Tensor:
    """torch.float4_e2m1fn_x2 / torch.float8_e8m0fnu tensors are taken as the bytes they are"""
    return t.view(torch.uint8) if t.dtype in _PACKED else t


def group_gemm_mxfp4(x: Tensor, x_scale: Tensor, weight: Tensor, weight_scale: Tensor, seqlens: Tensor, cu_seqlens: Tensor, *,
                     output: Tensor = None) -> Tensor:
    """y[r] = bf16(sum_kb x_scale[r, kb] * sum_{k in block kb} x[r, k] * e2m1(weight[g, :, k]) * 2^(weight_scale[g, :, k / 32] - 127))
    for the seqlens[g] rows from cu_seqlens[g] on.

    x e4m3 [M, K], x_scale float32 [M, K / 128]; weight uint8 (or float4_e2m1fn_x2) [G, N, K / 2]; weight_scale uint8 (or
    float8_e8m0fnu) [G, N, K / 32]; seqlens int32 [G], cu_seqlens int32 [G] or [G + 1].  K % 128 == 0, N % 64 == 0.  Returns bf16
    [M, N] (`output` when given).  G = 1 serves a dense layer or a shared expert.
    """
    return torch.ops.hpc_mxfp4.group_gemm(x, x_scale, _u8(weight), _u8(weight_scale), seqlens, cu_seqlens, None, output)


def fuse_moe_mxfp4(x: Tensor, x_scale: Tensor, gate_up_weight: Tensor, gate_up_weight_scale: Tensor, down_weight: Tensor,
                   down_weight_scale: Tensor, topk_ids: Tensor, topk_scale: Tensor, rank_ep: int, num_expert_total: int,
                   shared_output: Tensor = None, output: Tensor = None) -> Tensor:
    """Fused MoE on MXFP4 expert weights: `hpc.fuse_moe_blockwise`'s pipeline with the MXFP4 grouped GEMM in both places.

    x e4m3 [T, H] with x_scale float32 [T, H / 128]; gate_up_weight [E, 2I, H / 2] with scales [E, 2I, H / 32]; down_weight
    [E, H, I / 2] with scales [E, H, I / 32]; topk_ids int32 [T, k] (global expert ids; local experts are [rank_ep * E,
    (rank_ep + 1) * E)), topk_scale float32 [T, k]; optional shared_output bf16 [T, H].  H % 128 == 0, 2I % 256 == 0, k <= 128.
    Returns bf16 [T, H].  No host sync; with `output` given the call can be captured into a hipGraph.
    """
    return torch.ops.hpc_mxfp4.fuse_moe(x, x_scale, _u8(gate_up_weight), _u8(gate_up_weight_scale), _u8(down_weight),
                                        _u8(down_weight_scale), topk_ids, topk_scale, shared_output, rank_ep, num_expert_total,
                                        output)


@torch.library.register_fake("hpc_mxfp4::group_gemm")
def group_gemm_mxfp4_fake(x, x_scale, weight, weight_scale, seqlens, cu_seqlens, row_index, output):
    m = x.size(0) if row_index is None else row_index.size(0)
    return torch.empty((m, weight.size(1)), dtype=torch.bfloat16, device=x.device)


@torch.library.register_fake("hpc_mxfp4::fuse_moe")
def fuse_moe_mxfp4_fake(x, x_scale, gate_up_weight, gate_up_weight_scale, down_weight, down_weight_scale, topk_ids, topk_scale,
                        shared_output, rank_ep, num_expert_total, output):
    return torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
