"""hpc.gemm — router GEMM with an fp32 weight carried as two bf16 planes (reference hpc/gemm.py:7-80), the top-k routers
and the dense FP8 linear with 128-block scales."""
import torch
from torch import Tensor

from . import _C  # noqa: F401  (loads the libraries that register torch.ops.hpc.*)


def get_gemm_bf16xfp32_workspace(max_weight_hidden_size: int, max_tokens: int = 131072) -> Tensor:
    """Zeroed split-K arrival counters, one per (16-token, 64-row) tile (reference hpc/gemm.py:7-13)."""
    nm_max = (max_tokens + 15) // 16
    nn_max = (max_weight_hidden_size + 63) // 64
    return torch.zeros((nm_max, nn_max), dtype=torch.int32, device="cuda")


def gemm_bf16xfp32(
    x: Tensor,
    w_high: Tensor,
    w_low: Tensor,
    scale: float,
    use_fp32_output: bool = False,
    use_splitk: bool = True,
    split_flag: Tensor = None,
) -> Tensor:
    """y = x @ (w_high + scale * w_low)^T with fp32 accumulation, where w_high = bf16(w_fp32) and
    w_low = bf16((w_fp32 - w_high) / scale), scale = 1/256.
    x [m, k] bf16; w_high, w_low [n, k] bf16 (n % 64 == 0, k % 64 == 0); returns [m, n] bf16 (or fp32
    with use_fp32_output).  split_flag (optional, from get_gemm_bf16xfp32_workspace) must be zero on
    entry and is zero again on exit."""
    return torch.ops.hpc.gemm_bf16xfp32(x, w_high, w_low, scale, use_fp32_output, use_splitk, split_flag)


@torch.library.register_fake("hpc::gemm_bf16xfp32")
def _gemm_bf16xfp32_fake(a, b_high, b_low, scale, use_fp32_output=False, use_splitk=True, split_flag=None):
    return torch.empty((a.shape[0], b_high.shape[0]), dtype=torch.float32 if use_fp32_output else a.dtype,
                       device=a.device)


def topk_router(logits: Tensor, topk: int, renormalize: bool = True, topk_ids: Tensor = None,
                topk_scale: Tensor = None):
    """Fused softmax + top-k over the router logits (the fp32 output of gemm_bf16xfp32): returns
    (topk_ids int32 [m, topk], topk_scale float32 [m, topk]) - what fuse_moe / fuse_moe_blockwise_fp8 take.

    No reference counterpart (the reference stops at the GEMM); semantics = stable PyTorch:
    ids = argsort(logits, descending, stable)[:, :topk] (ties -> smaller expert id, bit-exact),
    p = softmax(logits.float(), -1), scale = p[ids] (renormalize=False) or p[ids] / p[ids].sum(-1) (True).
    logits [m, num_expert] float32, num_expert % 4 == 0 and <= 1024, topk <= 64."""
    return torch.ops.hpc.topk_router(logits, topk, renormalize, topk_ids, topk_scale)


@torch.library.register_fake("hpc::topk_router")
def _topk_router_fake(logits, topk, renormalize=True, topk_ids=None, topk_scale=None):
    m = logits.shape[0]
    return (torch.empty((m, topk), dtype=torch.int32, device=logits.device),
            torch.empty((m, topk), dtype=torch.float32, device=logits.device))


def grouped_topk_router(logits: Tensor, topk: int, num_expert_group: int = 1, topk_group: int = 1,
                        correction_bias: Tensor = None, scoring_func: str = "sigmoid", renormalize: bool = True,
                        routed_scaling_factor: float = 1.0, topk_ids: Tensor = None, topk_scale: Tensor = None):
    """Group-limited top-k router (DeepSeek-V3 / R1 and Kimi-K2: sigmoid + correction bias; DeepSeek-V2: softmax, no
    bias) over the fp32 output of gemm_bf16xfp32: returns (topk_ids int32 [m, topk], topk_scale float32 [m, topk]) -
    what fuse_moe / fuse_moe_blockwise_fp8 take.

    No reference counterpart; semantics = PyTorch, in fp32:
    s = sigmoid(logits) or softmax(logits, -1) (scoring_func "sigmoid" / "softmax"); c = s + correction_bias (c = s
    without one).  Group g is the contiguous expert range [g * gs, (g + 1) * gs), gs = num_expert // num_expert_group;
    its score is the sum of its two best c with a bias, its best c without.  The topk_group best groups stay (ties ->
    smaller group id), ids = argsort(c over the experts of those groups, descending, stable)[:, :topk] (ties -> smaller
    expert id, best first), scale = s[ids] - the UNBIASED scores -, divided by (scale.sum(-1) + 1e-20) with
    renormalize, times routed_scaling_factor.  num_expert_group == topk_group keeps every group.  A row that holds a
    NaN has an unspecified result with ids in range.
    logits [m, num_expert] float32 with 16-byte aligned rows, num_expert % 4 == 0 and <= 1024, gs % 4 == 0,
    topk <= min(64, topk_group * gs); correction_bias contiguous float32 [num_expert]."""
    return torch.ops.hpc_router.grouped_topk_router(logits, correction_bias, topk, num_expert_group, topk_group,
                                                    scoring_func, renormalize, routed_scaling_factor, topk_ids, topk_scale)


@torch.library.register_fake("hpc_router::grouped_topk_router")
def _grouped_topk_router_fake(logits, correction_bias, topk, num_expert_group, topk_group, scoring_func, renormalize,
                              routed_scaling_factor, topk_ids=None, topk_scale=None):
    m = logits.shape[0]
    return (torch.empty((m, topk), dtype=torch.int32, device=logits.device),
            torch.empty((m, topk), dtype=torch.float32, device=logits.device))


def gemm_blockwise_fp8(x: Tensor, x_scale: Tensor, weight: Tensor, weight_scale: Tensor, *, output: Tensor = None,
                       splits: int = 0) -> Tensor:
    """Dense FP8 linear with 128-block scales for decode batches: the Q/KV/O projections, dense and shared-expert MLPs
    and the LM head of a block-scaled FP8 model (DeepSeek-V3, Qwen3 FP8 checkpoints).  Returns y bf16 [M, N].

    No reference counterpart; semantics = the PyTorch statement tests/linear_fp8_ref.py, in fp32 or better:

        y[m, n] = bf16( sum_kb x_scale[m, kb] * weight_scale[n // 128, kb]
                               * sum_{k in block kb} float(x[m, k]) * float(weight[n, k]) )

    with kb running over the K / 128 blocks of 128 consecutive k.

    Layouts:
      x             float8_e4m3fn [M, K], contiguous;
      x_scale       float32 [M, K / 128], contiguous - (x, x_scale) is what blockwise_fp8_quant and
                    fused_rmsnorm_blockwise_quant return, as they return it;
      weight        float8_e4m3fn [N, K], contiguous;
      weight_scale  float32 [ceil(N / 128), K / 128], stride(1) == 1 and stride(0) >= K / 128: the checkpoint's layout
                    and rows padded to a multiple of four floats are both taken;
      output        bfloat16 [M, N], contiguous.  When given it is written and returned (the same object) and nothing
                    is allocated per call beyond the cached scratch, so the call captures into a hipGraph.

    Limits: K % 128 == 0, K >= 128; N % 64 == 0 (an N that ends inside a 128-row scale block, such as 576 or 2112, is
    fine); N * K <= 0xfffffff0 bytes; 1 <= M <= 256 - decode batches and speculative steps.  M == 0 returns an empty
    [0, N] tensor without a launch; M > 256 is refused: use group_gemm_blockwise_fp8 for prefill-sized calls.  NaN / Inf
    inputs: unspecified.

    splits: the number of K slices the weight stream is cut into, each slice a workgroup of its own per 64 weight rows
    and 64 tokens.  0 = the library chooses (enough to give every CU one to two workgroups, every slice at least four
    k-blocks); 1 .. max = the caller's count, max = min(16, K / 128) - what torch.ops / hpc_gemm_blockwise_fp8_plan
    reports; beyond it the call is refused.  With more than one slice the partial sums go through a cached scratch buffer
    per (device, stream, hipGraph capture) that hpc.release_decode_workspaces() drops.

    Determinism: the result for a given (M, N, K, splits, CU count) is bit-identical from call to call - the slices of
    a tile are summed in slice order 0 .. S - 1 by whichever arrives last, never in arrival order, and no float atomics
    are used.  Different split counts may differ in the last bit of the fp32 sum."""
    y = torch.ops.hpc_linear.gemm_blockwise_fp8(x, x_scale, weight, weight_scale, output, splits)
    return y if output is None else output


@torch.library.register_fake("hpc_linear::gemm_blockwise_fp8")
def _gemm_blockwise_fp8_fake(x, x_scale, weight, weight_scale, output=None, splits=0):
    if output is not None:
        return output
    return torch.empty((x.shape[0], weight.shape[0]), dtype=torch.bfloat16, device=x.device)
