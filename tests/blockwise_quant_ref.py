"""The PyTorch statement of hpc.blockwise_fp8_quant and hpc.fused_rmsnorm_blockwise_quant (no reference kernel exists).
CPU tensors only."""
import torch


def quant(a):
    """a [T, H] (any float dtype, values taken to fp32), H % 128 == 0 -> (q float8_e4m3fn [T, H], scale float32 [T, H/128]):
    per block of 128 consecutive columns scale = amax / 448, q = e4m3fn(a * (1 / (scale + 1e-8))), every step in fp32 - the
    arithmetic of oracle/fuse_moe.py::act_mul_and_blockwise_quant without the activation."""
    assert a.device.type == "cpu" and a.dim() == 2 and a.shape[1] % 128 == 0, (a.device, a.shape)
    t, h = a.shape
    b = a.float().view(t, h // 128, 128)
    s = b.abs().amax(-1) / 448.0
    inv = 1.0 / (s + 1e-8)
    q = (b * inv.unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.view(t, h), s


def norm64(a, weight, eps, residual=None):
    """(h bfloat16 [T, H], y float64 [T, H]): h = a, or bf16(a + residual) summed in fp32 and rounded once (the order of
    oracle/allreduce.py::ref_allreduce_rmsnorm); y = h * rsqrt(mean(h^2) + eps) * weight in float64, NOT rounded."""
    assert a.device.type == "cpu" and a.dtype == torch.bfloat16, (a.device, a.dtype)
    h = a if residual is None else (a.float() + residual.float()).bfloat16()
    h64 = h.double()
    y = h64 * torch.rsqrt(h64.pow(2).mean(-1, keepdim=True) + eps) * weight.double().reshape(1, -1)
    return h, y
