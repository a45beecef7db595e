"""The FP8 latent KV cache of hpc.attention_decode_mla_fp8 / hpc.mla_rope_norm_store_kv_fp8 on CPU tensors: the row's layout,
the writer's quantisation and the reader's dequantisation, restated from the ops' contract (csrc/mla_fp8_format.h).

    one token = 656 bytes:   0 .. 511  512 float8_e4m3fn codes, column d at byte d
                           512 .. 527  four little-endian float32 scales, scale g for columns 128 g .. 128 g + 127
                           528 .. 655  64 bfloat16: the RoPE'd k_pe, unquantised

    dequantise:  c[d] = bf16_rne( fp32(code[d]) * scale[d // 128] )      one fp32 multiply, one rounding
    quantise:    per group of 128 columns of the bf16 row, scale = amax / 448, code = e4m3fn(lat * (1 / (scale + 1e-8))), in fp32
                 = tests/blockwise_quant_ref.py::quant on the 512 columns"""
import torch

import blockwise_quant_ref as bq

ROW, CODES_AT, SCALES_AT, ROPE_AT = 656, 0, 512, 528
LAT, ROPE, GROUPS = 512, 64, 4
VARY = (1.0, 1.5, 2.0, 3.0)  # the factors quantise(vary_seed=...) multiplies scales by: all exact in fp32


def pack(codes, scales, rope):
    """codes float8_e4m3fn [..., 512], scales float32 [..., 4], rope bfloat16 [..., 64] -> uint8 [..., 656]"""
    assert codes.dtype == torch.float8_e4m3fn and scales.dtype == torch.float32 and rope.dtype == torch.bfloat16
    assert codes.shape[-1] == LAT and scales.shape[-1] == GROUPS and rope.shape[-1] == ROPE
    return torch.cat([codes.contiguous().view(torch.uint8), scales.contiguous().view(torch.uint8),
                      rope.contiguous().view(torch.uint8)], -1)


def unpack(cache_u8):
    """uint8 [..., 656] (any strides) -> (codes float8_e4m3fn [..., 512], scales float32 [..., 4], rope bfloat16 [..., 64])"""
    assert cache_u8.dtype == torch.uint8 and cache_u8.shape[-1] == ROW
    c = cache_u8.contiguous()
    return (c[..., CODES_AT: SCALES_AT].contiguous().view(torch.float8_e4m3fn),
            c[..., SCALES_AT: ROPE_AT].contiguous().view(torch.float32), c[..., ROPE_AT:].contiguous().view(torch.bfloat16))


def quantise(ckv_bf16, vary_seed=None):
    """bfloat16 [..., 576] -> uint8 [..., 656].  Without vary_seed: what the writer produces.  With it every (token, group)
    scale is multiplied by a factor drawn from VARY before the codes are formed - scales the writer never emits, which the
    reader must honour all the same."""
    assert ckv_bf16.dtype == torch.bfloat16 and ckv_bf16.shape[-1] == LAT + ROPE
    lead = ckv_bf16.shape[:-1]
    lat = ckv_bf16[..., :LAT].reshape(-1, LAT)
    if vary_seed is None:
        codes, scales = bq.quant(lat)
    else:
        g = torch.Generator().manual_seed(vary_seed)
        b = lat.float().view(-1, GROUPS, 128)
        scales = b.abs().amax(-1) / 448.0 * torch.tensor(VARY)[torch.randint(0, len(VARY), (b.shape[0], GROUPS), generator=g)]
        codes = (b * (1.0 / (scales + 1e-8)).unsqueeze(-1)).to(torch.float8_e4m3fn).view(-1, LAT)
    return pack(codes.view(*lead, LAT), scales.view(*lead, GROUPS), ckv_bf16[..., LAT:])


def dequantise(cache_u8):
    """uint8 [..., 656] -> bfloat16 [..., 576]: the only meaning the codes have"""
    codes, scales, rope = unpack(cache_u8)
    lat = (codes.float().view(*codes.shape[:-1], GROUPS, 128) * scales.unsqueeze(-1)).to(torch.bfloat16)
    return torch.cat([lat.view(*codes.shape[:-1], LAT), rope], -1)
