"""hpc.attention_decode_mla_fp8: MLA decode attention over the FP8 latent KV cache (656 bytes per token).

CPU: the cache helper (tests/mla_fp8_ref.py) against the layout and tests/blockwise_quant_ref.py; the bars of tests/mla_needles.py
measured again on dequantised caches - the split model stays within them, mutants of the FP8 path (scales ignored, the next
group's scale, the page neighbour's scale, the unquantised values) are rejected at >= 3 tau; the public surface and fakes; host
refusals through the C-ABI with never-dereferenced pointers.
GPU: equality with hpc.attention_decode_mla_bf16 on the dequantised cache bit for bit (the design's property: the same LDS
image, the same code behind it), needle parity against the float64 statement, exact one-token results, strided caches, forced
splits over NaN-filled scratch, a hipGraph replayed after everything changed in place, guard bands, refusals, repeatability."""
import ctypes
import functools
from ctypes import c_float, c_int, c_int64, c_void_p
from pathlib import Path

import pytest
import torch

import blockwise_quant_ref as bq
import mla_fp8_ref as f8
import mla_needles as mn
import mla_ref
from utils import attn_close, attn_rel_err

DIM, DIM_V = mla_ref.DIM, mla_ref.DIM_V
MAX_SPLITS = 64
VARY_SEED = 1234


# ---- CPU 1: the helper ---------------------------------------------------------------------------------------------------------
def test_layout_constants():
    assert (f8.CODES_AT, f8.SCALES_AT, f8.ROPE_AT, f8.ROW) == (0, 512, 528, 656)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, DIM, generator=g).bfloat16()
    u = f8.quantise(x)
    assert u.dtype == torch.uint8 and u.shape == (3, 5, 656)
    codes, scales = bq.quant(x[..., :512].reshape(-1, 512))
    assert torch.equal(u[..., :512].reshape(-1, 512), codes.view(torch.uint8))                       # column d at byte d
    assert torch.equal(u[..., 512:528].contiguous().view(torch.float32).reshape(-1, 4), scales)      # little-endian fp32
    assert torch.equal(u[..., 528:].contiguous().view(torch.bfloat16), x[..., 512:])                 # k_pe untouched
    assert u[0, 0, 512:516].tolist() == list(scales[0, 0].numpy().tobytes())


def test_pack_unpack_round_trip():
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, 256, (4, 7, 512), generator=g, dtype=torch.uint8).view(torch.float8_e4m3fn)
    scales = torch.rand(4, 7, 4, generator=g)
    rope = torch.randn(4, 7, 64, generator=g).bfloat16()
    c, s, r = f8.unpack(f8.pack(codes, scales, rope))
    assert torch.equal(c.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(s, scales)
    assert torch.equal(r.view(torch.int16), rope.view(torch.int16))
    u = torch.randint(0, 256, (2, 3, 656), generator=g, dtype=torch.uint8)
    assert torch.equal(f8.pack(*f8.unpack(u)), u)
    padded = torch.zeros(2, 3, 704, dtype=torch.uint8)
    padded[..., :656] = u
    assert torch.equal(f8.pack(*f8.unpack(padded[..., :656])), u)  # a strided view


def test_quantise_is_the_projects_quantiser_bit_for_bit():
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(50, DIM, generator=g) * torch.logspace(-4, 2, 50)[:, None]).bfloat16()
    codes, scales, _ = f8.unpack(f8.quantise(x))
    rc, rs = bq.quant(x[:, :512])
    assert torch.equal(codes.view(torch.uint8), rc.view(torch.uint8)) and torch.equal(scales.view(torch.int32), rs.view(torch.int32))


def test_a_zero_group_is_scale_zero_codes_zero_and_dequantises_to_zero():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, DIM, generator=g).bfloat16()
    x[2, 128:256] = 0
    x[4, :512] = 0
    u = f8.quantise(x)
    codes, scales, _ = f8.unpack(u)
    assert scales[2, 1] == 0 and bool((codes[2, 128:256].view(torch.uint8) == 0).all()) and bool((scales[4] == 0).all())
    d = f8.dequantise(u)
    assert bool((d[2, 128:256].view(torch.int16) == 0).all()) and bool((d[4, :512].view(torch.int16) == 0).all())
    assert torch.equal(d[:, 512:], x[:, 512:])
    # a scale of 0 makes its group zeros whatever the codes say
    u[1, 512:516] = 0
    assert bool((f8.dequantise(u)[1, :128] == 0).all())


def test_varied_scales_are_not_the_writers_and_round_trip_within_the_format():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(64, DIM, generator=g).bfloat16()
    plain, varied = f8.unpack(f8.quantise(x)), f8.unpack(f8.quantise(x, vary_seed=5))
    ratio = (varied[1].double() / plain[1].double()).flatten().tolist()
    assert {round(r, 4) for r in ratio} == set(f8.VARY)  # every factor occurs, nothing else
    # e4m3 has 3 mantissa bits: a value is within 2^-4 of itself relative, or half the smallest subnormal step of its scale
    for q in (f8.quantise(x), f8.quantise(x, vary_seed=5)):
        d, s = f8.dequantise(q)[:, :512].float(), f8.unpack(q)[1].repeat_interleave(128, 1)
        err = (d - x[:, :512].float()).abs()
        assert bool((err <= torch.maximum(x[:, :512].float().abs() * (2.0 ** -4 + 2.0 ** -8), s * 2.0 ** -10 * 1.01)).all())


# ---- CPU 2: the bars carry over ------------------------------------------------------------------------------------------------
# (lens before the step, Sq, H, P): three of the bf16 op's calibration cases
_CAL = [([0, 1, 63, 64, 1500, 4000], 2, 16, 64), ([0, 15, 16, 17, 65, 300], 4, 32, 16), ([5000, 700, 129], 1, 48, 32)]


@functools.lru_cache(maxsize=None)
def _cal_case(i):
    """(inputs over the dequantised cache, the cache, the original inputs, the statement's result), computed once"""
    lens, sq, H, P = _CAL[i]
    orig = mn.needle_inputs(lens, sq, P, H, seed=11)
    cache = f8.quantise(orig["ckv"], vary_seed=VARY_SEED + i)
    inp = dict(orig, ckv=f8.dequantise(cache))
    return inp, cache, orig, mn.statement(inp)


def test_split_model_within_bars_on_dequantised_caches():
    """what the kernel computes behind the gather, on the caches the FP8 op's tests use: within the bf16 op's bars"""
    w_tau, w_lse = 0.0, 0.0
    for i in range(len(_CAL)):
        inp, _, _, (ref, rlse) = _cal_case(i)
        for R in mn.PIECE_LENS:
            out, l = mn.split_model(inp, R)
            w_tau = max(w_tau, float(attn_rel_err(ref, out, inp["num_seq_q"]).max()))
            w_lse = max(w_lse, mn.lse_err(rlse, l))
    print(f"\ndequantised needle caches: split model worst out {w_tau:.5f} (tau {mn.TAU_NEEDLE} = {mn.TAU_NEEDLE / w_tau:.2f} x), "
          f"worst lse {w_lse:.3g} (bar {mn.LSE_BAR_NEEDLE} = {mn.LSE_BAR_NEEDLE / w_lse:.2f} x) over piece lengths {mn.PIECE_LENS}")
    assert w_tau <= mn.TAU_NEEDLE, w_tau
    assert w_lse <= mn.LSE_BAR_NEEDLE, w_lse


@pytest.mark.parametrize("i", range(len(_CAL)))
def test_needle_bar_rejects_mutants_of_the_fp8_path(i):
    """each mutant of a plausible bug of the FP8 gather, run through the statement, is >= 3 tau off the statement on the
    dequantised cache"""
    inp, cache, orig, (ref, _) = _cal_case(i)
    sq, P = inp["num_seq_q"], inp["P"]
    codes, scales, rope = f8.unpack(cache)

    def deq(s):
        return f8.dequantise(f8.pack(codes, s.contiguous(), rope))

    mutants = {
        "RoPE columns ignored": mn.statement(inp, use_rope=False)[0],
        "last token of a page lost": mn.statement(inp, drop=lambda L: range(P - 1, L, P))[0],
        "scales ignored": mn.statement(dict(inp, ckv=deq(torch.ones_like(scales))))[0],
        "group g read with group g + 1's scale": mn.statement(dict(inp, ckv=deq(scales.roll(-1, -1))))[0],
        "a token read with its page neighbour's scale": mn.statement(dict(inp, ckv=deq(scales.roll(1, 1))))[0],
        "the unquantised bf16 values where the codes should be": mn.statement(orig)[0],
    }
    if sq > 1:
        mutants["causal limit + 1"] = mn.statement(inp, causal_shift=1)[0]
        mutants["causal limit - 1"] = mn.statement(inp, causal_shift=-1)[0]
    short = []
    for name, y in mutants.items():
        m = float(attn_rel_err(ref, y, sq).max()) / mn.TAU_NEEDLE
        print(f"  case {i} {name:55s} {m:9.1f} tau")
        if not m >= 3:
            short.append((name, m))
    assert not short, short


# ---- CPU 3: surface and fakes --------------------------------------------------------------------------------------------------
def test_surface():
    import hpc

    assert "attention_decode_mla_fp8" in hpc.__all__ and callable(hpc.attention_decode_mla_fp8)
    doc = hpc.attention_decode_mla_fp8.__doc__
    for word in ("656", "offset 0", "offset 512", "offset 528", "c[d] = bf16_rne( fp32(code[d]) * scale[d // 128] )",
                 "amax / 448", "1e-8", "bit-identical", "torch.uint8", "splits", "release_decode_workspaces", "hipGraph",
                 "H % 16 == 0", "mtp 0..3", "{16, 32, 64, 128}"):
        assert word in doc, word


def test_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        q = torch.empty(6, 32, DIM, dtype=torch.bfloat16, device="cuda")
        ckv = torch.empty(9, 64, 656, dtype=torch.uint8, device="cuda")
        bid = torch.empty(3, 4, dtype=torch.int32, device="cuda")
        lens = torch.empty(3, dtype=torch.int32, device="cuda")
        out, lse = torch.ops.hpc_mla.attention_decode_mla_fp8(q, ckv, bid, lens, 0.07, 1, False, None, None, True, 0)
        assert (out.shape, out.dtype, lse.shape, lse.dtype) == ((6, 32, DIM_V), torch.bfloat16, (6, 32), torch.float32)
        out, lse = torch.ops.hpc_mla.attention_decode_mla_fp8(q, ckv, bid, lens, 0.07, 1, False, None, None, False, 0)
        assert out.shape == (6, 32, DIM_V) and lse.numel() == 0
        y = hpc.attention_decode_mla_fp8(q, ckv, bid, lens, 0.07, mtp=1)
        assert isinstance(y, torch.Tensor) and y.shape == (6, 32, DIM_V) and y.dtype == torch.bfloat16 and y.device.type == "cuda"
        y, l = hpc.attention_decode_mla_fp8(q, ckv, bid, lens, 0.07, mtp=1, return_lse=True, splits=4)
        assert y.shape == (6, 32, DIM_V) and l.shape == (6, 32)
        o = torch.empty(6, 32, DIM_V, dtype=torch.bfloat16, device="cuda")
        ol = torch.empty(6, 32, dtype=torch.float32, device="cuda")
        assert hpc.attention_decode_mla_fp8(q, ckv, bid, lens, 0.07, mtp=1, output=o) is o
        y, l = hpc.attention_decode_mla_fp8(q, ckv, bid, lens, 0.07, mtp=1, output=o, output_lse=ol)
        assert y is o and l is ol
        y, l = hpc.attention_decode_mla_fp8(q, ckv, bid, lens, 0.07, mtp=1, output_lse=ol)
        assert y.shape == (6, 32, DIM_V) and l is ol


# ---- CPU 4: the C-ABI refuses on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


def plan(lib, B, sq, H, splits, cus):
    s, mx, ws = c_int(-7), c_int(-7), c_int64(-7)
    rc = lib.hpc_attention_decode_mla_plan(B, sq, H, splits, cus, ctypes.byref(s), ctypes.byref(mx), ctypes.byref(ws))
    return rc, s.value, mx.value, ws.value


def call(lib, *, out=4096, lse=4096, q=4096, ckv=4096, bid=4096, lens=4096, B=2, sq=1, H=16, P=64, max_blocks=4,
         block_stride=64 * 656, token_stride=656, scale=0.07, nki=0, splits=1, ws=None, ws_bytes=0):
    """hpc_attention_decode_mla_fp8_async (cache strides in bytes) with pointers that are never dereferenced on the host"""
    return lib.hpc_attention_decode_mla_fp8_async(c_void_p(out), c_void_p(lse), c_void_p(q), c_void_p(ckv),
                                                  ctypes.cast(c_void_p(bid), ctypes.POINTER(c_int)),
                                                  ctypes.cast(c_void_p(lens), ctypes.POINTER(c_int)), B, sq, H, P, max_blocks,
                                                  c_int64(block_stride), c_int64(token_stride), c_float(scale), nki, splits,
                                                  c_void_p(ws) if ws else None, c_int64(ws_bytes), None)


UNSUPPORTED, INVALID = -1, -2


@pytest.mark.parametrize("kwargs,code", [
    # the bf16 launcher's table, strides restated in bytes
    (dict(H=8), UNSUPPORTED), (dict(H=24), UNSUPPORTED), (dict(H=144), UNSUPPORTED), (dict(sq=5), UNSUPPORTED),
    (dict(P=48), UNSUPPORTED), (dict(token_stride=655), UNSUPPORTED), (dict(token_stride=660), UNSUPPORTED),
    (dict(token_stride=672 - 8), UNSUPPORTED), (dict(token_stride=640), UNSUPPORTED),
    (dict(block_stride=64 * 656 + 8), UNSUPPORTED), (dict(block_stride=64 * 656 + 4), UNSUPPORTED),
    (dict(ckv=4096 + 8), UNSUPPORTED), (dict(q=4096 + 2), UNSUPPORTED),
    (dict(out=4096 + 4), UNSUPPORTED), (dict(max_blocks=1 << 26), UNSUPPORTED),
    (dict(splits=MAX_SPLITS + 1), INVALID), (dict(splits=-1), INVALID), (dict(B=-1), INVALID), (dict(sq=0), INVALID),
    (dict(sq=-1), INVALID), (dict(H=-16), INVALID), (dict(max_blocks=-1), INVALID), (dict(block_stride=-64 * 656), INVALID),
    (dict(out=0), INVALID), (dict(q=0), INVALID), (dict(ckv=0), INVALID), (dict(bid=0), INVALID), (dict(lens=0), INVALID),
    (dict(splits=2, ws=None), INVALID), (dict(splits=2, ws=4096 + 4, ws_bytes=1 << 30), UNSUPPORTED),
    # the cache's rule (csrc/mla_cache.h), as the writer's and the gather's tables pin it: it holds for an empty batch too, and
    # a negative block stride is an invalid argument that wins over whatever is merely unsupported
    (dict(token_stride=-656), UNSUPPORTED), (dict(P=8), UNSUPPORTED), (dict(P=256), UNSUPPORTED), (dict(P=0), UNSUPPORTED),
    (dict(B=0, P=48), UNSUPPORTED), (dict(H=8, block_stride=-64 * 656), INVALID),
])
def test_cabi_refuses_on_the_host(lib, kwargs, code):
    assert call(lib, **kwargs) == code


def test_cabi_takes_valid_strides_up_to_the_device_call(lib):
    """token stride 672 and 704, a block stride with a gap: accepted (an empty batch returns 0 without a device call)"""
    for kw in (dict(), dict(token_stride=672, block_stride=64 * 672), dict(token_stride=704, block_stride=67 * 704)):
        assert call(lib, B=0, **kw) == 0
    rc, s, _, need = plan(lib, 2, 1, 16, 2, 256)
    assert (rc, s) == (0, 2) and need > 0
    assert call(lib, splits=2, ws=4096, ws_bytes=need - 1) == INVALID


def test_both_libraries_export_the_launcher():
    pkg = Path(__file__).resolve().parent.parent / "hpc-ops_amd" / "hpc"
    for name in ("libhpc_amd.so", "libhpc_amd_dev.so"):
        assert hasattr(ctypes.CDLL(str(pkg / name)), "hpc_attention_decode_mla_fp8_async"), name


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _lens(inp, nki):
    return (inp["lens_total"] if nki else inp["lens_before"]).cuda()


def _run8(inp, cache, splits=0, nki=False, **kw):
    """the FP8 op on the uint8 cache `cache` (a CUDA tensor)"""
    import hpc

    return hpc.attention_decode_mla_fp8(inp["q"].cuda(), cache, inp["block_ids"].cuda(), _lens(inp, nki), inp["scale"],
                                        mtp=inp["num_seq_q"] - 1, new_kv_included=nki, return_lse=True, splits=splits, **kw)


def _run16(inp, splits=0, nki=False):
    """the bf16 op on inp["ckv"]"""
    import hpc

    return hpc.attention_decode_mla_bf16(inp["q"].cuda(), inp["ckv"].cuda(), inp["block_ids"].cuda(), _lens(inp, nki),
                                         inp["scale"], mtp=inp["num_seq_q"] - 1, new_kv_included=nki, return_lse=True,
                                         splits=splits)


def _fill_scratch_with_nan():
    import hpc  # noqa: F401  (registers the ops)

    for ws in torch.ops.hpc_mla._workspaces():
        ws.fill_(0xFF)  # every float of it a NaN


def _quantised(orig, seed):
    """(inputs over the dequantised cache, the uint8 cache on the CPU) of needle inputs"""
    cache = f8.quantise(orig["ckv"], vary_seed=seed)
    return dict(orig, ckv=f8.dequantise(cache)), cache


def _check(inp, ref, rlse, out, lse, label, tau=mn.TAU_NEEDLE, bar=mn.LSE_BAR_NEEDLE):
    sq = inp["num_seq_q"]
    w_out, w_lse = float(attn_rel_err(ref, out.cpu(), sq).max()), mn.lse_err(rlse, lse)
    print(f"{label}: out worst {w_out:.5f} (tau {tau}), lse worst {w_lse:.3g} (bar {bar})")
    assert attn_close(ref, out.cpu(), tau, sq, label=label)
    assert w_lse <= bar, (label, w_lse, bar)


# (H, mtp, P): narrow / a partly filled row tile / causal, pages of 16 / four row tiles / mtp 3
_CONFIGS = [(16, 0, 64), (48, 0, 32), (64, 1, 16), (128, 1, 64), (32, 3, 128)]


@functools.lru_cache(maxsize=None)
def _needle_case(H, mtp, P, chunk):
    """one half of a configuration's requests (B = 8): inputs over the dequantised cache and the uint8 cache, computed once"""
    lens = (mn.edge_lens(P) + [5000])[8 * chunk: 8 * chunk + 8]
    return _quantised(mn.needle_inputs(lens, mtp + 1, P, H, seed=200 + chunk), VARY_SEED + 10 * chunk + H)


@functools.lru_cache(maxsize=None)
def _needle_statement(H, mtp, P, chunk):
    return mn.statement(_needle_case(H, mtp, P, chunk)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("H,mtp,P", _CONFIGS)
def test_equal_to_the_bf16_op_on_the_dequantised_cache_bit_for_bit(H, mtp, P):
    for chunk in (0, 1):
        inp, cache = _needle_case(H, mtp, P, chunk)
        cache = cache.cuda()
        for splits in (0, 1, 3, 8):
            out8, lse8 = _run8(inp, cache, splits)
            out16, lse16 = _run16(inp, splits)
            assert out8.dtype == torch.bfloat16 and lse8.dtype == torch.float32
            assert torch.equal(out8.view(torch.int16), out16.view(torch.int16)), (H, mtp, P, chunk, splits)
            assert torch.equal(lse8.view(torch.int32), lse16.view(torch.int32)), (H, mtp, P, chunk, splits)


@pytest.mark.gpu
@pytest.mark.parametrize("H,mtp,P", _CONFIGS)
def test_needle_parity_on_the_dequantised_cache(H, mtp, P):
    for chunk in (0, 1):
        inp, cache = _needle_case(H, mtp, P, chunk)
        ref, rlse = _needle_statement(H, mtp, P, chunk)
        out, lse = _run8(inp, cache.cuda())
        _check(inp, ref, rlse, out, lse, f"fp8 H {H} mtp {mtp} P {P} chunk {chunk}")
        if (H, mtp, P) == (64, 1, 16):  # the lengths given the other way
            out2, lse2 = _run8(inp, cache.cuda(), nki=True)
            assert torch.equal(out2, out) and torch.equal(lse2, lse)


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 2, 8])
def test_one_token_is_the_cached_row_bit_for_bit(splits):
    g = torch.Generator().manual_seed(splits)
    for H, sq, P in ((16, 1, 64), (64, 2, 16)):
        B = 3
        cache = f8.quantise(torch.randn(2 * B + 1, P, DIM, generator=g).bfloat16(), vary_seed=splits)
        bid = torch.randperm(2 * B + 1, generator=g)[:B].to(torch.int32).reshape(B, 1)
        cache[int(bid[1, 0]), 0, 512 + 4 * 2: 512 + 4 * 3] = 0  # request 1: group 2 of its token has scale 0
        q = torch.randn(B * sq, H, DIM, generator=g).bfloat16()
        # every request has its sq new tokens only: row 0 sees one token (with sq > 1 the later rows see more)
        inp = dict(q=q, block_ids=bid, lens_before=torch.zeros(B, dtype=torch.int32),
                   lens_total=torch.full((B,), sq, dtype=torch.int32), num_seq_q=sq, scale=mn.SCALE)
        _fill_scratch_with_nan()
        out, _ = _run8(inp, cache.cuda(), splits)
        want = f8.dequantise(cache)[bid[:, 0].long(), 0, :DIM_V]
        assert bool((want[1, 256:384] == 0).all()) and bool((want[1, :256] != 0).any())
        got = out.cpu().reshape(B, sq, H, DIM_V)[:, 0]
        assert torch.equal(got, want[:, None, :].expand(B, H, DIM_V)), (H, sq, P)


@pytest.mark.gpu
def test_strided_caches_are_bit_equal_to_the_contiguous_one():
    """token stride 704 bytes; a view into a larger pool with leading and trailing pages and extra slots per page; every gap
    byte 0xA5"""
    P, H, sq = 32, 48, 2
    inp, cache = _quantised(mn.needle_inputs([0, 31, 33, 700, 1500], sq, P, H, seed=21), VARY_SEED)
    pool = cache.shape[0]
    padded = torch.full((pool, P, 704), 0xA5, dtype=torch.uint8, device="cuda")
    big = torch.full((pool + 2, P + 3, 704), 0xA5, dtype=torch.uint8, device="cuda")
    views = {"padded": padded[:, :, :656], "pool": big[1:-1, 2: 2 + P, :656]}
    assert views["padded"].stride() == (P * 704, 704, 1) and views["pool"].stride() == ((P + 3) * 704, 704, 1)
    for v in views.values():
        assert not v.is_contiguous()
        v.copy_(cache.cuda())
    for splits in (1, 3):
        a, la = _run8(inp, cache.cuda(), splits)
        for name, v in views.items():
            b, lb = _run8(inp, v, splits)
            assert torch.equal(a, b) and torch.equal(la, lb), (name, splits)
    ref, rlse = mn.statement(inp)
    _check(inp, ref, rlse, b, lb, "fp8 strided")


@functools.lru_cache(maxsize=None)
def _forced_case():
    inp, cache = _quantised(mn.needle_inputs([5, 64, 65, 700, 5000], 1, 64, 16, seed=9), VARY_SEED + 1)
    return inp, cache, mn.statement(inp)


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 3, 64])
def test_forced_splits_over_nan_scratch(splits):
    """splits = 64 on 5 tokens leaves 63 empty pieces; the scratch holds NaN bytes before each call, so a read of an empty or
    unwritten piece shows"""
    inp, cache, (ref, rlse) = _forced_case()
    _run8(inp, cache.cuda(), MAX_SPLITS)  # the scratch exists at its largest
    _fill_scratch_with_nan()
    out, lse = _run8(inp, cache.cuda(), splits)
    _check(inp, ref, rlse, out, lse, f"fp8 forced splits {splits}")


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 4])
def test_twenty_calls_are_bit_identical(splits):
    inp, cache = _quantised(mn.needle_inputs([3, 700, 2100], 2, 64, 32, seed=4), VARY_SEED + 2)
    cache = cache.cuda()
    first = _run8(inp, cache, splits)
    for _ in range(19):
        _fill_scratch_with_nan()
        again = _run8(inp, cache, splits)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])


@pytest.mark.gpu
def test_graph_replays_after_lengths_pages_and_cache_changed_in_place():
    """capture with every output given; replay; change the lengths, the pages and the cache in place; replay: the new result"""
    import hpc

    H, sq, P = 16, 1, 64
    a = mn.needle_inputs([700, 64, 3000, 5], sq, P, H, seed=31)
    b = mn.needle_inputs([65, 2000, 1, 900], sq, P, H, seed=32)
    pool, cols = max(a["ckv"].shape[0], b["ckv"].shape[0]), max(a["block_ids"].shape[1], b["block_ids"].shape[1])

    def padded(orig, seed):  # the case's pool inside the graph's pool, the rest poison
        full = torch.full((pool, P, DIM), mn.POISON, dtype=torch.bfloat16)
        full[: orig["ckv"].shape[0]] = orig["ckv"]
        return _quantised(dict(orig, ckv=full), seed)

    cases = [padded(a, VARY_SEED + 3), padded(b, VARY_SEED + 4)]
    ckv = torch.zeros(pool, P, 656, dtype=torch.uint8, device="cuda")
    bid = torch.full((4, cols), -999999, dtype=torch.int32, device="cuda")
    q = torch.zeros(4 * sq, H, DIM, dtype=torch.bfloat16, device="cuda")
    lens = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(4 * sq, H, DIM_V, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(4 * sq, H, dtype=torch.float32, device="cuda")

    def load(case):
        inp, cache = case
        ckv.copy_(cache)
        bid.fill_(-999999)
        bid[:, : inp["block_ids"].shape[1]].copy_(inp["block_ids"])
        q.copy_(inp["q"])
        lens.copy_(inp["lens_before"])

    def step():
        return hpc.attention_decode_mla_fp8(q, ckv, bid, lens, mn.SCALE, output=out, output_lse=lse, splits=4)

    load(cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y, l = step()
        assert y is out and l is lse
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated()
        step()
        grown = torch.cuda.memory_allocated() - before
    ws_bytes = sum(w.numel() for w in torch.ops.hpc_mla._workspaces())
    assert grown <= ws_bytes, (grown, ws_bytes)  # nothing allocated in the capture beyond the cached scratch
    for case in (cases[0], cases[1], cases[0]):
        load(case)
        out.zero_()
        lse.zero_()
        graph.replay()
        torch.cuda.synchronize()
        ref, rlse = mn.statement(case[0])
        _check(case[0], ref, rlse, out, lse, "fp8 graph")
    del graph
    hpc.release_decode_workspaces()
    assert len(torch.ops.hpc_mla._workspaces()) == 0


GUARD, PATTERN = 1 << 20, 0xA5


@pytest.mark.gpu
def test_guard_bands_through_the_cabi(lib):
    """out, lse and a workspace of exactly the planned bytes, each between 1 MiB guard bands: the bands are intact afterwards"""
    H, mtp, splits = 48, 1, 5
    sq, P = mtp + 1, 64
    inp, cache = _quantised(mn.needle_inputs([5, 64, 700, 1500], sq, P, H, seed=17), VARY_SEED + 5)
    B, rows = 4, 4 * sq * H
    rc, s, _, ws_bytes = plan(lib, B, sq, H, splits, 0)
    assert (rc, s) == (0, splits) and ws_bytes > 0
    sizes = [rows * DIM_V * 2, rows * 4, ws_bytes]
    bufs = [torch.full((2 * GUARD + n,), PATTERN, dtype=torch.uint8, device="cuda") for n in sizes]
    bufs[2][GUARD: GUARD + ws_bytes] = 0xFF
    q, ckv, bid, lens = inp["q"].cuda(), cache.cuda(), inp["block_ids"].cuda(), inp["lens_before"].cuda()
    torch.cuda.synchronize()
    rc = call(lib, out=bufs[0].data_ptr() + GUARD, lse=bufs[1].data_ptr() + GUARD, q=q.data_ptr(), ckv=ckv.data_ptr(),
              bid=bid.data_ptr(), lens=lens.data_ptr(), B=B, sq=sq, H=H, P=P, max_blocks=bid.shape[1], block_stride=ckv.stride(0),
              token_stride=ckv.stride(1), scale=mn.SCALE, splits=splits, ws=bufs[2].data_ptr() + GUARD, ws_bytes=ws_bytes)
    torch.cuda.synchronize()
    assert rc == 0
    for buf, n in zip(bufs, sizes):
        assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n:] == PATTERN).all())
    out = bufs[0][GUARD: GUARD + sizes[0]].view(torch.bfloat16).reshape(B * sq, H, DIM_V)
    lse = bufs[1][GUARD: GUARD + sizes[1]].view(torch.float32).reshape(B * sq, H)
    ref, rlse = mn.statement(inp)
    _check(inp, ref, rlse, out, lse, "fp8 guards")


@pytest.mark.gpu
def test_empty_batch_and_refusals():
    import hpc

    q = torch.empty(0, 16, DIM, dtype=torch.bfloat16, device="cuda")
    ckv = torch.zeros(2, 64, 656, dtype=torch.uint8, device="cuda")
    ckv16 = torch.zeros(2, 64, DIM, dtype=torch.bfloat16, device="cuda")
    bid = torch.empty(0, 1, dtype=torch.int32, device="cuda")
    lens = torch.empty(0, dtype=torch.int32, device="cuda")
    out, lse = hpc.attention_decode_mla_fp8(q, ckv, bid, lens, mn.SCALE, return_lse=True)
    assert out.shape == (0, 16, DIM_V) and out.dtype == torch.bfloat16 and lse.shape == (0, 16)
    q1 = torch.zeros(1, 16, DIM, dtype=torch.bfloat16, device="cuda")
    one = (torch.zeros(1, 1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="ckv_cache dtype must be uint8"):
        hpc.attention_decode_mla_fp8(q1, ckv16, *one, mn.SCALE)
    with pytest.raises(RuntimeError, match="ckv_cache dtype must be bfloat16"):
        hpc.attention_decode_mla_bf16(q1, ckv, *one, mn.SCALE)
    with pytest.raises(RuntimeError, match="656"):
        hpc.attention_decode_mla_fp8(q1, ckv[:, :, :576], *one, mn.SCALE)
    with pytest.raises(RuntimeError, match="token stride"):
        hpc.attention_decode_mla_fp8(q1, torch.zeros(2, 64, 664, dtype=torch.uint8, device="cuda")[:, :, :656], *one, mn.SCALE)
    with pytest.raises(RuntimeError, match="splits"):
        hpc.attention_decode_mla_fp8(q1, ckv, *one, mn.SCALE, splits=MAX_SPLITS + 1)
    with pytest.raises(RuntimeError, match="num_head"):
        hpc.attention_decode_mla_fp8(q1[:, :8], ckv, *one, mn.SCALE)
    with pytest.raises(RuntimeError, match="block_size"):
        hpc.attention_decode_mla_fp8(q1, ckv[:, :48], *one, mn.SCALE)
