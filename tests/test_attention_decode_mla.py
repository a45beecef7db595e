"""hpc.attention_decode_mla_bf16: MLA decode attention over the paged latent KV cache.

CPU: properties of the float64 statement (tests/mla_ref.py); the bars of tests/mla_needles.py measured again - the split model
stays within them, they are at most 3 x its worst case, mutants are rejected at >= 3 tau; the public surface and fakes; host
refusals through the C-ABI with never-dereferenced pointers; the plan against the route's arithmetic restated here.
GPU: exact results, needle parity at the measured bars, forced split counts over NaN-filled scratch, a strided cache, repeatability,
a hipGraph replayed after the lengths changed, guard bands, the near-uniform generator."""
import ctypes
import functools
import math
from ctypes import c_float, c_int, c_int64, c_void_p

import pytest
import torch

import mla_needles as mn
import mla_ref
from utils import attn_close, attn_rel_err

DIM, DIM_V = mla_ref.DIM, mla_ref.DIM_V
MAX_SPLITS = 64


# ---- CPU 1: the statement ----------------------------------------------------------------------------------------------------
def _tiny(L, sq=1, H=16, P=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    nb = (L + P - 1) // P
    ckv = torch.randn(nb + 2, P, DIM, generator=g).to(torch.bfloat16)
    bid = torch.randperm(nb + 2, generator=g)[:nb].to(torch.int32).reshape(1, nb)
    q = torch.randn(sq, H, DIM, generator=g).to(torch.bfloat16)
    return q, ckv, bid


def test_statement_one_token_is_the_tokens_row():
    q, ckv, bid = _tiny(1)
    out, lse = mla_ref.mla_statement(q, ckv, bid, [1], 1, mn.SCALE)
    row = ckv[int(bid[0, 0]), 0]
    assert torch.equal(out.to(torch.bfloat16), row[:DIM_V].expand(1, 16, DIM_V))
    z = mn.SCALE * (q[0].double() @ row.double())
    assert torch.allclose(lse[0], z, rtol=0, atol=1e-12)


def test_statement_zero_q_is_the_mean():
    q, ckv, bid = _tiny(40)
    out, lse = mla_ref.mla_statement(torch.zeros_like(q), ckv, bid, [40], 1, mn.SCALE)
    rows = mla_ref.latent_rows(ckv, bid[0], 40).double()
    assert torch.allclose(out[0, 3], rows[:, :DIM_V].mean(0), rtol=0, atol=1e-12)
    assert torch.allclose(lse, torch.full_like(lse, math.log(40)), rtol=0, atol=1e-12)


def test_statement_is_causal_among_the_new_tokens():
    q, ckv, bid = _tiny(21, sq=3)
    out, _ = mla_ref.mla_statement(q, ckv, bid, [21], 3, mn.SCALE)
    for s in range(3):  # row s = a one-row request of 19 + s tokens
        alone, _ = mla_ref.mla_statement(q[s: s + 1], ckv, bid, [19 + s], 1, mn.SCALE)
        assert torch.allclose(out[s], alone[0], rtol=0, atol=1e-12)


# ---- CPU 2: the bars ---------------------------------------------------------------------------------------------------------
# (lens before the step, Sq, H, P): the cases the bars are calibrated on
_NEEDLE_CAL = [([0, 1, 63, 64, 1500, 4000], 2, 16, 64), ([5000, 700, 129], 1, 48, 32), ([9000], 1, 16, 64),
               ([0, 15, 16, 17, 65, 300], 4, 32, 16)]
_UNIFORM_CAL = [([4095, 1000, 130, 1], 2, 16, 64), ([9000, 3], 1, 32, 64)]


def _worst(inputs):
    tau, lse = 0.0, 0.0
    for inp in inputs:
        ref, rlse = mn.statement(inp)
        for R in mn.PIECE_LENS:
            out, l = mn.split_model(inp, R)
            tau = max(tau, float(attn_rel_err(ref, out, inp["num_seq_q"]).max()))
            lse = max(lse, mn.lse_err(rlse, l))
    return tau, lse


@pytest.mark.parametrize("generator", ["needle", "uniform"])
def test_split_model_within_bars(generator):
    """the split model passes both bars at every piece length 16 ... 4096, and each bar is at most 3 x the model's worst case"""
    if generator == "needle":
        inputs = [mn.needle_inputs(l, sq, P, H, seed=11) for l, sq, H, P in _NEEDLE_CAL]
        tau, bar = mn.TAU_NEEDLE, mn.LSE_BAR_NEEDLE
    else:
        inputs = [mn.uniform_inputs(l, sq, P, H) for l, sq, H, P in _UNIFORM_CAL]
        tau, bar = mn.TAU_UNIFORM, mn.LSE_BAR_UNIFORM
    w_tau, w_lse = _worst(inputs)
    print(f"\n{generator}: split model worst out {w_tau:.5f} (tau {tau} = {tau / w_tau:.2f} x), "
          f"worst lse {w_lse:.3g} (bar {bar} = {bar / w_lse:.2f} x) over piece lengths {mn.PIECE_LENS}")
    assert w_tau <= tau <= 3 * w_tau, (w_tau, tau)
    assert w_lse <= bar <= 3 * w_lse, (w_lse, bar)


def test_needle_bar_rejects_mutants():
    """each mutant of a plausible kernel bug, run through the statement (or the model's merge), is >= 3 tau off"""
    sq, P = 2, 64
    inp = mn.needle_inputs([0, 1, 63, 64, 1500, 4000], sq, P, 16, seed=5)
    ref, rlse = mn.statement(inp)
    mutants = {
        "RoPE columns ignored": mn.statement(inp, use_rope=False)[0],
        "V columns shifted by one": mn.statement(inp, v_shift=1)[0],
        "causal limit + 1": mn.statement(inp, causal_shift=1)[0],
        "causal limit - 1": mn.statement(inp, causal_shift=-1)[0],
        "last token of a page lost": mn.statement(inp, drop=lambda L: range(P - 1, L, P))[0],
        "first piece dropped from the merge": mn.split_model(inp, 512, drop_piece=0)[0],
        "last piece dropped from the merge": mn.split_model(inp, 512, drop_piece=-1)[0],
        "softmax scale 1/sqrt(576)": mn.statement(inp, scale=1 / math.sqrt(DIM))[0],
        "zeros": torch.zeros_like(ref),
    }
    short = []
    for name, y in mutants.items():
        m = float(attn_rel_err(ref, y, sq).max()) / mn.TAU_NEEDLE
        print(f"  {name:40s} {m:9.1f} tau")
        if not m >= 3:
            short.append((name, m))
    assert not short, short
    assert attn_close(ref, mn.split_model(inp, 512)[0], mn.TAU_NEEDLE, sq)


def test_uniform_bar_rejects_zeros():
    inp = mn.uniform_inputs([4095, 1000, 130], 2, 64, 16)
    ref, _ = mn.statement(inp)
    assert float(ref[:2].float().abs().max()) < 0.1  # the 4096-token request: an absolute 0.1 would accept zeros
    assert not attn_close(ref, torch.zeros_like(ref), mn.TAU_UNIFORM, 2)
    assert float(attn_rel_err(ref, (ref.float() * 1.25).to(ref.dtype), 2).max()) > 3 * mn.TAU_UNIFORM


# ---- CPU 3: surface and fakes ------------------------------------------------------------------------------------------------
def test_surface():
    import hpc

    assert "attention_decode_mla_bf16" in hpc.__all__ and callable(hpc.attention_decode_mla_bf16)
    doc = hpc.attention_decode_mla_bf16.__doc__
    for word in ("softmax_scale", "576", "512", "splits", "bit-identical", "piece order", "num_seq_kvcache", "hipGraph",
                 "H % 16 == 0", "mtp 0..3", "{16, 32, 64, 128}", "lse", "natural log", "release_decode_workspaces"):
        assert word in doc, word


def test_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        q = torch.empty(6, 32, DIM, dtype=torch.bfloat16, device="cuda")
        ckv = torch.empty(9, 64, DIM, dtype=torch.bfloat16, device="cuda")
        bid = torch.empty(3, 4, dtype=torch.int32, device="cuda")
        lens = torch.empty(3, dtype=torch.int32, device="cuda")
        out, lse = torch.ops.hpc_mla.attention_decode_mla_bf16(q, ckv, bid, lens, 0.07, 1, False, None, None, True, 0)
        assert (out.shape, out.dtype, lse.shape, lse.dtype) == ((6, 32, DIM_V), torch.bfloat16, (6, 32), torch.float32)
        out, lse = torch.ops.hpc_mla.attention_decode_mla_bf16(q, ckv, bid, lens, 0.07, 1, False, None, None, False, 0)
        assert out.shape == (6, 32, DIM_V) and lse.numel() == 0
        y = hpc.attention_decode_mla_bf16(q, ckv, bid, lens, 0.07, mtp=1)
        assert isinstance(y, torch.Tensor) and y.shape == (6, 32, DIM_V) and y.device.type == "cuda"
        y, l = hpc.attention_decode_mla_bf16(q, ckv, bid, lens, 0.07, mtp=1, return_lse=True, splits=4)
        assert y.shape == (6, 32, DIM_V) and l.shape == (6, 32)
        o = torch.empty(6, 32, DIM_V, dtype=torch.bfloat16, device="cuda")
        ol = torch.empty(6, 32, dtype=torch.float32, device="cuda")
        assert hpc.attention_decode_mla_bf16(q, ckv, bid, lens, 0.07, mtp=1, output=o) is o
        y, l = hpc.attention_decode_mla_bf16(q, ckv, bid, lens, 0.07, mtp=1, output=o, output_lse=ol)
        assert y is o and l is ol
        y, l = hpc.attention_decode_mla_bf16(q, ckv, bid, lens, 0.07, mtp=1, output_lse=ol)
        assert y.shape == (6, 32, DIM_V) and l is ol


# ---- CPU 4: the C-ABI refuses on the host -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


def plan(lib, B, sq, H, splits, cus):
    s, mx, ws = c_int(-7), c_int(-7), c_int64(-7)
    rc = lib.hpc_attention_decode_mla_plan(B, sq, H, splits, cus, ctypes.byref(s), ctypes.byref(mx), ctypes.byref(ws))
    return rc, s.value, mx.value, ws.value


def call(lib, *, out=4096, lse=4096, q=4096, ckv=4096, bid=4096, lens=4096, B=2, sq=1, H=16, P=64, max_blocks=4,
         block_stride=64 * 576, token_stride=576, scale=0.07, nki=0, splits=1, ws=None, ws_bytes=0):
    """hpc_attention_decode_mla_bf16_async with pointers that are never dereferenced on the host"""
    return lib.hpc_attention_decode_mla_bf16_async(c_void_p(out), c_void_p(lse), c_void_p(q), c_void_p(ckv),
                                                   ctypes.cast(c_void_p(bid), ctypes.POINTER(c_int)),
                                                   ctypes.cast(c_void_p(lens), ctypes.POINTER(c_int)), B, sq, H, P, max_blocks,
                                                   c_int64(block_stride), c_int64(token_stride), c_float(scale), nki, splits,
                                                   c_void_p(ws) if ws else None, c_int64(ws_bytes), None)


UNSUPPORTED, INVALID = -1, -2


@pytest.mark.parametrize("kwargs,code", [
    (dict(H=8), UNSUPPORTED), (dict(H=24), UNSUPPORTED), (dict(H=144), UNSUPPORTED), (dict(sq=5), UNSUPPORTED),
    (dict(P=48), UNSUPPORTED), (dict(token_stride=575), UNSUPPORTED), (dict(token_stride=580), UNSUPPORTED),
    (dict(block_stride=64 * 576 + 4), UNSUPPORTED), (dict(ckv=4096 + 8), UNSUPPORTED), (dict(q=4096 + 2), UNSUPPORTED),
    (dict(out=4096 + 4), UNSUPPORTED), (dict(max_blocks=1 << 26), UNSUPPORTED),
    (dict(splits=MAX_SPLITS + 1), INVALID), (dict(splits=-1), INVALID), (dict(B=-1), INVALID), (dict(sq=0), INVALID),
    (dict(sq=-1), INVALID), (dict(H=-16), INVALID), (dict(max_blocks=-1), INVALID), (dict(out=0), INVALID),
    (dict(q=0), INVALID), (dict(ckv=0), INVALID), (dict(bid=0), INVALID), (dict(lens=0), INVALID),
    (dict(splits=2, ws=None), INVALID), (dict(splits=2, ws=4096 + 4, ws_bytes=1 << 30), UNSUPPORTED),
    # the cache's rule (csrc/mla_cache.h), as the writer's and the gather's tables pin it: it holds for an empty batch too, and
    # a negative block stride is an invalid argument that wins over whatever is merely unsupported
    (dict(token_stride=-576), UNSUPPORTED), (dict(P=8), UNSUPPORTED), (dict(P=256), UNSUPPORTED), (dict(P=0), UNSUPPORTED),
    (dict(B=0, P=48), UNSUPPORTED), (dict(H=8, block_stride=-64 * 576), INVALID), (dict(block_stride=-64 * 576), INVALID),
])
def test_cabi_refuses_on_the_host(lib, kwargs, code):
    assert call(lib, **kwargs) == code


def test_cabi_refuses_a_small_workspace_and_takes_an_empty_batch(lib):
    rc, s, _, need = plan(lib, 2, 1, 16, 2, 256)
    assert (rc, s) == (0, 2) and need > 0
    assert call(lib, splits=2, ws=4096, ws_bytes=need - 1) == INVALID
    assert call(lib, B=0) == 0  # nothing to launch: no device call either
    assert plan(lib, 0, 1, 16, 0, 256)[0] == 0


def _route(B, sq, H, splits_wanted, cus):
    """the arithmetic of mla_route() (csrc/attention_decode_mla_route.h) in its dense form, restated"""
    rows = sq * H
    tiles = -(-rows // 64)
    W = B * tiles
    if B == 0:  # nothing to launch: one piece, no scratch, whatever was asked for
        s = 1
    elif splits_wanted:
        s = splits_wanted
    else:
        s = 1 if W >= cus else min(MAX_SPLITS, -(-2 * cus // W))
    ws = 0 if s == 1 else s * B * rows * (DIM_V + 2) * 4
    return s, ws


@pytest.mark.parametrize("B,sq,H,cus", [(64, 1, 16, 256), (64, 1, 128, 256), (8, 2, 128, 256), (1, 1, 16, 256), (3, 4, 48, 304),
                                        (256, 1, 16, 256), (255, 1, 64, 256), (7, 3, 32, 80), (130, 2, 128, 256),
                                        # W one below, at and one above the CU count (one row tile per request; W = 256 on 256 CUs is in the line above)
                                        (255, 1, 16, 256), (257, 1, 16, 256), (79, 1, 48, 80), (80, 1, 48, 80), (81, 1, 48, 80),
                                        (303, 2, 32, 304), (304, 2, 32, 304), (305, 2, 32, 304),
                                        # two row tiles per request: the nearest W either side of the CU count, and at it
                                        (151, 2, 64, 304), (152, 2, 64, 304), (153, 2, 64, 304),
                                        # 16 heads: one 16-row block at mtp 0 (the narrow form), two at mtp 1 (not narrow)
                                        (5, 1, 16, 256), (5, 2, 16, 256),
                                        # an empty batch
                                        (0, 1, 16, 256), (0, 3, 128, 80)])
def test_plan_is_the_route(lib, B, sq, H, cus):
    for wanted in (0, 1, 2, 3, 8, 64):
        rc, s, mx, ws = plan(lib, B, sq, H, wanted, cus)
        assert rc == 0 and mx == MAX_SPLITS
        assert (s, ws) == _route(B, sq, H, wanted, cus), (wanted, s, ws)
        assert (ws == 0) == (s == 1)
    assert plan(lib, B, sq, H, 65, cus)[0] == INVALID
    assert plan(lib, B, 5, H, 0, cus)[0] == UNSUPPORTED and plan(lib, B, sq, 8, 0, cus)[0] == UNSUPPORTED


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _run(inp, splits=0, nki=False, return_lse=True, ckv=None, **kw):
    import hpc

    lens = (inp["lens_total"] if nki else inp["lens_before"]).cuda()
    ckv = inp["ckv"].cuda() if ckv is None else ckv
    return hpc.attention_decode_mla_bf16(inp["q"].cuda(), ckv, inp["block_ids"].cuda(), lens, inp["scale"],
                                         mtp=inp["num_seq_q"] - 1, new_kv_included=nki, return_lse=return_lse, splits=splits,
                                         **kw)


def _fill_scratch_with_nan():
    import hpc  # noqa: F401  (registers the ops)

    for ws in torch.ops.hpc_mla._workspaces():
        ws.fill_(0xFF)  # every float of it a NaN


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 2, 3, 8])
def test_one_token_is_the_cached_row_bit_for_bit(splits):
    g = torch.Generator().manual_seed(splits)
    for H, sq, P in ((16, 1, 64), (48, 1, 32), (64, 2, 16)):
        B = 3
        ckv = torch.randn(2 * B + 1, P, DIM, generator=g).to(torch.bfloat16)
        bid = torch.randperm(2 * B + 1, generator=g)[:B].to(torch.int32).reshape(B, 1)
        q = torch.randn(B * sq, H, DIM, generator=g).to(torch.bfloat16)
        inp = dict(q=q, ckv=ckv, block_ids=bid, lens_before=torch.full((B,), 1 - sq, dtype=torch.int32),
                   lens_total=torch.ones(B, dtype=torch.int32), num_seq_q=sq, scale=mn.SCALE)
        if sq > 1:  # rows s >= 1 see the new tokens too: only row 0 sees one token; give every request sq tokens
            inp["lens_before"] = torch.zeros(B, dtype=torch.int32)
        _fill_scratch_with_nan()
        out, _ = _run(inp, splits)
        want = ckv[bid[:, 0].long(), 0, :DIM_V]  # token 0 of each request
        got = out.cpu().reshape(B, sq, H, DIM_V)[:, 0]
        assert torch.equal(got, want[:, None, :].expand(B, H, DIM_V)), (H, sq, P)


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 2, 3, 8])
def test_zero_q_is_the_exact_mean(splits):
    """small-integer latents, a length that is a power of two: every partial sum is an integer below 2^24 and the division
    exact, so the mean is exact in fp32 whatever the split and the output is its one rounding to bf16"""
    g = torch.Generator().manual_seed(7)
    P, H = 64, 16
    lens = [64, 128, 512, 4096]
    nb = [L // P for L in lens]
    pool = sum(nb) + 2
    ckv = (torch.randint(-4, 5, (pool, P, DIM), generator=g) * 32).to(torch.bfloat16)
    perm = torch.randperm(pool, generator=g).to(torch.int32)
    bid = torch.full((len(lens), max(nb)), -999999, dtype=torch.int32)
    o = 0
    for i, n in enumerate(nb):
        bid[i, :n] = perm[o: o + n]
        o += n
    for H in (16, 64):
        inp = dict(q=torch.zeros(len(lens), H, DIM, dtype=torch.bfloat16), ckv=ckv, block_ids=bid,
                   lens_before=torch.tensor(lens, dtype=torch.int32) - 1, lens_total=torch.tensor(lens, dtype=torch.int32),
                   num_seq_q=1, scale=mn.SCALE)
        _fill_scratch_with_nan()
        out, lse = _run(inp, splits)
        for b, L in enumerate(lens):
            mean = mla_ref.latent_rows(ckv, bid[b], L)[:, :DIM_V].double().mean(0)
            assert torch.equal(out[b].cpu(), mean.to(torch.bfloat16)[None, :].expand(H, DIM_V)), (H, L)  # one rounding
        assert torch.allclose(lse.cpu(), torch.tensor(lens).float().log()[:, None].expand(len(lens), H), rtol=0, atol=2e-6)


# (H, mtp, P): the narrow path / a partly filled tile / two tiles, causal / one full tile pair / four tiles / mtp 3
_CONFIGS = [(16, 0, 64), (48, 0, 32), (64, 1, 16), (128, 0, 64), (128, 1, 64), (32, 3, 128)]


@functools.lru_cache(maxsize=None)
def _needle_case(H, mtp, P, chunk):
    """inputs and the statement's result of one half of a configuration's requests (B = 8), computed once"""
    lens = (mn.edge_lens(P) + [20000])[8 * chunk: 8 * chunk + 8]
    inp = mn.needle_inputs(lens, mtp + 1, P, H, seed=100 + chunk)
    return inp, mn.statement(inp)


def _check(inp, ref, rlse, out, lse, label, tau=mn.TAU_NEEDLE, bar=mn.LSE_BAR_NEEDLE):
    sq = inp["num_seq_q"]
    w_out, w_lse = float(attn_rel_err(ref, out.cpu(), sq).max()), mn.lse_err(rlse, lse)
    print(f"{label}: out worst {w_out:.5f} (tau {tau}), lse worst {w_lse:.3g} (bar {bar})")
    assert attn_close(ref, out.cpu(), tau, sq, label=label)
    assert w_lse <= bar, (label, w_lse, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("H,mtp,P", _CONFIGS)
def test_needle_parity(H, mtp, P):
    for chunk in (0, 1):
        inp, (ref, rlse) = _needle_case(H, mtp, P, chunk)
        out, lse = _run(inp)
        _check(inp, ref, rlse, out, lse, f"H {H} mtp {mtp} P {P} chunk {chunk}")
        if (H, mtp) == (64, 1):  # the lengths given the other way
            out2, lse2 = _run(inp, nki=True)
            assert torch.equal(out2, out) and torch.equal(lse2, lse)


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("H,mtp,P", [(16, 0, 64), (64, 1, 16)])
def test_forced_splits_over_nan_scratch(H, mtp, P, splits):
    """splits = 64 on 5 tokens leaves 63 empty pieces; the scratch holds NaN bytes before each call, so a read of an empty or
    unwritten piece shows"""
    inp = mn.needle_inputs([5, 64, 65, 700, 5000], mtp + 1, P, H, seed=9)
    ref, rlse = _forced_ref(H, mtp, P)
    _run(inp, MAX_SPLITS)  # the scratch exists at its largest
    _fill_scratch_with_nan()
    out, lse = _run(inp, splits)
    _check(inp, ref, rlse, out, lse, f"H {H} mtp {mtp} splits {splits}")


@functools.lru_cache(maxsize=None)
def _forced_ref(H, mtp, P):
    return mn.statement(mn.needle_inputs([5, 64, 65, 700, 5000], mtp + 1, P, H, seed=9))


@pytest.mark.gpu
def test_strided_cache_is_bit_equal_to_the_contiguous_one():
    """token stride 640 elements and a block stride with a gap, the gaps poisoned: the same pool as a contiguous one"""
    P, H, sq = 32, 48, 2
    inp = mn.needle_inputs([0, 31, 33, 700, 1500], sq, P, H, seed=21)
    pool = inp["ckv"].shape[0]
    big = torch.full((pool + 1, P + 3, 640), mn.POISON, dtype=torch.bfloat16, device="cuda")
    view = big[1:, 2: 2 + P, :DIM]
    assert view.stride() == ((P + 3) * 640, 640, 1) and not view.is_contiguous()
    view.copy_(inp["ckv"].cuda())
    for splits in (1, 3):
        a, la = _run(inp, splits)
        b, lb = _run(inp, splits, ckv=view)
        assert torch.equal(a, b) and torch.equal(la, lb)
    ref, rlse = mn.statement(inp)
    _check(inp, ref, rlse, b, lb, "strided")


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 4])
def test_twenty_calls_are_bit_identical(splits):
    inp = mn.needle_inputs([3, 700, 2100], 2, 64, 64, seed=4)
    first = _run(inp, splits)
    for _ in range(19):
        _fill_scratch_with_nan()
        again = _run(inp, splits)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])


@pytest.mark.gpu
def test_graph_replays_with_new_lengths():
    """capture with every output given; replay; change the lengths and the pages in place; replay: the new lengths' result"""
    import hpc

    H, sq, P = 16, 1, 64
    a = mn.needle_inputs([700, 64, 3000, 5], sq, P, H, seed=31)
    b = mn.needle_inputs([65, 2000, 1, 900], sq, P, H, seed=32)
    pool, cols = max(a["ckv"].shape[0], b["ckv"].shape[0]), max(a["block_ids"].shape[1], b["block_ids"].shape[1])
    ckv = torch.zeros(pool, P, DIM, dtype=torch.bfloat16, device="cuda")
    bid = torch.full((4, cols), -999999, dtype=torch.int32, device="cuda")
    q = torch.zeros(4 * sq, H, DIM, dtype=torch.bfloat16, device="cuda")
    lens = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(4 * sq, H, DIM_V, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(4 * sq, H, dtype=torch.float32, device="cuda")

    def load(inp):
        ckv.fill_(mn.POISON)
        ckv[: inp["ckv"].shape[0]].copy_(inp["ckv"])
        bid.fill_(-999999)
        bid[:, : inp["block_ids"].shape[1]].copy_(inp["block_ids"])
        q.copy_(inp["q"])
        lens.copy_(inp["lens_before"])

    def step():
        return hpc.attention_decode_mla_bf16(q, ckv, bid, lens, mn.SCALE, output=out, output_lse=lse, splits=4)

    load(a)
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
    for inp in (a, b, a):
        load(inp)
        out.zero_()
        lse.zero_()
        graph.replay()
        torch.cuda.synchronize()
        ref, rlse = mn.statement(inp)
        _check(inp, ref, rlse, out, lse, "graph")
    del graph
    hpc.release_decode_workspaces()
    assert len(torch.ops.hpc_mla._workspaces()) == 0


GUARD, PATTERN = 1 << 20, 0xA5


@pytest.mark.gpu
@pytest.mark.parametrize("H,mtp,splits", [(16, 0, 3), (48, 1, 5), (128, 0, 1)])
def test_guard_bands_through_the_cabi(lib, H, mtp, splits):
    """out, lse and a workspace of exactly the planned bytes, each between 1 MiB guard bands: the bands are intact afterwards"""
    sq, P = mtp + 1, 64
    inp = mn.needle_inputs([5, 64, 700, 1500], sq, P, H, seed=17)
    B, rows = 4, 4 * sq * H
    rc, s, _, ws_bytes = plan(lib, B, sq, H, splits, 0)
    assert (rc, s) == (0, splits)
    sizes = [rows * DIM_V * 2, rows * 4, ws_bytes]
    bufs = [torch.full((2 * GUARD + n,), PATTERN, dtype=torch.uint8, device="cuda") for n in sizes]
    if ws_bytes:
        bufs[2][GUARD: GUARD + ws_bytes] = 0xFF
    q, ckv, bid, lens = inp["q"].cuda(), inp["ckv"].cuda(), inp["block_ids"].cuda(), inp["lens_before"].cuda()
    torch.cuda.synchronize()
    rc = call(lib, out=bufs[0].data_ptr() + GUARD, lse=bufs[1].data_ptr() + GUARD, q=q.data_ptr(), ckv=ckv.data_ptr(),
              bid=bid.data_ptr(), lens=lens.data_ptr(), B=B, sq=sq, H=H, P=P, max_blocks=bid.shape[1], block_stride=ckv.stride(0),
              token_stride=ckv.stride(1), scale=mn.SCALE, splits=splits, ws=bufs[2].data_ptr() + GUARD if ws_bytes else None,
              ws_bytes=ws_bytes)
    torch.cuda.synchronize()
    assert rc == 0
    for buf, n in zip(bufs, sizes):
        assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n:] == PATTERN).all())
    out = bufs[0][GUARD: GUARD + sizes[0]].view(torch.bfloat16).reshape(B * sq, H, DIM_V)
    lse = bufs[1][GUARD: GUARD + sizes[1]].view(torch.float32).reshape(B * sq, H)
    ref, rlse = mn.statement(inp)
    _check(inp, ref, rlse, out, lse, f"guards H {H}")


@pytest.mark.gpu
def test_uniform_generator_at_its_own_bar():
    inp = mn.uniform_inputs([4095, 1000, 130, 1, 64], 2, 64, 32)
    ref, rlse = mn.statement(inp)
    assert not attn_close(ref, torch.zeros_like(ref), mn.TAU_UNIFORM, 2)  # an all-zero answer is rejected
    for splits in (0, 1, 5):
        out, lse = _run(inp, splits)
        _check(inp, ref, rlse, out, lse, f"uniform splits {splits}", mn.TAU_UNIFORM, mn.LSE_BAR_UNIFORM)


@pytest.mark.gpu
def test_empty_batch_and_refusals():
    import hpc

    q = torch.empty(0, 16, DIM, dtype=torch.bfloat16, device="cuda")
    ckv = torch.zeros(2, 64, DIM, dtype=torch.bfloat16, device="cuda")
    bid = torch.empty(0, 1, dtype=torch.int32, device="cuda")
    lens = torch.empty(0, dtype=torch.int32, device="cuda")
    out, lse = hpc.attention_decode_mla_bf16(q, ckv, bid, lens, mn.SCALE, return_lse=True)
    assert out.shape == (0, 16, DIM_V) and lse.shape == (0, 16)
    q1 = torch.zeros(1, 16, DIM, dtype=torch.bfloat16, device="cuda")
    one = (torch.zeros(1, 1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="splits"):
        hpc.attention_decode_mla_bf16(q1, ckv, *one, mn.SCALE, splits=MAX_SPLITS + 1)
    with pytest.raises(RuntimeError, match="num_head"):
        hpc.attention_decode_mla_bf16(q1[:, :8], ckv, *one, mn.SCALE)
    with pytest.raises(RuntimeError, match="block_size"):
        hpc.attention_decode_mla_bf16(q1, ckv[:, :48], *one, mn.SCALE)
