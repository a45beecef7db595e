"""hpc.mla_absorb_q / hpc.mla_unabsorb_o: the two per-head absorb matmuls of an MLA decode step, the second with the 128-block
e4m3 quantisation of the output projection's input.  Statements, mutants, bar and case builders: tests/mla_absorb_ref.py.

The bar is derived (products of bf16 are exact in fp32): |y - r| <= 2^-8 |r| + K 2^-23 A per element.  Exact-input cases and
everything about quant=True are compared bit for bit.

CPU: the statements' own properties, the bar against an fp32 restatement, `test_inputs_have_teeth` (the GPU cases' inputs tell
every mutant from the statement at several times the bar), surface, fakes, the exported and prototyped symbols, and every
host refusal through the C-ABI with never-dereferenced pointers, each with its own message.
GPU: exact inputs through the real views with guard bands, random inputs at the bar, quant=True against
tests/blockwise_quant_ref.py and through hpc.gemm_blockwise_fp8, the two writers of q_abs in both orders, repeatability,
hipGraph replay, rows 4.5 GiB apart (64-bit offsets), T == 0 and the refusals through the op.

Worst |y - r| / bar measured on the GPU (profiles/mla_absorb.txt): absorb_q 0.9590-0.9875, unabsorb_o 0.8562-0.9301 - the
half-ulp term of a correctly rounded result."""
import ctypes
from pathlib import Path

import pytest
import torch

import blockwise_quant_ref as bq
import mla_absorb_ref as ar
import mla_store_ref as ms

BF16 = torch.bfloat16
F8 = torch.float8_e4m3fn
ROOT = Path(__file__).resolve().parent.parent
TEETH = 4.0  # a mutant must miss by more than this many bars somewhere


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else (t.view(torch.uint8) if t.dtype == F8 else t)


# ------------------------------------------------------------------------------------------- the statements themselves
def test_unit_weight_gives_a_copy():
    c = ar.random_case(5, 3)
    eye_uk = torch.zeros(3, 128, 512, dtype=BF16)
    eye_uk[:, torch.arange(128), torch.arange(128)] = 1
    r, A = ar.absorb_q_statement(c.q, eye_uk)
    assert torch.equal(r[..., :128], c.q.double()) and not bool(r[..., 128:].any()) and torch.equal(A, r.abs())
    eye_uv = torch.zeros(3, 128, 512, dtype=BF16)
    eye_uv[:, torch.arange(128), 7 + torch.arange(128)] = 1
    r, A = ar.unabsorb_o_statement(c.o_lat, eye_uv)
    assert torch.equal(r, c.o_lat.double()[..., 7: 135]) and torch.equal(A, r.abs())


def test_scaling_one_heads_weight_moves_that_head_alone():
    c = ar.random_case(5, 3)
    for stmt, x, w in ((ar.absorb_q_statement, c.q, c.w_uk), (ar.unabsorb_o_statement, c.o_lat, c.w_uv)):
        r0, _ = stmt(x, w)
        w2 = w.clone()
        w2[1] *= 2
        r1, _ = stmt(x, w2)
        assert torch.equal(r1[:, 1], 2 * r0[:, 1]) and torch.equal(r1[:, 0], r0[:, 0]) and torch.equal(r1[:, 2], r0[:, 2])


def test_exact_inputs_are_exact_in_fp32_in_any_order():
    c = ar.exact_case(17, 3)
    for (r, A), x, w_nk in ((c.q_ref, c.q, c.w_uk.transpose(1, 2)), (c.o_ref, c.o_lat, c.w_uv)):
        assert float(A.max()) < 2 ** 20 and torch.equal(r, r.round())
        fwd = torch.einsum("thk,hnk->thn", x.float(), w_nk.float())
        K = x.shape[-1]
        perm = torch.randperm(K, generator=torch.Generator().manual_seed(3))
        acc = torch.zeros_like(fwd)
        for k in perm.tolist():  # one term at a time, in a scrambled order
            acc += x[..., k].float()[..., None] * w_nk[..., k].float()[None]
        assert torch.equal(fwd.double(), r) and torch.equal(acc.double(), r)
        assert torch.equal(_bits(ar.fp32_restatement(x, w_nk)), _bits(r.to(BF16)))


def test_the_fp32_restatement_stays_inside_the_bar():
    worst = {}
    for T, H in ((17, 16), (65, 16), (17, 48)):
        c = ar.random_case(T, H)
        worst["absorb_q", T, H] = ar.worst_ratio(ar.fp32_restatement(c.q, c.w_uk.transpose(1, 2)), *c.q_ref, 128)
        worst["unabsorb_o", T, H] = ar.worst_ratio(ar.fp32_restatement(c.o_lat, c.w_uv), *c.o_ref, 512)
    print("worst |y - r| / bar of the fp32 restatement:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def _misses(m, ref, K):
    """how many bars the mutant's result lies from the statement, at its worst element"""
    r, A = ref
    return float(((m - r).abs() / ar.bar(r, A, K).clamp_min(1e-300)).max())


def test_inputs_have_teeth():
    """every mutant is held to every GPU case in which the mutated quantity differs at all: a shifted head needs H > 1, the
    neighbour's row a second token behind a 16-token block (T > 16)"""
    for T, H in ar.SHAPES:
        c = ar.random_case(T, H)
        mutants = [("last 32 dropped", dict(drop_last=32))]
        if H > 1:
            mutants.append(("head h + 1's weight", dict(head_shift=1)))
        if T > ar.TOKEN_BLOCK:
            mutants.append(("a block's last row from its neighbour", dict(row_from_neighbour=True)))
        for name, kw in mutants:
            assert _misses(ar.absorb_q_statement(c.q, c.w_uk, **kw)[0], c.q_ref, 128) > TEETH, ("absorb_q", name, T, H)
            assert _misses(ar.unabsorb_o_statement(c.o_lat, c.w_uv, **kw)[0], c.o_ref, 512) > TEETH, ("unabsorb_o", name, T, H)
        assert _misses(ar.absorb_q_statement(c.q, c.w_uk, d_contiguous=True)[0], c.q_ref, 128) > TEETH, ("d contiguous", T, H)
        # quant=True is compared bit for bit: a mutant must change a code or a scale
        o = c.o_ref[0].to(BF16).view(T, H * 128)
        codes, scale = ar.quant_statement(o)
        qm = [("a scale over 64 columns", dict(cols=64))] + ([("the next head's scale", dict(head_shift=1))] if H > 1 else [])
        for name, kw in qm:
            mc, msc = ar.quant_statement(o, **kw)
            assert not torch.equal(msc, scale) and not torch.equal(_bits(mc), _bits(codes)), (name, T, H)
    # the exact cases tell the same mutants (bit for bit is at least as sharp), on the largest of them
    e = ar.exact_case(17, 48)
    assert not torch.equal(ar.absorb_q_statement(e.q, e.w_uk, head_shift=1)[0].to(BF16), e.q_ref[0].to(BF16))
    assert not torch.equal(ar.unabsorb_o_statement(e.o_lat, e.w_uv, drop_last=32)[0].to(BF16), e.o_ref[0].to(BF16))


# ----------------------------------------------------------------------------------------------- surface, fakes, symbols
def test_surface():
    import hpc

    for name in ("mla_absorb_q", "mla_unabsorb_o"):
        assert name in hpc.__all__ and callable(getattr(hpc, name)), name
    for word in ("w_kv_b.view(H, 256, 512)[:, :128]", "q[..., :128]", "q_abs[..., :512]", "hipGraph", "1 <= H <= 128",
                 "tests/mla_absorb_ref.py", "bit-identical"):
        assert word in hpc.mla_absorb_q.__doc__, word
    for word in ("w_kv_b.view(H, 256, 512)[:, 128:]", "amax_v |o| / 448", "1 / (scale + 1e-8)", "gemm_blockwise_fp8",
                 "blockwise_fp8_quant", "hipGraph", "tests/mla_absorb_ref.py"):
        assert word in hpc.mla_unabsorb_o.__doc__, word
    assert hasattr(torch.ops.hpc_mla, "absorb_q") and hasattr(torch.ops.hpc_mla, "unabsorb_o")


SYMBOLS = ("hpc_mla_absorb_q_async", "hpc_mla_unabsorb_o_async", "hpc_mla_absorb_q_refusal", "hpc_mla_unabsorb_o_refusal")


def test_symbols_are_exported_and_prototyped():
    header = (ROOT / "include" / "hpc_amd.h").read_text()
    for lib in ("libhpc_amd.so", "libhpc_amd_dev.so"):
        for fn in SYMBOLS:
            assert hasattr(ctypes.CDLL(str(ROOT / "hpc-ops_amd" / "hpc" / lib)), fn), (lib, fn)
    for fn in SYMBOLS:
        assert (("int " if fn.endswith("_async") else "const char* ") + fn + "(") in header, fn


def test_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        def T(*shape, dtype=BF16):
            return torch.empty(shape, dtype=dtype, device="cuda")

        w = T(16, 256, 512)
        q, q_abs = T(9, 16, 192), T(9, 16, 576)
        out = q_abs[..., :512]
        assert hpc.mla_absorb_q(q[..., :128], w[:, :128], output=out) is out
        y = hpc.mla_absorb_q(q[..., :128], w[:, :128])
        assert (y.shape, y.dtype, y.device.type) == ((9, 16, 512), BF16, "cuda") and y.is_contiguous()
        o_lat = T(9, 16, 512)
        y = hpc.mla_unabsorb_o(o_lat, w[:, 128:])
        assert (y.shape, y.dtype) == ((9, 2048), BF16) and y.is_contiguous()
        buf = T(9, 2112)[:, :2048]
        assert hpc.mla_unabsorb_o(o_lat, w[:, 128:], output=buf) is buf
        codes, scale = hpc.mla_unabsorb_o(o_lat, w[:, 128:], quant=True)
        assert (codes.shape, codes.dtype, scale.shape, scale.dtype) == ((9, 2048), F8, (9, 16), torch.float32)
        oc, osc = T(9, 2048, dtype=F8), T(9, 16, dtype=torch.float32)
        got = hpc.mla_unabsorb_o(o_lat, w[:, 128:], output=oc, quant=True, output_scale=osc)
        assert got[0] is oc and got[1] is osc
        with pytest.raises(RuntimeError, match="output_scale needs quant"):
            hpc.mla_unabsorb_o(o_lat, w[:, 128:], output_scale=osc)


# ------------------------------------------------------------------------------------------------- the C-ABI on the host
UNSUPPORTED, INVALID = -1, -2
A, B, W, S = 1 << 20, 1 << 24, 1 << 28, 1 << 30  # out, input, weight, scale: far apart, never dereferenced


def _call(unabsorb, **kw):
    """(code of the _async entry, message of the _refusal entry) for one call; every case here is refused, or has nothing to
    launch, before any device call"""
    from ctypes import c_int64, c_void_p

    from hpc import _C

    H = kw.get("H", 16)
    if unabsorb:
        a = dict(out=A, scale=0, x=B, w=W, T=40, H=H, x_rs=H * 512, x_hs=512, w_hs=256 * 512, w_rs=512, out_rs=H * 128, quant=0)
    else:
        a = dict(out=A, x=B, w=W, T=40, H=H, x_rs=H * 192, x_hs=192, w_hs=256 * 512, w_rs=512, out_rs=H * 576, out_hs=576)
    a.update(kw)
    vp = lambda v: c_void_p(v) if v else None  # noqa: E731
    L = c_int64
    if unabsorb:
        args = (vp(a["out"]), vp(a["scale"]), vp(a["x"]), vp(a["w"]), L(a["T"]), a["H"], L(a["x_rs"]), L(a["x_hs"]), L(a["w_hs"]), L(a["w_rs"]),
                L(a["out_rs"]), a["quant"])
        why, code = _C.lib.hpc_mla_unabsorb_o_refusal(*args), _C.lib.hpc_mla_unabsorb_o_async(*args, None)
    else:
        args = (vp(a["out"]), vp(a["x"]), vp(a["w"]), L(a["T"]), a["H"], L(a["x_rs"]), L(a["x_hs"]), L(a["w_hs"]), L(a["w_rs"]),
                L(a["out_rs"]), L(a["out_hs"]))
        why, code = _C.lib.hpc_mla_absorb_q_refusal(*args), _C.lib.hpc_mla_absorb_q_async(*args, None)
    return code, (None if why is None else why.decode())


# one case per rule: (arguments, code, words of its message)
_BOTH = [
    (dict(T=-1), INVALID, "num_tokens is negative"),
    (dict(H=0), UNSUPPORTED, "num_head must be 1 .. 128"), (dict(H=129), UNSUPPORTED, "num_head must be 1 .. 128"),
    (dict(x_rs=16 * 576 + 4), UNSUPPORTED, "an input stride is not a multiple of 8"),
    (dict(x_hs=516), UNSUPPORTED, "an input stride is not a multiple of 8"),
    (dict(w_rs=516), UNSUPPORTED, "a weight stride is not a multiple of 8"),
    (dict(w_hs=256 * 512 + 2), UNSUPPORTED, "a weight stride is not a multiple of 8"),
    (dict(x_hs=64), UNSUPPORTED, "an input stride is below the width of a head"),
    (dict(x_rs=64), UNSUPPORTED, "an input stride is below the width of a head"),
    (dict(w_rs=256), UNSUPPORTED, "a weight stride is below 512"), (dict(w_hs=128), UNSUPPORTED, "a weight stride is below 512"),
    (dict(x_rs=1 << 57), UNSUPPORTED, "spans more than 2^60 bytes"), (dict(w_hs=1 << 57), UNSUPPORTED, "spans more than 2^60 bytes"),
    (dict(T=1 << 40), UNSUPPORTED, "more workgroups than a grid holds"),
    (dict(out=0), INVALID, "a null pointer"), (dict(x=0), INVALID, "a null pointer"), (dict(w=0), INVALID, "a null pointer"),
    (dict(out=A + 8), UNSUPPORTED, "not 16-byte aligned"), (dict(x=B + 8), UNSUPPORTED, "not 16-byte aligned"),
    (dict(w=W + 2), UNSUPPORTED, "not 16-byte aligned"),
    (dict(out=B + 64), UNSUPPORTED, "the output overlaps an input"), (dict(out=W + 4096), UNSUPPORTED, "the output overlaps an input"),
    # accepted: nothing to launch, null pointers included; one head and one token carry any stride
    (dict(T=0), 0, None), (dict(T=0, out=0, x=0, w=0), 0, None),
]
_ABSORB = [
    (dict(out_rs=16 * 576 + 4), UNSUPPORTED, "an output stride is not a multiple of 8"),
    (dict(out_hs=580), UNSUPPORTED, "an output stride is not a multiple of 8"),
    (dict(out_hs=256), UNSUPPORTED, "the output strides let heads or rows overlap"),
    (dict(out_rs=15 * 576), UNSUPPORTED, "the output strides let heads or rows overlap"),
]
_UNABSORB = [
    (dict(scale=S), INVALID, "output_scale given without quant"),
    (dict(out_rs=16 * 128 + 4), UNSUPPORTED, "row stride must be a multiple of 8 and at least num_head * 128"),
    (dict(out_rs=15 * 128), UNSUPPORTED, "row stride must be a multiple of 8 and at least num_head * 128"),
    (dict(quant=1, scale=S, out_rs=16 * 128 + 64), UNSUPPORTED, "the quantised output must be contiguous"),
    (dict(quant=1, scale=0), INVALID, "a null pointer"),
    (dict(quant=1, scale=S + 2), UNSUPPORTED, "output_scale is not 4-byte aligned"),
    (dict(quant=1, scale=A + 256), UNSUPPORTED, "output_scale overlaps another tensor"),
    (dict(quant=1, scale=B + 256), UNSUPPORTED, "output_scale overlaps another tensor"),
    (dict(quant=1, scale=S, T=0), 0, None), (dict(out_rs=16 * 128 + 64, T=0), 0, None),
]


@pytest.mark.parametrize("unabsorb,kwargs,code,words",
                         [(u, kw, c, m) for u in (False, True) for kw, c, m in _BOTH + (_UNABSORB if u else _ABSORB)])
def test_cabi_refuses_on_the_host(unabsorb, kwargs, code, words):
    got, why = _call(unabsorb, **kwargs)
    assert got == code, (got, why)
    assert (why is None) if words is None else (why is not None and words in why), why


def test_every_rule_has_its_own_message():
    for unabsorb, extra in ((False, _ABSORB), (True, _UNABSORB)):
        by_words = {}
        for kw, code, words in _BOTH + extra:
            if words is not None:
                by_words.setdefault(words, set()).add(_call(unabsorb, **kw)[1])
        messages = [m for ms_ in by_words.values() for m in ms_]
        assert all(len(v) == 1 for v in by_words.values()) and len(set(messages)) == len(by_words), by_words


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD = 1 << 19  # int16 cells of a 1 MiB guard band
PATTERN = 0x5A5A


def _banded(cells):
    """an int16 buffer of `cells` cells between two 1 MiB guard bands, every byte of it the pattern; (whole, middle)"""
    whole = torch.full((2 * GUARD + cells,), PATTERN, dtype=torch.int16, device="cuda")
    return whole, whole[GUARD: GUARD + cells]


def _gpu_inputs(c):
    """the case's operands on the GPU as the real views: q[..., :128] of [T, H, 192] and o_lat[..., :512] of [T, H, 576] with
    NaN in the other columns, the weights as the two halves of one [H, 256, 512] tensor"""
    q192 = torch.full((c.T, c.H, 192), float("nan"), dtype=BF16, device="cuda")
    q192[..., :128] = c.q.cuda()
    o576 = torch.full((c.T, c.H, 576), float("nan"), dtype=BF16, device="cuda")
    o576[..., :512] = c.o_lat.cuda()
    w = c.w_kv_b.cuda()
    return q192[..., :128], o576[..., :512], w[:, :128], w[:, 128:]


def _absorb_into_q_abs(c, q, w_uk):
    """the op into [..., :512] of a banded [T, H, 576] buffer; returns the columns written after checking that every other
    cell of the allocation survived bit for bit"""
    import hpc

    whole, mid = _banded(c.T * c.H * 576)
    q_abs = mid.view(BF16).view(c.T, c.H, 576)
    out = q_abs[..., :512]
    assert hpc.mla_absorb_q(q, w_uk, output=out) is out
    torch.cuda.synchronize()
    got = whole.cpu()
    assert bool((got[:GUARD] == PATTERN).all()) and bool((got[GUARD + c.T * c.H * 576:] == PATTERN).all())
    inner = got[GUARD: GUARD + c.T * c.H * 576].view(c.T, c.H, 576)
    assert bool((inner[..., 512:] == PATTERN).all())
    return inner[..., :512].contiguous().view(BF16)


def _unabsorb_into_rows(c, o_lat, w_uv, pad=64):
    import hpc

    width = c.H * 128 + pad
    whole, mid = _banded(c.T * width)
    rows = mid.view(BF16).view(c.T, width)
    out = rows[:, : c.H * 128]
    assert hpc.mla_unabsorb_o(o_lat, w_uv, output=out) is out
    torch.cuda.synchronize()
    got = whole.cpu()
    assert bool((got[:GUARD] == PATTERN).all()) and bool((got[GUARD + c.T * width:] == PATTERN).all())
    inner = got[GUARD: GUARD + c.T * width].view(c.T, width)
    assert bool((inner[:, c.H * 128:] == PATTERN).all())
    return inner[:, : c.H * 128].contiguous().view(BF16)


@pytest.mark.gpu
@pytest.mark.parametrize("T,H", ar.SHAPES)
def test_exact_inputs_bit_for_bit(T, H):
    import hpc

    c = ar.exact_case(T, H)
    q, o_lat, w_uk, w_uv = _gpu_inputs(c)
    want_q, want_o = c.q_ref[0].to(BF16), c.o_ref[0].to(BF16).view(T, H * 128)
    # through the real views, every other byte unchanged
    assert torch.equal(_bits(_absorb_into_q_abs(c, q, w_uk)), _bits(want_q))
    assert torch.equal(_bits(_unabsorb_into_rows(c, o_lat, w_uv)), _bits(want_o))
    # contiguous operands, fresh outputs
    y = hpc.mla_absorb_q(c.q.cuda(), c.w_uk.contiguous().cuda())
    assert y.shape == (T, H, 512) and y.dtype == BF16 and y.is_contiguous() and torch.equal(_bits(y.cpu()), _bits(want_q))
    o = hpc.mla_unabsorb_o(c.o_lat.cuda(), c.w_uv.contiguous().cuda())
    assert o.shape == (T, H * 128) and o.dtype == BF16 and o.is_contiguous() and torch.equal(_bits(o.cpu()), _bits(want_o))


@pytest.mark.gpu
@pytest.mark.parametrize("T,H", ar.SHAPES)
def test_random_inputs_at_the_bar(T, H):
    c = ar.random_case(T, H)
    q, o_lat, w_uk, w_uv = _gpu_inputs(c)
    rq = ar.worst_ratio(_absorb_into_q_abs(c, q, w_uk), *c.q_ref, 128)
    ro = ar.worst_ratio(_unabsorb_into_rows(c, o_lat, w_uv).view(T, H, 128), *c.o_ref, 512)
    print(f"T={T} H={H}: worst |y - r| / bar: absorb_q {rq:.4f}, unabsorb_o {ro:.4f}")
    assert rq <= 1.0 and ro <= 1.0, (rq, ro)


@pytest.mark.gpu
@pytest.mark.parametrize("T,H", ar.SHAPES)
def test_quant_is_blockwise_quant_of_the_ops_own_bf16_output(T, H):
    import hpc

    c = ar.random_case(T, H)
    _, o_lat, _, w_uv = _gpu_inputs(c)
    o = hpc.mla_unabsorb_o(o_lat, w_uv)
    codes, scale = hpc.mla_unabsorb_o(o_lat, w_uv, quant=True)
    assert codes.shape == (T, H * 128) and codes.dtype == F8 and codes.is_contiguous()
    assert scale.shape == (T, H) and scale.dtype == torch.float32 and scale.is_contiguous()
    want_codes, want_scale = bq.quant(o.cpu())
    assert torch.equal(scale.cpu(), want_scale) and torch.equal(_bits(codes.cpu()), _bits(want_codes))
    # the bf16 values behind the codes are those of quant=False: given outputs, and the library's own quantiser on o
    oc, osc = torch.empty_like(codes), torch.empty_like(scale)
    got = hpc.mla_unabsorb_o(o_lat, w_uv, output=oc, quant=True, output_scale=osc)
    assert got[0] is oc and got[1] is osc
    lc, ls = hpc.blockwise_fp8_quant(o)
    assert torch.equal(_bits(oc.cpu()), _bits(lc.cpu())) and torch.equal(osc.cpu(), ls.cpu())
    # exact inputs: the same, and the quant=False output is the statement
    e = ar.exact_case(T, H)
    ec, es = hpc.mla_unabsorb_o(e.o_lat.cuda(), e.w_uv.contiguous().cuda(), quant=True)
    wc, ws = bq.quant(e.o_ref[0].to(BF16).view(T, H * 128))
    assert torch.equal(_bits(ec.cpu()), _bits(wc)) and torch.equal(es.cpu(), ws)


@pytest.mark.gpu
def test_quantised_pair_feeds_gemm_blockwise_fp8():
    import hpc

    T, H, N = 17, 16, 256
    c = ar.random_case(T, H)
    _, o_lat, _, w_uv = _gpu_inputs(c)
    g = torch.Generator().manual_seed(9)
    w_o = torch.randn(N, H * 128, generator=g).to(F8).cuda()
    w_o_scale = (torch.rand(N // 128, H, generator=g) * 0.01 + 0.001).cuda()
    x, xs = hpc.mla_unabsorb_o(o_lat, w_uv, quant=True)
    y = hpc.gemm_blockwise_fp8(x, xs, w_o, w_o_scale)
    x2, xs2 = hpc.blockwise_fp8_quant(hpc.mla_unabsorb_o(o_lat, w_uv))
    y2 = hpc.gemm_blockwise_fp8(x2, xs2, w_o, w_o_scale)
    assert y.shape == (T, N) and torch.equal(_bits(y.cpu()), _bits(y2.cpu())) and bool(y.float().abs().sum() > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("absorb_first", [True, False], ids=["absorb_then_rope", "rope_then_absorb"])
def test_two_writers_of_q_abs(absorb_first):
    """mla_absorb_q writes q_abs[..., :512], mla_rope_norm_store_kv (out_q_pe=) q_abs[..., 512:] of one buffer: in both call
    orders the buffer is the concatenation of the two separate results"""
    import hpc

    H, P = 16, 16
    s = ms.case("decode_mtp0_16", H, P)
    rows = s.rows
    g = torch.Generator().manual_seed(31)
    w_uk = (torch.randn(H, 128, 512, generator=g) * 0.05).to(BF16).cuda()
    q_src = s.q_src.cuda()  # the q_b output [rows, H, 192]
    store_args = (None, s.y.cuda()[:, ms.KV_A_AT: ms.KV_A_AT + ms.DIM], s.cos_sin.cuda(), s.w.cuda(), s.ns.cuda(), s.q_index.cuda(),
                  s.bid.cuda())
    ockv = torch.empty(rows, 576, dtype=BF16, device="cuda")
    lat = hpc.mla_absorb_q(q_src[..., :128], w_uk)
    pe = hpc.mla_rope_norm_store_kv(*store_args, q_pe=q_src[..., 128:], out_ckv=ockv)
    q_abs = torch.full((rows, H, 576), -777.0, dtype=BF16, device="cuda")
    steps = [lambda: hpc.mla_absorb_q(q_src[..., :128], w_uk, output=q_abs[..., :512]),
             lambda: hpc.mla_rope_norm_store_kv(*store_args, q_pe=q_src[..., 128:], out_q_pe=q_abs[..., 512:], out_ckv=ockv)]
    for step in (steps if absorb_first else steps[::-1]):
        step()
    assert torch.equal(_bits(q_abs.cpu()), _bits(torch.cat([lat, pe], -1).cpu()))


@pytest.mark.gpu
def test_two_calls_give_identical_bits():
    import hpc

    c = ar.random_case(130, 16)
    q, o_lat, w_uk, w_uv = _gpu_inputs(c)
    assert torch.equal(_bits(hpc.mla_absorb_q(q, w_uk)), _bits(hpc.mla_absorb_q(q, w_uk)))
    assert torch.equal(_bits(hpc.mla_unabsorb_o(o_lat, w_uv)), _bits(hpc.mla_unabsorb_o(o_lat, w_uv)))
    a, b = hpc.mla_unabsorb_o(o_lat, w_uv, quant=True), hpc.mla_unabsorb_o(o_lat, w_uv, quant=True)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_hipgraph_replay_after_the_inputs_changed():
    import hpc

    T, H = 17, 16
    c, d = ar.random_case(T, H), ar.random_case(T, H, seed=7)
    q, o_lat, w_uk, w_uv = _gpu_inputs(c)
    q_abs = torch.zeros(T, H, 576, dtype=BF16, device="cuda")
    o = torch.zeros(T, H * 128, dtype=BF16, device="cuda")
    codes, scale = torch.zeros(T, H * 128, device="cuda").to(F8), torch.zeros(T, H, device="cuda")

    def run():
        hpc.mla_absorb_q(q, w_uk, output=q_abs[..., :512])
        hpc.mla_unabsorb_o(o_lat, w_uv, output=o)
        hpc.mla_unabsorb_o(o_lat, w_uv, output=codes, quant=True, output_scale=scale)

    run()  # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    q.copy_(d.q.cuda())
    o_lat.copy_(d.o_lat.cuda())
    for t in (q_abs, o, scale):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want_q, want_o = hpc.mla_absorb_q(q, w_uk), hpc.mla_unabsorb_o(o_lat, w_uv)
    assert ar.worst_ratio(want_q.cpu(), *ar.absorb_q_statement(d.q, c.w_uk), 128) <= 1.0  # the new inputs, not the captured ones
    assert torch.equal(_bits(q_abs[..., :512].cpu()), _bits(want_q.cpu())) and not bool(q_abs[..., 512:].any())
    assert torch.equal(_bits(o.cpu()), _bits(want_o.cpu()))
    wc, ws = bq.quant(want_o.cpu())
    assert torch.equal(_bits(codes.cpu()), _bits(wc)) and torch.equal(scale.cpu(), ws)


@pytest.mark.gpu
def test_far_row_offsets_are_64_bit():
    """row 2 of every operand lies 4.5 GiB behind its base: a 32-bit row offset would read and write row 0's neighbourhood.
    Inputs in one pool, outputs in another (an output may not share a byte range with an input)."""
    import hpc

    T, H = 3, 2
    stride = 2 ** 30 + 2 ** 27  # elements: 2.25 GiB per row
    c = ar.exact_case(T, H)
    pool_in = torch.empty(2 * stride + 65536, dtype=BF16, device="cuda")
    pool_out = torch.empty(2 * stride + 65536, dtype=BF16, device="cuda")
    q = pool_in.as_strided((T, H, 128), (stride, 192, 1))
    o_lat = pool_in.as_strided((T, H, 512), (stride, 576, 1), 8192)
    q_abs = pool_out.as_strided((T, H, 512), (stride, 576, 1))
    o = pool_out.as_strided((T, H * 128), (stride, 1), 8192)
    q.copy_(c.q.cuda())
    o_lat.copy_(c.o_lat.cuda())
    q_abs.fill_(-777.0)
    o.fill_(-777.0)
    w = c.w_kv_b.cuda()
    hpc.mla_absorb_q(q, w[:, :128], output=q_abs)
    hpc.mla_unabsorb_o(o_lat, w[:, 128:], output=o)
    assert torch.equal(_bits(q_abs.cpu()), _bits(c.q_ref[0].to(BF16)))
    assert torch.equal(_bits(o.cpu()), _bits(c.o_ref[0].to(BF16).view(T, H * 128)))
    del pool_in, pool_out


@pytest.mark.gpu
def test_empty_calls_and_refusals_through_the_op():
    import hpc

    H = 16
    w = torch.zeros(H, 256, 512, dtype=BF16, device="cuda")
    q0, o0 = torch.zeros(0, H, 192, dtype=BF16, device="cuda")[..., :128], torch.zeros(0, H, 512, dtype=BF16, device="cuda")
    assert hpc.mla_absorb_q(q0, w[:, :128]).shape == (0, H, 512)
    assert hpc.mla_unabsorb_o(o0, w[:, 128:]).shape == (0, H * 128)
    codes, scale = hpc.mla_unabsorb_o(o0, w[:, 128:], quant=True)
    assert codes.shape == (0, H * 128) and codes.dtype == F8 and scale.shape == (0, H)
    q = torch.zeros(4, H, 192, dtype=BF16, device="cuda")
    o_lat = torch.zeros(4, H, 512, dtype=BF16, device="cuda")

    def refused(match, fn, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            fn(*a, **kw)

    refused("q_nope dtype", hpc.mla_absorb_q, q[..., :128].float(), w[:, :128])
    refused("w_uk must have shape", hpc.mla_absorb_q, q[..., :128], w[:8, :128])
    refused("q_nope must be", hpc.mla_absorb_q, q, w[:, :128])
    refused("contiguous last dim", hpc.mla_absorb_q, torch.zeros(4, H, 256, dtype=BF16, device="cuda")[..., ::2], w[:, :128])
    refused("not a multiple of 8", hpc.mla_absorb_q, torch.zeros(4, H, 132, dtype=BF16, device="cuda")[..., :128], w[:, :128])
    refused("not 16-byte aligned", hpc.mla_absorb_q, torch.zeros(4, H, 136, dtype=BF16, device="cuda")[..., 4:132], w[:, :128])
    refused("output overlaps an input", hpc.mla_absorb_q, q[..., :128], w[:, :128],
            output=w.view(-1)[: 4 * H * 512].view(4, H, 512))
    refused("num_head must be 1 .. 128", hpc.mla_unabsorb_o, torch.zeros(2, 129, 512, dtype=BF16, device="cuda"),
            torch.zeros(129, 128, 512, dtype=BF16, device="cuda"))
    refused("output_scale needs quant", hpc.mla_unabsorb_o, o_lat, w[:, 128:], output_scale=torch.zeros(4, H, device="cuda"))
    refused("output dtype", hpc.mla_unabsorb_o, o_lat, w[:, 128:], output=torch.zeros(4, H * 128, dtype=BF16, device="cuda"), quant=True)
    refused("quantised output must be contiguous", hpc.mla_unabsorb_o, o_lat, w[:, 128:], quant=True,
            output=torch.zeros(4, H * 128 + 64, device="cuda").to(F8)[:, : H * 128])
    refused("row stride must be a multiple of 8", hpc.mla_unabsorb_o, o_lat, w[:, 128:],
            output=torch.zeros(4, H * 128 + 4, dtype=BF16, device="cuda")[:, : H * 128])
