"""hpc.mla_indexer_prep_fp8: the front end of the DSA lightning indexer (key LayerNorm + RoPE + Hadamard rotation + FP8 quant +
store; queries RoPE + rotation + quant + the fold of the head weights) in one launch.

CPU: the float64 statement (tests/mla_indexer_prep_ref.py) against a brute-force loop, H.H = 128 I, the rotation keeps q.k, the
pow2 rule on its edge values; the public surface and fakes; every host refusal through the C-ABI with never-dereferenced
pointers; the bar of check_outputs() accepts an fp32 model of the kernel's arithmetic and rejects eleven mutants by wide factors.
GPU: exact inputs bit for bit; fused equals parts bit for bit with every other byte untouched; random inputs on the bar; guards;
graphs and repeatability; end to end with planted needles into hpc.mla_indexer_topk_fp8."""
import ctypes
from ctypes import c_float, c_int, c_int64, c_void_p
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import blockwise_quant_ref as bq
import mla_indexer_prep_ref as pr
import mla_indexer_ref as ir
from mla_indexer_prep_ref import PREP_SLACK

UNSUPPORTED, INVALID = -1, -2
PAIRINGS = [False, True]
FAR_CONFIG = (16, 16)  # the one configuration the far case runs with (its cos / sin table has 163,840 rows)


def _case_list():
    return [("mix", Hi, P) for Hi, P in pr.CONFIGS] + [("far",) + FAR_CONFIG]


# ---- CPU 1: the statement --------------------------------------------------------------------------------------------------------
def test_statement_against_a_brute_force_loop():
    g = torch.Generator().manual_seed(0)
    rows, Hi, eps, rs = 4, 2, 1e-6, 0.25
    k = torch.randn(rows, 128, generator=g).bfloat16()
    q = torch.randn(rows, Hi, 128, generator=g).bfloat16()
    w, b = torch.randn(128, generator=g), torch.randn(128, generator=g)
    cs = pr.ms.cos_sin_table(pr.MAX_POS)
    ns, qi = torch.tensor([7, 300], dtype=torch.int32), torch.tensor([0, 2, 3], dtype=torch.int32)  # row 3 past q_index[-1]
    for interleaved in PAIRINGS:
        kr, qr, req, pos = pr.statement(k, q, w, b, cs, ns, qi, interleaved=interleaved, eps=eps, rotate_scale=rs)
        assert req.tolist() == [0, 0, 1, -1] and pos.tolist() == [5, 6, 299, -1]
        assert bool((kr[3] == 0).all()) and bool((qr[3] == 0).all())
        for r in range(3):
            x = [float(v) for v in k[r]]
            mean = sum(x) / 128
            var = sum((v - mean) ** 2 for v in x) / 128
            n = [(x[i] - mean) / (var + eps) ** 0.5 * float(w[i]) + float(b[i]) for i in range(128)]
            for vec, got in [(n, kr[r])] + [([float(v) for v in q[r, h]], qr[r, h]) for h in range(Hi)]:
                t = list(vec)
                for i in range(32):
                    lo, hi = (2 * i, 2 * i + 1) if interleaved else (i, i + 32)
                    c, s = float(cs[int(pos[r]), i]), float(cs[int(pos[r]), 32 + i])
                    t[lo], t[hi] = vec[lo] * c - vec[hi] * s, vec[hi] * c + vec[lo] * s
                want = [rs * sum((-1) ** bin(i & j).count("1") * t[j] for j in range(128)) for i in range(128)]
                assert torch.allclose(got, torch.tensor(want, dtype=torch.float64), rtol=0, atol=1e-11), (r, interleaved)


def test_hadamard_is_its_own_inverse_and_the_rotation_keeps_the_dot_product():
    H = pr.hadamard_matrix()
    assert torch.equal(H @ H, 128 * torch.eye(128, dtype=torch.float64)) and torch.equal(H, H.T)
    assert torch.equal(H[1], torch.tensor([1.0, -1.0] * 64, dtype=torch.float64)) and bool((H[0] == 1).all())
    # the fp32 butterfly in natural order is that matrix
    x = torch.randint(-8, 9, (5, 128)).float()
    assert torch.equal(pr._fwht32(x).double(), x.double() @ H.T)
    # rotated, unquantised q . k = unrotated q . k x 128 rotate_scale^2
    c = pr.case("mix", 16, 16)
    for rs in (128 ** -0.5, 0.125):
        kr, qr, _, _ = pr.statement(c.k, c.q, c.w, c.b, c.cos_sin, c.ns, c.q_index, rotate_scale=rs)
        k0, q0, _, _ = pr.statement(c.k, c.q, c.w, c.b, c.cos_sin, c.ns, c.q_index, rotate=False, use_rotate_scale=False)
        rot, flat = torch.einsum("rhd,rd->rh", qr, kr), torch.einsum("rhd,rd->rh", q0, k0)
        assert torch.allclose(rot, flat * (128 * rs * rs), rtol=1e-12, atol=1e-9 * float(flat.abs().max()))


def test_pow2_rule():
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    tiny = 2.0 ** -126
    big = float(torch.tensor(float.fromhex("0x1.fep127")).bfloat16())  # the largest bf16
    amax = f32([0.0, 2.0 ** -140, 448 * 2.0 ** -126, 448.0, 448 * 0.25, 448 * (1 + 2.0 ** -20), 448 * 1024.0, 3.0, big])
    got = pr.pow2_scale_of(amax)
    want = [tiny, tiny, tiny, 1.0, 0.25, 2.0, 1024.0, 2.0 ** -7, None]
    for a, g, w in zip(amax.tolist(), got.tolist(), want):
        s = a / 448
        assert g >= s and (g == tiny or g < 2 * s) and torch.frexp(f32(g))[0] == 0.5, (a, g)  # the smallest power of two >= s
        assert w is None or g == w, (a, g, w)
    assert torch.isfinite(got).all() and float(got[-1]) == 2.0 ** 120  # 3.39e38 / 448 = 7.6e35 -> 2^120
    # the division is exact and never saturates: codes decode to x / scale rounded to e4m3, and |x / scale| <= 448
    g = torch.Generator().manual_seed(1)
    a = (torch.randn(64, 128, generator=g) * torch.exp2(torch.randint(-20, 20, (64, 1), generator=g).float())).bfloat16()
    a[3] = 0
    codes, scale = pr.quant_pow2(a)
    assert bool(((a.float() / scale[:, None]).abs() <= 448).all()) and bool((codes.float().abs() <= 448).all())
    assert torch.equal(pr.pow2_scale_of(a.float().abs().amax(-1)), scale) and bool((codes[3].float() == 0).all())


# ---- CPU 2: surface and fakes ------------------------------------------------------------------------------------------------------
def test_surface():
    import hpc

    assert "mla_indexer_prep_fp8" in hpc.__all__ and callable(hpc.mla_indexer_prep_fp8)
    assert hasattr(torch.ops.hpc_mla, "mla_indexer_prep_fp8")
    doc = hpc.mla_indexer_prep_fp8.__doc__
    for word in ("tests/mla_indexer_prep_ref.py", "biased variance", "FIRST 64", "H128", "popcount", "rotate_scale", "ONE rounding",
                 "{16, 32, 64}", "pow2_scale", "ue8m0", "[1, 254]", "scale = amax / 448", "Hi ** -0.5", "mla_indexer_store_k_fp8",
                 "bit for bit", "zeros", "max_pos - 1", "multiples of 8", "hipGraph", "bit-identical", "int32", "neox"):
        assert word in doc, word
    assert "are the caller's" not in __import__("hpc.mla_indexer", fromlist=["x"]).__doc__


def test_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        def T(*shape, dtype=torch.bfloat16):
            return torch.empty(shape, dtype=dtype, device="cuda")

        rows, Hi = 6, 32
        cache, k, q = T(9, 64 * 132, dtype=torch.uint8), T(rows, 384)[:, 128:256], T(rows, Hi, 128)
        w, b, cs = T(128, dtype=torch.float32), T(128, dtype=torch.float32), T(4096, 64, dtype=torch.float32)
        ns, qi, bid = T(3, dtype=torch.int32), T(4, dtype=torch.int32), T(3, 64, dtype=torch.int32)
        hw, ok = T(rows, Hi, dtype=torch.float32), T(rows, 128)
        assert hpc.mla_indexer_prep_fp8(cache, k, w, b, cs, ns, qi, bid) is None
        assert hpc.mla_indexer_prep_fp8(None, k, w, b, cs, ns, qi, bid, out_k=ok) is None
        q8, wt = hpc.mla_indexer_prep_fp8(cache, k, w, b, cs, ns, qi, bid, q=q, head_weights=hw, softmax_scale=0.1, pow2_scale=True)
        assert (q8.shape, q8.dtype, q8.device.type) == ((rows, Hi, 128), torch.float8_e4m3fn, "cuda")
        assert (wt.shape, wt.dtype, wt.device.type) == ((rows, Hi), torch.float32, "cuda")
        oq, ow, orot = T(rows, Hi, 128, dtype=torch.float8_e4m3fn), T(rows, Hi, dtype=torch.float32), T(rows, Hi, 128)
        got = hpc.mla_indexer_prep_fp8(cache, k, w, b, cs, ns, qi, bid, q=q, head_weights=hw.bfloat16(), softmax_scale=0.1,
                                       out_k=ok, out_q=oq, out_weights=ow, out_q_rot=orot, interleaved=True)
        assert got[0] is oq and got[1] is ow


# ---- CPU 3: the C-ABI refuses on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


def call_prep(lib, refusal=False, **kw):
    """hpc_mla_indexer_prep_fp8_async / _refusal with pointers that are never dereferenced: every case here is refused, or has
    nothing to launch, before any device call"""
    a = dict(cache=4096, out_k=0, out_q=4096, out_w=4096, out_q_rot=0, k=4096, q=4096, hw=4096, nw=4096, nb=4096, cs=4096, ns=4096,
             qi=4096, bid=4096, rows=6, req=3, Hi=64, P=64, max_blocks=8, num_blocks=9, max_pos=4096, bs=None, k_rs=128, q_rs=None,
             q_hs=128, hw_bf16=0, ws=0.011, eps=1e-6, rs=0.088)
    a.update(kw)
    if a["bs"] is None:
        a["bs"] = a["P"] * 132
    if a["q_rs"] is None:
        a["q_rs"] = a["Hi"] * a["q_hs"]
    vp = lambda v: c_void_p(v) if v else None  # noqa: E731
    ip = lambda v: ctypes.cast(c_void_p(v), ctypes.POINTER(c_int)) if v else None  # noqa: E731
    args = (vp(a["cache"]), vp(a["out_k"]), vp(a["out_q"]), vp(a["out_w"]), vp(a["out_q_rot"]), vp(a["k"]), vp(a["q"]), vp(a["hw"]),
            vp(a["nw"]), vp(a["nb"]), vp(a["cs"]), ip(a["ns"]), ip(a["qi"]), ip(a["bid"]), a["rows"], a["req"], a["Hi"], a["P"],
            a["max_blocks"], a["num_blocks"], a["max_pos"], c_int64(a["bs"]), c_int64(a["k_rs"]), c_int64(a["q_rs"]), c_int64(a["q_hs"]),
            a["hw_bf16"], c_float(a["ws"]), c_float(a["eps"]), c_float(a["rs"]))
    if refusal:
        return lib.hpc_mla_indexer_prep_fp8_refusal(*args)
    return lib.hpc_mla_indexer_prep_fp8_async(*args, 0, 0, None)


_NO_Q = dict(q=0, hw=0, out_q=0, out_w=0)
_REFUSALS = [
    # Hi not in {16, 32, 64}
    (dict(Hi=8), UNSUPPORTED), (dict(Hi=48), UNSUPPORTED), (dict(Hi=128), UNSUPPORTED), (dict(Hi=0), UNSUPPORTED), (dict(rows=0, Hi=24), UNSUPPORTED),
    # a bad P; the cache's rule as the other indexer ops pin it
    (dict(P=48), UNSUPPORTED), (dict(P=8), UNSUPPORTED), (dict(P=256), UNSUPPORTED), (dict(P=0), UNSUPPORTED), (dict(rows=0, P=48), UNSUPPORTED),
    (dict(bs=64 * 132 - 16), UNSUPPORTED), (dict(bs=64 * 132 + 8), UNSUPPORTED), (dict(bs=-64 * 132), INVALID), (dict(cache=4096 + 8), UNSUPPORTED),
    # misaligned or short strides and bases
    (dict(k_rs=132), UNSUPPORTED), (dict(k_rs=120), UNSUPPORTED), (dict(k_rs=-128), UNSUPPORTED), (dict(q_hs=132), UNSUPPORTED),
    (dict(q_hs=120, q_rs=64 * 128), UNSUPPORTED), (dict(q_rs=64 * 128 + 4), UNSUPPORTED), (dict(q_rs=63 * 128 + 120), UNSUPPORTED),
    (dict(q_hs=136, q_rs=64 * 128), UNSUPPORTED), (dict(k=4096 + 8), UNSUPPORTED), (dict(q=4096 + 8), UNSUPPORTED),
    (dict(out_k=4096 + 8), UNSUPPORTED), (dict(out_q_rot=4096 + 2), UNSUPPORTED), (dict(out_q=4096 + 4), UNSUPPORTED),
    (dict(out_w=4096 + 2), UNSUPPORTED), (dict(hw=4096 + 2), UNSUPPORTED), (dict(hw=4096 + 1, hw_bf16=1), UNSUPPORTED),
    (dict(nw=4096 + 4), UNSUPPORTED), (dict(nb=4096 + 8), UNSUPPORTED), (dict(cs=4096 + 4), UNSUPPORTED),
    # no destination for the key
    (dict(cache=0), INVALID), (dict(cache=0, rows=0), INVALID),
    # q without head_weights or softmax_scale (the C-ABI takes float32(softmax_scale * Hi ** -0.5): not finite when it is
    # missing), or without its outputs; q's things without q
    (dict(hw=0), INVALID), (dict(ws=float("nan")), INVALID), (dict(ws=float("inf")), INVALID), (dict(out_q=0), INVALID),
    (dict(out_w=0), INVALID), (dict(q=0), INVALID), (dict(_NO_Q, out_q_rot=4096), INVALID), (dict(_NO_Q, hw=4096), INVALID),
    # the vector count overflowing int32
    (dict(rows=(1 << 31) // 65 + 1), UNSUPPORTED), (dict(rows=(1 << 31) - 1, Hi=16), UNSUPPORTED), (dict(_NO_Q, rows=(1 << 31) - 8), UNSUPPORTED),
    # the rest
    (dict(rows=-1), INVALID), (dict(req=-1), INVALID), (dict(max_blocks=-1), INVALID), (dict(num_blocks=-1), INVALID), (dict(max_pos=-1), INVALID),
    (dict(max_pos=0), INVALID), (dict(k=0), INVALID), (dict(nw=0), INVALID), (dict(nb=0), INVALID), (dict(cs=0), INVALID), (dict(ns=0), INVALID),
    (dict(qi=0), INVALID), (dict(bid=0), INVALID), (dict(eps=-1e-6), INVALID), (dict(eps=float("nan")), INVALID), (dict(rs=float("inf")), INVALID),
    # accepted up to the device call: nothing to launch
    (dict(rows=0), 0), (dict(req=0), 0), (dict(_NO_Q, rows=0), 0), (dict(_NO_Q, rows=0, Hi=0), 0), (dict(rows=0, cache=0, out_k=4096, P=48, bid=0), 0),
    (dict(rows=0, Hi=16, hw_bf16=1, hw=4096 + 2, out_q_rot=4096), 0), (dict(rows=0, P=128, bs=128 * 132 + 32), 0), (dict(rows=0, max_pos=0), 0),
]


@pytest.mark.parametrize("kwargs,code", _REFUSALS)
def test_cabi_refuses_on_the_host(lib, kwargs, code):
    assert call_prep(lib, **kwargs) == code, kwargs
    why = call_prep(lib, refusal=True, **kwargs)
    assert (why is None) == (code == 0), (kwargs, why)  # a message exactly when the call is refused
    assert why is None or len(why.decode()) > 10


def test_cabi_accepts_calls_with_work_in_words(lib):
    """calls with work that every host check accepts are refused by nothing (no launch is made here: the words only); the
    largest vector count that fits is accepted"""
    for kw in (dict(), dict(_NO_Q), dict(cache=0, out_k=4096, bid=0, P=0), dict(Hi=16, q_hs=136, q_rs=16 * 136 + 8), dict(k_rs=384),
               dict(hw_bf16=1, hw=4096 + 2), dict(out_k=4096, out_q_rot=4096), dict(rows=((1 << 31) - 17) // 65), dict(rows=1, k_rs=0)):
        assert call_prep(lib, refusal=True, **kw) is None, kw
    assert b"int32" in call_prep(lib, refusal=True, rows=(1 << 31) // 65 + 1)
    assert b"16, 32 or 64" in call_prep(lib, refusal=True, Hi=48)
    assert b"destination" in call_prep(lib, refusal=True, cache=0)
    assert b"head_weights" in call_prep(lib, refusal=True, ws=float("nan"))


def test_both_libraries_export_the_launcher():
    pkg = Path(__file__).resolve().parent.parent / "hpc-ops_amd" / "hpc"
    for name in ("libhpc_amd.so", "libhpc_amd_dev.so"):
        so = ctypes.CDLL(str(pkg / name))
        for kind in ("async", "refusal"):
            assert hasattr(so, f"hpc_mla_indexer_prep_fp8_{kind}"), (name, kind)


# ---- CPU 4: the bar has teeth, on the GPU tests' own inputs --------------------------------------------------------------------------
def test_cases_cover_what_they_claim():
    for Hi, P in pr.CONFIGS:
        c = pr.case("mix", Hi, P)
        ref = pr.reference(c, False)
        assert c.rows <= 100 and {0, P - 1} <= set(ref.slot.tolist()) and int(ref.pos.max()) >= 8192
        assert c.rows > int(c.q_index[-1]) and int(c.ns[-1]) == 0 and int(c.q_index[-1]) > int(c.q_index[-2])  # both paddings
        assert any(n == 0 and s > 0 for s, n in c.reqs) and any(s == 0 for s, n in c.reqs)
        pages = [sorted(set(ref.page[ref.req[ref.idx] == r].tolist())) for r in range(c.num_req)]
        assert sum(len(p) > 1 for p in pages) >= 3  # runs over a page edge
        small = c.k.float().pow(2).mean(-1)[ref.idx]
        assert int((small < 1e-5).sum()) >= 4 and int((small > 500).sum()) >= 4
    assert int(pr.reference(pr.case("far", *FAR_CONFIG), False).pos.max()) >= 160000
    for Hi, P in pr.CONFIGS:  # the exact inputs: integers in [-8, 8], and the one rounding does round somewhere, for both pairings
        c = pr.case("mix", Hi, P, True)
        assert bool((c.q.float() == c.q.float().round()).all()) and float(c.q.float().abs().max()) == 8
        for interleaved in PAIRINGS:
            want = pr.reference(c, interleaved, 0.125).q
            assert bool((want * 8 == (want * 8).round()).all()) and int((want.bfloat16().double() != want).sum()) >= 4


@pytest.mark.parametrize("interleaved", PAIRINGS)
def test_bar_accepts_fp32_model(interleaved):
    worst = [0.0, 0.0]
    for name, Hi, P in _case_list():
        c = pr.case(name, Hi, P)
        out_k, out_q = pr.model32(c.k, c.q, c.w, c.b, c.cos_sin, c.ns, c.q_index, interleaved=interleaved)
        failed = pr.check_outputs(c, interleaved, out_k, out_q, label=f"model {name} Hi {Hi} P {P}")
        assert not failed, failed
        worst = [max(a, b) for a, b in zip(worst, pr.worst_excess(c, interleaved, out_k, out_q))]
    print(f"\nfp32 model, worst excess over the half-ulp term: key {worst[0]:.3g} = {worst[0] / PREP_SLACK:.3g} x PREP_SLACK, "
          f"queries {worst[1]:.3g} = {worst[1] / PREP_SLACK:.3g} x PREP_SLACK")
    assert 8 * max(worst) <= PREP_SLACK <= 2.0 ** -16  # the slack keeps the margin it was given, below its cap


@pytest.mark.parametrize("name", list(pr.MUTANTS))
def test_bar_rejects_mutants(name):
    """each mutant, as the float64 statement with one thing wrong rounded once to bf16, through check_outputs(): rejected, and by
    a wide factor (printed) - on every vector kind it touches"""
    c = pr.case("mix", 16, 16)
    kr, qr, _, _ = pr.statement(c.k, c.q, c.w, c.b, c.cos_sin, c.ns, c.q_index, **pr.MUTANTS[name])
    out_k, out_q = kr.bfloat16(), qr.bfloat16()
    failed = pr.check_outputs(c, False, out_k, out_q, label=name)
    ek, eq = pr.worst_excess(c, False, out_k, out_q)
    print(f"{name}: rejected by {failed}; worst excess key {ek / PREP_SLACK:.3g} x PREP_SLACK, queries {eq / PREP_SLACK:.3g} x PREP_SLACK")
    assert failed == (["out_k"] if name in pr.KEY_ONLY else ["out_k", "out_q_rot"]), failed
    assert ek > 1000 * PREP_SLACK and (name in pr.KEY_ONLY or eq > 1000 * PREP_SLACK)


def test_another_eps_shows_on_the_small_rows():
    """eps = 1e-5 moves a row of scale 1 by 5e-6 relative - a few times the slack -, every row of scale 1e-3 by a third of its
    largest value"""
    from utils import rope_excess

    c = pr.case("mix", 16, 16)
    ref = pr.reference(c, False)
    kr, _, _, _ = pr.statement(c.k, c.q, c.w, c.b, c.cos_sin, c.ns, c.q_index, eps=1e-5)
    ex = rope_excess(ref.k[:, None], kr.bfloat16()[:, None])[:, 0]
    small = (c.k.float().pow(2).mean(-1) < 1e-5) & (ref.req >= 0)
    assert int(small.sum()) >= 4 and bool((ex[small] > 1e5 * PREP_SLACK).all()) and bool((ex[~small] < 1e-5).all())


def test_rows_of_no_request_must_be_zero():
    c = pr.case("mix", 16, 16)
    out_k, out_q = pr.model32(c.k, c.q, c.w, c.b, c.cos_sin, c.ns, c.q_index)
    dead = pr.reference(c, False).dead
    assert dead.numel() == 3
    out_k[dead[0], 5] = 1e-30
    out_q[dead[-1], 3, 7] = -1e-30
    assert pr.check_outputs(c, False, out_k, out_q) == ["out_k rows of no request", "out_q_rot rows of no request"]


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _guarded(rows, tail, dtype, fill):
    """an output of [rows, *tail] between two sentinel rows of a parent: (parent, the contiguous view)"""
    if dtype == pr.F8:
        parent = torch.full((rows + 2,) + tail, fill, dtype=torch.uint8, device="cuda").view(pr.F8)
    else:
        parent = torch.full((rows + 2,) + tail, fill, dtype=dtype, device="cuda")
    return parent, parent[1:-1]


def _guards_hold(parent, fill):
    raw = parent.view(torch.uint8) if parent.dtype == pr.F8 else parent
    return bool((raw[0] == fill).all()) and bool((raw[-1] == fill).all())


def _run(c, *, interleaved=False, pow2=False, rotate_scale=128 ** -0.5, cache=True, bid=None, with_q=True, hw_bf16=False):
    """one call on the case's inputs as views of sentinel-filled parents, every output between sentinel rows; returns the
    buffers (GPU) and what the op returned"""
    import hpc

    kp, qp, k, q = pr.parents(c, "cuda")
    o = SimpleNamespace(kp=kp, qp=qp, interleaved=interleaved, rotate_scale=rotate_scale)
    o.cache = torch.full((c.nblocks, c.P * 132), pr.FILL, dtype=torch.uint8, device="cuda") if cache else None
    o.out_k_parent, o.out_k = _guarded(c.rows, (128,), torch.bfloat16, pr.SENTINEL)
    o.q8_parent, o.q8 = _guarded(c.rows, (c.Hi, 128), pr.F8, pr.FILL)
    o.w_parent, o.weights = _guarded(c.rows, (c.Hi,), torch.float32, pr.SENTINEL)
    o.rot_parent, o.out_q_rot = _guarded(c.rows, (c.Hi, 128), torch.bfloat16, pr.SENTINEL)
    hw = c.head_weights.bfloat16() if hw_bf16 else c.head_weights
    qargs = dict(q=q, head_weights=hw.cuda(), softmax_scale=c.softmax_scale, out_q=o.q8, out_weights=o.weights,
                 out_q_rot=o.out_q_rot) if with_q else {}
    o.ret = hpc.mla_indexer_prep_fp8(o.cache, k, c.w.cuda(), c.b.cuda(), c.cos_sin.cuda(), c.ns.cuda(), c.q_index.cuda(),
                                     (c.bid if bid is None else bid).cuda(), eps=1e-6, interleaved=interleaved,
                                     rotate_scale=rotate_scale, pow2_scale=pow2, out_k=o.out_k, **qargs)
    torch.cuda.synchronize()
    return o


def _inputs_and_guards_untouched(c, o, with_q=True):
    kp, qp, _, _ = pr.parents(c)
    ok = torch.equal(o.kp.cpu().view(torch.int16), kp.view(torch.int16)) and torch.equal(o.qp.cpu().view(torch.int16), qp.view(torch.int16))
    ok = ok and _guards_hold(o.out_k_parent, pr.SENTINEL)
    if with_q:
        ok = ok and _guards_hold(o.q8_parent, pr.FILL) and _guards_hold(o.w_parent, pr.SENTINEL) and _guards_hold(o.rot_parent, pr.SENTINEL)
    return ok


def _quantised(rows_bf16, pow2):
    """(codes, scales) of bf16 rows [N, 128] by the torch statement of the quantiser in force"""
    if pow2:
        return pr.quant_pow2(rows_bf16)
    codes, scales = bq.quant(rows_bf16)
    return codes, scales[:, 0]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("interleaved", PAIRINGS)
@pytest.mark.parametrize("Hi,P", pr.CONFIGS)
def test_exact_inputs_bit_for_bit(Hi, P, interleaved, pow2):
    """q integer-valued in [-8, 8], a cos / sin table of quarter turns, rotate_scale = 1 / 8: every intermediate of the query
    path is exact in fp32, so out_q_rot must EQUAL the float64 statement rounded once to bf16; q8 and the scales must equal the
    quantiser's torch statement on out_q_rot, weights the two fp32 multiplies done in torch; the cache holds the quantised out_k"""
    c = pr.case("mix", Hi, P, True)
    o = _run(c, interleaved=interleaved, pow2=pow2, rotate_scale=0.125)
    ref = pr.reference(c, interleaved, 0.125)
    assert o.ret[0] is o.q8 and o.ret[1] is o.weights
    rot = o.out_q_rot.cpu()
    assert torch.equal(_bits(rot), _bits(ref.q.bfloat16()))
    codes, scales = _quantised(rot.reshape(-1, 128), pow2)
    assert torch.equal(_bits(o.q8.cpu().reshape(-1, 128)), _bits(codes))
    want_w = pr.fold(c.head_weights, scales.view(c.rows, Hi), c.softmax_scale, Hi)
    want_w[ref.dead] = 0
    assert torch.equal(_bits(o.weights.cpu()), _bits(want_w))
    # the key (LayerNorm is not exact: on the bar), and the cache = the quantiser's statement on out_k
    out_k = o.out_k.cpu()
    assert not pr.check_outputs(c, interleaved, out_k, None, label=f"exact Hi {Hi} P {P}", rotate_scale=0.125)
    kc, ks = _quantised(out_k, pow2)
    cache0 = torch.full((c.nblocks, P * 132), pr.FILL, dtype=torch.uint8)
    assert torch.equal(o.cache.cpu(), pr.expected_cache(c, ref, kc, ks, cache0))
    assert _inputs_and_guards_untouched(c, o)


@pytest.mark.gpu
@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("name,Hi,P", _case_list())
def test_fused_equals_parts_bit_for_bit(name, Hi, P, pow2):
    """random inputs: the cache after the op equals a second cache written by hpc.mla_indexer_store_k_fp8(out_k) and every byte
    the op should not touch is unchanged (page tails, the guard page, unlisted pages); q8 / weights equal
    hpc.blockwise_fp8_quant(out_q_rot) plus the fold.  pow2_scale: against the torch statement of the rule."""
    import hpc

    c = pr.case(name, Hi, P)
    ref = pr.reference(c, False)
    o = _run(c, pow2=pow2, hw_bf16=pow2)
    out_k, rot = o.out_k.cpu(), o.out_q_rot.cpu()
    cache0 = torch.full((c.nblocks, P * 132), pr.FILL, dtype=torch.uint8)
    hw = c.head_weights.bfloat16() if pow2 else c.head_weights
    if pow2:
        kc, ks = pr.quant_pow2(out_k)
        codes, scales = pr.quant_pow2(rot.reshape(-1, 128))
        want_cache = pr.expected_cache(c, ref, kc, ks, cache0)
        assert bool((torch.frexp(scales)[0] == 0.5).all())  # powers of two
    else:
        second = cache0.cuda()
        hpc.mla_indexer_store_k_fp8(second, o.out_k, c.ns.cuda(), c.q_index.cuda(), c.bid.cuda())
        want_cache = second.cpu()
        kc, ks = _quantised(out_k, False)
        assert torch.equal(want_cache, pr.expected_cache(c, ref, kc, ks, cache0))  # and the parts are the statement's
        codes, scales = hpc.blockwise_fp8_quant(o.out_q_rot.reshape(-1, 128))
        codes, scales = codes.cpu(), scales.cpu()[:, 0]
    got_cache = o.cache.cpu()
    assert torch.equal(got_cache, want_cache)
    written = torch.zeros(c.nblocks, dtype=torch.bool)
    written[ref.page] = True
    assert bool((got_cache[~written] == pr.FILL).all()) and not written[c.guard] and int((~written).sum()) >= 4
    assert torch.equal(_bits(o.q8.cpu().reshape(-1, 128)), _bits(codes))
    want_w = pr.fold(hw, scales.view(c.rows, Hi), c.softmax_scale, Hi)
    want_w[ref.dead] = 0
    assert torch.equal(_bits(o.weights.cpu()), _bits(want_w))
    assert _inputs_and_guards_untouched(c, o)


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", PAIRINGS)
@pytest.mark.parametrize("name,Hi,P", _case_list())
def test_random_inputs_on_the_bar(name, Hi, P, interleaved):
    """bf16 Gaussian inputs, a fifth of the requests' rows scaled by 1e-3 and a fifth by 30, random norm weight and bias: out_k
    and out_q_rot through the check_outputs() of the CPU bar test"""
    c = pr.case(name, Hi, P)
    o = _run(c, interleaved=interleaved)
    failed = pr.check_outputs(c, interleaved, o.out_k.cpu(), o.out_q_rot.cpu(), label=f"{name} Hi {Hi} P {P} interleaved {interleaved}")
    assert not failed, failed
    # the key alone, into out_k alone, gives the same bits
    only = _run(c, interleaved=interleaved, cache=False, with_q=False)
    assert only.ret is None and torch.equal(_bits(only.out_k), _bits(o.out_k)) and _inputs_and_guards_untouched(c, only, with_q=False)


@pytest.mark.gpu
def test_guards():
    """poisoned page ids (-7 and one far outside the pool), -1 padding and positions beyond the table store nothing; rows of no
    request come back as zeros in all four outputs; the sentinels around the k / q views and behind every output survive"""
    Hi, P = 32, 128
    c = pr.case("mix", Hi, P)
    ref = pr.reference(c, False)
    clean = _run(c)
    for t in (clean.out_k, clean.q8.view(torch.uint8), clean.weights, clean.out_q_rot):
        assert bool((t[ref.dead.cuda()] == 0).all()) and bool((t[ref.idx.cuda()] != 0).any())
    assert _inputs_and_guards_untouched(c, clean)
    # poison the page of some live rows, pad others with -1, and cut the table so that the positions at 4096+ lie beyond it
    cols = 4096 // P
    bid = c.bid[:, :cols].clone()
    kept = torch.ones(ref.idx.numel(), dtype=torch.bool)
    for i in range(ref.idx.numel()):
        r, blk = int(ref.req[ref.idx[i]]), int(ref.pos[ref.idx[i]]) // P
        if blk >= cols:
            kept[i] = False
        elif r % 3 != 2:
            bid[r, blk] = (-7, ir.POISONED, -1)[(r // 3) % 3] if r % 3 == 0 else -1
            kept[i] = False
    assert 5 <= int(kept.sum()) <= ref.idx.numel() - 20 and int((ref.pos[ref.idx] >= 4096).sum()) >= 10
    o = _run(c, bid=bid)
    kc, ks = _quantised(o.out_k.cpu(), False)
    want = torch.full((c.nblocks, P * 132), pr.FILL, dtype=torch.uint8)
    for i in kept.nonzero().squeeze(1).tolist():
        r, page, t = int(ref.idx[i]), int(ref.page[i]), int(ref.slot[i])
        want[page, 128 * t: 128 * t + 128] = kc[r].view(torch.uint8)
        want[page, 128 * P + 4 * t: 128 * P + 4 * t + 4] = ks[r: r + 1].view(torch.uint8)
    assert torch.equal(o.cache.cpu(), want)
    # the outputs do not depend on the table
    for a, b in ((o.out_k, clean.out_k), (o.q8, clean.q8), (o.weights, clean.weights), (o.out_q_rot, clean.out_q_rot)):
        assert torch.equal(_bits(a), _bits(b))
    assert _inputs_and_guards_untouched(c, o)


@pytest.mark.gpu
def test_refusals_and_empty_calls():
    import hpc

    c = pr.case("mix", 16, 16)
    dev = lambda t: t.cuda()  # noqa: E731
    cache = torch.zeros(c.nblocks, 16 * 132, dtype=torch.uint8, device="cuda")
    base = (dev(c.k), dev(c.w), dev(c.b), dev(c.cos_sin), dev(c.ns), dev(c.q_index), dev(c.bid))
    with pytest.raises(RuntimeError, match="one of k_cache and out_k"):
        hpc.mla_indexer_prep_fp8(None, *base)
    with pytest.raises(RuntimeError, match="head_weights and softmax_scale"):
        hpc.mla_indexer_prep_fp8(cache, *base, q=dev(c.q))
    with pytest.raises(RuntimeError, match="head_weights and softmax_scale"):
        hpc.mla_indexer_prep_fp8(cache, *base, q=dev(c.q), head_weights=dev(c.head_weights))
    with pytest.raises(RuntimeError, match="need q"):
        hpc.mla_indexer_prep_fp8(cache, *base, head_weights=dev(c.head_weights))
    with pytest.raises(RuntimeError, match="16, 32 or 64"):
        hpc.mla_indexer_prep_fp8(cache, *base, q=dev(c.q)[:, :12], head_weights=dev(c.head_weights)[:, :12].contiguous(), softmax_scale=0.1)
    with pytest.raises(RuntimeError, match="k dtype must be bfloat16"):
        hpc.mla_indexer_prep_fp8(cache, base[0].float(), *base[1:])
    with pytest.raises(RuntimeError, match="block_size"):
        hpc.mla_indexer_prep_fp8(cache[:, : 12 * 132], *base)
    with pytest.raises(RuntimeError, match="k row stride"):
        hpc.mla_indexer_prep_fp8(cache, torch.zeros(c.rows, 132, dtype=torch.bfloat16, device="cuda")[:, :128], *base[1:])
    # no rows, no requests: no launch, the outputs' shapes
    k0, q0 = torch.empty(0, 128, dtype=torch.bfloat16, device="cuda"), torch.empty(0, 16, 128, dtype=torch.bfloat16, device="cuda")
    q8, w = hpc.mla_indexer_prep_fp8(cache, k0, *base[1:], q=q0, head_weights=torch.empty(0, 16, device="cuda"), softmax_scale=0.1)
    assert q8.shape == (0, 16, 128) and w.shape == (0, 16)
    none = (torch.empty(0, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
            torch.empty(0, 4, dtype=torch.int32, device="cuda"))
    assert hpc.mla_indexer_prep_fp8(cache, *base[:4], *none) is None


@pytest.mark.gpu
def test_repeatable_and_replays_in_a_graph_after_everything_changed_in_place():
    """two calls are bit-identical; a hipGraph captured once and replayed after lengths, page table and inputs changed in place
    gives the new result, and the capture allocates nothing"""
    import hpc

    Hi, P = 64, 32
    a = pr.case("mix", Hi, P)
    g = torch.Generator().manual_seed(99)
    # a second step over the same buffers: other data, every request one token further (other slots; a token that moves into a
    # block the request has no page for is not stored: -1), the pool's pages renamed
    rename = torch.randperm(a.nblocks, generator=g).int()
    bid2 = torch.where(a.bid == a.guard, torch.full_like(a.bid, -1), rename[a.bid.long()])
    step2 = SimpleNamespace(k=(torch.randn(a.rows, 128, generator=g) * 3).bfloat16(), q=torch.randn(a.rows, Hi, 128, generator=g).bfloat16(),
                            head_weights=torch.randn(a.rows, Hi, generator=g), ns=a.ns + (a.ns > 0).int(), bid=bid2)
    first = _run(a)
    again = _run(a)
    for name in ("cache", "out_k", "q8", "weights", "out_q_rot"):
        assert torch.equal(_bits(getattr(first, name)), _bits(getattr(again, name))), name

    k, q, hw = a.k.cuda(), a.q.cuda(), a.head_weights.cuda()
    ns, bid, qi = a.ns.cuda(), a.bid.cuda(), a.q_index.cuda()
    w, b, cs = a.w.cuda(), a.b.cuda(), a.cos_sin.cuda()
    cache = torch.full((a.nblocks, P * 132), pr.FILL, dtype=torch.uint8, device="cuda")
    out_k = torch.zeros(a.rows, 128, dtype=torch.bfloat16, device="cuda")
    q8 = torch.zeros(a.rows, Hi, 128, device="cuda").to(pr.F8)
    wt = torch.zeros(a.rows, Hi, device="cuda")
    rot = torch.zeros(a.rows, Hi, 128, dtype=torch.bfloat16, device="cuda")

    def step():
        return hpc.mla_indexer_prep_fp8(cache, k, w, b, cs, ns, qi, bid, q=q, head_weights=hw, softmax_scale=a.softmax_scale,
                                        out_k=out_k, out_q=q8, out_weights=wt, out_q_rot=rot)

    def eager(src_ns, src_bid):
        c2 = torch.full((a.nblocks, P * 132), pr.FILL, dtype=torch.uint8, device="cuda")
        o = [torch.empty_like(t) for t in (out_k, q8, wt, rot)]
        hpc.mla_indexer_prep_fp8(c2, k.clone(), w, b, cs, src_ns.cuda(), qi, src_bid.cuda(), q=q.clone(), head_weights=hw.clone(),
                                 softmax_scale=a.softmax_scale, out_k=o[0], out_q=o[1], out_weights=o[2], out_q_rot=o[3])
        return [c2] + o

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated()
        step()
        assert torch.cuda.memory_allocated() == before  # nothing allocated in the capture
    for data in (a, step2, a):
        k.copy_(data.k), q.copy_(data.q), hw.copy_(data.head_weights), ns.copy_(data.ns), bid.copy_(data.bid)
        cache.fill_(pr.FILL)
        for t in (out_k, wt, rot):
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((cache, out_k, q8, wt, rot), eager(data.ns, data.bid)):
            assert torch.equal(_bits(got), _bits(want))
        assert torch.equal(cache, first.cache) == (data is a) and torch.equal(_bits(rot), _bits(first.out_q_rot)) == (data is a)
    assert torch.equal(_bits(out_k), _bits(first.out_k)) and torch.equal(cache, first.cache)
    del graph


# ---- GPU: end to end with planted needles ---------------------------------------------------------------------------------------------
NEEDLE_FACTOR = 2.0
"""The float64 gap between the topk-th and the next logit of every request must exceed NEEDLE_FACTOR x the sum of the two sides'
worst quantisation error bounds.  The bound of logit j, from the ROTATED vectors qr, kr that are quantised: a column x_d of a
128-block with abs-max A and scale s <= 2 A / 448 (the pow2 scale is at most twice amax / 448) is stored with an error of at
most eta * max(|x_d|, 2^-6 s) <= eta * xa_d, xa_d = max(|x_d|, A * 2^-13), eta = 2^-4 + 2^-8: half an e4m3 ulp relative (2^-4),
below the subnormal threshold 2^-6 s half the subnormal step, and the bf16 rounding in front (2^-9) with the cross term.  Then
|d(q . k)| <= ((1 + eta)^2 - 1) sum_d qa_d ka_d, ReLU is 1-Lipschitz, and the accumulation of the logits op and the fp32 fold stay
within 2^-13 of the same sum (C_BAR of tests/test_mla_indexer.py is 2^-14 of it):
    E_j = sum_h |w_h| ((1 + eta)^2 - 1 + 2^-13) sum_d qa_hd ka_jd."""


def _needle_case(P, Hi, topk, contexts, seed=11):
    """every token of every request as one prefill batch.  Keys: Gaussian rows; `topk` needle positions per request get a
    multiple of a fixed +-1 pattern U on the 64 columns RoPE does not turn.  Queries: the same pattern times a per-head
    amplitude, small Gaussian values on the RoPE columns.  Head weights positive.  LayerNorm weight near 1, small bias."""
    g = torch.Generator().manual_seed(seed)
    T = sum(contexts)
    U = torch.zeros(128)
    U[64:] = torch.tensor([1.0, -1.0] * 32)[torch.randperm(64, generator=g)]
    k = torch.randn(T, 128, generator=g)
    needles, off = [], 0
    for L in contexts:
        pick = torch.randperm(L, generator=g)[: min(topk, L)].sort()[0]
        needles.append(pick)
        if L > topk:
            k[off + pick] += (3.0 + 2.0 * torch.rand(len(pick), 1, generator=g)) * U
        off += L
    q = (0.5 + torch.rand(T, Hi, 1, generator=g)) * U + 0.05 * torch.randn(T, Hi, 128, generator=g) * (torch.arange(128) < 64)
    nblk = [-(-L // P) for L in contexts]
    perm = torch.randperm(sum(nblk) + 2, generator=g).int()
    bid = torch.full((len(contexts), max(nblk) + 1), -1, dtype=torch.int32)
    o = 0
    for r, n in enumerate(nblk):
        bid[r, :n] = perm[o: o + n]
        o += n
    qi = torch.tensor([0] + torch.tensor(contexts).cumsum(0).tolist(), dtype=torch.int32)
    return SimpleNamespace(k=k.bfloat16(), q=q.bfloat16(), w=1 + 0.05 * torch.randn(128, generator=g), b=0.02 * torch.randn(128, generator=g),
                           head_weights=0.25 + torch.rand(T, Hi, generator=g), ns=torch.tensor(contexts, dtype=torch.int32), q_index=qi,
                           bid=bid, nblocks=sum(nblk) + 2, P=P, needles=needles, contexts=contexts, cos_sin=pr.ms.cos_sin_table(pr.MAX_POS))


def _float64_indexer(c, Hi, topk, softmax_scale):
    """(logits float64 [B, columns] of each request's LAST token over its context on the UNROTATED, UNQUANTISED key and queries,
    NaN past the context; E the error bound of NEEDLE_FACTOR's docstring, from the rotated ones)"""
    k0, q0, _, _ = pr.statement(c.k, c.q, c.w, c.b, c.cos_sin, c.ns, c.q_index, rotate=False, use_rotate_scale=False)
    kr, qr, _, _ = pr.statement(c.k, c.q, c.w, c.b, c.cos_sin, c.ns, c.q_index)
    cols = c.bid.shape[1] * c.P
    logits = torch.full((len(c.contexts), cols), float("nan"), dtype=torch.float64)
    bound = torch.zeros_like(logits)
    eta = 2.0 ** -4 + 2.0 ** -8
    factor = (1 + eta) ** 2 - 1 + 2.0 ** -13
    floor = lambda x: torch.maximum(x.abs(), x.abs().amax(-1, keepdim=True) * 2.0 ** -13)  # noqa: E731
    for b, L in enumerate(c.contexts):
        if L == 0:
            continue
        lo, last = int(c.q_index[b]), int(c.q_index[b + 1]) - 1
        hw = c.head_weights[last].double() * (softmax_scale * Hi ** -0.5)
        logits[b, :L] = (hw[:, None] * (q0[last] @ k0[lo: last + 1].T).clamp_min(0)).sum(0)
        bound[b, :L] = factor * (hw.abs()[:, None] * (floor(qr[last]) @ floor(kr[lo: last + 1]).T)).sum(0)
    return logits, bound


@pytest.mark.gpu
def test_end_to_end_with_planted_needles():
    """the op's (q8, weights) and cache through hpc.mla_indexer_topk_fp8 against the top-k of a float64 indexer on the unrotated,
    unquantised inputs, torch.equal; the gap condition of NEEDLE_FACTOR is checked on the CPU first"""
    import hpc

    P, Hi, topk, contexts = 64, 16, 24, [150, 20, 260, 24, 25]
    c = _needle_case(P, Hi, topk, contexts)
    ss = 128 ** -0.5
    logits, bound = _float64_indexer(c, Hi, topk, ss)
    lens = torch.tensor(contexts)
    want = ir.topk_statement(logits, lens, 1, topk)
    worst = float("inf")
    for b, L in enumerate(contexts):
        if L <= topk:
            assert want[b].tolist() == list(range(L)) + [-1] * (topk - L)
            continue
        assert torch.equal(want[b].long(), c.needles[b])  # the float64 indexer finds the planted positions
        order = logits[b, :L].argsort(descending=True)
        kth, nxt = int(order[topk - 1]), int(order[topk])
        gap, err = float(logits[b, kth] - logits[b, nxt]), float(bound[b, :L][order[:topk]].max() + bound[b, :L][order[topk:]].max())
        print(f"request {b}: gap {gap:.4g}, error bounds {err:.4g}, ratio {gap / err:.3g} (needs {NEEDLE_FACTOR})")
        worst = min(worst, gap / err)
    assert worst > NEEDLE_FACTOR, worst
    T = sum(contexts)
    cache = torch.full((c.nblocks, P * 132), pr.FILL, dtype=torch.uint8, device="cuda")
    for pow2 in (False, True):
        cache.fill_(pr.FILL)
        q8, weights = hpc.mla_indexer_prep_fp8(cache, c.k.cuda(), c.w.cuda(), c.b.cuda(), c.cos_sin.cuda(), c.ns.cuda(), c.q_index.cuda(),
                                               c.bid.cuda(), q=c.q.cuda(), head_weights=c.head_weights.cuda(), softmax_scale=ss,
                                               pow2_scale=pow2)
        assert q8.shape == (T, Hi, 128) and weights.shape == (T, Hi)
        last = (c.q_index[1:] - 1).clamp_min(0).long().cuda()  # each request's last token is its decode query
        idx = hpc.mla_indexer_topk_fp8(q8[last].contiguous(), weights[last].contiguous(), cache, c.bid.cuda(), c.ns.cuda(), topk,
                                       new_kv_included=True)
        assert torch.equal(idx.cpu(), want), pow2
