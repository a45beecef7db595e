"""CPU: the bar of the MLA latent-cache write op (tests/mla_store_ref.py::check_outputs) has teeth.

* an fp32 model of a correct kernel (one rounding) passes every check on every case builder, both pairings and every layout,
  and its worst excess over the half-ulp term - the figure ROPE_SLACK is a margin on - is printed;
* fourteen planted errors, each the output of a plausibly wrong kernel, are rejected;
* the fake op returns the real op's shapes and dtypes for every argument combination; both libraries export the launcher, which
  refuses bad arguments on the host (never-dereferenced pointers through the C-ABI)."""
import pytest
import torch

import mla_store_ref as ms
from utils import ROPE_SLACK


def _run_model(c, sp, interleaved, **plant):
    stores = ms.make_stores(c, sp)
    before = ms.snapshot(stores)
    ret = ms.model(c, sp, stores, interleaved, **plant)
    return stores, before, ret


def test_statement_basics():
    """position 0 does not turn; a row of ones with weight one normalises to 1 / sqrt(1 + eps); the two pairings are one
    rotation under the permutation that maps (2i, 2i + 1) to (i, i + 32)"""
    cs = ms.cos_sin_table(ms.MAX_POS)
    kv = torch.ones(2, ms.DIM).bfloat16()
    q = torch.randn(2, 3, 64).bfloat16()
    ns, qi = torch.tensor([1, 5000], dtype=torch.int32), torch.tensor([0, 1, 2], dtype=torch.int32)
    lat, qo, req, pos = ms.statement(kv, q, cs, torch.ones(512), ns, qi, True)
    assert pos.tolist() == [0, 4999] and req.tolist() == [0, 1]
    assert torch.equal(qo[0], q[0].double()) and torch.equal(lat[0, 512:], kv[0, 512:].double())
    assert torch.allclose(lat[:, :512], torch.full((2, 512), 1 / (1 + 1e-6) ** 0.5, dtype=torch.float64), rtol=0, atol=1e-15)
    perm = torch.cat([torch.arange(0, 64, 2), torch.arange(1, 64, 2)])  # interleaved element order -> neox order
    _, qn, _, _ = ms.statement(kv, q[..., perm], cs, torch.ones(512), ns, qi, False)
    assert torch.equal(qn, qo[..., perm])
    assert float((qo[1] - q[1].double()).abs().max()) > 0.1  # position 4999 does turn


def test_row_positions_rule():
    ns = torch.tensor([10, 0, 7, 0], dtype=torch.int32)
    qi = torch.tensor([0, 2, 2, 5, 7], dtype=torch.int32)  # request 1 owns no row, request 3 (length 0) owns rows 5, 6
    req, pos = ms.row_positions(ns, qi, 9)
    assert req.tolist() == [0, 0, 2, 2, 2, -1, -1, -1, -1] and pos.tolist() == [8, 9, 4, 5, 6, -1, -1, -1, -1]


@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("name", ms.CASES)
def test_bar_accepts_fp32_model(name, interleaved):
    worst = [0.0, 0.0, 0.0]
    for H, P, sp in ((3, 16, ms.spec("plain")), (16, 64, ms.spec("padded", out_ckv=True)), (20, 128, ms.spec("pool", q="inplace")),
                     (16, 16, ms.spec(cache=False, out_ckv=True, q="fresh")), (16, 64, ms.spec(q=None))):
        c = ms.case(name, H, P)
        stores, before, ret = _run_model(c, sp, interleaved)
        failed = ms.check_outputs(c, sp, stores, before, ret, interleaved, label=f"{name} H {H} P {P} {sp.layout}")
        assert not failed, failed
        worst = [max(a, b) for a, b in zip(worst, ms.worst_excess(c, sp, stores, ret, interleaved))]
    print(f"\nfp32 model on {name}, worst excess over the half-ulp term: latent {worst[0] / ROPE_SLACK:.3g}, k_pe "
          f"{worst[1] / ROPE_SLACK:.3g}, q_pe {worst[2] / ROPE_SLACK:.3g} x ROPE_SLACK")
    assert 4 * max(worst) <= ROPE_SLACK  # the slack keeps the margin it was given over a correct fp32 kernel


def test_cases_cover_what_they_claim():
    far = ms.reference(ms.case("far", 3, 16), True)
    assert int(far.pos.max()) >= 160000
    for P in (16, 64, 128):
        slots, reqs, highest = set(), [], 0
        for name in ms.CASES[:5]:
            c = ms.case(name, 3, P)
            ref = ms.reference(c, True)
            slots |= set(ref.slot.tolist())
            highest = max(highest, int(ref.pos.max()))
            reqs += c.reqs
            assert c.rows > int(c.q_index[-1]) and int(c.ns[-1]) == 0 and int(c.q_index[-1]) > int(c.q_index[-2])  # both paddings
            small = c.y[:, ms.KV_A_AT: ms.KV_A_AT + 512].float().pow(2).mean(-1)[ref.idx]
            assert bool((small < 1e-5).any()) and (bool((small > 500).any()) or c.num_req < 4)
            pages = [sorted(set(ref.page[ref.req[ref.idx] == r].tolist())) for r in range(c.num_req)]
            assert any(len(p) > 1 for p in pages) or name == "decode_mtp0_7" or name == "decode_mtp0_16"  # a run over a page edge
        assert {0, P - 1} <= slots and highest >= 8192
        assert any(n == 0 and s > 0 for s, n in reqs) and any(s == 0 for s, n in reqs)


PLANTED = {
    "epsilon 1e-5": dict(eps=1e-5),
    "mean over 576 columns": dict(mean_cols=576),
    "norm also on k_pe": dict(on_kpe="norm"),
    "norm weight also on k_pe": dict(on_kpe="weight"),
    "latent left unnormalised": dict(normalise=False),
    "sine with the wrong sign": dict(sin_sign=-1.0),
    "position off by one": dict(pos_shift=1),
    "position off by minus one": dict(pos_shift=-1),
    "the other pairing": dict(other_pairing=True),
    "cos / sin of another request's row": dict(neighbours_cos_sin=True),
    "token stored one slot later": dict(slot_shift=1),
    "truncation instead of round-to-nearest": dict(truncate=True),
    "write into columns :512 of the q buffer": dict(touch_q_nope=True),
    "cleared page tail": dict(clear_tail=True),
}
# which checks may object to each (a planted error must be caught where it is, not by accident elsewhere)
_LATENT = {"cache latent", "out_ckv latent"}
_KPE = {"cache k_pe", "out_ckv k_pe"}
_ROT = _KPE | {"q_pe"}
EXPECT = {"epsilon 1e-5": _LATENT, "mean over 576 columns": _LATENT, "norm also on k_pe": _KPE, "norm weight also on k_pe": _KPE,
          "latent left unnormalised": _LATENT, "sine with the wrong sign": _ROT, "position off by one": _ROT,
          "position off by minus one": _ROT, "the other pairing": _ROT, "cos / sin of another request's row": _ROT,
          "token stored one slot later": {"cache latent", "cache k_pe", "cache changed outside the written cells"},
          "truncation instead of round-to-nearest": _LATENT | _ROT,
          "write into columns :512 of the q buffer": {"q_abs changed outside the written cells"},
          "cleared page tail": {"cache changed outside the written cells"}}


@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("name", list(PLANTED))
def test_bar_rejects_planted_error(name, interleaved):
    c = ms.case("decode_mtp1_16", 16, 16)
    sp = ms.spec("padded", out_ckv=True)
    stores, before, ret = _run_model(c, sp, interleaved, **PLANTED[name])
    failed = ms.check_outputs(c, sp, stores, before, ret, interleaved, label=name)
    print(f"{name}: rejected by {failed}")
    assert failed and set(failed) <= EXPECT[name], failed


def test_epsilon_shows_on_every_small_row():
    """a wrong epsilon moves rows of scale 1 by 5e-6 relative, far below half a bf16 ulp; every row of scale 1e-3 is far over"""
    c, sp = ms.case("decode_mtp1_16", 16, 16), ms.spec(cache=False, out_ckv=True, q=None)
    stores, _, _ = _run_model(c, sp, True, eps=1e-5)
    ref = ms.reference(c, True)
    from utils import rope_excess

    ex = rope_excess(ref.lat[:, None, :512], ms.views(c, sp, stores).out_ckv[:, None, :512])[:, 0]
    small = c.y[:, ms.KV_A_AT: ms.KV_A_AT + 512].float().pow(2).mean(-1) < 1e-5
    small &= ref.req >= 0
    assert int(small.sum()) >= 4 and bool((ex[small] > 1e3 * ROPE_SLACK).all())


# ------------------------------------------------------------------------------------------------------ surface, fakes
def test_surface():
    import hpc

    assert "mla_rope_norm_store_kv" in hpc.__all__ and callable(hpc.mla_rope_norm_store_kv)
    doc = hpc.mla_rope_norm_store_kv.__doc__
    for word in ("kv_norm_weight", "576", "interleaved", "neox", "out_q_pe", "out_ckv", "hipGraph", "max_pos - 1", "-1",
                 "{16, 32, 64, 128}", "1 <= H <= 128", "tests/mla_store_ref.py", "zeros"):
        assert word in doc, word


def test_both_libraries_export_the_launcher():
    import ctypes
    from pathlib import Path

    pkg = Path(__file__).resolve().parent.parent / "hpc-ops_amd" / "hpc"
    for name in ("libhpc_amd.so", "libhpc_amd_dev.so"):
        assert hasattr(ctypes.CDLL(str(pkg / name)), "hpc_mla_rope_norm_store_kv_async"), name


UNSUPPORTED, INVALID = -1, -2


def _launch(**kw):
    """hpc_mla_rope_norm_store_kv_async with pointers that are never dereferenced on the host; every case here is refused, or
    has nothing to launch, before any device call"""
    from ctypes import POINTER, c_float, c_int, c_int64, c_void_p, cast

    from hpc import _C

    a = dict(cache=4096, out_ckv=0, out_q_pe=1 << 20, kv_a=4096, q_pe=4096, cos_sin=4096, w=4096, ns=4096, qi=4096, bid=4096, rows=6,
             num_req=3, H=16, P=64, max_blocks=8, num_blocks=9, max_pos=4096, bs=64 * 576, ts=576, kv_rs=2112, ockv_rs=576,
             q_rs=16 * 192, q_hs=192, oq_rs=16 * 576, oq_hs=576, eps=1e-6, interleaved=1)
    a.update(kw)
    vp = lambda v: c_void_p(v) if v else None  # noqa: E731
    ip = lambda v: cast(c_void_p(v), POINTER(c_int)) if v else None  # noqa: E731
    return _C.lib.hpc_mla_rope_norm_store_kv_async(
        vp(a["cache"]), vp(a["out_ckv"]), vp(a["out_q_pe"]), vp(a["kv_a"]), vp(a["q_pe"]), vp(a["cos_sin"]), vp(a["w"]), ip(a["ns"]),
        ip(a["qi"]), ip(a["bid"]), a["rows"], a["num_req"], a["H"], a["P"], a["max_blocks"], a["num_blocks"], a["max_pos"],
        c_int64(a["bs"]), c_int64(a["ts"]), c_int64(a["kv_rs"]), c_int64(a["ockv_rs"]), c_int64(a["q_rs"]), c_int64(a["q_hs"]),
        c_int64(a["oq_rs"]), c_int64(a["oq_hs"]), c_float(a["eps"]), a["interleaved"], None)


@pytest.mark.parametrize("kwargs,code", [
    (dict(H=0), UNSUPPORTED), (dict(H=129), UNSUPPORTED), (dict(P=48), UNSUPPORTED), (dict(P=256), UNSUPPORTED),
    (dict(ts=575), UNSUPPORTED), (dict(ts=580), UNSUPPORTED), (dict(bs=64 * 576 + 4), UNSUPPORTED), (dict(cache=4096 + 8), UNSUPPORTED),
    (dict(kv_a=4096 + 2), UNSUPPORTED), (dict(kv_rs=2116), UNSUPPORTED), (dict(kv_rs=568), UNSUPPORTED), (dict(q_pe=4096 + 4), UNSUPPORTED),
    (dict(out_q_pe=(1 << 20) + 8), UNSUPPORTED), (dict(q_hs=196), UNSUPPORTED), (dict(oq_hs=56), UNSUPPORTED), (dict(oq_rs=580), UNSUPPORTED),
    (dict(oq_rs=15 * 576 + 56), UNSUPPORTED), (dict(oq_hs=64, oq_rs=512), UNSUPPORTED), (dict(out_q_pe=4096 + 128), UNSUPPORTED),
    (dict(out_q_pe=4096, oq_rs=16 * 192, oq_hs=200), UNSUPPORTED), (dict(out_q_pe=4096 + 2 * (5 * 16 * 192 + 15 * 192 + 64) - 16), UNSUPPORTED),
    (dict(out_ckv=4096 + 4), UNSUPPORTED), (dict(out_ckv=4096, ockv_rs=568), UNSUPPORTED), (dict(cos_sin=4096 + 4), UNSUPPORTED),
    (dict(w=4096 + 8), UNSUPPORTED),
    (dict(cache=0), INVALID), (dict(q_pe=0), INVALID), (dict(out_q_pe=0), INVALID), (dict(kv_a=0), INVALID), (dict(cos_sin=0), INVALID),
    (dict(w=0), INVALID), (dict(ns=0), INVALID), (dict(qi=0), INVALID), (dict(bid=0), INVALID), (dict(rows=-1), INVALID),
    (dict(num_req=-1), INVALID), (dict(H=-1), INVALID), (dict(max_blocks=-1), INVALID), (dict(num_blocks=-1), INVALID),
    (dict(max_pos=0), INVALID), (dict(bs=-64 * 576), INVALID),
    (dict(rows=0), 0), (dict(num_req=0), 0), (dict(cache=0, out_ckv=4096, bid=0, rows=0), 0), (dict(q_pe=0, out_q_pe=0, H=0, rows=0), 0),
    # the cache's rule (csrc/mla_cache.h), as the readers' tables pin it: it holds for a call without rows too, a negative
    # block stride is an invalid argument that wins over whatever is merely unsupported, and an absent cache has no page size
    (dict(ts=-576), UNSUPPORTED), (dict(P=8), UNSUPPORTED), (dict(P=0), UNSUPPORTED), (dict(rows=0, P=48), UNSUPPORTED),
    (dict(P=48, bs=-64 * 576), INVALID), (dict(rows=0, cache=0, out_ckv=4096, P=48), 0),
])
def test_cabi_refuses_on_the_host(kwargs, code):
    assert _launch(**kwargs) == code


def test_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        def T(*shape, dtype=torch.bfloat16):
            return torch.empty(shape, dtype=dtype, device="cuda")

        rows, H = 6, 20
        ckv, kv_a = T(9, 64, 576), T(rows, 2112)[:, 1536:]
        cs, w = T(4096, 64, dtype=torch.float32), T(512, dtype=torch.float32)
        ns, qi, bid = T(3, dtype=torch.int32), T(4, dtype=torch.int32), T(3, 64, dtype=torch.int32)
        q_pe, q_abs, ockv = T(rows, H, 192)[..., 128:], T(rows, H, 576), T(rows, 576)
        for cache in (ckv, None):
            for out_ckv in (ockv, None):
                if cache is None and out_ckv is None:
                    continue
                raw = torch.ops.hpc_mla.rope_norm_store_kv(cache, kv_a, cs, w, ns, qi, bid, None, None, out_ckv, 1e-6, True)
                assert raw.shape == (0,) and raw.dtype == torch.bfloat16  # the entry's placeholder without q_pe
                assert hpc.mla_rope_norm_store_kv(cache, kv_a, cs, w, ns, qi, bid, out_ckv=out_ckv) is None
                y = hpc.mla_rope_norm_store_kv(cache, kv_a, cs, w, ns, qi, bid, q_pe=q_pe, out_ckv=out_ckv, interleaved=False)
                assert (y.shape, y.dtype, y.device.type) == ((rows, H, 64), torch.bfloat16, "cuda") and y.is_contiguous()
                out = q_abs[..., 512:]
                assert hpc.mla_rope_norm_store_kv(cache, kv_a, cs, w, ns, qi, bid, q_pe=q_pe, out_q_pe=out, out_ckv=out_ckv) is out
                assert hpc.mla_rope_norm_store_kv(cache, kv_a, cs, w, ns, qi, bid, q_pe=q_pe, out_q_pe=q_pe, out_ckv=out_ckv) is q_pe
