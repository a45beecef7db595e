"""hpc.token_logprobs - the log-probability, rank and top-N of the token each logits row emitted - against its PyTorch
statement (tests/token_logprobs_ref.py).  Ranks, top ids and dead rows by equality; logprobs against float64 under

    |got - lp64| <= C_BAR * 2^-24 * (1 + |lp64|),   an exact -inf coming back as -inf.

C_BAR by the project's rule (tests/test_group_gemm_mxfp4.py, tests/test_mla_indexer.py): MEASURED_C is the worst error in
those units on one MI355X over the real cases of test_grid_against_reference (every case prints its own), C_BAR twice it
rounded up to a power of two.  A rounding model of the kernels allows about 64 units in the worst case (32 serial adds per
thread, the cross-lane and cross-segment folds, the exponentials, the logarithm, the last subtractions), so C_BAR <= 64 is
the condition; the kernels subtract the row's maximum before the logarithm of the sum, which keeps the usual case far
below that."""
import ctypes
import functools
import math
from pathlib import Path

import pytest
import torch

import token_logprobs_ref as lref

ROOT = Path(__file__).resolve().parent.parent
F32, BF16 = torch.float32, torch.bfloat16

MEASURED_C = 3.853  # V = 131080, 64 rows, bfloat16, a temperature per row; the 60 cases' own worsts are 0.90 - 3.85
C_BAR = 8.0
assert C_BAR == 2.0 ** math.ceil(math.log2(2 * MEASURED_C)) and C_BAR <= 64


# ---- CPU: the statement, at V = 8 where every result can be written down -------------------------------------------------
def test_statement_on_a_hand_written_case():
    probs = torch.tensor([.5, .25, .125, .0625, .03125, .015625, .0078125, .0078125])
    logits = probs.log().repeat(6, 1)
    tok = torch.tensor([0, 3, 7, 6, -1, 8])
    lp, rank, ids, tlp = lref.ref_token_logprobs(logits, tok, 1.0, 3)
    assert rank.tolist() == [1, 4, 8, 7, 0, 0] and rank.dtype == torch.int32 and ids.dtype == torch.int32
    assert torch.allclose(lp[:4], torch.tensor([.5, .0625, .0078125, .0078125], dtype=torch.float64).log(), atol=1e-6)
    assert lp[4:].tolist() == [0.0, 0.0]
    assert ids.tolist() == [[0, 1, 2]] * 4 + [[-1, -1, -1]] * 2
    assert torch.allclose(tlp[:4], torch.tensor([.5, .25, .125], dtype=torch.float64).log().expand(4, 3), atol=1e-6)
    assert tlp[4:].abs().sum() == 0
    # T = 0.5 squares the probabilities: p_i^2 / sum p^2; T per row, and T == 0 is the raw distribution
    sq = probs.double() ** 2 / (probs.double() ** 2).sum()
    lp2, rank2, ids2, _ = lref.ref_token_logprobs(logits, tok, torch.tensor([0.5, 0.5, 0.5, 0.0, 1.0, 1.0]), 8)
    assert torch.allclose(lp2[:3], sq[[0, 3, 7]].log(), atol=1e-6) and abs(float(lp2[3]) - math.log(.0078125)) < 1e-6
    assert torch.equal(rank2, rank) and ids2[0].tolist() == list(range(8))
    # a tensor of 3 entries over 6 rows: rows 0-1, 2-3, 4-5
    assert lref.row_temperature(torch.tensor([1., 2., 3.]), 6).tolist() == [1., 1., 2., 2., 3., 3.]
    # -0.0 == +0.0 and ties go to the smaller id; -inf ranks last and has logprob -inf
    x = torch.tensor([[0.0, -0.0, 1.0, -0.0, 0.0, -math.inf, -1.0, -math.inf]]).repeat(4, 1)
    lp3, rank3, ids3, tlp3 = lref.ref_token_logprobs(x, torch.tensor([1, 4, 5, 7]), 1.0, 8)
    assert rank3.tolist() == [3, 5, 7, 8] and ids3[0].tolist() == [2, 0, 1, 3, 4, 6, 5, 7]
    assert lp3[2:].tolist() == [-math.inf, -math.inf] and float(lp3[0]) == float(lp3[1])
    assert abs(float(lp3[0]) + math.log(math.e + 4 + 1 / math.e)) < 1e-12 and tlp3[0, 6:].tolist() == [-math.inf] * 2
    assert lref.units(torch.tensor([-math.inf, 0.0]), torch.tensor([-math.inf, 0.0], dtype=torch.float64)) == 0.0
    assert lref.units(torch.tensor([-1e30]), torch.tensor([-math.inf], dtype=torch.float64)) == math.inf
    assert lref.units(torch.tensor([1 + 2.0 ** -22]), torch.tensor([1.0], dtype=torch.float64)) == 2.0


# ---- CPU: the C entry refuses before any device call ------------------------------------------------------------------------
def _entry():
    from ctypes import c_float, c_int, c_int64, c_void_p

    lib = ctypes.CDLL(str(ROOT / "hpc-ops_amd" / "hpc" / "libhpc_amd.so"))
    fn = lib.hpc_token_logprobs_async
    fn.restype = c_int
    fn.argtypes = [c_void_p] * 6 + [c_int, c_int64, c_void_p, c_int, c_void_p, c_int, c_float] + [c_int] * 3 + [c_void_p]
    ws = lib.hpc_token_logprobs_workspace_bytes
    ws.restype = c_int64
    ws.argtypes = [c_int] * 3
    return fn, ws


# The pointers are never dereferenced on the host and rows is 0 wherever the call is accepted: every check runs before the
# `rows == 0` return, so no case here can reach a launch.
_P = 4096
_OK = dict(lp=_P, rank=_P, ids=_P, tlp=_P, ws=_P, lg=_P, dt=0, ld=1024, tok=_P, tb=4, t=None, tc=0, tv=1.0, rows=0, k=5, v=1024)
_INVALID = [dict(lp=None), dict(rank=None), dict(ws=None), dict(lg=None), dict(tok=None), dict(ids=None), dict(tlp=None),
            dict(rows=-1), dict(k=-1), dict(v=0), dict(v=-8), dict(dt=2), dict(dt=-1), dict(ld=1016), dict(tb=2), dict(tb=0),
            dict(t=_P, tc=0), dict(t=_P, tc=-1), dict(t=_P, tc=4, rows=6), dict(tv=-1.0)]
_UNSUPPORTED = [dict(v=1028, ld=1028), dict(v=1 << 20, ld=1 << 20), dict(k=33), dict(k=16, v=8, ld=8)]


def _call(fn, **kw):
    a = dict(_OK, **kw)
    return fn(a["lp"], a["rank"], a["ids"], a["tlp"], a["ws"], a["lg"], a["dt"], a["ld"], a["tok"], a["tb"], a["t"], a["tc"],
              a["tv"], a["rows"], a["k"], a["v"], None)


def test_c_entry_refusals():
    fn, ws = _entry()
    assert _call(fn) == 0 and _call(fn, dt=1, tb=8) == 0 and _call(fn, t=_P, tc=3) == 0 and _call(fn, tv=0.0) == 0
    assert _call(fn, k=0, ids=None, tlp=None) == 0 and _call(fn, k=32) == 0 and _call(fn, ld=1152) == 0
    assert _call(fn, k=8, v=8, ld=8) == 0
    for kw in _INVALID:
        assert _call(fn, **kw) == -2, kw
    for kw in _UNSUPPORTED:
        assert _call(fn, **kw) == -1, kw


def test_workspace_formula():
    """16 bytes of statistics and num_top composites of 8 bytes per (row, segment); 16 segments up to V = 131072, then
    ceil(V / 8192)."""
    _, ws = _entry()
    assert ws(2, 5, 1024) == 2 * 16 * (16 + 5 * 8) and ws(1, 0, 131080) == 17 * 16 and ws(3, 32, 131080) == 3 * 17 * (16 + 256)
    assert ws(0, 5, 1024) == 0 and ws(-1, 5, 1024) == 0 and ws(2, -1, 1024) == 0 and ws(2, 5, 0) == 0
    assert ws(65537, 32, 8) == 65537 * 16 * (16 + 256) and ws(1 << 20, 32, (1 << 20) - 8) == (1 << 20) * 128 * (16 + 256)
    assert lref.segments_of(131072) == 16 and lref.segments_of(131080) == 17 and lref.segment_size(8200) == 513


def test_fake():
    from torch._subclasses import FakeTensorMode

    import hpc  # noqa: F401

    with FakeTensorMode():
        lg = torch.empty(20, 1024, dtype=BF16, device="cuda")
        tok = torch.empty(5, 4, dtype=torch.int32, device="cuda")
        outs = torch.ops.hpc_logprobs.token_logprobs(lg, tok, None, 0.7, 5, None, None, None, None)
        want = [((20,), torch.float32), ((20,), torch.int32), ((20, 5), torch.int32), ((20, 5), torch.float32)]
        assert [(tuple(o.shape), o.dtype) for o in outs] == want and all(o.device == lg.device for o in outs)
        z = hpc.token_logprobs(lg, tok.view(20).long(), temperature=torch.empty(5, device="cuda"))
        assert [tuple(o.shape) for o in z] == [(20,), (20,), (20, 0), (20, 0)]
        given = [torch.empty(s, dtype=d, device="cuda") for s, d in want]
        back = hpc.token_logprobs(lg, tok, 0.7, 5, *given)
        assert all(b is g for b, g in zip(back, given))
        back = hpc.token_logprobs(lg, tok, num_top=5, token_ranks=given[1], top_logprobs=given[3])
        assert back[1] is given[1] and back[3] is given[3] and back[0] is not given[0] and back[0].shape == (20,)


# ---- CPU: planted errors in a model of the two phases -------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _model_inputs():
    """The committed inputs of the planted-error test: V = 1000 (ragged segments of 63), randn rows at T = 0.7 whose tokens
    are the (likely) last element, an element of segment 1 and likely tokens; bf16 rows of four values (ties), their tokens inside a
    tie class; a row of -0.0 and +0.0 in turn with a token at a +0.0 behind a -0.0."""
    V = 1000
    c = lref.make_case(V, 4, 5, F32, temperature=0.7)
    logits, tok = c["logits"], c["tok"].clone()
    tok[1], tok[3] = V - 1, 70
    logits[:, V - 1] = 2.0  # a last element that weighs more than the bar
    g = torch.Generator().manual_seed(6)
    ties = torch.randint(0, 4, (2, V), generator=g).float()
    tied = [torch.nonzero(ties[i] == 3).flatten() for i in range(2)]
    zeros = torch.randn(1, V, generator=g) - 3.0
    zeros[0, 100:200:2], zeros[0, 101:200:2] = -0.0, 0.0
    logits = torch.cat([logits, ties, zeros])
    tok = torch.cat([tok, torch.stack([tied[0][len(tied[0]) // 2], tied[1][-1]]), torch.tensor([151])])
    return logits, tok, 0.7, lref.ref_token_logprobs(logits, tok, 0.7, 32)


def test_model_meets_the_statement():
    logits, tok, T, ref = _model_inputs()
    for k in (0, 5, 32):
        lref.check(lref.two_phase_model(logits, tok, T, k), ref, tok, k, C_BAR)


@pytest.mark.parametrize("plant", lref.PLANTS)
def test_planted_errors_are_caught(plant):
    logits, tok, T, ref = _model_inputs()
    with pytest.raises(AssertionError):
        lref.check(lref.two_phase_model(logits, tok, T, 5, plant=plant), ref, tok, 5, C_BAR)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
def _padded(x, pad):
    """The same rows with a row stride of V + pad; the padding holds NaN."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=x.dtype, device=x.device)
    buf[:, : x.shape[1]] = x
    return buf[:, : x.shape[1]]


def _cpu(outs):
    return tuple(o.cpu() for o in outs)


def _run_and_check(logits, tok, T, num_top, ref=None, dev_logits=None, dev_tok=None):
    """One call on CPU inputs (or their given device forms), held to the statement; returns (worst units, outputs)."""
    import hpc

    ref = lref.ref_token_logprobs(logits, tok, T, num_top) if ref is None else ref
    t = T.cuda() if isinstance(T, torch.Tensor) else T
    got = _cpu(hpc.token_logprobs(logits.cuda() if dev_logits is None else dev_logits, tok.cuda() if dev_tok is None else dev_tok,
                                  temperature=t, num_top=num_top))
    return lref.check(got, ref, tok, num_top, C_BAR), got


# ---- GPU 1: the grid - the real cases of MEASURED_C -----------------------------------------------------------------------------
# V = 8 leaves 8 of the 16 segments empty, 1000 gives ragged segments of 63, 131080 is the first size with 17 segments
@pytest.mark.gpu
@pytest.mark.parametrize("tensor_t", [False, True], ids=["scalarT", "tensorT"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R", [1, 5, 64])
@pytest.mark.parametrize("V", [8, 1000, 1024, 8200, 131080])
def test_grid_against_reference(V, R, dtype, tensor_t):
    worst = 0.0
    for scale in (1.0, 4.0):  # randn, and a peaked row as a model's are
        c = lref.make_case(V, R, 1000 + V + 7 * R + int(scale), dtype, scale=scale, tensor_count=R if tensor_t else None)
        ref = lref.ref_token_logprobs(c["logits"], c["tok"], c["T"], min(32, V))
        lg, tok = c["logits"].cuda(), c["tok"].cuda()
        for pad in (0, 128):
            lgp = _padded(lg, pad) if pad else lg
            for num_top in sorted({min(k, V) for k in (0, 1, 5, 20, 32)}):
                w, _ = _run_and_check(c["logits"], c["tok"], c["T"], num_top, ref=ref, dev_logits=lgp, dev_tok=tok)
                worst = max(worst, w)
    print(f"V={V} R={R} {dtype} tensorT={tensor_t}: worst logprob error {worst:.3f} units of 2^-24 (1 + |lp|)")


# ---- GPU 2: needles - no element is skipped ----------------------------------------------------------------------------------------
def _needle_places(V):
    seg = lref.segment_size(V)  # 513 at V = 8200: segment s is [513 s, 513 (s + 1)), thread t holds i0 + 256 e + t
    places = {0, V - 1}
    for s in range(1, 16):
        places |= {s * seg - 1, s * seg}
    for i0 in (0, 7 * seg, 15 * seg):
        places |= {i0 + 5, i0 + 256 + 5, i0 + 255, i0 + 256 + 255, i0 + 512}
    return sorted(p for p in places if p < V)


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [-math.inf, -1e4], ids=["neginf", "minus1e4"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_needles(dtype, fill):
    """Row i is `fill` everywhere but the token and a needle at place i: of equal value in the first half of the rows (the
    logprob is -log 2, and would be 0 were the needle lost), one above it in the second half (rank 2, top_ids[0] the
    needle, logprob -log(1 + e))."""
    V = 8200
    places = _needle_places(V)
    assert lref.segment_size(V) == 513 and len(places) >= 40
    n = len(places)
    tok = torch.tensor([4100 if p != 4100 else 4101 for p in places] * 2)
    logits = torch.full((2 * n, V), fill)
    rows = torch.arange(2 * n)
    logits[rows, tok] = 1.0
    logits[rows, torch.tensor(places * 2)] = torch.cat([torch.full((n,), 1.0), torch.full((n,), 2.0)])
    logits = logits.to(dtype)
    _, (lp, rank, ids, tlp) = _run_and_check(logits, tok, 1.0, 2)
    assert lref.units(lp[:n], torch.full((n,), -math.log(2.0), dtype=torch.float64)) <= C_BAR
    assert lref.units(lp[:n], torch.zeros(n, dtype=torch.float64)) > 1e6  # the needle lost
    assert rank[:n].tolist() == [2 if p < t else 1 for p, t in zip(places, tok[:n].tolist())]
    assert rank[n:].tolist() == [2] * n and ids[n:, 0].tolist() == places and ids[n:, 1].tolist() == tok[n:].tolist()
    assert lref.units(lp[n:], torch.full((n,), -math.log(1 + math.e), dtype=torch.float64)) <= C_BAR


# ---- GPU 3: ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V", [1000, 8200])
def test_ties(V):
    """bf16 rows of four distinct values, about V / 4 tokens per value (as test_spec_verify.py::test_greedy builds them):
    the token at the first, a middle and the last member of a tie class; and rows holding both -0.0 and +0.0."""
    g = torch.Generator().manual_seed(3)
    R = 12
    logits = torch.randint(0, 4, (R, V), generator=g).to(BF16)
    tok = torch.empty(R, dtype=torch.int64)
    for r in range(R):
        tied = torch.nonzero(logits[r] == r % 4).flatten()
        assert tied.numel() > 8
        tok[r] = tied[(0, tied.numel() // 2, tied.numel() - 1)[r // 4]]
    for num_top in (5, 32):
        _run_and_check(logits, tok, 0.9, num_top)
    z = (torch.randn(6, V, generator=g) - 2.5)
    z[:, 10:V:7], z[:, 13:V:7] = -0.0, 0.0
    z[3:, 0] = 0.5  # one element above the zeros, and rows where a zero is the maximum
    ztok = torch.tensor([10, 13, 10 + 7 * 40, 13 + 7 * 40, 10 + 7 * ((V - 11) // 7), 13 + 7 * ((V - 14) // 7)])
    assert (z[torch.arange(6), ztok] == 0).all() and int(torch.signbit(z[torch.arange(6), ztok]).sum()) == 3
    for dtype in (F32, BF16):
        for num_top in (5, 32):
            _run_and_check(z.to(dtype), ztok, 1.3, num_top)


# ---- GPU 4: where the token sits --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_token_placement(dtype):
    V = 8200
    seg = lref.segment_size(V)
    places = [0, V - 1, seg - 1, seg, 15 * seg, 15 * seg - 1, 4 * seg + 100]
    c = lref.make_case(V, len(places) + 4, 77, dtype, scale=2.0, tensor_count=len(places) + 4)
    logits, tok = c["logits"].clone(), torch.tensor(places + [17, 4000, 5000, 6000])
    n = len(places)
    logits[n, 17] = 30.0       # the row's maximum: rank 1
    logits[n + 1, 4000] = -30.0  # its minimum: rank V
    logits[n + 2, 5000] = -math.inf  # a masked token: logprob -inf, the last rank
    logits[n + 3, 6000:6100] = -math.inf  # one of several: the rank counts the -inf entries in front of it
    logits[n + 3, 10:20] = -math.inf
    for num_top in (0, 5):
        _, (lp, rank, _, _) = _run_and_check(logits, tok, c["T"], num_top)
        assert rank[n:].tolist() == [1, V, V, V - 99] and lp[n + 2:].tolist() == [-math.inf] * 2


# ---- GPU 5: dead rows, straight from hpc.speculative_verify ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_speculative_chain_and_dead_rows(dtype):
    import hpc
    import spec_verify_ref as sref

    V, B, K = 8200, 8, 4
    c = sref.make_case(V, B, K, 41, dtype)
    lg, T = c["logits"].cuda(), c["T"].cuda()
    out, acc = hpc.speculative_verify(lg, c["draft"].cuda(), temperature=T, uniform_samples=c["u"].cuda(),
                                      gumbel_noise=c["gumbel"].cuda())
    assert out.shape == (B, K + 1) and out.dtype == torch.int32 and T.shape == (B,)
    tok = out.cpu()
    dead = (tok.flatten() == -1)
    assert 0 < int(dead.sum()) < B * K  # some rows are dead, some requests go on
    ref = lref.ref_token_logprobs(c["logits"], tok, c["T"], 5)
    got = _cpu(hpc.token_logprobs(lg, out, temperature=T, num_top=5))
    lref.check(got, ref, tok, 5, C_BAR)
    lp, rank, ids, tlp = got
    assert (lp[dead] == 0).all() and (rank[dead] == 0).all() and (ids[dead] == -1).all() and (tlp[dead] == 0).all()
    assert (rank[~dead] >= 1).all()
    poisoned = lg.clone()
    poisoned[dead.cuda()] = float("nan")  # dead rows are not read
    again = _cpu(hpc.token_logprobs(poisoned, out, temperature=T, num_top=5))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again, got))


# ---- GPU 6: the forms of the temperature --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_temperature_forms():
    import hpc

    V, B, K = 1000, 3, 3
    R = B * (K + 1)
    c = lref.make_case(V, R, 9, BF16, scale=3.0, tensor_count=R)
    _run_and_check(c["logits"], c["tok"], c["T"], 5)  # C == R
    per_request = torch.tensor([0.4, 1.7, 0.9])
    _, got = _run_and_check(c["logits"], c["tok"], per_request, 5)  # C == B: rows 0-3, 4-7, 8-11
    for b in range(B):  # a request's rows equal the same rows under that scalar, bit for bit
        rows = slice(b * (K + 1), (b + 1) * (K + 1))
        _, one = _run_and_check(c["logits"][rows], c["tok"][rows], float(per_request[b]), 5)
        assert all(torch.equal(a[rows].view(torch.int32), o.view(torch.int32)) for a, o in zip(got, one))
    # T == 0 (a greedy request) is the raw distribution: the same bits as T == 1
    zeros = torch.tensor([0.0, 0.6, 0.0, 1.0, 0.0, 0.0, 1.5, 0.0, 1.0, 0.0, 0.3, 0.0])
    ones = torch.where(zeros == 0, torch.ones_like(zeros), zeros)
    _, g0 = _run_and_check(c["logits"], c["tok"], zeros, 5)
    _, g1 = _run_and_check(c["logits"], c["tok"], ones, 5)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(g0, g1))
    lg, tok = c["logits"].cuda(), c["tok"].cuda()
    s0, s1 = _cpu(hpc.token_logprobs(lg, tok, 0.0, 5)), _cpu(hpc.token_logprobs(lg, tok, 1.0, 5))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(s0, s1))
    lref.check(s0, lref.ref_token_logprobs(c["logits"], c["tok"], 0.0, 5), c["tok"], 5, C_BAR)


# ---- GPU 7: the forms of the ids ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_id_forms(dtype):
    import hpc

    V, B = 8200, 6
    c = lref.make_case(V, B, 21, dtype, scale=2.0, tensor_count=B)
    lg, T = c["logits"].cuda(), c["T"].cuda()
    sampled = hpc.fused_sampler(lg, temperature=T, seed=42)
    assert sampled.shape == (B, 1) and sampled.dtype == torch.int32
    a = _cpu(hpc.token_logprobs(lg, sampled, temperature=T, num_top=20))
    tok = sampled.cpu().flatten().long()
    lref.check(a, lref.ref_token_logprobs(c["logits"], tok, c["T"], 20), tok, 20, C_BAR)
    b = _cpu(hpc.token_logprobs(lg, tok.cuda(), temperature=T, num_top=20))
    assert tok.dtype == torch.int64 and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---- GPU 8: the token's slot of the top list --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_top_list_holds_the_token(dtype):
    """Row r's token is the one of rank r + 1, r = 0 .. 39: inside the list for num_top 32 up to row 31, for 5 up to row 4.
    lref.check asserts top_ids[r, rank - 1] == token and the bits of the two logprobs; here the ranks that reach it."""
    V, R = 8200, 40
    c = lref.make_case(V, R, 33, dtype, scale=4.0, tensor_count=R)
    order = torch.sort(c["logits"].float(), dim=-1, descending=True, stable=True).indices
    tok = order[torch.arange(R), torch.arange(R)]
    for num_top in (1, 5, 32):
        _, (lp, rank, ids, tlp) = _run_and_check(c["logits"], tok, c["T"], num_top)
        assert rank.tolist() == list(range(1, R + 1))
        k = torch.arange(num_top)
        assert torch.equal(ids[k, k].long(), tok[:num_top]) and torch.equal(tlp[k, k].view(torch.int32), lp[:num_top].view(torch.int32))


# ---- GPU 9: outputs passed in, hipGraph replay -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_outputs_passed_in_and_graph_replay():
    import hpc

    V, R, K = 8200, 10, 5
    cs = [lref.make_case(V, R, 50 + s, BF16, scale=2.0, tensor_count=R) for s in range(3)]
    for c in cs:
        c["tok"][3] = -1  # a dead row goes over the poison too
    dev = [{k: c[k].cuda() for k in ("logits", "tok", "T")} for c in cs]
    outs = [torch.full((R,), 7.0, device="cuda"), torch.full((R,), 7, dtype=torch.int32, device="cuda"),
            torch.full((R, K), 7, dtype=torch.int32, device="cuda"), torch.full((R, K), 7.0, device="cuda")]
    d = dev[0]
    lg0, tok0 = d["logits"].clone(), d["tok"].clone()
    back = hpc.token_logprobs(d["logits"], d["tok"], d["T"], K, *outs)
    assert all(b is o for b, o in zip(back, outs))
    lref.check(_cpu(outs), lref.ref_token_logprobs(cs[0]["logits"], cs[0]["tok"], cs[0]["T"], K), cs[0]["tok"], K, C_BAR)
    assert torch.equal(d["logits"].view(torch.int16), lg0.view(torch.int16)) and torch.equal(d["tok"], tok0)

    buf = {k: v.clone() for k, v in d.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        hpc.token_logprobs(buf["logits"], buf["tok"], buf["T"], K, *outs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hpc.token_logprobs(buf["logits"], buf["tok"], buf["T"], K, *outs)
    for i in (1, 2):
        for k in buf:
            buf[k].copy_(dev[i][k])
        for o in outs:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        eager = hpc.token_logprobs(dev[i]["logits"], dev[i]["tok"], dev[i]["T"], K)
        assert all(torch.equal(o.view(torch.int32), e.view(torch.int32)) for o, e in zip(outs, eager))
        lref.check(_cpu(outs), lref.ref_token_logprobs(cs[i]["logits"], cs[i]["tok"], cs[i]["T"], K), cs[i]["tok"], K, C_BAR)


# ---- GPU 10: more rows than a grid's y extent -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("num_top", [0, 3])
def test_chunked_launches(num_top):
    V, R = 8, 65537
    c = lref.make_case(V, R, 8, F32, scale=2.0, tensor_count=R)
    c["tok"][65535] = -1
    _, (lp, rank, ids, tlp) = _run_and_check(c["logits"], c["tok"], c["T"], num_top)
    ref = lref.ref_token_logprobs(c["logits"][65534:], c["tok"][65534:], c["T"][65534:], num_top)
    lref.check((lp[65534:], rank[65534:], ids[65534:], tlp[65534:]), ref, c["tok"][65534:], num_top, C_BAR)
    assert rank[65534:].tolist()[1] == 0 and int(rank[65534]) >= 1 and int(rank[65536]) >= 1


# ---- GPU 11: refusals of the torch op, the empty call ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_error_paths():
    import hpc

    V, R = 1024, 6
    lg = torch.randn(R, V, device="cuda")
    tok = torch.randint(0, V, (R,), device="cuda")
    hpc.token_logprobs(lg, tok)
    with pytest.raises(RuntimeError, match="num_top must be in"):
        hpc.token_logprobs(lg, tok, num_top=33)
    with pytest.raises(RuntimeError, match="num_top must be <= vocab_size"):
        hpc.token_logprobs(lg[:, :8], tok % 8, num_top=9)
    with pytest.raises(RuntimeError, match="token_ids must have one element per logits row"):
        hpc.token_logprobs(lg, tok[:-1])
    with pytest.raises(RuntimeError, match="token_ids dtype must be int32 or int64"):
        hpc.token_logprobs(lg, tok.float())
    with pytest.raises(RuntimeError, match="token_ids tensor must be contiguous"):
        hpc.token_logprobs(lg, tok.repeat(2)[::2])
    with pytest.raises(RuntimeError, match="temperature must have a number of elements that divides"):
        hpc.token_logprobs(lg, tok, temperature=torch.ones(4, device="cuda"))
    with pytest.raises(RuntimeError, match="temperature dtype must be float32"):
        hpc.token_logprobs(lg, tok, temperature=torch.ones(R, device="cuda", dtype=torch.float64))
    with pytest.raises(RuntimeError, match="scalar temperature must be >= 0"):
        hpc.token_logprobs(lg, tok, temperature=-1.0)
    with pytest.raises(RuntimeError, match="unsupported vocab_size"):
        hpc.token_logprobs(torch.randn(R, V + 4, device="cuda"), tok)
    with pytest.raises(RuntimeError, match="top_ids must be a contiguous tensor of shape"):
        hpc.token_logprobs(lg, tok, num_top=5, top_ids=torch.empty(R, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="token_ranks dtype must be int32"):
        hpc.token_logprobs(lg, tok, token_ranks=torch.empty(R, dtype=torch.int64, device="cuda"))
    outs = hpc.token_logprobs(lg[:0], tok[:0], num_top=5)  # R == 0: empty tensors, no launch
    assert [tuple(o.shape) for o in outs] == [(0,), (0,), (0, 5), (0, 5)] and outs[1].dtype == torch.int32
